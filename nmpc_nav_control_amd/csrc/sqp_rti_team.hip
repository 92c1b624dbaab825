// sqp_rti_team.hip -- batched SQP-RTI step, one 16-lane team (one DPP row) per robot instance.
//
// Same algorithm as oracle/nmpc_oracle.c (RK4 + forward sensitivities, Gauss-Newton cost, box bounds,
// Mehrotra IPM with damped corrector and centring safeguard, Riccati recursion),
// mapped MI355X-first:
//   * four robots per wavefront; inside a team lane v owns QP variable v of every stage (v < NU: input,
//     NU <= v < NU+NX: state); cross-lane operands are DPP row_newbcast broadcasts, fused into the
//     multiply-accumulates (v_fmac_f32_dpp / v_fmac_f64_dpp);
//   * the stage factor is a classic Riccati step in fp64: lane NU+i carries row i of the cost-to-go Hessian
//     P_{k+1}; PG = P_{k+1}[B A] and the rows of M = D + [B A]' PG are fused fp64 DPP blocks
//     (team_asm_gen.hpp), then a right-looking Cholesky of the NU x NU input block leaves the Schur complement
//     P_k in the state block (near the solution the barrier weights of active bounds reach 1e12, and fp32
//     Schur complements cancel catastrophically). The input columns of the factor are stored in fp32 and every
//     solve with them runs in fp32 (u0 error ~1e-4 against the fp64 oracle, DESIGN.md "Algorithm and precision");
//   * rows of [B A] that do not depend on the state (model trait NGV) live in registers for the whole launch;
//     only the NGV varying rows are stored per stage;
//   * each lane's per-stage record (slacks, multipliers, iterate, directions, factor row, Jacobian column) is
//     RS contiguous floats at [team][stage][slot][RS]: one record = RS/4 dwordx4 loads, and every sweep
//     prefetches the next stage's record while the current stage computes (the ~170 MB working set of 4096
//     robots stays in the 256 MB Infinity Cache);
//   * the linearisation is column-parallel: lane v integrates the nominal RK4 step and propagates column v of
//     its sensitivity, and the initial (dynamics-feasible) iterate is simulated in the same forward pass.
// The IPM iteration count is per team; a wave iterates until its four teams have converged (finished teams
// skip their loads and stores).
#include "nmpc_kernels.hpp"
#include "team_common.hpp"
#include "sqp_steps.hpp"
#include "path_march.hpp"
#include "team_tick_defs.hpp"  // the sweeps' buffer counts, g_zero4, g_rec_sentinel, kModeRunPath, HoList

namespace nmpc {

#ifdef NMPC_STAMPS
// diagnostic build only: s_memtime at phase boundaries for the first team of the first 256 waves
constexpr int kStampIts = 64;
__device__ unsigned long long g_stamps[256][2 + 4 * kStampIts];
#define STAMP(slot)                                                                                              \
    do {                                                                                                         \
        if (r == 0 && (team & 3) == 0 && (team >> 2) < 256) g_stamps[team >> 2][(slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// fine-grained stamps inside one P1 stage body (iteration 2, stage 20)
__device__ unsigned long long g_stamps_p1[256][8];
// end of the split launches' stage-parallel P0 part (row 0 of the first robot of each group of 4)
__device__ unsigned long long g_stamps_pa[256];
#define STAMPPA()                                                                                                \
    do {                                                                                                         \
        if (r == 0 && (team & 3) == 0 && (team >> 2) < 256) g_stamps_pa[team >> 2] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// end of the corrector backward sweep (C1) of iteration it, first team of the first 256 waves
__device__ unsigned long long g_stamps_c1[256][kStampIts];
#define STAMPC1()                                                                                                \
    do {                                                                                                         \
        if (it < kStampIts && r == 0 && (team & 3) == 0 && (team >> 2) < 256)                                   \
            g_stamps_c1[team >> 2][it] = __builtin_amdgcn_s_memtime();                                           \
    } while (0)
#define STAMPF(slot)                                                                                             \
    do {                                                                                                         \
        if (it == 2 && k == 20 && r == 0 && (team & 3) == 0 && (team >> 2) < 256)                                 \
            g_stamps_p1[team >> 2][(slot)] = __builtin_amdgcn_s_memtime();                                        \
    } while (0)
#else
#define STAMP(slot) ((void)0)
#define STAMPF(slot) ((void)0)
#define STAMPC1() ((void)0)
#define STAMPPA() ((void)0)
#endif

template <class M>
size_t team_scratch_floats(int N, int stride)
{
    // the lane records [robot][stage][slot][RSS], the DZ plane [robot][stage][16], then the row-parallel kernel's
    // dummy stage blocks [256 robots][4 waves][16][RSS] and dummy DZ rows [256][4][16] (sqp_rti_rowpar.hip)
    return (size_t)stride * (N + 1) * 16 * (TeamRec<M>::RSS + 1) + (size_t)256 * 4 * 16 * (TeamRec<M>::RSS + 1) + 64;
}

namespace {
#ifdef NMPC_STAMPS
constexpr int kStampItsC = kStampIts;
#else
constexpr int kStampItsC = 0;
#endif

// MS: store the slack / multiplier quad only where a bound lives (launches with more waves than SIMDs, where the
// record traffic shows: tric N=60 B=8192 4.47 -> 4.39 ms; with one wave per SIMD the exec-mask switches cost
// more than the bytes save: diff N=40 B=4096 1.555 -> 1.566 ms)
// SD: one direction per IPM iteration (P1 builds the rhs with the centring target sigma mu, one forward sweep
// computes the direction, the step and the complementarity polynomial that predicts the next mu) instead of
// Mehrotra's predictor-corrector (P1 + F0 + C1 + F1 sweeps)
// MODE is a template parameter: kModeSolve, kModeRun, or kModeRunPath (run mode with the in-kernel path march,
// a.segs set). As runtime arguments their branches inside P0's stage loop (reference unwrap, yref or pose-reference
// loads, and a pose load from either LDS or global memory, i.e. a flat load) made the compiler's waits drain the
// whole memory counter, the stage's record stores and the prefetched rows included
// RP: the launch reads the handle's per-robot table of bounds and weights or its stage table (KArgs::rparams or
// KArgs::sbounds != nullptr; the launcher picks it from the pointers). P0 then loads each lane's box per stage
// (stage_box). Launches with both tables off run the RP = false instantiations, which mention neither table
// MT: the launch reads the handle's model table (KArgs::rmodel != nullptr). Each team loads its robot's parameters in
// the prologue (robot_vals), and the column-form M block takes its constant rows from the team's own lanes
// (m_block_team: the same structural-nonzero FMAs with broadcast operands): m_block's come from the wave's first team
// and are right only while the four robots of a wave share their model parameters. The row form (mrow_pg_block) was
// measured against it and lost 2.6 to 8.6 % (profiles/r07/ab/robot_model.txt). MT implies RP: these instantiations
// serve every combination of the other two tables (stage_box_ctx's fallback), so the model table adds one
// instantiation per launch shape, not two. Launches with all three tables off run the RP = MT = false
// instantiations, which mention none of them
// The tick's text (sqp_rti_team_tick.hpp) is the body of two kernels: k_sqp_rti_team, which keeps the code it had
// before the hand-off, and k_sqp_rti_team_ho (sqp_rti_team_ho.hip, HO = true), whose unfinished teams leave the loop at
// the hand-off iteration and write a list entry (ho_ent, ho_pend) instead of their outputs
template <class M, bool MS, bool SD, int MODE, bool SP, bool RP, bool MT>
__global__ __launch_bounds__(256, 1) void k_sqp_rti_team(KParams P, KArgs a)
{
    constexpr bool HO = false;
    float* const ho_ent = nullptr;
    bool ho_pend = false;
    (void)ho_ent;
    (void)ho_pend;
#include "sqp_rti_team_tick.hpp"
}

}  // namespace

template <class M>
hipError_t launch_sqp_rti_team(const KParams& P, const KArgs& a, int mode, hipStream_t stream)
{
    if (a.B <= 0) return hipSuccess;
    // split launches: one robot per 256-lane block, P0's stage inputs in LDS (41 KB for diff at N = 80); a
    // horizon whose inputs do not fit runs unsplit
    const size_t stg = (size_t)(P.N + 1) * 16 * StageLds<M>::SF * sizeof(float);
    const size_t split_lds = stg + (mode == kModeRun ? (sizeof(double) + 3 * sizeof(float)) * (size_t)(P.N + 1) : 0);
    KArgs as = a;
    if (as.split && split_lds > 65536) as.split = 0;
    const int block = 256;  // 16 teams, or 1 robot (split)
    const long long threads = (long long)a.B * (as.split ? 256 : 16);
    const int grid = (int)((threads + block - 1) / block);
    // path mode: each team's N+1 path parameters and reference poses in LDS (16 teams x (N+1) x (8 + 12) B,
    // 26 KB at N = 80)
    const size_t lds = as.split ? split_lds
                                : ((mode == kModeRun && a.segs) ? (sizeof(double) + 3 * sizeof(float)) * 16 * (size_t)(P.N + 1) : 0);
    if (lds > 65536) return hipErrorInvalidValue;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, stream, P, as); };
    // compile-time mode (the kernel's MODE parameter)
    const int km = mode != kModeRun ? kModeSolve : (a.segs ? kModeRunPath : kModeRun);
    auto pick2 = [&](auto msc, auto sdc, auto spc) {
        constexpr bool ms = decltype(msc)::value, sd = decltype(sdc)::value, sp = decltype(spc)::value;
        auto pick3 = [&](auto rpc, auto mtc) {
            constexpr bool rp = decltype(rpc)::value, mt = decltype(mtc)::value;
            if (km == kModeRunPath) go(k_sqp_rti_team<M, ms, sd, kModeRunPath, sp, rp, mt>);
            else if (km == kModeRun) go(k_sqp_rti_team<M, ms, sd, kModeRun, sp, rp, mt>);
            else go(k_sqp_rti_team<M, ms, sd, kModeSolve, sp, rp, mt>);
        };
        // the tables: instantiations of their own (sqp_steps.hpp lane_ctx, stage_box, robot_vals). The model table's
        // read the other two as well
        if (a.rmodel) pick3(std::true_type{}, std::true_type{});
        else if (a.rparams || a.sbounds) pick3(std::true_type{}, std::false_type{});
        else pick3(std::false_type{}, std::false_type{});
    };
    // record layout: tric always split, diff per launch (a.rec_split), omni4 and Mehrotra never
    auto pick = [&](auto msc, auto sdc) {
        using R = TeamRec<M, decltype(sdc)::value>;
        if constexpr (R::SPLIT) pick2(msc, sdc, std::true_type{});
        else if constexpr (R::SPLIT_OK) {
            if (a.rec_split) pick2(msc, sdc, std::true_type{});
            else pick2(msc, sdc, std::false_type{});
        } else pick2(msc, sdc, std::false_type{});
    };
    using T = std::true_type;
    using F = std::false_type;
    if (P.ipm == 1) {
        if (a.dense) pick(T{}, T{});
        else pick(F{}, T{});
    } else if (a.dense) {
        pick(T{}, F{});
    } else {
        pick(F{}, F{});
    }
    return hipGetLastError();
}

template hipError_t launch_sqp_rti_team<Diff2>(const KParams&, const KArgs&, int, hipStream_t);
template hipError_t launch_sqp_rti_team<Omni4>(const KParams&, const KArgs&, int, hipStream_t);
template hipError_t launch_sqp_rti_team<Tric3>(const KParams&, const KArgs&, int, hipStream_t);
template size_t team_scratch_floats<Diff2>(int, int);
template size_t team_scratch_floats<Omni4>(int, int);
template size_t team_scratch_floats<Tric3>(int, int);

#ifdef NMPC_STAMPS
extern "C" int nmpc_debug_stamps_c1(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps_c1), sizeof(g_stamps_c1), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
extern "C" int nmpc_debug_stamps_pa(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps_pa), sizeof(g_stamps_pa), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
extern "C" int nmpc_debug_stamps_p1(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps_p1), sizeof(g_stamps_p1), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
extern "C" int nmpc_debug_stamps(unsigned long long* host, int n)
{
    const size_t bytes = sizeof(unsigned long long) * (size_t)n;
    if (bytes > sizeof(g_stamps)) return -1;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif

}  // namespace nmpc
