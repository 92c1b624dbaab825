// sqp_rti_rowpar.hip -- batched SQP-RTI step for small batches: one block of W wavefronts per robot (W = 4 up to
// 256 robots: one wave per SIMD of the robot's CU), the stage-independent work spread over the block's 4 W DPP rows,
// only the recursions over the horizon serial.
//
// The same single-direction IPM as k_sqp_rti_team (sqp_rti_team.hip, SD rule; DESIGN.md "Algorithm and
// precision"), the same records, warm start and stopping rule, reorganised for latency. In the team kernel one
// 16-lane team runs every stage of every sweep in turn: per IPM iteration 81 x ~350 instructions of P1 and
// 81 x ~130 of the forward sweep at N = 80, one robot's solve being the reference's whole deployment
// (NMPCNavControlROS.cpp:713 -> NMPCNavControlDiff.cpp:142). Most of that work does not depend on the
// neighbouring stage: applying the step, the slacks / multipliers, the residuals, the barrier weights and the
// rhs terms before the Riccati step (phase A), and the bound directions, the step bound and the complementarity
// polynomial after the forward recursion (phase D). Here row q of the block (lanes 16q .. 16q+15 of its wave
// q / 4; lane 16q + v owns variable v as in a team) runs those phases for stages q, q + 4 W, ..., and block
// reductions (LDS) combine the rows; the Riccati factorisation (phase B: fp64 P G, G'P G, input-block Cholesky,
// rhs) and the forward recursion of the directions (phase C) are the only stage-serial passes, and every wave
// computes them identically on its row 0 (same records, same DPP broadcasts inside the row), so no wave waits on
// another; wave 0 stores them, the other waves store to pads. The fields an IPM iteration makes and uses up stay in
// LDS (ItLds: barrier weights, rhs terms, factor columns, the direction), so only the iterate, slacks and
// multipliers are written back to the global records per iteration. P0 likewise: the RK4
// linearisation of stage k on row k mod 4 W, then the serial initial-iterate pass from LDS.
// One robot per block also makes every loop exit block-uniform (no lockstep teams).
#include "nmpc_kernels.hpp"
#include "team_common.hpp"
#include "sqp_steps.hpp"
#include "rowpar_layout.hpp"  // RowRec, ItLds, SegLayout, RowLds, TickResume, the row reductions

namespace nmpc {

#ifdef NMPC_STAMPS
// diagnostic build only: s_memtime after each phase, robots 0..255, lane 0: [0] start, [1] P0a, [2] P0b, then per
// IPM iteration it: [3 + 4 it + 0..3] after phases A, B, C, D
constexpr int kRpIts = 64;
__device__ unsigned long long g_rp_stamps[256][3 + 4 * kRpIts];
#define RP_STAMP(slot)                                                                                           \
    do {                                                                                                         \
        if (tid == 0 && inst < 256 && (slot) < 3 + 4 * kRpIts) g_rp_stamps[inst][(slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
extern "C" int nmpc_debug_stamps_rowpar(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_rp_stamps), sizeof(g_rp_stamps), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
// the segment master's parts, per IPM iteration (lane 0): [0] start, [1] both sweeps done, [4] join done,
// [5] both propagations done, [7] after the block barrier (slots 2, 3, 6: unused since the one-stream master)
__device__ unsigned long long g_rp_mstamps[256][kRpIts][8];
#define RP_MSTAMP(slot, lane)                                                                                    \
    do {                                                                                                         \
        if (tid == (lane) && inst < 256 && it < kRpIts) g_rp_mstamps[inst][it][(slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
extern "C" int nmpc_debug_mstamps_rowpar(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_rp_mstamps), sizeof(g_rp_mstamps), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
// per master step of the backward sweep (lane 0): [it][i] after boundary step i
__device__ unsigned long long g_rp_sstamps[256][kRpIts][16];
#define RP_SSTAMP(i)                                                                                            \
    do {                                                                                                         \
        if (tid == 0 && inst < 256 && it < kRpIts && (i) < 16) g_rp_sstamps[inst][it][(i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
extern "C" int nmpc_debug_sstamps_rowpar(unsigned long long* host)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_rp_sstamps), sizeof(g_rp_sstamps), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#else
#define RP_STAMP(slot) ((void)0)
#define RP_MSTAMP(slot, lane) ((void)0)
#define RP_SSTAMP(i) ((void)0)
#endif

#ifdef NMPC_LAG_WAVE
// checker build only (lib/chk_lag, tests/test_gpu_rowpar_handoff.py): one wave of every robot with inst % 3 == 1 --
// wave NMPC_LAG_WAVE of a four-wave block, wave 0 (the factorisation's) of a two-wave block -- falls behind the rest of
// its block before its first P0a round and at its entry to phase B in every IPM iteration, so that every wave that
// takes its data through an LDS counter really has to wait for it. Timing only: the arithmetic is the product's, so a
// result that differs from the product's is an ordering dependence. The lag is a fixed run of 16 s_sleep 127
// (16 x 127 x 64 = about 130 k cycles; no loop on memory, no data-dependent bound), sized against the whole of P0a
// (24 k cycles) and a phase-B segment (20.7 k mean, 33.5 k max: profiles/r06/stamps/rowpar_B1024_N40.txt): the other
// waves are done with either well before the lagging wave starts. The spin loops' bound of 1 << 24 polls of at least
// 64 cycles each is four orders of magnitude above it.
#define RP_LAG()                                                                                                 \
    do {                                                                                                         \
        if (wave == (W == 4 ? (NMPC_LAG_WAVE) : 0) && inst % 3 == 1)                                             \
            for (int lag_i = 0; lag_i < 16; lag_i++) __builtin_amdgcn_s_sleep(127);                              \
    } while (0)
#else
#define RP_LAG() ((void)0)
#endif

namespace {

// W waves per robot (one per SIMD): the stage-parallel phases run on all 4 W rows; every wave runs the serial
// phases (identically) and wave 0 stores their results (into LDS; the other waves store into pads).
// SEG: the horizon is cut into a.seg segments of L = N / S stages whose Riccati sweeps (phase B) and forward
// recursions (phase C) run at the same time, one segment per row, joined by a master recursion over the segment
// boundaries (DESIGN.md "Segmented Riccati"); a robot's serial chain shrinks from N + 1 stage steps to L + 1 plus S - 1
// master steps. The rhs is built in absolute form (no adjoint), so the stationarity residual of the stopping rule is
// evaluated by its own serial adjoint pass, only when the rest of the exit test already holds.
// Register bound of the segmented diff / tric instantiations: two waves per SIMD for W <= 2 (launches above 256
// robots put two robots' waves on each SIMD, tests/test_reg_usage.py), one for W = 4 (launches of at most 256 robots,
// one block per CU). Bounding the four-wave kernel to 256 registers as well (round 5) made the compiler serialise the
// master step's LDS operand loads through one register; without it the one-robot capsule takes 0.260 instead of
// 0.279 ms cold (same box, profiles/r06/ab/p0b_w4.txt). -DNMPC_W4_BOUND2 keeps round 5's bound for A/B runs.
#ifdef NMPC_W4_BOUND2
constexpr int kRowparW2Max = 4;
#else
constexpr int kRowparW2Max = 2;
#endif
// MT: the launch reads the handle's model table (KArgs::rmodel != nullptr; the launcher picks it from the pointer).
// The tick's text (sqp_rti_rowpar_tick.hpp) is the body of two kernels: k_sqp_rti_rowpar (MT = false), whose model
// functors read KParams::p as kernel arguments and which keeps the code it had before the model table, and
// k_sqp_rti_rowtab (MT = true), which loads the robot's column in the prologue. Measured alternatives
// (profiles/r07/ab/robot_model.txt): a run-time branch on the pointer held p in registers from the prologue to the
// output block and cost diff1024 1.05 % with the table off; one __device__ body called by both kernels takes the
// kernel arguments by reference and no longer compiles to the table-off code either. (Two kernel names, not a fourth
// template parameter: tests/test_reg_usage.py counts k_sqp_rti_rowpar's instantiations.)
#define ROWPAR_BOUNDS __launch_bounds__(64 * W, (SEG && M::NX < 10 && W <= kRowparW2Max) ? 2 : 1)
template <class M, int W, bool SEG>
__global__ ROWPAR_BOUNDS void k_sqp_rti_rowpar(KParams P, KArgs a, int mode)
{
    constexpr bool MT = false, RESUME = false;
    const TickResume rs{};
#include "sqp_rti_rowpar_tick.hpp"
}
template <class M, int W, bool SEG>
__global__ ROWPAR_BOUNDS void k_sqp_rti_rowtab(KParams P, KArgs a, int mode)
{
    constexpr bool MT = true, RESUME = false;
    const TickResume rs{};
#include "sqp_rti_rowpar_tick.hpp"
}
#undef ROWPAR_BOUNDS

}  // namespace

template <class M>
size_t rowpar_lds_bytes(int N, int mode, int seg)
{
    (void)mode;
    return RowLds<M>::floats(N, seg) * sizeof(float);
}

template <class M>
hipError_t launch_sqp_rti_rowpar(const KParams& P, const KArgs& a, int mode, hipStream_t stream)
{
    if (a.B <= 0) return hipSuccess;
    const size_t lds = rowpar_lds_bytes<M>(P.N, mode, a.seg);
    if (lds > 163840 || P.ipm != 1 || a.segs) return hipErrorInvalidValue;  // (the host keeps every robot resident)
    // segments: N % S == 0, at most kSegMax and at most one per row of the block
    const int W = a.rowpar >= 4 ? 4 : (a.rowpar == 2 ? 2 : 1);
    if (a.seg < 0 || a.seg > kSegMax || a.seg > 4 * W || (a.seg > 0 && P.N % a.seg != 0))
        return hipErrorInvalidValue;
    const int grid = a.B;
    // (a block above 64 KiB of LDS -- a long horizon on four waves, or omni4's wider stage fields -- asks for it)
    auto go = [&](auto kern, int threads) {
        if (lds > 65536) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, P, a, mode);
        return hipGetLastError();
    };
    if (a.rmodel) {  // the model table: k_sqp_rti_rowtab, the same shapes
        if (W == 4) return a.seg > 0 ? go(k_sqp_rti_rowtab<M, 4, true>, 256) : go(k_sqp_rti_rowtab<M, 4, false>, 256);
        if (W == 2 && a.seg > 0) return go(k_sqp_rti_rowtab<M, 2, true>, 128);
        return a.seg > 0 ? go(k_sqp_rti_rowtab<M, 1, true>, 64) : go(k_sqp_rti_rowtab<M, 1, false>, 64);
    }
    if (W == 4)  // four waves per robot (one per SIMD of its CU)
        return a.seg > 0 ? go(k_sqp_rti_rowpar<M, 4, true>, 256) : go(k_sqp_rti_rowpar<M, 4, false>, 256);
    if (W == 2 && a.seg > 0)  // two waves per robot above 256 robots (the default there)
        return go(k_sqp_rti_rowpar<M, 2, true>, 128);
    return a.seg > 0 ? go(k_sqp_rti_rowpar<M, 1, true>, 64) : go(k_sqp_rti_rowpar<M, 1, false>, 64);
}

#define INST(M)                                                                                                      \
    template hipError_t launch_sqp_rti_rowpar<M>(const KParams&, const KArgs&, int, hipStream_t);                   \
    template size_t rowpar_lds_bytes<M>(int, int, int);
INST(Diff2)
INST(Omni4)
INST(Tric3)
#undef INST

}  // namespace nmpc
