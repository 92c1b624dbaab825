// sqp_rti_team_ho.hip -- the team kernel with an in-block hand-off of its long solves ("Hand-off
// inside the block").
//
// k_sqp_rti_team's launch lasts as long as its hardest robot: a wave iterates until its slowest team stops, at about
// 104 k cycles per IPM iteration, while most of the chip's waves have long finished. Here a team that has not stopped
// at the top of IPM iteration C (KArgs::handoff) leaves the team loop, and the block's four waves, free by then,
// finish the block's unfinished robots one robot per wave in the segmented row-parallel form (four horizon segments on
// the wave's four DPP rows), whose iteration costs about 0.64 of the team's (profiles/r10/ab/handoff.txt).
//
// Phase 1 is the team tick's text (sqp_rti_team_tick.hpp, HO = true): P0 and the IPM iterations below C, unchanged; a
// finished team writes its outputs as always, an unfinished one its entry of the block's hand-off list (HoList) in
// LDS. Every wave of the block -- also one whose teams lie past the batch or past the node tick's active count, and
// one whose teams all finished -- then reaches the one block barrier. Phase 2 is the row-parallel tick's text
// (sqp_rti_rowpar_tick.hpp, RESUME, W = 1, SEG): wave w takes the flagged entries w, w + 4, ... in slot order and
// runs each from the top of iteration C to its end on its own LDS slice (ResumeLds), with the tick's own stopping
// rule, full step and output block. No second launch, no prediction, no counter between waves and no spin loop.
//
// The rule looks at the robot's own iteration count only, and which wave finishes a robot changes no arithmetic, so a
// robot's result does not depend on its slot or its neighbours (tests/test_gpu_team_handoff.py).
#include "nmpc_kernels.hpp"
#include "team_common.hpp"
#include "sqp_steps.hpp"
#include "path_march.hpp"
#include "team_tick_defs.hpp"
#include "rowpar_layout.hpp"

namespace nmpc {

// the team tick's and the row-parallel tick's diagnostic hooks (sqp_rti_team.hip, sqp_rti_rowpar.hip): this kernel
// keeps stamps of its own
#define STAMP(slot) ((void)0)
#define STAMPF(slot) ((void)0)
#define STAMPC1() ((void)0)
#define STAMPPA() ((void)0)
#define RP_MSTAMP(slot, lane) ((void)0)
#define RP_SSTAMP(i) ((void)0)
#define RP_LAG() ((void)0)
#ifdef NMPC_STAMPS
// diagnostic build only: s_memtime of the first 256 blocks. g_ho_stamps[block][wave]: [0] the wave left the team
// tick, [1] it passed the block barrier, [2] it finished its last entry, [3] the entries it ran, [4] the block's
// flagged entries. g_ho_it[block][wave]: the row-parallel tick's phase stamps (3 + 4 it + 0..3: after phases A, B,
// the master, C + D) of the first entry the wave ran
constexpr int kHoIts = 64;
__device__ unsigned long long g_ho_stamps[256][4][8];
__device__ unsigned long long g_ho_it[256][4][3 + 4 * kHoIts];
#define HO_STAMP(slot, val)                                                                                      \
    do {                                                                                                         \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 256) g_ho_stamps[blockIdx.x][ho_wave][(slot)] = (val);       \
    } while (0)
#define RP_STAMP(slot)                                                                                           \
    do {                                                                                                         \
        if (tid == 0 && ho_ran == 0 && blockIdx.x < 256 && (slot) < 3 + 4 * kHoIts)                              \
            g_ho_it[blockIdx.x][ho_wave][(slot)] = __builtin_amdgcn_s_memtime();                                 \
    } while (0)
extern "C" int nmpc_debug_stamps_ho(unsigned long long* stamps, unsigned long long* its)
{
    if (hipMemcpyFromSymbol(stamps, HIP_SYMBOL(g_ho_stamps), sizeof(g_ho_stamps), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -2;
    return hipMemcpyFromSymbol(its, HIP_SYMBOL(g_ho_it), sizeof(g_ho_it), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#else
#define HO_STAMP(slot, val) ((void)0)
#define RP_STAMP(slot) ((void)0)
#endif

namespace {

constexpr int kStampItsC = 0;  // (the team tick's stamp bound: none here)

// MODE: kModeSolve or kModeRun (run_path launches keep the plain kernel: the march owns the LDS). The other
// parameters of the team tick are fixed: the sparse store form and the single-direction rule (MS = false, SD = true:
// at most one wave per SIMD), wide records (SP = false: the records the row-parallel tick reads, tric included) and no
// per-robot table (RP = MT = false)
template <class M, int MODE>
__global__ __launch_bounds__(256, 1) void k_sqp_rti_team_ho(KParams P, KArgs a)
{
    extern __shared__ float s_ho[];
    const int ho_wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // ---- phase 1: the team tick. Its early exits (a team past the batch or past the active count) and its hand-off
    // exit return from the lambda, not from the kernel: every wave goes on to the barrier below
    float* const ho_ent = s_ho + (threadIdx.x >> 4) * HoList::ENTRY;  // this team's list entry
    bool ho_pend = false;
    [&]() __attribute__((always_inline)) {
        constexpr bool MS = false, SD = true, SP = false, RP = false, MT = false, HO = true;
#include "sqp_rti_team_tick.hpp"
    }();
    if ((threadIdx.x & 15) == 0) ho_ent[HoList::FLAG] = ho_pend ? 1.0f : 0.0f;
    HO_STAMP(0, __builtin_amdgcn_s_memtime());
    // the records, the DZ plane and the iterate rows the teams wrote, and the list: visible to the block's other waves
    __threadfence_block();
    __syncthreads();
    HO_STAMP(1, __builtin_amdgcn_s_memtime());

    // ---- phase 2: the flagged entries in slot order, entry number e on wave e mod 4
    constexpr int W = 1;
    constexpr bool SEG = true, MT = false, RESUME = true;
    constexpr int mode = MODE;
    const size_t slice = ResumeLds<M>::floats(P.N, a.seg);
    int ho_seen = 0, ho_ran = 0;
    for (int e = 0; e < 16; e++) {
        const float* const ent = s_ho + e * HoList::ENTRY;
        if (ent[HoList::FLAG] == 0.0f) continue;  // (block-uniform)
        if ((ho_seen++ & 3) != ho_wave) continue;  // (wave-uniform)
        TickResume rs;
        rs.inst = __builtin_amdgcn_readfirstlane(__float_as_int(ent[HoList::INST]));
        rs.it = a.handoff;
        rs.lds = s_ho + HoList::FLOATS + (size_t)ho_wave * slice;
        rs.alpha = ent[HoList::ALPHA];
        rs.sigma_mu = ent[HoList::SIGMA_MU];
        rs.tg_rhs = ent[HoList::TG_RHS];
        rs.mu_prev = ent[HoList::MU_PREV];
        rs.we_lane = ent[HoList::WE + (threadIdx.x & 15)];
        {
#include "sqp_rti_rowpar_tick.hpp"
        }
        ho_ran++;
    }
    (void)ho_ran;  // (read by the diagnostic build's stamps only)
    HO_STAMP(2, __builtin_amdgcn_s_memtime());
    HO_STAMP(3, (unsigned long long)ho_ran);
    HO_STAMP(4, (unsigned long long)ho_seen);
}

}  // namespace

template <class M>
size_t team_ho_lds_bytes(int N)
{
    if constexpr (M::NX >= 10) return 0;
    else {
        if (N % kHandoffSeg != 0 || N / kHandoffSeg < 2) return 0;
        return (HoList::FLOATS + 4 * ResumeLds<M>::floats(N, kHandoffSeg)) * sizeof(float);
    }
}

template <class M>
hipError_t launch_sqp_rti_team_ho(const KParams& P, const KArgs& a, int mode, hipStream_t stream)
{
    if (a.B <= 0) return hipSuccess;
    if constexpr (M::NX >= 10) {
        return hipErrorInvalidValue;
    } else {
        const size_t lds = team_ho_lds_bytes<M>(P.N);
        // (the plan's conditions, nmpc_batch.cpp plan_launch: nothing else reaches this launcher)
        if (lds == 0 || lds > 163840 || P.ipm != 1 || a.handoff <= 0 || a.seg != kHandoffSeg || a.segs || a.split ||
            a.dense || a.rec_split || a.rowpar || a.rparams || a.sbounds || a.rmodel)
            return hipErrorInvalidValue;
        const int grid = (a.B + 15) / 16;
        auto go = [&](auto kern) {
            if (lds > 65536) {
                const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) return e;
            }
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, P, a);
            return hipGetLastError();
        };
        return mode == kModeRun ? go(k_sqp_rti_team_ho<M, kModeRun>) : go(k_sqp_rti_team_ho<M, kModeSolve>);
    }
}

#define INST(M)                                                                                                      \
    template hipError_t launch_sqp_rti_team_ho<M>(const KParams&, const KArgs&, int, hipStream_t);                  \
    template size_t team_ho_lds_bytes<M>(int);
INST(Diff2)
INST(Omni4)
INST(Tric3)
#undef INST

}  // namespace nmpc
