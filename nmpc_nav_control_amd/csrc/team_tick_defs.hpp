// team_tick_defs.hpp -- what the kernels that include the team tick (sqp_rti_team_tick.hpp) share besides
// team_common.hpp and sqp_steps.hpp: the sweeps' buffer counts, the constant load sources and the march's mode value.
// Included by sqp_rti_team.hip and sqp_rti_team_ho.hip.
#pragma once
#include "nmpc_kernels.hpp"
#include "team_common.hpp"

namespace nmpc {

// The hand-off list of a k_sqp_rti_team_ho block, at the start of its LDS: one entry per team slot of the block. A
// team that leaves the team loop unfinished writes its entry (every lane its terminal weight, lane 0 the scalars), and
// every team its flag; after the block barrier the waves take the flagged entries in slot order
struct HoList {
    static constexpr int ENTRY = 32;                 // floats per entry
    static constexpr int WE = 0;                     // [16] the lanes' terminal weights (run mode: after the hack)
    static constexpr int INST = 16, ALPHA = 17, SIGMA_MU = 18, TG_RHS = 19, MU_PREV = 20, FLAG = 21;
    static constexpr int FLOATS = 16 * ENTRY;        // the waves' slices follow
};

namespace {
#ifndef LIGHT_D
#define LIGHT_D 4  // record buffers of the forward light sweeps (F0, F1)
#endif
#ifndef LIGHT_DC
#define LIGHT_DC LIGHT_D  // record buffers of the corrector backward sweep (C1)
#endif
#ifndef P1_D
#define P1_D 2  // record buffers of the factorisation sweep (2: ping-pong)
#endif

// zeros: the source of a cold robot's warm-start multiplier loads (load_l in P0)
__device__ float g_zero4[4];
// split records (TeamRec::SPLIT): the bound pair of a slot without a bound -- TL TU LL LU | LB UB -- as P0 writes
// it for bounded slots outside their stage range (kFar slacks and bounds, zero multipliers)
__device__ __attribute__((aligned(16))) float g_rec_sentinel[8] = {kFar, kFar, 0.0f, 0.0f, -kFar, kFar, 0.0f, 0.0f};

// the team kernels' MODE value of run mode with the in-kernel path march (a.segs set)
constexpr int kModeRunPath = 2;
}  // namespace
}  // namespace nmpc
