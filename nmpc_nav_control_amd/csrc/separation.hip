// separation.hip -- fleet separation (nmpc_batch.h "Fleet separation"; DESIGN.md section 4 "Fleet separation"): the
// export of the resident horizons as tracks (nmpc_batch_export_tracks) and, for nmpc_batch_stage_limits_from_tracks,
// the squared distance q_k from every stage of every processed robot to the nearest counting track. The rule's tail
// (gap_k, s_k, z_k, r_k, lim_k and the table's rows) is k_speed_map's, which reads the q plane as an optional operand.
//
// k_track_boxes: one lane per track, the bounding box of the track stages 0..min(K, N) the rule can read (fmin / fmax:
// a NaN position, which never counts, leaves no mark).
// k_sep_min: a 16-lane row per robot, 16 robots per block, no LDS and no barrier. A lane owns the stages
// k0 + lane + 16 u, u < kU, of a tile of 16 kU stages: their fp64 map positions, directions of travel and running
// minima stay in registers; a horizon longer than a tile takes further passes over the tracks. The tracks are taken
// in chunks of 16: each lane tests one track's box against the robot's horizon box, the hits of the row come out of
// one ballot, and for every hit the lanes evaluate their stages. The loop over a chunk's hits is bounded by 16.
// The cull is invisible: a pair that the rule counts has fl(fl(dx^2) + fl(dy^2)) <= range^2, so its exact
// dx^2 + dy^2 is within 2^-21 of range^2 relative; the boxes contain both ends, the fp64 subtraction is monotone, so
// the boxes' squared distance is no larger; it is compared with range^2 (1 + 1e-5). Every comparison that involves a
// NaN keeps the track. min is exact, so neither tiles nor chunks show in the bits; the file is compiled without
// contraction (Makefile), so dx*dx + dy*dy is mul, mul, add.
// The guard form (k_sep_min<true>, nmpc_sep_guard): a lane keeps two running minima per owned stage, qa over every
// counting pair (the q of the form above) and qy over those whose track has priority[j] >= the robot's own; the
// priority of a hit is one row-uniform load per hit, inside the loop bounded by 16. A held robot stands at its pose
// like a reset one but keeps the iterate's direction. The cull's argument is unchanged: the filter only removes pairs
// from the set the cull is conservative for, and qa is that set's minimum. k_sep_min<false> is the code above.
// k_sep_hold: one lane per robot strides the stages 0..min(hold_stages, N) of the qa plane (instance-minor reads, a
// trip count that no data decides) and applies the hysteresis of the protective hold.
#include "nmpc_kernels.hpp"

namespace nmpc {
namespace {

constexpr int kThreads = 256;
constexpr int kRow = 16;  // lanes per robot
constexpr int kU = 3;     // stages per lane and tile: 48 stages, the bench's N = 40 in one pass

__global__ void __launch_bounds__(kThreads) k_export_tracks(ExportTracksArgs a)
{
    const long long n = (long long)(a.K + 1) * a.B;
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const int k = (int)(e / a.B), i = (int)(e % a.B);
    bool stand = a.reset && a.reset[i] != 0;
    if (!stand && a.held) stand = a.held[i] != 0;
    if (!stand && a.mode) stand = !(a.mode[i] == NMPC_NODE_GOTO_POSE || a.mode[i] == NMPC_NODE_FOLLOW_PATH);
    const int kk = k <= a.N ? k : a.N;
    const float x = stand ? a.pose[i] : a.xbar[((size_t)kk * a.nx + 0) * a.cap + i];
    const float y = stand ? a.pose[(size_t)a.B + i] : a.xbar[((size_t)kk * a.nx + 1) * a.cap + i];
    const double ox = a.origin ? a.origin[i] : 0.0, oy = a.origin ? a.origin[(size_t)a.cap + i] : 0.0;
    a.xy[((size_t)k * 2 + 0) * a.M + a.first + i] = (double)x + ox;
    a.xy[((size_t)k * 2 + 1) * a.M + a.first + i] = (double)y + oy;
}

// boxes [4][M]: lo x, hi x, lo y, hi y over the track stages 0..last
__global__ void __launch_bounds__(kThreads) k_track_boxes(const double* xy, int M, int last, double* boxes)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= M) return;
    double lx = INFINITY, hx = -INFINITY, ly = INFINITY, hy = -INFINITY;
    for (int k = 0; k <= last; k++) {
        const double x = xy[((size_t)k * 2 + 0) * M + j], y = xy[((size_t)k * 2 + 1) * M + j];
        lx = fmin(lx, x); hx = fmax(hx, x);
        ly = fmin(ly, y); hy = fmax(hy, y);
    }
    boxes[j] = lx;
    boxes[(size_t)M + j] = hx;
    boxes[(size_t)2 * M + j] = ly;
    boxes[(size_t)3 * M + j] = hy;
}

__device__ inline double row_min(double v)
{
    for (int d = kRow / 2; d > 0; d >>= 1) v = fmin(v, __shfl_xor(v, d, kRow));
    return v;
}
__device__ inline double row_max(double v)
{
    for (int d = kRow / 2; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d, kRow));
    return v;
}

template <bool Guard>
__global__ void __launch_bounds__(kThreads) k_sep_min(SepArgs a)
{
    const int row = threadIdx.x / kRow, lane = threadIdx.x % kRow;
    const int i = blockIdx.x * (kThreads / kRow) + row;
    const int N = a.d.N, cap = a.d.cap, M = a.M;
    bool go = i < a.B;
    if (go && a.mask) go = a.mask[i] != 0;
    if (go && a.mode) go = a.mode[i] == NMPC_NODE_GOTO_POSE || a.mode[i] == NMPC_NODE_FOLLOW_PATH;
    const int ic = i < a.B ? i : 0;  // (a row without a robot reads robot 0's data, in bounds, and writes nothing)
    const bool fresh = a.reset && a.reset[ic] != 0;  // has no direction: h_k = 0
    bool stand = fresh;                              // stands: the pose at every stage
    int pown = 0;
    if constexpr (Guard) {
        stand = fresh || a.held[ic] != 0;
        // (own_priority NULL: the host has checked own_first >= 0 and own_first + B <= M)
        if (a.priority) pown = a.own_priority ? a.own_priority[ic] : a.priority[a.own_first + ic];
    }
    const double ox = a.origin ? a.origin[ic] : 0.0, oy = a.origin ? a.origin[(size_t)cap + ic] : 0.0;
    const float px = stand ? a.pose[ic] : 0.0f, py = stand ? a.pose[(size_t)a.B + ic] : 0.0f;
    const int own = a.own_first >= 0 ? a.own_first + i : -1;
    const int rsh = ((threadIdx.x % warpSize) / kRow) * kRow;  // the row's bits in the wave's ballot

    // the robot's horizon box in map coordinates
    double rlx = INFINITY, rhx = -INFINITY, rly = INFINITY, rhy = -INFINITY;
    for (int k = lane; k <= N; k += kRow) {
        const float x = stand ? px : a.xbar[((size_t)k * a.nx + 0) * cap + ic];
        const float y = stand ? py : a.xbar[((size_t)k * a.nx + 1) * cap + ic];
        const double X = (double)x + ox, Y = (double)y + oy;
        rlx = fmin(rlx, X); rhx = fmax(rhx, X);
        rly = fmin(rly, Y); rhy = fmax(rhy, Y);
    }
    rlx = row_min(rlx); rhx = row_max(rhx);
    rly = row_min(rly); rhy = row_max(rhy);

    for (int k0 = 0; k0 <= N; k0 += kRow * kU) {
        double X[kU], Y[kU];
        float hx[kU], hy[kU], q[kU];
        [[maybe_unused]] float qa[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int k = k0 + lane + kRow * u;
            const int kc = k <= N ? k : N;  // (in bounds; a stage past N is not written)
            const int k1 = kc + 1 <= N ? kc + 1 : N, k2 = kc <= N - 1 ? kc : N - 1;
            const float x = stand ? px : a.xbar[((size_t)kc * a.nx + 0) * cap + ic];
            const float y = stand ? py : a.xbar[((size_t)kc * a.nx + 1) * cap + ic];
            X[u] = (double)x + ox;
            Y[u] = (double)y + oy;
            hx[u] = fresh ? 0.0f : a.xbar[((size_t)k1 * a.nx + 0) * cap + ic] - a.xbar[((size_t)k2 * a.nx + 0) * cap + ic];
            hy[u] = fresh ? 0.0f : a.xbar[((size_t)k1 * a.nx + 1) * cap + ic] - a.xbar[((size_t)k2 * a.nx + 1) * cap + ic];
            q[u] = INFINITY;
            if constexpr (Guard) qa[u] = INFINITY;
        }
        for (int c = 0; c < M; c += kRow) {
            const int jt = c + lane;
            const int jc = jt < M ? jt : M - 1;
            const double tlx = a.boxes[jc], thx = a.boxes[(size_t)M + jc];
            const double tly = a.boxes[(size_t)2 * M + jc], thy = a.boxes[(size_t)3 * M + jc];
            const double gx = fmax(0.0, fmax(tlx - rhx, rlx - thx)), gy = fmax(0.0, fmax(tly - rhy, rly - thy));
            const bool far = gx * gx + gy * gy > a.cull2;  // (false for a NaN: the track is kept)
            const bool hit = go && jt < M && jt != own && !far;
            unsigned bits = (unsigned)((__ballot(hit) >> rsh) & 0xffffull);
            while (bits) {  // at most 16 rounds
                const int j = c + __ffs(bits) - 1;
                bits &= bits - 1;
                [[maybe_unused]] bool yields = true;  // the robot gives way to this track: the pair enters qy
                if constexpr (Guard) yields = !a.priority || a.priority[j] >= pown;
#pragma unroll
                for (int u = 0; u < kU; u++) {
                    const int k = k0 + lane + kRow * u;
                    const int kc = k <= N ? k : N;
                    const int kk = kc <= a.K ? kc : a.K;
                    const double Tx = a.xy[((size_t)kk * 2 + 0) * M + j], Ty = a.xy[((size_t)kk * 2 + 1) * M + j];
                    const float dx = (float)(Tx - X[u]), dy = (float)(Ty - Y[u]);
                    const float qq = dx * dx + dy * dy;
                    bool counts = qq <= a.range2;  // (a NaN fails)
                    if (a.ahead_only) counts = counts && ((hx[u] == 0.0f && hy[u] == 0.0f) || dx * hx[u] + dy * hy[u] > 0.0f);
                    if constexpr (Guard) {
                        if (counts) qa[u] = fminf(qa[u], qq);
                        if (counts && yields) q[u] = fminf(q[u], qq);
                    } else {
                        if (counts) q[u] = fminf(q[u], qq);
                    }
                }
            }
        }
        if (go) {
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int k = k0 + lane + kRow * u;
                if (k <= N) a.q[(size_t)k * cap + i] = q[u];
                if constexpr (Guard)
                    if (k <= N) {
                        a.qa[(size_t)k * cap + i] = qa[u];
                        if (a.gap_all) a.gap_all[(size_t)k * a.B + i] = sqrtf(qa[u]);
                    }
            }
        }
    }
}

// held' = reset ? 0 : (held ? m < release_gap : m < stop_gap), m the smallest gap over the protective field's stages
// (fminf: a NaN never counts; +inf when nothing counts); a robot in a mode that does not solve, and every robot with
// hold == 0, gets 0
__global__ void __launch_bounds__(kThreads) k_sep_hold(SepHoldArgs a)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.B) return;
    float m = INFINITY;
    for (int k = 0; k <= a.last; k++) m = fminf(m, sqrtf(a.qa[(size_t)k * a.cap + i]));
    const unsigned char md = a.mode ? a.mode[i] : (unsigned char)NMPC_NODE_GOTO_POSE;
    const bool drives = md == NMPC_NODE_GOTO_POSE || md == NMPC_NODE_FOLLOW_PATH;
    const bool fresh = a.reset && a.reset[i] != 0;
    const bool was = a.held[i] != 0;
    const bool now = a.hold && drives && !fresh && (was ? m < a.release_gap : m < a.stop_gap);
    a.held[i] = now ? 1 : 0;
    if (a.held_out) a.held_out[i] = now ? 1 : 0;
    if (a.mode_rw) {  // the cycle: the gate sees a held robot in IDLE; k_cycle_status brings its mode back
        a.mode_save[i] = md;
        if (a.remains) a.remains_save[i] = a.remains[i];
        if (now) a.mode_rw[i] = NMPC_NODE_IDLE;
    }
}

}  // namespace

hipError_t launch_export_tracks(const ExportTracksArgs& a, hipStream_t stream)
{
    if (a.B <= 0) return hipSuccess;
    const long long n = (long long)(a.K + 1) * a.B;
    hipLaunchKernelGGL(k_export_tracks, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_sep_min(const SepArgs& a, hipStream_t stream)
{
    if (a.B <= 0) return hipSuccess;
    if (a.M > 0) {
        const int last = a.K < a.d.N ? a.K : a.d.N;
        hipLaunchKernelGGL(k_track_boxes, dim3((a.M + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, a.xy, a.M,
                           last, a.boxes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int R = kThreads / kRow;
    if (a.guard)
        hipLaunchKernelGGL(k_sep_min<true>, dim3((a.B + R - 1) / R), dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(k_sep_min<false>, dim3((a.B + R - 1) / R), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_sep_hold(const SepHoldArgs& a, hipStream_t stream)
{
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sep_hold, dim3((a.B + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nmpc
