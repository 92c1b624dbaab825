// speed_map.hip -- the stage table's speed rows from a speed map (nmpc_batch_stage_limits_from_map, nmpc_batch.h
// "Speed zones"; DESIGN.md section 4 "Speed zones"). One launch: every processed robot's stage positions are looked up
// in the grid and the limit profile of the rule is written into the rows nmpc_batch_set_stage_limits' v_max writes.
//
// Mapping: a block of 256 lanes holds R robots, blockDim / R lanes each (16 lanes, one DPP row, per robot up to
// N = 1023; fewer robots per block above, so that the block's z values fit 64 KiB of LDS). A robot's lanes stride the
// stages. Phase 1: a lane loads the positions of up to kChunk of its stages (instance-minor rows of xbar: the loads of
// a chunk are issued together), looks each up (the cell index is clamped into the grid, the load is unconditional and
// `outside` is selected afterwards: no data-dependent branch) and leaves z_k in LDS as [stage][robot of the block].
// Phase 2, behind a block barrier: a lane evaluates the closed form min_j (z_j + (j - k) g) for each of its stages,
// one multiply and one add per candidate. min is exact, so the mapping does not show in the bits; the file is compiled
// without contraction (Makefile), so neither does the compiler.
// Fleet separation (separation.hip, nmpc_batch_stage_limits_from_tracks) reaches the rule through one optional
// operand: sep_q, the squared distance to the nearest counting track per stage, caps z_k before phase 2. The map is
// optional then (vmax nullptr: no cell limits). With sep_q nullptr the kernel computes what it computed without it.
#include "nmpc_kernels.hpp"

namespace nmpc {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4;  // stages a lane has in flight in phase 1
constexpr size_t kLdsMax = 65536;

// m_k: the cell of the map position (X, Y), or `outside` off the grid and for a position that is not finite
__device__ inline float cell_limit(const nmpc_speed_map& m, double X, double Y)
{
    const double fx = floor((X - m.x0) / m.res), fy = floor((Y - m.y0) / m.res);
    // (a NaN fails every comparison; an infinity fails one of them)
    const bool in = fx >= 0.0 && fx < (double)m.w && fy >= 0.0 && fy < (double)m.h;
    const int cx = in ? (int)fx : 0, cy = in ? (int)fy : 0;
    const float v = m.vmax[(size_t)cy * (size_t)m.w + (size_t)cx];
    return in ? v : m.outside;
}

__global__ void __launch_bounds__(kThreads) k_speed_map(SpeedMapArgs a, int R)
{
    extern __shared__ float zs[];  // [N+1][R]
    const int L = kThreads / R;    // lanes per robot
    const int row = threadIdx.x / L, lane = threadIdx.x % L;
    const int i = blockIdx.x * R + row;
    const int N = a.d.N, cap = a.d.cap;
    bool go = i < a.B;
    if (go && a.mask) go = a.mask[i] != 0;
    if (go && a.mode) go = a.mode[i] == NMPC_NODE_GOTO_POSE || a.mode[i] == NMPC_NODE_FOLLOW_PATH;
    const int nv = sb_speed_rows(a.tric, a.d.nbx);

    // (a lane without a robot reads nothing and writes nothing, but meets the barrier)
    float g = 0.0f, c = 0.0f;
    if (go) {
        const float vcap = a.rp ? a.rp[(size_t)a.rp_ubx * cap + i] : a.cap;
        const float acc = a.rp ? a.rp[(size_t)a.rp_ubu * cap + i] : a.a;
        g = (a.slope * acc) * a.dt;
        for (int j = 0; j < nv; j++) c = fmaxf(c, fabsf(a.carried[(size_t)j * cap + i]));
        const bool fresh = a.reset && a.reset[i] != 0;  // the iterate is about to be zeroed: the pose at every stage
        const double ox = a.origin ? a.origin[i] : 0.0, oy = a.origin ? a.origin[(size_t)cap + i] : 0.0;
        const float px = fresh ? a.pose[i] : 0.0f, py = fresh ? a.pose[(size_t)a.B + i] : 0.0f;
        for (int k0 = lane; k0 <= N; k0 += kChunk * L) {
            float x[kChunk], y[kChunk];
#pragma unroll
            for (int u = 0; u < kChunk; u++) {
                const int k = k0 + u * L;
                const int kk = k <= N ? k : N;  // (in bounds; the value is dropped below)
                x[u] = fresh ? px : a.xbar[((size_t)kk * a.nx + 0) * cap + i];
                y[u] = fresh ? py : a.xbar[((size_t)kk * a.nx + 1) * cap + i];
            }
#pragma unroll
            for (int u = 0; u < kChunk; u++) {
                const int k = k0 + u * L;
                // (no map: m_k = +inf, the limit is the cap)
                const float m = a.map.vmax ? cell_limit(a.map, (double)x[u] + ox, (double)y[u] + oy) : INFINITY;
                float z = fminf(vcap, fmaxf(a.v_floor, m));
                if (a.sep_q && k <= N) {  // fleet separation: the cap from the gap to the nearest counting track
                    const float gap = sqrtf(a.sep_q[(size_t)k * cap + i]);
                    const float sk = a.sep_gain * (gap - a.sep_clearance);
                    z = fminf(z, fmaxf(a.v_floor, sk));
                    if (a.gap) a.gap[(size_t)k * a.B + i] = gap;
                }
                if (k <= N) zs[(size_t)k * R + row] = z;
            }
        }
    }
    __syncthreads();
    if (!go) return;
    const int rows = sb_rows(a.d.nbx, a.d.nbu);
    const int lo = sb_off(kSbLbx, a.d.nbx, a.d.nbu), hi = sb_off(kSbUbx, a.d.nbx, a.d.nbu);
    for (int k = lane; k <= N; k += L) {
        float r = zs[(size_t)k * R + row];  // j = k: z_k + 0 * g
        for (int j = k + 1; j <= N; j++) r = fminf(r, zs[(size_t)j * R + row] + (float)(j - k) * g);
        const float lim = fmaxf(r, c - (float)k * g);
        for (int j = 0; j < nv; j++) {
            a.sb[sb_at(k, lo + j, i, cap, rows)] = -lim;
            a.sb[sb_at(k, hi + j, i, cap, rows)] = lim;
        }
        if (a.vlim) a.vlim[(size_t)k * a.B + i] = lim;
    }
}

}  // namespace

hipError_t launch_speed_map(const SpeedMapArgs& a, hipStream_t stream)
{
    if (a.B <= 0) return hipSuccess;
    // robots per block: 16 (one 16-lane row each) while the block's z values fit the LDS, else the next power of two
    int R = 16;
    while (R > 1 && sizeof(float) * (size_t)(a.d.N + 1) * R > kLdsMax) R /= 2;
    const size_t lds = sizeof(float) * (size_t)(a.d.N + 1) * R;
    if (lds > kLdsMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_speed_map, dim3((a.B + R - 1) / R), dim3(kThreads), lds, stream, a, R);
    return hipGetLastError();
}

}  // namespace nmpc
