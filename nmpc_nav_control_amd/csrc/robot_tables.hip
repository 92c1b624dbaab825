// robot_tables.hip -- the writers of the handle's four per-robot device tables (DESIGN.md "Per-robot device tables",
// nmpc_batch.h):
//   the per-robot table of bounds and weights, [rows][capacity] fp32, rows lbx ubx lbu ubu W W_e (RpRows,
//   nmpc_kernels.hpp); both solve kernels read a robot's column in their prologue (lane_ctx / load_x0, sqp_steps.hpp);
//   the model table, [NP][capacity] fp32, row j every robot's p[j] (diff {b, tau_v}, omni4 {l1 + l2, tau_v}, tric
//   {d, tau_v, tau_a}); the solve kernels read a column in their prologue (robot_vals), the harness plant in its lead
//   lane (fleet_sim.hip);
//   the stage table, every robot's box at every stage, rows lbx ubx lbu ubu per stage and robot laid out by sb_at
//   (nmpc_kernels.hpp); the solve kernels read a lane's pair of a stage in P0 (stage_box);
//   the frame table, [2][capacity] fp64, every robot's map origin x, then y; the launches that read path segments
//   bridge a robot's frame and the map with it (the team kernel's march, node_gate.hip, path_nearest.hip), and its
//   writer moves the resident iterate's position rows along, so that the iterate's map position stays.
// Every writer is one elementwise launch on the caller's stream: x over robots in blocks of 256, thread i of a row, of
// a (stage, row) or of a stage writes robot i (a row-major row's stores are coalesced), every index is checked against
// B <= capacity, and nothing is read back or checked on the host.
#include "frame_move.hpp"
#include "nmpc_kernels.hpp"

namespace nmpc {
namespace {

constexpr int kThreads = 256;
dim3 grid_of(int n, int y = 1) { return dim3((n + kThreads - 1) / kThreads, y); }

// the field of a row: the last of kFields fields whose first row (off(g)) is not past it
template <int kFields, class Off>
__device__ inline int field_of(int row, Off off)
{
    int f = 0;
#pragma unroll
    for (int g = 1; g < kFields; g++)
        if (row >= off(g)) f = g;
    return f;
}

// ---- the row-major tables [row][cap] ------------------------------------------------------------------------------
// every robot's column = col, the handle's own values (block y: the row)
__global__ void k_rows_fill(float* table, int cap, RpColumn col)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (i < cap) table[(size_t)row * cap + i] = col.v[row];
}

// a field list: field f holds the rows [off[f], off[f + 1]) and its source is [n][B], or nullptr (those rows stay)
template <int kFields>
struct RowFields {
    int off[kFields + 1];
    const float* src[kFields];
};

// block y: the row (the per-robot table's six fields, or the model table's one)
template <int kFields>
__global__ void k_rows_set(float* table, int cap, int B, RowFields<kFields> fl, const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (i >= B || (mask && !mask[i])) return;
    const int f = field_of<kFields>(row, [&](int g) { return fl.off[g]; });
    const float* const s = fl.src[f];
    if (!s) return;
    table[(size_t)row * cap + i] = s[(size_t)(row - fl.off[f]) * B + i];
}

// ---- nmpc_model_params_set_limits per robot, or per robot and stage -----------------------------------------------
struct LimSrc {
    const float *v_max, *a_max, *alpha_min, *alpha_max, *dalpha_max;
};

// Robot i's box (stage k's when the sources are per stage: v_max, alpha_min, alpha_max [N+1][B], a_max, dalpha_max
// [N][B], so the input rows stop at k < N; else [B] each): ref states in [-v_max, v_max], inputs in [-a_max, a_max];
// tric: the second bounded state in [alpha_min, alpha_max], the second input in [-dalpha_max, dalpha_max].
// at(field, j): the table's float of slot j of the box field (kSbLbx .. kSbUbu, the per-robot table's first four)
template <bool kPerStage, class At>
__device__ inline void limits_body(At at, int i, int k, int N, int B, int nbx, int nbu, int tric, const LimSrc& s)
{
    const int nv = sb_speed_rows(tric, nbx), na = tric ? 1 : nbu;  // tric: slot 1 of each box is the steering's
    const size_t e = kPerStage ? (size_t)k * B + i : (size_t)i;
    const bool inp = !kPerStage || k < N;
    if (s.v_max) {
        const float v = s.v_max[e];
        for (int j = 0; j < nv; j++) { at(kSbLbx, j) = -v; at(kSbUbx, j) = v; }
    }
    if (s.a_max && inp) {
        const float v = s.a_max[e];
        for (int j = 0; j < na; j++) { at(kSbLbu, j) = -v; at(kSbUbu, j) = v; }
    }
    if (tric) {
        if (s.alpha_min) at(kSbLbx, 1) = s.alpha_min[e];
        if (s.alpha_max) at(kSbUbx, 1) = s.alpha_max[e];
        if (s.dalpha_max && inp) { at(kSbLbu, 1) = -s.dalpha_max[e]; at(kSbUbu, 1) = s.dalpha_max[e]; }
    }
}
static_assert((int)kSbLbx == (int)kRpLbx && (int)kSbUbx == (int)kRpUbx && (int)kSbLbu == (int)kRpLbu &&
                  (int)kSbUbu == (int)kRpUbu,
              "the box fields come first in the per-robot table, in the stage table's order");

__global__ void k_rp_limits(float* table, int cap, int B, RpRows rr, int tric, LimSrc src, const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B || (mask && !mask[i])) return;
    auto at = [&](int field, int j) -> float& { return table[(size_t)(rr.off[field] + j) * cap + i]; };
    limits_body<false>(at, i, 0, 0, B, rr.off[kRpUbx] - rr.off[kRpLbx], rr.off[kRpUbu] - rr.off[kRpLbu], tric, src);
}

// block y: the stage
__global__ void k_sb_limits(float* sb, SbDims d, int B, int tric, LimSrc src, const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= B || (mask && !mask[i])) return;
    const int rows = sb_rows(d.nbx, d.nbu);
    auto at = [&](int field, int j) -> float& { return sb[sb_at(k, sb_off(field, d.nbx, d.nbu) + j, i, d.cap, rows)]; };
    limits_body<true>(at, i, k, d.N, B, d.nbx, d.nbu, tric, src);
}

// ---- the stage table [stage][robot][row] ---------------------------------------------------------------------------
// block y: stage * rows + row. Every stage of robot i = its column of the per-robot table, or the handle's values
__global__ void k_sb_fill(float* sb, SbDims d, RpColumn col, const float* rp, RpRows rr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int rows = sb_rows(d.nbx, d.nbu);
    const int k = blockIdx.y / rows, row = blockIdx.y % rows;
    if (i >= d.cap) return;
    // (the stage rows are the first rows of the per-robot table, in the same order)
    sb[sb_at(k, row, i, d.cap, rows)] = rp ? rp[(size_t)(rr.off[kRpLbx] + row) * d.cap + i] : col.v[row];
}

struct SbSrc {
    const float* f[kSbFields];
};

// block y: stage * rows + row; the row's field source is [N+1 or N][n][B], or nullptr (the row stays)
__global__ void k_sb_set(float* sb, SbDims d, int B, SbSrc src, const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int rows = sb_rows(d.nbx, d.nbu);
    const int k = blockIdx.y / rows, row = blockIdx.y % rows;
    if (i >= B || (mask && !mask[i])) return;
    const int f = field_of<kSbFields>(row, [&](int g) { return sb_off(g, d.nbx, d.nbu); });
    const float* const s = src.f[f];
    const bool inp = f >= kSbLbu;  // input rows: the caller's arrays have N stages
    if (!s || (inp && k >= d.N)) return;
    const int n = inp ? d.nbu : d.nbx;
    sb[sb_at(k, row, i, d.cap, rows)] = s[((size_t)k * n + (row - sb_off(f, d.nbx, d.nbu))) * B + i];
}

// block y: the row. Stage k takes stage min(k + n, last) of the same row, last = N (state rows) or N - 1 (input rows);
// k walks upwards and k + n >= k, so a source is read before it is overwritten
__global__ void k_sb_shift(float* sb, SbDims d, int B, int n, const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (i >= B || (mask && !mask[i])) return;
    const int rows = sb_rows(d.nbx, d.nbu);
    const int last = row >= sb_off(kSbLbu, d.nbx, d.nbu) ? d.N - 1 : d.N;
    for (int k = 0; k <= last; k++) {
        const int ks = (n > last - k) ? last : k + n;  // (no k + n overflow for a large n)
        sb[sb_at(k, row, i, d.cap, rows)] = sb[sb_at(ks, row, i, d.cap, rows)];
    }
}

// ---- the frame table [2][cap], fp64 ---------------------------------------------------------------------------------
// One thread per robot: it reads both of the robot's old origins before it writes either, decides (pose_map) from both
// coordinates, and walks the stages of the iterate's x and y rows, so no other thread needs what it overwrites
__global__ void k_frame_set(double* fr, int cap, int B, float* xbar, int N, int nx, const double* origin,
                            const double* pose_map, double radius, unsigned char* moved, const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    bool go = !mask || mask[i];
    const double ox = fr[i], oy = fr[(size_t)cap + i];
    double nx_o = 0.0, ny_o = 0.0;
    if (pose_map) {
        const double x = pose_map[i], y = pose_map[(size_t)B + i];
        go = go && frame_recentre_go(x, y, ox, oy, radius);
        nx_o = rint(x);
        ny_o = rint(y);
        if (moved) moved[i] = go ? 1 : 0;
    } else if (origin) {
        nx_o = origin[i];
        ny_o = origin[(size_t)B + i];
    }
    if (!go) return;
    frame_move(fr, cap, i, xbar, N, nx, ox, oy, nx_o, ny_o);
}

// element e of an array [n][c][B]: robot e % B, component (e / B) % c
template <bool kTo>
__global__ void k_frame_map(const double* fr, int cap, int B, int c, size_t total, const double* map_in,
                            const float* frame_in, float* frame_out, double* map_out)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e % (size_t)B), comp = (int)((e / (size_t)B) % (size_t)c);
    const double o = (fr && comp < 2) ? fr[(size_t)comp * cap + i] : 0.0;
    if (kTo) {
        const double v = map_in[e];
        frame_out[e] = (float)(comp < 2 ? v - o : v);
    } else {
        const double v = (double)frame_in[e];
        map_out[e] = comp < 2 ? v + o : v;
    }
}

}  // namespace

hipError_t launch_rows_fill(float* table, int cap, int rows, const RpColumn& col, hipStream_t stream)
{
    if (cap <= 0 || rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_fill, grid_of(cap, rows), dim3(kThreads), 0, stream, table, cap, col);
    return hipGetLastError();
}

template <int kFields>
hipError_t launch_rows_set(float* table, int cap, int B, const int (&off)[kFields + 1],
                           const float* const (&src)[kFields], const unsigned char* mask, hipStream_t stream)
{
    if (B <= 0 || off[kFields] <= 0) return hipSuccess;
    RowFields<kFields> fl;
    for (int f = 0; f <= kFields; f++) fl.off[f] = off[f];
    for (int f = 0; f < kFields; f++) fl.src[f] = src[f];
    hipLaunchKernelGGL(k_rows_set<kFields>, grid_of(B, off[kFields]), dim3(kThreads), 0, stream, table, cap, B, fl,
                       mask);
    return hipGetLastError();
}
template hipError_t launch_rows_set<kRpFields>(float*, int, int, const int (&)[kRpFields + 1],
                                               const float* const (&)[kRpFields], const unsigned char*, hipStream_t);
template hipError_t launch_rows_set<1>(float*, int, int, const int (&)[2], const float* const (&)[1],
                                       const unsigned char*, hipStream_t);

hipError_t launch_rp_limits(float* table, int cap, int B, const RpRows& rr, int tric, const float* v_max,
                            const float* a_max, const float* alpha_min, const float* alpha_max,
                            const float* dalpha_max, const unsigned char* mask, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    const LimSrc src = {v_max, a_max, alpha_min, alpha_max, dalpha_max};
    hipLaunchKernelGGL(k_rp_limits, grid_of(B), dim3(kThreads), 0, stream, table, cap, B, rr, tric, src, mask);
    return hipGetLastError();
}

hipError_t launch_sb_limits(float* sb, const SbDims& d, int B, int tric, const float* v_max, const float* a_max,
                            const float* alpha_min, const float* alpha_max, const float* dalpha_max,
                            const unsigned char* mask, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    const LimSrc src = {v_max, a_max, alpha_min, alpha_max, dalpha_max};
    hipLaunchKernelGGL(k_sb_limits, grid_of(B, d.N + 1), dim3(kThreads), 0, stream, sb, d, B, tric, src, mask);
    return hipGetLastError();
}

hipError_t launch_sb_fill(float* sb, const SbDims& d, const RpColumn& col, const float* rp, const RpRows& rr,
                          hipStream_t stream)
{
    if (d.cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sb_fill, grid_of(d.cap, (d.N + 1) * sb_rows(d.nbx, d.nbu)), dim3(kThreads), 0, stream, sb, d,
                       col, rp, rr);
    return hipGetLastError();
}

hipError_t launch_sb_set(float* sb, const SbDims& d, int B, const nmpc_stage_bounds& s, const unsigned char* mask,
                         hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    const SbSrc src = {{s.lbx, s.ubx, s.lbu, s.ubu}};
    hipLaunchKernelGGL(k_sb_set, grid_of(B, (d.N + 1) * sb_rows(d.nbx, d.nbu)), dim3(kThreads), 0, stream, sb, d, B,
                       src, mask);
    return hipGetLastError();
}

hipError_t launch_sb_shift(float* sb, const SbDims& d, int B, int n, const unsigned char* mask, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sb_shift, grid_of(B, sb_rows(d.nbx, d.nbu)), dim3(kThreads), 0, stream, sb, d, B, n, mask);
    return hipGetLastError();
}

hipError_t launch_frame_set(double* fr, int cap, int B, float* xbar, int N, int nx, const double* origin,
                            const double* pose_map, double radius, unsigned char* moved, const unsigned char* mask,
                            hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_frame_set, grid_of(B), dim3(kThreads), 0, stream, fr, cap, B, xbar, N, nx, origin, pose_map,
                       radius, moved, mask);
    return hipGetLastError();
}

namespace {
template <bool kTo>
hipError_t launch_frame_map(const double* fr, int cap, int B, int n, int c, const double* map_in, const float* frame_in,
                            float* frame_out, double* map_out, hipStream_t stream)
{
    const size_t total = (size_t)n * (size_t)c * (size_t)B;
    if (total == 0) return hipSuccess;
    const size_t blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_frame_map<kTo>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, fr, cap, B, c, total,
                       map_in, frame_in, frame_out, map_out);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_to_frame(const double* fr, int cap, int B, int n, int c, const double* map, float* out,
                           hipStream_t stream)
{
    return launch_frame_map<true>(fr, cap, B, n, c, map, nullptr, out, nullptr, stream);
}

hipError_t launch_from_frame(const double* fr, int cap, int B, int n, int c, const float* in, double* map,
                             hipStream_t stream)
{
    return launch_frame_map<false>(fr, cap, B, n, c, nullptr, in, nullptr, map, stream);
}

}  // namespace nmpc
