// stage_bounds.hip -- the writers of the stage table (nmpc_batch.h "Stage-varying bounds"): every robot's box at every
// stage of the horizon, fp32, rows lbx[NBX] ubx[NBX] lbu[NBU] ubu[NBU] per stage and robot, laid out by sb_at
// (nmpc_kernels.hpp). Both solve kernels read a lane's pair of a stage in P0 (stage_box, sqp_steps.hpp). Every writer
// is one elementwise launch on the caller's stream: thread i of a (stage, row) or of a row takes robot i, every index
// is checked against B <= capacity, and nothing is read back on the host.
#include "nmpc_kernels.hpp"

namespace nmpc {
namespace {

constexpr int kSbThreads = 256;

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
    int f = 0;
#pragma unroll
    for (int g = 1; g < kSbFields; g++)
        if (row >= sb_off(g, d.nbx, d.nbu)) f = g;
    const float* const s = src.f[f];
    const bool inp = f >= kSbLbu;  // input rows: the caller's arrays have N stages
    if (!s || (inp && k >= d.N)) return;
    const int n = inp ? d.nbu : d.nbx;
    sb[sb_at(k, row, i, d.cap, rows)] = s[((size_t)k * n + (row - sb_off(f, d.nbx, d.nbu))) * B + i];
}

// nmpc_model_params_set_limits per robot and stage (block y: the stage): v_max, alpha_min, alpha_max [N+1][B],
// a_max, dalpha_max [N][B]
__global__ void k_sb_limits(float* sb, SbDims d, int B, int tric, const float* v_max, const float* a_max,
                            const float* alpha_min, const float* alpha_max, const float* dalpha_max,
                            const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= B || (mask && !mask[i])) return;
    const int rows = sb_rows(d.nbx, d.nbu);
    const int nv = tric ? 1 : d.nbx, na = tric ? 1 : d.nbu;  // tric: slot 1 of each box is the steering's
    auto at = [&](int field, int j) -> float& { return sb[sb_at(k, sb_off(field, d.nbx, d.nbu) + j, i, d.cap, rows)]; };
    const size_t e = (size_t)k * B + i;
    if (v_max) {
        const float v = v_max[e];
        for (int j = 0; j < nv; j++) { at(kSbLbx, j) = -v; at(kSbUbx, j) = v; }
    }
    if (a_max && k < d.N) {
        const float v = a_max[e];
        for (int j = 0; j < na; j++) { at(kSbLbu, j) = -v; at(kSbUbu, j) = v; }
    }
    if (tric) {
        if (alpha_min) at(kSbLbx, 1) = alpha_min[e];
        if (alpha_max) at(kSbUbx, 1) = alpha_max[e];
        if (dalpha_max && k < d.N) { at(kSbLbu, 1) = -dalpha_max[e]; at(kSbUbu, 1) = dalpha_max[e]; }
    }
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

dim3 grid_of(int n, int y) { return dim3((n + kSbThreads - 1) / kSbThreads, y); }

}  // namespace

hipError_t launch_sb_fill(float* sb, const SbDims& d, const RpColumn& col, const float* rp, const RpRows& rr,
                          hipStream_t stream)
{
    if (d.cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sb_fill, grid_of(d.cap, (d.N + 1) * sb_rows(d.nbx, d.nbu)), dim3(kSbThreads), 0, stream, sb, d,
                       col, rp, rr);
    return hipGetLastError();
}

hipError_t launch_sb_set(float* sb, const SbDims& d, int B, const nmpc_stage_bounds& s, const unsigned char* mask,
                         hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    const SbSrc src = {{s.lbx, s.ubx, s.lbu, s.ubu}};
    hipLaunchKernelGGL(k_sb_set, grid_of(B, (d.N + 1) * sb_rows(d.nbx, d.nbu)), dim3(kSbThreads), 0, stream, sb, d, B,
                       src, mask);
    return hipGetLastError();
}

hipError_t launch_sb_limits(float* sb, const SbDims& d, int B, int tric, const float* v_max, const float* a_max,
                            const float* alpha_min, const float* alpha_max, const float* dalpha_max,
                            const unsigned char* mask, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sb_limits, grid_of(B, d.N + 1), dim3(kSbThreads), 0, stream, sb, d, B, tric, v_max, a_max,
                       alpha_min, alpha_max, dalpha_max, mask);
    return hipGetLastError();
}

hipError_t launch_sb_shift(float* sb, const SbDims& d, int B, int n, const unsigned char* mask, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sb_shift, grid_of(B, sb_rows(d.nbx, d.nbu)), dim3(kSbThreads), 0, stream, sb, d, B, n, mask);
    return hipGetLastError();
}

}  // namespace nmpc
