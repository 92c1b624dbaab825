// robot_params.hip -- the writers of the per-robot table of bounds and weights (nmpc_batch.h "Per-robot bounds and
// weights"). The table is [rows][capacity] fp32, instance-minor like the carried refs: rows lbx ubx lbu ubu W W_e
// (RpRows, nmpc_kernels.hpp). Both solve kernels read a robot's column in their prologue (lane_ctx / load_x0,
// sqp_steps.hpp). Every writer is one elementwise launch on the caller's stream: thread i of a row writes robot i, so
// a row's stores are coalesced, and nothing is read back on the host.
#include "nmpc_kernels.hpp"

namespace nmpc {
namespace {

constexpr int kRpThreads = 256;

// every robot's column = the handle's own parameters (block y: the row)
__global__ void k_rp_fill(float* table, int cap, RpColumn col)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (i < cap) table[(size_t)row * cap + i] = col.v[row];
}

struct RpSrc {
    const float* f[kRpFields];
};

// block y: the row; its field's source is [n][B], or nullptr (the row stays)
__global__ void k_rp_set(float* table, int cap, int B, RpRows rr, RpSrc src, const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (i >= B || (mask && !mask[i])) return;
    int f = 0;
#pragma unroll
    for (int g = 1; g < kRpFields; g++)
        if (row >= rr.off[g]) f = g;
    const float* const s = src.f[f];
    if (!s) return;
    table[(size_t)row * cap + i] = s[(size_t)(row - rr.off[f]) * B + i];
}

// nmpc_model_params_set_limits per robot: ref states in [-v_max, v_max], inputs in [-a_max, a_max]; tric: the second
// bounded state in [alpha_min, alpha_max], the second input in [-dalpha_max, dalpha_max]
__global__ void k_rp_limits(float* table, int cap, int B, RpRows rr, int tric, const float* v_max, const float* a_max,
                            const float* alpha_min, const float* alpha_max, const float* dalpha_max,
                            const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B || (mask && !mask[i])) return;
    const int nbx = rr.off[kRpUbx] - rr.off[kRpLbx], nbu = rr.off[kRpUbu] - rr.off[kRpLbu];
    const int nv = tric ? 1 : nbx, na = tric ? 1 : nbu;  // tric: slot 1 of each box is the steering's
    auto at = [&](int field, int j) -> float& { return table[(size_t)(rr.off[field] + j) * cap + i]; };
    if (v_max) {
        const float v = v_max[i];
        for (int j = 0; j < nv; j++) { at(kRpLbx, j) = -v; at(kRpUbx, j) = v; }
    }
    if (a_max) {
        const float v = a_max[i];
        for (int j = 0; j < na; j++) { at(kRpLbu, j) = -v; at(kRpUbu, j) = v; }
    }
    if (tric) {
        if (alpha_min) at(kRpLbx, 1) = alpha_min[i];
        if (alpha_max) at(kRpUbx, 1) = alpha_max[i];
        if (dalpha_max) { at(kRpLbu, 1) = -dalpha_max[i]; at(kRpUbu, 1) = dalpha_max[i]; }
    }
}

}  // namespace

hipError_t launch_rp_fill(float* table, int cap, int rows, const RpColumn& col, hipStream_t stream)
{
    if (cap <= 0 || rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rp_fill, dim3((cap + kRpThreads - 1) / kRpThreads, rows), dim3(kRpThreads), 0, stream, table,
                       cap, col);
    return hipGetLastError();
}

hipError_t launch_rp_set(float* table, int cap, int B, const RpRows& rr, const nmpc_robot_params& rp,
                         const unsigned char* mask, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    const RpSrc src = {{rp.lbx, rp.ubx, rp.lbu, rp.ubu, rp.W, rp.W_e}};
    hipLaunchKernelGGL(k_rp_set, dim3((B + kRpThreads - 1) / kRpThreads, rr.off[kRpFields]), dim3(kRpThreads), 0,
                       stream, table, cap, B, rr, src, mask);
    return hipGetLastError();
}

hipError_t launch_rp_limits(float* table, int cap, int B, const RpRows& rr, int tric, const float* v_max,
                            const float* a_max, const float* alpha_min, const float* alpha_max,
                            const float* dalpha_max, const unsigned char* mask, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rp_limits, dim3((B + kRpThreads - 1) / kRpThreads), dim3(kRpThreads), 0, stream, table, cap,
                       B, rr, tric, v_max, a_max, alpha_min, alpha_max, dalpha_max, mask);
    return hipGetLastError();
}

}  // namespace nmpc
