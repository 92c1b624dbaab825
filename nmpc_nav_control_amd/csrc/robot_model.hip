// robot_model.hip -- the writers of the model table (nmpc_batch.h "Per-robot model parameters"). The table is
// [NP][capacity] fp32, instance-minor like the per-robot table of bounds and weights: row j holds every robot's p[j]
// (diff {b, tau_v}, omni4 {l1 + l2, tau_v}, tric {d, tau_v, tau_a}). Both solve kernels read a robot's column in their
// prologue (robot_vals, sqp_steps.hpp), the harness plant in its lead lane (fleet_sim.hip). Every writer is one
// elementwise launch on the caller's stream: thread i of a row writes robot i, so a row's stores are coalesced, and
// nothing is read back or checked on the host.
#include "nmpc_kernels.hpp"

namespace nmpc {
namespace {

constexpr int kRmThreads = 256;

// every robot's column = the handle's own parameters (block y: the row)
__global__ void k_rm_fill(float* table, int cap, RmColumn p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (i < cap) table[(size_t)row * cap + i] = p.v[row];
}

// block y: the row; src is [np][B]
__global__ void k_rm_set(float* table, int cap, int B, const float* src, const unsigned char* mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (i >= B || (mask && !mask[i])) return;
    table[(size_t)row * cap + i] = src[(size_t)row * B + i];
}

}  // namespace

hipError_t launch_rm_fill(float* table, int cap, int np, const RmColumn& p, hipStream_t stream)
{
    if (cap <= 0 || np <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rm_fill, dim3((cap + kRmThreads - 1) / kRmThreads, np), dim3(kRmThreads), 0, stream, table, cap,
                       p);
    return hipGetLastError();
}

hipError_t launch_rm_set(float* table, int cap, int B, int np, const float* src, const unsigned char* mask,
                         hipStream_t stream)
{
    if (B <= 0 || np <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rm_set, dim3((B + kRmThreads - 1) / kRmThreads, np), dim3(kRmThreads), 0, stream, table, cap, B,
                       src, mask);
    return hipGetLastError();
}

}  // namespace nmpc
