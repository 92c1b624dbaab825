// path_nearest.hip -- nmpc_path_nearest (include/nmpc_amd/nmpc_path.h): each robot's nearest path point, the first
// step of a FollowPath tick (NMPCNavControlROS.cpp:648-664), for B robots in one launch.
//
// One 16-lane row per robot, four robots per wave, blocks of 256 (16 robots). The search is path_nearest.hpp's: 16
// samples per segment, a fixed number of safeguarded Newton steps per lane, a row min-reduction by lane shuffles; no
// LDS, no loop on data. Rows past the last robot run with an empty path (no loads, no stores) and still take part in
// the wave's cross-lane operations, so nothing returns early.
#include <hip/hip_runtime.h>

#include "nmpc_amd/nmpc_path.h"
#include "nmpc_kernels.hpp"
#include "path_nearest.hpp"

namespace nmpc {
namespace {

constexpr int kNearBlock = 256;

__global__ void __launch_bounds__(kNearBlock) k_path_nearest(int B, const nmpc_path_segment* segs, int seg_stride,
                                                             const int* nseg, const float* pose,
                                                             const double* origin, int ostride, const double* lo,
                                                             const double* hi, int holo, double* nearest_u,
                                                             double* near, double* err)
{
    const size_t t = (size_t)blockIdx.x * kNearBlock + threadIdx.x;
    const size_t i = t >> 4;
    const int j = (int)(t & 15);
    const bool live = i < (size_t)B;
    const size_t Bn = (size_t)B;
    int n = live ? nseg[i] : 0;
    n = n > seg_stride ? seg_stride : n;  // never past the robot's own records
    n = n < 1 ? 0 : n;
    double px = 0.0, py = 0.0, pth = 0.0, lo_in = 0.0, hi_in = 0.0;
    if (live) {
        px = (double)pose[i];
        py = (double)pose[Bn + i];
        if (origin) {  // a handle's frame: the pose is relative to the robot's origin, the path in map coordinates
            px += origin[i];
            py += origin[(size_t)ostride + i];
        }
        pth = (double)pose[2 * Bn + i];
        lo_in = lo ? lo[i] : __builtin_nan("");
        hi_in = hi ? hi[i] : __builtin_nan("");
    }
    const NearResult R = near_search(segs + i * (size_t)seg_stride, n, j, px, py, pth, lo_in, hi_in, holo);
    if (live && j == 0) {
        nearest_u[i] = R.U;
        if (near) {
#pragma unroll
            for (int c = 0; c < 4; c++) near[c * Bn + i] = R.near[c];
        }
        if (err) {
            err[i] = R.err[0];
            err[Bn + i] = R.err[1];
        }
    }
}

// the path-error check of a FollowPath tick (NMPCNavControlROS.cpp:658-660): a robot whose position or orientation
// error reaches its threshold is flagged and gets the stop command; use_pos / use_ori: the comparison is on
__global__ void k_path_guard(int B, const double* err, double max_pos, double max_ori, int use_pos, int use_ori,
                             unsigned char* off_path, float* cmd)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const bool off = (use_pos && err[i] >= max_pos) || (use_ori && err[(size_t)B + i] >= max_ori);
    if (off_path) off_path[i] = off ? 1 : 0;
    if (off && cmd)
        for (int j = 0; j < 3; j++) cmd[(size_t)j * B + i] = 0.0f;
}

}  // namespace

hipError_t launch_path_guard(int B, const double* err, double max_pos, double max_ori, int use_pos, int use_ori,
                             unsigned char* off_path, float* cmd, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_path_guard, dim3((B + 255) / 256), dim3(256), 0, stream, B, err, max_pos, max_ori, use_pos,
                       use_ori, off_path, cmd);
    return hipGetLastError();
}

hipError_t launch_path_nearest(int B, const nmpc_path_segment* segs, int seg_stride, const int* nseg,
                               const float* pose, const double* origin, int ostride, const double* lo,
                               const double* hi, int holo, double* nearest_u, double* near, double* err,
                               hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((size_t)B * 16 + kNearBlock - 1) / kNearBlock);
    hipLaunchKernelGGL(k_path_nearest, dim3(blocks), dim3(kNearBlock), 0, stream, B, segs, seg_stride, nseg, pose,
                       origin, ostride, lo, hi, holo, nearest_u, near, err);
    return hipGetLastError();
}

}  // namespace nmpc
