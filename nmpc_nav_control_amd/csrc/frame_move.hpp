// frame_move.hpp -- one robot's step of the frame table's writers (robot_tables.hip: k_frame_set; node_input.hip: the
// input stage's in-launch recentre), stated once so that the two launches take the same decision and move the resident
// iterate by the same arithmetic, bit for bit. fr is the frame table [2][cap] (fp64: origin x, then y), xbar the
// resident iterate [(N+1)*nx][cap]; the calling thread owns robot i < cap and nothing else reads or writes its columns.
#pragma once
#include <hip/hip_runtime.h>

namespace nmpc {

// nmpc_batch_recentre's decision for a robot at (x, y) in map coordinates whose origin is (ox, oy): farther than radius
// in x or y, and finite (false on a NaN position or radius)
__device__ inline bool frame_recentre_go(double x, double y, double ox, double oy, double radius)
{
    return (fabs(x - ox) > radius || fabs(y - oy) > radius) && isfinite(x) && isfinite(y);
}

// Robot i takes the origin (nox, noy) in place of (ox, oy): the x and y row of every stage of its iterate becomes
// (float)((double)x + (o_old - o_new)), so that its map position stays
__device__ inline void frame_move(double* fr, int cap, int i, float* xbar, int N, int nx, double ox, double oy,
                                  double nox, double noy)
{
    fr[i] = nox;
    fr[(size_t)cap + i] = noy;
    const double dx = ox - nox, dy = oy - noy;
    for (int k = 0; k <= N; k++) {
        float* const x = xbar + ((size_t)k * nx) * cap + i;
        x[0] = (float)((double)x[0] + dx);
        x[cap] = (float)((double)x[cap] + dy);
    }
}

}  // namespace nmpc
