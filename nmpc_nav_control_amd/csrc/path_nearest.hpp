// path_nearest.hpp -- the nearest-point search of a FollowPath tick as device functions (k_path_nearest in
// path_nearest.hip; kept apart from the kernel so that a later fused run mode can call them).
//
// What it stands for: TPathProcessMinDist::GetMinDist as NMPCNavControlROS.cpp:597-610 calls it. That class lives in
// parametric_trajectories_common, which the reference does not vendor, so the search below is THIS project's
// (specification: include/nmpc_amd/nmpc_path.h): the exact fp64 minimiser of |P(U) - r| over the piecewise cubic path
// inside a search range, ties to the smallest U. Only the near pose and the two errors follow reference code
// (NMPCNavControlROS.cpp:654-657, utils.h:41-47).
//
// One 16-lane row per robot. Per segment, lane j takes the sample u_j = a + (b - a) j / 15 of the segment's part
// [a, b] of the search range and refines it inside its bracket [u_{j-1}, u_{j+1}] by a fixed number of safeguarded
// Newton steps on g(u) = (P - r) . P' (half the derivative of the squared distance). Every lane refines: a lane whose
// sample is a discrete local minimum brackets a true one, and the others still end on a valid path point, so their
// candidates can only help and no lane needs its neighbours' samples. The lane's candidate is the better of the
// refined point and the sample itself; a row min-reduction on (d^2, U) picks the segment's best and the rows carry
// theirs across segments. Nothing iterates on data: 16 samples, kNearNewton steps, 4 reduction steps.
#pragma once

#include <hip/hip_runtime.h>

#include "nmpc_amd/nmpc_path.h"
#include "path_march.hpp"

namespace nmpc {

constexpr int kNearNewton = 8;  // safeguarded Newton steps per lane and segment (5 reach 1e-15 m on seeded paths)

// (f1, U1) before (f2, U2): smaller squared distance, then smaller path parameter
__host__ __device__ inline bool near_less(double f1, double U1, double f2, double U2)
{
    return f1 < f2 || (f1 == f2 && U1 < U2);
}

__host__ __device__ inline double near_dist2(const double* cx, const double* cy, double rx, double ry, double u)
{
    const double dx = ((cx[3] * u + cx[2]) * u + cx[1]) * u + cx[0] - rx;
    const double dy = ((cy[3] * u + cy[2]) * u + cy[1]) * u + cy[0] - ry;
    return dx * dx + dy * dy;
}

// sample m of 16 on [a, b] (m is clamped: the brackets of lanes 0 and 15 end on the range)
__host__ __device__ inline double near_sample(double a, double b, int m)
{
    m = m < 0 ? 0 : m;
    const double u = a + (b - a) * (1.0 / 15.0) * (double)m;
    return (m >= 15 || u > b) ? b : u;
}

// Lane j's candidate on one segment (coefficients cx, cy) for the robot at (rx, ry), local range [a, b] inside
// [0, 1]: squared distance *f at local parameter *u.
__host__ __device__ inline void near_lane(const double* cx, const double* cy, double rx, double ry, double a,
                                          double b, int j, double* f, double* u_out)
{
    const double us = near_sample(a, b, j);
    double l = near_sample(a, b, j - 1), h = near_sample(a, b, j + 1);
    double u = us;
#pragma unroll
    for (int it = 0; it < kNearNewton; it++) {
        const double x = ((cx[3] * u + cx[2]) * u + cx[1]) * u + cx[0] - rx;
        const double y = ((cy[3] * u + cy[2]) * u + cy[1]) * u + cy[0] - ry;
        const double xp = (3.0 * cx[3] * u + 2.0 * cx[2]) * u + cx[1];
        const double yp = (3.0 * cy[3] * u + 2.0 * cy[2]) * u + cy[1];
        const double xpp = 6.0 * cx[3] * u + 2.0 * cx[2];
        const double ypp = 6.0 * cy[3] * u + 2.0 * cy[2];
        const double g = x * xp + y * yp;
        const double gp = xp * xp + yp * yp + x * xpp + y * ypp;
        // the minimum lies right of u while the distance still falls there
        l = (g < 0.0) ? u : l;
        h = (g < 0.0) ? h : u;
        const double un = u - g / gp;
        const bool newton = gp > 0.0 && un >= l && un <= h;  // (false on NaN): bisect
        u = newton ? un : 0.5 * (l + h);
    }
    const double fs = near_dist2(cx, cy, rx, ry, us);
    const double fu = near_dist2(cx, cy, rx, ry, u);
    const bool refined = near_less(fu, u, fs, us);
    *f = refined ? fu : fs;
    *u_out = refined ? u : us;
}

// normAngRad (include/nmpc_nav_control/utils.h:41-47, the fmod form)
__device__ inline double near_norm_ang(double a)
{
    a = fmod(a + M_PI, M_PI * 2.0);
    if (a < 0.0) a += M_PI * 2.0;
    return a - M_PI;
}

// The search range [lo, hi] of a path of n >= 1 segments from the caller's bounds (NaN: unbounded on that side)
__host__ __device__ inline void near_range(double lo_in, double hi_in, int n, double* lo, double* hi)
{
    const double N = (double)n;
    double a = (lo_in != lo_in) ? 0.0 : lo_in, b = (hi_in != hi_in) ? N : hi_in;
    a = a < 0.0 ? 0.0 : (a > N ? N : a);
    b = b < 0.0 ? 0.0 : (b > N ? N : b);
    *lo = a;
    *hi = b < a ? a : b;
}

// 16-byte loads of a record whose alignment is only that of its doubles
typedef double near_d2a __attribute__((ext_vector_type(2)));
typedef near_d2a near_d2 __attribute__((aligned(8)));

__device__ inline void near_load4(const double* p, double* c)
{
    const near_d2 v0 = *reinterpret_cast<const near_d2*>(p);
    const near_d2 v1 = *reinterpret_cast<const near_d2*>(p + 2);
    c[0] = v0.x;
    c[1] = v0.y;
    c[2] = v1.x;
    c[3] = v1.y;
}

// min-reduction of (f, U) over the 16 lanes of a row: every lane of the row returns with the row's best
__device__ inline void near_row_min(double* f, double* U)
{
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        const double of = __shfl_xor(*f, m, 16);
        const double oU = __shfl_xor(*U, m, 16);
        const bool take = near_less(of, oU, *f, *U);
        *f = take ? of : *f;
        *U = take ? oU : *U;
    }
}

// Result of one robot's search (the same in every lane of its row)
struct NearResult {
    double U;        // nearest_u
    double near[4];  // x, y, theta, theta_holonomic at U (GetMinDist's raw outputs: no reverse-driving pi)
    double err[2];   // pos_error_to_path, ori_error_to_path (NMPCNavControlROS.cpp:654-657)
};

// The whole search of one robot by its row; called by all 64 lanes of a wave, the four rows with their own robots.
//   S, n     the robot's segments and their count; n < 1 marks a row without a robot or path (no segment is read)
//   j        lane in the row
//   px..pth  the robot's pose (fp32 widened exactly)
//   lo_in, hi_in  caller's range bounds (NaN: none)
//   holo     heading of the orientation error: 1 theta_holonomic, 0 theta (+ pi on a segment driven backwards)
// (always inlined: the gate of the node tick calls it from two kernel instantiations, each of which keeps the code it
// had as the only caller)
__device__ __forceinline__ NearResult near_search(const nmpc_path_segment* S, int n, int j, double px, double py,
                                                  double pth, double lo_in, double hi_in, int holo)
{
    NearResult R;
    const double nan = __builtin_nan("");
    double lo = 0.0, hi = 0.0;
    if (n >= 1) near_range(lo_in, hi_in, n, &lo, &hi);
    // one trip count for the wave: the longest path of its four rows
    int nmax = n;
    nmax = max(nmax, __shfl_xor(nmax, 16));
    nmax = max(nmax, __shfl_xor(nmax, 32));
    nmax = __builtin_amdgcn_readfirstlane(nmax);
    double bf = INFINITY, bU = lo;
    int bad = (px != px) || (py != py) || (pth != pth);
    for (int k = 0; k < nmax; k++) {
        const double K = (double)k;
        const bool in = k < n && lo <= K + 1.0 && hi >= K;  // the same in every lane of a row
        double f = INFINITY, U = lo;
        if (in) {
            double cx[4], cy[4];
            near_load4(S[k].x, cx);
            near_load4(S[k].y, cy);
            // lo - K and hi - K are exact where they are inside [0, 1], so K + a returns lo itself
            const double a = fmin(fmax(lo - K, 0.0), 1.0), b = fmin(fmax(hi - K, 0.0), 1.0);
            double u;
            near_lane(cx, cy, px, py, a, b, j, &f, &u);
            U = K + u;
            bad |= !(f < INFINITY);  // NaN or overflow in the pose or the coefficients
            f = (f < INFINITY) ? f : INFINITY;
        }
        near_row_min(&f, &U);
        const bool take = near_less(f, U, bf, bU);
        bf = take ? f : bf;
        bU = take ? U : bU;
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) bad |= __shfl_xor(bad, m, 16);
    // (last cross-lane operation)
    R.U = (n >= 1) ? (bad ? lo : bU) : 0.0;
    if (n >= 1) {
        int k;
        double w;
        path_seg_param(R.U, n, &k, &w);
        double cx[4], cy[4], ct[4];
        near_load4(S[k].x, cx);
        near_load4(S[k].y, cy);
        near_load4(S[k].th, ct);
        const double v = S[k].v;
        R.near[0] = path_horner(cx, w);
        R.near[1] = path_horner(cy, w);
        R.near[2] = atan2(path_dhorner(cy, w), path_dhorner(cx, w));
        R.near[3] = path_horner(ct, w);
        const double head = holo ? R.near[3] : ((v < 0.0) ? R.near[2] + M_PI : R.near[2]);
        const double dx = R.near[0] - px, dy = R.near[1] - py;
        R.err[0] = bad ? nan : sqrt(dx * dx + dy * dy);
        R.err[1] = bad ? nan : fabs(near_norm_ang(head - pth));
    } else {
        R.near[0] = R.near[1] = R.near[2] = R.near[3] = nan;
        R.err[0] = R.err[1] = nan;
    }
    return R;
}

}  // namespace nmpc
