// node_input.hip -- the node's input stage (include/nmpc_amd/nmpc_batch.h: nmpc_batch_push_samples,
// nmpc_batch_node_input, nmpc_batch_node_cycle): getInputData (NMPCNavControlROS.cpp:545-553) for B robots.
//
// Three elementwise launches, one lane per robot in blocks of 256, every index checked against B <= capacity:
//   k_push_samples  the listener: a robot's new sample into the slot after its newest one.
//   k_node_input    getRobotPose, getRobotVel and the steering angle on the robot's ring into its held values, the
//                   validity rule, the recentre of its map frame (frame_move.hpp, the function nmpc_batch_recentre's
//                   launch uses) and the fp32 frame values the tick takes.
//   k_cycle_status  nmpc_batch_node_cycle's status rule after the tick.
// The state is instance-minor (lane i reads element i of every row, so a wave's loads coalesce). A lane walks its ring
// once, depth trips whatever the ring holds, and finds in that walk the newest sample and the neighbours of both
// lookups; nothing else loops over data. The stage moves depth * 32 bytes of ring and about 150 bytes of held values,
// origins and outputs per robot.
// Every fp64 product-sum below is compiled without contraction, so the host restatement (tests/node_input_ref.py)
// reproduces the ring, held.x, y and theta and both lookups bit for bit; v, vn and w go through cos and sin. The
// Makefile compiles this file with -ffp-contract=off: the library's -ffp-contract=fast disregards the pragma below,
// which is what a build with fast-honor-pragmas goes by.
#include <hip/hip_runtime.h>

#include "frame_move.hpp"
#include "nmpc_amd/nmpc_batch.h"
#include "nmpc_kernels.hpp"
#include "path_nearest.hpp"

#pragma clang fp contract(off)

namespace nmpc {
namespace {

constexpr int kThreads = 256;
enum { kHeldX = 0, kHeldY, kHeldTheta, kHeldV, kHeldVn, kHeldW, kHeldSteer, kHeldRows };

// ros::Duration::toSec of d nanoseconds: whole seconds (floor) plus the nanosecond part
__device__ inline double in_sec(long long d)
{
    long long q = d / 1000000000LL, r = d - q * 1000000000LL;
    if (r < 0) {
        q -= 1;
        r += 1000000000LL;
    }
    return (double)q + 1e-9 * (double)r;
}

// a robot's slot and count as stored, brought into range (a restored checkpoint is device data like any other)
__device__ inline int in_slot(int v, int depth) { return (int)((unsigned)v % (unsigned)depth); }
__device__ inline int in_count(int v, int depth) { return v < 0 ? 0 : (v > depth ? depth : v); }

__global__ void k_push_samples(NodeInputState st, int B, const long long* stamp_ns, const double* sample,
                               const unsigned char* mask, unsigned char* dropped)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const size_t cap = (size_t)st.cap, Bn = (size_t)B;
    bool drop = false;
    if (!mask || mask[i]) {
        const long long ts = stamp_ns[i];
        const double x = sample[i], y = sample[Bn + i], yaw = sample[2 * Bn + i];
        const int c = in_count(st.count[i], st.depth), nw = in_slot(st.newest[i], st.depth);
        drop = !(isfinite(x) && isfinite(y) && isfinite(yaw)) || (c > 0 && ts <= st.stamp[(size_t)nw * cap + i]);
        if (!drop) {
            const int s = c > 0 ? (nw + 1) % st.depth : 0;
            st.stamp[(size_t)s * cap + i] = ts;
            double* const v = st.sample + (size_t)s * 3 * cap + i;
            v[0] = x;
            v[cap] = y;
            v[2 * cap] = yaw;
            st.newest[i] = s;
            st.count[i] = c < st.depth ? c + 1 : st.depth;
        }
    }
    if (dropped) dropped[i] = drop ? 1 : 0;
}

// lookup(t) while the ring is walked: an exact hit, or the stored neighbours a (the latest before t) and b (the
// earliest after it)
struct Lookup {
    long long t, ta, tb;
    bool hit, has_a, has_b;
    double h[3], a[3], b[3];
    __device__ void start(long long t_) { t = t_; ta = tb = 0; hit = has_a = has_b = false; }
    __device__ void see(long long s, double x, double y, double yaw)
    {
        if (s == t) {
            hit = true;
            h[0] = x; h[1] = y; h[2] = yaw;
        } else if (s < t) {
            if (!has_a || s > ta) {
                has_a = true;
                ta = s;
                a[0] = x; a[1] = y; a[2] = yaw;
            }
        } else if (!has_b || s < tb) {
            has_b = true;
            tb = s;
            b[0] = x; b[1] = y; b[2] = yaw;
        }
    }
    // false: t is outside the stored stamps (or the ring is empty)
    __device__ bool get(double* x, double* y, double* yaw) const
    {
        if (hit) {
            *x = h[0]; *y = h[1]; *yaw = h[2];
            return true;
        }
        if (!(has_a && has_b)) return false;
        const double r = in_sec(t - ta) / in_sec(tb - ta);
        *x = (1.0 - r) * a[0] + r * b[0];
        *y = (1.0 - r) * a[1] + r * b[1];
        *yaw = a[2] + r * near_norm_ang(b[2] - a[2]);
        return true;
    }
};

__global__ void __launch_bounds__(kThreads) k_node_input(NodeInputArgs g)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.B) return;
    const size_t cap = (size_t)g.st.cap, Bn = (size_t)g.B;
    const int depth = g.st.depth;
    const nmpc_node_input& in = g.in;
    const int m = (int)g.mode[i];
    const bool ran = m == NMPC_NODE_GOTO_POSE || m == NMPC_NODE_FOLLOW_PATH || m == NMPC_NODE_BREAK;
    double held[kHeldRows];
    for (int r = 0; r < kHeldRows; r++) held[r] = g.st.held[(size_t)r * cap + i];
    bool valid = true;
    if (ran) {
        // one walk: the newest sample (getRobotPose's lookup at Time(0)) and both of getRobotVel's lookups
        const int c = in_count(g.st.count[i], depth), nw = in_slot(g.st.newest[i], depth);
        const long long t2 = g.st.stamp[(size_t)nw * cap + i], t1 = t2 - in.period_ns;
        Lookup l1, l2;
        l1.start(t1);
        l2.start(t2);
        for (int s = 0; s < depth; s++) {
            const long long ts = g.st.stamp[(size_t)s * cap + i];
            const double* const v = g.st.sample + (size_t)s * 3 * cap + i;
            const double x = v[0], y = v[cap], yaw = v[2 * cap];
            if ((nw - s + depth) % depth < c) {  // slot s holds one of the robot's c samples
                l1.see(ts, x, y, yaw);
                l2.see(ts, x, y, yaw);
            }
        }
        bool pose_ok = false, vel_ok = false;
        double x2 = 0.0, y2 = 0.0, yaw2 = 0.0;
        if (c > 0 && l2.get(&x2, &y2, &yaw2)) {
            // getRobotPose (:409-429)
            held[kHeldX] = x2;
            held[kHeldY] = y2;
            const double last_theta = held[kHeldTheta];
            double curr_theta = yaw2;
            const double delta = curr_theta - last_theta;
            if (delta > M_PI) curr_theta -= 2.0 * M_PI;
            else if (delta < -M_PI) curr_theta += 2.0 * M_PI;
            for (int k = 0; k < 2; k++)
                if (curr_theta >= 2.0 * M_PI) curr_theta -= 2.0 * M_PI;
            for (int k = 0; k < 2; k++)
                if (curr_theta <= -2.0 * M_PI) curr_theta += 2.0 * M_PI;
            held[kHeldTheta] = curr_theta;
            pose_ok = !(in_sec(in.now_ns - t2) > in.transform_timeout);
            // getRobotVel (:441-476); the looked-up transforms carry the stamps they were asked for
            double x1, y1, yaw1;
            if (l1.get(&x1, &y1, &yaw1)) {
                const double dt = in_sec(t2 - t1);
                if (!(dt <= 0.0 || dt > in.transform_timeout)) {
                    const double dx = x2 - x1;
                    const double dy = y2 - y1;
                    const double dyaw = near_norm_ang(yaw2 - yaw1);
                    const double mid_yaw = yaw1 + dyaw / 2.0;
                    const double vx_global = dx / dt;
                    const double vy_global = dy / dt;
                    const double cos_yaw = cos(-mid_yaw);
                    const double sin_yaw = sin(-mid_yaw);
                    held[kHeldV] = vx_global * cos_yaw - vy_global * sin_yaw;
                    held[kHeldVn] = vx_global * sin_yaw + vy_global * cos_yaw;
                    held[kHeldW] = dyaw / dt;
                    vel_ok = true;
                }
            }
        }
        valid = in.pose_valid_overwritten ? vel_ok : (pose_ok && vel_ok);  // :549-550
        if (g.tric) {
            const bool ok = !in.steer_ok || in.steer_ok[i];
            if (ok) held[kHeldSteer] = in.steer ? (double)in.steer[i] : 0.0;
            valid = valid && ok;
        }
        for (int r = 0; r < kHeldRows; r++) g.st.held[(size_t)r * cap + i] = held[r];
        if (g.mode_rw && !valid) g.mode_rw[i] = NMPC_NODE_ERROR;
    }
    // the robot's origin, after the recentre when there is one
    double ox = g.fr ? g.fr[i] : 0.0, oy = g.fr ? g.fr[cap + i] : 0.0;
    bool go = false;
    if (isfinite(in.recentre_radius) && g.fr) {
        go = ran && frame_recentre_go(held[kHeldX], held[kHeldY], ox, oy, in.recentre_radius);
        if (go) {
            const double nox = rint(held[kHeldX]), noy = rint(held[kHeldY]);
            frame_move(g.fr, g.st.cap, i, g.xbar, g.N, g.nx, ox, oy, nox, noy);
            ox = nox;
            oy = noy;
        }
    }
    if (in.moved) in.moved[i] = go ? 1 : 0;
    in.valid[i] = valid ? 1 : 0;
    in.pose[i] = (float)(held[kHeldX] - ox);
    in.pose[Bn + i] = (float)(held[kHeldY] - oy);
    in.pose[2 * Bn + i] = (float)held[kHeldTheta];
    in.vel[i] = (float)held[kHeldV];
    in.vel[Bn + i] = (float)held[kHeldVn];
    in.vel[2 * Bn + i] = (float)held[kHeldW];
    in.steer_out[i] = (float)held[kHeldSteer];
    if (g.goal_map && g.goal_out) {
        g.goal_out[i] = (float)(g.goal_map[i] - ox);
        g.goal_out[Bn + i] = (float)(g.goal_map[Bn + i] - oy);
        g.goal_out[2 * Bn + i] = (float)g.goal_map[2 * Bn + i];
    }
}

__global__ void k_cycle_status(int B, const unsigned char* valid, int strict, unsigned char* mode, unsigned char* event,
                               double* remains, const unsigned char* held, const unsigned char* mode_save,
                               const double* remains_save)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    if (held && held[i]) {  // the protective hold parked the robot in IDLE for the gate: the mode it had comes back
        mode[i] = mode_save[i];
        if (remains) remains[i] = remains_save[i];
        if (event) event[i] = NMPC_NODE_EV_HELD;
    }
    if (valid[i]) return;
    if (strict) {
        if (event) event[i] = NMPC_NODE_EV_INPUT_INVALID;
    } else if (mode[i] == NMPC_NODE_GOTO_POSE || mode[i] == NMPC_NODE_FOLLOW_PATH) {
        mode[i] = NMPC_NODE_ERROR;
        if (remains) remains[i] = __builtin_nan("");  // (node_tick_queue: no longer in FollowPath)
    }
}

dim3 grid_of(int n) { return dim3((n + kThreads - 1) / kThreads); }

}  // namespace

hipError_t launch_push_samples(const NodeInputState& st, int B, const long long* stamp_ns, const double* sample,
                               const unsigned char* mask, unsigned char* dropped, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_push_samples, grid_of(B), dim3(kThreads), 0, stream, st, B, stamp_ns, sample, mask, dropped);
    return hipGetLastError();
}

hipError_t launch_node_input(const NodeInputArgs& a, hipStream_t stream)
{
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_node_input, grid_of(a.B), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cycle_status(int B, const unsigned char* valid, int strict, unsigned char* mode, unsigned char* event,
                               double* remains, const unsigned char* held, const unsigned char* mode_save,
                               const double* remains_save, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_cycle_status, grid_of(B), dim3(kThreads), 0, stream, B, valid, strict, mode, event, remains,
                       held, mode_save, remains_save);
    return hipGetLastError();
}

}  // namespace nmpc
