// node_gate.hip -- the gate of nmpc_batch_node_tick (include/nmpc_amd/nmpc_batch.h): per robot the mode switch of
// NMPCNavControlROS::mainCycle (NMPCNavControlROS.cpp:516-538) up to the decision whether the robot solves.
//
// Two launches, each in the thread mapping its work wants:
//   k_node_gate   one 16-lane row per robot, four robots per wave, blocks of 256 (16 robots), like k_path_nearest.
//                 Every row runs the nearest-point search (path_nearest.hpp); rows whose robot is not in FollowPath
//                 run it on an empty path, so the search's cross-lane operations stay outside divergent control flow
//                 and nothing returns early. The row then takes the mode switch as far as it goes without the
//                 discretizer: everything but a FollowPath robot that passed the path guard is decided here, with
//                 its reference (the goal repeated), its mode, event, `active` byte and, when it does not solve, its
//                 zero outputs. A robot that passed the guard is handed on (`active` = kGateMarch).
//   k_node_march  one lane per robot, one wave per block, like k_path_discretize: getNextNPoses of the robots handed
//                 on (path_march.hpp, the 65536-step cap included; the march is serial and data-dependent), the
//                 end-of-trajectory test on the last pose in fp64, and the robot's reference poses or its stop.
//                 Lanes without such a robot leave at once (nothing here crosses lanes).
// The march ran in lane 0 of the 16-lane rows at first (one kernel): 331 us at 4096 robots against 9 + 166 us for
// the nearest and discretize launches, and as much at 1024, i.e. per wave and not by contention; in the
// discretizer's own mapping the march costs what it costs there (DESIGN.md "Node tick").
//
// Both kernels are templates on `Queue`. false is nmpc_batch_node_tick: a robot's list is its active path. true is
// nmpc_batch_node_tick_queue: the robot's records hold its whole path set and the gate keeps the node's window
// over them (active_path_ = parts [head, tail), upcoming_path_ = parts [tail, npart)): it clamps and, for a new set,
// fills the window, searches it, pops the parts behind the robot and extends it (processPathBuffers,
// NMPCNavControlROS.cpp:576-595 and :603-609); the march hops to the next queued part at the end of one (:685-690)
// and writes patch_remains (:374-375). The window is plain scalar work that every lane of a row repeats; its loops
// end before the search starts, so the search's shuffles still run with all 64 lanes.
#include <hip/hip_runtime.h>

#include "nmpc_amd/nmpc_batch.h"
#include "nmpc_amd/nmpc_path.h"
#include "nmpc_kernels.hpp"
#include "path_march.hpp"
#include "path_nearest.hpp"

namespace nmpc {
namespace {

constexpr int kGateBlock = 256;
constexpr unsigned char kGateMarch = 2;  // `active` between the two launches: passed the path guard, not yet decided

// the end-of-trajectory test of processGoToPose / processFollowPath (:636-639, :681-684)
__device__ inline bool gate_arrived(const nmpc_node_params& np, double px, double py, double pth, double rx,
                                    double ry, double rth)
{
    const double dx = px - rx, dy = py - ry;
    const double d = sqrt(dx * dx + dy * dy);
    double ang = near_norm_ang(pth - rth);
    ang = np.final_ori_signed ? ang : fabs(ang);
    return d <= np.final_pos_err && ang <= np.final_ori_err;
}

// the zero outputs of a robot that does not solve
__device__ inline void gate_stop(const NodeGateArgs& g, size_t i)
{
    const size_t Bn = (size_t)g.B;
    if (g.cmd)
        for (int c = 0; c < 3; c++) g.cmd[(size_t)c * Bn + i] = 0.0f;
    if (g.u0)
        for (int c = 0; c < g.nu; c++) g.u0[(size_t)c * Bn + i] = 0.0f;
    if (g.qp_res)
        for (int c = 0; c < 3; c++) g.qp_res[(size_t)c * Bn + i] = 0.0f;
    if (g.status) g.status[i] = 0;
    if (g.qp_iter) g.qp_iter[i] = 0;
}

// step 1 of nmpc_batch_node_tick_queue: the window of robot i, never past its own records
__device__ inline void queue_window(const NodeGateArgs& g, size_t i, int* nP, int* h, int* t)
{
    int n = g.q.npart[i];
    n = n > g.seg_stride ? g.seg_stride : n;
    n = n < 0 ? 0 : n;
    int a = g.q.head[i];
    a = a < 0 ? 0 : (a > n ? n : a);
    int b = g.q.tail[i];
    b = b < a ? a : (b > n ? n : b);
    *nP = n;
    *h = a;
    *t = b;
}

// processPathBuffers(U) (:576-595) on the window [h, t) of the parts S[0 .. nP) (S: the robot's first record, `base`
// its index into frame / length): the new t. At most nP - t trips.
__device__ inline int queue_fill(const NodeGateArgs& g, const nmpc_path_segment* S, size_t base, int h, int t, int nP,
                                 double U)
{
#pragma clang fp contract(off)
    const double* len = g.q.length ? g.q.length + base : nullptr;
    const int* frame = g.q.frame ? g.q.frame + base : nullptr;
    double L = 0.0;
    for (int k = h; k < t; k++) {
        const double l = len ? len[k] : g.q.part_length;
        L += (k == h) ? l * (1.0 - U) : l;  // :580-581
    }
    for (int it = 0; it < g.seg_stride && L < g.q.max_active_len && t < nP; it++) {  // :584
        if (t > h) {
            if (S[t - 1].v * S[t].v < 0.0) break;          // :588
            if (frame && frame[t - 1] != frame[t]) break;  // :589
        }
        t++;
        L += len ? len[t - 1] : g.q.part_length;  // :593
    }
    return t;
}

// patch_remains (:374-375) of a robot that stays in FollowPath
__device__ inline double queue_remains(int nP, int h, double path_u)
{
    const double r = (double)(nP - h);
    return r > 0.0 ? r - path_u : r;
}

template <bool Queue>
__global__ void __launch_bounds__(kGateBlock) k_node_gate(NodeGateArgs g)
{
    const size_t t = (size_t)blockIdx.x * kGateBlock + threadIdx.x;
    const size_t i = t >> 4;
    const int j = (int)(t & 15);
    const int N = g.N;
    const size_t Bn = (size_t)g.B;
    const bool live = i < Bn;
    const double nan = __builtin_nan("");
    const nmpc_node_params& np = g.np;

    int m = live ? (int)g.mode[i] : NMPC_NODE_IDLE;
    m = m > NMPC_NODE_ERROR ? NMPC_NODE_ERROR : m;
    // a mode whose inputs are missing: Error, nothing published
    if (m == NMPC_NODE_GOTO_POSE && !g.goal) m = NMPC_NODE_ERROR;
    if (m == NMPC_NODE_FOLLOW_PATH && !(g.segs && (Queue || g.nseg) && g.path_u)) m = NMPC_NODE_ERROR;
    const bool follow = m == NMPC_NODE_FOLLOW_PATH;
    double px = 0.0, py = 0.0, pth = 0.0;
    double mx = 0.0, my = 0.0;  // the robot in map coordinates, where its path is (px, py: in its frame, as its goal)
    if (live) {
        px = mx = (double)g.pose[i];
        py = my = (double)g.pose[Bn + i];
        pth = (double)g.pose[2 * Bn + i];
        if (g.origin) {
            mx += g.origin[i];
            my += g.origin[(size_t)g.ostride + i];
        }
    }
    const nmpc_path_segment* S = g.segs + (follow ? i * (size_t)g.seg_stride : 0);
    int n;
    int nP = 0, qh = 0, qt = 0;  // (Queue) the robot's part count and its window [qh, qt)
    if constexpr (Queue) {
        if (follow) {
            queue_window(g, i, &nP, &qh, &qt);
            if (qt == qh) qt = queue_fill(g, S, i * (size_t)g.seg_stride, qh, qt, nP, 0.0);  // a new set (:573)
        }
        n = qt - qh;
        S += qh;
    } else {
        n = follow ? g.nseg[i] : 0;
        n = n > g.seg_stride ? g.seg_stride : n;  // never past the robot's own records
        n = n < 1 ? 0 : n;
    }
    // (the rows of a wave are together again here: the search's shuffles need all 64 lanes)
    const double lo_in = n >= 1 ? g.path_u[i] : nan;
    NearResult R = near_search(S, n, j, mx, my, pth, lo_in, nan, g.holo_err);
    // (no cross-lane operation below; every decision is the same in the 16 lanes of a row)
    if constexpr (Queue) {
        if (n >= 1) {
            const int k = (int)floor(R.U);  // 0 <= U <= n
            if (n > k) {                    // the parts behind the robot (:603-609); U - k is exact
                qh += k;
                R.U -= (double)k;
            } else if (!g.holo_err) {
                // U == n: nothing is popped and the front part is the window's first, whose sign decides the pi
                // of :655 (near_search took the last part's)
                const double head = (S[0].v < 0.0) ? R.near[2] + M_PI : R.near[2];
                R.err[1] = (R.err[0] != R.err[0]) ? nan : fabs(near_norm_ang(head - pth));
            }
            qt = queue_fill(g, g.segs + i * (size_t)g.seg_stride, i * (size_t)g.seg_stride, qh, qt, nP, R.U);  // :652
        }
    }

    int mode_out = m, ev = NMPC_NODE_EV_NONE;
    bool solve = false, march = false;
    double gx = 0.0, gy = 0.0, gth = 0.0;
    if (m == NMPC_NODE_BREAK) {
        mode_out = NMPC_NODE_IDLE;
        ev = NMPC_NODE_EV_BREAK;
    } else if (m == NMPC_NODE_GOTO_POSE) {
        gx = (double)g.goal[i];
        gy = (double)g.goal[Bn + i];
        gth = (double)g.goal[2 * Bn + i];
        const double dx = gx - px, dy = gy - py;
        const double d = sqrt(dx * dx + dy * dy);
        if (np.enable_safe_conditions && d >= np.max_goal_dist) {
            mode_out = NMPC_NODE_IDLE;
            ev = NMPC_NODE_EV_GOAL_TOO_FAR;
        } else if (gate_arrived(np, px, py, pth, gx, gy, gth)) {
            mode_out = NMPC_NODE_IDLE;
            ev = NMPC_NODE_EV_ARRIVED;
        } else {
            solve = true;
            ev = NMPC_NODE_EV_SOLVED;  // (the finish kernel turns a failed solve into SOLVE_FAILED)
        }
    } else if (follow) {
        if (n < 1) {
            mode_out = NMPC_NODE_IDLE;  // executeNMPC's empty list
        } else if (np.enable_safe_conditions && (R.err[0] >= np.max_pos_err || R.err[1] >= np.max_ori_err)) {
            mode_out = NMPC_NODE_ERROR;  // (a threshold of +inf or NaN never compares true)
            ev = NMPC_NODE_EV_OFF_PATH;
        } else {
            march = true;  // k_node_march decides
        }
    }
    if (!live) return;

    // the reference poses: the handle's copy for the solve launch, the caller's (NaN where the robot does not solve)
    if (!march) {
        for (int q = j; q <= N; q += 16) {
            const size_t o = (size_t)q * 3 * Bn + i;
            if (solve) {
                g.traj[o] = (float)gx;
                g.traj[o + Bn] = (float)gy;
                g.traj[o + 2 * Bn] = (float)gth;
            }
            if (g.traj_out) {
                g.traj_out[o] = solve ? (float)gx : __builtin_nanf("");
                g.traj_out[o + Bn] = solve ? (float)gy : __builtin_nanf("");
                g.traj_out[o + 2 * Bn] = solve ? (float)gth : __builtin_nanf("");
            }
        }
    }
    if (j == 0) {
        g.mode[i] = (unsigned char)mode_out;
        if (g.event) g.event[i] = (unsigned char)ev;
        const bool searched = follow && n >= 1;
        if (searched) g.path_u[i] = R.U;
        if constexpr (Queue) {
            if (follow && nP >= 1) {
                g.q.head[i] = qh;
                g.q.tail[i] = qt;
            }
            // every robot the gate decides is out of FollowPath; the march writes the others'
            if (g.q.remains && !march) g.q.remains[i] = nan;
        }
        if (g.err) {
            g.err[i] = searched ? R.err[0] : nan;
            g.err[Bn + i] = searched ? R.err[1] : nan;
        }
        g.active[i] = march ? kGateMarch : (solve ? 1 : 0);
        g.traj_len[i] = march ? N + 1 : 1;
        if (!solve && !march) gate_stop(g, i);
    }
}

template <bool Queue>
__global__ void __launch_bounds__(64) k_node_march(NodeGateArgs g)
{
    extern __shared__ double s_emit[];  // [N+1][blockDim.x]: path parameter of every emitted pose
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.B || g.active[i] != kGateMarch) return;
    const int N = g.N;
    const size_t Bn = (size_t)g.B;
    const nmpc_node_params& np = g.np;
    double* emit_u = s_emit + threadIdx.x;
    const int es = blockDim.x;
    const nmpc_path_segment* S = g.segs + (size_t)i * g.seg_stride;
    int n;
    int nP = 0, qh = 0, qt = 0;
    if constexpr (Queue) {
        queue_window(g, (size_t)i, &nP, &qh, &qt);  // the gate's window (already clamped)
        n = qt - qh;
        S += qh;
    } else {
        n = g.nseg[i];
        n = n > g.seg_stride ? g.seg_stride : n;
    }
    const int count = path_march(S, n, g.path_u[i], np.sample_period, N + 1,
                                 [&](int q, double u) { emit_u[q * es] = u; });
    // the end test against the last pose (the path end when the march stopped short: the padding of :58-63)
    // (the robot and the last pose both in map coordinates; the reference poses leave in the robot's frame)
    const double ox = g.origin ? g.origin[i] : 0.0, oy = g.origin ? g.origin[(size_t)g.ostride + i] : 0.0;
    const double pth = (double)g.pose[2 * Bn + i];
    double px = (double)g.pose[i], py = (double)g.pose[Bn + i];
    if (g.origin) {
        px += ox;
        py += oy;
    }
    double lx, ly, lth;
    path_pose(S, n, (N < count) ? emit_u[N * es] : (double)n, np.is_holonomic, &lx, &ly, &lth);
    const bool solve = !gate_arrived(np, px, py, pth, lx, ly, lth);
    const bool hop = Queue && !solve && qt < nP;  // the end of a part with parts still queued (:686-690)
    for (int q = 0; q <= N; q++) {
        const size_t o = (size_t)q * 3 * Bn + i;
        if (solve) {
            double x, y, th;
            path_pose(S, n, (q < count) ? emit_u[q * es] : (double)n, np.is_holonomic, &x, &y, &th);
            const float fx = (float)(x - ox), fy = (float)(y - oy);
            g.traj[o] = fx;
            g.traj[o + Bn] = fy;
            g.traj[o + 2 * Bn] = (float)th;
            if (g.traj_out) {
                g.traj_out[o] = fx;
                g.traj_out[o + Bn] = fy;
                g.traj_out[o + 2 * Bn] = (float)th;
            }
        } else if (g.traj_out) {
            g.traj_out[o] = g.traj_out[o + Bn] = g.traj_out[o + 2 * Bn] = __builtin_nanf("");
        }
    }
    g.active[i] = solve ? 1 : 0;
    if (solve) {
        if (g.event) g.event[i] = NMPC_NODE_EV_SOLVED;  // (the finish kernel turns a failed solve into SOLVE_FAILED)
    } else if (hop) {
        // pop_front, then the upcoming front joins without a sign or frame test (:687-689); the mode stays
        qh += 1;
        g.q.head[i] = qh;
        g.q.tail[i] = qt + 1;
        g.path_u[i] = 0.0;
        if (g.event) g.event[i] = NMPC_NODE_EV_NEXT_PART;
        gate_stop(g, (size_t)i);
    } else {
        g.mode[i] = NMPC_NODE_IDLE;
        if (g.event) g.event[i] = NMPC_NODE_EV_ARRIVED;
        gate_stop(g, (size_t)i);
    }
    if constexpr (Queue) {
        if (g.q.remains)
            g.q.remains[i] = (solve || hop) ? queue_remains(nP, qh, g.path_u[i]) : __builtin_nan("");
    }
}

// lanes per block of the march: one wave, narrower when the emitted parameters of 64 robots would not fit 64 KiB
inline int march_block(int N)
{
    int block = 64;
    while (block > 1 && (size_t)block * (size_t)(N + 1) * sizeof(double) > 65536) block /= 2;
    return block;
}

// after a node tick's solve launch: a robot that solved has consumed its pending reset, and a failed solve sends it
// to Error (NMPCNavControlROS.cpp:716-719); n_solved receives the active count
__global__ void k_node_finish(int B, const unsigned char* active, const int* status, const int* n_active,
                              unsigned char* mode, unsigned char* event, unsigned char* reset, int* n_solved,
                              double* remains)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && n_solved) n_solved[0] = n_active[0];
    if (i >= B || !active[i]) return;
    if (reset) reset[i] = 0;
    if (status[i] != 0) {
        mode[i] = NMPC_NODE_ERROR;
        if (event) event[i] = NMPC_NODE_EV_SOLVE_FAILED;
        if (remains) remains[i] = __builtin_nan("");  // (node_tick_queue: no longer in FollowPath)
    }
}

}  // namespace

hipError_t launch_node_finish(int B, const unsigned char* active, const int* status, const int* n_active,
                              unsigned char* mode, unsigned char* event, unsigned char* reset, int* n_solved,
                              double* remains, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_node_finish, dim3((B + kGateBlock - 1) / kGateBlock), dim3(kGateBlock), 0, stream, B, active,
                       status, n_active, mode, event, reset, n_solved, remains);
    return hipGetLastError();
}

size_t node_gate_lds_bytes(int N)
{
    return (size_t)march_block(N) * (size_t)(N + 1) * sizeof(double);
}

hipError_t launch_node_gate(const NodeGateArgs& g, hipStream_t stream)
{
    if (g.B <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((size_t)g.B * 16 + kGateBlock - 1) / kGateBlock);
    if (g.queue)
        hipLaunchKernelGGL(k_node_gate<true>, dim3(blocks), dim3(kGateBlock), 0, stream, g);
    else
        hipLaunchKernelGGL(k_node_gate<false>, dim3(blocks), dim3(kGateBlock), 0, stream, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !(g.segs && (g.queue || g.nseg) && g.path_u)) return e;  // (without paths no robot marches)
    const int block = march_block(g.N);
    const size_t lds = node_gate_lds_bytes(g.N);
    if (lds > 65536) return hipErrorInvalidValue;
    if (g.queue)
        hipLaunchKernelGGL(k_node_march<true>, dim3((g.B + block - 1) / block), dim3(block), lds, stream, g);
    else
        hipLaunchKernelGGL(k_node_march<false>, dim3((g.B + block - 1) / block), dim3(block), lds, stream, g);
    return hipGetLastError();
}

}  // namespace nmpc
