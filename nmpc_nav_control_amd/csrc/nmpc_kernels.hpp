// nmpc_kernels.hpp -- kernel-side interface shared by the HIP kernels and the C-ABI host code.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "nmpc_amd/nmpc_batch.h"
#include "nmpc_amd/nmpc_path.h"
#include "nmpc_models.hpp"

// Internal to the library (acados_shim.cpp -> nmpc_batch.cpp, not part of the public ABI): nmpc_batch_solve_iterate
// for one robot whose I/O block the row-parallel kernel stages itself (KArgs::stage_*): it reads [in_d, in_d + in_n)
// from the host-mapped in_h at its start and writes [out_d, out_d + out_n) to the host-mapped out_h at its end.
// NMPC_ERR_ARG when the launch would not run the row-parallel kernel.
struct nmpc_stage_io {
    const float* in_h;
    float* in_d;
    int in_n;
    float* out_h;
    const float* out_d;
    int out_n;
};
extern "C" int nmpc_batch_solve_iterate_staged(nmpc_batch* b, const float* x0, const float* yref, int ny_in,
                                               const float* We, float* xbar, float* ubar, int* status, int* qp_iter,
                                               float* qp_res, void* stream, const nmpc_stage_io* io);

namespace nmpc {

constexpr float kPi = 3.14159265358979323846f;

enum KernelMode { kModeSolve = 0, kModeRun = 1 };

// Device pointers of one batched launch. Public inputs/outputs are [field][B] (instance-minor);
// the device-resident state (iterate, carried refs, scratch) is [field][stride], stride = capacity.
struct KArgs {
    int B, stride;   // stride: leading dimension of xbar / ubar / carried (the capacity, or the caller's ld)
    int sstride;     // the handle's capacity: row count of the scratch planes (DZ plane, dummy blocks), whatever stride is
    float* xbar;     // [(N+1)*NX][stride]   SQP iterate, warm start of the next tick
    float* ubar;     // [N*NU][stride]
    float* carried;  // [NBX][stride]        ref states carried between ticks (run mode)
    float* scratch;  // per-stage workspace
    // solve mode
    const float* x0;    // [NX][B]
    const float* yref;  // [N+1][ny_in][B]
    int ny_in;
    const float* We;  // [NX][B] or nullptr
    // run mode
    const float* pose;   // [3][B]
    const float* vel;    // [3][B]  {v, vn, w}
    const float* steer;  // [B] or nullptr
    const float* traj;   // [N+1][3][B]
    const int* traj_len; // [B] or nullptr (= N+1)
    const unsigned char* reset;  // [B] or nullptr
    // run mode from parametric paths (nmpc_batch_run_path): getNextNPoses in the kernel instead of traj
    const nmpc_path_segment* segs;  // [B][seg_stride] or nullptr
    int seg_stride, holo;
    const int* nseg;                // [B]
    const double* nearest_u;        // [B]
    double period;
    float* traj_out;                // [N+1][3][B] or nullptr: the poses the march produced
    // Per-robot map frames (robot_tables.hip): the handle's frame table, fp64 [2][sstride], every robot's origin x, then
    // y; nullptr: the table is off and the march's poses stay in map coordinates. Only a launch that marches reads it,
    // and such a launch is given no poses, so the table travels in traj's slot: the launches without a march keep their
    // argument layout, and with it their device code
    void set_origin(const double* o) { traj = reinterpret_cast<const float*>(o); }
    __host__ __device__ const double* origin() const { return reinterpret_cast<const double*>(traj); }
    // outputs (each may be nullptr)
    float* u0;     // [NU][B]
    float* x1;     // [NX][B]
    float* cmd;    // [3][B]
    int* status;   // [B]
    int* qp_iter;  // [B]
    float* qp_res; // [3][B] res_stat, res_ineq, mu at IPM exit
    float* xtraj;  // [(N+1)*NX][B]
    float* utraj;  // [N*NU][B]
    // team placement (schedule.hip): team slot -> instance, or nullptr (slot i = instance i)
    const int* order;
    // node ticks (nmpc_batch_node_tick): device count of the robots that solve, the first *n_active slots of `order`;
    // a team / block whose slot is past it leaves at once. nullptr: every slot below B runs
    const int* n_active;
    int* iter_key;  // [stride] resident: executed IPM iterations of the last solve, or nullptr
    unsigned char* warm;  // [stride] resident: the robot's last solve succeeded and its records hold its multipliers
                          // in the layout tagged (NMPC_WARM_TAG_*), 0 otherwise; nullptr: cold start, nothing written
    int warm_tag;   // this launch's record layout tag: a robot starts warm only if warm[inst] == warm_tag
    int dense;      // the launch has more waves than the device has SIMDs (selects the team kernel variant)
    int rowpar;     // 0: team kernel; W > 0: k_sqp_rti_rowpar with W waves per robot
    int rec_split;  // team kernel, diff: split core / bound record planes (TeamRec::SPLIT_OK; tric always)
    int split;      // one 256-lane block per robot: P0's integrations spread over its 16 rows (4 waves, stage k on
                    // row k mod 16, joined by a block barrier); small batches
    int seg;        // k_sqp_rti_rowpar: horizon segments S (N % S == 0) whose Riccati sweeps run in parallel on S rows,
                    // joined by a master recursion over the segment boundaries; 0: the serial phases B / C
    // one-robot capsule solves (acados_shim.cpp, k_sqp_rti_rowpar only): the kernel copies the capsule's input block
    // from host-mapped memory into the device block at its start and the output block back at its end, in place of a
    // copy launch on each side (stage_in_n / stage_out_n = 0: nothing staged)
    const float* stage_in_h;
    float* stage_in_d;
    int stage_in_n;
    float* stage_out_h;
    const float* stage_out_d;
    int stage_out_n;
    // per-robot bounds and weights (robot_tables.hip): the handle's table [rows][sstride], rows as rp_rows() of the
    // model lays them out; nullptr: the table is off and every robot takes KParams' values. (The row offsets are
    // compile-time values of the model in the kernels, not launch arguments: the team kernel has no scalar registers
    // to spare.)
    const float* rparams;
    // stage-varying bounds (robot_tables.hip): the handle's stage table, every robot's box at every stage of the
    // horizon (sb_at below); nullptr: the table is off and a robot's box is the same at every stage (rparams, else
    // KParams). While it is on, the bound rows of rparams and of KParams reach no launch
    const float* sbounds;
    // per-robot model parameters (robot_tables.hip): the handle's model table [NP][sstride]; nullptr: the table is off
    // and every robot takes KParams::p. While it is on, KParams::p reaches no launch (robot_vals, sqp_steps.hpp)
    const float* rmodel;
    // k_sqp_rti_team_ho (sqp_rti_team_ho.hip): the hand-off iteration C > 0; a team that has not stopped at the top of
    // IPM iteration C leaves the team loop, and a wave of its block finishes the robot in the segmented one-wave form
    // with `seg` segments. 0: every other launch. (The last field: the arguments before it keep their offsets.)
    int handoff;
};

// Rows of the per-robot table, in this order: lbx[NBX] ubx[NBX] lbu[NBU] ubu[NBU] W[NY] W_e[NX]
enum RpField { kRpLbx = 0, kRpUbx, kRpLbu, kRpUbu, kRpW, kRpWe, kRpFields };
struct RpRows {
    int off[kRpFields + 1];  // first row of each field; off[kRpFields] = rows of the table
};
__host__ __device__ constexpr RpRows rp_rows(int nx, int nu, int nbx, int nbu)
{
    const int n[kRpFields] = {nbx, nbx, nbu, nbu, nx + nu, nx};
    RpRows r{};
    r.off[0] = 0;
    for (int f = 0; f < kRpFields; f++) r.off[f + 1] = r.off[f] + n[f];
    return r;
}
constexpr int kRpRowsMax = 48;  // omni4: 4 * 4 + 15 + 11 = 42
// one robot's column of a table (the handle's own values: the fill kernels' argument)
struct RpColumn {
    float v[kRpRowsMax];
};

// The stage table: per stage and robot the rows lbx[NBX] ubx[NBX] lbu[NBU] ubu[NBU], (N + 1) stages, `cap` robots.
// Laid out [stage][robot][row]: one robot's rows of a stage are one cache line (diff, tric 32 B, omni4 64 B), and the
// lanes of a DPP row read consecutive floats. (The per-robot table's orientation, [stage][row][robot], measured level
// and was removed: profiles/r07/ab/stage_bounds.txt)
enum SbField { kSbLbx = 0, kSbUbx, kSbLbu, kSbUbu, kSbFields };
__host__ __device__ constexpr int sb_rows(int nbx, int nbu) { return 2 * nbx + 2 * nbu; }
__host__ __device__ constexpr int sb_off(int field, int nbx, int nbu)
{
    return field == kSbLbx ? 0 : field == kSbUbx ? nbx : field == kSbLbu ? 2 * nbx : 2 * nbx + nbu;
}
// float index of robot i's row `row` at stage k, and the distance from one stage to the next
__host__ __device__ inline size_t sb_at(int k, int row, int i, int cap, int rows)
{
    return ((size_t)k * cap + i) * (size_t)rows + row;
}
__host__ __device__ inline size_t sb_stage_stride(int cap, int rows) { return (size_t)cap * rows; }
// the slots of a box that a speed limit covers (nmpc_model_params_set_limits' v_max): tric's slot 1 is the steering's
__host__ __device__ constexpr int sb_speed_rows(int tric, int nbx) { return tric ? 1 : nbx; }

template <class M>
size_t team_scratch_floats(int N, int stride);
template <class M>
hipError_t launch_sqp_rti_team(const KParams& P, const KArgs& a, int mode, hipStream_t stream);
// small batches: one wave per robot, stage-parallel phases over its four rows (sqp_rti_rowpar.hip)
template <class M>
hipError_t launch_sqp_rti_rowpar(const KParams& P, const KArgs& a, int mode, hipStream_t stream);
template <class M>
size_t rowpar_lds_bytes(int N, int mode, int seg);
// the team kernel with the in-block hand-off (sqp_rti_team_ho.hip; a.handoff > 0, a.seg = kHandoffSeg): diff and tric,
// solve and run mode, unsplit launches with at most one wave per SIMD, wide records, every per-robot table off.
// team_ho_lds_bytes: the LDS of one block (the hand-off list and four resume slices), 0 for a model or horizon it
// does not serve
constexpr int kHandoffSeg = 4;  // one segment per DPP row of the resuming wave
// the hand-off iteration of NMPC_HANDOFF_AUTO (nmpc_batch_set_handoff; a handle is created with 0, off): the best of {10, 12, 14, 16} on the
// metric config, diff N = 40 B = 4096, +5.4 % same-box (profiles/r10/ab/handoff.txt); 0 = off
constexpr int kHandoffDefault = 16;
template <class M>
hipError_t launch_sqp_rti_team_ho(const KParams& P, const KArgs& a, int mode, hipStream_t stream);
template <class M>
size_t team_ho_lds_bytes(int N);
constexpr int kSegMax = 16;  // most horizon segments of the segmented row-parallel kernel
// rmodel: the handle's model table when it is on (the plant then steps each robot with its own column), else nullptr
template <class M>
hipError_t launch_fleet_sim(const KParams& P, int B, int stride, float* path, float* s, float* pose, float* vel,
                            float* steer, const float* u0, const int* status, const float* carried, float* traj,
                            int* traj_len, int advance, const nmpc_fleet_renew* renew, const float* rmodel,
                            hipStream_t stream);
hipError_t launch_team_order(const int* key, int B, int layout, int* sorted, int* order, hipStream_t stream);
// node ticks: the robots with active[i] != 0 first (hardest first by key when `sorted`, else in index order), the
// others behind them; n_active[0] = their count
hipError_t launch_node_order(const int* key, const unsigned char* active, int B, int sorted, int* order, int* n_active,
                             hipStream_t stream);
// the resident state of the first B robots as nmpc_batch_init_iterate leaves it (mode 0 create, 1 reset), warm flags
// cleared; launch_forget_warm clears the warm flags alone, of the robots with mask[i] != 0 (nullptr: all)
hipError_t launch_init_iterate(float* xbar, float* ubar, float* carried, unsigned char* warm, int B, int stride, int N,
                               int nx, int nu, int nbx, int mode, hipStream_t stream);
hipError_t launch_forget_warm(unsigned char* warm, const unsigned char* mask, int B, hipStream_t stream);
// The writers of the per-robot device tables (robot_tables.hip), each one launch; mask: the robots with
// mask[i] != 0 (nullptr: all of the first B).
// Row-major tables [rows][cap] (the per-robot table, the model table): fill: every robot's column = col (the first
// `cap` robots); set: the rows of the non-NULL fields of a list of kFields fields (field f: the rows [off[f],
// off[f + 1]), its source src[f] [n][B]; kRpFields fields for the per-robot table, the one field p for the model
// table); rp_limits: the batched nmpc_model_params_set_limits (each array [B] or nullptr: those rows stay)
hipError_t launch_rows_fill(float* table, int cap, int rows, const RpColumn& col, hipStream_t stream);
template <int kFields>
hipError_t launch_rows_set(float* table, int cap, int B, const int (&off)[kFields + 1],
                           const float* const (&src)[kFields], const unsigned char* mask, hipStream_t stream);
hipError_t launch_rp_limits(float* table, int cap, int B, const RpRows& rr, int tric, const float* v_max,
                            const float* a_max, const float* alpha_min, const float* alpha_max,
                            const float* dalpha_max, const unsigned char* mask, hipStream_t stream);
// The stage table sb, N + 1 stages of `cap` robots. fill: every stage of every robot = the robot's column of the
// per-robot table rp (rows rr, stride cap) when rp is not nullptr, else col's first sb_rows values (lbx ubx lbu ubu of
// the handle). set: the non-NULL fields of s. limits: the per-stage nmpc_model_params_set_limits. shift: stage k =
// stage min(k + n, last)
struct SbDims {
    int N, cap, nbx, nbu;
};
hipError_t launch_sb_fill(float* sb, const SbDims& d, const RpColumn& col, const float* rp, const RpRows& rr,
                          hipStream_t stream);
hipError_t launch_sb_set(float* sb, const SbDims& d, int B, const nmpc_stage_bounds& s, const unsigned char* mask,
                         hipStream_t stream);
hipError_t launch_sb_limits(float* sb, const SbDims& d, int B, int tric, const float* v_max, const float* a_max,
                            const float* alpha_min, const float* alpha_max, const float* dalpha_max,
                            const unsigned char* mask, hipStream_t stream);
hipError_t launch_sb_shift(float* sb, const SbDims& d, int B, int n, const unsigned char* mask, hipStream_t stream);
// The stage table's speed rows from a speed map (speed_map.hip, nmpc_batch_stage_limits_from_map: the rule is stated
// there). Device pointers; the resident arrays have the stride d.cap, the caller's the stride B
struct SpeedMapArgs {
    float* sb;
    SbDims d;
    int B, nx, tric;
    nmpc_speed_map map;
    float slope, v_floor, dt;
    float cap, a;            // the handle's ubx[0] and ubu[0] ...
    const float* rp;         // ... or, while the per-robot table is on, the robot's column: rows rp_ubx and rp_ubu
    int rp_ubx, rp_ubu;
    const float* xbar;       // [(N+1)*nx][d.cap]
    const float* carried;    // [nbx][d.cap]
    const double* origin;    // the frame table [2][d.cap], or nullptr while it is off
    const float* pose;       // [3][B], or nullptr (then reset is nullptr too)
    const unsigned char* reset;  // [B] or nullptr
    const unsigned char* mask;   // [B] or nullptr: all
    const unsigned char* mode;   // [B] or nullptr; the cycle's: only GOTO_POSE and FOLLOW_PATH robots are processed
    float* vlim;             // [N+1][B] or nullptr
    // fleet separation's operand (nmpc_batch_stage_limits_from_tracks), or nullptr: q_k [N+1][d.cap], written by
    // launch_sep_min for the same robots; then map.vmax may be nullptr (no map), and gap [N+1][B] or nullptr is written
    const float* sep_q;
    float sep_gain, sep_clearance;
    float* gap;
};
hipError_t launch_speed_map(const SpeedMapArgs& a, hipStream_t stream);
// Fleet separation (separation.hip; the rule is stated at nmpc_batch_stage_limits_from_tracks). The export of the
// resident horizons into a track buffer xy [K+1][2][M] at the columns first..first+B-1
struct ExportTracksArgs {
    int B, N, nx, cap;
    const float* xbar;           // [(N+1)*nx][cap]
    const double* origin;        // the frame table [2][cap], or nullptr while it is off
    const float* pose;           // [3][B], or nullptr (then reset and mode are nullptr too)
    const unsigned char* reset;  // [B] or nullptr
    const unsigned char* mode;   // [B] or nullptr
    const unsigned char* held;   // [cap] or nullptr: the protective hold's state; a held robot stands, like a reset one
    double* xy;
    int M, K, first;
};
hipError_t launch_export_tracks(const ExportTracksArgs& a, hipStream_t stream);
// q_k, the squared distance from stage k of every processed robot to its nearest counting track (+inf: none), into
// q [N+1][d.cap]: the box prepass over the tracks (boxes [4][M], handle-owned scratch) and the culled minimum
struct SepArgs {
    SbDims d;
    int B, nx;
    const float* xbar;
    const double* origin;
    const float* pose;
    const unsigned char* reset;
    const unsigned char* mask;
    const unsigned char* mode;  // as SpeedMapArgs': the same robots are processed
    const double* xy;           // [K+1][2][M]
    int M, K, own_first, ahead_only;
    float range2;               // range * range, one fp32 product
    double cull2;               // a track whose box is farther than this (squared) from the robot's is skipped
    double* boxes;
    float* q;
    // the guard form (nmpc_batch_stage_limits_from_tracks_ex with a guard; guard == 0: none of these is read). q is
    // then qy, the minimum over the pairs that also have priority[j] >= the robot's own; qa [N+1][d.cap] takes the
    // unfiltered minimum. A robot with held[i] != 0 stands at its pose and keeps the iterate's direction
    int guard;
    const int* priority;         // [M] or nullptr: no filter, qy == qa
    const int* own_priority;     // [B] or nullptr: priority[own_first + i]
    const unsigned char* held;   // [d.cap]
    float* qa;
    float* gap_all;              // [N+1][B] or nullptr: sqrtf(qa_k)
};
hipError_t launch_sep_min(const SepArgs& a, hipStream_t stream);
// The protective hold (k_sep_hold): held' of every robot of [0, B) from the qa plane of the preceding writer call.
// park, the cycle's: mode_rw is then the cycle's mode array; every robot's mode is saved to mode_save [cap] (and its
// remains to remains_save when the queue's remains is given), and a robot with held' != 0 is parked in IDLE for the
// gate. launch_cycle_status brings both back
struct SepHoldArgs {
    int B, N, cap;
    const float* qa;             // [N+1][cap]
    int last;                    // min(hold_stages, N)
    float stop_gap, release_gap;
    int hold;
    const unsigned char* mode;   // [B] or nullptr: every robot is judged
    const unsigned char* reset;  // [B] or nullptr
    unsigned char* held;         // [cap]
    unsigned char* held_out;     // [B] or nullptr
    unsigned char* mode_rw;      // park: [B], else nullptr
    unsigned char* mode_save;    // park: [cap]
    const double* remains;       // park: [B] or nullptr
    double* remains_save;        // park: [cap]
};
hipError_t launch_sep_hold(const SepHoldArgs& a, hipStream_t stream);
// The frame table fr [2][cap] (fp64: every robot's origin x, then y) and the resident iterate's position rows.
// frame_set: the masked robots of the first B take a new origin and the x and y row of every stage of xbar
// ([(N+1)*nx][cap]) becomes (float)((double)x + (o_old - o_new)). The new origin is origin[2][B]; or, with pose_map
// ([>= 2 rows][B]) given instead, rint of the robot's map position where that is finite and farther than radius from
// the old origin in x or y (moved[i] = 1; the others stay, moved[i] = 0; moved [B] or nullptr); or, with neither, zero.
// to_frame / from_frame: arrays [n][c][B], components 0 and 1 of each group (float)(v - origin) / (double)v + origin,
// the others converted; fr may be nullptr (the table is off: origin zero)
hipError_t launch_frame_set(double* fr, int cap, int B, float* xbar, int N, int nx, const double* origin,
                            const double* pose_map, double radius, unsigned char* moved, const unsigned char* mask,
                            hipStream_t stream);
hipError_t launch_to_frame(const double* fr, int cap, int B, int n, int c, const double* map, float* out,
                           hipStream_t stream);
hipError_t launch_from_frame(const double* fr, int cap, int B, int n, int c, const float* in, double* map,
                             hipStream_t stream);
hipError_t launch_path_discretize(int B, const nmpc_path_segment* segs, int seg_stride, const int* nseg,
                                  const double* nearest_u, double period, int num_poses, int holo, float* traj,
                                  double* traj64, hipStream_t stream);
// nearest path point of every robot (path_nearest.hip): lo / hi [B] bounds of the search range, each may be nullptr;
// lo may alias nearest_u (a robot's bound is read before its result is written). origin [2][ostride]: a handle's frame
// table, the pose then being in each robot's frame (the search runs at (double)pose + origin), or nullptr
hipError_t launch_path_nearest(int B, const nmpc_path_segment* segs, int seg_stride, const int* nseg,
                               const float* pose, const double* origin, int ostride, const double* lo,
                               const double* hi, int holo, double* nearest_u, double* near, double* err,
                               hipStream_t stream);
// the path-error check of nmpc_batch_follow_path on err [2][B]: off_path [B] (or nullptr) and the stop command in cmd
// [3][B] (or nullptr) for the robots whose error reaches a threshold whose comparison is on (use_pos / use_ori)
hipError_t launch_path_guard(int B, const double* err, double max_pos, double max_ori, int use_pos, int use_ori,
                             unsigned char* off_path, float* cmd, hipStream_t stream);

// The gate of a node tick (node_gate.hip): per robot the mode switch of NMPCNavControlROS::mainCycle up to the solve
// decision. Device pointers, [field][B]; the nullable ones as in nmpc_batch_node_tick.
struct NodeGateArgs {
    int B, N, nu, seg_stride;
    int holo_err;  // heading of the path orientation error: 1 holonomic (omni4)
    nmpc_node_params np;
    unsigned char* mode;
    const float* pose;
    const float* goal;
    // the handle's frame table [2][ostride], or nullptr while it is off: pose, goal and the reference poses are in each
    // robot's frame, the segments in map coordinates
    const double* origin;
    int ostride;
    const nmpc_path_segment* segs;
    const int* nseg;
    double* path_u;
    unsigned char* event;
    double* err;
    float* traj;            // [N+1][3][B] handle-owned: the reference of every solving robot
    int* traj_len;          // [B]
    unsigned char* active;  // [B] 1: the robot solves this tick
    float* traj_out;
    float *cmd, *u0, *qp_res;
    int *status, *qp_iter;
    // nmpc_batch_node_tick_queue: the robots' windows over their part lists (the kernels' Queue instantiations; nseg
    // is not read then). 0: the plain tick, q unread
    int queue;
    nmpc_path_queue q;
};
hipError_t launch_node_gate(const NodeGateArgs& g, hipStream_t stream);
size_t node_gate_lds_bytes(int N);
// after the tick's solve launch, for the robots with active[i] != 0: reset consumed, a failed solve (status != 0) to
// NMPC_NODE_ERROR (remains, the queue's, to NaN); n_solved[0] = n_active[0]
hipError_t launch_node_finish(int B, const unsigned char* active, const int* status, const int* n_active,
                              unsigned char* mode, unsigned char* event, unsigned char* reset, int* n_solved,
                              double* remains, hipStream_t stream);

// The node's input stage (node_input.hip, nmpc_batch_node_input): the handle's sample rings and held values, all
// instance-minor with stride cap (ring: stamp [depth][cap], sample [depth][3][cap], count / newest [cap]; held [7][cap])
struct NodeInputState {
    int cap, depth;
    long long* stamp;
    double* sample;
    int* count;
    int* newest;
    double* held;
};
hipError_t launch_push_samples(const NodeInputState& st, int B, const long long* stamp_ns, const double* sample,
                               const unsigned char* mask, unsigned char* dropped, hipStream_t stream);
struct NodeInputArgs {
    NodeInputState st;
    int B, tric;
    nmpc_node_input in;         // scalars and the caller's arrays; valid, pose, vel, steer_out resolved (never NULL)
    const unsigned char* mode;  // [B]
    unsigned char* mode_rw;     // the cycle under strict: an invalid robot's mode becomes NMPC_NODE_ERROR; else nullptr
    const double* goal_map;     // [3][B] or nullptr
    float* goal_out;
    double* fr;  // the frame table [2][cap] or nullptr (off: origin zero); written only with a finite recentre_radius
    float* xbar;  // the resident iterate, moved with a robot's origin
    int N, nx;
};
hipError_t launch_node_input(const NodeInputArgs& a, hipStream_t stream);
// the status rule of nmpc_batch_node_cycle after the tick, for the robots with valid[i] == 0: strict: event
// INPUT_INVALID; else a mode that is still GOTO_POSE or FOLLOW_PATH becomes ERROR (remains, the queue's, NaN)
// held [cap] or nullptr (the protective hold, before the rule above): a robot with held[i] != 0 was parked by
// launch_sep_hold; it gets its mode back from mode_save, its remains from remains_save and the event HELD
hipError_t launch_cycle_status(int B, const unsigned char* valid, int strict, unsigned char* mode, unsigned char* event,
                               double* remains, const unsigned char* held, const unsigned char* mode_save,
                               const double* remains_save, hipStream_t stream);

}  // namespace nmpc
