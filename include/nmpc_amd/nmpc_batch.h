/*
 * nmpc_batch.h -- batched MI355X SQP-RTI solve path (libnmpc_amd.so), C ABI.
 *
 * The batched entry points behind which thousands of NMPCNavControl*::run() calls of the reference
 * (src/nmpc_nav_control/NMPCNavControl{Diff,Omni4,Tric}.cpp:82/91/88) execute as one device launch.
 * The per-robot acados-compatible ABI ({name}_acados_*, ocp_nlp_*) lives in acados_solver_{name}.h
 * and acados_c/ocp_nlp_interface.h and is implemented on top of these functions.
 *
 * Conventions
 *   - All array arguments of nmpc_batch_solve / nmpc_batch_run are DEVICE pointers (hipMalloc or torch
 *     CUDA tensors), fp32, instance-minor "[field][B]" layout so that lane i of a wave reads element i.
 *   - `stream` is a hipStream_t (NULL = default stream). Calls are asynchronous on that stream.
 *   - Return value: 0 on success, < 0 on an API error (see nmpc_last_error()). Per-instance solver
 *     status codes follow acados (0 success, 1 NaN detected, 4 QP failure) and are written to `status`.
 *   - Array outputs may be NULL when not wanted.
 */
#ifndef NMPC_AMD_NMPC_BATCH_H
#define NMPC_AMD_NMPC_BATCH_H

#include "nmpc_amd/nmpc_path.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NMPC_MODEL_DIFF2AMR 0
#define NMPC_MODEL_OMNI4AMR 1
#define NMPC_MODEL_TRIC3AMR 2

#define NMPC_OK 0
#define NMPC_ERR_ARG (-1)
#define NMPC_ERR_HIP (-2)
#define NMPC_ERR_UNSUPPORTED (-3)

/* Model + OCP + solver configuration. Mirrors the two parameter surfaces of the reference:
 *   codegen yaml  config/nmpc_nav_control_acados_models.yaml  (N, dt = 1/freq; bakes the model)
 *   ROS yaml      config/nmpc_nav_control.yaml                (dt_ctrl = 1/control_freq, p, bounds, W) */
typedef struct nmpc_model_params {
    int model; /* NMPC_MODEL_* */
    int N;     /* horizon (common.py:6: N = ceil(tf_ini / dt)) */
    double dt;      /* solver time step */
    double dt_ctrl; /* wrapper time step used for vel_ref integration (NMPCNavControlDiff.cpp:155-157) */
    double p[3];    /* diff {b, tau_v}; omni4 {l1+l2, tau_v}; tric {d, tau_v, tau_a} */
    double lbx[4], ubx[4]; /* bounds of the ref states idxbx (stages 1..N) */
    double lbu[4], ubu[4]; /* bounds of the inputs idxbu (stages 0..N-1) */
    double W[15];   /* stage weight diagonal [Q_diag; R_diag] (NY entries) */
    double W_e[11]; /* terminal weight diagonal (NX entries); constructors set it to Q_diag */
    int terminal_hack; /* diff run(): x100 terminal pose weight when yref[N]==yref[N-1] (default 1 for diff) */
    int tric_sin_bug;  /* tric_amr_model.py:45 cos_alpha = sin(alpha) (default 1: reproduce) */
    int qp_iter_max;   /* 50 */
    double qp_tol_stat, qp_tol_ineq, qp_tol_comp; /* fp32 stopping rule, see DESIGN.md */
    double qp_mu0, qp_thr0, qp_tau;              /* IPM initial point and fraction-to-boundary */
    /* IPM direction rule: NMPC_IPM_SINGLE (default) one Newton direction per iteration with the centring
     * sigma = clamp((1 - alpha_prev)^2, qp_sigma_lo, qp_sigma_hi); NMPC_IPM_MEHROTRA predictor-corrector (the
     * fp64 oracle's rule). Both solve the same QP to the same stopping rule (DESIGN.md "Algorithm"). */
    int qp_ipm;
    double qp_sigma_lo, qp_sigma_hi; /* 0.01, 0.5 */
    /* IPM warm start (default 1): a robot whose previous solve on this handle succeeded starts its bound
     * multipliers at max(lambda_previous, qp_warm_kappa / t) instead of qp_mu0 / t (the QP solution is the same;
     * the IPM path is shorter, so qp_iter counts are not acados'). This departs from the reference, whose
     * generated HPIPM never sets qp_solver_warm_start (every QP there starts cold); 0 restores that. Reset robots,
     * nmpc_batch_init_iterate and nmpc_batch_forget_warm start cold. The multipliers live in the handle's slot i
     * of instance i: keep an instance's slot stable across calls (nmpc_batch_solve_iterate included) or clear it
     * with nmpc_batch_forget_warm. The capsule ABI warm-starts a capsule only while it still owns its engine slot
     * (its last solve there succeeded and no reset / create came in between), with kappa 0.01. */
    int qp_warm_start;
    double qp_warm_kappa; /* diff 0.2, omni4 / tric 0.01 */
    /* Warm-start only after a solve that converged within this many IPM iterations (default 12; 0 = qp_iter_max).
     * A robot whose QP was hard last tick starts its next IPM cold: warm-started multipliers speed up the easy
     * majority but lengthen exactly the hard QPs that set the launch time (DESIGN.md "Algorithm and precision"). */
    int qp_warm_iter_max;
    /* Early infeasibility exit (status 4): the IPM stops once its largest bound multiplier exceeds
     * qp_infeas_lambda * max(1, w_max / 10) (w_max: the largest stage or terminal weight of the robot, terminal
     * hack included) while the bound residual stays above 1e-3. HPIPM has no such test (a hard QP runs to
     * qp_iter_max, which acados' RTI accepts), so 0 switches it off; the batched default is 1e5, the capsule ABI
     * default 0 (acados semantics). */
    double qp_infeas_lambda;
} nmpc_model_params;

enum { NMPC_IPM_MEHROTRA = 0, NMPC_IPM_SINGLE = 1 };

typedef struct nmpc_batch nmpc_batch;

/* Dimensions of a model: nx, nu, ny (=nx+nu), nbx, nbu, np. Any pointer may be NULL. */
int nmpc_model_dims(int model, int* nx, int* nu, int* ny, int* nbx, int* nbu, int* np);
/* Defaults = the reference's shipped runtime configuration. */
int nmpc_model_params_default(int model, int N, nmpc_model_params* prm);
/* Bounds from the wrapper-constructor scalars (NMPCNavControlDiff.cpp:18-22, NMPCNavControlOmni4.cpp:18-22,
 * NMPCNavControlTric.cpp:18-29): ref states in [-v_max, v_max] (tric alpha_ref in [alpha_min, alpha_max]),
 * inputs in [-a_max, a_max] (tric dalpha_ref in [-dalpha_max, dalpha_max]); angles in radians. */
int nmpc_model_params_set_limits(nmpc_model_params* prm, double v_max, double a_max, double alpha_min,
                                 double alpha_max, double dalpha_max);

/* Create a batch engine for up to `capacity` instances on the current HIP device. The iterate is
 * initialised with {name}_acados_create semantics (x = [0,0,pi,0,...], u = 0) and carried refs = 0. */
int nmpc_batch_create(const nmpc_model_params* prm, int capacity, nmpc_batch** out);
int nmpc_batch_destroy(nmpc_batch* b);
/* Replace weights / bounds / parameters / QP options (model and N must not change). While the per-robot table is
 * on (nmpc_batch_set_robot_params below), lbx, ubx, lbu, ubu, W and W_e do not reach a launch; while the stage table
 * is on (nmpc_batch_set_stage_bounds below), the four bound fields do not; while the model table is on
 * (nmpc_batch_set_robot_model below), p does not. */
int nmpc_batch_set_params(nmpc_batch* b, const nmpc_model_params* prm);
int nmpc_batch_get_params(const nmpc_batch* b, nmpc_model_params* prm);
/* Re-initialise instances [0, B): mode 0 = create semantics (x = [0,0,pi,0,...], u = 0, carried ref states 0);
 * mode 1 = reset semantics ({name}_acados_reset: iterate zeroed, the carried ref states kept, like the
 * per-robot `reset` mask of nmpc_batch_solve / nmpc_batch_run). */
int nmpc_batch_init_iterate(nmpc_batch* b, int B, int mode, void* stream);

/* One SQP-RTI iteration ({name}_acados_solve) for instances [0, B) on caller-packed QP data:
 *   x0    [NX][B]          initial state (stage-0 lbx = ubx)
 *   yref  [N+1][ny_in][B]  stage references; entries j >= ny_in are 0 (ny_in = 3 pose-only or NY);
 *                          stage N uses entries 0..NX-1
 *   We    [NX][B] or NULL  per-instance terminal weight diagonal (NULL: params W_e)
 *   reset [B] or NULL      nonzero: zero the iterate before solving ({name}_acados_reset)
 * outputs: u0 [NU][B], x1 [NX][B], xtraj [(N+1)*NX][B], utraj [N*NU][B], status [B], qp_iter [B],
 *          qp_res [3][B] = {max |stationarity residual|, max |bound residual|, mu} at IPM exit. */
int nmpc_batch_solve(nmpc_batch* b, int B, const float* x0, const float* yref, int ny_in, const float* We,
                     const unsigned char* reset, float* u0, float* x1, float* xtraj, float* utraj, int* status,
                     int* qp_iter, float* qp_res, void* stream);

/* nmpc_batch_solve with the iterate held by the caller instead of the handle: xbar [(N+1)*NX][ld] and
 * ubar [N*NU][ld] (device) are read as the linearisation point and overwritten with the new iterate (a failed solve
 * keeps its own). Used by the capsule ABI, whose iterate travels with each call; the warm-start records are still
 * the handle's (slot i = instance i). */
int nmpc_batch_solve_iterate(nmpc_batch* b, int B, const float* x0, const float* yref, int ny_in, const float* We,
                             const unsigned char* reset, float* xbar, float* ubar, int ld, int* status, int* qp_iter,
                             float* qp_res, void* stream);

/* Batched NMPCNavControl*::run(): pre-solve + SQP-RTI + post-solve for B robots.
 *   pose  [3][B] {x, y, theta}; vel [3][B] {v, vn, w}; steer [B] (tric; NULL = 0)
 *   traj  [N+1][3][B] reference poses; traj_len [B] poses valid per robot (NULL = N+1; padded with the
 *         last valid pose, NMPCNavControlDiff.cpp:113-117)
 * outputs: cmd [3][B] (diff {v, w, 0}, omni4 {v, vn, w}, tric {v, alpha, 0}), u0 [NU][B], status, qp_iter,
 * qp_res [3][B] (as nmpc_batch_solve). The carried vel-ref states are kept on the device between calls
 * (NMPCNavControlDiff.cpp:168-172). A robot whose solve fails (status != 0) gets a zero (stop) cmd, keeps its
 * carried refs and its iterate: the reference throws there and the node publishes a stop command
 * (NMPCNavControl.cpp:14-23, NMPCNavControlROS.cpp:716-719). Failures stay on their robot: a NaN robot exits
 * its IPM at the first iteration and no other robot's arithmetic depends on it.
 * The unwrap decision (|delta| > pi) and the terminal-weight hack's equality test are taken in fp32 on the fp32
 * inputs. A heading step within one fp32 ulp of pi may therefore unwrap the other way than the fp64 reference would
 * (e.g. from pose theta = 0 to a reference theta = (float)pi), and two references that differ by less than an fp32
 * ulp at magnitude 2 pi may compare equal after the unwrap; both outcomes are valid headings.
 * x and y are absolute fp32 map coordinates throughout: the 1e-3 parity with the fp64 reference is measured up to
 * 64 m from the map origin; beyond that the first solve of a robot and every solve after a reset lose accuracy in
 * proportion to the distance (u0 within 1e-2 at 4096 m, status 0 throughout), warm solves do not (DESIGN.md
 * "Coordinate range"). A per-robot map frame (nmpc_batch_set_robot_frame below) removes the limit: the fp32 positions
 * are then relative to an origin near the robot and the 1e-3 parity holds at any distance from the map origin. */
int nmpc_batch_run(nmpc_batch* b, int B, const float* pose, const float* vel, const float* steer,
                   const float* traj, const int* traj_len, const unsigned char* reset, float* cmd, float* u0,
                   int* status, int* qp_iter, float* qp_res, void* stream);

/* A path-following tick in one launch: PathDiscretizer::getNextNPoses (nmpc_path.h, PathDiscretizer.cpp:14-63)
 * of every robot followed by nmpc_batch_run on those N+1 poses -- processFollowPath's discretize + run
 * (NMPCNavControlROS.cpp:666-668 -> :713) without the trip of the poses through a second launch. The march
 * runs in the solve kernel (fp64, the reference's operation order: the same poses as nmpc_path_discretize
 * with num_poses = N+1, bit for bit). Arguments as nmpc_path_discretize and nmpc_batch_run; traj_out
 * [N+1][3][B] receives the poses (NULL: not written). Every robot's reference has N+1 poses (padded with the
 * path end). nseg [B] >= 1. */
int nmpc_batch_run_path(nmpc_batch* b, int B, const float* pose, const float* vel, const float* steer,
                        const nmpc_path_segment* segs, int seg_stride, const int* nseg, const double* nearest_u,
                        double sample_period, int is_holonomic, const unsigned char* reset, float* traj_out,
                        float* cmd, float* u0, int* status, int* qp_iter, float* qp_res, void* stream);

/* The whole FollowPath tick (NMPCNavControlROS.cpp:648-698 -> :713) from the measured pose to the command:
 * nmpc_path_nearest (nmpc_path.h: processNearestPoint and the path errors, :650-657), then nmpc_batch_run_path
 * from that parameter, then the path-error check (:658-664). Three launches on `stream`, no host synchronisation.
 *   path_u   [B] in: lower bound of the nearest-point search, the robot's progress so far (0 on a new path; the
 *            node pops the segments behind the robot, :603-609, so its search never goes back either);
 *            out: nearest_u, which is also next tick's bound
 *   max_pos_err, max_ori_err  max_pos_error_to_path_ / max_ori_error_to_path_; a robot with pos_err >= max_pos_err
 *            or ori_err >= max_ori_err (:658-659) is off its path: off_path[i] = 1 and cmd[:, i] = 0, the stop
 *            command of :660. +inf or NaN switches a comparison off (enable_safe_conditions_ = false: both)
 *   err      [2][B] {pos_error_to_path, ori_error_to_path} or NULL; the heading of the orientation error is the
 *            holonomic one when the handle's model is omni4 (:654), whatever is_holonomic says: that flag is the
 *            discretizer's, and the node passes false there for every model (:666)
 *   off_path [B] or NULL
 * Everything else as nmpc_batch_run_path. One departure from the node: it skips the solve of an off-path robot
 * (:663); here that robot's solve still runs (its iterate and carried refs advance) and only its command is
 * stopped. The node then waits for a new goal, which resets the controller anyway: pass reset[i] = 1 with it.
 * (nmpc_batch_node_tick below does skip that solve.)
 * sample_period must be finite here. */
int nmpc_batch_follow_path(nmpc_batch* b, int B, const float* pose, const float* vel, const float* steer,
                           const nmpc_path_segment* segs, int seg_stride, const int* nseg, double* path_u,
                           double sample_period, int is_holonomic, double max_pos_err, double max_ori_err,
                           const unsigned char* reset, double* err, unsigned char* off_path, float* traj_out,
                           float* cmd, float* u0, int* status, int* qp_iter, float* qp_res, void* stream);

/* The node's control cycle (NMPCNavControlROS::mainCycle, NMPCNavControlROS.cpp:516-538) for B robots, each in its
 * own state, in one call: the gate (two small launches) decides per robot what the node would do this tick, the robots that
 * solve are compacted on the device, and the solve launch works for them alone. No host synchronisation; everything is
 * queued on `stream`. */
#define NMPC_NODE_IDLE 0
#define NMPC_NODE_GOTO_POSE 1
#define NMPC_NODE_FOLLOW_PATH 2
#define NMPC_NODE_BREAK 3
#define NMPC_NODE_ERROR 4

#define NMPC_NODE_EV_NONE 0          /* Idle / Error: the node publishes nothing */
#define NMPC_NODE_EV_SOLVED 1        /* executeNMPC ran and succeeded: cmd is the command */
#define NMPC_NODE_EV_ARRIVED 2       /* end of trajectory (:636-643, :681-694): stop command, -> Idle */
#define NMPC_NODE_EV_GOAL_TOO_FAR 3  /* :622-627: stop command, -> Idle */
#define NMPC_NODE_EV_OFF_PATH 4      /* :658-664: stop command, -> Error */
#define NMPC_NODE_EV_SOLVE_FAILED 5  /* status != 0 (:716-719): zero cmd, -> Error */
#define NMPC_NODE_EV_BREAK 6         /* processBreak :612-616: stop command, -> Idle */

typedef struct nmpc_node_params {
    double final_pos_err, final_ori_err; /* m, rad: final_position_error / final_orientation_error
                                          * (nmpc_nav_control.yaml:7-8; the yaml is in degrees) */
    double max_goal_dist;                /* m: max_goal_pose_dist (:11) */
    double max_pos_err, max_ori_err;     /* m, rad: max_pos_error_to_path / max_ori_error_to_path (:12-13) */
    int enable_safe_conditions;          /* :10; 0 switches the goal-distance and the path-error guard off */
    /* 1 (default): the end-of-trajectory test compares the signed ang = normAngRad(pose.theta - ref.theta) with
     * final_ori_err, exactly as NMPCNavControlROS.cpp:638-639 / :683-684 write it (so any negative heading error
     * counts as arrived); 0: |ang|. */
    int final_ori_signed;
    double sample_period; /* PathDiscretizer arguments, as nmpc_batch_run_path (the node: getDeltaTime(), false) */
    int is_holonomic;
} nmpc_node_params;
/* The shipped nmpc_nav_control.yaml (0.01 m, 1 deg, 2 m, 0.5 m, 60 deg, safe conditions on), degrees converted to
 * radians; final_ori_signed 1, sample_period 1/40 s (the codegen yaml's dt), is_holonomic 0. */
int nmpc_node_params_default(nmpc_node_params* np);

/* One tick of the node for robots [0, B). Arrays are device pointers, [field][B]:
 *   mode     [B] in/out NMPC_NODE_*; a value above 4 is read as Error (and written back as NMPC_NODE_ERROR)
 *   pose, vel, steer  as nmpc_batch_run
 *   goal     [3][B] {x, y, theta}, read for GOTO_POSE robots; NULL when no robot is in GOTO_POSE
 *   segs, seg_stride, nseg, path_u  as nmpc_batch_follow_path, read / written for FOLLOW_PATH robots only; segs,
 *            nseg and path_u may all be NULL when no robot is in FOLLOW_PATH. A robot's list is its active path
 *   reset    [B] in/out or NULL: pending controller reset. The node's goal and path callbacks call reset_mpc() at
 *            once (:304-327), which shows only at the next solve: reset[i] is consumed (and cleared to 0) when
 *            robot i solves and stays set while it does not
 *   event    [B] out NMPC_NODE_EV_* or NULL
 *   err      [2][B] out or NULL: path errors of the FOLLOW_PATH robots that reached the nearest-point step, NaN
 *            elsewhere
 *   traj_out [N+1][3][B] out or NULL: the reference poses each solving robot used; NaN for the others
 *   n_solved device int[1] out or NULL: robots that ran a solve
 *   cmd, u0, status, qp_iter, qp_res  as nmpc_batch_run; all zero for a robot that did not solve
 * A robot in a mode whose inputs are NULL goes to Error with EV_NONE. Per robot (all tests in fp64 on the fp32
 * inputs widened exactly; dist and normAngRad as utils.h):
 *   IDLE, ERROR   nothing runs: event NONE, the mode stays.
 *   BREAK         stop command, -> Idle, event BREAK.
 *   GOTO_POSE     d = dist(goal, pose). enable_safe_conditions && d >= max_goal_dist: stop, -> Idle, GOAL_TOO_FAR.
 *                 Else d <= final_pos_err && ang <= final_ori_err: stop, -> Idle, ARRIVED. Else solve on the
 *                 one-pose reference (traj_len 1, padded with the goal: diff's terminal-weight hack fires, as in
 *                 the node).
 *   FOLLOW_PATH   nseg < 1: -> Idle, EV_NONE (executeNMPC's empty list, :702-705). Else the nearest point from
 *                 path_u[i] and the path errors (exactly nmpc_path_nearest / nmpc_batch_follow_path, the
 *                 holonomic heading for omni4); path_u[i] is updated. enable_safe_conditions and an error >= its
 *                 threshold (+inf or NaN: that comparison is off): stop, -> Error, OFF_PATH, and the robot does
 *                 NOT solve. Else getNextNPoses (N+1 poses, bit-identical to nmpc_path_discretize), then the end
 *                 test against the last pose (in fp64, before its rounding to fp32): stop, -> Idle, ARRIVED, or
 *                 the solve on those poses.
 *   A solve with status != 0: zero cmd, -> Error, SOLVE_FAILED; the robot keeps its iterate and carried refs
 *   (nmpc_batch_run's rule).
 * A robot that does not solve is not touched: its rows of the iterate and the carried refs, its warm flag, its
 * scratch records and its placement key are bit for bit what they were. The solve is nmpc_batch_run's on the gate's
 * references: the kernel form follows B (nmpc_batch_plan_ex, NMPC_PLAN_RUN), the grid is sized for B, and blocks
 * past the active count leave at once. Placement: the active robots fill the lowest team slots, in index order
 * under NMPC_SCHED_OFF (and AUTO below the dense threshold, and in the one-robot-per-block forms), hardest first
 * under SORTED (and AUTO when dense); INTERLEAVED and SPREAD fall back to SORTED for node ticks.
 * sample_period must be finite and >= 0.
 * Out of scope here: the upcoming_path_ queue, the velocity-sign split of processPathBuffers (:576-595) and the hop
 * to the next queued path at :686-690. A robot's list is one active path, and on ARRIVED the caller hands the robot
 * its next part and sets reset[i]; nmpc_batch_node_tick_queue below keeps the whole path set on the device instead.
 * Both ticks start after getInputData (:545-553): pose, vel and steer are its results. That first line of mainCycle
 * has a stage of its own, nmpc_batch_node_input below, and nmpc_batch_node_cycle runs the stage and a tick in one
 * call, from fp64 map coordinates to the command. */
int nmpc_batch_node_tick(nmpc_batch* b, int B, const nmpc_node_params* np, unsigned char* mode, const float* pose,
                         const float* vel, const float* steer, const float* goal, const nmpc_path_segment* segs,
                         int seg_stride, const int* nseg, double* path_u, unsigned char* reset, unsigned char* event,
                         double* err, float* traj_out, int* n_solved, float* cmd, float* u0, int* status,
                         int* qp_iter, float* qp_res, void* stream);

/* The node tick with each robot's path-set queue on the device: the bookkeeping NMPCNavControlROS keeps in
 * active_path_ / upcoming_path_ runs in the gate, so a mission of several parts (forward, reversing, forward again)
 * needs no host round trip at the part ends. A robot's whole set stays in its records segs[i*seg_stride ..
 * +npart[i]-1]; active_path_ is the parts [head, tail) and upcoming_path_ the parts [tail, npart). Same launches as
 * nmpc_batch_node_tick (gate, march, order, solve, finish), no host synchronisation.
 * (The value is parenthesised to keep this constant apart from the seven events of the plain tick above.) */
/* end of a part with parts still queued (:686-692): stop command, stays FOLLOW_PATH */
#define NMPC_NODE_EV_NEXT_PART (7)

typedef struct nmpc_path_queue {
    const int* npart;      /* [B] parts of robot i's whole set */
    int* head;             /* [B] in/out: first active part */
    int* tail;             /* [B] in/out: one past the last active part */
    const int* frame;      /* [B][seg_stride] frame id per part as a number, or NULL: all equal (:589) */
    const double* length;  /* [B][seg_stride] GetPathLength() per part, or NULL: part_length for every part */
    double part_length;    /* default 1000: the node's SetPathLength(1000), :571 */
    double max_active_len; /* default 5.0: max_active_path_length (nmpc_nav_control.yaml:6) */
    double* remains;       /* [B] out or NULL: patch_remains (:374-375) for FOLLOW_PATH robots, NaN for the others */
} nmpc_path_queue;
int nmpc_path_queue_default(nmpc_path_queue* q); /* scalars as above, pointers NULL */

/* Arguments: q, then those of nmpc_batch_node_tick without nseg. path_u[i] is active_path_u_, the path parameter
 * relative to part head[i]. A new path set is given by writing the parts, npart[i], head[i] = tail[i] = 0,
 * path_u[i] = 0, reset[i] = 1 (the path callbacks call reset_mpc(), :316 / :326) and mode[i] = FOLLOW_PATH.
 * Dropping the parts with an empty frame id (:569) and decoding the messages stay with the caller. Everything not
 * named here is nmpc_batch_node_tick's: the other modes, the outputs, the untouched non-solvers, placement, n_solved
 * and the reset rule. Argument errors as there; also q NULL, npart / head / tail NULL while segs is given, and a
 * non-finite part_length or max_active_len. Per FOLLOW_PATH robot, all in fp64:
 *   1. nP = clamp(npart, 0, seg_stride), h = clamp(head, 0, nP), t = clamp(tail, h, nP): no segment outside the
 *      robot's own records is read, and the clamped values are what is written back. nP < 1: -> Idle, EV_NONE, the
 *      window untouched.
 *   2. t == h (a new set): fill(0), processPathReceived's processPathBuffers(0.0) (:573). Still empty: -> Idle,
 *      EV_NONE.
 *   3. The nearest point over the parts [h, t) from path_u: nmpc_path_nearest's search on those parts, U.
 *   4. The pop (:603-609): k = floor(U); if t - h > k: h += k, U -= k.
 *   5. fill(U) (:652).
 *   6. The path errors and the guard as in nmpc_batch_node_tick, with one difference: the pi of a part driven
 *      backwards follows the FRONT part after the pop (active_path_.front().GetVelocity(), :655), where
 *      nmpc_path_nearest takes the segment of nearest_u. The two differ only when U == t - h exactly (the end of the
 *      window: nothing is popped, and the front part is the first one). OFF_PATH leaves head, tail and path_u as
 *      updated so far, as the node does.
 *   7. getNextNPoses over [h, t) from U, bit-identical to nmpc_path_discretize on those parts.
 *   8. The end test on the last pose. Arrived with t == nP: -> Idle, ARRIVED. Arrived with parts queued: h += 1,
 *      t += 1 (pop_front and push of the upcoming front without a sign or frame test, :687-689), path_u = 0, the mode
 *      stays FOLLOW_PATH, EV_NEXT_PART, stop command; reset[i] is not touched. Else the robot solves.
 *   9. remains[i] = r > 0 ? r - path_u : r with r = nP - h, from the values the tick leaves behind; NaN for a robot
 *      that is not in FOLLOW_PATH after the tick (a failed solve included).
 *   fill(U) is processPathBuffers (:576-595):
 *      L = sum over k in [h, t) of len(k) * (k == h ? 1 - U : 1)
 *      while L < max_active_len and t < nP:
 *          if t > h: break if v[t-1] * v[t] < 0, or if frame is given and frame[t-1] != frame[t]
 *          t += 1; L += len(t-1) */
int nmpc_batch_node_tick_queue(nmpc_batch* b, int B, const nmpc_node_params* np, const nmpc_path_queue* q,
                               unsigned char* mode, const float* pose, const float* vel, const float* steer,
                               const float* goal, const nmpc_path_segment* segs, int seg_stride, double* path_u,
                               unsigned char* reset, unsigned char* event, double* err, float* traj_out,
                               int* n_solved, float* cmd, float* u0, int* status, int* qp_iter, float* qp_res,
                               void* stream);

/* The node's input stage, getInputData (NMPCNavControlROS.cpp:545-553), on the device: per robot a history of
 * localisation samples (the TF buffer of base_frame in the frame the robot's goal or path is expressed in), the pose
 * with the heading hack of getRobotPose (:401-436), the finite-difference body velocity of getRobotVel (:438-484), the
 * data ages, and the conversion of pose and goal into the robot's map frame (nmpc_batch_set_robot_frame), with the
 * recentre decision in the same launch. Everything here is fp64 in map coordinates with int64 nanosecond stamps; the
 * outputs are the fp32 frame values the ticks above take.
 *
 * nmpc_batch_enable_input allocates the state, per handle and on demand like the tables, instance-minor:
 *   stamp  [depth][capacity]     int64 ns
 *   sample [depth][3][capacity]  fp64 {x, y, yaw}, map coordinates
 *   count  [capacity]            samples stored, at most depth
 *   newest [capacity]            slot of the newest sample
 *   held   [7][capacity]         fp64 {x, y, theta, v, vn, w, steer}: robot_pose_, robot_vel_ and
 *                                robot_steering_wheel_angle_ of every robot
 * 2 <= depth <= 64. Everything is 0 at enable: the reference leaves the three held members uninitialised until their
 * first successful read, 0 is this project's rule. A second call with the same depth is a no-op, another depth is
 * NMPC_ERR_ARG. nmpc_batch_input_state is the checkpoint view (each output may be NULL; every pointer is NULL and
 * *depth 0 while the state is off; *stride = capacity). */
int nmpc_batch_enable_input(nmpc_batch* b, int depth);
int nmpc_batch_input_state(nmpc_batch* b, long long** stamp, double** sample, int** count, int** newest, double** held,
                           int* depth, int* stride);

/* The listener: one small launch, one lane per robot. For the robots [0, B) with mask[i] != 0 (mask [B] device, NULL:
 * all) the sample (stamp_ns[i], sample[:, i]) goes into the slot after newest (slot 0 of an empty ring), newest moves
 * there and count saturates at depth. A sample is dropped -- dropped[i] = 1, nothing of the robot changes -- when its
 * stamp is <= the newest stored stamp or any of its three values is not finite; every other robot of [0, B) gets
 * dropped[i] = 0 (dropped [B] device, or NULL). tf2 is not in the reference tree: this rule (stamps strictly increase,
 * the oldest sample is overwritten) is the project's own, as the nearest-point search is.
 * Argument errors: B out of range, stamp_ns or sample NULL, a NULL handle, no input state. */
int nmpc_batch_push_samples(nmpc_batch* b, int B, const long long* stamp_ns, const double* sample /* [3][B] x, y, yaw */,
                            const unsigned char* mask, unsigned char* dropped /* [B] or NULL */, void* stream);

#define NMPC_NODE_EV_INPUT_INVALID (8) /* nmpc_batch_node_cycle, strict: the input data were invalid, -> Error */

typedef struct nmpc_node_input {
    long long now_ns;              /* ros::Time::now() of this cycle */
    long long period_ns;           /* Duration(1.0 / control_freq): default 25000000 */
    double transform_timeout;      /* s, default 0.1 (nmpc_nav_control.yaml:5) */
    int pose_valid_overwritten;    /* default 1: getInputData:549-550 assigns valid_data twice, so the pose check is lost */
    int strict;                    /* default 0, see the cycle */
    double recentre_radius;        /* default +inf: never; finite: recentre in this launch */
    const float* steer;            /* [B] measured steering angle (tric) or NULL = 0 */
    const unsigned char* steer_ok; /* [B] or NULL = all ok: getSteeringWheelAngle's result */
    unsigned char* valid;          /* [B] out or NULL */
    float *pose, *vel, *steer_out; /* [3][B], [3][B], [B] out or NULL (handle-owned buffers then) */
    unsigned char* moved;          /* [B] out or NULL: 1 where this launch gave the robot a new origin */
} nmpc_node_input;
int nmpc_node_input_default(nmpc_node_input* in); /* scalars as above, pointers NULL */

/* The stage: one launch, one lane per robot. It runs for a robot whose mode is GOTO_POSE, FOLLOW_PATH or BREAK (mode is
 * read only); for IDLE, ERROR or a value above 4 it skips the input steps, leaves held untouched and sets valid = 1.
 * For a robot that runs:
 *   sec(d)     = (double)floor_div(d, 1e9) + 1e-9 * (double)(d - floor_div * 1e9): ros::Duration::toSec.
 *   lookup(t)  (the project's rule) fails when count == 0, t < the oldest stored stamp or t > the newest. A stored
 *              stamp equal to t gives that sample. Otherwise, with a and b the stored neighbours, ta < t < tb, and
 *              r = sec(t - ta) / sec(tb - ta): x = (1 - r) xa + r xb, y likewise, yaw = ya + r normAngRad(yb - ya).
 *   pose       (getRobotPose) an empty ring: pose_ok = 0 and the held pose stays. Otherwise held.x, held.y are the
 *              newest sample's and held.theta the hack of :414-423 on (held.theta, yaw), the same comparisons and the
 *              two loops, each coded for at most two trips (one is all a yaw within [-pi, pi], tf2::getYaw's range,
 *              can need, so no value can spin them); pose_ok = !(sec(now - stamp_newest) > transform_timeout). The
 *              pose is written even when it is stale, as in the reference.
 *   velocity   (getRobotVel) t2 = the newest stamp, t1 = t2 - period_ns, both looked up. A failed lookup, or
 *              dt = sec(t2 - t1) with dt <= 0 || dt > transform_timeout, gives vel_ok = 0 and the velocity is held;
 *              otherwise :456-476 in that operation order into held.v, vn, w.
 *   steering   (tric handles) steer_ok[i] == 0: steer_valid = 0, the held value stays; else held.steer = steer[i].
 *   valid      pose_valid_overwritten ? vel_ok : pose_ok && vel_ok; tric: &= steer_valid.
 *   recentre   recentre_radius finite: nmpc_batch_recentre's decision and move on (held.x, held.y), for the robots that
 *              ran the stage, in this launch (a frame table that is off is started, as nmpc_batch_recentre does); moved
 *              as there. A non-finite radius reads nothing of the frame table but the origins.
 * Outputs, for every robot of [0, B): pose = (float)(held.xy - origin_i) with the origin after any recentre ((0, 0)
 * while the table is off) and (float)held.theta; vel and steer_out the fp32 roundings of the held values; goal_out =
 * (float)(goal_map.xy - origin_i), (float)goal_map.theta when goal_map and goal_out are both given. No loop depends on
 * the data (the ring is walked depth times by every lane), every read is instance-minor, and every fp64 product-sum is
 * compiled without contraction, so x, y, theta and the ring are reproducible on the host bit for bit; the velocity
 * goes through cos and sin and is reproducible to 1e-12.
 * Out of scope: quaternion decoding (tf2::getYaw: the samples carry a yaw), the per-mode TF frame ids of
 * mainCycle:520-528 (one map frame per robot, the caller's), the wheel-frame TF chain of getSteeringWheelAngle (the
 * caller gives angle and ok flag) and the capsule ABI.
 * Argument errors: B out of range, in NULL, mode NULL, a NULL handle, no input state. */
int nmpc_batch_node_input(nmpc_batch* b, int B, const nmpc_node_input* in, const unsigned char* mode,
                          const double* goal_map /* [3][B] or NULL */, float* goal_out /* [3][B] or NULL */, void* stream);

/* The whole cycle: the stage, then nmpc_batch_node_tick (q NULL; nseg is read) or nmpc_batch_node_tick_queue (q given)
 * on the stage's fp32 outputs, with those calls' launches and kernels, then the status rule in one small launch.
 * Everything is queued on `stream`, no host synchronisation. goal_map [3][B] fp64 map coordinates or NULL (no robot in
 * GOTO_POSE); in->pose, vel, steer_out, valid may be NULL (the handle's buffers carry the values to the tick). steer
 * reaches the tick on tric handles only. Everything else as the tick's arguments.
 *   strict = 0 (the node as written): getInputData sets Error, but the process* call of the same cycle still runs on
 *     the held values (:519-529), so the tick runs as the mode says. Afterwards a robot with valid == 0 whose mode is
 *     still GOTO_POSE or FOLLOW_PATH goes to ERROR (its remains to NaN); a robot the tick sent to IDLE or ERROR keeps
 *     that. Event and command are the tick's.
 *   strict = 1: an invalid robot does not tick: stop command, mode ERROR, event NMPC_NODE_EV_INPUT_INVALID, and its
 *     resident rows (iterate, carried refs, warm flag, records, placement key, path window, path_u, reset) stay bit for
 *     bit. (Its mode is set to ERROR before the gate and its event after the tick; the gate is unchanged.)
 * Argument errors: the tick's, in NULL, and a handle without input state. The ticks compute what they computed, with
 * the input state on or off. */
int nmpc_batch_node_cycle(nmpc_batch* b, int B, const nmpc_node_params* np, const nmpc_path_queue* q /* NULL: plain tick */,
                          const nmpc_node_input* in, unsigned char* mode, const double* goal_map,
                          const nmpc_path_segment* segs, int seg_stride, const int* nseg /* read when q is NULL */,
                          double* path_u, unsigned char* reset, unsigned char* event, double* err, float* traj_out,
                          int* n_solved, float* cmd, float* u0, int* status, int* qp_iter, float* qp_res, void* stream);

/* Kernel variant: NMPC_KERNEL_TEAM (16-lane team per robot, DPP row exchange) is the only one; any other value
 * returns NMPC_ERR_UNSUPPORTED. (The round-1 one-lane-per-robot kernel was removed: its fp32 factor is not
 * accurate enough at bench scale, DESIGN.md "Algorithm and precision".) */
#define NMPC_KERNEL_TEAM 0
int nmpc_batch_set_kernel(nmpc_batch* b, int kernel);

/* Team placement of the team kernel (no effect on any result; DESIGN.md "Scheduling"). A robot's IPM iteration
 * count persists from tick to tick, so the handle keeps each robot's last count and, before a launch, orders the
 * robots by it (one small sort kernel on the same stream):
 *   NMPC_SCHED_OFF          robot i in team slot i;
 *   NMPC_SCHED_AUTO         (default) NMPC_SCHED_SORTED when the launch has more waves (B/4) than the device
 *                           has SIMDs, else OFF (with one wave per SIMD the slowest robot sets the time
 *                           whatever the placement);
 *   NMPC_SCHED_SORTED       hardest robots in the lowest slots (tric N=60 B=8192: 5.24 -> 5.06 ms per tick);
 *   NMPC_SCHED_INTERLEAVED  even 16-team blocks from the hard end, odd blocks from the easy end (best when
 *                           several models' launches share the GPU on concurrent streams: mixed fleet
 *                           4.44 -> 4.26 ms per tick). */
#define NMPC_SCHED_OFF 0
#define NMPC_SCHED_AUTO 1
#define NMPC_SCHED_SORTED 2
#define NMPC_SCHED_INTERLEAVED 3
#define NMPC_SCHED_SPREAD 4 /* the hardest 4 robots per block in its first wave, easy CU-mates (schedule.hip) */
int nmpc_batch_set_schedule(nmpc_batch* b, int mode);

/* Device pointers of the resident state: xbar [(N+1)*NX][stride], ubar [N*NU][stride],
 * carried [NBX][stride]; stride = capacity. */
int nmpc_batch_state(nmpc_batch* b, float** xbar, float** ubar, float** carried, int* stride);

/* Forget the IPM warm start of instances [0, B) where mask[i] != 0 (mask NULL: all of them): their next solve
 * starts its multipliers cold (qp_mu0 / t), as after a reset, while the iterate is kept. For callers that move
 * instances between slots (a slot's multipliers belong to whatever instance solved there last). mask: device. */
int nmpc_batch_forget_warm(nmpc_batch* b, int B, const unsigned char* mask, void* stream);

/* Device pointers of the IPM warm-start state (qp_warm_start): warm [capacity] per-robot flags and the scratch
 * records [scratch_bytes] that hold each robot's multipliers. A flag is 0 (the next solve starts cold) or the tag of
 * the record layout its multipliers were stored in (NMPC_WARM_TAG_*): a solve reads them only when its launch uses
 * the same layout, so a robot whose launches change kernel or layout (e.g. a handle whose batch crosses the
 * row-parallel kernel's limit) starts cold on its own, and no other robot is touched. With nmpc_batch_state this
 * is everything a solve reads from the handle, e.g. to checkpoint a fleet or to replay a tick bit for bit.
 * Checkpoints of this state are tied to the library version that wrote them: before round 5 a flag of 1 meant
 * "succeeded", whatever the layout, and now reads as NMPC_WARM_TAG_WIDE (a tric team-kernel record written then
 * was split-layout). After restoring a warm state saved by an older build, call nmpc_batch_forget_warm on the
 * restored robots: their first solve then starts cold (wrong warm multipliers would only be clamped, costing
 * IPM iterations, never a wrong solution). */
#define NMPC_WARM_TAG_WIDE 1     /* single-direction field order, one record per lane (team / row-parallel) */
#define NMPC_WARM_TAG_SPLIT 2    /* the team kernel's split core / bound planes */
#define NMPC_WARM_TAG_MEHROTRA 3 /* the Mehrotra rule's field order (NMPC_IPM_MEHROTRA) */
int nmpc_batch_warm_state(nmpc_batch* b, unsigned char** warm, float** scratch, size_t* scratch_bytes);

/* Per-robot bounds and weights. A handle has one nmpc_model_params; a fleet of one geometry still has loaded and
 * empty vehicles, zones with their own speed limits and aisles that want a heavier heading weight (the reference runs
 * one node per robot, each with its own yaml values, NMPCNavControlROS.cpp:96-110,164-176,234-259). The handle
 * therefore owns a device table [rows][capacity], fp32, instance-minor like the carried refs, with the rows
 *     lbx[NBX] ubx[NBX] lbu[NBU] ubu[NBU] W[NY] W_e[NX]
 * in this order (diff 24 rows, omni4 42, tric 24). It is allocated by the first writer call below and starts with the
 * handle's own parameters in every column (the fp32 values the kernels take from nmpc_model_params). While the table
 * is on, every launch of the handle -- nmpc_batch_solve, _solve_iterate, _run, _run_path, _follow_path and both node
 * ticks -- takes each robot's bounds and weights from the robot's column; while it is off (never written, or after
 * nmpc_batch_clear_robot_params) every launch computes exactly what it computed without this interface.
 * Each writer is one small launch on `stream`, with no host synchronisation and no host-side validation (the values
 * are device data): a zone change for some robots costs one enqueue before the next tick.
 * Rules:
 *   - While the table is on, the six fields lbx, ubx, lbu, ubu, W and W_e of nmpc_batch_set_params do not reach a
 *     launch (they are what a table allocated or cleared later starts from). The QP options, p, dt, dt_ctrl,
 *     terminal_hack and tric_sin_bug still do.
 *   - In nmpc_batch_solve / _solve_iterate a caller's We argument still wins over the table's W_e rows. Run mode's
 *     terminal hack uses the robot's own stage weights, and the early infeasibility exit (qp_infeas_lambda) scales
 *     with the robot's own largest stage or terminal weight.
 *   - A robot's warm flag is left alone when its rows change: warm multipliers are clamped at the start of the
 *     next solve (max(min(lambda, cap), kappa / t)), which covers multipliers that went stale with the old box.
 *   - A NaN bound fails that robot alone, with status 1, as a NaN input does. A NaN weight does the same.
 *   - lb > ub, and a box that the robot's carried reference state cannot reach within one stage, give that robot
 *     a nonzero status through the solver's existing exits (status 4: infeasible QP or iteration limit); no other
 *     robot is affected, and the robot keeps its iterate and carried refs and gets a stop command, as after any
 *     failed solve. The input weights R must stay > 0, as nmpc_batch_create requires of the handle's.
 *   - One scope stays with the handle: weights that vary along the horizon (one W per robot, for every stage).
 *     Bounds that vary along the horizon have a table of their own (nmpc_batch_set_stage_bounds below), which then
 *     replaces this table's four bound rows, and the model parameters p (b, tau_v, ...) have one too
 *     (nmpc_batch_set_robot_model below).
 * Argument errors (NMPC_ERR_ARG): B out of range, rp NULL, every field NULL (nmpc_batch_set_robot_limits: every
 * array NULL), a NULL handle. */
typedef struct nmpc_robot_params {
    const float* lbx; /* [NBX][B] device, or NULL: those rows stay as they are */
    const float* ubx; /* [NBX][B] */
    const float* lbu; /* [NBU][B] */
    const float* ubu; /* [NBU][B] */
    const float* W;   /* [NY][B] */
    const float* W_e; /* [NX][B] */
} nmpc_robot_params;
/* Write the rows of the non-NULL fields for robots [0, B) where mask[i] != 0 (mask [B] device, NULL: all). */
int nmpc_batch_set_robot_params(nmpc_batch* b, int B, const nmpc_robot_params* rp, const unsigned char* mask,
                                void* stream);
/* The batched nmpc_model_params_set_limits, with the same mapping: ref states in [-v_max, v_max] (tric: v_ref only,
 * alpha_ref in [alpha_min, alpha_max]), inputs in [-a_max, a_max] (tric: dv_ref only, dalpha_ref in [-dalpha_max,
 * dalpha_max]). Each argument is a device array [B] or NULL (those rows stay); the three steering arrays are read
 * for tric only. mask as above. */
int nmpc_batch_set_robot_limits(nmpc_batch* b, int B, const float* v_max, const float* a_max, const float* alpha_min,
                                const float* alpha_max, const float* dalpha_max, const unsigned char* mask,
                                void* stream);
/* The table's device view for checkpoints: *table [rows][stride] (stride = capacity), or NULL while the table is
 * off. Each output may be NULL. With nmpc_batch_state and nmpc_batch_warm_state this is everything a solve reads
 * from the handle. */
int nmpc_batch_robot_params(nmpc_batch* b, float** table, int* rows, int* stride);
/* Turn the table off: launches use the handle's parameters again. The next writer call starts a fresh table from the
 * handle's parameters. (Host-side switch: it applies to the launches enqueued after it.) */
int nmpc_batch_clear_robot_params(nmpc_batch* b);

/* Stage-varying bounds. One box per robot holds at every stage of the horizon, so a speed limit that drops when a
 * robot enters a zone can only be applied at once, and a robot that is faster than the new limit gets an infeasible
 * QP (status 4, stop command). With a box per stage the limit can come down along the horizon and the solve brakes
 * into it. The handle therefore owns a second device table, the stage table: for every robot and every stage
 * k = 0..N the rows
 *     lbx[NBX] ubx[NBX] lbu[NBU] ubu[NBU]
 * in fp32. It is allocated by the first writer call below. Its size is (N+1) * (2 NBX + 2 NBU) * capacity * 4 bytes:
 * 5.4 MB for diff at N = 40 and 4096 robots, 86 MB at 65536. The bounded-state rows of stages 1..N and the input rows
 * of stages 0..N-1 reach a launch; the state rows of stage 0 and the input rows of stage N are allocated and never
 * interpreted (a NaN there is harmless). The device layout is the library's business ([stage][robot][row] today: one
 * robot's rows of a stage share a cache line); the checkpoint view is opaque bytes.
 * Rules:
 *   - While the stage table is on, every launch of the handle -- nmpc_batch_solve, _solve_iterate, _run, _run_path,
 *     _follow_path and both node ticks -- takes each robot's box at stage k from it. W and W_e still come from the
 *     per-robot table if that is on, else from the handle (a caller's We still wins in solve mode). The four bound
 *     rows of the per-robot table, and the handle's, then do not reach a launch: they are what a stage table
 *     allocated or cleared later starts from (the robot's column if the per-robot table is on at that moment, else
 *     the handle's values, at every stage).
 *   - While it is off (never written, or after nmpc_batch_clear_stage_bounds) every launch computes exactly what it
 *     computed without this interface.
 *   - Each writer is one small launch on `stream`, with no host synchronisation and no host-side validation.
 *   - A NaN in a bound the QP uses fails that robot alone with status 1; lb > ub at a stage gives that robot a
 *     nonzero status through the solver's existing exits. The robot keeps its iterate and carried refs and gets a
 *     stop command, as after any failed solve; no other robot is affected. Warm flags are left alone.
 *   - nmpc_batch_shift_stage_bounds moves a profile one tick down the horizon. A shift by one stage per tick matches
 *     the plant only when dt_ctrl == dt, which holds for the defaults (both 1/40); otherwise upload the profile
 *     again, sampled at the solver's stage times.
 *   - Still with the handle: stage-varying weights (the stage weight is read inside every IPM iteration, so a weight
 *     per stage would cost the hot loop), and the capsule ABI, which keeps rejecting stage-varying data.
 * Argument errors (NMPC_ERR_ARG): B out of range, sb NULL, every field NULL (nmpc_batch_set_stage_limits: every array
 * NULL), n < 0, a NULL handle. */
typedef struct nmpc_stage_bounds {
    const float* lbx; /* [N+1][NBX][B] device, or NULL: those rows stay as they are */
    const float* ubx; /* [N+1][NBX][B] */
    const float* lbu; /* [N][NBU][B] */
    const float* ubu; /* [N][NBU][B] */
} nmpc_stage_bounds;
/* Write the rows of the non-NULL fields at every stage for robots [0, B) where mask[i] != 0 (mask [B] device, NULL:
 * all). */
int nmpc_batch_set_stage_bounds(nmpc_batch* b, int B, const nmpc_stage_bounds* sb, const unsigned char* mask,
                                void* stream);
/* The batched, per-stage nmpc_model_params_set_limits, with the mapping of nmpc_batch_set_robot_limits: v_max,
 * alpha_min, alpha_max are device arrays [N+1][B], a_max and dalpha_max [N][B]; each may be NULL (those rows stay).
 * The three steering arrays are read for tric only. mask as above. */
int nmpc_batch_set_stage_limits(nmpc_batch* b, int B, const float* v_max, const float* a_max, const float* alpha_min,
                                const float* alpha_max, const float* dalpha_max, const unsigned char* mask,
                                void* stream);
/* Receding horizon: stage k takes stage min(k + n, last) of the same row (last = N for state rows, N-1 for input
 * rows), n >= 0, for the robots with mask[i] != 0; the last stage is repeated. One thread per (row, robot) walks k
 * upwards, so the shift is in place. */
int nmpc_batch_shift_stage_bounds(nmpc_batch* b, int B, int n, const unsigned char* mask, void* stream);
/* The table's device view for checkpoints: *table and *bytes (opaque: copy it whole, into a handle of the same model,
 * N and capacity), or NULL / 0 while the table is off. Each output may be NULL. */
int nmpc_batch_stage_bounds(nmpc_batch* b, void** table, size_t* bytes);
/* Turn the stage table off: launches use the per-robot table's or the handle's one box again. The next writer call
 * starts a fresh table. (Host-side switch: it applies to the launches enqueued after it.) */
int nmpc_batch_clear_stage_bounds(nmpc_batch* b);

/* Speed zones: the speed rows of the stage table from a speed map, on the device. A speed map is a grid mask in map
 * coordinates, the shape fleet software uses for speed filters; the writer below looks up every stage of every
 * processed robot's predicted horizon in it and writes a limit profile that the QP can follow, so a zoned fleet needs
 * no host round trip per tick (csrc/speed_map.hip, DESIGN.md "Speed zones").
 * The rule, for a processed robot i; the fp32 operations and their order are part of the contract (nothing is fused):
 *   cap    the robot's own speed cap: ubx[0] of its column of the per-robot table while that table is on, else the
 *          handle's ubx[0]; a = ubu[0] from the same source
 *   g      = (slope * a) * (float)dt
 *   c      the largest |carried[j][i]| over the speed reference states (diff, omni4: all NBX states; tric: the first)
 *   stage k's position: rows k*NX and k*NX+1 of the resident iterate's xbar (RTI does not shift: this is the
 *          linearisation point the stage-k box applies to); for a robot with reset[i] != 0, whose iterate is about to
 *          be zeroed, pose[0..1][i] at every stage. In map coordinates (double)position + origin_i while the frame
 *          table is on, else (double)position
 *   cell   cx = floor((X - x0) / res), cy = floor((Y - y0) / res) in fp64 (half a cell below x0 is outside, not cell
 *          0); off the grid or not finite: m_k = outside, else m_k = vmax[cy * w + cx]
 *   z_k    = fminf(cap, fmaxf(v_floor, m_k)); a NaN cell therefore acts as v_floor
 *   r_k    = min over j = k..N of (z_j + (float)(j - k) * g): a limit comes down along the horizon before the robot
 *          reaches the zone, at most g per stage
 *   lim_k  = fmaxf(r_k, c - (float)k * g), k = 0..N: the robot's current reference speed stays reachable
 * Written: for k = 0..N the rows nmpc_batch_set_stage_limits' v_max writes, lbx = -lim_k and ubx = lim_k, and
 * vlim[k*B + i] = lim_k when vlim is given. Not written: the input rows, tric's steering rows, and every row of a
 * robot that was not processed.
 * The caller's duties:
 *   - A robot whose iterate holds no solution yet must be flagged in reset (its xbar is no prediction). In the node's
 *     flow that always holds: the goal and path callbacks set the flag together with the new target.
 *   - The map is configuration, not state: checkpoints carry the stage table (nmpc_batch_stage_bounds), not the map;
 *     attach it again after a restore. The grid stays the caller's device memory and must outlive its use.
 *   - With per-robot frames on, the map is in map coordinates and the frame table bridges; nothing else is needed.
 * Out of scope: rotated or per-robot maps, maps for anything but the speed rows, the capsule ABI,
 * nmpc_batch_solve_iterate's caller-held iterate (the writer reads the resident one), and any change to the solve
 * kernels or to what a launch computes while no map is attached.
 * Argument errors (NMPC_ERR_ARG): B out of range, map NULL, res <= 0 or not finite, w < 1, h < 1, vmax NULL, slope
 * outside (0, 1], v_floor <= 0, reset without pose, a NULL handle. */
typedef struct nmpc_speed_map {
    double x0, y0;     /* map coordinates of the low corner of cell (0, 0) */
    double res;        /* cell edge, m, > 0 */
    int w, h;          /* cells along x, along y, >= 1 */
    const float* vmax; /* [h][w] device, row cy, column cx: speed limit of the cell, m/s; +inf: none */
    float outside;     /* the limit off the grid (default +inf) */
} nmpc_speed_map;
typedef struct nmpc_speed_rule {
    float slope;   /* fraction of a_max * dt a limit may come down per stage, default 0.8 (the ramps' value) */
    float v_floor; /* smallest limit ever written, default 0.05 m/s: a box must keep an interior */
} nmpc_speed_rule;
int nmpc_speed_map_default(nmpc_speed_map* map); /* zeros, outside = +inf */
int nmpc_speed_rule_default(nmpc_speed_rule* rule);
/* One launch on `stream`, no host synchronisation, through the stage table's writer path: the first call allocates and
 * fills the table as every stage writer does. pose [3][B] frame values (required when reset is given), reset [B] or
 * NULL, mask [B] or NULL (all), vlim [N+1][B] out or NULL; all device. */
int nmpc_batch_stage_limits_from_map(nmpc_batch* b, int B, const nmpc_speed_map* map,
                                     const nmpc_speed_rule* rule /* NULL: defaults */, const float* pose,
                                     const unsigned char* reset, const unsigned char* mask, float* vlim, void* stream);
/* Attach (a copy of the structs; the grid stays the caller's device memory) or detach (map NULL) the handle's speed
 * map. While a map is attached, nmpc_batch_node_cycle runs the writer between the input stage and the tick, on the
 * stage's fp32 pose and the cycle's reset array, for exactly the robots whose mode at that point is GOTO_POSE or
 * FOLLOW_PATH (under strict an invalid robot is ERROR by then, so its rows stay bit for bit). While none is attached
 * the cycle enqueues the launches it enqueued without this interface and allocates no stage table. */
int nmpc_batch_set_speed_map(nmpc_batch* b, const nmpc_speed_map* map, const nmpc_speed_rule* rule /* NULL: defaults */);

/* Fleet separation: the speed rows of the stage table from the other robots' predictions. A robot that closes on
 * another one slows down, as it does under a safety scanner's warning field: every stage of a processed robot's
 * horizon gets a speed cap from the distance to the nearest "track" at the same time, and the speed map's rule turns
 * the caps into a limit profile the QP can follow (csrc/separation.hip, DESIGN.md "Fleet separation"). A track is a
 * predicted path in map coordinates: another robot's horizon (nmpc_batch_export_tracks; several handles write into one
 * buffer at different columns), a person from a tracker, a standing obstacle (K = 0).
 * The rule, for a processed robot i; the fp32 operations and their order are part of the contract (nothing is fused):
 *   p_k, cap, g, c   exactly the speed map's: the position of stage k in fp32 frame values (pose[0..1][i] at every
 *          stage for a robot with reset[i] != 0), the robot's speed cap, its ramp step and its carried speed; X_k, Y_k
 *          the fp64 map coordinates of p_k ((double)p_k + origin_i while the frame table is on)
 *   h_k    = p_{min(k+1, N)} - p_{min(k, N-1)}, the direction of travel, one fp32 subtraction per component; a reset
 *          robot has h_k = 0. Driving backwards needs no special case
 *   pair   every track j other than own_first + i, at track stage kk = min(k, K): dx = (float)(Tx - X_k),
 *          dy = (float)(Ty - Y_k), q = dx*dx + dy*dy (mul, mul, add)
 *   counts when q <= range*range (an fp32 product; a NaN fails, so a NaN or infinite track never counts) and, with
 *          ahead_only, when hx == 0 && hy == 0 or dx*hx + dy*hy > 0 (a track exactly abeam does not count)
 *   q_k    the minimum q over the counting pairs, +inf when there is none (min is exact: the kernel's tiles and culls
 *          do not show in the bits)
 *   gap_k  = sqrtf(q_k), correctly rounded
 *   s_k    = gain * (gap_k - clearance)
 *   zmap_k = fminf(cap, fmaxf(v_floor, m_k)), m_k the map's cell as in "Speed zones", +inf without a map
 *   z_k    = fminf(zmap_k, fmaxf(v_floor, s_k))
 *   r_k, lim_k from z_k as in the speed map's rule, and the same rows are written; vlim[k*B + i] = lim_k and
 *          gap[k*B + i] = gap_k when given
 * With M == 0, or when no pair counts, the writer writes exactly what nmpc_batch_stage_limits_from_map writes (without
 * a map: cap, corrected by c). The steady gap behind a leader at speed v is clearance + v / gain.
 * ahead_only: two robots side by side in adjacent aisles, or one that has just been passed, do not brake each other;
 * a standing robot (h = 0) has no direction and counts every track in range.
 * The caller's duties are the speed map's, and: the tracks are configuration, not state: checkpoints carry the stage
 * table, not the tracks; the buffer stays the caller's device memory and must outlive its use.
 * Out of scope: this is speed limiting, not collision avoidance: by this rule alone two robots head-on both come down
 * to v_floor and keep creeping; with the separation guard below attached they stop at stop_gap and stay held until
 * one of them is given another path. No general constraints in the QP, no change to the solve kernels, no per-track
 * radii (a caller with mixed vehicle sizes takes the largest clearance), no rotated footprints, not the capsule ABI,
 * not nmpc_batch_solve_iterate's caller-held iterate, no spatial index over the map.
 * Argument errors (NMPC_ERR_ARG): B out of range, tracks NULL, M < 0, K < 0, xy NULL with M > 0, own_first < -1,
 * own_first >= 0 && own_first + B > M, gain not finite or <= 0, clearance not finite or < 0, range not finite or
 * <= clearance, the speed map's payload checks when map is given and the speed rule's when rule is given, reset
 * without pose, a NULL handle. */
typedef struct nmpc_tracks {
    const double* xy; /* [K+1][2][M] device, fp64 MAP coordinates: track j at stage k (k * dt from now) */
    int M, K;         /* M >= 0 tracks (xy may be NULL when M == 0), K >= 0: robot stage k reads track stage min(k, K) */
    int own_first;    /* robot i of the call is track own_first + i and skips it; -1: no track is the handle's */
} nmpc_tracks;
typedef struct nmpc_sep_rule {
    float clearance;  /* m, >= 0: the centre distance at which the cap reaches 0 (default 0.6) */
    float gain;       /* 1/s, > 0: cap = gain * (gap - clearance) (default 1.0, a one-second headway) */
    float range;      /* m, finite, > clearance: a track farther away does not count (default 3.0) */
    int ahead_only;   /* default 1: only tracks in the half plane of the robot's direction of travel count */
} nmpc_sep_rule;
int nmpc_tracks_default(nmpc_tracks* tracks); /* zeros, own_first -1 */
int nmpc_sep_rule_default(nmpc_sep_rule* sep);
/* The handle's resident horizons as tracks: one small launch that writes, for the robots i in [0, B) and the stages
 * k = 0..K, xy[(k*2 + c)*M + first + i] = the position of stage min(k, N) as the speed map reads it (rows k*NX and
 * k*NX+1 of the resident xbar, widened to fp64, plus the robot's origin while the frame table is on). A robot with
 * reset[i] != 0, and, when mode is given, a robot whose mode[i] is neither GOTO_POSE nor FOLLOW_PATH, is a standing
 * obstacle: pose[0..1][i] plus the origin at every stage. The export reads the resident state and changes nothing of
 * it. pose [3][B] frame values, reset [B] or NULL, mode [B] or NULL; all device. Argument errors: first < 0 or
 * first + B > M, K < 0, xy NULL, pose NULL while reset or mode is given, B out of range, a NULL handle. */
int nmpc_batch_export_tracks(nmpc_batch* b, int B, const float* pose, const unsigned char* reset,
                             const unsigned char* mode, double* xy, int M, int K, int first, void* stream);
/* The writer: on `stream`, no host synchronisation, through the stage table's writer path (the first call allocates and
 * fills the table, as nmpc_batch_stage_limits_from_map does). pose, reset, mask, vlim as there; gap [N+1][B] out or NULL. */
int nmpc_batch_stage_limits_from_tracks(nmpc_batch* b, int B, const nmpc_tracks* tracks,
                                        const nmpc_sep_rule* sep /* NULL: defaults */,
                                        const nmpc_speed_map* map /* or NULL */,
                                        const nmpc_speed_rule* rule /* NULL: defaults */, const float* pose,
                                        const unsigned char* reset, const unsigned char* mask,
                                        float* vlim /* [N+1][B] or NULL */, float* gap /* [N+1][B] or NULL */,
                                        void* stream);
/* Attach (a copy of the two structs; the buffer stays the caller's device memory) or detach (tracks NULL) the handle's
 * tracks. While tracks are attached, nmpc_batch_node_cycle runs between the input stage and the tick: (1) with
 * export_own, the export of the handle's robots [0, B) at own_first, on the stage's fp32 pose, the cycle's reset and
 * mode and K = tracks.K (export_own requires own_first >= 0; the library treats the buffer as writable then); (2) the
 * writer, with the attached speed map and its rule if there is one, for the robots whose mode at that point is
 * GOTO_POSE or FOLLOW_PATH (the speed map's remark on strict applies unchanged). With only a map attached, or with
 * nothing attached, the cycle enqueues exactly the launches it enqueued without this interface. */
int nmpc_batch_set_tracks(nmpc_batch* b, const nmpc_tracks* tracks, const nmpc_sep_rule* sep /* NULL: defaults */,
                          int export_own);

/* The separation guard: right of way and a protective hold on top of the rule above. The rule is a scanner's warning
 * field: it slows a robot down and, because a speed box must keep an interior (v_floor > 0), can never stop it. The
 * guard adds the protective field, which stops a robot that is too close to anything, and a priority filter, which lets
 * one robot of a crossing pair drive on. Neither reaches the solve kernels or the gate's kernels.
 * Right of way. With priority given, a pair (robot i, track j) that counts under the rule must also have
 * priority[j] >= own_i to enter the minimum the speed cap is made from:
 *   own_i  = own_priority[i], or priority[own_first + i] when own_priority is NULL
 *   qa_k   the rule's q_k: the minimum over every counting pair
 *   qy_k   the minimum over the counting pairs with priority[j] >= own_i; with priority NULL, qy_k == qa_k
 *   gap_k  = sqrtf(qy_k) feeds s_k, z_k, r_k and lim_k exactly as in the rule; gap[k*B + i] = gap_k
 *   gapa_k = sqrtf(qa_k) feeds the hold only; gap_all[k*B + i] = gapa_k when given
 * Larger wins; equal priorities both count (today's behaviour). A track that must always count -- a person, a pallet,
 * a robot outside the scheme -- gets INT_MAX: that is the caller's duty. Priorities are meant for crossings. In one
 * lane a high-priority follower behind a low-priority leader is not slowed by the leader and ends in a hold behind
 * it; a caller who does not want that gives a convoy one priority.
 * Standing robots. A robot with held[i] != 0 on entry takes pose[0..1][i] as its position at every stage, as a reset
 * robot does: it stands. It keeps the iterate's direction h_k, which a reset robot (h_k = 0) does not have; so
 * "stands" is reset || held and "has no direction" is reset. The map lookup of a held robot stays at its iterate's
 * positions, the linearisation points its boxes apply to.
 * The hold, for a robot whose mode is GOTO_POSE or FOLLOW_PATH (every robot when mode is NULL):
 *   m      = min over k = 0..min(hold_stages, N) of gapa_k (fminf; +inf when nothing counts; a NaN never counts)
 *   held'  = reset[i] ? 0 : (held ? m < release_gap : m < stop_gap)
 * A robot in any other mode gets held' = 0, and with hold == 0 every robot does. A reset robot is never held: it has no
 * prediction and no direction, so it counts every track in range, behind it too; once held it would never solve, never
 * get a direction and never be released. It solves once under the writer's cap and is judged from the next cycle on.
 * The hold never writes reset (in the fp64 closed loop every solve of a released robot succeeds). One duty comes with
 * it: a held robot's carried refs stay at what they were when it was held (forwards, at least v_floor) while the robot
 * stands, so a prediction that starts from them still moves forwards for a stage or two. A robot released by the
 * hysteresis has room for that. A caller that gives a held robot a new target to get it out of a deadlock zeroes its
 * carried speed refs (nmpc_batch_state) along with setting reset; otherwise the hold takes the robot again in the cycle
 * after the reset one. The speed refs are the rows c is taken from: all NBX rows of carried for diff and omni4, row 0
 * (v_ref) for tric, whose row 1 (alpha_ref) stays.
 * held is one byte per robot, owned by the handle, 0 at first. Unlike the tracks and the guard, which are
 * configuration, it is state: a checkpoint carries it (nmpc_batch_sep_state) next to the stage table.
 * Out of scope: deadlock resolution (a head-on pair stays held and reports HELD every cycle; replanning is the fleet
 * manager's), priorities that depend on geometry, per-track radii and footprints, the capsule ABI,
 * nmpc_batch_solve_iterate's caller-held iterate, a spatial index, and any change to the solve kernels or the gate's.
 * Argument errors (NMPC_ERR_ARG), on top of the writer's: stop_gap not finite or <= 0, release_gap not finite,
 * < stop_gap or > the rule's range, hold_stages < 0, priority given with own_priority NULL and own_first < 0, a
 * guard without pose (a held robot stands at it), gap_all without a guard,
 * nmpc_batch_sep_hold before any nmpc_batch_stage_limits_from_tracks_ex call with a guard on the handle. */
#define NMPC_NODE_EV_HELD (9) /* protective hold: stop command, the mode stays, the robot did not tick */

typedef struct nmpc_sep_guard {
    const int* priority;     /* [M] device or NULL: right of way of every track; larger wins; equal: both count */
    const int* own_priority; /* [B] device or NULL: NULL reads priority[own_first + i] (needs own_first >= 0) */
    float stop_gap;          /* m, > 0: hold below this centre distance (default 0.45) */
    float release_gap;       /* m, >= stop_gap, <= the rule's range: a held robot is released at or above it
                                (default 0.55) */
    int hold_stages;         /* >= 0: the stages 0..min(hold_stages, N) form the protective field (default 4) */
    int hold;                /* default 1; 0: right of way only, nobody is held */
} nmpc_sep_guard;
int nmpc_sep_guard_default(nmpc_sep_guard* g);
/* nmpc_batch_stage_limits_from_tracks plus the guard (NULL: exactly that call) and gap_all. With a guard the call
 * reads the handle's held and leaves the qa plane on the handle for nmpc_batch_sep_hold. */
int nmpc_batch_stage_limits_from_tracks_ex(nmpc_batch* b, int B, const nmpc_tracks* tracks,
                                           const nmpc_sep_rule* sep /* NULL: defaults */,
                                           const nmpc_sep_guard* guard /* or NULL */,
                                           const nmpc_speed_map* map /* or NULL */,
                                           const nmpc_speed_rule* rule /* NULL: defaults */, const float* pose,
                                           const unsigned char* reset, const unsigned char* mask,
                                           float* vlim /* [N+1][B] or NULL */, float* gap /* [N+1][B] or NULL */,
                                           float* gap_all /* [N+1][B] or NULL */, void* stream);
/* The hold: one small launch, one lane per robot, on the qa plane the preceding _ex writer call left (the same B; a
 * robot the writer did not process has a stale plane). It updates the handle's held for the robots [0, B), writes
 * held_out [B] when given, and does nothing else: a caller of the plain ticks acts on held_out itself. mode [B] or
 * NULL (every robot is judged), reset [B] or NULL; all device. Only stop_gap, release_gap, hold_stages and hold of the
 * guard are read, and release_gap's upper bound is the writer call's to check. */
int nmpc_batch_sep_hold(nmpc_batch* b, int B, const nmpc_sep_guard* guard, const unsigned char* mode,
                        const unsigned char* reset, unsigned char* held_out /* [B] or NULL */, void* stream);
/* Attach (a copy of the struct; the priority arrays stay the caller's device memory) or detach (NULL) the guard. Both
 * clear held. While a guard and tracks are attached, nmpc_batch_node_cycle runs between the input stage and the tick:
 * (1) the export with export_own, in which a robot held on entry is a standing obstacle at its pose, like a reset one;
 * (2) the _ex writer; (3) the hold. A robot with held' != 0 then does not tick: it gets a stop command (zero cmd, u0,
 * status, qp_iter, qp_res: the values of a robot that does not solve; err and traj_out NaN), keeps the mode it had, so
 * that it resumes by itself, and reports NMPC_NODE_EV_HELD; its reset flag, iterate, carried refs, warm flag, records,
 * placement key, path window, remains and path_u stay bit for bit, and n_solved does not count it. (It is parked in
 * IDLE before the gate, whose kernels are unchanged, and its mode comes back after the tick from the handle's scratch;
 * under strict an invalid robot is ERROR before the hold and is not held; without strict an invalid held robot gets its
 * mode back and then goes to ERROR by the cycle's rule. If the cycle returns an error after the hold's launch was
 * queued -- a failed allocation or launch in the tick -- the status launch does not run and a held robot's entry of the
 * caller's mode array stays IDLE: after an error from the cycle the caller writes its modes again, as it has to after
 * any error in the middle of a cycle.) A guard without tracks attached is inert. With no guard
 * attached the cycle enqueues exactly the launches it enqueued without this interface and allocates nothing. */
int nmpc_batch_set_sep_guard(nmpc_batch* b, const nmpc_sep_guard* guard);
/* The hold's state for checkpoints: *held [capacity] device bytes, zeros at first. The call allocates the guard's
 * scratch if no call has needed it yet: held, the qa plane [N+1][capacity] and the cycle's two save arrays come in one
 * piece. nmpc_batch_export_tracks has no held operand: a caller of the plain ticks who wants a held robot exported as a
 * standing obstacle, as the cycle does, passes reset | held as the export's reset. */
int nmpc_batch_sep_state(nmpc_batch* b, unsigned char** held);

/* Per-robot model parameters. A fleet of one model family mixes vehicles: two wheelbases of the same differential
 * base, loaded and empty trucks whose tau_v differ by a factor of two or three (the reference runs one node per robot,
 * each sending its own geometry and time constants through {name}_acados_update_params, NMPCNavControlDiff.cpp:44-46,
 * NMPCNavControlROS.cpp:96-110,164-176,234-259). The handle therefore owns a third device table, the model table:
 * [NP][capacity], fp32, instance-minor, row j = every robot's p[j] (diff {b, tau_v}, omni4 {l1 + l2, tau_v}, tric
 * {d, tau_v, tau_a}); 8 or 12 bytes per robot. It is allocated by the first nmpc_batch_set_robot_model call and starts
 * with the handle's own p in every column (the fp32 values the kernels take from nmpc_model_params).
 * Rules:
 *   - While the table is on, every launch of the handle -- nmpc_batch_solve, _solve_iterate, _run, _run_path,
 *     _follow_path and both node ticks -- takes robot i's p from column i wherever it read the handle's p: the RK4
 *     linearisation and its sensitivities, the constant rows of the stage Jacobian, run mode's direct kinematics of
 *     the measured velocity, and the inverse kinematics of the command. nmpc_batch_set_params' p then reaches no
 *     launch (it is what a table allocated or cleared later starts from). dt, dt_ctrl, the QP options, terminal_hack
 *     and tric_sin_bug stay with the handle.
 *   - While it is off (never written, or after nmpc_batch_clear_robot_model) every launch computes exactly what it
 *     computed without this interface.
 *   - The three tables are independent: any combination of them being on or off is legal.
 *   - The writer is one small launch on `stream`, with no host synchronisation and no host-side validation. Warm
 *     flags are left alone when a column changes.
 *   - A NaN or a zero in a parameter fails that robot alone with status 1, through the NaN its dynamics then
 *     produce; no other robot changes. The robot keeps its iterate and carried refs and gets a stop command, as after
 *     any failed solve.
 *   - The harness plant (nmpc_fleet_sim_step, _step_renew) reads the robot's column too while the table is on, in
 *     its RK4 step and in the velocity it measures, so the closed loop simulates the vehicle the controller models.
 *   - Out of scope: per-robot dt and QP options, parameters that vary along the horizon, and the capsule ABI, which
 *     keeps one p per capsule and keeps rejecting stage-varying parameters.
 * Argument errors (NMPC_ERR_ARG): B out of range, p NULL, a NULL handle. */
/* Write the columns of robots [0, B) where mask[i] != 0 (mask [B] device, NULL: all) from p [NP][B] (device). */
int nmpc_batch_set_robot_model(nmpc_batch* b, int B, const float* p, const unsigned char* mask, void* stream);
/* The table's device view for checkpoints: *table [rows][stride] (rows = NP, stride = capacity), or NULL while the
 * table is off. Each output may be NULL. */
int nmpc_batch_robot_model(nmpc_batch* b, float** table, int* rows, int* stride);
/* Turn the model table off: launches use the handle's p again. The next writer call starts a fresh table from the
 * handle's p. (Host-side switch: it applies to the launches enqueued after it.) */
int nmpc_batch_clear_robot_model(nmpc_batch* b);

/* Per-robot map frames. x and y are fp32 from the inputs to the stored iterate, so in absolute map coordinates the
 * 1e-3 parity holds up to 64 m from the map origin only (nmpc_batch_run above), and at 4.6e6 m, a projected map
 * coordinate, an fp32 position has an ulp of half a metre. The SQP-RTI step is translation-covariant in exact
 * arithmetic: no model's f reads x or y, the position rows of the stage Jacobian are the identity and no bound touches
 * x or y, so a solve whose iterate, x0 and references are all relative to a point near the robot is the solve the
 * reference does, at fp32's full resolution. The handle therefore owns a fourth device table, the frame
 * table: [2][capacity], fp64, instance-minor, row 0 every robot's origin x and row 1 its origin y, in map coordinates;
 * 16 bytes per robot. It is allocated by the first nmpc_batch_set_robot_frame or nmpc_batch_recentre call and starts
 * with the origin (0, 0) in every column.
 * Rules:
 *   - While the table is on, every fp32 position of every launch of the handle is in robot i's frame, map coordinate
 *     minus origin i: as inputs pose x and y, traj x and y, goal x and y, solve mode's x0 rows 0 and 1 and yref
 *     components 0 and 1; as outputs x1, xtraj and traj_out; and the resident iterate's position rows
 *     (nmpc_batch_state). Headings, velocities, the carried refs, u0, cmd, the multipliers and the other three tables
 *     are unaffected.
 *   - Every fp64 path quantity stays in map coordinates: the nmpc_path_segment coefficients, near, and the path
 *     parameter. The launches that read segments -- nmpc_batch_run_path, _follow_path and both node ticks -- bridge
 *     the two in fp64: the nearest-point search and the path errors take the robot at (double)pose + origin, the
 *     end-of-trajectory test compares that map position with the fp64 last pose, and every reference pose the march
 *     emits becomes (float)(p - origin), for the solve and for traj_out: one fp64 subtraction, then the one rounding
 *     it had. GoToPose compares goal and pose, both in the frame, as before.
 *   - nmpc_batch_run, _solve and _solve_iterate read nothing new: their inputs are frame values by contract. A reset
 *     (reset[i] = 1) or nmpc_batch_init_iterate puts the iterate at the frame origin, which is the point: the first
 *     solve's primal step is then the robot's distance from its origin, not from the map's. This departs from the
 *     reference, whose {name}_acados_create / _reset leave the iterate at the map origin, as qp_warm_start departs
 *     from its cold IPM start; by the covariance above it is the solve the reference would do in exact arithmetic.
 *   - While it is off (never written, or after nmpc_batch_clear_robot_frame) every launch computes exactly what it
 *     computed without this interface, bit for bit.
 *   - The four tables are independent: any combination of them being on or off is legal.
 *   - Each writer is one small launch on `stream`, with no host synchronisation and no host-side validation (a NaN
 *     origin gives that robot NaN positions and fails it alone, with status 1, as a NaN input does).
 *   - Placing a robot somewhere new: set its frame, then reset it (reset[i] = 1) or nmpc_batch_init_iterate.
 *   - Out of scope: the capsule ABI (its iterate travels with the caller and keeps map coordinates);
 *     nmpc_batch_solve_iterate's caller-held iterate (nmpc_batch_set_robot_frame moves the resident one only); the
 *     harness plant (nmpc_fleet_sim_step* works on whatever fp32 positions it is given, under a frame those are frame
 *     values, and it does not follow a changing origin); rotated frames. nmpc_path_nearest and nmpc_path_discretize
 *     take no handle and stay in map coordinates.
 * Argument errors (NMPC_ERR_ARG): B out of range, a NULL payload (origin, pose_map, map / in / out), n < 0, c < 2, a
 * NULL handle. radius is not an argument error: a NaN or +inf radius moves nothing. */
/* Write the origins of robots [0, B) where mask[i] != 0 (mask [B] device, NULL: all) from origin [2][B] (device, fp64),
 * and in the same launch move those robots' resident iterate so that its map position does not change: the x and y
 * row of every stage becomes (float)((double)x + (o_old - o_new)). Nothing else of the robot changes: warm flag,
 * scratch records, carried refs, ubar, the other rows of xbar, the placement key. */
int nmpc_batch_set_robot_frame(nmpc_batch* b, int B, const double* origin, const unsigned char* mask, void* stream);
/* The same launch with a computed origin, which keeps a long-running robot near its origin without a host decision:
 * pose_map [2 or 3][B] (device, fp64; rows 0 and 1 are read) is every robot's map position. A masked robot with
 * max(|x_map - o_x|, |y_map - o_y|) > radius gets the origin (rint(x_map), rint(y_map)), whole metres, its iterate
 * moves as above and moved[i] = 1; every other robot gets moved[i] = 0 and is untouched (moved [B] device, or NULL). A
 * non-finite position, or a NaN radius, moves nothing. */
int nmpc_batch_recentre(nmpc_batch* b, int B, const double* pose_map, double radius, const unsigned char* mask,
                        unsigned char* moved, void* stream);
/* Map coordinates into the robots' frames and back, for arrays [n][c][B] (device): components 0 and 1 of each group of
 * c become (float)(v - origin) / (double)v + origin, the others are only converted. (n, c) = (1, 3) for pose and goal,
 * (N+1, 3) for traj and traj_out, (1, NX) for x0 and x1, (N+1, ny_in) for yref, (N+1, NX) for xtraj. While the table
 * is off the origin is (0, 0). */
int nmpc_batch_to_frame(nmpc_batch* b, int B, const double* map, int n, int c, float* out, void* stream);
int nmpc_batch_from_frame(nmpc_batch* b, int B, const float* in, int n, int c, double* map, void* stream);
/* The table's device view for checkpoints: *table [2][stride] fp64 (stride = capacity), or NULL while the table is
 * off. Each output may be NULL. Restore it before the iterate, which is relative to it. */
int nmpc_batch_robot_frame(nmpc_batch* b, double** table, int* stride);
/* Move every robot's iterate back to map coordinates (the writer with origin 0 for the whole capacity, one launch on
 * `stream`), then turn the table off: the launches enqueued after it take every position as a map coordinate again.
 * The next writer call starts a fresh table of zero origins. */
int nmpc_batch_clear_robot_frame(nmpc_batch* b, void* stream);

/* Record layout of the team kernel's single-direction scratch records, a per-handle choice fixed at create time
 * and changed only by this call (never by other handles):
 *   NMPC_REC_WIDE   one 64-B record per lane and stage (diff's default alone on a device: the metric fleet's
 *                   107 MB fit the Infinity Cache, and the issue-bound kernel is 1.2 % faster with it);
 *   NMPC_REC_SPLIT  core and bound planes (tric always; diff beside other resident fleets: the mixed fleet's
 *                   272 MB drop under the 256 MB Infinity Cache, 5.25 -> 5.70 M it/s);
 *   NMPC_REC_AUTO   the model's choice from this handle alone: tric SPLIT, omni4 WIDE, diff SPLIT when its own
 *                   records (capacity x (N+1) x 640 B) exceed 192 MB, else WIDE.
 * diff accepts all three; tric only SPLIT / AUTO and omni4 only WIDE / AUTO (NMPC_ERR_UNSUPPORTED otherwise). The
 * environment variable NMPC_AMD_REC_SPLIT (0 / 1) overrides the create-time choice (A/B runs). Changing the layout
 * leaves every robot's warm flag in place: each robot starts its next IPM cold because its tag no longer matches. */
#define NMPC_REC_AUTO (-1)
#define NMPC_REC_WIDE 0
#define NMPC_REC_SPLIT 1
int nmpc_batch_set_record_layout(nmpc_batch* b, int layout);

/* The warm-start rule the solve kernels apply (the parameters after the NMPC_AMD_WARM / NMPC_AMD_WARM_ITER_MAX
 * overrides): a robot's flag is set after a solve iff warm && status == 0 && iterations < iter_max &&
 * iterations <= warm_iter_max. Hosts that mirror the device flags (the capsule shim) use this, not their copy of
 * the parameters. Each output may be NULL. */
int nmpc_batch_warm_rule(const nmpc_batch* b, int* warm, int* warm_iter_max, int* iter_max);

/* The launch a call of B robots makes on this handle (nmpc_batch_plan_ex; nmpc_batch_plan: a solve launch):
 *   kernel          0 = k_sqp_rti_team (four robots per wave), 1 = k_sqp_rti_rowpar;
 *   waves_per_robot the row-parallel kernel's waves per robot (0 for the team kernel);
 *   segments        its horizon segments (0 = the serial phases, or the team kernel);
 *   record_layout   NMPC_REC_WIDE / NMPC_REC_SPLIT: the scratch record layout of the launch;
 *   warm_tag        the NMPC_WARM_TAG_* the launch reads and writes (nmpc_batch_warm_state);
 *   record_bytes    this handle's records touched per sweep over its capacity (the NMPC_REC_AUTO measure).
 * mode: NMPC_PLAN_SOLVE (nmpc_batch_solve / _solve_iterate), NMPC_PLAN_RUN (nmpc_batch_run: run mode keeps the
 * reference poses in LDS, which can push a long horizon off the row-parallel kernel) or NMPC_PLAN_RUN_PATH
 * (nmpc_batch_run_path: always the team kernel). */
#define NMPC_PLAN_SOLVE 0
#define NMPC_PLAN_RUN 1
#define NMPC_PLAN_RUN_PATH 2
typedef struct nmpc_launch_plan {
    int kernel, waves_per_robot, segments, record_layout, warm_tag;
    size_t record_bytes;
} nmpc_launch_plan;
int nmpc_batch_plan_ex(const nmpc_batch* b, int B, int mode, nmpc_launch_plan* plan);
int nmpc_batch_plan(const nmpc_batch* b, int B, int* kernel, int* waves_per_robot, int* segments);

/* The team kernel's hand-off iteration C of this handle: 0 = off, the create-time value; NMPC_HANDOFF_AUTO = the
 * measured default, C = 16 (the best of 10, 12, 14, 16 on the metric launch, diff N = 40 with 4096 robots: +5.4 %
 * same-box); the environment variable NMPC_AMD_HANDOFF overrides the create-time value (A/B runs). It is off at
 * create because a handed-over robot's result is the segmented kernel's, equal to the plain kernel's only within
 * the bars below: whoever owns several handles of one fleet (other layouts, stream groups) sets all of them alike, as
 * nmpc_nav_control_amd/fleet.py does for a diff fleet alone on the device. A team-kernel launch that qualifies runs k_sqp_rti_team_ho: a robot whose IPM has
 * not stopped at the top of iteration C leaves the four-robots-per-wave loop there, and one wave of its block finishes
 * it alone in the segmented form, four horizon segments on the wave's four rows, inside the same launch. The rule
 * looks at the robot's own iteration count only. The iteration count, the warm rule and the stopping rule count both
 * parts as one solve; a robot that was handed over ends with the segmented kernel's arithmetic (status equal, IPM
 * count within a few iterations, u0 within the fp32 bars of the row-parallel kernel). A launch qualifies with the
 * single-direction IPM, in solve and run mode (not run_path), unsplit and with at most one wave per SIMD, N a multiple
 * of 4 with N >= 8, diff or tric, diff's wide records, every per-robot table off and the block's LDS (four resume
 * slices) within the device's; every other launch keeps the plain kernel. C >= qp_iter_max hands nobody over.
 * nmpc_batch_plan_handoff reports the decision for a launch of B robots (mode: NMPC_PLAN_*): iteration = C or 0,
 * segments = the resumed form's horizon segments or 0, lds_bytes = the block's LDS or 0. Each output may be NULL.
 * nmpc_batch_plan_ex describes the same launch as the team kernel (kernel 0); its record_layout and warm_tag are the
 * hand-off launch's (wide). */
#define NMPC_HANDOFF_AUTO (-1)
int nmpc_batch_set_handoff(nmpc_batch* b, int iteration);
int nmpc_batch_plan_handoff(const nmpc_batch* b, int B, int mode, int* iteration, int* segments, size_t* lds_bytes);

/* Bench / test harness: closed-loop plant step and path-reference regeneration for B robots
 * (see DESIGN.md "Synthetic closed loop"). All device pointers, [field][B]:
 *   path [6][B] = {x0, y0, th0, kappa, speed, length} circular-arc paths; goal-pose robots have length < 0
 *   and {x0, y0, th0} is the goal. s [B] arc-length progress (in/out). pose/vel/steer in/out: advanced by
 *   one RK4 step of the plant with the applied input u0 [NU][B]; traj [N+1][3][B], traj_len [B] out. */
int nmpc_fleet_sim_step(nmpc_batch* b, int B, const float* path, float* s, float* pose, float* vel, float* steer,
                        const float* u0, const int* status, float* traj, int* traj_len, int advance, void* stream);

/* Stationary closed loop (bench / test harness): the fleet manager issues a robot a new goal or path when it
 * has arrived (the end-of-trajectory test of processGoToPose / processFollowPath, NMPCNavControlROS.cpp:637-643 /
 * :682-693, with |heading error|) or when its current one has been active for `ttl` ticks, and the node resets
 * the controller as its goal / path callbacks do (reset_mpc -> {name}_acados_reset, NMPCNavControlROS.cpp:304-327):
 * `reset` [B] is set for the next nmpc_batch_run. A new target depends only on (seed, start + robot index, event
 * count) and the robot's pose: draw j of event e is u = (h >> 8) / 2^24 with h = nmpc_fleet_hash(seed,
 * global index, 16 e + j) (the same 32-bit integer hash on host and device), so any sharding or stream grouping
 * issues the same targets. Goal robots (path length < 0) get a goal at distance U(goal_r_lo, goal_r_hi) in a
 * uniform direction with a uniform heading; path robots an arc starting within 0.2 m / 0.3 rad of the robot
 * (curvature U(-kappa_max, kappa_max), speed U(speed_lo, speed_hi), length U(len_lo, len_hi)), progress s = 0.
 * The new ttl is ttl_min + ((h >> 8) * (ttl_max - ttl_min + 1) >> 24).
 * `stats` (optional) accumulates the statistics of the solve that preceded this step in the same launch, before the
 * renewal rewrites `reset` (so `cold_*` count the solves that ran with reset set): */
typedef struct nmpc_fleet_stats {
    const int* qp_iter;         /* [B] in: the solve's executed IPM iterations */
    long long* iters_sum;       /* [B] += qp_iter */
    int* iters_max;             /* [B] = max(iters_max, qp_iter) */
    long long* fail_cnt;        /* [B] += (status != 0) */
    long long* hist;            /* [64] += robots per executed iteration count (clamped to [0, 63]) */
    long long* cold_cnt;        /* [B] += reset */
    long long* cold_iters;      /* [B] += reset * qp_iter */
} nmpc_fleet_stats;
typedef struct nmpc_fleet_renew {
    unsigned int seed;
    int start;                  /* global index of robot 0 of this call */
    int ttl_min, ttl_max;       /* ticks a goal / path stays active (inclusive range) */
    float goal_r_lo, goal_r_hi; /* m */
    float kappa_max, speed_lo, speed_hi, len_lo, len_hi;
    float pos_tol, ang_tol;     /* final_position_error (m) / final_orientation_error (rad), nmpc_nav_control.yaml:6-7 */
    int* ev;                    /* [B] events so far (in/out) */
    int* ttl;                   /* [B] ticks left (in/out) */
    unsigned char* reset;       /* [B] in: the flags the last solve ran with; out: 1 where this step issued a new
                                 * goal / path */
    const nmpc_fleet_stats* stats; /* NULL: no statistics (every pointer of a given one is required, and status) */
} nmpc_fleet_renew;
int nmpc_fleet_sim_step_renew(nmpc_batch* b, int B, float* path, float* s, float* pose, float* vel, float* steer,
                              const float* u0, const int* status, float* traj, int* traj_len,
                              const nmpc_fleet_renew* renew, void* stream);
/* The harness hash: lowbias32(lowbias32(lowbias32(seed ^ 0x9e3779b9) + index) + counter) (uint32 arithmetic). */
unsigned int nmpc_fleet_hash(unsigned int seed, unsigned int index, unsigned int counter);

const char* nmpc_last_error(void);
const char* nmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif
