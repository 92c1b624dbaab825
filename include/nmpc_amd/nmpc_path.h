/*
 * nmpc_path.h -- batched reference-pose generation on the device (libnmpc_amd.so), C ABI.
 *
 * nmpc_path_discretize is PathDiscretizer::getNextNPoses (src/nmpc_nav_control/PathDiscretizer.cpp:14-63,
 * include/nmpc_nav_control/PathDiscretizer.h:12-51) for B robots in one launch: the step the reference runs
 * per robot on the CPU right before NMPCNavControl*::run (NMPCNavControlROS.cpp:669-681). Its output is the
 * traj argument of nmpc_batch_run (nmpc_batch.h), so a path-following tick never leaves the GPU.
 *
 * The parametric path segments (parametric_trajectories_common::TPath) come from a library the reference does
 * not vendor; nmpc_path_segment restates the interface PathDiscretizer uses (GetX/GetY/GetDX/GetDY/GetTheta/
 * GetThetaHolomonic/GetVelocity) as cubic polynomials in the segment parameter u in [0, 1]:
 *   GetX(u) = x[0] + x[1] u + x[2] u^2 + x[3] u^3      (Horner order, no fused multiply-add)
 *   GetY(u) likewise with y[], GetThetaHolomonic(u) likewise with th[]
 *   GetDX(u), GetDY(u): the derivatives; GetTheta(u) = atan2(GetDY(u), GetDX(u)); GetVelocity() = v.
 * Lines, cubic Bezier / Hermite curves and polynomial approximations of arcs all fit this form.
 *
 * Conventions as in nmpc_batch.h: DEVICE pointers, asynchronous on `stream` (hipStream_t, NULL = default),
 * 0 on success or < 0 with nmpc_last_error().
 */
#ifndef NMPC_AMD_NMPC_PATH_H
#define NMPC_AMD_NMPC_PATH_H

#ifdef __cplusplus
extern "C" {
#endif

/* One parametric path segment (128 bytes). */
typedef struct nmpc_path_segment {
    double x[4];  /* GetX(u) coefficients, ascending powers of u */
    double y[4];  /* GetY(u) */
    double th[4]; /* GetThetaHolomonic(u) */
    double v;     /* GetVelocity(): signed segment speed; v < 0 drives the segment backwards (theta + pi) */
    double reserved[3];
} nmpc_path_segment;

/* getNextNPoses for robots [0, B):
 *   segs       [B][seg_stride] segments; robot i's path list is segs[i*seg_stride .. i*seg_stride+nseg[i]-1]
 *   nseg       [B] segments per robot (>= 1)
 *   nearest_u  [B] path parameter of the robot's nearest point (integer part = segment index)
 *   sample_period, num_poses, is_holonomic: the PathDiscretizer constructor arguments (num_poses <= 8192)
 *              (PathDiscretizer.cpp:5-12; the ROS node passes dt, N+1, false: NMPCNavControlROS.cpp:669)
 * outputs (either may be NULL):
 *   traj       [num_poses][3][B] float {x, y, theta}: the traj input of nmpc_batch_run
 *   traj64     [num_poses][3][B] double, the same poses unrounded
 * Differences from the reference, all on inputs where it is undefined: the segment index of the first
 * velocity lookup is clamped to [0, nseg-1] (PathDiscretizer.cpp:23 indexes without a check), a NaN path
 * parameter selects segment 0, and a robot stops after 65536 loop steps (the reference loop has no cap;
 * a non-degenerate path needs about 10 steps per pose). */
int nmpc_path_discretize(int B, const nmpc_path_segment* segs, int seg_stride, const int* nseg,
                         const double* nearest_u, double sample_period, int num_poses, int is_holonomic,
                         float* traj, double* traj64, void* stream);

/* Each robot's nearest path point: the step that produces nearest_u, processNearestPoint (NMPCNavControlROS.cpp:
 * 597-610) with the path errors of :654-657, for robots [0, B) in one launch.
 *
 * The reference calls TPathProcessMinDist(10, 0.01)::GetMinDist of parametric_trajectories_common, which it does
 * not vendor: that search's tolerance and tie rule cannot be read. The search rule here is THIS PROJECT'S OWN:
 *   path parameter U in [0, n], n = nseg[i]; segment k = min(floor(U), n-1), local parameter u = U - k;
 *   P(U) = (GetX(u), GetY(u)) of segment k; r = (pose x, pose y) widened from fp32 exactly
 *   search range [lo, hi]: [0, n] without u_range, else u_range's bounds clamped into [0, n]; a NaN bound leaves
 *     that side open; lo > hi is read as hi = lo
 *   nearest_u = the U in range that minimises |P(U) - r| in fp64: |P(nearest_u) - r| <= d_min + 1e-9 m on
 *     metre-scale paths (measured 1e-15); ties go to the smallest U; the same inputs give the same bits whatever
 *     B and the robot's slot.
 * Arguments:
 *   segs, seg_stride, nseg  as nmpc_path_discretize (an nseg[i] above seg_stride is read as seg_stride)
 *   pose       [3][B] float {x, y, theta}
 *   u_range    [2][B] {lo, hi} or NULL
 *   holonomic_heading  heading of the orientation error: != 0 theta_holonomic (the node: omni4, :654), 0 theta,
 *              plus pi when the segment of nearest_u has v < 0 (:655)
 * outputs:
 *   nearest_u  [B]
 *   near       [4][B] {x, y, theta, theta_holonomic} at nearest_u or NULL: GetMinDist's raw outputs, theta =
 *              atan2(GetDY, GetDX) without the reverse-driving pi
 *   err        [2][B] {pos_error_to_path, ori_error_to_path} or NULL: sqrt(dx^2 + dy^2) and
 *              |normAngRad(heading - pose theta)| (:656-657, utils.h:41-47)
 * Undefined inputs: a NaN (or infinite) pose or coefficient gives nearest_u = lo and err = NaN; nseg[i] < 1 gives
 * nearest_u = 0, near = err = NaN and reads no segment; a segment whose derivative is zero everywhere is one
 * candidate point. No loop depends on the data. */
int nmpc_path_nearest(int B, const nmpc_path_segment* segs, int seg_stride, const int* nseg, const float* pose,
                      const double* u_range, int holonomic_heading, double* nearest_u, double* near, double* err,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NMPC_AMD_NMPC_PATH_H */
