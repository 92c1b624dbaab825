// nmpc_batch.cpp -- C ABI of the batched solve path (include/nmpc_amd/nmpc_batch.h).
#include "nmpc_amd/nmpc_batch.h"
#include "nmpc_amd/nmpc_path.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "nmpc_kernels.hpp"
#include "nmpc_trace.hpp"

using namespace nmpc;

// One per-robot device table of a handle (DESIGN.md "Per-robot device tables"): off until its first writer, which
// allocates it and fills it with what the launches used until then (table_ready); nmpc_batch_clear_* switches it off
// and keeps the allocation for the next writer, which refills it. Sized in floats; the frame table's doubles count as
// two each and are reached through view64 / p64 (a device allocation is aligned for either)
struct DevTable {
    float* p = nullptr;
    size_t floats = 0;  // its size, fixed at create
    bool on = false;    // launches read it
    float* view() const { return on ? p : nullptr; }  // what launches and the view functions see
    double* p64() const { return reinterpret_cast<double*>(p); }
    double* view64() const { return on ? p64() : nullptr; }
};

struct nmpc_batch {
    nmpc_model_params prm;
    KParams kp;
    int capacity;
    int nx, nu, nbx, nbu, ny;
    float* xbar = nullptr;
    float* ubar = nullptr;
    float* carried = nullptr;
    float* scratch = nullptr;
    int sched = NMPC_SCHED_AUTO;
    int n_simd = 1024;           // SIMDs of the device (4 per CU)
    int n_cu = 256;              // CUs of the device and LDS bytes per CU (MI355X: 256, 160 KiB; read at create)
    size_t lds_per_cu = 163840;
    int split_max = 256;         // team-kernel launches of at most this many robots run one block per robot (split)
    // launches of at most this many robots (single-direction IPM, not run_path) run k_sqp_rti_rowpar (DESIGN.md
    // section 4): four waves per robot up to 256 robots; above, rowpar_w waves per robot and there only with
    // segments, all on the first wave's four rows (the second wave takes half of the stage-parallel phases; segments
    // on both waves of a SIMD's two resident waves contend: diff N = 40 B = 1024 1.15 M it/s on the team kernel ->
    // 1.57 M on one wave per robot -> 1.65 M on two, 1.52 M with 5 segments over both; profiles/r04/ab/seg.txt)
    int rowpar_max = 1024;
    int rowpar_w = 2;  // (NMPC_AMD_ROWPAR_W=1 for A/B)
    // horizon segments of the row-parallel kernel (sqp_rti_rowpar.hip SEG): -1 = chosen per launch (seg_count),
    // 0 = the serial phases B / C, S > 0 = S segments when N % S == 0 (NMPC_AMD_SEG overrides)
    int seg = -1;
    // rows that may hold a segment above 256 robots: the first wave's 4 (NMPC_AMD_SEG_ROWS = 8: both waves, A/B)
    int seg_rows = 4;
    int* iter_key = nullptr;     // [capacity] last executed IPM iterations per robot (written by the team kernel)
    int* order = nullptr;        // [capacity] team slot -> robot
    unsigned char* warm = nullptr;  // [capacity] the robot's last solve succeeded: its scratch records hold its
                                    // multipliers (IPM warm start)
    int* sorted = nullptr;       // [capacity] sort scratch
    // the team kernel's single-direction record layout (NMPC_REC_WIDE / NMPC_REC_SPLIT), fixed per handle: resolved
    // at create time from this handle alone and changed only by nmpc_batch_set_record_layout
    int rec_split = 0;
    // the team kernel's hand-off iteration C (nmpc_batch_set_handoff; NMPC_AMD_HANDOFF overrides at create, A/B runs):
    // launches that qualify (plan_launch) run k_sqp_rti_team_ho, whose teams leave the team loop unfinished at the top
    // of IPM iteration C and are finished one robot per wave in the segmented form. 0: off, the create-time
    // value: a handed-over robot ends with the segmented kernel's arithmetic, and the handles of one fleet in different
    // layouts or groupings are held to each other bit for bit, so the owner of the fleet turns it on, for all of them
    // (fleet.py, as for the record layout). NMPC_HANDOFF_AUTO: the measured default kHandoffDefault
    int handoff = 0;
    double* path_err = nullptr;  // [2][capacity] path errors of nmpc_batch_follow_path when the caller keeps none
                                 // (allocated at the first such call)
    // node ticks (nmpc_batch_node_tick), allocated at the first one: the gate's reference poses [N+1][3][capacity]
    // and their lengths, the robots that solve (active [capacity], their count node_n [1]) and a status array for
    // callers that keep none
    float* node_traj = nullptr;
    int* node_len = nullptr;
    unsigned char* node_active = nullptr;
    int* node_n = nullptr;
    int* node_status = nullptr;
    // the per-robot device tables, read by the launches (resident_args) while they are on:
    // bounds and weights (nmpc_batch_set_robot_params), [rp.off[kRpFields]][capacity];
    // stage-varying bounds (nmpc_batch_set_stage_bounds), (N + 1) * sb_rows * capacity floats (sb_at, nmpc_kernels.hpp);
    // model parameters (nmpc_batch_set_robot_model), [np][capacity], which the harness plant reads too (fleet_sim);
    // map frames (nmpc_batch_set_robot_frame), fp64 [2][capacity]: every robot's origin x, then y
    DevTable rparams, sbounds, rmodel, rframe;
    RpRows rp{};
    int np = 0;
    // the node's input state (nmpc_batch_enable_input; in_depth 0: off): every robot's sample ring and held values,
    // and the buffers that carry the stage's outputs to the tick when the caller keeps none (pose, vel, goal [3][B],
    // steer, valid [B], each allocated for the capacity)
    NodeInputState in_st{};
    float *in_pose = nullptr, *in_vel = nullptr, *in_goal = nullptr, *in_steer = nullptr;
    unsigned char* in_valid = nullptr;
    // the attached speed map and its rule (nmpc_batch_set_speed_map; smap_on false: none): the cycle's writer reads them
    nmpc_speed_map smap{};
    nmpc_speed_rule srule{};
    bool smap_on = false;
    // fleet separation (nmpc_batch_set_tracks; trk_on false: none attached): the attached tracks and rule, whether the
    // cycle exports the handle's own robots, and the writer's scratch, allocated at its first call: the q plane
    // [N+1][capacity] and the track boxes [4][sep_boxes_m]
    nmpc_tracks trk{};
    nmpc_sep_rule seprule{};
    bool trk_on = false, trk_export = false;
    float* sep_q = nullptr;
    double* sep_boxes = nullptr;
    int sep_boxes_m = 0;
    // the separation guard (nmpc_batch_set_sep_guard; sguard_on false: none attached) and its scratch, allocated by the
    // first call that needs it: the qa plane [N+1][capacity] (sep_qa_ready: a guarded writer call has filled it), the
    // hold's state held [capacity], and the cycle's saved modes and remains [capacity] of the parked robots
    nmpc_sep_guard sguard{};
    bool sguard_on = false, sep_qa_ready = false;
    float* sep_qa = nullptr;
    unsigned char *sep_held = nullptr, *sep_mode_save = nullptr;
    double* sep_remains_save = nullptr;
};

namespace {

thread_local std::string g_err;

int set_err(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

int hip_err(hipError_t e, const char* what)
{
    if (e == hipSuccess) return NMPC_OK;
    return set_err(NMPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The one model switch: f(M{}) with the model's type (nmpc_models.hpp), whose result every M must give in one type.
// The id was checked (dims_of) wherever it came from outside
template <class F>
auto with_model(int model, F&& f)
{
    switch (model) {
    case NMPC_MODEL_DIFF2AMR: return f(Diff2{});
    case NMPC_MODEL_OMNI4AMR: return f(Omni4{});
    default: return f(Tric3{});
    }
}

bool dims_of(int model, int* nx, int* nu, int* nbx, int* nbu, int* np)
{
    if (model != NMPC_MODEL_DIFF2AMR && model != NMPC_MODEL_OMNI4AMR && model != NMPC_MODEL_TRIC3AMR) return false;
    with_model(model, [&](auto m) {
        using M = decltype(m);
        *nx = M::NX; *nu = M::NU; *nbx = M::NBX; *nbu = M::NBU; *np = M::NP;
    });
    return true;
}

KParams to_kparams(const nmpc_model_params& p, int nx, int nu, int nbx, int nbu)
{
    KParams k;
    std::memset(&k, 0, sizeof(k));
    k.N = p.N;
    k.dt = (float)p.dt;
    k.dt_ctrl = (float)p.dt_ctrl;
    for (int i = 0; i < 3; i++) k.p[i] = (float)p.p[i];
    for (int i = 0; i < nbx; i++) { k.lbx[i] = (float)p.lbx[i]; k.ubx[i] = (float)p.ubx[i]; }
    for (int i = 0; i < nbu; i++) { k.lbu[i] = (float)p.lbu[i]; k.ubu[i] = (float)p.ubu[i]; }
    for (int i = 0; i < nx + nu; i++) k.W[i] = (float)p.W[i];
    for (int i = 0; i < nx; i++) k.We[i] = (float)p.W_e[i];
    k.terminal_hack = p.terminal_hack;
    k.sin_bug = p.tric_sin_bug;
    k.iter_max = p.qp_iter_max;
    k.tol_stat = (float)p.qp_tol_stat;
    k.tol_ineq = (float)p.qp_tol_ineq;
    k.tol_comp = (float)p.qp_tol_comp;
    k.mu0 = (float)p.qp_mu0;
    k.thr0 = (float)p.qp_thr0;
    k.tau = (float)p.qp_tau;
    k.ipm = p.qp_ipm;
    k.sd_lo = (float)p.qp_sigma_lo;
    k.sd_hi = (float)p.qp_sigma_hi;
    // same-box A/B overrides (tools/ab_env.py): the IPM rule and its sigma clamp
    if (const char* v = std::getenv("NMPC_AMD_IPM")) {  // single | mehrotra
        if (!std::strcmp(v, "single")) k.ipm = NMPC_IPM_SINGLE;
        else if (!std::strcmp(v, "mehrotra")) k.ipm = NMPC_IPM_MEHROTRA;
    }
    if (const char* v = std::getenv("NMPC_AMD_SIGMA_LO")) k.sd_lo = std::strtof(v, nullptr);
    if (const char* v = std::getenv("NMPC_AMD_SIGMA_HI")) k.sd_hi = std::strtof(v, nullptr);
    k.warm = p.qp_warm_start;
    k.warm_kappa = (float)p.qp_warm_kappa;
    if (const char* v = std::getenv("NMPC_AMD_WARM")) k.warm = std::atoi(v) != 0;
    if (const char* v = std::getenv("NMPC_AMD_WARM_KAPPA")) k.warm_kappa = std::strtof(v, nullptr);
    k.warm_iter_max = p.qp_warm_iter_max > 0 ? p.qp_warm_iter_max : p.qp_iter_max;
    if (const char* v = std::getenv("NMPC_AMD_WARM_ITER_MAX")) k.warm_iter_max = std::atoi(v);
    k.infeas_lam = p.qp_infeas_lambda > 0.0 ? (float)p.qp_infeas_lambda : INFINITY;
    k.wmax = 0.0f;
    for (int i = 0; i < nx + nu; i++) k.wmax = std::fmax(k.wmax, (float)p.W[i]);
    return k;
}

size_t scratch_floats(int model, int N, int stride)
{
    return with_model(model, [&](auto m) { return team_scratch_floats<decltype(m)>(N, stride); });
}

template <class M>
hipError_t launch_m(nmpc_batch* b, const KArgs& a, int mode, hipStream_t s)
{
    if (a.rowpar) return launch_sqp_rti_rowpar<M>(b->kp, a, mode, s);
    if (a.stage_in_n > 0 || a.stage_out_n > 0) return hipErrorInvalidValue;  // (only the row-parallel kernel stages)
    if (a.handoff > 0) return launch_sqp_rti_team_ho<M>(b->kp, a, mode, s);
    return launch_sqp_rti_team<M>(b->kp, a, mode, s);
}

// Segments of the row-parallel kernel's Riccati sweeps for a horizon N on `rows` rows per robot: the divisor S of N
// (S <= rows, <= kSegMax) that minimises the robot's chain per IPM iteration, N / S stage steps of the segments'
// sweeps (backward 2.4 k + forward 1.2 k cycles) plus S - 1 master steps (5 k cycles, 1.4 stage steps; diag stamps,
// profiles/r04/stamps/); 0 (the serial phases) when no S > 1 divides N. N = 80 -> 8, N = 40 -> 5 (4 on one wave)
inline int seg_count(int N, int rows)
{
    int best = 0;
    double cost = (double)N;
    for (int S = 2; S <= rows && S <= kSegMax; S++) {
        if (N % S) continue;
        const double c = (double)N / S + 1.4 * (S - 1);
        if (c < cost) {
            cost = c;
            best = S;
        }
    }
    return best;
}

// waves per robot of a row-parallel launch of B robots (eight waves per robot up to 64 robots measured no faster:
// the one-robot phases are chains, not rounds; profiles/r05/ab/w8_rowchol2.txt)
inline int rowpar_waves(const nmpc_batch* b, int B)
{
    return B <= 256 ? 4 : b->rowpar_w;
}

// LDS a row-parallel launch of B robots may give each block: one CU's LDS shared by the ceil(B / CUs) robots each
// CU holds (one block per robot), so that every robot of the launch is resident at once. The CU count and the LDS
// per CU are the device's (hipDeviceProp_t at create: a CU-partitioned GPU has fewer CUs)
inline size_t rowpar_lds_cap(const nmpc_batch* b, int B)
{
    const int n_cu = b->n_cu > 0 ? b->n_cu : 1;
    const int per_cu = (B + n_cu - 1) / n_cu;
    return b->lds_per_cu / (size_t)(per_cu > 0 ? per_cu : 1);
}

// Whether a launch of B robots (path_march: a run_path launch, whose march only the team kernel has) runs the
// row-parallel kernel: its horizon segments (0: the serial phases), or -1 for the team kernel
template <class M>
int rowpar_ok(const nmpc_batch* b, int B, bool path_march, int mode)
{
    if (b->kp.ipm != NMPC_IPM_SINGLE || path_march || B > b->rowpar_max) return -1;
    const int rows = B <= 256 ? 16 : b->seg_rows;  // segments: any row up to 256 robots, the first wave's above
    const size_t cap = rowpar_lds_cap(b, B);
    int S = b->seg >= 0 ? b->seg : seg_count(b->prm.N, rows);
    if (S > rows || S > kSegMax || (S > 0 && b->prm.N % S)) S = 0;
    if (S > 0 && rowpar_lds_bytes<M>(b->prm.N, mode, S) > cap) S = 0;
    if (B > 256 && S == 0 && b->seg < 0) return -1;  // one wave per robot only with segments (auto)
    // above 256 robots two robots' waves share a SIMD, which needs <= 256 registers per lane: diff and tric's
    // segmented kernels take 246-250, omni4's (11 x 11 master blocks) 357 (tools/reg_usage.py), so omni4 keeps the
    // team kernel there
    if (B > 256 && M::NU == 4 && b->rowpar_max <= 1024) return -1;
    return rowpar_lds_bytes<M>(b->prm.N, mode, S) <= cap ? S : -1;
}

// Records one sweep of the team kernel touches over the handle's capacity in the wide layout (9 or 16 slots of
// 64 / 80 B per stage, plus the 64-B DZ plane entry): the measure of NMPC_REC_AUTO. diff takes the split planes when
// its own records exceed 3/4 of the 256 MB Infinity Cache. Alone on the device the metric fleet (4096 robots,
// 107 MB) keeps the wide records, 1.2 % faster there (issue-bound); a fleet beside other models (the mixed config)
// is set to SPLIT by its caller (fleet.py), where the split planes win 7 % (profiles/r04/ab/split.txt). The choice
// depends on this handle only, so no other handle can change it.
constexpr size_t kRecSplitBytes = (size_t)192 << 20;

size_t rec_footprint(const nmpc_batch* b)
{
    const size_t slots = b->prm.model == NMPC_MODEL_OMNI4AMR ? 16 : 9;  // omni4: quad-major, 16 slots of 80 B
    const size_t rec = b->prm.model == NMPC_MODEL_OMNI4AMR ? 80 : 64;
    return (size_t)b->capacity * (size_t)(b->prm.N + 1) * (slots * rec + 64);
}

int rec_layout_auto(const nmpc_batch* b)
{
    switch (b->prm.model) {
    case NMPC_MODEL_TRIC3AMR: return NMPC_REC_SPLIT;
    case NMPC_MODEL_OMNI4AMR: return NMPC_REC_WIDE;
    default: return rec_footprint(b) > kRecSplitBytes ? NMPC_REC_SPLIT : NMPC_REC_WIDE;
    }
}

// the warm-flag tag of a launch (NMPC_WARM_TAG_*): its multipliers' record layout and field order
int warm_tag_of(const nmpc_batch* b, int rec_split)
{
    if (b->kp.ipm != NMPC_IPM_SINGLE) return NMPC_WARM_TAG_MEHROTRA;
    return rec_split ? NMPC_WARM_TAG_SPLIT : NMPC_WARM_TAG_WIDE;
}

// What a launch of B robots runs: the kernel (waves per robot of k_sqp_rti_rowpar, 0: the team kernel), the
// row-parallel kernel's horizon segments, the team kernel's record layout and the tag the launch leaves in the warm
// flags. schedule() launches from it and nmpc_batch_plan_ex reports it; nothing else decides any of the four
struct LaunchPlan {
    int waves, seg, rec_split, warm_tag;
    int handoff;     // > 0: k_sqp_rti_team_ho with this hand-off iteration (then seg = kHandoffSeg, rec_split = 0)
    size_t ho_lds;   // its LDS bytes per block
};

// Whether a team-kernel launch of B robots takes the in-block hand-off (sqp_rti_team_ho.hip), and its LDS per block.
// The form exists for the single-direction rule, solve and run mode (the march of run_path owns the LDS), unsplit
// launches with at most one wave per SIMD (then one block per CU: the four resume slices have the CU's LDS to
// themselves), horizons of four segments of at least two stages, models whose segmented tick fits one wave per SIMD
// (diff, tric), diff's wide records (tric's hand-off launches take them too) and with every per-robot table off; a
// cap at or above qp_iter_max hands nobody off. Everything else keeps the plain kernel
inline int handoff_of(const nmpc_batch* b, int B)
{
    (void)B;  // (the rule looks at no batch size: a fleet split into stream groups hands over the same robots)
    return b->handoff == NMPC_HANDOFF_AUTO ? kHandoffDefault : b->handoff;
}

template <class M>
size_t handoff_ok(const nmpc_batch* b, int B, bool path_march)
{
    if (handoff_of(b, B) <= 0 || b->kp.ipm != NMPC_IPM_SINGLE || path_march) return 0;
    if ((B + 3) / 4 > b->n_simd || B <= b->split_max) return 0;  // dense, split (schedule())
    if (b->rparams.on || b->sbounds.on || b->rmodel.on) return 0;
    if (b->prm.model == NMPC_MODEL_DIFF2AMR && b->rec_split) return 0;
    const size_t lds = team_ho_lds_bytes<M>(b->prm.N);
    const int blocks = (B + 15) / 16, n_cu = b->n_cu > 0 ? b->n_cu : 1;
    if (lds == 0 || lds > b->lds_per_cu / (size_t)((blocks + n_cu - 1) / n_cu)) return 0;
    return lds;
}

LaunchPlan plan_launch(const nmpc_batch* b, int B, bool path_march, int mode)
{
    LaunchPlan p{};
    const int S = with_model(b->prm.model, [&](auto m) { return rowpar_ok<decltype(m)>(b, B, path_march, mode); });
    if (S >= 0) {
        p.waves = rowpar_waves(b, B);
        p.seg = S;
    }
    // the row-parallel kernel keeps the wide single-direction records; the team kernel the handle's layout
    p.rec_split = (!p.waves && b->kp.ipm == NMPC_IPM_SINGLE) ? b->rec_split : 0;
    if (!p.waves) {
        p.ho_lds = with_model(b->prm.model, [&](auto m) { return handoff_ok<decltype(m)>(b, B, path_march); });
        if (p.ho_lds) {
            p.handoff = handoff_of(b, B);
            p.seg = kHandoffSeg;
            p.rec_split = 0;
        }
    }
    p.warm_tag = warm_tag_of(b, p.rec_split);
    return p;
}

// The launch's plan and (team kernel) placement before a launch (schedule.hip); fills a.order / a.iter_key. Every
// robot's warm flag carries the tag of the layout its multipliers sit in, so a launch whose layout differs from a
// robot's last one starts that robot cold and leaves the others alone
hipError_t schedule(nmpc_batch* b, KArgs& a, int mode, hipStream_t s)
{
    const LaunchPlan p = plan_launch(b, a.B, a.segs != nullptr, mode);
    a.iter_key = b->iter_key;
    a.warm = b->warm;
    a.rowpar = p.waves;
    a.seg = p.seg;
    a.rec_split = p.rec_split;
    a.warm_tag = p.warm_tag;
    a.handoff = p.handoff;
    if (a.rowpar && !a.n_active) return hipSuccess;  // one robot per wave: nothing to place
    a.dense = ((a.B + 3) / 4 > b->n_simd) ? 1 : 0;  // 4 teams per wave
    // small batches leave most of the chip idle: one wave per robot, whose spare rows integrate P0's stages
    a.split = (!a.dense && a.B <= b->split_max) ? 1 : 0;
    int layout = b->sched;
    if (layout == NMPC_SCHED_AUTO) layout = a.dense ? NMPC_SCHED_SORTED : NMPC_SCHED_OFF;
    if (a.n_active) {
        // node tick: every form takes the compacted order (the robots that solve first). The forms with one robot
        // per block keep index order; the team kernel follows the handle's schedule (interleaved and spread: sorted)
        if (a.rowpar) a.dense = a.split = 0;
        const int sorted = (!a.rowpar && !a.split && layout != NMPC_SCHED_OFF) ? 1 : 0;
        a.order = b->order;
        return launch_node_order(b->iter_key, b->node_active, a.B, sorted, b->order, b->node_n, s);
    }
    if (a.split) return hipSuccess;  // one robot per wave: nothing to place
    if (layout == NMPC_SCHED_OFF) return hipSuccess;
    a.order = b->order;
    return launch_team_order(b->iter_key, a.B, layout, b->sorted, b->order, s);
}

hipError_t launch(nmpc_batch* b, KArgs& a, int mode, hipStream_t s)
{
    const hipError_t e = schedule(b, a, mode, s);
    if (e != hipSuccess) return e;
    return with_model(b->prm.model, [&](auto m) { return launch_m<decltype(m)>(b, a, mode, s); });
}

// the handle and batch-size checks every entry point of a handle starts with
int check_batch(const nmpc_batch* b, int B)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (B < 0 || B > b->capacity) return set_err(NMPC_ERR_ARG, "B out of range [0, capacity]");
    return NMPC_OK;
}

// a launch of B robots on the handle's resident state; the entry points add the fields that are theirs
KArgs resident_args(const nmpc_batch* b, int B)
{
    KArgs a;
    std::memset(&a, 0, sizeof(a));
    a.B = B;
    a.stride = b->capacity;
    a.sstride = b->capacity;
    a.xbar = b->xbar;
    a.ubar = b->ubar;
    a.carried = b->carried;
    a.scratch = b->scratch;
    a.rparams = b->rparams.view();
    a.sbounds = b->sbounds.view();
    a.rmodel = b->rmodel.view();
    a.set_origin(b->rframe.view64());  // (in traj's slot: the launches that are given their poses overwrite it)
    return a;
}

// A table ready for a writer on stream s: allocated at the first call and, whenever it was off, filled by fill(table)
// (one launch on s) with what the launches used until now, so a table nobody wrote to solves what the handle solved.
// It is on only if that launch succeeded
template <class Fill>
int table_ready(DevTable& t, const char* what, Fill&& fill)
{
    if (t.on) return NMPC_OK;
    if (!t.p) {
        const hipError_t e = hipMalloc(&t.p, sizeof(float) * t.floats);
        if (e != hipSuccess) return hip_err(e, "hipMalloc");
    }
    const int rc = hip_err(fill(t.p), what);
    if (rc == NMPC_OK) t.on = true;
    return rc;
}

// the handle's own column of the per-robot table (KParams' fp32 values); its first sb_rows rows are the stage table's
RpColumn own_column(const nmpc_batch* b)
{
    RpColumn col;
    std::memset(&col, 0, sizeof(col));
    const KParams& k = b->kp;
    for (int i = 0; i < b->nbx; i++) { col.v[b->rp.off[kRpLbx] + i] = k.lbx[i]; col.v[b->rp.off[kRpUbx] + i] = k.ubx[i]; }
    for (int i = 0; i < b->nbu; i++) { col.v[b->rp.off[kRpLbu] + i] = k.lbu[i]; col.v[b->rp.off[kRpUbu] + i] = k.ubu[i]; }
    for (int i = 0; i < b->ny; i++) col.v[b->rp.off[kRpW] + i] = k.W[i];
    for (int i = 0; i < b->nx; i++) col.v[b->rp.off[kRpWe] + i] = k.We[i];
    return col;
}

int rp_table(nmpc_batch* b, hipStream_t s)
{
    return table_ready(b->rparams, "robot_params fill launch", [&](float* t) {
        return launch_rows_fill(t, b->capacity, b->rp.off[kRpFields], own_column(b), s);
    });
}

int rm_table(nmpc_batch* b, hipStream_t s)
{
    return table_ready(b->rmodel, "robot_model fill launch", [&](float* t) {
        RpColumn col{};
        for (int i = 0; i < b->np; i++) col.v[i] = b->kp.p[i];
        return launch_rows_fill(t, b->capacity, b->np, col, s);
    });
}

// the frame table's fill: every origin (0, 0), where the launches took the positions to be until now
int rf_table(nmpc_batch* b, hipStream_t s)
{
    return table_ready(b->rframe, "robot_frame fill launch",
                       [&](float* t) { return hipMemsetAsync(t, 0, sizeof(float) * b->rframe.floats, s); });
}

// the frame table's one writer launch (nmpc_batch_set_robot_frame, _recentre, _clear_robot_frame: launch_frame_set)
hipError_t frame_set(nmpc_batch* b, int B, const double* origin, const double* pose_map, double radius,
                     unsigned char* moved, const unsigned char* mask, hipStream_t s)
{
    return launch_frame_set(b->rframe.p64(), b->capacity, B, b->xbar, b->prm.N, b->nx, origin, pose_map, radius, moved,
                            mask, s);
}

SbDims sb_dims(const nmpc_batch* b) { return SbDims{b->prm.N, b->capacity, b->nbx, b->nbu}; }

// the stage table's fill: at every stage the box the launches used until now (the robot's column of the per-robot
// table if that is on, else the handle's)
int sb_table(nmpc_batch* b, hipStream_t s)
{
    return table_ready(b->sbounds, "stage_bounds fill launch", [&](float* t) {
        return launch_sb_fill(t, sb_dims(b), own_column(b), b->rparams.view(), b->rp, s);
    });
}

// A table's writer entry point: the checks every one of them makes, in their order (those that need no handle first;
// bad: the failed check of the writer's own payload, or nullptr), the table ready on the stream, then the writer's
// one launch
template <class Write>
int table_write(nmpc_batch* b, int B, const char* bad, int (*ready)(nmpc_batch*, hipStream_t), void* stream,
                const char* what, Write&& write)
{
    if (B < 0) return set_err(NMPC_ERR_ARG, "B out of range [0, capacity]");
    if (bad) return set_err(NMPC_ERR_ARG, bad);
    if (const int rc = check_batch(b, B)) return rc;
    if (B == 0) return NMPC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = ready(b, s)) return rc;
    return hip_err(write(s), what);
}

// the payload check of the two limits writers: msg when every array is NULL
const char* no_limits(const float* v_max, const float* a_max, const float* alpha_min, const float* alpha_max,
                      const float* dalpha_max, const char* msg)
{
    return (!v_max && !a_max && !alpha_min && !alpha_max && !dalpha_max) ? msg : nullptr;
}

nmpc_speed_rule speed_rule_default()
{
    nmpc_speed_rule r;
    r.slope = 0.8f;     // the ramps' value (tests/stage_bound_cases.py SLOPE)
    r.v_floor = 0.05f;
    return r;
}

// the speed rule's payload check (rule may be NULL: defaults)
const char* bad_speed_rule(const nmpc_speed_rule* r)
{
    if (r && !(r->slope > 0.0f && r->slope <= 1.0f)) return "speed rule: slope must be in (0, 1]";
    if (r && !(r->v_floor > 0.0f)) return "speed rule: v_floor must be > 0";
    return nullptr;
}

// the payload check of the speed map's two entry points: the failed check, or nullptr (rule may be NULL: defaults)
const char* bad_speed_map(const nmpc_speed_map* m, const nmpc_speed_rule* r)
{
    if (!m) return "speed map is NULL";
    if (!std::isfinite(m->res) || !(m->res > 0.0)) return "speed map: res must be finite and > 0";
    if (m->w < 1 || m->h < 1) return "speed map: w and h must be >= 1";
    if (!m->vmax) return "speed map: vmax is NULL";
    return bad_speed_rule(r);
}

nmpc_sep_rule sep_rule_default()
{
    nmpc_sep_rule r;
    r.clearance = 0.6f;
    r.gain = 1.0f;  // a one-second headway
    r.range = 3.0f;
    r.ahead_only = 1;
    return r;
}

// the payload check of fleet separation's writer and attach: the failed check, or nullptr (sep may be NULL: defaults;
// B < 0: the batch size is not known yet, own_first + B is checked by the call that knows it)
const char* bad_tracks(const nmpc_tracks* t, const nmpc_sep_rule* r, int B)
{
    if (!t) return "tracks is NULL";
    if (t->M < 0) return "tracks: M must be >= 0";
    if (t->K < 0) return "tracks: K must be >= 0";
    if (t->M > 0 && !t->xy) return "tracks: xy is NULL";
    if (t->own_first < -1) return "tracks: own_first must be >= -1";
    if (t->own_first >= 0 && B >= 0 && (long long)t->own_first + B > t->M) return "tracks: own_first + B exceeds M";
    if (r && (!std::isfinite(r->gain) || !(r->gain > 0.0f))) return "separation rule: gain must be finite and > 0";
    if (r && (!std::isfinite(r->clearance) || !(r->clearance >= 0.0f)))
        return "separation rule: clearance must be finite and >= 0";
    if (r && (!std::isfinite(r->range) || !(r->range > r->clearance)))
        return "separation rule: range must be finite and > clearance";
    return nullptr;
}

nmpc_sep_guard sep_guard_default()
{
    nmpc_sep_guard g;
    std::memset(&g, 0, sizeof(g));
    g.stop_gap = 0.45f;
    g.release_gap = 0.55f;
    g.hold_stages = 4;
    g.hold = 1;
    return g;
}

// the guard's payload check: the failed check, or nullptr (g may be NULL: no guard). range < 0: not known to the call
// (nmpc_batch_sep_hold), release_gap's upper bound is the writer's; own_first < -1: likewise not known
const char* bad_guard(const nmpc_sep_guard* g, float range, int own_first)
{
    if (!g) return nullptr;
    if (!std::isfinite(g->stop_gap) || !(g->stop_gap > 0.0f)) return "separation guard: stop_gap must be finite and > 0";
    if (!std::isfinite(g->release_gap) || !(g->release_gap >= g->stop_gap))
        return "separation guard: release_gap must be finite and >= stop_gap";
    if (range >= 0.0f && !(g->release_gap <= range)) return "separation guard: release_gap must be <= range";
    if (g->hold_stages < 0) return "separation guard: hold_stages must be >= 0";
    if (g->priority && !g->own_priority && own_first == -1)
        return "separation guard: priority without own_priority needs own_first >= 0";
    return nullptr;
}

// the speed map's writer launch on the stage table (which is ready): its arguments from the handle's tables and state
// (map nullptr and sep given: fleet separation without a map; sep: the q plane is ready on the stream)
hipError_t speed_map_write(nmpc_batch* b, int B, const nmpc_speed_map* map, const nmpc_speed_rule& rule,
                           const float* pose, const unsigned char* reset, const unsigned char* mask,
                           const unsigned char* mode, float* vlim, hipStream_t s, const nmpc_sep_rule* sep = nullptr,
                           float* gap = nullptr)
{
    SpeedMapArgs a;
    std::memset(&a, 0, sizeof(a));
    a.sb = b->sbounds.p;
    a.d = sb_dims(b);
    a.B = B;
    a.nx = b->nx;
    a.tric = b->prm.model == NMPC_MODEL_TRIC3AMR ? 1 : 0;
    if (map) a.map = *map;
    a.slope = rule.slope;
    a.v_floor = rule.v_floor;
    a.dt = b->kp.dt;
    a.cap = b->kp.ubx[0];
    a.a = b->kp.ubu[0];
    a.rp = b->rparams.view();
    a.rp_ubx = b->rp.off[kRpUbx];
    a.rp_ubu = b->rp.off[kRpUbu];
    a.xbar = b->xbar;
    a.carried = b->carried;
    a.origin = b->rframe.view64();
    a.pose = pose;
    a.reset = reset;
    a.mask = mask;
    a.mode = mode;
    a.vlim = vlim;
    if (sep) {
        a.sep_q = b->sep_q;  // (with a guard: the qy plane)
        a.sep_gain = sep->gain;
        a.sep_clearance = sep->clearance;
        a.gap = gap;
    }
    return launch_speed_map(a, s);
}

// the scratch of fleet separation's writer: the q plane, and boxes for M tracks (a larger M takes a new allocation;
// hipFree waits for the launches that read the old one)
int sep_scratch(nmpc_batch* b, int M)
{
    if (!b->sep_q) {
        const hipError_t e = hipMalloc(&b->sep_q, sizeof(float) * (size_t)(b->prm.N + 1) * (size_t)b->capacity);
        if (e != hipSuccess) return hip_err(e, "hipMalloc");
    }
    if (M > b->sep_boxes_m) {
        (void)hipFree(b->sep_boxes);
        b->sep_boxes = nullptr;
        b->sep_boxes_m = 0;
        const hipError_t e = hipMalloc(&b->sep_boxes, sizeof(double) * 4 * (size_t)M);
        if (e != hipSuccess) return hip_err(e, "hipMalloc");
        b->sep_boxes_m = M;
    }
    return NMPC_OK;
}

// the guard's scratch (see the handle): everything at once, held zeroed, the qa plane +inf
int guard_scratch(nmpc_batch* b)
{
    if (b->sep_held) return NMPC_OK;
    const size_t S = (size_t)b->capacity, n = (size_t)(b->prm.N + 1) * S;
    float* qa = nullptr;
    unsigned char *held = nullptr, *ms = nullptr;
    double* rs = nullptr;
    const float inf = INFINITY;
    int bits;
    std::memcpy(&bits, &inf, sizeof(bits));
    hipError_t e;
    if ((e = hipMalloc(&qa, sizeof(float) * n)) != hipSuccess || (e = hipMalloc(&held, S)) != hipSuccess ||
        (e = hipMalloc(&ms, S)) != hipSuccess || (e = hipMalloc(&rs, sizeof(double) * S)) != hipSuccess ||
        (e = hipMemsetD32((hipDeviceptr_t)qa, bits, n)) != hipSuccess || (e = hipMemset(held, 0, S)) != hipSuccess ||
        (e = hipMemset(ms, 0, S)) != hipSuccess || (e = hipMemset(rs, 0, sizeof(double) * S)) != hipSuccess ||
        (e = hipStreamSynchronize(nullptr)) != hipSuccess) {
        for (void* p : {(void*)qa, (void*)held, (void*)ms, (void*)rs}) (void)hipFree(p);
        return hip_err(e, "hipMalloc");
    }
    b->sep_qa = qa;
    b->sep_held = held;
    b->sep_mode_save = ms;
    b->sep_remains_save = rs;
    return NMPC_OK;
}

// held = 0 for every robot (attach and detach of the guard); nothing to do before the scratch exists
int guard_clear_held(nmpc_batch* b)
{
    if (!b->sep_held) return NMPC_OK;
    hipError_t e = hipDeviceSynchronize();  // (launches that read or write held on any stream)
    if (e == hipSuccess) e = hipMemset(b->sep_held, 0, (size_t)b->capacity);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return hip_err(e, "hipMemset");
}

hipError_t export_tracks(nmpc_batch* b, int B, const float* pose, const unsigned char* reset,
                         const unsigned char* mode, double* xy, int M, int K, int first, hipStream_t s,
                         const unsigned char* held = nullptr)
{
    ExportTracksArgs a;
    std::memset(&a, 0, sizeof(a));
    a.B = B;
    a.N = b->prm.N;
    a.nx = b->nx;
    a.cap = b->capacity;
    a.xbar = b->xbar;
    a.origin = b->rframe.view64();
    a.pose = pose;
    a.reset = reset;
    a.mode = mode;
    a.held = held;
    a.xy = xy;
    a.M = M;
    a.K = K;
    a.first = first;
    return launch_export_tracks(a, s);
}

// the hold's launch on the qa plane (ready). mode_rw: the cycle's mode array, whose held robots are parked in IDLE
hipError_t sep_hold(nmpc_batch* b, int B, const nmpc_sep_guard& g, const unsigned char* mode, const unsigned char* reset,
                    unsigned char* held_out, unsigned char* mode_rw, const double* remains, hipStream_t s)
{
    SepHoldArgs a;
    std::memset(&a, 0, sizeof(a));
    a.B = B;
    a.N = b->prm.N;
    a.cap = b->capacity;
    a.qa = b->sep_qa;
    a.last = g.hold_stages < b->prm.N ? g.hold_stages : b->prm.N;
    a.stop_gap = g.stop_gap;
    a.release_gap = g.release_gap;
    a.hold = g.hold ? 1 : 0;
    a.mode = mode;
    a.reset = reset;
    a.held = b->sep_held;
    a.held_out = held_out;
    a.mode_rw = mode_rw;
    a.mode_save = b->sep_mode_save;
    a.remains = remains;
    a.remains_save = b->sep_remains_save;
    return launch_sep_hold(a, s);
}

// fleet separation's writer on the stage table and the scratch (both ready): the q plane, then the rule's launch.
// guard: the guard form (its scratch is ready too): q is qy, the qa plane is written, gap_all takes its square roots
hipError_t tracks_write(nmpc_batch* b, int B, const nmpc_tracks& t, const nmpc_sep_rule& sep, const nmpc_speed_map* map,
                        const nmpc_speed_rule& rule, const float* pose, const unsigned char* reset,
                        const unsigned char* mask, const unsigned char* mode, float* vlim, float* gap, hipStream_t s,
                        const nmpc_sep_guard* guard = nullptr, float* gap_all = nullptr)
{
    SepArgs a;
    std::memset(&a, 0, sizeof(a));
    a.d = sb_dims(b);
    a.B = B;
    a.nx = b->nx;
    a.xbar = b->xbar;
    a.origin = b->rframe.view64();
    a.pose = pose;
    a.reset = reset;
    a.mask = mask;
    a.mode = mode;
    a.xy = t.xy;
    a.M = t.M;
    a.K = t.K;
    a.own_first = t.own_first;
    a.ahead_only = sep.ahead_only ? 1 : 0;
    a.range2 = sep.range * sep.range;
    a.cull2 = (double)a.range2 * (1.0 + 1e-5);  // separation.hip: why this is conservative
    a.boxes = b->sep_boxes;
    a.q = b->sep_q;
    if (guard) {
        a.guard = 1;
        a.priority = guard->priority;
        a.own_priority = guard->own_priority;
        a.held = b->sep_held;
        a.qa = b->sep_qa;
        a.gap_all = gap_all;
    }
    const hipError_t e = launch_sep_min(a, s);
    if (e != hipSuccess) return e;
    if (guard) b->sep_qa_ready = true;
    return speed_map_write(b, B, map, rule, pose, reset, mask, mode, vlim, s, &sep, gap);
}

// nmpc_batch_robot_params / nmpc_batch_robot_model: the view of a row-major table, [rows][capacity]
int rows_view(nmpc_batch* b, DevTable nmpc_batch::*t, float** table, int* rows, int* stride)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (table) *table = (b->*t).view();
    if (rows) *rows = (int)((b->*t).floats / (size_t)b->capacity);
    if (stride) *stride = b->capacity;
    return NMPC_OK;
}

int table_clear(nmpc_batch* b, DevTable nmpc_batch::*t)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    (b->*t).on = false;  // (the allocation stays for the next writer, which refills it)
    return NMPC_OK;
}

// ... with the inputs and outputs every run-mode launch has; the reference (traj or the path march) is the caller's
KArgs run_args(const nmpc_batch* b, int B, const float* pose, const float* vel, const float* steer,
               const unsigned char* reset, float* cmd, float* u0, int* status, int* qp_iter, float* qp_res)
{
    KArgs a = resident_args(b, B);
    a.pose = pose;
    a.vel = vel;
    a.steer = steer;
    a.reset = reset;
    a.cmd = cmd;
    a.u0 = u0;
    a.status = status;
    a.qp_iter = qp_iter;
    a.qp_res = qp_res;
    return a;
}

int check_params(const nmpc_model_params* prm)
{
    int nx, nu, nbx, nbu, np;
    if (!prm) return set_err(NMPC_ERR_ARG, "params is NULL");
    if (!dims_of(prm->model, &nx, &nu, &nbx, &nbu, &np)) return set_err(NMPC_ERR_ARG, "unknown model id");
    if (prm->N < 1 || prm->N > 4096) return set_err(NMPC_ERR_ARG, "horizon N out of range [1, 4096]");
    if (!(prm->dt > 0.0) || !(prm->dt_ctrl > 0.0)) return set_err(NMPC_ERR_ARG, "dt must be positive");
    if (prm->qp_iter_max < 1) return set_err(NMPC_ERR_ARG, "qp_iter_max must be >= 1");
    if (prm->qp_ipm != NMPC_IPM_MEHROTRA && prm->qp_ipm != NMPC_IPM_SINGLE)
        return set_err(NMPC_ERR_ARG, "qp_ipm must be NMPC_IPM_MEHROTRA or NMPC_IPM_SINGLE");
    if (prm->qp_warm_start != 0 && prm->qp_warm_start != 1) return set_err(NMPC_ERR_ARG, "qp_warm_start must be 0 or 1");
    if (prm->qp_warm_start && !(prm->qp_warm_kappa > 0.0)) return set_err(NMPC_ERR_ARG, "qp_warm_kappa must be > 0");
    if (prm->qp_warm_iter_max < 0) return set_err(NMPC_ERR_ARG, "qp_warm_iter_max must be >= 0");
    if (!(prm->qp_infeas_lambda >= 0.0)) return set_err(NMPC_ERR_ARG, "qp_infeas_lambda must be >= 0 (0: off)");
    if (prm->qp_ipm == NMPC_IPM_SINGLE &&
        !(prm->qp_sigma_lo > 0.0 && prm->qp_sigma_lo <= prm->qp_sigma_hi && prm->qp_sigma_hi <= 1.0))
        return set_err(NMPC_ERR_ARG, "qp_sigma_lo / qp_sigma_hi need 0 < lo <= hi <= 1");
    for (int i = 0; i < nbx; i++)
        if (!(prm->lbx[i] < prm->ubx[i])) return set_err(NMPC_ERR_ARG, "state bounds need lbx < ubx");
    for (int i = 0; i < nbu; i++)
        if (!(prm->lbu[i] < prm->ubu[i])) return set_err(NMPC_ERR_ARG, "input bounds need lbu < ubu");
    for (int i = 0; i < np; i++)
        if (!(prm->p[i] > 0.0)) return set_err(NMPC_ERR_ARG, "model parameters must be positive");
    for (int i = 0; i < nu; i++)
        if (!(prm->W[nx + i] > 0.0)) return set_err(NMPC_ERR_UNSUPPORTED, "input weights R must be > 0");
    return NMPC_OK;
}

}  // namespace

extern "C" {

const char* nmpc_last_error(void) { return g_err.c_str(); }
const char* nmpc_version(void) { return "nmpc_amd 0.4 (team-per-instance DPP SQP-RTI, gfx950)"; }

int nmpc_model_dims(int model, int* nx, int* nu, int* ny, int* nbx, int* nbu, int* np)
{
    int a, b, c, d, e;
    if (!dims_of(model, &a, &b, &c, &d, &e)) return set_err(NMPC_ERR_ARG, "unknown model id");
    if (nx) *nx = a;
    if (nu) *nu = b;
    if (ny) *ny = a + b;
    if (nbx) *nbx = c;
    if (nbu) *nbu = d;
    if (np) *np = e;
    return NMPC_OK;
}

int nmpc_model_params_default(int model, int N, nmpc_model_params* prm)
{
    int nx, nu, nbx, nbu, np;
    if (!prm) return set_err(NMPC_ERR_ARG, "params is NULL");
    if (!dims_of(model, &nx, &nu, &nbx, &nbu, &np)) return set_err(NMPC_ERR_ARG, "unknown model id");
    std::memset(prm, 0, sizeof(*prm));
    prm->model = model;
    prm->N = N;
    prm->dt = 1.0 / 40.0;      // config/nmpc_nav_control_acados_models.yaml:28
    prm->dt_ctrl = 1.0 / 40.0; // config/nmpc_nav_control.yaml:4
    const double deg = M_PI / 180.0;
    // rob_wh_max_vel / rob_wh_max_ace 1.0 (nmpc_nav_control.yaml:20-21/31-32/44-45),
    // steering -45..45 deg, 15 deg/s (nmpc_nav_control.yaml:46-48)
    nmpc_model_params_set_limits(prm, 1.0, 1.0, -45.0 * deg, 45.0 * deg, 15.0 * deg);
    if (model == NMPC_MODEL_DIFF2AMR) {
        prm->p[0] = 0.270; prm->p[1] = 0.1;  // nmpc_nav_control.yaml:29-30
        const double W[9] = {10, 10, 5, 0, 0, 0, 0, 1, 1};
        std::memcpy(prm->W, W, sizeof(W));
        prm->terminal_hack = 1;
    } else if (model == NMPC_MODEL_OMNI4AMR) {
        prm->p[0] = 0.265 + 0.270; prm->p[1] = 0.1;  // nmpc_nav_control.yaml:17-19, NMPCNavControlROS.cpp:97-99
        const double W[15] = {10, 10, 5, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1};
        std::memcpy(prm->W, W, sizeof(W));
    } else {
        prm->p[0] = 0.270; prm->p[1] = 0.1; prm->p[2] = 0.5;  // nmpc_nav_control.yaml:41-43
        const double W[9] = {10, 10, 5, 0, 0, 0, 0, 1, 1};
        std::memcpy(prm->W, W, sizeof(W));
        prm->tric_sin_bug = 1;
    }
    for (int i = 0; i < nx; i++) prm->W_e[i] = prm->W[i];  // NMPCNavControlDiff.cpp:39-41
    prm->qp_iter_max = 50;
    prm->qp_tol_stat = 1e-4;
    prm->qp_tol_ineq = 1e-6;
    prm->qp_tol_comp = 1e-10;
    prm->qp_mu0 = 1.0;
    // initial slack floor t0 = max(z - lb, thr0): 0.25 instead of the oracle's 0.5 starts nearly active bounds
    // closer to their solution (steady-state closed loop: 8.0 -> 7.5 IPM iterations, 6 % faster ticks) while
    // the cold-start tail grows by at most 2 iterations (DESIGN.md "Algorithm and precision")
    prm->qp_thr0 = 0.25;
    prm->qp_tau = 0.995;
    // one direction per IPM iteration (P1 + one forward sweep) instead of Mehrotra's two (P1 + F0 + C1 + F1):
    // more, cheaper iterations; the slowest robot, which sets the kernel time, gets there sooner. Same-box A/B,
    // M it/s: diff N=40 B=4096 2.89 -> 3.24 (2 stream groups; 3.52 with one), B=1024 0.89 -> 1.00, tric 2.12 ->
    // 2.28, mixed 3.51 -> 3.64, omni4 2.45 -> 2.44 (profiles/r02/ab/ipm_single.txt)
    prm->qp_ipm = NMPC_IPM_SINGLE;
    prm->qp_sigma_lo = 0.01;
    prm->qp_sigma_hi = 0.5;
    // warm-started bound multipliers, floored at kappa / t: steady-state closed loop, emulator on 4096 robots of
    // real bench ticks: mean 10.9 -> 9.3 single-direction iterations, tail 22 -> 19 (DESIGN.md "Algorithm").
    // kappa per model from same-box A/B runs (profiles/r02/ab/warm.txt): diff 0.2 (as fast as 0.05, shorter
    // worst case: 29 against 39 iterations), omni4 and tric 0.01 (+7 % / +4 % against 0.05)
    prm->qp_warm_start = 1;
    prm->qp_warm_kappa = (model == NMPC_MODEL_DIFF2AMR) ? 0.2 : 0.01;
    // diff: warm start only after an easy solve. On 3 x 4096 stationary bench QPs (tools/warm_study.py, renewals
    // in the loop) warm after <= 12 iterations gives mean 8.78 / per-tick max 22, 21, 21 IPM iterations against
    // 8.60 / 30, 25, 27 for warm always and 9.38 / 22, 21, 21 for cold; same-box A/B (profiles/r03/ab/warm_iter.txt)
    // metric 3.00 -> 3.73 M it/s (cold 3.75, <= 10: 3.74, <= 16: 3.19), diff1024 0.87 -> 1.02 M. omni4 and tric
    // (kappa 0.01) lose with the rule (omni4 2.88 -> 2.47, tric 3.06 -> 2.82, mixed 4.52 -> 3.96 M): always warm
    prm->qp_warm_iter_max = (model == NMPC_MODEL_DIFF2AMR) ? 12 : 0;
    // early status-4 exit for infeasible QPs (a carried vel-ref far outside its bound): multipliers > 1e5 x the
    // weight scale with an open bound residual (tools/infeas_study.py: feasible bench QPs stay below 88)
    prm->qp_infeas_lambda = 1e5;
    return NMPC_OK;
}

int nmpc_model_params_set_limits(nmpc_model_params* prm, double v_max, double a_max, double alpha_min,
                                 double alpha_max, double dalpha_max)
{
    int nx, nu, nbx, nbu, np;
    if (!prm) return set_err(NMPC_ERR_ARG, "params is NULL");
    if (!dims_of(prm->model, &nx, &nu, &nbx, &nbu, &np)) return set_err(NMPC_ERR_ARG, "unknown model id");
    for (int i = 0; i < 4; i++) prm->lbx[i] = prm->ubx[i] = prm->lbu[i] = prm->ubu[i] = 0.0;
    for (int i = 0; i < nbx; i++) { prm->lbx[i] = -v_max; prm->ubx[i] = v_max; }
    for (int i = 0; i < nbu; i++) { prm->lbu[i] = -a_max; prm->ubu[i] = a_max; }
    if (prm->model == NMPC_MODEL_TRIC3AMR) {
        prm->lbx[1] = alpha_min;
        prm->ubx[1] = alpha_max;
        prm->lbu[1] = -dalpha_max;
        prm->ubu[1] = dalpha_max;
    }
    return NMPC_OK;
}

int nmpc_batch_create(const nmpc_model_params* prm, int capacity, nmpc_batch** out)
{
    if (!out) return set_err(NMPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    int rc = check_params(prm);
    if (rc) return rc;
    if (capacity < 1) return set_err(NMPC_ERR_ARG, "capacity must be >= 1");
    nmpc_batch* b = new nmpc_batch();
    b->prm = *prm;
    b->capacity = capacity;
    dims_of(prm->model, &b->nx, &b->nu, &b->nbx, &b->nbu, &b->np);
    b->ny = b->nx + b->nu;
    b->kp = to_kparams(*prm, b->nx, b->nu, b->nbx, b->nbu);
    b->rp = rp_rows(b->nx, b->nu, b->nbx, b->nbu);
    b->rparams.floats = (size_t)b->rp.off[kRpFields] * (size_t)capacity;
    b->sbounds.floats = (size_t)(prm->N + 1) * (size_t)sb_rows(b->nbx, b->nbu) * (size_t)capacity;
    b->rmodel.floats = (size_t)b->np * (size_t)capacity;
    b->rframe.floats = 4 * (size_t)capacity;  // [2][capacity] doubles
    if (const char* sv = std::getenv("NMPC_AMD_SCHED")) {  // off | auto | sorted | interleaved
        const char* names[5] = {"off", "auto", "sorted", "interleaved", "spread"};
        for (int i = 0; i < 5; i++)
            if (std::strcmp(sv, names[i]) == 0) b->sched = i;
    }
    if (const char* v = std::getenv("NMPC_AMD_SPLIT_MAX")) b->split_max = std::atoi(v);  // A/B: 0 = never split
    if (const char* v = std::getenv("NMPC_AMD_ROWPAR_MAX")) b->rowpar_max = std::atoi(v);  // A/B: 0 = never
    if (const char* v = std::getenv("NMPC_AMD_SEG")) b->seg = std::atoi(v);  // A/B: 0 = serial, S = S segments
    if (const char* v = std::getenv("NMPC_AMD_ROWPAR_W")) b->rowpar_w = std::atoi(v) == 1 ? 1 : 2;  // A/B
    if (const char* v = std::getenv("NMPC_AMD_SEG_ROWS")) b->seg_rows = std::atoi(v) == 8 ? 8 : 4;  // A/B
    if (const char* v = std::getenv("NMPC_AMD_HANDOFF")) b->handoff = std::atoi(v) > 0 ? std::atoi(v) : 0;  // A/B: 0 = off
    const int N = prm->N;
    const size_t S = (size_t)capacity;
    hipError_t e;
    int dev = 0;
    hipDeviceProp_t props;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&props, dev) == hipSuccess &&
        props.multiProcessorCount > 0) {
        b->n_simd = 4 * props.multiProcessorCount;
        b->n_cu = props.multiProcessorCount;
        if (props.maxSharedMemoryPerMultiProcessor > 0) b->lds_per_cu = props.maxSharedMemoryPerMultiProcessor;
    }
    if ((e = hipMalloc(&b->iter_key, sizeof(int) * S)) != hipSuccess ||
        (e = hipMalloc(&b->order, sizeof(int) * S)) != hipSuccess ||
        (e = hipMalloc(&b->sorted, sizeof(int) * S)) != hipSuccess ||
        (e = hipMemset(b->iter_key, 0, sizeof(int) * S)) != hipSuccess ||
        (e = hipMalloc(&b->warm, S)) != hipSuccess || (e = hipMemset(b->warm, 0, S)) != hipSuccess ||
        (e = hipMalloc(&b->xbar, sizeof(float) * (N + 1) * b->nx * S)) != hipSuccess ||
        (e = hipMalloc(&b->ubar, sizeof(float) * N * b->nu * S)) != hipSuccess ||
        (e = hipMalloc(&b->carried, sizeof(float) * b->nbx * S)) != hipSuccess ||
        (e = hipMalloc(&b->scratch, sizeof(float) * scratch_floats(prm->model, N, capacity))) != hipSuccess) {
        nmpc_batch_destroy(b);
        return hip_err(e, "hipMalloc");
    }
    rc = nmpc_batch_init_iterate(b, capacity, 0, nullptr);
    if (rc == NMPC_OK) rc = hip_err(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    if (rc) {
        nmpc_batch_destroy(b);
        return rc;
    }
    // the record layout: this handle's own choice (NMPC_REC_AUTO), fixed until nmpc_batch_set_record_layout
    b->rec_split = rec_layout_auto(b);
    if (const char* v = std::getenv("NMPC_AMD_REC_SPLIT"))  // A/B runs: 0 wide, 1 split (where the model has it)
        if (prm->model == NMPC_MODEL_DIFF2AMR) b->rec_split = std::atoi(v) ? NMPC_REC_SPLIT : NMPC_REC_WIDE;
    *out = b;
    return NMPC_OK;
}

int nmpc_batch_destroy(nmpc_batch* b)
{
    if (!b) return NMPC_OK;
    (void)hipFree(b->xbar);
    (void)hipFree(b->ubar);
    (void)hipFree(b->carried);
    (void)hipFree(b->scratch);
    (void)hipFree(b->iter_key);
    (void)hipFree(b->order);
    (void)hipFree(b->sorted);
    (void)hipFree(b->warm);
    (void)hipFree(b->path_err);
    (void)hipFree(b->node_traj);
    (void)hipFree(b->node_len);
    (void)hipFree(b->node_active);
    (void)hipFree(b->node_n);
    (void)hipFree(b->node_status);
    for (const DevTable* t : {&b->rparams, &b->sbounds, &b->rmodel, &b->rframe}) (void)hipFree(t->p);
    for (void* p : {(void*)b->in_st.stamp, (void*)b->in_st.sample, (void*)b->in_st.count, (void*)b->in_st.newest,
                    (void*)b->in_st.held, (void*)b->in_pose, (void*)b->in_vel, (void*)b->in_goal, (void*)b->in_steer,
                    (void*)b->in_valid, (void*)b->sep_q, (void*)b->sep_boxes, (void*)b->sep_qa, (void*)b->sep_held,
                    (void*)b->sep_mode_save, (void*)b->sep_remains_save})
        (void)hipFree(p);
    delete b;
    return NMPC_OK;
}

int nmpc_batch_set_params(nmpc_batch* b, const nmpc_model_params* prm)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    int rc = check_params(prm);
    if (rc) return rc;
    if (prm->model != b->prm.model || prm->N != b->prm.N)
        return set_err(NMPC_ERR_ARG, "set_params cannot change model or horizon");
    b->prm = *prm;
    b->kp = to_kparams(*prm, b->nx, b->nu, b->nbx, b->nbu);
    return NMPC_OK;
}

int nmpc_batch_get_params(const nmpc_batch* b, nmpc_model_params* prm)
{
    if (!b || !prm) return set_err(NMPC_ERR_ARG, "NULL argument");
    *prm = b->prm;
    return NMPC_OK;
}

int nmpc_batch_init_iterate(nmpc_batch* b, int B, int mode, void* stream)
{
    if (const int rc = check_batch(b, B)) return rc;
    if (mode != 0 && mode != 1) return set_err(NMPC_ERR_ARG, "mode must be 0 (create) or 1 (reset)");
    return hip_err(launch_init_iterate(b->xbar, b->ubar, b->carried, b->warm, B, b->capacity, b->prm.N, b->nx, b->nu,
                                       b->nbx, mode, (hipStream_t)stream),
                   "init_iterate launch");
}

int nmpc_batch_solve(nmpc_batch* b, int B, const float* x0, const float* yref, int ny_in, const float* We,
                     const unsigned char* reset, float* u0, float* x1, float* xtraj, float* utraj, int* status,
                     int* qp_iter, float* qp_res, void* stream)
{
    const TraceRange trace("nmpc_batch_solve");
    if (const int rc = check_batch(b, B)) return rc;
    if (B == 0) return NMPC_OK;
    if (!x0 || !yref) return set_err(NMPC_ERR_ARG, "x0 and yref are required");
    if (ny_in < 1 || ny_in > b->ny) return set_err(NMPC_ERR_ARG, "ny_in out of range [1, NY]");
    KArgs a = resident_args(b, B);
    a.x0 = x0;
    a.yref = yref;
    a.ny_in = ny_in;
    a.We = We;
    a.reset = reset;
    a.u0 = u0;
    a.x1 = x1;
    a.xtraj = xtraj;
    a.utraj = utraj;
    a.status = status;
    a.qp_iter = qp_iter;
    a.qp_res = qp_res;
    return hip_err(launch(b, a, kModeSolve, (hipStream_t)stream), "solve launch");
}

namespace {
int solve_iterate(nmpc_batch* b, int B, const float* x0, const float* yref, int ny_in, const float* We,
                  const unsigned char* reset, float* xbar, float* ubar, int ld, int* status, int* qp_iter,
                  float* qp_res, void* stream, const nmpc_stage_io* io)
{
    if (const int rc = check_batch(b, B)) return rc;
    if (B == 0) return NMPC_OK;
    if (!x0 || !yref || !xbar || !ubar) return set_err(NMPC_ERR_ARG, "x0, yref, xbar and ubar are required");
    if (ld < B) return set_err(NMPC_ERR_ARG, "ld < B");
    if (ny_in < 1 || ny_in > b->ny) return set_err(NMPC_ERR_ARG, "ny_in out of range [1, NY]");
    KArgs a = resident_args(b, B);
    a.stride = ld;  // the caller's iterate; sstride stays: the scratch planes follow the allocation, not ld
    a.xbar = xbar;
    a.ubar = ubar;
    a.x0 = x0;
    a.yref = yref;
    a.ny_in = ny_in;
    a.We = We;
    a.reset = reset;
    a.status = status;
    a.qp_iter = qp_iter;
    a.qp_res = qp_res;
    if (io) {
        // one robot on the row-parallel kernel only (the team kernel does not stage)
        if (B != 1 || !plan_launch(b, B, false, kModeSolve).waves)
            return set_err(NMPC_ERR_ARG, "staged I/O needs a one-robot row-parallel launch");
        a.stage_in_h = io->in_h;
        a.stage_in_d = io->in_d;
        a.stage_in_n = io->in_n;
        a.stage_out_h = io->out_h;
        a.stage_out_d = io->out_d;
        a.stage_out_n = io->out_n;
    }
    return hip_err(launch(b, a, kModeSolve, (hipStream_t)stream), "solve launch");
}
}  // namespace

int nmpc_batch_solve_iterate(nmpc_batch* b, int B, const float* x0, const float* yref, int ny_in, const float* We,
                             const unsigned char* reset, float* xbar, float* ubar, int ld, int* status, int* qp_iter,
                             float* qp_res, void* stream)
{
    const TraceRange trace("nmpc_batch_solve_iterate");
    return solve_iterate(b, B, x0, yref, ny_in, We, reset, xbar, ubar, ld, status, qp_iter, qp_res, stream, nullptr);
}

int nmpc_batch_solve_iterate_staged(nmpc_batch* b, const float* x0, const float* yref, int ny_in, const float* We,
                                    float* xbar, float* ubar, int* status, int* qp_iter, float* qp_res, void* stream,
                                    const nmpc_stage_io* io)
{
    const TraceRange trace("nmpc_batch_solve_iterate_staged");
    if (!io || !io->in_h || !io->in_d || !io->out_h || !io->out_d || io->in_n < 0 || io->out_n < 0)
        return set_err(NMPC_ERR_ARG, "staged I/O: host and device blocks are required");
    return solve_iterate(b, 1, x0, yref, ny_in, We, nullptr, xbar, ubar, 1, status, qp_iter, qp_res, stream, io);
}

int nmpc_batch_run(nmpc_batch* b, int B, const float* pose, const float* vel, const float* steer,
                   const float* traj, const int* traj_len, const unsigned char* reset, float* cmd, float* u0,
                   int* status, int* qp_iter, float* qp_res, void* stream)
{
    const TraceRange trace("nmpc_batch_run");
    if (const int rc = check_batch(b, B)) return rc;
    if (B == 0) return NMPC_OK;
    if (!pose || !vel || !traj) return set_err(NMPC_ERR_ARG, "pose, vel and traj are required");
    KArgs a = run_args(b, B, pose, vel, steer, reset, cmd, u0, status, qp_iter, qp_res);
    a.traj = traj;
    a.traj_len = traj_len;
    return hip_err(launch(b, a, kModeRun, (hipStream_t)stream), "run launch");
}

int nmpc_batch_run_path(nmpc_batch* b, int B, const float* pose, const float* vel, const float* steer,
                        const nmpc_path_segment* segs, int seg_stride, const int* nseg, const double* nearest_u,
                        double sample_period, int is_holonomic, const unsigned char* reset, float* traj_out,
                        float* cmd, float* u0, int* status, int* qp_iter, float* qp_res, void* stream)
{
    const TraceRange trace("nmpc_batch_run_path");
    if (const int rc = check_batch(b, B)) return rc;
    if (B == 0) return NMPC_OK;
    if (!pose || !vel || !segs || !nseg || !nearest_u)
        return set_err(NMPC_ERR_ARG, "pose, vel, segs, nseg and nearest_u are required");
    if (seg_stride < 1) return set_err(NMPC_ERR_ARG, "seg_stride < 1");
    if (!(sample_period >= 0.0)) return set_err(NMPC_ERR_ARG, "sample_period must be >= 0");
    if (16 * (sizeof(double) + 3 * sizeof(float)) * (size_t)(b->prm.N + 1) > 65536)
        return set_err(NMPC_ERR_UNSUPPORTED, "horizon too long for the in-kernel path march");
    KArgs a = run_args(b, B, pose, vel, steer, reset, cmd, u0, status, qp_iter, qp_res);
    a.segs = segs;
    a.seg_stride = seg_stride;
    a.nseg = nseg;
    a.nearest_u = nearest_u;
    a.period = sample_period;
    a.holo = is_holonomic ? 1 : 0;
    a.traj_out = traj_out;
    return hip_err(launch(b, a, kModeRun, (hipStream_t)stream), "run_path launch");
}

int nmpc_batch_follow_path(nmpc_batch* b, int B, const float* pose, const float* vel, const float* steer,
                           const nmpc_path_segment* segs, int seg_stride, const int* nseg, double* path_u,
                           double sample_period, int is_holonomic, double max_pos_err, double max_ori_err,
                           const unsigned char* reset, double* err, unsigned char* off_path, float* traj_out,
                           float* cmd, float* u0, int* status, int* qp_iter, float* qp_res, void* stream)
{
    const TraceRange trace("nmpc_batch_follow_path");
    if (const int rc = check_batch(b, B)) return rc;
    if (B == 0) return NMPC_OK;
    if (!pose || !vel || !segs || !nseg || !path_u)
        return set_err(NMPC_ERR_ARG, "pose, vel, segs, nseg and path_u are required");
    if (seg_stride < 1) return set_err(NMPC_ERR_ARG, "seg_stride < 1");
    if (!std::isfinite(sample_period) || sample_period < 0.0)
        return set_err(NMPC_ERR_ARG, "sample_period must be finite and >= 0");
    // a threshold of +inf or NaN switches its comparison off
    const int use_pos = !(std::isnan(max_pos_err) || max_pos_err == INFINITY);
    const int use_ori = !(std::isnan(max_ori_err) || max_ori_err == INFINITY);
    const bool guard = use_pos || use_ori || off_path;
    if (guard && !err) {
        if (!b->path_err) {
            const hipError_t e = hipMalloc(&b->path_err, sizeof(double) * 2 * (size_t)b->capacity);
            if (e != hipSuccess) return hip_err(e, "hipMalloc");
        }
        err = b->path_err;
    }
    hipStream_t s = (hipStream_t)stream;
    // the search starts at the robot's progress so far and writes nearest_u over it
    // (under a frame the pose is the robot's frame value and the search runs at its map position)
    int rc = hip_err(launch_path_nearest(B, segs, seg_stride, nseg, pose, b->rframe.view64(), b->capacity, path_u,
                                         nullptr, b->prm.model == NMPC_MODEL_OMNI4AMR ? 1 : 0, path_u, nullptr, err, s),
                     "path_nearest launch");
    if (rc) return rc;
    rc = nmpc_batch_run_path(b, B, pose, vel, steer, segs, seg_stride, nseg, path_u, sample_period, is_holonomic,
                             reset, traj_out, cmd, u0, status, qp_iter, qp_res, stream);
    if (rc || !guard) return rc;
    return hip_err(launch_path_guard(B, err, max_pos_err, max_ori_err, use_pos, use_ori, off_path, cmd, s),
                   "path_guard launch");
}

int nmpc_node_params_default(nmpc_node_params* np)
{
    if (!np) return set_err(NMPC_ERR_ARG, "node params is NULL");
    std::memset(np, 0, sizeof(*np));
    const double deg = M_PI / 180.0;
    np->final_pos_err = 0.01;        // nmpc_nav_control.yaml:7
    np->final_ori_err = 1.0 * deg;   // :8
    np->enable_safe_conditions = 1;  // :10
    np->max_goal_dist = 2.0;         // :11
    np->max_pos_err = 0.5;           // :12
    np->max_ori_err = 60.0 * deg;    // :13
    np->final_ori_signed = 1;        // NMPCNavControlROS.cpp:638-639 compares the signed angle
    np->sample_period = 1.0 / 40.0;  // getDeltaTime(): nmpc_nav_control_acados_models.yaml:28
    np->is_holonomic = 0;            // NMPCNavControlROS.cpp:666
    return NMPC_OK;
}

int nmpc_path_queue_default(nmpc_path_queue* q)
{
    if (!q) return set_err(NMPC_ERR_ARG, "path queue is NULL");
    std::memset(q, 0, sizeof(*q));
    q->part_length = 1000.0;  // NMPCNavControlROS.cpp:571
    q->max_active_len = 5.0;  // nmpc_nav_control.yaml:6
    return NMPC_OK;
}

namespace {

// the argument checks of a node tick, those that need no handle first; *go: there is work (B > 0)
int node_tick_check(const nmpc_batch* b, int B, const nmpc_node_params* np, const nmpc_path_queue* q,
                    const unsigned char* mode, const float* pose, const float* vel, const nmpc_path_segment* segs,
                    int seg_stride, const int* nseg, const double* path_u, bool* go)
{
    *go = false;
    if (!np) return set_err(NMPC_ERR_ARG, "node params is NULL");
    if (q) {
        if (segs && !(q->npart && q->head && q->tail))
            return set_err(NMPC_ERR_ARG, "path queue: npart, head and tail are required with segs");
        if (!std::isfinite(q->part_length) || !std::isfinite(q->max_active_len))
            return set_err(NMPC_ERR_ARG, "path queue: part_length and max_active_len must be finite");
    }
    if (B < 0) return set_err(NMPC_ERR_ARG, "B out of range [0, capacity]");
    if (!mode) return set_err(NMPC_ERR_ARG, "mode is required");
    if (segs && seg_stride < 1) return set_err(NMPC_ERR_ARG, "seg_stride < 1");
    if (!std::isfinite(np->sample_period) || np->sample_period < 0.0)
        return set_err(NMPC_ERR_ARG, "sample_period must be finite and >= 0");
    if (const int rc = check_batch(b, B)) return rc;
    if (B == 0) return NMPC_OK;
    if (!pose || !vel) return set_err(NMPC_ERR_ARG, "pose and vel are required");
    const bool paths = segs && (q || nseg) && path_u;
    if (paths && node_gate_lds_bytes(b->prm.N) > 65536)
        return set_err(NMPC_ERR_UNSUPPORTED, "horizon too long for the gate's path march");
    *go = true;
    return NMPC_OK;
}

// nmpc_batch_node_tick (q == nullptr) and nmpc_batch_node_tick_queue (q given, nseg unused)
int node_tick(nmpc_batch* b, int B, const nmpc_node_params* np, const nmpc_path_queue* q, unsigned char* mode,
              const float* pose, const float* vel, const float* steer, const float* goal,
              const nmpc_path_segment* segs, int seg_stride, const int* nseg, double* path_u, unsigned char* reset,
              unsigned char* event, double* err, float* traj_out, int* n_solved, float* cmd, float* u0, int* status,
              int* qp_iter, float* qp_res, void* stream)
{
    bool go = false;
    if (const int rc = node_tick_check(b, B, np, q, mode, pose, vel, segs, seg_stride, nseg, path_u, &go)) return rc;
    if (!go) return NMPC_OK;
    const bool paths = segs && (q || nseg) && path_u;
    hipStream_t s = (hipStream_t)stream;
    if (!b->node_traj) {
        const size_t S = (size_t)b->capacity;
        hipError_t e;
        if ((e = hipMalloc(&b->node_len, sizeof(int) * S)) != hipSuccess ||
            (e = hipMalloc(&b->node_active, S)) != hipSuccess ||
            (e = hipMalloc(&b->node_n, sizeof(int))) != hipSuccess ||
            (e = hipMalloc(&b->node_status, sizeof(int) * S)) != hipSuccess ||
            (e = hipMalloc(&b->node_traj, sizeof(float) * 3 * (size_t)(b->prm.N + 1) * S)) != hipSuccess)
            return hip_err(e, "hipMalloc");
    }
    if (!status) status = b->node_status;  // (the finish launch reads it)
    NodeGateArgs g;
    std::memset(&g, 0, sizeof(g));
    g.B = B;
    g.N = b->prm.N;
    g.nu = b->nu;
    g.seg_stride = paths ? seg_stride : 1;
    g.holo_err = b->prm.model == NMPC_MODEL_OMNI4AMR ? 1 : 0;  // NMPCNavControlROS.cpp:654
    g.np = *np;
    g.mode = mode;
    g.pose = pose;
    g.goal = goal;
    g.origin = b->rframe.view64();
    g.ostride = b->capacity;
    g.segs = paths ? segs : nullptr;
    g.nseg = (paths && !q) ? nseg : nullptr;
    g.path_u = paths ? path_u : nullptr;
    if (q) {
        g.queue = 1;
        g.q = *q;
    }
    g.event = event;
    g.err = err;
    g.traj = b->node_traj;
    g.traj_len = b->node_len;
    g.active = b->node_active;
    g.traj_out = traj_out;
    g.cmd = cmd;
    g.u0 = u0;
    g.qp_res = qp_res;
    g.status = status;
    g.qp_iter = qp_iter;
    int rc = hip_err(launch_node_gate(g, s), "node_gate launch");
    if (rc) return rc;
    // nmpc_batch_run's launch on the gate's references, for the compacted robots
    KArgs a = run_args(b, B, pose, vel, steer, reset, cmd, u0, status, qp_iter, qp_res);
    a.traj = b->node_traj;
    a.traj_len = b->node_len;
    a.n_active = b->node_n;
    rc = hip_err(launch(b, a, kModeRun, s), "node_tick solve launch");
    if (rc) return rc;
    return hip_err(launch_node_finish(B, b->node_active, status, b->node_n, mode, event, reset, n_solved,
                                      q ? q->remains : nullptr, s),
                   "node_finish launch");
}

}  // namespace

int nmpc_batch_node_tick(nmpc_batch* b, int B, const nmpc_node_params* np, unsigned char* mode, const float* pose,
                         const float* vel, const float* steer, const float* goal, const nmpc_path_segment* segs,
                         int seg_stride, const int* nseg, double* path_u, unsigned char* reset, unsigned char* event,
                         double* err, float* traj_out, int* n_solved, float* cmd, float* u0, int* status,
                         int* qp_iter, float* qp_res, void* stream)
{
    const TraceRange trace("nmpc_batch_node_tick");
    return node_tick(b, B, np, nullptr, mode, pose, vel, steer, goal, segs, seg_stride, nseg, path_u, reset, event,
                     err, traj_out, n_solved, cmd, u0, status, qp_iter, qp_res, stream);
}

int nmpc_batch_node_tick_queue(nmpc_batch* b, int B, const nmpc_node_params* np, const nmpc_path_queue* q,
                               unsigned char* mode, const float* pose, const float* vel, const float* steer,
                               const float* goal, const nmpc_path_segment* segs, int seg_stride, double* path_u,
                               unsigned char* reset, unsigned char* event, double* err, float* traj_out,
                               int* n_solved, float* cmd, float* u0, int* status, int* qp_iter, float* qp_res,
                               void* stream)
{
    const TraceRange trace("nmpc_batch_node_tick_queue");
    if (!q) return set_err(NMPC_ERR_ARG, "path queue is NULL");
    return node_tick(b, B, np, q, mode, pose, vel, steer, goal, segs, seg_stride, nullptr, path_u, reset, event, err,
                     traj_out, n_solved, cmd, u0, status, qp_iter, qp_res, stream);
}

int nmpc_batch_enable_input(nmpc_batch* b, int depth)
{
    if (depth < 2 || depth > 64) return set_err(NMPC_ERR_ARG, "input depth out of range [2, 64]");
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (b->in_st.depth) {
        if (b->in_st.depth == depth) return NMPC_OK;
        return set_err(NMPC_ERR_ARG, "input state is enabled with another depth");
    }
    const size_t S = (size_t)b->capacity, D = (size_t)depth;
    NodeInputState st{};
    st.cap = b->capacity;
    st.depth = depth;
    // everything starts as 0: empty rings, and held values where the reference has uninitialised members
    auto zeroed = [&](auto** p, size_t n) {
        const size_t bytes = sizeof(**p) * n;
        hipError_t e = hipMalloc(p, bytes);
        return e != hipSuccess ? e : hipMemset(*p, 0, bytes);
    };
    hipError_t e;
    if ((e = zeroed(&st.stamp, D * S)) != hipSuccess || (e = zeroed(&st.sample, D * 3 * S)) != hipSuccess ||
        (e = zeroed(&st.count, S)) != hipSuccess || (e = zeroed(&st.newest, S)) != hipSuccess ||
        (e = zeroed(&st.held, 7 * S)) != hipSuccess || (e = zeroed(&b->in_pose, 3 * S)) != hipSuccess ||
        (e = zeroed(&b->in_vel, 3 * S)) != hipSuccess || (e = zeroed(&b->in_goal, 3 * S)) != hipSuccess ||
        (e = zeroed(&b->in_steer, S)) != hipSuccess || (e = zeroed(&b->in_valid, S)) != hipSuccess ||
        (e = hipStreamSynchronize(nullptr)) != hipSuccess) {
        for (void* p : {(void*)st.stamp, (void*)st.sample, (void*)st.count, (void*)st.newest, (void*)st.held,
                        (void*)b->in_pose, (void*)b->in_vel, (void*)b->in_goal, (void*)b->in_steer, (void*)b->in_valid})
            (void)hipFree(p);
        b->in_pose = b->in_vel = b->in_goal = b->in_steer = nullptr;
        b->in_valid = nullptr;
        return hip_err(e, "hipMalloc");
    }
    b->in_st = st;
    return NMPC_OK;
}

int nmpc_batch_input_state(nmpc_batch* b, long long** stamp, double** sample, int** count, int** newest, double** held,
                           int* depth, int* stride)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (stamp) *stamp = b->in_st.stamp;
    if (sample) *sample = b->in_st.sample;
    if (count) *count = b->in_st.count;
    if (newest) *newest = b->in_st.newest;
    if (held) *held = b->in_st.held;
    if (depth) *depth = b->in_st.depth;
    if (stride) *stride = b->capacity;
    return NMPC_OK;
}

int nmpc_batch_push_samples(nmpc_batch* b, int B, const long long* stamp_ns, const double* sample,
                            const unsigned char* mask, unsigned char* dropped, void* stream)
{
    if (B < 0) return set_err(NMPC_ERR_ARG, "B out of range [0, capacity]");
    if (!stamp_ns || !sample) return set_err(NMPC_ERR_ARG, "push_samples: stamp_ns and sample are required");
    if (const int rc = check_batch(b, B)) return rc;
    if (!b->in_st.depth) return set_err(NMPC_ERR_ARG, "the input state is not enabled (nmpc_batch_enable_input)");
    return hip_err(launch_push_samples(b->in_st, B, stamp_ns, sample, mask, dropped, (hipStream_t)stream),
                   "push_samples launch");
}

int nmpc_node_input_default(nmpc_node_input* in)
{
    if (!in) return set_err(NMPC_ERR_ARG, "node input is NULL");
    std::memset(in, 0, sizeof(*in));
    in->period_ns = 25000000;         // Duration(1.0 / control_freq), nmpc_nav_control.yaml:4
    in->transform_timeout = 0.1;      // :5
    in->pose_valid_overwritten = 1;   // NMPCNavControlROS.cpp:549-550
    in->recentre_radius = INFINITY;
    return NMPC_OK;
}

namespace {
// The stage's launch. mode_rw: the cycle's mode array under strict, else nullptr; goal_out may be the handle's buffer.
// *res: the stage's arguments with the handle's buffers where the caller keeps none
int node_input(nmpc_batch* b, int B, const nmpc_node_input* in, const unsigned char* mode, unsigned char* mode_rw,
               const double* goal_map, float* goal_out, hipStream_t s, nmpc_node_input* res)
{
    NodeInputArgs a;
    std::memset(&a, 0, sizeof(a));
    a.st = b->in_st;
    a.B = B;
    a.tric = b->prm.model == NMPC_MODEL_TRIC3AMR ? 1 : 0;
    a.in = *in;
    if (!a.in.valid) a.in.valid = b->in_valid;
    if (!a.in.pose) a.in.pose = b->in_pose;
    if (!a.in.vel) a.in.vel = b->in_vel;
    if (!a.in.steer_out) a.in.steer_out = b->in_steer;
    a.mode = mode;
    a.mode_rw = mode_rw;
    a.goal_map = goal_map;
    a.goal_out = goal_out;
    if (std::isfinite(in->recentre_radius))  // a frame table that is off is started, as nmpc_batch_recentre does
        if (const int rc = rf_table(b, s)) return rc;
    a.fr = b->rframe.view64();
    a.xbar = b->xbar;
    a.N = b->prm.N;
    a.nx = b->nx;
    if (res) *res = a.in;
    return hip_err(launch_node_input(a, s), "node_input launch");
}
}  // namespace

int nmpc_batch_node_input(nmpc_batch* b, int B, const nmpc_node_input* in, const unsigned char* mode,
                          const double* goal_map, float* goal_out, void* stream)
{
    const TraceRange trace("nmpc_batch_node_input");
    if (B < 0) return set_err(NMPC_ERR_ARG, "B out of range [0, capacity]");
    if (!in) return set_err(NMPC_ERR_ARG, "node input is NULL");
    if (!mode) return set_err(NMPC_ERR_ARG, "mode is required");
    if (const int rc = check_batch(b, B)) return rc;
    if (!b->in_st.depth) return set_err(NMPC_ERR_ARG, "the input state is not enabled (nmpc_batch_enable_input)");
    if (B == 0) return NMPC_OK;
    return node_input(b, B, in, mode, nullptr, goal_map, goal_out, (hipStream_t)stream, nullptr);
}

int nmpc_batch_node_cycle(nmpc_batch* b, int B, const nmpc_node_params* np, const nmpc_path_queue* q,
                          const nmpc_node_input* in, unsigned char* mode, const double* goal_map,
                          const nmpc_path_segment* segs, int seg_stride, const int* nseg, double* path_u,
                          unsigned char* reset, unsigned char* event, double* err, float* traj_out, int* n_solved,
                          float* cmd, float* u0, int* status, int* qp_iter, float* qp_res, void* stream)
{
    const TraceRange trace("nmpc_batch_node_cycle");
    if (!in) return set_err(NMPC_ERR_ARG, "node input is NULL");
    // every check of the tick before the stage changes anything (pose and vel are the stage's: never NULL)
    bool go = false;
    const float some = 0.0f;
    if (const int rc = node_tick_check(b, B, np, q, mode, &some, &some, segs, seg_stride, q ? nullptr : nseg, path_u, &go))
        return rc;
    if (!b->in_st.depth) return set_err(NMPC_ERR_ARG, "the input state is not enabled (nmpc_batch_enable_input)");
    if (b->trk_on && b->trk.own_first >= 0 && (long long)b->trk.own_first + B > b->trk.M)
        return set_err(NMPC_ERR_ARG, "tracks: own_first + B exceeds M");
    const bool guarded = b->trk_on && b->sguard_on;  // (a guard without tracks is inert)
    if (guarded) {
        if (const char* bad = bad_guard(&b->sguard, b->seprule.range, b->trk.own_first)) return set_err(NMPC_ERR_ARG, bad);
    }
    if (!go) return NMPC_OK;
    hipStream_t s = (hipStream_t)stream;
    nmpc_node_input r;
    float* const goal = goal_map ? b->in_goal : nullptr;
    int rc = node_input(b, B, in, mode, in->strict ? mode : nullptr, goal_map, goal, s, &r);
    if (rc) return rc;
    if (b->trk_on) {
        // fleet separation: the handle's own horizons into the track buffer, then the stage limits of the robots that
        // are about to solve from the tracks and, if one is attached, the speed map
        // (a robot held on entry is exported as a standing obstacle at its pose)
        if (b->trk_export) {
            rc = hip_err(export_tracks(b, B, r.pose, reset, mode, const_cast<double*>(b->trk.xy), b->trk.M, b->trk.K,
                                       b->trk.own_first, s, guarded ? b->sep_held : nullptr), "export_tracks launch");
            if (rc) return rc;
        }
        if ((rc = sb_table(b, s)) || (rc = sep_scratch(b, b->trk.M))) return rc;
        rc = hip_err(tracks_write(b, B, b->trk, b->seprule, b->smap_on ? &b->smap : nullptr,
                                  b->smap_on ? b->srule : speed_rule_default(), r.pose, reset, nullptr, mode, nullptr,
                                  nullptr, s, guarded ? &b->sguard : nullptr), "separation launch");
        if (rc) return rc;
        // the protective hold: a held robot is parked in IDLE for the gate; the status launch brings its mode back
        if (guarded) {
            rc = hip_err(sep_hold(b, B, b->sguard, mode, reset, nullptr, mode, q ? q->remains : nullptr, s),
                         "sep_hold launch");
            if (rc) return rc;
        }
    } else if (b->smap_on) {
        // speed zones: the stage limits of the robots that are about to solve, from the stage's pose (under strict an
        // invalid robot's mode is ERROR by now: its rows stay)
        if ((rc = sb_table(b, s))) return rc;
        rc = hip_err(speed_map_write(b, B, &b->smap, b->srule, r.pose, reset, nullptr, mode, nullptr, s),
                     "speed_map launch");
        if (rc) return rc;
    }
    const float* const steer = b->prm.model == NMPC_MODEL_TRIC3AMR ? r.steer_out : nullptr;
    rc = node_tick(b, B, np, q, mode, r.pose, r.vel, steer, goal, segs, seg_stride, q ? nullptr : nseg, path_u, reset,
                   event, err, traj_out, n_solved, cmd, u0, status, qp_iter, qp_res, stream);
    if (rc) return rc;
    return hip_err(launch_cycle_status(B, r.valid, in->strict ? 1 : 0, mode, event, q ? q->remains : nullptr,
                                       guarded ? b->sep_held : nullptr, b->sep_mode_save, b->sep_remains_save, s),
                   "cycle_status launch");
}

int nmpc_batch_set_kernel(nmpc_batch* b, int kernel)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (kernel != NMPC_KERNEL_TEAM) return set_err(NMPC_ERR_UNSUPPORTED, "unknown kernel (only NMPC_KERNEL_TEAM)");
    return NMPC_OK;
}

int nmpc_batch_set_schedule(nmpc_batch* b, int mode)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (mode < NMPC_SCHED_OFF || mode > NMPC_SCHED_SPREAD) return set_err(NMPC_ERR_ARG, "unknown schedule");
    b->sched = mode;
    return NMPC_OK;
}

int nmpc_batch_state(nmpc_batch* b, float** xbar, float** ubar, float** carried, int* stride)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (xbar) *xbar = b->xbar;
    if (ubar) *ubar = b->ubar;
    if (carried) *carried = b->carried;
    if (stride) *stride = b->capacity;
    return NMPC_OK;
}

int nmpc_batch_forget_warm(nmpc_batch* b, int B, const unsigned char* mask, void* stream)
{
    if (const int rc = check_batch(b, B)) return rc;
    return hip_err(launch_forget_warm(b->warm, mask, B, (hipStream_t)stream), "forget_warm launch");
}

int nmpc_batch_set_robot_params(nmpc_batch* b, int B, const nmpc_robot_params* rp, const unsigned char* mask,
                                void* stream)
{
    const char* bad = !rp ? "robot params is NULL"
                      : (!rp->lbx && !rp->ubx && !rp->lbu && !rp->ubu && !rp->W && !rp->W_e)
                          ? "robot params: every field is NULL"
                          : nullptr;
    return table_write(b, B, bad, rp_table, stream, "robot_params launch", [&](hipStream_t s) {
        const float* const fields[kRpFields] = {rp->lbx, rp->ubx, rp->lbu, rp->ubu, rp->W, rp->W_e};
        return launch_rows_set<kRpFields>(b->rparams.p, b->capacity, B, b->rp.off, fields, mask, s);
    });
}

int nmpc_batch_set_robot_limits(nmpc_batch* b, int B, const float* v_max, const float* a_max, const float* alpha_min,
                                const float* alpha_max, const float* dalpha_max, const unsigned char* mask,
                                void* stream)
{
    const char* bad = no_limits(v_max, a_max, alpha_min, alpha_max, dalpha_max, "robot limits: every array is NULL");
    return table_write(b, B, bad, rp_table, stream, "robot_limits launch", [&](hipStream_t s) {
        return launch_rp_limits(b->rparams.p, b->capacity, B, b->rp, b->prm.model == NMPC_MODEL_TRIC3AMR ? 1 : 0, v_max,
                                a_max, alpha_min, alpha_max, dalpha_max, mask, s);
    });
}

int nmpc_batch_robot_params(nmpc_batch* b, float** table, int* rows, int* stride)
{
    return rows_view(b, &nmpc_batch::rparams, table, rows, stride);
}

int nmpc_batch_clear_robot_params(nmpc_batch* b) { return table_clear(b, &nmpc_batch::rparams); }

int nmpc_batch_set_stage_bounds(nmpc_batch* b, int B, const nmpc_stage_bounds* sb, const unsigned char* mask,
                                void* stream)
{
    const char* bad = !sb ? "stage bounds is NULL"
                      : (!sb->lbx && !sb->ubx && !sb->lbu && !sb->ubu) ? "stage bounds: every field is NULL"
                                                                       : nullptr;
    return table_write(b, B, bad, sb_table, stream, "stage_bounds launch", [&](hipStream_t s) {
        return launch_sb_set(b->sbounds.p, sb_dims(b), B, *sb, mask, s);
    });
}

int nmpc_batch_set_stage_limits(nmpc_batch* b, int B, const float* v_max, const float* a_max, const float* alpha_min,
                                const float* alpha_max, const float* dalpha_max, const unsigned char* mask,
                                void* stream)
{
    const char* bad = no_limits(v_max, a_max, alpha_min, alpha_max, dalpha_max, "stage limits: every array is NULL");
    return table_write(b, B, bad, sb_table, stream, "stage_limits launch", [&](hipStream_t s) {
        return launch_sb_limits(b->sbounds.p, sb_dims(b), B, b->prm.model == NMPC_MODEL_TRIC3AMR ? 1 : 0, v_max, a_max,
                                alpha_min, alpha_max, dalpha_max, mask, s);
    });
}

int nmpc_batch_shift_stage_bounds(nmpc_batch* b, int B, int n, const unsigned char* mask, void* stream)
{
    const char* bad = n < 0 ? "stage shift: n must be >= 0" : nullptr;
    return table_write(b, B, bad, sb_table, stream, "stage_shift launch",
                       [&](hipStream_t s) { return launch_sb_shift(b->sbounds.p, sb_dims(b), B, n, mask, s); });
}

int nmpc_batch_stage_bounds(nmpc_batch* b, void** table, size_t* bytes)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (table) *table = b->sbounds.view();
    if (bytes) *bytes = b->sbounds.on ? sizeof(float) * b->sbounds.floats : 0;
    return NMPC_OK;
}

int nmpc_batch_clear_stage_bounds(nmpc_batch* b) { return table_clear(b, &nmpc_batch::sbounds); }

int nmpc_speed_map_default(nmpc_speed_map* map)
{
    if (!map) return set_err(NMPC_ERR_ARG, "speed map is NULL");
    std::memset(map, 0, sizeof(*map));
    map->outside = INFINITY;
    return NMPC_OK;
}

int nmpc_speed_rule_default(nmpc_speed_rule* rule)
{
    if (!rule) return set_err(NMPC_ERR_ARG, "speed rule is NULL");
    *rule = speed_rule_default();
    return NMPC_OK;
}

int nmpc_batch_stage_limits_from_map(nmpc_batch* b, int B, const nmpc_speed_map* map, const nmpc_speed_rule* rule,
                                     const float* pose, const unsigned char* reset, const unsigned char* mask,
                                     float* vlim, void* stream)
{
    const TraceRange trace("nmpc_batch_stage_limits_from_map");
    const char* bad = bad_speed_map(map, rule);
    if (!bad && reset && !pose) bad = "speed map: reset needs pose";
    return table_write(b, B, bad, sb_table, stream, "speed_map launch", [&](hipStream_t s) {
        return speed_map_write(b, B, map, rule ? *rule : speed_rule_default(), pose, reset, mask, nullptr, vlim, s);
    });
}

int nmpc_batch_set_speed_map(nmpc_batch* b, const nmpc_speed_map* map, const nmpc_speed_rule* rule)
{
    if (map)
        if (const char* bad = bad_speed_map(map, rule)) return set_err(NMPC_ERR_ARG, bad);
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    b->smap_on = map != nullptr;
    if (map) {
        b->smap = *map;
        b->srule = rule ? *rule : speed_rule_default();
    }
    return NMPC_OK;
}

int nmpc_tracks_default(nmpc_tracks* tracks)
{
    if (!tracks) return set_err(NMPC_ERR_ARG, "tracks is NULL");
    std::memset(tracks, 0, sizeof(*tracks));
    tracks->own_first = -1;
    return NMPC_OK;
}

int nmpc_sep_rule_default(nmpc_sep_rule* sep)
{
    if (!sep) return set_err(NMPC_ERR_ARG, "separation rule is NULL");
    *sep = sep_rule_default();
    return NMPC_OK;
}

int nmpc_batch_export_tracks(nmpc_batch* b, int B, const float* pose, const unsigned char* reset,
                             const unsigned char* mode, double* xy, int M, int K, int first, void* stream)
{
    const TraceRange trace("nmpc_batch_export_tracks");
    if (B < 0) return set_err(NMPC_ERR_ARG, "B out of range [0, capacity]");
    if (first < 0 || (long long)first + B > M) return set_err(NMPC_ERR_ARG, "export tracks: first out of range [0, M - B]");
    if (K < 0) return set_err(NMPC_ERR_ARG, "export tracks: K must be >= 0");
    if (!xy) return set_err(NMPC_ERR_ARG, "export tracks: xy is NULL");
    if ((reset || mode) && !pose) return set_err(NMPC_ERR_ARG, "export tracks: reset and mode need pose");
    if (const int rc = check_batch(b, B)) return rc;
    if (B == 0) return NMPC_OK;
    return hip_err(export_tracks(b, B, pose, reset, mode, xy, M, K, first, (hipStream_t)stream), "export_tracks launch");
}

int nmpc_batch_stage_limits_from_tracks(nmpc_batch* b, int B, const nmpc_tracks* tracks, const nmpc_sep_rule* sep,
                                        const nmpc_speed_map* map, const nmpc_speed_rule* rule, const float* pose,
                                        const unsigned char* reset, const unsigned char* mask, float* vlim, float* gap,
                                        void* stream)
{
    const TraceRange trace("nmpc_batch_stage_limits_from_tracks");
    const char* bad = bad_tracks(tracks, sep, B);
    if (!bad) bad = map ? bad_speed_map(map, rule) : bad_speed_rule(rule);
    if (!bad && reset && !pose) bad = "tracks: reset needs pose";
    return table_write(b, B, bad, sb_table, stream, "separation launch", [&](hipStream_t s) {
        if (sep_scratch(b, tracks->M)) return hipErrorOutOfMemory;
        return tracks_write(b, B, *tracks, sep ? *sep : sep_rule_default(), map, rule ? *rule : speed_rule_default(),
                            pose, reset, mask, nullptr, vlim, gap, s);
    });
}

int nmpc_sep_guard_default(nmpc_sep_guard* g)
{
    if (!g) return set_err(NMPC_ERR_ARG, "separation guard is NULL");
    *g = sep_guard_default();
    return NMPC_OK;
}

int nmpc_batch_stage_limits_from_tracks_ex(nmpc_batch* b, int B, const nmpc_tracks* tracks, const nmpc_sep_rule* sep,
                                           const nmpc_sep_guard* guard, const nmpc_speed_map* map,
                                           const nmpc_speed_rule* rule, const float* pose, const unsigned char* reset,
                                           const unsigned char* mask, float* vlim, float* gap, float* gap_all,
                                           void* stream)
{
    const TraceRange trace("nmpc_batch_stage_limits_from_tracks_ex");
    const char* bad = bad_tracks(tracks, sep, B);
    if (!bad) bad = map ? bad_speed_map(map, rule) : bad_speed_rule(rule);
    if (!bad && reset && !pose) bad = "tracks: reset needs pose";
    if (!bad) bad = bad_guard(guard, sep ? sep->range : sep_rule_default().range, tracks->own_first);
    if (!bad && gap_all && !guard) bad = "tracks: gap_all needs a guard";
    if (!bad && guard && !pose) bad = "separation guard: pose is required (a held robot stands at it)";
    return table_write(b, B, bad, sb_table, stream, "separation launch", [&](hipStream_t s) {
        if (sep_scratch(b, tracks->M) || (guard && guard_scratch(b))) return hipErrorOutOfMemory;
        return tracks_write(b, B, *tracks, sep ? *sep : sep_rule_default(), map, rule ? *rule : speed_rule_default(),
                            pose, reset, mask, nullptr, vlim, gap, s, guard, gap_all);
    });
}

int nmpc_batch_sep_hold(nmpc_batch* b, int B, const nmpc_sep_guard* guard, const unsigned char* mode,
                        const unsigned char* reset, unsigned char* held_out, void* stream)
{
    const TraceRange trace("nmpc_batch_sep_hold");
    if (B < 0) return set_err(NMPC_ERR_ARG, "B out of range [0, capacity]");
    if (!guard) return set_err(NMPC_ERR_ARG, "separation guard is NULL");
    if (const char* bad = bad_guard(guard, -1.0f, -2)) return set_err(NMPC_ERR_ARG, bad);
    if (const int rc = check_batch(b, B)) return rc;
    if (!b->sep_qa_ready)
        return set_err(NMPC_ERR_ARG, "sep_hold: no nmpc_batch_stage_limits_from_tracks_ex call with a guard came before");
    return hip_err(sep_hold(b, B, *guard, mode, reset, held_out, nullptr, nullptr, (hipStream_t)stream),
                   "sep_hold launch");
}

int nmpc_batch_set_sep_guard(nmpc_batch* b, const nmpc_sep_guard* guard)
{
    if (const char* bad = bad_guard(guard, -1.0f, -2)) return set_err(NMPC_ERR_ARG, bad);
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (guard)
        if (const int rc = guard_scratch(b)) return rc;
    if (const int rc = guard_clear_held(b)) return rc;
    b->sguard_on = guard != nullptr;
    if (guard) b->sguard = *guard;
    return NMPC_OK;
}

int nmpc_batch_sep_state(nmpc_batch* b, unsigned char** held)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (const int rc = guard_scratch(b)) return rc;
    if (held) *held = b->sep_held;
    return NMPC_OK;
}

int nmpc_batch_set_tracks(nmpc_batch* b, const nmpc_tracks* tracks, const nmpc_sep_rule* sep, int export_own)
{
    if (tracks) {
        if (const char* bad = bad_tracks(tracks, sep, -1)) return set_err(NMPC_ERR_ARG, bad);
        if (export_own && tracks->own_first < 0) return set_err(NMPC_ERR_ARG, "tracks: export_own needs own_first >= 0");
    }
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    b->trk_on = tracks != nullptr;
    if (tracks) {
        b->trk = *tracks;
        b->seprule = sep ? *sep : sep_rule_default();
        b->trk_export = export_own != 0;
    }
    return NMPC_OK;
}

int nmpc_batch_set_robot_model(nmpc_batch* b, int B, const float* p, const unsigned char* mask, void* stream)
{
    return table_write(b, B, p ? nullptr : "robot model: p is NULL", rm_table, stream, "robot_model launch",
                       [&](hipStream_t s) {
                           const int off[2] = {0, b->np};  // the one field p
                           const float* const fields[1] = {p};
                           return launch_rows_set<1>(b->rmodel.p, b->capacity, B, off, fields, mask, s);
                       });
}

int nmpc_batch_robot_model(nmpc_batch* b, float** table, int* rows, int* stride)
{
    return rows_view(b, &nmpc_batch::rmodel, table, rows, stride);
}

int nmpc_batch_clear_robot_model(nmpc_batch* b) { return table_clear(b, &nmpc_batch::rmodel); }

int nmpc_batch_set_robot_frame(nmpc_batch* b, int B, const double* origin, const unsigned char* mask, void* stream)
{
    return table_write(b, B, origin ? nullptr : "robot frame: origin is NULL", rf_table, stream, "robot_frame launch",
                       [&](hipStream_t s) { return frame_set(b, B, origin, nullptr, 0.0, nullptr, mask, s); });
}

int nmpc_batch_recentre(nmpc_batch* b, int B, const double* pose_map, double radius, const unsigned char* mask,
                        unsigned char* moved, void* stream)
{
    return table_write(b, B, pose_map ? nullptr : "recentre: pose_map is NULL", rf_table, stream, "recentre launch",
                       [&](hipStream_t s) { return frame_set(b, B, nullptr, pose_map, radius, moved, mask, s); });
}

namespace {
// the checks nmpc_batch_to_frame and _from_frame share, those that need no handle first; *go: there is work
int frame_map_check(const nmpc_batch* b, int B, const void* src, const void* dst, int n, int c, bool* go)
{
    if (B < 0) return set_err(NMPC_ERR_ARG, "B out of range [0, capacity]");
    if (n < 0) return set_err(NMPC_ERR_ARG, "frame: n must be >= 0");
    if (c < 2) return set_err(NMPC_ERR_ARG, "frame: c must be >= 2");
    if (!src || !dst) return set_err(NMPC_ERR_ARG, "frame: the input and output arrays are required");
    if (const int rc = check_batch(b, B)) return rc;
    *go = B > 0 && n > 0;
    return NMPC_OK;
}
}  // namespace

int nmpc_batch_to_frame(nmpc_batch* b, int B, const double* map, int n, int c, float* out, void* stream)
{
    bool go = false;
    if (const int rc = frame_map_check(b, B, map, out, n, c, &go)) return rc;
    if (!go) return NMPC_OK;
    return hip_err(launch_to_frame(b->rframe.view64(), b->capacity, B, n, c, map, out, (hipStream_t)stream),
                   "to_frame launch");
}

int nmpc_batch_from_frame(nmpc_batch* b, int B, const float* in, int n, int c, double* map, void* stream)
{
    bool go = false;
    if (const int rc = frame_map_check(b, B, in, map, n, c, &go)) return rc;
    if (!go) return NMPC_OK;
    return hip_err(launch_from_frame(b->rframe.view64(), b->capacity, B, n, c, in, map, (hipStream_t)stream),
                   "from_frame launch");
}

int nmpc_batch_robot_frame(nmpc_batch* b, double** table, int* stride)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (table) *table = b->rframe.view64();
    if (stride) *stride = b->capacity;
    return NMPC_OK;
}

int nmpc_batch_clear_robot_frame(nmpc_batch* b, void* stream)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (!b->rframe.on) return NMPC_OK;
    // every robot's iterate back to map coordinates (origin zero for the whole capacity), then off
    const int rc = hip_err(frame_set(b, b->capacity, nullptr, nullptr, 0.0, nullptr, nullptr, (hipStream_t)stream),
                           "robot_frame clear launch");
    if (rc == NMPC_OK) b->rframe.on = false;
    return rc;
}

int nmpc_batch_set_record_layout(nmpc_batch* b, int layout)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (layout != NMPC_REC_AUTO && layout != NMPC_REC_WIDE && layout != NMPC_REC_SPLIT)
        return set_err(NMPC_ERR_ARG, "layout must be NMPC_REC_AUTO, NMPC_REC_WIDE or NMPC_REC_SPLIT");
    const int want = layout == NMPC_REC_AUTO ? rec_layout_auto(b) : layout;
    if ((b->prm.model == NMPC_MODEL_TRIC3AMR && want != NMPC_REC_SPLIT) ||
        (b->prm.model == NMPC_MODEL_OMNI4AMR && want != NMPC_REC_WIDE))
        return set_err(NMPC_ERR_UNSUPPORTED, "this model's team kernel has one record layout (tric split, omni4 wide)");
    b->rec_split = want;  // robots warm-started in the other layout start cold at their next solve (warm tags)
    return NMPC_OK;
}

int nmpc_batch_plan_ex(const nmpc_batch* b, int B, int mode, nmpc_launch_plan* plan)
{
    if (!b || !plan) return set_err(NMPC_ERR_ARG, "NULL argument");
    if (B < 0 || B > b->capacity) return set_err(NMPC_ERR_ARG, "B out of range");
    if (mode != NMPC_PLAN_SOLVE && mode != NMPC_PLAN_RUN && mode != NMPC_PLAN_RUN_PATH)
        return set_err(NMPC_ERR_ARG, "mode must be NMPC_PLAN_SOLVE, NMPC_PLAN_RUN or NMPC_PLAN_RUN_PATH");
    // the plan schedule() launches from (a run_path launch marches its paths in the kernel)
    const LaunchPlan p = plan_launch(b, B, mode == NMPC_PLAN_RUN_PATH, mode == NMPC_PLAN_SOLVE ? kModeSolve : kModeRun);
    plan->kernel = p.waves ? 1 : 0;
    plan->waves_per_robot = p.waves;
    plan->segments = p.waves ? p.seg : 0;  // (the team kernel reports none, with or without the hand-off)
    plan->record_layout = p.rec_split ? NMPC_REC_SPLIT : NMPC_REC_WIDE;
    plan->warm_tag = p.warm_tag;
    plan->record_bytes = rec_footprint(b);
    return NMPC_OK;
}

int nmpc_batch_set_handoff(nmpc_batch* b, int iteration)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (iteration < 0 && iteration != NMPC_HANDOFF_AUTO)
        return set_err(NMPC_ERR_ARG, "the hand-off iteration must be >= 0 (0: off) or NMPC_HANDOFF_AUTO");
    b->handoff = iteration;
    return NMPC_OK;
}

int nmpc_batch_plan_handoff(const nmpc_batch* b, int B, int mode, int* iteration, int* segments, size_t* lds_bytes)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (B < 0 || B > b->capacity) return set_err(NMPC_ERR_ARG, "B out of range");
    if (mode != NMPC_PLAN_SOLVE && mode != NMPC_PLAN_RUN && mode != NMPC_PLAN_RUN_PATH)
        return set_err(NMPC_ERR_ARG, "mode must be NMPC_PLAN_SOLVE, NMPC_PLAN_RUN or NMPC_PLAN_RUN_PATH");
    const LaunchPlan p = plan_launch(b, B, mode == NMPC_PLAN_RUN_PATH, mode == NMPC_PLAN_SOLVE ? kModeSolve : kModeRun);
    if (iteration) *iteration = p.handoff;
    if (segments) *segments = p.handoff ? p.seg : 0;
    if (lds_bytes) *lds_bytes = p.handoff ? p.ho_lds : 0;
    return NMPC_OK;
}

int nmpc_batch_plan(const nmpc_batch* b, int B, int* kernel, int* waves_per_robot, int* segments)
{
    nmpc_launch_plan p;
    const int rc = nmpc_batch_plan_ex(b, B, NMPC_PLAN_SOLVE, &p);
    if (rc) return rc;
    if (kernel) *kernel = p.kernel;
    if (waves_per_robot) *waves_per_robot = p.waves_per_robot;
    if (segments) *segments = p.segments;
    return NMPC_OK;
}

int nmpc_batch_warm_rule(const nmpc_batch* b, int* warm, int* warm_iter_max, int* iter_max)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (warm) *warm = b->kp.warm ? 1 : 0;
    if (warm_iter_max) *warm_iter_max = b->kp.warm_iter_max;
    if (iter_max) *iter_max = b->kp.iter_max;
    return NMPC_OK;
}

int nmpc_batch_warm_state(nmpc_batch* b, unsigned char** warm, float** scratch, size_t* scratch_bytes)
{
    if (!b) return set_err(NMPC_ERR_ARG, "batch is NULL");
    if (warm) *warm = b->warm;
    if (scratch) *scratch = b->scratch;
    if (scratch_bytes) *scratch_bytes = sizeof(float) * scratch_floats(b->prm.model, b->prm.N, b->capacity);
    return NMPC_OK;
}

namespace {
int fleet_sim(nmpc_batch* b, int B, float* path, float* s, float* pose, float* vel, float* steer, const float* u0,
              const int* status, float* traj, int* traj_len, int advance, const nmpc_fleet_renew* renew, void* stream)
{
    const TraceRange trace("nmpc_fleet_sim_step");
    if (const int rc = check_batch(b, B)) return rc;
    if (!path || !s || !pose || !vel || !traj || (advance && !u0)) return set_err(NMPC_ERR_ARG, "NULL argument");
    const hipError_t e = with_model(b->prm.model, [&](auto m) {
        return launch_fleet_sim<decltype(m)>(b->kp, B, b->capacity, path, s, pose, vel, steer, u0, status, b->carried,
                                             traj, traj_len, advance, renew, b->rmodel.view(), (hipStream_t)stream);
    });
    return hip_err(e, "fleet_sim launch");
}
}  // namespace

int nmpc_fleet_sim_step(nmpc_batch* b, int B, const float* path, float* s, float* pose, float* vel, float* steer,
                        const float* u0, const int* status, float* traj, int* traj_len, int advance, void* stream)
{
    // without a renewal record the kernel never writes `path`
    return fleet_sim(b, B, const_cast<float*>(path), s, pose, vel, steer, u0, status, traj, traj_len, advance,
                     nullptr, stream);
}

int nmpc_fleet_sim_step_renew(nmpc_batch* b, int B, float* path, float* s, float* pose, float* vel, float* steer,
                              const float* u0, const int* status, float* traj, int* traj_len,
                              const nmpc_fleet_renew* renew, void* stream)
{
    if (!renew || !renew->ev || !renew->ttl || !renew->reset) return set_err(NMPC_ERR_ARG, "renew: NULL argument");
    if (renew->ttl_min < 1 || renew->ttl_max < renew->ttl_min) return set_err(NMPC_ERR_ARG, "renew: ttl range");
    if (const nmpc_fleet_stats* st = renew->stats)
        if (!st->qp_iter || !st->iters_sum || !st->iters_max || !st->fail_cnt || !st->hist || !st->cold_cnt ||
            !st->cold_iters || !status)
            return set_err(NMPC_ERR_ARG, "renew: stats needs every pointer and status");
    return fleet_sim(b, B, path, s, pose, vel, steer, u0, status, traj, traj_len, 1, renew, stream);
}

int nmpc_path_discretize(int B, const nmpc_path_segment* segs, int seg_stride, const int* nseg,
                         const double* nearest_u, double sample_period, int num_poses, int is_holonomic,
                         float* traj, double* traj64, void* stream)
{
    if (B < 0) return set_err(NMPC_ERR_ARG, "B < 0");
    if (B == 0) return NMPC_OK;
    if (!segs || !nseg || !nearest_u) return set_err(NMPC_ERR_ARG, "segs, nseg and nearest_u are required");
    if (seg_stride < 1) return set_err(NMPC_ERR_ARG, "seg_stride < 1");
    if (num_poses < 1 || num_poses > 8192) return set_err(NMPC_ERR_ARG, "num_poses out of range [1, 8192]");
    if (!(sample_period >= 0.0)) return set_err(NMPC_ERR_ARG, "sample_period must be >= 0");
    return hip_err(launch_path_discretize(B, segs, seg_stride, nseg, nearest_u, sample_period, num_poses,
                                          is_holonomic ? 1 : 0, traj, traj64, (hipStream_t)stream),
                   "path_discretize launch");
}

int nmpc_path_nearest(int B, const nmpc_path_segment* segs, int seg_stride, const int* nseg, const float* pose,
                      const double* u_range, int holonomic_heading, double* nearest_u, double* near, double* err,
                      void* stream)
{
    const TraceRange trace("nmpc_path_nearest");
    if (B < 0) return set_err(NMPC_ERR_ARG, "B < 0");
    if (B == 0) return NMPC_OK;
    if (!segs || !nseg || !pose) return set_err(NMPC_ERR_ARG, "segs, nseg and pose are required");
    if (!nearest_u) return set_err(NMPC_ERR_ARG, "nearest_u is required");
    if (seg_stride < 1) return set_err(NMPC_ERR_ARG, "seg_stride < 1");
    return hip_err(launch_path_nearest(B, segs, seg_stride, nseg, pose, nullptr, 0, u_range,
                                       u_range ? u_range + B : nullptr, holonomic_heading ? 1 : 0, nearest_u, near, err,
                                       (hipStream_t)stream),
                   "path_nearest launch");
}

}  // extern "C"
