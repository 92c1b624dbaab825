// sqp_steps.hpp -- the rules of one SQP-RTI tick that do not depend on the thread mapping, stated once for
// k_sqp_rti_team (sqp_rti_team.hip: one 16-lane team per robot) and k_sqp_rti_rowpar (sqp_rti_rowpar.hip: one block
// per robot). team_common.hpp holds the arithmetic blocks; this file holds what a tick does with them. What stays in
// the kernels is the mapping: which lane stores, which buffer is in flight, pads and dummy targets, barriers and LDS
// counters. In both kernels lane r of a DPP row owns QP variable r of a stage.
//
//   step                                   team kernel                         row-parallel kernel
//   lane_ctx         roles, weights, bounds  prologue                            prologue
//   robot_vals       model parameters        prologue                            prologue
//   load_x0          x0, x0_lane, we_lane    prologue                            prologue
//   const_rows       gcol, grow              before P0's stage loop              after P0a's rounds
//   stage_column, stage_dyn                  C1 (column), F0 / F1 (dyn)          phases B, C and the adjoint
//   StageLds         stage inputs in LDS     split launch: P0 part 1 and 2       P0a, P0b, P0c
//   p0_stage_inputs  zbar, b_k, GV rows      split launch: P0 part 1             P0a `round`
//   RefUnwrap        reference unwrap + pad  p0_body                             P0b `uw`
//   stage_box        the lane's box at k     load_p0 (split launch: beside lds_ld) P0c
//   bound_start      bounds, slacks, lambda  p0_body                             P0c
//   terminal_weight  the terminal hack       p0_body (stage N)                   before P0c
//   sqp_full_step    z += dz, x_0 = x0       epilogue                            epilogue
//   write_outputs    the output block        epilogue (lane 0 of the team)       written out (see there)
//
// Not here:
//   * the IPM stopping rule (DESIGN.md "Stopping rule") stays written out at its three sites (team: after P1;
//     row-parallel: after phase B, and after phase A with the lazy adjoint). As one function taking the stationarity
//     clause as a callable it cost the team kernel 1.0-1.3 % of the metric config's kernel time in two shapes (early
//     returns, and flags with selects), and in the segmented kernel it moved the adjoint's loop and grew the master's
//     fp64 loop (profiles/r06/ab/shared_steps.txt);
//   * the row-parallel kernel's output block is write_outputs' text written out: the call changed the register
//     allocation of its phase B loop;
//   * the team kernel's main P0 pipeline computes zbar and b_k from its three-row rotation (the defect against the
//     next buffer's row), so it does not call p0_stage_inputs.
#pragma once
#include "team_common.hpp"

namespace nmpc {
namespace {

// ---- per-lane roles, weights and bounds -----------------------------------------------------------------------
template <class M>
struct LaneCtx {
    bool lv, is_u, is_x;  // live slot (r < NV), input slot, state slot
    int xi, cx;           // state index (0 on other lanes), index among the bounded states or -1
    bool has_b;           // bounded slot: every input (idxbu = all), states on idxbx
    float w_lane, h_stage;  // this lane's stage weight, and dt times it
    float lo_b, hi_b;       // this lane's box
};
// a: the launch (its per-robot table, KArgs::rparams), inst: the robot. Table on: this lane's three values from the
// robot's column, one load each, here in the prologue (idle lanes read rows of slot 0's kind and drop them). A NaN
// bound makes the lane's weight NaN, so the robot fails alone with status 1, as it does on a NaN input.
// TBL = false compiles the table out (the team kernel's table-off instantiations: even a branch that is never taken
// moved its scalar register allocation and cost the metric config 0.9 %, profiles/r07/ab/robot_params.txt)
template <class M, bool TBL = true>
__device__ __forceinline__ LaneCtx<M> lane_ctx(const KParams& P, const KArgs& a, int inst, int r)
{
    constexpr int NX = M::NX, NU = M::NU;
    LaneCtx<M> c;
    c.lv = r < NX + NU;
    c.is_u = r < NU;
    c.is_x = c.lv && !c.is_u;
    c.xi = c.is_x ? r - NU : 0;
    c.cx = c.is_x ? xcomp<M>(c.xi) : -1;
    c.has_b = c.is_u || c.cx >= 0;
    if (TBL && a.rparams) {
        constexpr RpRows RR = rp_rows(NX, NU, M::NBX, M::NBU);
        const float* const t = a.rparams + inst;
        const size_t C = (size_t)a.sstride;
        const int bj = c.is_u ? r : (c.cx >= 0 ? c.cx : 0);
        const float w = t[(size_t)(RR.off[kRpW] + (c.is_u ? NX + r : c.xi)) * C];
        const float lo = t[(size_t)((c.is_u ? RR.off[kRpLbu] : RR.off[kRpLbx]) + bj) * C];
        const float hi = t[(size_t)((c.is_u ? RR.off[kRpUbu] : RR.off[kRpUbx]) + bj) * C];
        const bool nan_b = c.has_b && (lo != lo || hi != hi);
        c.w_lane = c.lv ? (nan_b ? __builtin_nanf("") : w) : 0.0f;
        c.lo_b = c.has_b ? lo : 0.0f;
        c.hi_b = c.has_b ? hi : 0.0f;
    } else {
        // this lane's stage weight, read once: indexed by the lane, the W entries are vector loads from the kernel
        // arguments, and inside P0's loop each one waited on vmcnt(0), i.e. on the previous stage's record stores
        c.w_lane = c.is_u ? P.W[NX + r] : (c.is_x ? P.W[c.xi] : 0.0f);
        c.lo_b = 0.0f;
        c.hi_b = 0.0f;
#pragma unroll
        for (int q = 0; q < NU; q++)
            if (r == q) { c.lo_b = P.lbu[q]; c.hi_b = P.ubu[q]; }
#pragma unroll
        for (int b = 0; b < M::NBX; b++)
            if (c.cx == b) { c.lo_b = P.lbx[b]; c.hi_b = P.ubx[b]; }
    }
    c.h_stage = P.dt * c.w_lane;
    return c;
}

// ---- the robot's model parameters (nmpc_models.hpp ModelPar): the handle's, or with the model table on
// (KArgs::rmodel) the robot's column, NP loads here in the prologue (robot_vals; the kernels keep the values and hand
// the functors a view of them). Every reader of the model parameters takes that view: P0's RK4 columns, const_rows,
// load_x0's direct kinematics and write_outputs' inverse kinematics. A NaN or a zero in the column makes the robot's
// dynamics NaN: it fails alone with status 1 ----
template <class M>
__device__ __forceinline__ ModelVals robot_vals(const KParams& P, const KArgs& a, int inst)
{
    return model_vals<M>(P, a.rmodel, (size_t)a.sstride, inst);
}

// ---- this lane's box at a stage (the stage table, KArgs::sbounds) ------------------------------------------------
// lo / hi: the lane's pair of stage 0, ks: floats from one stage to the next. An input lane points at its lbu / ubu
// row, a bounded state lane at its lbx / ubx row, every other lane at the robot's first row (a valid dummy, dropped).
// The table decides the addresses here, once; the loads in P0 are unconditional, as load_l's and RefUnwrap's are, for
// their reasons (a load under a lane mask, or a value selected behind a branch, turns the waits of P0's loop into full
// drains). Stage table off and per-robot table on (the team kernel's RP instantiations serve both): the same loads
// read the robot's column of the per-robot table with ks = 0, so that launch keeps one box for every stage.
// FB (the team kernel's model-table instantiations, which serve every combination of the three tables): with both
// bound tables off the loads read a dummy pair and stage_box returns the lane's own box fb = {lo_b, hi_b} by a select.
struct StageBox {
    const float *lo, *hi;
    size_t ks;
    bool use_fb;
    float2 fb;
};
template <class M, bool FB = false>
__device__ __forceinline__ StageBox stage_box_ctx(const KArgs& a, int inst, const LaneCtx<M>& c, int r)
{
    constexpr int NBX = M::NBX, NBU = M::NBU, SR = sb_rows(NBX, NBU);
    const int bj = c.is_u ? r : (c.cx >= 0 ? c.cx : 0);
    StageBox s;
    s.use_fb = false;
    s.fb = make_float2(c.lo_b, c.hi_b);
    if (FB && !a.sbounds && !a.rparams) {
        s.lo = s.hi = a.scratch;  // (a valid address; the value is dropped)
        s.ks = 0;
        s.use_fb = true;
    } else if (a.sbounds) {
        const int lo = (c.is_u ? sb_off(kSbLbu, NBX, NBU) : sb_off(kSbLbx, NBX, NBU)) + bj;
        const int hi = (c.is_u ? sb_off(kSbUbu, NBX, NBU) : sb_off(kSbUbx, NBX, NBU)) + bj;
        s.lo = a.sbounds + sb_at(0, lo, inst, a.sstride, SR);
        s.hi = a.sbounds + sb_at(0, hi, inst, a.sstride, SR);
        s.ks = sb_stage_stride(a.sstride, SR);
    } else {
        constexpr RpRows RR = rp_rows(M::NX, M::NU, NBX, NBU);
        const size_t C = (size_t)a.sstride;
        s.lo = a.rparams + (size_t)((c.is_u ? RR.off[kRpLbu] : RR.off[kRpLbx]) + bj) * C + inst;
        s.hi = a.rparams + (size_t)((c.is_u ? RR.off[kRpUbu] : RR.off[kRpUbx]) + bj) * C + inst;
        s.ks = 0;
    }
    return s;
}
// {lo, hi} of stage k, k clamped to N (the rows past a field's last used stage are allocated and never interpreted).
// FB as in stage_box_ctx: only those instantiations have the select
template <bool FB = false>
__device__ __forceinline__ float2 stage_box(const StageBox& s, int k, int N)
{
    const size_t kk = (size_t)(k <= N ? k : N);
    const float2 v = make_float2(s.lo[kk * s.ks], s.hi[kk * s.ks]);
    if constexpr (FB) return s.use_fb ? s.fb : v;
    else return v;
}
// fmaxf in bound_start would swallow a NaN bound, so a NaN in a bound the QP uses (bd) poisons that stage's gradient
// entry gr: the robot then fails alone with status 1, as lane_ctx's NaN weight makes it
__device__ __forceinline__ float stage_box_poison(float gr, float2 box, bool bd)
{
    return (bd && (box.x != box.x || box.y != box.y)) ? __builtin_nanf("") : gr;
}

// ---- x0 (every lane keeps the full vector) --------------------------------------------------------------------
struct X0Lane {
    float pose_th;  // run mode: the pose's heading, where the reference unwrap starts
    float x0_lane;  // this lane's entry of x0 (state lanes)
    float we_lane;  // terminal weight of this lane's state: the caller's W_e (solve mode), else the robot's table row,
                    // else the constructor W_e
};
// run mode: pose, direct kinematics of the measured velocity, and the carried refs on the bounded states
// (NMPCNavControlDiff.cpp:88-101); solve mode: the caller's x0
template <class M, bool TBL = true>
__device__ __forceinline__ X0Lane load_x0(const KParams& P, const KArgs& a, int mode, int inst, const LaneCtx<M>& c,
                                          const typename M::Par& mp, float (&x0)[M::NX])
{
    constexpr int NX = M::NX;
    const size_t S = (size_t)a.stride, Bn = (size_t)a.B;
    X0Lane o;
    o.pose_th = 0.0f;
    if (mode == kModeRun) {
        const float pose[3] = {a.pose[inst], a.pose[Bn + inst], a.pose[2 * Bn + inst]};
        const float vel[3] = {a.vel[inst], a.vel[Bn + inst], a.vel[2 * Bn + inst]};
        const float steer = a.steer ? a.steer[inst] : 0.0f;
        x0[0] = pose[0];
        x0[1] = pose[1];
        x0[2] = pose[2];
        o.pose_th = pose[2];
        M::direct_kin(vel, steer, mp, x0 + 3);
#pragma unroll
        for (int i = 0; i < M::NBX; i++) x0[M::idxbx(i)] = a.carried[(size_t)i * S + inst];
    } else {
#pragma unroll
        for (int j = 0; j < NX; j++) x0[j] = a.x0[(size_t)j * Bn + inst];
    }
    o.x0_lane = 0.0f;
#pragma unroll
    for (int j = 0; j < NX; j++)
        if (c.xi == j) o.x0_lane = x0[j];
    o.we_lane = 0.0f;
    if (c.is_x) {
        if (mode != kModeRun && a.We) o.we_lane = a.We[(size_t)c.xi * Bn + inst];
        else if (TBL && a.rparams)
            o.we_lane = a.rparams[(size_t)(rp_rows(NX, M::NU, M::NBX, M::NBU).off[kRpWe] + c.xi) * (size_t)a.sstride + inst];
        else o.we_lane = P.We[c.xi];
    }
    return o;
}

// ---- constant rows of [B A] (rows >= NGV) from stage 0's iterate row: lane v holds column v (gcol), lane NU+xi
// holds row xi (grow), so the dynamics products need only NGV row sums ---------------------------------------------
template <class M>
__device__ __forceinline__ void const_rows(const KParams& P, const typename M::Par& mp, const LaneCtx<M>& c, int r,
                                           const float (&xb)[M::NX], const float (&ub)[M::NU], float (&gcol)[M::NX],
                                           float (&grow)[M::NX + M::NU])
{
    constexpr int NX = M::NX, NU = M::NU, NV = NX + NU, NGV = M::NGV;
    float dxn0[NX], g0[NX];
    rk4_column<M>(xb, ub, P, mp, c.lv ? r : NU, dxn0, g0);
#pragma unroll
    for (int i = 0; i < NX; i++) gcol[i] = (c.lv && i >= NGV) ? g0[i] : 0.0f;
    sfor<0, NV>([&](auto vc) {
        constexpr int v = decltype(vc)::value;
        float sv = 0.0f;
#pragma unroll
        for (int i = NGV; i < NX; i++) {
            const float t = bc<v>(gcol[i]);
            if (c.is_x && c.xi == i) sv = t;
        }
        grow[v] = sv;
    });
}

// column v of [B A] at a stage (rows < NGV from the record image rc, field GV on)
template <class M, int GV, int RS>
__device__ __forceinline__ void stage_column(const float (&rc)[RS], const float (&gcol)[M::NX], float (&Gc)[M::NX])
{
    constexpr int NGV = M::NGV;
#pragma unroll
    for (int i = 0; i < M::NX; i++) Gc[i] = (i < NGV) ? rc[GV + (i < NGV ? i : 0)] : gcol[i];
}
// dx_{k+1} (lane NU+i) = sum_v G_k[i][v] dz_v: NGV row sums over the stored columns + the constant rows
template <class M, int GV, int RS>
__device__ __forceinline__ float stage_dyn(const LaneCtx<M>& c, const float (&rc)[RS], float dzv,
                                           const float (&grow)[M::NX + M::NU])
{
    constexpr int NGV = M::NGV;
    float nxt = 0.0f;
#pragma unroll
    for (int i = 0; i < NGV; i++) {
        const float s = row_sum16(c.lv ? rc[GV + i] * dzv : 0.0f);
        if (c.xi == i) nxt = s;
    }
    const float cr = dot_v<M::NX, M::NU>(0.0f, dzv, grow);
    return (c.xi >= NGV) ? cr : nxt;
}

// ---- a stage's P0 inputs in LDS: [k][field][lane], SF fields of 16 lanes. at(k, r) is lane r's entry of field 0 of
// stage k; field F of it is at + F (the names are float offsets), Jacobian row i at + gv(i) -----------------------
template <class M>
struct StageLds {
    static constexpr int SF = 5 + M::NGV;
    static constexpr int ZBAR = 0, YREF = 16, LL = 32, LU = 48, DEFECT = 64;  // iterate entry, yref entry (solve
    // mode), warm multipliers, defect b_k = (xbar_{k,i} - xbar_{k+1,i}) + dxn_i
    static constexpr int gv(int i) { return (5 + i) * 16; }                   // the NGV varying Jacobian rows
    __device__ static size_t at(int k, int r) { return (size_t)k * SF * 16 + r; }
};

// this lane's iterate entry zbar, its defect b_k and its column of the stage's Jacobian (RK4 + sensitivities) from
// the stage's iterate row (x, u) and this lane's entry xnext of the next stage's state; stages k >= N: no dynamics
template <class M>
struct P0In {
    float zb, bk, g[M::NX];
};
template <class M>
__device__ __forceinline__ P0In<M> p0_stage_inputs(const KParams& P, const typename M::Par& mp, const LaneCtx<M>& c,
                                                   int r, int k, int N, const float (&x)[M::NX],
                                                   const float (&u)[M::NU], float xnext)
{
    constexpr int NX = M::NX, NU = M::NU;
    P0In<M> o;
    float dxn[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) { dxn[i] = 0.0f; o.g[i] = 0.0f; }
    o.bk = 0.0f;
    if (k < N) {
        rk4_column<M>(x, u, P, mp, c.lv ? r : NU, dxn, o.g);
        // (x - xnext first: both are stored iterate entries a stage apart, so the difference is exact at any
        // distance from the map origin, and only then the step's increment)
#pragma unroll
        for (int i = 0; i < NX; i++)
            if (c.is_x && c.xi == i) o.bk = (x[i] - xnext) + dxn[i];
    }
    o.zb = 0.0f;
#pragma unroll
    for (int j = 0; j < NU; j++)
        if (r == j) o.zb = u[j];
#pragma unroll
    for (int j = 0; j < NX; j++)
        if (c.is_x && c.xi == j) o.zb = x[j];
    return o;
}

// ---- run mode's stage reference: unwrap the heading against the previous reference and pad past the trajectory's
// end with the last pose (NMPCNavControlDiff.cpp:104-118); starts at the robot's heading --------------------------
struct RefUnwrap {
    float ref_x, ref_y, ref_t;
    __device__ __forceinline__ explicit RefUnwrap(float pose_th) : ref_x(0.0f), ref_y(0.0f), ref_t(pose_th) {}
    // in: the stage is inside the trajectory (k < len); pose: its reference pose
    // branch-free (selects): a divergent branch here (len is per robot) made the compiler's waits at its join drain
    // the whole memory counter, the stage's record stores included
    __device__ __forceinline__ void step(bool in, const float (&pose)[3])
    {
        const float th = pose[2], d = th - ref_t;
        const float thu = (d > kPi) ? th - 2.0f * kPi : ((d < -kPi) ? th + 2.0f * kPi : th);
        ref_x = in ? pose[0] : ref_x;
        ref_y = in ? pose[1] : ref_y;
        ref_t = in ? thu : ref_t;
    }
};

// ---- bounds, slacks and multipliers of the initial point ------------------------------------------------------
struct BoundStart {
    float lb, ub, tl, tu, ll, lu;
    float c0;  // the slot's complementarity ll tl + lu tu (0 without a bound)
};
// zbar: the iterate entry, z: the initial step entry, [lo_b, hi_b]: the lane's box, lp: the previous multipliers
// (read under warm only), bd: the slot has a bound at this stage.
// Slots without a bound (or outside their stage range) get a sentinel bound at +-kFar with slack kFar and zero
// multipliers: every bounded-variable expression of the sweeps then vanishes on them (r = 0, Sigma = 0, no step
// bound), so the sweeps need no per-lane branches
__device__ __forceinline__ BoundStart bound_start(const KParams& P, float zbar, float z, float lo_b, float hi_b,
                                                  bool warm, float2 lp, bool bd)
{
    const float lb = lo_b - zbar, ubd = hi_b - zbar;
    const float tl = fmaxf(z - lb, P.thr0), tu = fmaxf(ubd - z, P.thr0);
    // cold: t lambda = mu0; warm: the previous multipliers, floored at kappa / t
    // (previous multipliers capped at kWarmLambdaCap: a feasible QP of this OCP ends with multipliers of the size of
    // its weights, < 1e2; a runaway value from a struggling solve would start the IPM at a huge complementarity)
    // (one division per slack: with one per branch of the warm flag, a per-robot value, the compiler split the lanes
    // around two division sequences)
    const float num = warm ? P.warm_kappa : P.mu0;
    const float ql = num / tl, qu = num / tu;
    const float ll0 = warm ? fmaxf(fminf(lp.x, kWarmLambdaCap), ql) : ql;
    const float lu0 = warm ? fmaxf(fminf(lp.y, kWarmLambdaCap), qu) : qu;
    BoundStart o;
    o.lb = bd ? lb : -kFar;
    o.ub = bd ? ubd : kFar;
    o.tl = bd ? tl : kFar;
    o.tu = bd ? tu : kFar;
    o.ll = bd ? ll0 : 0.0f;
    o.lu = bd ? lu0 : 0.0f;
    // (the products outside the select: with them inside it the compiler computed them under the lane mask, and the
    // waits of the team kernel's P0 loop became full drains: vmcnt(5) (14) (2) (2) -> 31 waits, three of them vmcnt(0))
    const float c0 = ll0 * tl + lu0 * tu;
    o.c0 = bd ? c0 : 0.0f;
    return o;
}

// ---- the terminal-weight hack (NMPCNavControlDiff.cpp:127-139): the pose states' terminal weight is the stage
// weight, times 100 when the last two stage references are equal (same: ref_N == ref_{N-1}); other lanes keep theirs
template <class M>
__device__ __forceinline__ float terminal_weight(const LaneCtx<M>& c, float we_lane, bool same)
{
    const float wh = (same ? 100.0f : 1.0f) * c.w_lane;
    return (c.is_x && c.xi < 3) ? wh : we_lane;
}

// ---- full SQP step: every entry of the iterate += its z, the first state = x0 --------------------------------
// entry(k): this lane's entry of stage k's iterate row (clamped: stages past N repeat stage N's, read-only), or a
// dummy for lanes without one; z_at(kk): its z of stage kk <= N.
// One unconditional load of z and of the iterate entry, one store per lane and stage (lanes without an entry -- idle
// slots, u at stage N -- read and write the dummy record): under lane masks every wait in this loop was a vmcnt(0),
// one memory round trip per stage
template <class E, class Z>
__device__ __forceinline__ void sqp_full_step(int N, bool is_x, float x0_lane, E&& entry, Z&& z_at)
{
    constexpr int EC = 8;  // stages per batch: EC loads of each kind in flight, then EC stores
    for (int k0 = 0; k0 <= N; k0 += EC) {
        float zs[EC], vs[EC];
#pragma unroll
        for (int j = 0; j < EC; j++) {
            const int kk = (k0 + j) <= N ? k0 + j : N;
            zs[j] = z_at(kk);
            vs[j] = *entry(k0 + j);
        }
#pragma unroll
        for (int j = 0; j < EC; j++) {
            const int k = k0 + j;
            const float nv = (is_x && k == 0) ? x0_lane : vs[j] + zs[j];
            if (k <= N) *entry(k) = nv;
        }
    }
}

// ---- the robot's outputs (one lane): u0, x1, status, iteration counts, warm tag, exit residuals, and in run mode the
// carried refs and the command ---------------------------------------------------------------------------------
template <class M>
__device__ __forceinline__ void write_outputs(const KParams& P, const KArgs& a, const typename M::Par& mp, int mode,
                                              int inst, int status, int it_done, const float (&exit_res)[3],
                                              const float (&x0)[M::NX])
{
    constexpr int NX = M::NX, NU = M::NU;
    const size_t S = (size_t)a.stride, Bn = (size_t)a.B;
    float u0[NU];
#pragma unroll
    for (int j = 0; j < NU; j++) {
        u0[j] = a.ubar[(size_t)j * S + inst];
        if (a.u0) a.u0[(size_t)j * Bn + inst] = u0[j];
    }
    if (a.x1) {
#pragma unroll
        for (int j = 0; j < NX; j++) a.x1[(size_t)j * Bn + inst] = a.xbar[((size_t)NX + j) * S + inst];
    }
    if (a.status) a.status[inst] = status;
    if (a.qp_iter) a.qp_iter[inst] = it_done;
    if (a.iter_key) a.iter_key[inst] = it_done;
    // warm-start the next solve only from a solve that converged (not from one that ran to qp_iter_max)
    // and only from an easy one (P.warm_iter_max, 12 by default: warm multipliers lengthen the hard QPs)
    if (a.warm)
        a.warm[inst] = (P.warm && status == 0 && it_done < P.iter_max && it_done <= P.warm_iter_max) ? a.warm_tag : 0;
    if (a.qp_res) {
#pragma unroll
        for (int j = 0; j < 3; j++) a.qp_res[(size_t)j * Bn + inst] = exit_res[j];
    }
    if (mode == kModeRun && status == 0) {
        float rr[M::NBX], cmd[3];
#pragma unroll
        for (int i = 0; i < M::NBX; i++) {
            rr[i] = x0[M::idxbx(i)] + u0[i] * P.dt_ctrl;
            a.carried[(size_t)i * S + inst] = rr[i];
        }
        M::inverse_kin(rr, mp, cmd);
        if (a.cmd) {
#pragma unroll
            for (int j = 0; j < 3; j++) a.cmd[(size_t)j * Bn + inst] = cmd[j];
        }
    } else if (mode == kModeRun && a.cmd) {
        // failed solve: the reference throws (processAcadosStatus, NMPCNavControl.cpp:14-23) and the node
        // publishes a stop command (executeNMPC catch -> Status::Error, NMPCNavControlROS.cpp:716-719); the
        // carried refs and the iterate stay as they were
#pragma unroll
        for (int j = 0; j < 3; j++) a.cmd[(size_t)j * Bn + inst] = 0.0f;
    }
}

}  // namespace
}  // namespace nmpc
