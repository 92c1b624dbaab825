// sqp_rti_team_tick.hpp -- the text of one team-kernel SQP-RTI tick: the body of k_sqp_rti_team (sqp_rti_team.hip) and
// of k_sqp_rti_team_ho (sqp_rti_team_ho.hip), which include it with M, MS, SD, MODE, SP, RP, MT, HO, P and a in scope.
// Not a header in its own right: no include guard, nothing at namespace scope.
    constexpr int mode = MODE == kModeRunPath ? kModeRun : MODE;
    using R = TeamRec<M, SD>;
    constexpr int NX = M::NX, NU = M::NU, NV = R::NV, NGV = R::NGV, RS = R::RS, RSS = R::RSS;
    constexpr bool QM = rec_quad_major<NV>();
    constexpr int KS = 16 * RSS;  // floats per stage block (16 slots of RSS stored floats)
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    // split launches (a.split: small batches on an otherwise idle chip): one 256-lane block per robot. Row 0 of
    // the block is the robot's team; rows 1-15 share the stage-parallel part of P0 with it and leave.
    const int team = a.split ? (int)blockIdx.x : (gt >> 4);
    const int row = a.split ? (int)(threadIdx.x >> 4) : 0;
    const int r = gt & 15;
    if (team >= a.B) return;  // whole DPP rows leave together
    // node ticks: the robots that solve fill the first *n_active slots of the order; the other slots leave
    if (a.n_active && team >= *a.n_active) return;
    const int N = P.N;
    const size_t S = (size_t)a.stride;  // resident state stride (capacity)
    const size_t Bn = (size_t)a.B;
    const int inst = a.order ? a.order[team] : team;  // difficulty-ordered placement (schedule.hip)
    // this lane's roles, stage weight and box (sqp_steps.hpp)
    const LaneCtx<M> lc = lane_ctx<M, RP>(P, a, inst, r);
    const bool lv = lc.lv, is_u = lc.is_u, is_x = lc.is_x, has_b = lc.has_b;
    const int xi = lc.xi, cx = lc.cx;
    const float sc = P.dt, w_lane = lc.w_lane, h_stage = lc.h_stage, lo_b = lc.lo_b, hi_b = lc.hi_b;
    // RP: where P0 loads this lane's box of a stage from (the stage table, else the per-robot table's one box)
    StageBox sbx{};
    if constexpr (RP) sbx = stage_box_ctx<M, MT>(a, inst, lc, r);
    // the robot's model parameters: the handle's (a view of KParams::p), or (MT) its column of the model table
    ModelVals mvals{};
    if constexpr (MT) mvals = robot_vals<M>(P, a, inst);
    const ModelPar mp = MT ? model_par(P, mvals) : model_par(P);
    // this lane's record of stage k: tbase + k * KS
    // idle slots (r >= NV) alias slot 0's record: their (unpredicated) loads then read valid data and touch no
    // extra cache lines; they never store
    // the robot's records (indexed by the robot, not the team slot, so that they carry its multipliers to its next
    // solve whatever the placement)
    float* const tbase = a.scratch + (size_t)inst * (N + 1) * KS + (lv ? r : 0) * rec_lane<RSS, QM>();
    // every lane's own slot (idle lanes: one nobody reads), for P0's unconditional record stores
    float* const tbase_own = a.scratch + (size_t)inst * (N + 1) * KS + r * rec_lane<RSS, QM>();
    // a record nobody reads (slot 15 of the robot's stage-N block: the idle slot of every model), the target of
    // stores that lanes without work issue unconditionally
    float* const tdummy = a.scratch + (size_t)inst * (N + 1) * KS + (size_t)N * KS + 15 * rec_lane<RSS, QM>();
    // split records (R::SPLIT, TeamRec): this lane's core and bound plane entries of stage 0 (stage k: + k CS,
    // + k kb) in the robot's record region; slots without a bound (and idle slots) read the sentinel pair with
    // stride 0; the dummy pair is tdummy (past the planes)
    constexpr bool SPL = R::SPLIT_OK && SP;  // split record planes (TeamRec::SPLIT, KArgs::rec_split)
    float* const pc0 = a.scratch + (size_t)inst * (N + 1) * KS + (lv ? r : 0) * R::CW;
    float* const pb0 = has_b ? a.scratch + (size_t)inst * (N + 1) * KS + (size_t)(N + 1) * R::CS +
                                   (is_u ? r : NU + (cx >= 0 ? cx : 0)) * R::CW
                             : g_rec_sentinel;
    const int kb = has_b ? R::BS : 0;
    // this lane's DZ in the dense plane after the records: dzbase + k * 16 (every lane its own float)
    float* const dzbase = a.scratch + (size_t)a.sstride * (N + 1) * KS + (size_t)inst * (N + 1) * 16 + r;
    // IPM warm start: the bound multipliers of the robot's previous successful solve are still in its records, in
    // this launch's layout when its tag matches (nmpc_batch.h NMPC_WARM_TAG_*)
    const bool warm = P.warm && a.warm && a.warm[inst] == a.warm_tag && !(a.reset && a.reset[inst]);

#define XB(k, j) a.xbar[((size_t)(k) * NX + (j)) * S + inst]
#define UBAR(k, j) a.ubar[((size_t)(k) * NU + (j)) * S + inst]

    STAMP(0);
    // ---- reset -----------------------------------------------------------------------------------------
    if (a.reset && a.reset[inst]) {
        for (int k = r; k <= N; k += 16)
            for (int j = 0; j < NX; j++) XB(k, j) = 0.0f;
        for (int k = r; k < N; k += 16)
            for (int j = 0; j < NU; j++) UBAR(k, j) = 0.0f;
        __threadfence_block();
    }

    // ---- path-following tick (nmpc_batch_run_path): getNextNPoses in-kernel ------------------------------
    // Lane 0 of the team marches the robot's path (PathDiscretizer.cpp:14-63, path_march.hpp, fp64 without
    // contraction: bit-identical poses to k_path_discretize) and records the path parameter of each pose in the
    // team's LDS slice; the rest is padded with the path end (:58-63). The team's 16 lanes then evaluate the
    // poses 16 at a time (atan2 and all), so no lane waits in a divergent emit. A team's lanes share the wave
    // and LDS accesses of a wave retire in order, so P0 reads the poses from LDS directly afterwards.
    // LDS: path mode and split run launches: [teams][N+1] path parameters, then [teams][N+1][3] float poses
    // (split: one team); split launches then the serial P0 pass's stage inputs
    extern __shared__ double s_path[];
    constexpr bool path = MODE == kModeRunPath;  // (the launcher picks it exactly when a.segs is set)
    const bool traj_lds = path || (a.split && mode == kModeRun);
    const int nslot = a.split ? 1 : 16;
    const int tslot = a.split ? 0 : (int)(threadIdx.x >> 4);
    float* const my_traj = reinterpret_cast<float*>(s_path + nslot * (N + 1)) + (size_t)tslot * (N + 1) * 3;
    float* const s_stg = reinterpret_cast<float*>(s_path) + (traj_lds ? (size_t)nslot * (N + 1) * 5 : 0);
    if (path && row == 0) {
        double* const my_u = s_path + (size_t)tslot * (N + 1);
        const nmpc_path_segment* S = a.segs + (size_t)inst * a.seg_stride;
        const int n = a.nseg[inst];
        if (r == 0) {
            const int cnt = path_march(S, n, a.nearest_u[inst], a.period, N + 1, [&](int j, double su) { my_u[j] = su; });
            for (int j = cnt; j <= N; j++) my_u[j] = (double)n;
        }
        // the robot's frame (nmpc_batch_set_robot_frame): the map poses move into it in fp64, before their one rounding
        const double* const fr = a.origin();
        const double ox = fr ? fr[inst] : 0.0, oy = fr ? fr[(size_t)a.sstride + inst] : 0.0;
        for (int j = r; j <= N; j += 16) {
            double px, py, pt;
            path_pose(S, n, my_u[j], a.holo, &px, &py, &pt);
            const float fx = (float)(px - ox), fy = (float)(py - oy);
            my_traj[j * 3 + 0] = fx;
            my_traj[j * 3 + 1] = fy;
            my_traj[j * 3 + 2] = (float)pt;
            if (a.traj_out) {
                a.traj_out[((size_t)j * 3 + 0) * Bn + inst] = fx;
                a.traj_out[((size_t)j * 3 + 1) * Bn + inst] = fy;
                a.traj_out[((size_t)j * 3 + 2) * Bn + inst] = (float)pt;
            }
        }
    }

    // ---- x0 (every lane keeps the full vector) ----------------------------------------------------------
    float x0[NX];
    const X0Lane xl = load_x0<M, RP>(P, a, mode, inst, lc, mp, x0);
    const float pose_th = xl.pose_th, x0_lane = xl.x0_lane;
    float we_lane = xl.we_lane;  // (run mode: + the terminal hack, P0's stage N)

    // ---- P0: linearisation (lane v: nominal step + column v), gradient, bounds, feasible initial iterate --
    // Split launches: the RK4 integrations and every global load of P0 do not depend on each other; only the
    // initial-iterate simulation (and the reference unwrap) is a recursion over the stages. The block's 16 rows
    // (4 waves) take stages row, row + 16, ... and, after a block barrier, leave each lane's stage inputs in LDS
    // (StageLds, sqp_steps.hpp) and run-mode reference poses in row 0's pose slice; row 0 then runs the serial
    // pass from LDS only.
    using SL = StageLds<M>;
    if (a.split) {
        const int len_a = (mode == kModeRun) ? ((a.traj_len && !path) ? a.traj_len[inst] : N + 1) : 0;
        // a stage's global inputs, loaded one stage (of this row) ahead while the current one integrates
        struct In {
            float x[NX], u[NU], y, xnext, tq;
            float2 l;
        };
        auto ld = [&](int k, In& v) {
            const int kk = k <= N ? k : N;
#pragma unroll
            for (int j = 0; j < NX; j++) v.x[j] = XB(kk, j);
            const int ku = kk < N ? kk : N - 1;
#pragma unroll
            for (int j = 0; j < NU; j++) v.u[j] = UBAR(ku, j);
            v.xnext = XB(kk < N ? kk + 1 : N, xi);
            v.y = 0.0f;
            v.tq = 0.0f;
            if (mode != kModeRun) {
                const int j = is_u ? NX + r : xi;
                v.y = (lv && j < a.ny_in) ? a.yref[((size_t)kk * a.ny_in + j) * Bn + inst] : 0.0f;
            } else if (!path && r < 3) {
                const int kt = kk < len_a ? kk : (len_a > 0 ? len_a - 1 : 0);
                v.tq = a.traj[((size_t)kt * 3 + r) * Bn + inst];
            }
            v.l = warm ? *reinterpret_cast<const float2*>(SPL ? pb0 + (size_t)kk * kb + 2
                                                              : tbase + (size_t)kk * KS + rec_off<RS, QM>(R::LL))
                       : make_float2(0.0f, 0.0f);
        };
        In cur, nxt;
        ld(row, cur);
        for (int k = row; k <= N; k += 16) {
            ld(k + 16, nxt);
            if (mode == kModeRun && !path && r < 3) my_traj[k * 3 + r] = cur.tq;
            const P0In<M> in = p0_stage_inputs<M>(P, mp, lc, r, k, N, cur.x, cur.u, cur.xnext);
            float* const st = s_stg + SL::at(k, r);
            st[SL::ZBAR] = in.zb;
            st[SL::YREF] = cur.y;
            st[SL::LL] = cur.l.x;
            st[SL::LU] = cur.l.y;
            st[SL::DEFECT] = in.bk;
#pragma unroll
            for (int i = 0; i < NGV; i++) st[SL::gv(i)] = in.g[i];
            cur = nxt;
        }
        __syncthreads();  // every row's stage inputs are in LDS
        if (row != 0) return;
        STAMPPA();
    }
    const int len = (mode == kModeRun) ? ((a.traj_len && !path) ? a.traj_len[inst] : N + 1) : 0;
    RefUnwrap ref(pose_th);  // the stage reference (run mode), and stage N - 1's for the terminal hack
    float prv_x = 0.0f, prv_y = 0.0f, prv_t = 0.0f;
    // Iterate rows are read two stages ahead (every lane of a team reads the same addresses: one request per
    // wave), the reference row likewise.
    auto load_row = [&](int k, float (&xr)[NX], float (&ur)[NU], float (&tr)[3]) {
        const int kk = k <= N ? k : N;
#pragma unroll
        for (int j = 0; j < NX; j++) xr[j] = XB(kk, j);
        const int ku = kk < N ? kk : N - 1;
#pragma unroll
        for (int j = 0; j < NU; j++) ur[j] = UBAR(ku, j);
        if (mode == kModeRun) {
            const int kt = kk < len ? kk : (len > 0 ? len - 1 : 0);
#pragma unroll
            for (int j = 0; j < 3; j++) tr[j] = path ? my_traj[kt * 3 + j] : a.traj[((size_t)kt * 3 + j) * Bn + inst];
        } else {
            tr[0] = tr[1] = tr[2] = 0.0f;
        }
    };
    float xb[NX], ub[NU], tr[3], xb1[NX], ub1[NU], tr1[3];
    load_row(0, xb, ub, tr);
    load_row(1, xb1, ub1, tr1);
    // constant rows of [B A] (rows >= NGV) from stage 0, before the sweep: lane v holds column v (gcol), lane
    // NU+xi holds row xi (grow), so the initial-iterate dynamics below need only NGV row sums
    float gcol[NX], grow[NV];
    const_rows<M>(P, mp, lc, r, xb, ub, gcol, grow);
    float dx = is_x ? x0_lane - XB(0, xi) : 0.0f;  // this lane's state delta at the current stage
    float sum_c0 = 0.0f;  // complementarity of the initial point (its mean sets the first SD target)
    // warm start: the previous multipliers (LL, LU) of the stage, prefetched one stage ahead
    // (the flag selects the address, not the value: a cold team reads a zero pair. A load whose value is only
    // used under the team's warm flag is issued under that lane mask, and the compiler's waits for every later load
    // of the loop then drain the whole memory counter)
    auto load_l = [&](int k) -> float2 {
        const int kk = k <= N ? k : N;
        const float* const src = warm ? (SPL ? pb0 + (size_t)kk * kb + 2 : tbase + (size_t)kk * KS + rec_off<RS, QM>(R::LL))
                                      : g_zero4;
        return *reinterpret_cast<const float2*>(src);
    };
    // One stage of the serial pass: reference (run mode: unwrap + pad), cost gradient, bounds / slacks /
    // multipliers, the stage record, and the dynamics-feasible initial state of the next stage. Inputs: this
    // lane's iterate entry zbar, its yref entry (solve mode) or the stage's pose ref (run mode), its warm
    // multipliers, the NGV varying Jacobian rows of its column and its defect b_k.
    // RP: this lane's box of the stage, box = {lo, hi} (stage_box, sqp_steps.hpp); else the launch's one box
    auto p0_body = [&](int k, float zbar, float yr_in, const float (&trk)[3], float2 lp, const float (&g)[NX],
                       float bk, float2 box) __attribute__((always_inline)) {
        // stage reference of this lane: run mode unwraps + pads the pose refs (NMPCNavControlDiff.cpp:104-118),
        // entries >= 3 of yref are left at zero
        float yr = yr_in;
        if (mode == kModeRun) {
            ref.step(k < len, trk);
            if (k == N - 1) { prv_x = ref.ref_x; prv_y = ref.ref_y; prv_t = ref.ref_t; }
            // (one select per value: the nested conditional compiled to lane-mask branches)
            float v = 0.0f;
            v = (is_x && xi == 2) ? ref.ref_t : v;
            v = (is_x && xi == 1) ? ref.ref_y : v;
            v = (is_x && xi == 0) ? ref.ref_x : v;
            yr = v;
        }
        float rec[RS];
#pragma unroll
        for (int f = 0; f < RS; f++) rec[f] = 0.0f;
        const bool vu = is_u && k < N, vx = is_x && k >= 1;
        const bool valid = vu || vx;
        // gradient of the Gauss-Newton cost (stage weights scaled by dt, terminal weight unscaled). Every per-lane
        // condition of this body is a select: as lane-mask branches they cost P0 about 14 branch regions per stage
        float w = sc * w_lane;
        if (k == N) {  // (k is wave-uniform)
            if (mode == kModeRun && P.terminal_hack)
                we_lane = terminal_weight(lc, we_lane, ref.ref_x == prv_x && ref.ref_y == prv_y && ref.ref_t == prv_t);
            w = vx ? we_lane : w;
        }
        rec[R::GR] = valid ? w * (zbar - yr) : 0.0f;
        if constexpr (RP) rec[R::GR] = stage_box_poison(rec[R::GR], box, valid && has_b);
        // iterate, bounds, slacks, multipliers
        const float z = vx ? dx : 0.0f;
        rec[R::Z] = z;
        // (sentinels on the slots without a bound, or outside their stage range: bound_start, sqp_steps.hpp)
        {
            const BoundStart b = bound_start(P, zbar, z, RP ? box.x : lo_b, RP ? box.y : hi_b, warm, lp, valid && has_b);
            rec[R::LB] = b.lb;
            rec[R::UB] = b.ub;
            rec[R::TL] = b.tl;
            rec[R::TU] = b.tu;
            rec[R::LL] = b.ll;
            rec[R::LU] = b.lu;
            sum_c0 += b.c0;
        }
#pragma unroll
        for (int i = 0; i < NGV; i++) rec[R::GV + i] = (k < N && lv) ? g[i] : 0.0f;
        // 15-slot teams (omni4): unconditional (the idle lane stores zeros / sentinels into its own unused
        // slot). A store under a lane mask may or may not be issued, so the compiler's waits for the next loads
        // drain the whole memory counter, these stores included. Same-box A/B: omni4 kernel 1.303 -> 1.256 ms;
        // diff (7 idle lanes, +78 % P0 store bytes) 1.043 -> 1.065 ms, so 9-slot teams do not store per idle lane
        // (profiles/r02/ab/uncond_stores.txt)
        if constexpr (NV > 12) rec_store_range<0, RSS, RS, QM>(tbase_own + (size_t)k * KS, rec);
        // 9-slot teams: the idle lanes all store into the team's dummy record (one record's bytes, not seven)
        else if constexpr (SPL)
            split_store<R, 0, R::GR + 1, RS>(lv ? pc0 + (size_t)k * R::CS : tdummy,
                                             (lv && has_b) ? pb0 + (size_t)k * kb : tdummy + R::CW, rec);
        else rec_store_range<0, RSS, RS, QM>(lv ? tbase + (size_t)k * KS : tdummy, rec);
        dzbase[(size_t)k * 16] = 0.0f;  // P1 of iteration 0 applies a zero step
        // dynamics-feasible initial states: dx_{k+1} = A dx_k + b_k (inputs start at du = 0, dx_0 = x0 - xbar_0);
        // row i of [B A] dz: NGV row sums over the columns + the constant rows held in grow
        if (k < N) {
            const float dzd = is_x ? dx : 0.0f;
            float nxt = dot_v<NX, NU>(0.0f, dzd, grow);
#pragma unroll
            for (int i = 0; i < NGV; i++) {
                const float sr = row_sum16(lv ? g[i] * dzd : 0.0f);
                if (xi == i) nxt = sr;
            }
            dx = is_x ? nxt + bk : 0.0f;
        }
    };
    if (a.split) {
        // split launches: every input from LDS. A loop of its own: merged with the global-load loop below, the
        // LDS values waited on vmcnt(0), i.e. on the previous stage's record stores (about one memory latency
        // per stage). Nothing is in flight past this point but the loop's own stores: the waits the compiler
        // would otherwise place inside the loop for the loads above (len, x0) wait on those stores too.
        __builtin_amdgcn_s_waitcnt(0);
        // the stage inputs are read from LDS one stage ahead (each dependent LDS read costs a round trip of the
        // one wave that runs this pass)
        struct Stg {
            float zb, y, ll, lu, b, g[NGV], t[3];
        };
        auto lds_ld = [&](int k, Stg& o) {
            const int kk = k <= N ? k : N;
            const float* const st = s_stg + SL::at(kk, r);
            o.zb = st[SL::ZBAR];
            o.y = st[SL::YREF];
            o.ll = st[SL::LL];
            o.lu = st[SL::LU];
            o.b = st[SL::DEFECT];
#pragma unroll
            for (int i = 0; i < NGV; i++) o.g[i] = st[SL::gv(i)];
#pragma unroll
            for (int j = 0; j < 3; j++) o.t[j] = (mode == kModeRun) ? my_traj[kk * 3 + j] : 0.0f;
        };
        Stg cur, nxt;
        lds_ld(0, cur);
        // RP: the stage's box from the table, one stage ahead beside the LDS reads (the only global loads of this loop)
        float2 box = make_float2(lo_b, hi_b), box_n = box;
        if constexpr (RP) box = stage_box<MT>(sbx, 0, N);
        for (int k = 0; k <= N; k++) {
            lds_ld(k + 1, nxt);
            if constexpr (RP) box_n = stage_box<MT>(sbx, k + 1, N);
            float g[NX];
#pragma unroll
            for (int i = 0; i < NX; i++) g[i] = (i < NGV && k < N) ? cur.g[i < NGV ? i : 0] : 0.0f;
            p0_body(k, cur.zb, cur.y, cur.t, make_float2(cur.ll, cur.lu), g, cur.b, box);
            cur = nxt;
            box = box_n;
        }
    } else {
        // three row buffers used in turn (the loop unrolled by 3, compile-time buffer indices): buffer i holds stage
        // k + i while the loop is at stage k and is refilled with stage k + 3 after its body. A rotation by copies
        // (xb = xb1; xb1 = xb2) copied registers whose loads were still in flight, and each copy waited for every
        // memory operation issued before it (a full drain per stage)
        struct Row {
            float xb[NX], ub[NU], tr[3], yr;
            float2 lp, bx;  // bx (RP): the lane's box of the stage
        };
        auto load_p0 = [&](int k, Row& o) {
            load_row(k, o.xb, o.ub, o.tr);
            o.lp = load_l(k);
            if constexpr (RP) o.bx = stage_box<MT>(sbx, k, N);
            o.yr = 0.0f;
            if (mode != kModeRun) {  // (unconditional load of a valid entry, then a select)
                const int kk = k <= N ? k : N;
                const int j = is_u ? NX + r : xi;
                const bool use = lv && j < a.ny_in;
                const float v = a.yref[((size_t)kk * a.ny_in + (use ? j : 0)) * Bn + inst];
                o.yr = use ? v : 0.0f;
            }
        };
        Row rw[3];
#pragma unroll
        for (int j = 0; j < NX; j++) { rw[0].xb[j] = xb[j]; rw[1].xb[j] = xb1[j]; }
#pragma unroll
        for (int j = 0; j < NU; j++) { rw[0].ub[j] = ub[j]; rw[1].ub[j] = ub1[j]; }
#pragma unroll
        for (int j = 0; j < 3; j++) { rw[0].tr[j] = tr[j]; rw[1].tr[j] = tr1[j]; }
        rw[0].lp = load_l(0);
        rw[1].lp = load_l(1);
        if constexpr (RP) {
            rw[0].bx = stage_box<MT>(sbx, 0, N);
            rw[1].bx = stage_box<MT>(sbx, 1, N);
        }
        rw[0].yr = rw[1].yr = 0.0f;
        if (mode != kModeRun) {
            Row t0, t1;
            load_p0(0, t0);
            load_p0(1, t1);
            rw[0].yr = t0.yr;
            rw[1].yr = t1.yr;
        }
        for (int k0 = 0;; k0 += 3) {
            bool stop = false;
            sfor<0, 3>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if (stop) return;
                const int k = k0 + i;
                load_p0(k + 2, rw[(i + 2) % 3]);  // two stages ahead (clamped)
                const Row& c = rw[i];
                const Row& n1 = rw[(i + 1) % 3];
                float dxn[NX], g[NX];
#pragma unroll
                for (int q = 0; q < NX; q++) { dxn[q] = 0.0f; g[q] = 0.0f; }
                if (k < N) rk4_column<M>(c.xb, c.ub, P, mp, lv ? r : NU, dxn, g);
                float zbar = 0.0f;
#pragma unroll
                for (int j = 0; j < NU; j++)
                    if (r == j) zbar = c.ub[j];
#pragma unroll
                for (int j = 0; j < NX; j++)
                    if (is_x && xi == j) zbar = c.xb[j];
                float bk = 0.0f;
#pragma unroll
                for (int q = 0; q < NX; q++)
                    if (xi == q) bk = (c.xb[q] - n1.xb[q]) + dxn[q];  // (p0_stage_inputs' order)
                p0_body(k, zbar, c.yr, c.tr, c.lp, g, bk, RP ? c.bx : make_float2(lo_b, hi_b));
                if (k == N) stop = true;
            });
            if (stop) break;
        }
    }
    // e_r: places the diagonal D of M = D + G'PG with one multiply per entry instead of two selects (same-box
    // A/B: diff N=40 B=4096 +0.8 %, B=1024 +1.2 %, tric +0.6 %; profiles/r02/ab/onehot.txt)
    double onehot[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) onehot[j] = (r == j) ? 1.0 : 0.0;
    double gcol64[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) gcol64[i] = (double)gcol[i];
#ifdef NMPC_MROW
    constexpr bool kMcol = false;  // checker build (lib/mrow): the row form for every model
#else
    constexpr bool kMcol = M::kMcolForm;  // per model (nmpc_models.hpp)
#endif
    GConst<M> gcs;  // the constant rows of [B A] as uniform operands of the column-form M block (m_block)
    if constexpr (kMcol && !MT) gconst_load<M>(gcs, gcol);

    STAMP(1);
    // infeasibility threshold of this robot: qp_infeas_lambda scaled by its largest weight (terminal hack included)
    // (the robot's own largest stage weight when the per-robot table is on)
    const float wmax = (RP && a.rparams) ? row_max16(w_lane) : P.wmax;
    const float lam_thr = P.infeas_lam * fmaxf(1.0f, fmaxf(wmax, row_max16(is_x ? we_lane : 0.0f)) * 0.1f);
    const int m = N * NU + N * M::NBX;
    const float inv_m2 = 0.5f / (float)m;
    sum_c0 = row_sum16(lv ? sum_c0 : 0.0f);

    // Stage sweeps k = k0, k0 + dir, ..., k1 with the next stage's record (sweep2: the next two) in flight while
    // body(k, rec) runs. The loop is unrolled by the number of register buffers, which are used in turn (no
    // copies between them), and the loads are never predicated: a conditional load or a buffer copy would make
    // the compiler move the in-flight registers, which waits for the load. Lanes that do not sweep (idle slots,
    // converged teams) re-read one fixed record instead; past k1 the pointer stays on k1.
    // P1's loads of one stage: its record fields and (DZ plane) the lane's DZ; dz points at the plane entry of
    // the stage whose record p points at (p - tbase = k KS <=> dz - dzbase = 16 k)
    auto p1_load = [&](int kk, float (&v)[RS]) {
        if constexpr (SPL) split_load<R, R::P1L0, R::P1L1, RS>(pc0 + (size_t)kk * R::CS, pb0 + (size_t)kk * kb, v);
        else rec_load_range<R::P1L0, R::P1L1, RS, QM>(tbase + (size_t)kk * KS, v);
        v[R::DZ] = dzbase[(size_t)kk * 16];
    };
    auto sweep = [&](int k0, int k1, int dir, bool ld, auto&& body) {  // 2 buffers (compute-heavy P1)
        const int sd = ld ? dir : 0;  // stage step of this lane's loads (0: a lane that does not sweep)
        int kp = k0;
        float ra[RS], rb[RS];
        p1_load(kp, ra);
        for (int k = k0;; k += 2 * dir) {
            const int kp1 = (k == k1) ? kp : kp + sd;
            p1_load(kp1, rb);
            body(k, ra);
            if (k == k1) break;
            const int kp2 = (k + dir == k1) ? kp1 : kp1 + sd;
            p1_load(kp2, ra);
            body(k + dir, rb);
            if (k + dir == k1) break;
            kp = kp2;
        }
    };
    // D buffers: buf[i] holds stage k + i*dir while the loop is at k; after body(k + i*dir) it is refilled with
    // stage k + (i + D)*dir (clamped at k1), so D - 1 records are in flight during every body
    auto sweepd = [&](auto dc, auto f0c, auto fc, int k0, int k1, int dir, bool ld, auto&& body) {
        constexpr int D = decltype(dc)::value;
        constexpr int F0 = decltype(f0c)::value, F = decltype(fc)::value;  // floats [F0, F) this sweep reads
        const int sd = ld ? dir : 0;
        float buf[D][RS];
        int kp = k0;
        int kl = k0;
        // P1 with P1_D > 2 buffers also takes DZ from the plane (the light sweeps read only the prefix)
        auto load = [&](int kk, float (&v)[RS]) {
            if constexpr (SPL) split_load<R, F0, F, RS>(pc0 + (size_t)kk * R::CS, pb0 + (size_t)kk * kb, v);
            else rec_load_range<F0, F, RS, QM>(tbase + (size_t)kk * KS, v);
            if constexpr (F == R::P1L1) v[R::DZ] = dzbase[(size_t)kk * 16];
        };
        load(kp, buf[0]);
        sfor<1, D>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            kp = (kl == k1) ? kp : kp + sd;
            kl = (kl == k1) ? kl : kl + dir;
            load(kp, buf[i]);
        });
        for (int k = k0;; k += D * dir) {
            bool stop = false;
            sfor<0, D>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if (stop) return;
                body(k + i * dir, buf[i]);
                if (k + i * dir == k1) {
                    stop = true;
                    return;
                }
                kp = (kl == k1) ? kp : kp + sd;
                kl = (kl == k1) ? kl : kl + dir;
                load(kp, buf[i]);
            });
            if (stop) break;
        }
    };
    // ---- interior-point iterations ----------------------------------------------------------------------
    int status = 0, it_done = 0;
    bool done = false;
    float exit_res[3] = {0.0f, 0.0f, 0.0f};
    float alpha = 0.0f, sigma_mu = 0.0f, eta = 0.0f, mu_prev = 3.0e38f;
    // SD: centring target of the next direction, built into P1's rhs. The first direction: sigma = sd_hi (no
    // previous step) and the initial point's mu (P0; mu0 for a cold start, where every pair has t lambda = mu0)
    float tg_rhs = P.sd_hi * sum_c0 * inv_m2;
    for (int it = 0;; it++) {
        // HO: the hand-off iteration (KArgs::handoff = C, below qp_iter_max). The teams of a wave count their
        // iterations together, so every team that has not stopped by the top of iteration C leaves the loop here, by
        // its own count alone
        if constexpr (HO) {
            if (it == a.handoff && it < P.iter_max) break;
        }
        // P1 (backward): apply the previous step, residuals, adjoint, fp64 classic Riccati factorisation,
        // predictor rhs
        double Lrow[NV];  // lane NU+i: row i of P_{k+1} (the state block of the previous stage's M after its pivots)
#pragma unroll
        for (int j = 0; j < NV; j++) Lrow[j] = 0.0;
        float pv = 0.0f, piv = 0.0f;
        float res_stat = 0.0f, res_ineq = 0.0f, sum_c = 0.0f, max_c = 0.0f, stat_scale = 1.0f, nanf_ = 0.0f;
        float lam_max = 0.0f;
        bool fail = false;
        const bool act = lv && !done;
        const float a_upd = (it > 0 && !done) ? alpha : 0.0f;
        // P1_D record buffers: the heavy sweep's next records are in flight for P1_D - 1 stage bodies (at four
        // waves per CU a record load from the Infinity Cache takes about one stage body)
#if P1_D > 2
        sweepd(std::integral_constant<int, P1_D>{}, std::integral_constant<int, R::P1L0>{},
               std::integral_constant<int, R::P1L1>{}, N, 0, -1, act, [&](int k, float (&rc)[RS]) {
#else
        sweep(N, 0, -1, act, [&](int k, float (&rc)[RS]) {
#endif
            STAMPF(0);
            const bool vu = is_u && k < N;
            const bool vx = is_x && k >= 1;
            const bool valid = vu || vx;
            const bool bnd = valid && has_b;
            // Branch-free: slots without a bound hold the kFar sentinel (P0), for which every bounded-variable
            // term below is 0; only the slack / multiplier step is masked (it would move lambda off zero).
            float z = rc[R::Z];
            float tl = rc[R::TL], tu = rc[R::TU], ll = rc[R::LL], lu = rc[R::LU];
            const float lb = rc[R::LB], ubd = rc[R::UB];
            {
                const float dz = rc[R::DZ];
                const float rl = z - lb - tl, rr = ubd - z - tu;
                const float itl = frcp(tl), itu = frcp(tu);
                float tgl = sigma_mu, tgu = sigma_mu;  // SD: the previous direction's target
                if constexpr (!SD) {
                    const BoundDir da = bound_dir(rc[R::DZA], rl, rr, tl, tu, ll, lu, itl, itu, 0.0f, 0.0f);
                    tgl = sigma_mu - eta * da.dll * da.dtl;
                    tgu = sigma_mu - eta * da.dlu * da.dtu;
                }
                const BoundDir d = bound_dir(dz, rl, rr, tl, tu, ll, lu, itl, itu, tgl, tgu);
                const float ab = bnd ? a_upd : 0.0f, av = valid ? a_upd : 0.0f;
                tl += ab * d.dtl;
                tu += ab * d.dtu;
                ll += ab * d.dll;
                lu += ab * d.dlu;
                z += av * dz;
                rc[R::Z] = z;
                rc[R::TL] = tl;
                rc[R::TU] = tu;
                rc[R::LL] = ll;
                rc[R::LU] = lu;
            }
            const float rl = z - lb - tl, rr = ubd - z - tu;
            const float itl = frcp(tl), itu = frcp(tu);
            res_ineq = fmaxf(res_ineq, fmaxf(fabsf(rl), fabsf(rr)));  // NaN: caught by nanf_ (ghat, sig)
            sum_c += ll * tl + lu * tu;
            max_c = fmaxf(max_c, fmaxf(ll * tl, lu * tu));
            lam_max = fmaxf(lam_max, fmaxf(ll, lu));  // 0 on the kFar-sentinel slots
            const float lamdiff = ll - lu;
            const float sig = ll * itl + lu * itu;
            // predictor rhs (zero complementarity target); SD: the centring target tg_rhs (0 on kFar slots)
            const float gh = SD ? ll * rl * itl + ll - lu * rr * itu - lu - tg_rhs * itl + tg_rhs * itu
                                : ll * rl * itl + ll - lu * rr * itu - lu;
            STAMPF(1);
            float Gc[NX];
            stage_column<M, R::GV>(rc, gcol, Gc);
            // adjoint: c_v = sum_l G[l][v] pi_{k+1}[l]
            const float cpi = (k < N) ? dot_x<NX, NU>(0.0f, piv, Gc) : 0.0f;
            const float hz = ((k < N) ? h_stage : we_lane) * z;
            const float g = rc[R::GR];
            const float base = hz + g - lamdiff + cpi;
            rc[R::RU] = base;  // read back for the u slots only
            res_stat = fmaxf(res_stat, vu ? fabsf(base) : 0.0f);
            stat_scale = fmaxf(stat_scale, vu ? fmaxf(fabsf(cpi), fmaxf(fabsf(g), fabsf(lamdiff))) : 0.0f);
            const float ghat = valid ? (vu ? gh + base : gh) : 0.0f;
            const float pi_new = vx ? base : 0.0f;
            if (ghat != ghat || sig != sig) nanf_ = 1.0f;
            if (k == N) {
                // terminal: P_N = diag(W_e + Sigma) on the state lanes
                const double d = is_x ? (double)fmaxf(we_lane + sig, 0.0f) : 0.0;
#pragma unroll
                for (int j = 0; j < NV; j++) Lrow[j] = (is_x && j == r) ? d : 0.0;
                pv = is_x ? ghat : 0.0f;
            } else {
                double Gd[NX];
#pragma unroll
                for (int l = 0; l < NX; l++) Gd[l] = (l < NGV) ? (double)Gc[l] : gcol64[l];
                // classic Riccati in fp64: PG column v = P_{k+1} G[:, v] (P[i][l] sits in lane NU+i at Lrow[NU+l]),
                // row r of M = D + G' P G, then the right-looking row-distributed Cholesky of the input block only:
                // after the NU input pivots the state block of M holds the Schur complement
                // Qxx - Qxu Quu^-1 Qux = P_k, which the state lanes carry to the next stage
                double pg[NX];
#pragma unroll
                for (int i = 0; i < NX; i++) pg[i] = 0.0;
                STAMPF(2);
                pg_block<NX, NU>(pg, Lrow, Gd);
                STAMPF(3);
                const double dg = valid ? (double)h_stage + (double)sig : 1.0;
                double Lr[NV];
#pragma unroll
                for (int j = 0; j < NV; j++) Lr[j] = onehot[j] * dg;
                double pivot;  // = M[0][0]
                bool seq_pivots = true;
                if constexpr (kMcol) {
                    double m11, m10;
                    // column form: 3 broadcast rows + the constant rows as uniform operands, or (model table on) as
                    // broadcasts from the team's own lanes
                    if constexpr (MT) m_block_team<M>(Lr, pivot, m11, m10, pg, Gd);
                    else m_block<M>(Lr, pivot, m11, m10, pg, Gd, gcs);
                    STAMPF(4);
                    if constexpr (NU == 2 && M::kPivotsUpFront) {
                        chol_input_2<NX>(Lr, pivot, m11, m10, r, fail);  // both pivots up front
                        seq_pivots = false;
                    } else {
                        (void)m11;
                        (void)m10;
                    }
                } else {
                    mrow_pg_block<NX, NU>(Lr, pivot, pg, Gd);  // the row form (NX x NV broadcast FMAs)
                    STAMPF(4);
                }
                if (seq_pivots) sfor<0, NU>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    if (!(pivot > 0.0)) fail = true;
                    const double rd = drsq(fmax(pivot, 1e-300));
                    // lane j: Lr[j] == pivot; rows r < j are the upper triangle of the stored input columns (LM)
                    const double lj = (r >= j) ? Lr[j] * rd : 0.0;
                    Lr[j] = lj;
                    chol_update<NX, NU, j>(Lr, lj, pivot);
                });
                STAMPF(5);
                float Lm[NU];
#pragma unroll
                for (int q = 0; q < NU; q++) {
                    Lm[q] = (float)Lr[q];
                    rc[R::LM + q] = Lm[q];
                }
                // rhs: w = g^ + G' p_{k+1}; forward substitution over the input block (fp32)
                float y = dot_x<NX, NU>(ghat, pv, Gc);
                float my_lr = 0.0f;
                sfor<0, NU>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    const float lrj = bc<j>(y * frcp(Lm[j]));  // (y_j / L_jj) from lane j
                    if (r == j) my_lr = lrj;
                    y -= Lm[j] * lrj;
                });
                rc[R::LR] = my_lr;
                pv = is_x ? y : 0.0f;
#pragma unroll
                for (int j = 0; j < NV; j++) Lrow[j] = Lr[j];
            }
            piv = pi_new;
            STAMPF(6);
            // Unconditional stores: lanes without work (idle slots, finished teams) write a record nobody reads.
            // Under a lane mask the stores sit in a branch the wave may skip, and the compiler then placed an
            // s_waitcnt vmcnt(0) at the loop header of the ping-pong sweep (it waited for the stores just issued
            // and for the prefetch); unconditional, every wait in the loop is counted (tools/isa_waits.py)
            float* const pk = act ? tbase + (size_t)k * KS : tdummy;
            if constexpr (SPL) {
                // core quad (LR LM Z) of the sweeping lanes; the bound quad only where a bound lives
                split_store<R, 0, R::TL, RS>(act ? pc0 + (size_t)k * R::CS : tdummy, tdummy + R::CW, rc);
                split_store<R, R::TL, R::TL + 4, RS>(tdummy, (act && bnd) ? pb0 + (size_t)k * kb : tdummy + R::CW, rc);
            } else if constexpr (MS) {
                // slack / multiplier quad only where a bound lives (elsewhere it holds the constant sentinel)
                rec_store_range<R::TL, R::TL + 4, RS, QM>(bnd ? pk : tdummy, rc);
                if constexpr (R::TL > 0) rec_store_range<0, R::TL, RS, QM>(pk, rc);
                if constexpr (R::TL + 4 < R::P1S1) rec_store_range<R::TL + 4, R::P1S1, RS, QM>(pk, rc);
            } else {
                rec_store_range<0, R::P1S1, RS, QM>(pk, rc);
            }
            STAMPF(7);
        });
        if (it < kStampItsC) STAMP(2 + 4 * it);
        // team reductions
        sum_c = row_sum16(lv ? sum_c : 0.0f);
        max_c = row_max16(lv ? max_c : 0.0f);
        lam_max = row_max16(lv ? lam_max : 0.0f);
        res_ineq = row_max16(lv ? res_ineq : 0.0f);
        res_stat = row_max16(lv ? res_stat : 0.0f);
        stat_scale = row_max16(stat_scale);
        nanf_ = row_max16(nanf_);
        const float failf = row_max16(fail ? 1.0f : 0.0f);
        const float mu = sum_c * inv_m2;
        if (!done) {
            exit_res[0] = res_stat;
            exit_res[1] = res_ineq;
            exit_res[2] = mu;
            bool stop = false;
            if (nanf_ > 0.0f || mu != mu) {
                status = 1;
                stop = true;
            } else if (failf > 0.0f) {
                status = (mu <= kBreakdownMuT && res_ineq <= P.tol_ineq * 10.0f) ? 0 : 4;
                stop = true;
            } else if (lam_max > lam_thr && res_ineq > kInfeasRes) {
                status = 4;  // primal infeasible: stop now instead of holding the wave for qp_iter_max iterations
                stop = true;
            } else {
                const bool stat_ok = res_stat <= P.tol_stat || res_stat <= kStatRelT * stat_scale;
                // fp32 floor: below ~1e-12 the complementarity no longer decreases and the fp32 multiplier
                // updates (Sigma ~ 1e10 times the rounding of dz) degrade stationarity, so a stalled mu that is
                // already under tol_comp ends the iteration as well
                const bool cmax_ok = max_c <= kCompMaxRatio * P.tol_comp;
                const bool stalled = mu <= P.tol_comp && mu > 0.5f * mu_prev;
                if (res_ineq <= P.tol_ineq &&
                    ((stat_ok && mu <= P.tol_comp && cmax_ok) || mu <= 1e-2f * P.tol_comp || (stalled && cmax_ok)))
                    stop = true;
                if (it >= P.iter_max) stop = true;
            }
            if (stop) {
                done = true;
                it_done = it;
            }
        }
        mu_prev = mu;
        if (__all(done)) break;

        // pass 0: affine direction (forward; stores DZA, sums s1/s2 of the mu_aff polynomial);
        // pass 1: Mehrotra corrector (backward rhs through the stored factor, then forward; stores DZ);
        // pass 2: pure-centring safeguard for teams whose pass-1 step stayed below 0.1.
        // SD: pass 1 only, without the backward sweep: P1 already built the rhs with the target tg_rhs
        float sigma = 0.0f, alpha_aff = 0.0f;
        for (int pass = SD ? 1 : 0; pass < (SD ? 2 : 3); pass++) {
            bool run = !done;
            if (SD) {
                sigma_mu = tg_rhs;
                eta = 0.0f;
            } else if (pass == 1) {
                sigma_mu = sigma * mu;
                eta = alpha_aff;
            } else if (pass == 2) {
                if (__all(done || alpha >= 0.1f)) break;
                run = run && alpha < 0.1f;
                // only the teams that take the safeguard step change their targets: the next P1 rebuilds the
                // slack / multiplier step of every team from (DZ, DZA, sigma_mu, eta)
                sigma_mu = run ? fmaxf(sigma, 0.3f) * mu : sigma_mu;
                eta = run ? 0.0f : eta;
            }
            const bool ld = lv && run;
            if (!SD && pass > 0) {
                // corrector rhs through the stored factorisation (backward)
                float pvc = 0.0f;
                sweepd(std::integral_constant<int, LIGHT_DC>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, R::NB>{}, N, 0, -1, ld, [&](int k, float (&rc)[RS]) {
                    const bool vu = is_u && k < N;
                    float ghat;
                    {  // branch-free: 0 on the kFar-sentinel slots (see P0)
                        const float z = rc[R::Z];
                        const float tl = rc[R::TL], tu = rc[R::TU], ll = rc[R::LL], lu = rc[R::LU];
                        const float rl = z - rc[R::LB] - tl, rr = rc[R::UB] - z - tu;
                        const float itl = frcp(tl), itu = frcp(tu);
                        const BoundDir da = bound_dir(rc[R::DZA], rl, rr, tl, tu, ll, lu, itl, itu, 0.0f, 0.0f);
                        const float tgl = sigma_mu - eta * da.dll * da.dtl, tgu = sigma_mu - eta * da.dlu * da.dtu;
                        ghat = -(tgl - ll * rl) * itl + ll + (tgu - lu * rr) * itu - lu;
                    }
                    ghat += vu ? rc[R::RU] : 0.0f;
                    if (k == N) {
                        pvc = is_x ? ghat : 0.0f;
                    } else {
                        float Gc[NX];
                        stage_column<M, R::GV>(rc, gcol, Gc);
                        float y = dot_x<NX, NU>(ghat, pvc, Gc);
                        float my_lr = 0.0f;
                        sfor<0, NU>([&](auto jc) {
                            constexpr int j = decltype(jc)::value;
                            const float Lmj = rc[R::LM + j];
                            const float lrj = bc<j>(y * frcp(Lmj));
                            if (r == j) my_lr = lrj;
                            y -= Lmj * lrj;
                        });
                        if (ld && is_u) (SPL ? pc0[(size_t)k * R::CS] : tbase[(size_t)k * KS + rec_off<RS, QM>(R::LR)]) = my_lr;
                        rc[R::LR] = my_lr;
                        pvc = is_x ? y : 0.0f;
                    }
                });
            }
            if (pass == 1) STAMPC1();
            // forward: du from the stored factor, dz, bounded-variable directions, next-stage dx
            float amax = 1e30f, s1 = 0.0f, s2 = 0.0f;
            // body kind 0: affine pass, 1: corrector / safeguard pass, 2: SD direction (target sigma_mu without the
            // affine correction; sums the complementarity polynomial of the step) -- compile-time bodies
            auto fwd = [&](auto cc) {
            constexpr int kind = decltype(cc)::value;
            constexpr bool corr = kind != 0;
            float dxs = 0.0f;
            sweepd(std::integral_constant<int, LIGHT_D>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, R::NF>{}, 0, N, 1, ld, [&](int k, float (&rc)[RS]) {
                const bool vu = is_u && k < N;
                const bool vx = is_x && k >= 1;
                const bool valid = vu || vx;
                // NU = 2: computed at every stage and zeroed at k = N (a select): under `if (k < N)` the compiler
                // sank the first stage's LR / LM load into the branch and waited for it (and every prefetch) at once
                // (same-box: metric +0.4 %, tric +1.1 %; omni4's longer substitution lost 0.6 %, so NU = 4 keeps
                // the branch; profiles/r03/ab/f1_uncond.txt)
                float du_all[NU];
#pragma unroll
                for (int q = 0; q < NU; q++) du_all[q] = 0.0f;
                if (NU == 2 || k < N) {
                    float w[NU];
                    sfor<0, NU>([&](auto qc) {
                        constexpr int q = decltype(qc)::value;
                        w[q] = bc<q>(rc[R::LR]) + ((k > 0) ? row_sum16(is_x ? rc[R::LM + q] * dxs : 0.0f) : 0.0f);
                    });
                    sfor<0, NU>([&](auto qqc) {
                        constexpr int q = NU - 1 - decltype(qqc)::value;
                        float sq = w[q];
                        sfor<q + 1, NU>([&](auto jc) {
                            constexpr int j = decltype(jc)::value;
                            sq -= bc<j>(rc[R::LM + q]) * du_all[j];
                        });
                        du_all[q] = sq * frcp(bc<q>(rc[R::LM + q]));
                    });
#pragma unroll
                    for (int q = 0; q < NU; q++) du_all[q] = (k < N) ? -du_all[q] : 0.0f;
                }
                float dz = 0.0f;
#pragma unroll
                for (int q = 0; q < NU; q++)
                    if (r == q) dz = du_all[q];
                dz = is_x ? ((k >= 1) ? dxs : 0.0f) : dz;
                {  // branch-free: the kFar-sentinel slots bound no step and add nothing to s1, s2
                    const float z = rc[R::Z];
                    const float tl = rc[R::TL], tu = rc[R::TU], ll = rc[R::LL], lu = rc[R::LU];
                    const float rl = z - rc[R::LB] - tl, rr = rc[R::UB] - z - tu;
                    const float itl = frcp(tl), itu = frcp(tu);
                    float tgl = 0.0f, tgu = 0.0f;
                    if (kind == 1) {
                        const BoundDir da = bound_dir(rc[R::DZA], rl, rr, tl, tu, ll, lu, itl, itu, 0.0f, 0.0f);
                        tgl = sigma_mu - eta * da.dll * da.dtl;
                        tgu = sigma_mu - eta * da.dlu * da.dtu;
                    } else if (kind == 2) {
                        tgl = sigma_mu;
                        tgu = sigma_mu;
                    }
                    const BoundDir d = bound_dir(dz, rl, rr, tl, tu, ll, lu, itl, itu, tgl, tgu);
                    amax = step_bound_r(amax, tl, d.dtl);
                    amax = step_bound_r(amax, tu, d.dtu);
                    amax = step_bound_r(amax, ll, d.dll);
                    amax = step_bound_r(amax, lu, d.dlu);
                    if (kind == 0) {  // dll = dlu = 0 on sentinel slots at zero targets
                        s1 += ll * d.dtl + tl * d.dll + lu * d.dtu + tu * d.dlu;
                        s2 += d.dll * d.dtl + d.dlu * d.dtu;
                    } else if (kind == 2) {  // a nonzero target moves the sentinels' multipliers: bounded slots only
                        const bool bnd = valid && has_b;
                        s1 += bnd ? ll * d.dtl + tl * d.dll + lu * d.dtu + tu * d.dlu : 0.0f;
                        s2 += bnd ? d.dll * d.dtl + d.dlu * d.dtu : 0.0f;
                    }
                }
                {  // unconditional (lanes without a direction write the dummy record): a masked store here left
                   // the compiler's wait after the sweep a full drain
                    const bool st = ld && valid;
                    if (corr) *(st ? dzbase + (size_t)k * 16 : tdummy) = dz;
                    else  // (the affine direction; split records are single-direction only and have none)
                        *((st && !SPL) ? tbase + (size_t)k * KS + rec_off<RS, QM>(R::DZA) : tdummy) = dz;
                }
                if (k < N) dxs = stage_dyn<M, R::GV>(lc, rc, valid ? dz : 0.0f, grow);
            });
            };
            // one compiled body per pass kind: same-box A/B diff metric 1.553 -> 1.526 ms, tric 4.382 -> 4.363 ms
            if constexpr (SD) fwd(std::integral_constant<int, 2>{});
            else if (pass == 0) fwd(std::integral_constant<int, 0>{});
            else fwd(std::integral_constant<int, 1>{});
            amax = row_min16(lv ? amax : 1e30f);
            if (SD) {
                // the step, then the next direction's target: mu after the step is exactly the complementarity
                // polynomial (sum_c + a s1 + a^2 s2) / 2m; sigma = clamp((1 - a)^2, sd_lo, sd_hi)
                s1 = row_sum16(lv ? s1 : 0.0f);
                s2 = row_sum16(lv ? s2 : 0.0f);
                if (run) alpha = fminf(1.0f, P.tau * amax);
                const float mu_next = fmaxf((sum_c + alpha * s1 + alpha * alpha * s2) * inv_m2, 0.0f);
                const float om = 1.0f - alpha;
                tg_rhs = fminf(fmaxf(om * om, P.sd_lo), P.sd_hi) * mu_next;
                if (it < kStampItsC) STAMP(4 + 4 * it);
            } else if (pass == 0) {
                s1 = row_sum16(lv ? s1 : 0.0f);
                s2 = row_sum16(lv ? s2 : 0.0f);
                alpha_aff = fminf(1.0f, amax);
                const float mu_aff = (sum_c + alpha_aff * s1 + alpha_aff * alpha_aff * s2) * inv_m2;
                float sg = (mu > 0.0f) ? mu_aff / mu : 0.0f;
                sg = fmaxf(sg, 0.0f);
                sigma = fminf(sg * sg * sg, 1.0f);
                if (it < kStampItsC) STAMP(3 + 4 * it);
            } else {
                if (run) alpha = fminf(1.0f, P.tau * amax);
                if (pass == 1 && it < kStampItsC) STAMP(4 + 4 * it);
            }
        }
        if (it < kStampItsC) STAMP(5 + 4 * it);
    }

    // ---- HO: an unfinished team hands its robot over (HoList, rowpar_layout.hpp): its records, multipliers and DZ plane
    // stay where they are, and the scalars the top of the next iteration needs go to the team's list entry; a wave of
    // the block finishes the solve and writes the outputs (k_sqp_rti_team_ho)
    if constexpr (HO) {
        if (!done) {
            ho_ent[HoList::WE + r] = we_lane;
            if (r == 0) {
                ho_ent[HoList::INST] = __int_as_float(inst);
                ho_ent[HoList::ALPHA] = alpha;
                ho_ent[HoList::SIGMA_MU] = sigma_mu;
                ho_ent[HoList::TG_RHS] = tg_rhs;
                ho_ent[HoList::MU_PREV] = mu_prev;
            }
            ho_pend = true;
            return;
        }
    }
    // ---- full SQP step + outputs ----------------------------------------------------------------------
    if (status == 0) {
        // this lane's entry of stage k (clamped: stages past N repeat stage N's, read-only below)
        // (both candidate addresses computed for every lane, then selected: as a pointer choice per lane class the
        // compiler branched around each address computation, two lane-mask regions per stage)
        auto entry = [&](int k) -> float* {
            const int kk = k <= N ? k : N;
            float* const px = &XB(kk, xi);
            float* const pu = &UBAR(kk < N ? kk : N - 1, is_u ? r : 0);
            return is_x ? px : ((is_u && kk < N) ? pu : tdummy);
        };
        sqp_full_step(N, is_x, x0_lane, entry, [&](int kk) {
            return SPL ? pc0[(size_t)kk * R::CS + R::Z] : tbase[(size_t)kk * KS + rec_off<RS, QM>(R::Z)];
        });
        if (a.xtraj || a.utraj) {
            __threadfence_block();
            for (int k = 0; k <= N; k++) {
                if (is_x && a.xtraj) a.xtraj[((size_t)k * NX + xi) * Bn + inst] = XB(k, xi);
                if (is_u && k < N && a.utraj) a.utraj[((size_t)k * NU + r) * Bn + inst] = UBAR(k, r);
            }
        }
    }
    __threadfence_block();
    if (r == 0) write_outputs<M>(P, a, mp, mode, inst, status, it_done, exit_res, x0);
#undef XB
#undef UBAR
