// rowpar_layout.hpp -- what the kernels that include the row-parallel tick (sqp_rti_rowpar_tick.hpp) share: the record
// view, the LDS layouts and the row reductions. Included by sqp_rti_rowpar.hip and sqp_rti_team_ho.hip.
#pragma once
#include "nmpc_kernels.hpp"
#include "team_common.hpp"
#include "sqp_steps.hpp"

namespace nmpc {

// Record layout: TeamRec<M, true> (the team kernel's single-direction layout: the warm-start multipliers LL / LU
// and the record stride are shared, so a handle may alternate kernels between solves). Global memory keeps what
// outlives an IPM iteration -- the iterate Z, slacks / multipliers TL TU LL LU (phase A), bounds LB UB, Jacobian rows
// GV and gradient GR (P0) -- and the fields an iteration makes and uses up live in LDS (ItLds): SIG (barrier
// weight), C0 (h z + g - (l_lo - l_up), the stationarity term without the adjoint) and GH (the bound part of the
// rhs) from phase A for phase B, LR / LM (the factor's input columns and rhs) from phase B for phase C, DZ (the
// direction) from phase C for phases D and A. SIG / C0 / GH are register-image slots past GR only.
template <class M>
struct RowRec {
    using T = TeamRec<M, true>;
    static constexpr int NX = M::NX, NU = M::NU, NV = NX + NU, NGV = M::NGV;
    static constexpr int LR = T::LR, LM = T::LM, Z = T::Z, TL = T::TL, TU = T::TU, LL = T::LL, LU = T::LU;
    static constexpr int LB = T::LB, UB = T::UB, GV = T::GV, GR = T::GR, RS = T::RS, RSS = T::RSS;
    static constexpr int SIG = GR + 1, C0 = GR + 2, GH = GR + 3;
    static_assert(GH < RS, "phase-A fields fit the register image");
    static_assert(LM + NU <= Z && Z < TL, "LR / LM below Z");
};

// The per-iteration stage fields in LDS (RowRec): [N+1][NF][NV] floats, live slots only (lane r < NV reads / writes
// slot r; idle lanes read slot 0 and write a pad). Round 4 kept them in the global records, which cost about 1.06 KB
// of writes per robot, stage and IPM iteration at diff1024 (phase A's SIG / C0 / GH sector, phase B's LR / LM into
// the sector phase A had just written, the DZ plane): 6.3x the fetched bytes
template <class M>
struct ItLds {
    static constexpr int NU = M::NU, NV = M::NX + M::NU;
    static constexpr int SIG = 0, C0 = 1, GH = 2, LR = 3, LM = 4, DZ = 4 + NU, NF = 5 + NU;
    __host__ __device__ static constexpr size_t floats(int N) { return (size_t)(N + 1) * NF * NV; }
};

// LDS of the segmented phases (SEG, a.seg = S > 0), in floats from its base (8-byte aligned; fp64 parts at even
// offsets). Per segment q: the entry quantities of its backward sweep -- P (fp64 rows), pbar, Phi, Gam, t; per master step i: Q_i (fp64), c_i, phat_{i+1}; a transpose scratch; the
// boundary states s_q and
// costates lam_q; the lam-sensitivity Z of every stage's LR (rows of the NU input lanes).
template <class M>
struct SegLayout {
    static constexpr int NX = M::NX, NU = M::NU, NXP = (M::NX + 3) / 4 * 4;
    int SUM_P, SUM_PB, SUM_PHI, SUM_GAM, SUM_T, QS, CS, PHS, LT, XA, SL, ZL;
    __host__ __device__ explicit SegLayout(int S)
    {
        SUM_P = 0;                          // [S][NX][NX] double
        SUM_GAM = SUM_P + 2 * S * NX * NX;  // [S][NX][NX] double (fp64 sum: the dual sweep factors -Gam_0)
        SUM_PB = SUM_GAM + 2 * S * NX * NX; // [S][NX]
        SUM_PHI = SUM_PB + S * NX;          // [S][NX][NX]
        SUM_T = SUM_PHI + S * NX * NX;      // [S][NX]
        QS = (SUM_T + S * NX + 1) / 2 * 2;  // [S][NX][NX] double
        CS = QS + 2 * S * NX * NX;          // [S][NX] double
        PHS = CS + 2 * S * NX;              // [S][NX] double
        LT = PHS + 2 * S * NX;              // [2][NX][NX] double: the master rows' transpose scratch
        XA = LT + 4 * NX * NX;              // [2][NX + 1][NX] + [NX] double: Phat_m, phat_m / Shat_m, shat_m; lam_m
        SL = XA + 4 * (NX + 1) * NX + 2 * NX;  // [S + 1][2][NX]: s_q, lam_q
        ZL = SL + (S + 1) * 2 * NX;         // [N + 1][NU][NXP]
    }
    __host__ __device__ size_t floats(int N) const { return (size_t)ZL + (size_t)(N + 1) * NU * NXP; }
};

// layout of the kernel's dynamic LDS (floats): P0's stage inputs [N+1][SF][16], reference poses [N+1][3], block
// reductions [W][8], dx [N+1][16], unwrapped references [N+1][3], 64 pad floats (per-lane store targets nobody
// reads); then the IPM's per-iteration stage fields (ItLds) and (SEG) the segment area, each reusing the stage-input
// region where it fits there (P0 is done with it before the first IPM iteration, behind a block barrier)
template <class M>
struct RowLds {
    static constexpr int SF = StageLds<M>::SF;
    __host__ __device__ static constexpr size_t r4(size_t f) { return (f + 3) / 4 * 4; }
    __host__ __device__ static constexpr size_t stage_floats(int N) { return (size_t)(N + 1) * SF * 16; }
    __host__ __device__ static constexpr size_t pad_off(int N) { return (size_t)(N + 1) * (16 * SF + 3 + 16 + 3) + 32; }
    __host__ __device__ static constexpr size_t base_floats(int N) { return pad_off(N) + 64; }
    __host__ __device__ static constexpr size_t it_off(int N)
    {
        return ItLds<M>::floats(N) <= stage_floats(N) ? 0 : r4(base_floats(N));
    }
    __host__ __device__ static constexpr size_t it_end(int N) { return r4(it_off(N) + ItLds<M>::floats(N)); }
    __host__ __device__ static size_t seg_off(int N, int S)
    {
        const size_t sf = SegLayout<M>(S).floats(N);
        if (it_off(N) == 0) return it_end(N) + sf <= stage_floats(N) ? it_end(N) : r4(base_floats(N));
        return it_end(N);
    }
    __host__ __device__ static size_t floats(int N, int S)
    {
        size_t end = base_floats(N) > it_end(N) ? base_floats(N) : it_end(N);
        if (S > 0) {
            const size_t se = seg_off(N, S) + SegLayout<M>(S).floats(N);
            end = se > end ? se : end;
        }
        return end;
    }
};

// LDS of a resumed tick (RESUME: the team kernel's hand-off, sqp_rti_team_ho.hip), one slice per wave, in floats from
// the slice's base (8-byte aligned): 64 pad floats (per-lane store targets nobody reads), the IPM's per-iteration
// stage fields (ItLds), the segment area (SegLayout). No stage inputs, reference poses, dx or block reductions: P0 ran
// in the team form, and a one-wave tick reduces inside the wave. diff N = 40, S = 4: 5348 floats (21.4 KB)
template <class M>
struct ResumeLds {
    __host__ __device__ static constexpr size_t r4(size_t f) { return (f + 3) / 4 * 4; }
    __host__ __device__ static constexpr size_t it_off() { return 64; }
    __host__ __device__ static constexpr size_t seg_off(int N) { return it_off() + r4(ItLds<M>::floats(N)); }
    __host__ __device__ static size_t floats(int N, int S) { return r4(seg_off(N) + SegLayout<M>(S).floats(N)); }
};

// Whether the one-wave kernels of a translation unit take the block barrier at their phase boundaries, as they did
// before the team kernel's hand-off gave them the wave-local fence (blk_sync, sqp_rti_rowpar_tick.hpp). The product:
// no. chk_w1bar.hip, the source of the checker build lib/chk_w1bar, specialises it to true before it includes
// sqp_rti_rowpar.hip (a trait, not a macro: the tick's text has no preprocessor branch for it)
template <class T = void>
struct W1Barrier {
    static constexpr bool value = false;
};

// What a resumed tick takes from its includer in place of P0's results (rs in sqp_rti_rowpar_tick.hpp; the plain
// kernels hold an empty one): the robot, its LDS slice, the iteration it resumes at the top of, and the IPM scalars
// the team loop carried there
struct TickResume {
    int inst, it;
    float* lds;
    float alpha, sigma_mu, tg_rhs, mu_prev, we_lane;
};

namespace {

template <int F0, int F1, int RS, bool QM>
__device__ __forceinline__ void ld_range(const float* p, float (&v)[RS])
{
    rec_load_range<F0, F1, RS, QM>(p, v);
}

// zeros: the warm-start multiplier source of a cold robot (the flag selects the address, not the value)
__device__ __attribute__((aligned(16))) float g_rp_zero4[4];

// cross-row reductions of the wave (the four rows hold disjoint stages in the stage-parallel phases)
__device__ __forceinline__ float wave_sum_rows(float v)
{
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}
__device__ __forceinline__ float wave_max_rows(float v)
{
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float wave_min_rows(float v)
{
    v = fminf(v, __shfl_xor(v, 16));
    return fminf(v, __shfl_xor(v, 32));
}

}  // namespace

}  // namespace nmpc
