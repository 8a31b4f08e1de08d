// qp_wave_solve.inc — the wave-register path (nk <= 36), substitutions: products with the knots' M_j staged through LDS (KsPieces ..
// solve_staged).  Included by qp.hip after qp_wave_factor.inc, whose twist_mid, KF_SLOT / KF_ELEM / KF_DINV and coupling_coef it needs; from qp.hip the levers
// (QP_THREADS, QP_STAGE_BUFS, QP_STAGE_REGS, QP_LF_PACKED, QP_CHAIN_PRIO), knot_factor_layout.h and QG / QGC; QpDims, QpWs (qp_base.inc); kl_lds, kl_sync, KL_LD, KL_I (knot_lds.inc).

// Substitutions T du = rhs for the twisted factorisation (round 3: matrix-vector products with the explicit M_j = L_j^-T instead of
// 36-step dependent triangular solves).  With X_j = T_{j,jp} M_jp (jp = the chain's previous knot, never stored):
//   forward   r'  = rhs_j - T_{j,jp} v_jp          (3x3-block sparse)         y = M_j' r'      z_j = D_j^-1 y      v_j = M_j z_j
//   backward  w   = T_{jn,j}' x_jn                 (jn = next knot towards the middle)
//             x_j = M_j (z_j - D_j^-1 M_j' w)
// i.e. two dense products with the SAME staged matrix per chain step (one by columns, one by rows), vectors broadcast from LDS.
// The knots' M_j are STAGED THROUGH LDS: waves 2.. prefetch the blocks of step s + QP_STAGE_BUFS - 1 (coalesced global reads) while
// waves 0 / 1 run step s of the left / right chain.  rhs -> z -> x lives in LDS throughout (vec).
// ROLE: 0 = compiled for the two chain waves, 1 = for the staging waves (2..): two __noinline__ functions (solve_entry_*), so that the
// staging waves -- a dozen registers -- have no prologue saving callee-saved VGPRs.
// The step bodies and their two products (KsPieces: a lane owns a piece of a row or column) are stated in knot_subst.h, for this file,
// for the forward steps the chain waves take along the factorisation (QP_FWD_IN_FACTOR, qp_wave_factor.inc) and for the host.
#include "knot_subst.h"

template <int NK>
struct KsLayout {  // doubles
    static constexpr int SM = NK * KL_LD, SCH = SM + KL_I, STG = 2 * SCH;  // a stage: left chain (M, 1/d), right chain (M, 1/d)
    static constexpr int LEAD = 16;  // zeros in front of the first stage buffer (a row piece may start a few entries before its block)
    // per chain: A (r' / w), Z (z / u), V (v / x of the block just done), each with zero padding either side, and the pieces' scratch
    static constexpr int VECS = 6 * KS_VLEN + 2 * 64;
};

// (round 6) the solution's way back to control space (apply_F) can start from the LDS vector the substitutions end with, instead of from a copy
// in global memory written by one loop and read back by the next: dx_out != null fuses it into the epilogue (wave path only)
struct SolveOut {
    double* dx_out;    // [nb][3][oq] direction in control space, or null: the reduced solution goes to rhs as before
    const double* Lk;  // QpWs::Lk
    int oq;
    // ... and the right-hand side (rhs_from_acc) can be formed straight into that LDS vector: rhs_mode 1 = predictor, 2 = corrector, 0 = read rhs
    // 3 (QP_FWD_IN_FACTOR, blocks on the fused path): BACKWARD ONLY -- the chains took the forward steps and the middle block along the
    // factorisation (wave_forward_step, wave_factor_mid): rhs holds z_j and x_mid; both chains' V start as x_mid, the steps SF + 1 .. 2 SF run,
    // and only their blocks are staged
    int rhs_mode = 0;
    const double* cpacc = nullptr;  // QpWs::cpacc
    const double* rbase = nullptr;  // QpWs::rbase
    double sigma_mu = 0;
};
template <int NK, int ROLE>
__device__ __forceinline__ void solve_staged(const QpDims& d, const QpWs& w, double* rhs, double* lds, SolveOut so = SolveOut{nullptr, nullptr, 0}) {
    using KS = KsLayout<NK>;
    constexpr int STG = KS::STG, SCH = KS::SCH, SM = KS::SM;
    const int tid = threadIdx.x, nj = d.nj, mid = twist_mid(nj);
    const int nl = mid, nr = nj - 1 - mid, SF = nl > nr ? nl : nr;
    const int nsteps = 2 * SF + 1;  // SF forward steps, the middle block, SF backward steps
    constexpr bool FWD = QP_FWD_IN_FACTOR && kl_fused_path(NK);  // (only then can rhs_mode be 3)
    const bool bwd_only = FWD && so.rhs_mode == 3;
    const int s_first = bwd_only ? SF + 1 : 0;  // first step of this call
    lds += KS::LEAD;                                   // (zero-filled with the stage buffers below)
    kl_lds* vec = (kl_lds*)(lds + QP_STAGE_BUFS * STG);  // nj*NK: rhs -> z -> x  (LDS pointers: through generic ones every access is a flat instruction)
    kl_lds* small = vec + ((nj * NK + 1) & ~1);        // [2 chains][A, Z, V][KS_VLEN], then [2 chains][64] partial sums
    // block indices handled at step s by the left / right wave (-1: idle)
    auto left_j = [&](int s) { return s < SF ? (s - (SF - nl) >= 0 ? s - (SF - nl) : -1) : (s == SF ? mid : (mid - 1 - (s - SF - 1) >= 0 ? mid - 1 - (s - SF - 1) : -1)); };
    auto right_j = [&](int s) { return s < SF ? (s - (SF - nr) >= 0 ? nj - 1 - (s - (SF - nr)) : -1) : (s == SF ? -1 : (mid + 1 + (s - SF - 1) <= nj - 1 ? mid + 1 + (s - SF - 1) : -1)); };
    // Staging (waves 2..): what a knot left for the substitutions -- the triangle of M_j, row behind row, then 1 / d_j -- is ONE RUN of
    // QpWs::Lf (knot_factor_layout.h), and the staging threads share the two chains' runs in UNITS of 16 bytes (odd NK: 8), consecutive
    // threads consecutive units: thread t has the units t, t + NST, ... of the left chain's run followed by the right chain's, the same for
    // every step.  Their sources follow from the unit's number; their destinations inside a stage are mapped once per call, so that a
    // step is ONE batch of loads in flight per thread and a batch of LDS stores.  What lies left of the diagonal in the stage buffers is
    // zero-filled once per call (an odd row's first pair brings the zero left of its diagonal along).
    // (QP_LF_PACKED = 0: the square image, a unit is one of the NE doubles of the triangle and 1 / d_j, and its source is mapped as well.)
    constexpr bool PK = QP_LF_PACKED != 0;
    constexpr int NTRI = NK * (NK + 1) / 2, NE = NTRI + NK;
    constexpr int UN = PK ? kf_unit(NK) : 1, NU = PK ? kf_units(NK) : NE;  // doubles per unit, units per chain
    constexpr int NST = QP_THREADS - 128, MAXE = (2 * NU + NST - 1) / NST;
    typedef typename std::conditional<UN == 2, kl_d2, double>::type unit_t;
    // (explicitly GLOBAL loads and LDS stores: through generic pointers they are flat instructions, which count on both memory counters
    // and make the compiler wait for ALL of them at the first use -- no load would stay in flight across a barrier)
    typedef __attribute__((address_space(1))) const double gdbl;
    typedef __attribute__((address_space(1))) const unit_t gunit;
    typedef __attribute__((address_space(3))) unit_t lunit;
    static_assert(UN == 1 || (KL_LD % 2 == 0 && SM % 2 == 0 && SCH % 2 == 0 && STG % 2 == 0 && KS::LEAD % 2 == 0), "16-byte units: even offsets in a stage");
    int doff[MAXE];                              // unit u of this thread: destination inside a stage (-1: none)
    [[maybe_unused]] int soff[PK ? 1 : MAXE];    // square image: its source offset inside a knot's slot
    if (ROLE == 1) {
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const int e = (tid - 128) + u * NST;
            doff[u] = -1;
            if constexpr (!PK) soff[u] = 0;
            if (e < 2 * NU) {
                [[maybe_unused]] const int side = e >= NU, idx = side ? e - NU : e;
                if constexpr (PK) {
                    const int dd = kf_stage_dst(NK, kf_unit_off(NK, e), KL_LD, SM);  // (-1: the gap between an odd triangle and 1 / d)
                    doff[u] = dd >= 0 ? kf_unit_side(NK, e) * SCH + dd : -1;
                } else if (idx < NTRI) {
                    int rw = (int)(((2 * NK + 1) - sqrtf((float)((2 * NK + 1) * (2 * NK + 1) - 8 * idx))) * 0.5f);
                    if (rw * NK - rw * (rw - 1) / 2 > idx) rw--;
                    if ((rw + 1) * NK - (rw + 1) * rw / 2 <= idx) rw++;
                    const int k = rw + idx - (rw * NK - rw * (rw - 1) / 2);
                    soff[u] = KF_ELEM(NK, rw, k), doff[u] = side * SCH + rw * KL_LD + k;
                } else {
                    soff[u] = KF_DINV(NK) + (idx - NTRI), doff[u] = side * SCH + SM + (idx - NTRI);
                }
            }
        }
    }
    // unit u of this thread at the chains' slots srcl / srcr.  No predicates: a unit nobody needs (behind both runs; a chain that idles:
    // the callers pass knot 0) reads a valid address and is never stored where a product sees it -- straight-line loads are what lets the
    // compiler count them (s_waitcnt vmcnt(n), n > 0) instead of waiting for all
    auto unit_src = [&](int u, gdbl* srcl, gdbl* srcr) {
        if constexpr (PK) {
            const int e = (tid - 128) + u * NST;
            return (gunit*)((kf_unit_side(NK, e) ? srcr : srcl) + (e < 2 * NU ? kf_unit_off(NK, e) : 0));
        } else {
            return (gunit*)((doff[u] >= SCH ? srcr : srcl) + soff[u]);
        }
    };
    auto stage_load = [&](int s, unit_t (&tmp)[MAXE]) {
        if (s >= nsteps) return;
        const int jl = left_j(s), jr = right_j(s);
        gdbl* srcl = (gdbl*)(w.Lf + (size_t)(jl >= 0 ? jl : 0) * KF_SLOT(NK));
        gdbl* srcr = (gdbl*)(w.Lf + (size_t)(jr >= 0 ? jr : 0) * KF_SLOT(NK));
#pragma unroll
        for (int u = 0; u < MAXE; ++u) tmp[u] = *unit_src(u, srcl, srcr);
    };
    auto stage_store = [&](int s, const unit_t (&tmp)[MAXE], double* buf) {
        if (s >= nsteps) return;
        const int jl = left_j(s), jr = right_j(s);
        kl_lds* bl = (kl_lds*)buf;
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const bool right = doff[u] >= SCH;
            if (doff[u] >= 0 && (right ? jr >= 0 : jl >= 0)) *(lunit*)(bl + doff[u]) = tmp[u];
        }
    };
    auto stage = [&](int s, double* buf) {  // one step's blocks, loaded and stored on the spot
        unit_t tmp[MAXE];
        stage_load(s, tmp);
        stage_store(s, tmp, buf);
    };
    // (round 6) The two halves apart let a staging thread's loads stay in flight ACROSS step barriers: under full load a trip to global
    // memory (3-5 us) is longer than a chain step (~1.5 us), and a staging wave that loads, waits and stores inside one step made every
    // step as long as that trip however many stage buffers there were (which is why a third buffer never paid).  With QP_STAGE_REGS = R
    // register sets the loads of step s + QP_STAGE_BUFS - 1 + R are issued at step s and stored R steps later.
    // (Issuing the call's first loads up here, ahead of the right-hand side's own, was built and measured: no gain; profiles/packed_m_ab.txt.)
    if (FWD ? so.rhs_mode == 1 || so.rhs_mode == 2 : so.rhs_mode != 0) {  // rhs_from_acc into the LDS vector (same arithmetic): rhs = rbase + F'(G'v) of the sweep's accumulators
        constexpr int nu = NK / 3;
        const int oq = so.oq;
        const size_t ncp = (size_t)(NK / 9) * oq;
        const bool corrector = so.rhs_mode == 2;
        for (int it = tid; it < nj * nu; it += QP_THREADS) {
            const int j = it / nu + 1, u = it % nu, a = u / 3, k = u % 3;
            double g[6];  // G'v at control points 6(j-1)+3 .. 6j+2 of (agent a, dim k)
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int j6 = 6 * (j - 1) + 3 + q;
                const __attribute__((address_space(1))) double* ac = QGC(so.cpacc) + (size_t)a * oq + j6;
                g[q] = corrector ? ac[k * ncp] - so.sigma_mu * ac[(3 + k) * ncp] : ac[(6 + k) * ncp];
            }
            const __attribute__((address_space(1))) double* L = QGC(so.Lk) + 9 * j;
            const size_t o0 = (size_t)(j - 1) * NK + u * 3;
#pragma unroll
            for (int e = 0; e < 3; ++e) vec[o0 + e] = QGC(so.rbase)[o0 + e] + g[3 + e] + L[0 + e] * g[0] + L[3 + e] * g[1] + L[6 + e] * g[2];
        }
    } else {  // rhs -> LDS: every thread's loads first, then its stores (one trip to memory instead of one per round; see apply_F)
        constexpr int RQ = 4;
        for (int i0 = tid; i0 < nj * NK; i0 += RQ * QP_THREADS) {
            double t[RQ];
#pragma unroll
            for (int q = 0; q < RQ; ++q) t[q] = i0 + q * QP_THREADS < nj * NK ? rhs[i0 + q * QP_THREADS] : 0.0;
#pragma unroll
            for (int q = 0; q < RQ; ++q)
                if (i0 + q * QP_THREADS < nj * NK) vec[i0 + q * QP_THREADS] = t[q];
        }
    }
    for (int i = tid; i < KS::VECS; i += QP_THREADS) small[i] = 0.0;
    for (int i = tid; i < KS::LEAD + QP_STAGE_BUFS * STG; i += QP_THREADS) (lds - KS::LEAD)[i] = 0.0;
    __syncthreads();
    if (bwd_only && tid < NK) small[KS_VPAD + 2 * KS_VLEN + tid] = small[KS_VPAD + 5 * KS_VLEN + tid] = vec[mid * NK + tid];  // x_mid into both chains' V
    if (ROLE == 1)  // the stages the chains start with
        for (int s0 = s_first; s0 < s_first + QP_STAGE_BUFS - 1 && s0 < nsteps; ++s0) stage(s0, lds + (s0 % QP_STAGE_BUFS) * STG);
    __syncthreads();
    const int wave = ROLE == 0 ? (tid >> 6) & 1 : 2, r = tid & 63;  // (role 1 only needs "wave >= 2")
    const bool act = r < NK;
    const int rr = act ? r : 0, g3 = 3 * (rr / 3), r3 = rr % 3;
    const int rs = act ? r : NK + 12;  // lanes >= NK write a slot behind the zero padding of the chain vectors
    if (wave < 2) __builtin_amdgcn_s_setprio(QP_CHAIN_PRIO);  // see twisted_factor
    // the three coupling coefficients a chain step starts with (forward: row rr of T_{j,jp}; backward: column rr of T_{jn,j}) come from
    // global memory: fetched ONE STEP AHEAD (the trip to the L2, ~1 us under load, was the first thing every step waited for)
    auto step_coef = [&](int s, double& q0, double& q1, double& q2) {
        q0 = q1 = q2 = 0.0;
        if (ROLE != 0 || s >= nsteps || s == SF) return;
        const int jb = wave == 0 ? left_j(s) : right_j(s);
        if (jb < 0) return;
        const int dir = wave == 0 ? +1 : -1;
        if (s < SF) {
            const bool has_prev = wave == 0 ? jb > 0 : jb + 1 < nj;
            if (has_prev) coupling_coef(w, jb - dir, dir, rr, q0, q1, q2);
        } else {
            const __attribute__((address_space(1))) double* E = QGC(w.Ek) + 9 * (dir > 0 ? jb + 1 : jb);
            q0 = dir > 0 ? E[3 * r3] : E[r3], q1 = dir > 0 ? E[3 * r3 + 1] : E[3 + r3], q2 = dir > 0 ? E[3 * r3 + 2] : E[6 + r3];
        }
    };
    double cf0, cf1, cf2;
    step_coef(s_first, cf0, cf1, cf2);
#ifdef QP_SOLVE_TIMERS  // developer build: left chain wave, SC 25 = work of the steps, 26 = waiting at the step barrier (staging wave: 29 / 30, right chain: 33 / 34)
    long long st_ = wall_clock64();
#define SOLVE_T(slot)                                                              \
    do {                                                                           \
        const long long t_ = wall_clock64();                                       \
        const int who_ = ROLE == 0 ? (tid == 0 ? 0 : (tid == 64 ? 8 : -1)) : (tid == 128 ? 4 : -1); /* left chain 25/26, staging wave 29/30, right chain 33/34 */ \
        if (w.prof && who_ >= 0) w.prof[slot + who_] += (double)(t_ - st_);        \
        st_ = t_;                                                                  \
    } while (0)
#else
#define SOLVE_T(slot)
#endif
    if (ROLE == 1 && QP_STAGE_REGS > 0) {
        constexpr int R = QP_STAGE_REGS > 0 ? QP_STAGE_REGS : 1;
        unit_t tq[R][MAXE];
#pragma unroll
        for (int k = 0; k < R; ++k) stage_load(s_first + QP_STAGE_BUFS - 1 + k, tq[k]);
        // steady state, straight-line (no predicate, no branch between a load and its store: only then does the compiler count the loads in
        // flight instead of waiting for all of them): every unit is stored -- the ones a thread does not have go to padding columns
        // nobody's products see (row 0, from column NK for a 16-byte unit, else column KL_LD - 1: times the zero padding of the vectors), a
        // chain that idles at a step gets knot 0's numbers into its half of the buffer, which it does not read
        constexpr int DUMP = UN == 2 ? NK : KL_LD - 1;
        static_assert(DUMP + UN <= KL_LD, "the padding columns of row 0");
        int dsto[MAXE];
#pragma unroll
        for (int u = 0; u < MAXE; ++u) dsto[u] = doff[u] >= 0 ? doff[u] : DUMP;
        // The loads of the NEXT R steps are issued at the top of an iteration and first touched at its bottom, R step barriers later: the
        // compiler drains the memory counter completely wherever a loop-carried load is used (it does not count across a back edge), so the
        // one place where everything must have landed is made to be the place where it drains.
        unit_t nq[R][MAXE];
        int s = s_first;
        for (; s + 2 * R + QP_STAGE_BUFS - 1 <= nsteps; s += R) {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int sl = s + R + k + QP_STAGE_BUFS - 1;
                const int jl = left_j(sl), jr = right_j(sl);
                gdbl* srcl = (gdbl*)(w.Lf + (size_t)(jl >= 0 ? jl : 0) * KF_SLOT(NK));
                gdbl* srcr = (gdbl*)(w.Lf + (size_t)(jr >= 0 ? jr : 0) * KF_SLOT(NK));
#pragma unroll
                for (int u = 0; u < MAXE; ++u) nq[k][u] = *unit_src(u, srcl, srcr);
            }
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int sp = s + k + QP_STAGE_BUFS - 1;
                kl_lds* bl = (kl_lds*)(lds + (sp % QP_STAGE_BUFS) * STG);
#pragma unroll
                for (int u = 0; u < MAXE; ++u) *(lunit*)(bl + dsto[u]) = tq[k][u];
                __syncthreads();
            }
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int u = 0; u < MAXE; ++u) tq[k][u] = nq[k][u];
        }
        for (; s < nsteps; s += R) {  // the last few steps (loads or stores that do not exist any more: predicated)
#pragma unroll
            for (int k = 0; k < R; ++k) {
                if (s + k < nsteps) {  // (uniform: every thread of the workgroup passes nsteps barriers, here or in the chains' loop)
                    const int sp = s + k + QP_STAGE_BUFS - 1;
                    stage_store(sp, tq[k], lds + (sp % QP_STAGE_BUFS) * STG);
                    stage_load(sp + R, tq[k]);
                    __syncthreads();
                }
            }
        }
    } else
    for (int s = s_first; s < nsteps; ++s) {
        SOLVE_T(26);
        const double e0 = cf0, e1 = cf1, e2 = cf2;
        step_coef(s + 1, cf0, cf1, cf2);
        double* buf = lds + (s % QP_STAGE_BUFS) * STG;
        if (ROLE == 1) {
            const int sp = s + QP_STAGE_BUFS - 1;
            if (sp < nsteps) stage(sp, lds + (sp % QP_STAGE_BUFS) * STG);
        } else if (s == SF) {
            if (wave == 0) {  // middle block: forward with both neighbours' v, then backward; x_mid goes to both chains' V
                const kl_lds* Mst = (const kl_lds*)buf;
                kl_lds *A0 = (kl_lds*)small + KS_VPAD, *Z0 = A0 + KS_VLEN, *V0 = A0 + 2 * KS_VLEN, *V1 = A0 + 5 * KS_VLEN;
                kl_lds* ps = (kl_lds*)small + 6 * KS_VLEN;
                double v = vec[mid * NK + rr];
                if (mid > 0) {
                    double e0, e1, e2;
                    coupling_coef(w, mid - 1, +1, rr, e0, e1, e2);
                    v -= e0 * V0[g3] + e1 * V0[g3 + 1] + e2 * V0[g3 + 2];
                }
                if (mid + 1 < nj) {
                    double e0, e1, e2;
                    coupling_coef(w, mid + 1, -1, rr, e0, e1, e2);
                    v -= e0 * V1[g3] + e1 * V1[g3 + 1] + e2 * V1[g3 + 2];
                }
                const double x = ks_step_middle<NK>(Mst, Mst + SM + rr, v, A0, Z0, ps, r, rs, [] { kl_sync(); });
                V0[rs] = x, V1[rs] = x;
                if (act) vec[mid * NK + r] = x;
            }
        } else {
            const bool fwd = s < SF;
            const int jb = wave == 0 ? left_j(s) : right_j(s);
            if (jb >= 0) {
                const kl_lds* Mst = (const kl_lds*)(buf + (wave == 0 ? 0 : SCH));
                kl_lds *A = (kl_lds*)small + KS_VPAD + (wave == 0 ? 0 : 3 * KS_VLEN), *Z = A + KS_VLEN, *V = A + 2 * KS_VLEN;
                kl_lds* ps = (kl_lds*)small + 6 * KS_VLEN + (wave == 0 ? 0 : 64);
                const double dinv = Mst[SM + rr];
                if (fwd) {
                    const bool has_prev = wave == 0 ? jb > 0 : jb + 1 < nj;
                    ks_step_forward<NK>(Mst, dinv, vec[jb * NK + rr], has_prev, e0, e1, e2, A, Z, V, ps, r, g3, rs, [] { kl_sync(); }, [&](double z) {
                        if (act) vec[jb * NK + r] = z;
                    });
                } else {
                    const double x = ks_step_backward<NK>(Mst, dinv, vec + jb * NK + rr, e0, e1, e2, A, Z, V, ps, r, g3, rs, [] { kl_sync(); });
                    if (act) vec[jb * NK + r] = x;
                }
            }
        }
        SOLVE_T(25);
        __syncthreads();
    }
    if (wave < 2) __builtin_amdgcn_s_setprio(0);
    if (so.dx_out) {  // apply_F from the LDS vector (same arithmetic, same order)
        constexpr int nu = NK / 3;
        const int oq = so.oq;
        for (int it = tid; it < nj * nu; it += QP_THREADS) {
            const int j = it / nu + 1, u = it % nu;
            const kl_lds* uu = vec + (size_t)(j - 1) * NK + u * 3;
            const __attribute__((address_space(1))) double* L = QGC(so.Lk) + 9 * j;
            const double u0 = uu[0], u1 = uu[1], u2 = uu[2];
            __attribute__((address_space(1))) double* o = QG(so.dx_out) + (size_t)u * oq + 6 * (j - 1) + 3;  // control points 6(j-1)+3 .. 6j+2
            o[0] = L[0] * u0 + L[1] * u1 + L[2] * u2;
            o[1] = L[3] * u0 + L[4] * u1 + L[5] * u2;
            o[2] = L[6] * u0 + L[7] * u1 + L[8] * u2;
            o[3] = u0, o[4] = u1, o[5] = u2;
        }
        for (int it = tid; it < nu * 6; it += QP_THREADS) {  // the pinned ends
            const int u = it / 6, q = it % 6;
            QG(so.dx_out)[(size_t)u * oq + (q < 3 ? q : oq - 6 + q)] = 0.0;
        }
    } else {
        for (int i = tid; i < nj * NK; i += QP_THREADS) rhs[i] = vec[i];
    }
    __threadfence_block();
    __syncthreads();
}
