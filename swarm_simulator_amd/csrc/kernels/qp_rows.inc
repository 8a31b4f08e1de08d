// qp_rows.inc — the row sweeps of the batch QP: the passes (PASS_*), what a sweep takes and returns (PassIO), the row context of a batch QP
// (SweepMeta, RowCtx), the arithmetic of one row (row_op), the walk over the rows of a work item with its three frozen-row streams (row_pass)
// and the stand-alone sweeps of the interior-point loop (sweep<PASS>, SWEEP).  Included by qp.hip after qp_polish_types.inc, whose Cand,
// PolishWs and emit_cand it needs; from qp.hip the levers (QP_THREADS, QP_ROW_UNROLL, QP_ROW_PF, QP_ROW_BLK, QP_WARM_TAU) and QG / QGC / QGF;
// QpDims, QpWs (qp_base.inc); the row arithmetic of ipm:: (common/ipm_rows.h, which only qp.hip itself includes).

// ------------------------------------------------------------------------------------------------------------
// row sweeps (the rows of a batch QP and the work item of a sweep: see row_pass)
// ------------------------------------------------------------------------------------------------------------
enum { PASS_INIT = 0, PASS_BUILD, PASS_AFF, PASS_STEP, PASS_PRESOLVE, PASS_CAND, PASS_VERIFY, PASS_CAND_GEO,
       PASS_UPBUILD /* step of iteration i (old state -> new state arrays) fused with BUILD of iteration i+1 */ };

// the passes whose frozen-row stream runs in blocks where QP_ROW_BLK > 0: the four sweeps of the interior-point loop and the polish's
constexpr bool pass_in_blocks(int pass) {
    return pass == PASS_BUILD || pass == PASS_AFF || pass == PASS_STEP || pass == PASS_UPBUILD || pass == PASS_CAND || pass == PASS_VERIFY ||
           pass == PASS_CAND_GEO;
}
// the passes that read a row's stored (s, z): the sweeps of the interior-point loop and the polish's candidate search on its iterate
constexpr bool pass_reads_sz(int pass) {
    return pass == PASS_BUILD || pass == PASS_AFF || pass == PASS_STEP || pass == PASS_UPBUILD || pass == PASS_CAND;
}

struct PassIO {
    // inputs
    double mu0, s_floor, dreg, sigma_mu, alpha;
    // outputs (block-reduced by the caller)
    double sum0, sum1, sum2, vmax, vmin;
};

// (round 6) what a sweep looks up per control point before it can request anything -- its group, the group's row counts and normal offset,
// its tile's first slot -- copied ONCE per batch QP into LDS (by rank, i.e. already through fperm): in global memory these were two dependent
// trips per control point.  Only filled when the batch fits (wave path: nb <= 4); RowCtx::meta is null otherwise.
#define QP_META_G 160
struct SweepMeta {
    unsigned short fbase[QP_META_G];
    unsigned char grp[QP_META_G], near[QP_META_G], all[QP_META_G];
    int tile_base[16];
};
struct RowCtx {
    const SweepMeta* meta;  // LDS (see SweepMeta), or null: EVERY construction site sets it
    const PolishWs* pw;
    double* scal;  // this mission's diagnostic scalars (DevSession::scalars + mission * SC_N).  NOT a pointer to the DevSession:
                   // taking the kernel argument's address forces the whole struct into scratch memory
    int mission;
    int lds_avail;  // doubles of dynamic LDS behind the work-area pointer handed to the phases
    QpDims d;
    QpWs w;
    const double* ctrl;  // [N][3][oq] of this mission
    const float* normals;  // [npair][M][3]
    const double* radius;  // [N]
};

// 1/sqrt(x): v_rsq_f64 plus two Newton steps (full double precision for normal x > 0); an IEEE sqrt followed by an IEEE
// division is ~6x the instructions and sits on the dependent chain of every Cholesky column
__device__ __forceinline__ double fast_rsqrt(double x) {
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    y = fma(y, fma(-h * y, y, 0.5), y);
    y = fma(y, fma(-h * y, y, 0.5), y);
    return y;
}

// One row of G x <= h at slot r.  slack = h - g.x at the CURRENT control points (PASS_UPBUILD: at the trial point x + alpha dx),
// ga = g . dx_aff, gd = g . dx.  cw = 1 for rows that count in the sums, 0 for the second copy of a pair row.  Returns the
// Newton weight wgt, the right-hand-side scalar v and the multiplier zo where the pass defines them.  Step-length limits are
// tracked as io.vmax = max(-ds/s, -dz/z) (the caller takes the reciprocal), which needs no data-dependent division.
// Three steps per pass: fetch (s, z), the row's arithmetic (common/ipm_rows.h), store and reduce.  The corrector term and the step
// (ds, dz) are functions of (s, z, ga, gd): the STEP and UPBUILD sweeps recompute them instead of reading them back (three stored
// arrays fewer, see the note above QpWs).
// PRE: (s, z) of the row were fetched by the caller (the prefetch ring / the blocks of the frozen-row stream, QP_ROW_PF / QP_ROW_BLK)
template <int PASS, bool PRE = false>
__device__ __forceinline__ void row_op(double slack, double ga, double gd, size_t r, const QpWs& w, PassIO& io, double cw, double& wgt,
                                       double& v, double& zo, double s_in = 0.0, double z_in = 0.0) {
    constexpr bool rd_sz = pass_reads_sz(PASS);
    double s = 0.0, z = 0.0;
    if (rd_sz) s = PRE ? s_in : QGC(w.s)[r], z = PRE ? z_in : QGC(w.z)[r];
    if (PASS == PASS_INIT) {
        const double s0 = slack < io.s_floor ? io.s_floor : slack;
        w.s[r] = s0;
        w.z[r] = io.mu0 / s0;
    } else if (PASS == PASS_BUILD) {
        const Build b = build(s, z, slack, io.dreg);
        wgt = b.wgt, v = b.v, zo = z;
        io.sum0 += cw * s * z;
        io.vmax = fmax(io.vmax, fabs(b.rg));
    } else if (PASS == PASS_AFF) {
        const Affine a = affine(s, z, slack, ga, io.dreg);
        io.vmax = fmax(io.vmax, a.lim);
        io.sum0 += cw * s * z, io.sum1 += cw * (s * a.dza + z * a.dsa), io.sum2 += cw * a.cc;
        v = a.v, wgt = a.wz;  // the two parts of the corrector's right-hand side: it needs no sweep of its own
    } else if (PASS == PASS_STEP) {
        const Dir d = direction(s, z, slack, ga, gd, io.dreg, io.sigma_mu, 0.0);
        io.vmax = fmax(io.vmax, step_limit(s, z, d.ds, d.dz));
    } else if (PASS == PASS_UPBUILD) {
        // old state (s, z) at the old point: slack_old = slack + alpha * gd
        const State n = step_state(s, z, direction(s, z, slack + io.alpha * gd, ga, gd, io.dreg, io.sigma_mu, 0.0), io.alpha);
        QG(w.s2)[r] = n.s, QG(w.z2)[r] = n.z;
        io.vmin = fmin(io.vmin, n.sz);  // wide-neighbourhood test of the step just applied
        // ... and the next iteration's weights / residuals at the new point
        const Build b = build(n.s, n.z, slack, io.dreg);
        wgt = b.wgt, v = b.v, zo = n.z;
        io.sum0 += cw * n.s * n.z;
        io.vmax = fmax(io.vmax, fabs(b.rg));
    } else if (PASS == PASS_PRESOLVE) {
        io.vmax = fmax(io.vmax, -slack);  // violation of a pinned (constant) row
    } else if (PASS == PASS_CAND) {
        wgt = cand_strength(s, z);
        QG(w.cc)[r] = wgt;
        v = slack;
    } else if (PASS == PASS_CAND_GEO) {
        // candidates from the geometry alone (no interior-point iterate): rows within QP_WARM_TAU of their bound at the
        // current point.  Used from the second Gauss-Seidel pass on, where the current point is the previous pass's
        // optimum of this very batch and its active rows sit at slack ~ 0.
        wgt = slack < QP_WARM_TAU ? (slack < 1e-8 ? 1e3 : 1.0) : 0.0;
        QG(w.cc)[r] = wgt;
        v = slack;
    } else if (PASS == PASS_VERIFY) {
        const double sn = slack - gd;  // slack at x + dx
        QG(w.ds)[r] = sn;
        io.vmax = fmax(io.vmax, -sn);
        if (sn < VERIFY_TOL && QGC(w.cc)[r] == 0.0) {  // violated row that is not a candidate yet
            QG(w.cc)[r] = 1.0;
            wgt = 1.0;
        }
    }
}

// One sweep over all rows of the batch QP.  Rows (G x <= h form, as in the oracle):
//   bound   (a,k,side,j6):  +x <= hi   /  -x <= -lo                       rbp_planner.hpp:626-635
//   pair    (a<b,j6):       n . x_a - n . x_b <= -rr                      :668-679
//   frozen  (a,f,j6):       sg * n . x_a <= -rr + sg * n . dummy_f        :645-666   sg = +1 if a < f else -1
// Control points j6 < 3 and j6 >= 6M-3 are pinned by the end-state equalities: their rows are constants and are only checked
// once (presolve).  Work item = one free control point of one batch agent with ALL its rows (see the note above QpWs).
// The whole batch QP runs on one workgroup: a thread takes the control points threadIdx.x, threadIdx.x + QP_THREADS, ... below nb * oq.
template <int PASS>
__device__ void row_pass(const RowCtx& c, PassIO& io) {
    const int wi0 = threadIdx.x;
    const QpDims& d = c.d;
    const QpWs& w = c.w;
    const int oq = d.oq, N = d.N, M = d.M, nb = d.nb;
    constexpr bool build = (PASS == PASS_BUILD || PASS == PASS_UPBUILD);
    constexpr bool aff = (PASS == PASS_AFF);  // S[0..2] / S[3..5] then hold the two parts of the corrector rhs (see row_op)
    constexpr bool accum = (build || aff);
    constexpr bool pinned_only = (PASS == PASS_PRESOLVE);
    constexpr bool cand = (PASS == PASS_CAND || PASS == PASS_CAND_GEO || PASS == PASS_VERIFY);
    constexpr bool need_da = (PASS == PASS_AFF || PASS == PASS_STEP || PASS == PASS_UPBUILD);
    constexpr bool need_dd = (PASS == PASS_STEP || PASS == PASS_VERIFY || PASS == PASS_UPBUILD);
    const int ncp = nb * oq;
    // tiles are ranked by falling row count and handed to the waves round robin
    // (the clamp never binds -- ncp <= QP_MAX_NB * oq -- but the compiler cannot know that and uses the bound wi < 2^30 it is given, like
    // the signed wi0: without either the sweeps and qp_batch_kernel compile to other code than the one that was measured)
    const int wi_stop = (1 << 30) < ncp ? (1 << 30) : ncp;
    for (int rnd = 0;; ++rnd) {
        const int wi = wi0 + rnd * QP_THREADS;
        if (wi >= wi_stop) break;
        constexpr bool blk_pass = QP_ROW_BLK > 0 && pass_in_blocks(PASS);  // passes that take the round-6 prologue (LDS look-ups, global loads, blocks)
        constexpr bool pre_b = blk_pass && (PASS == PASS_BUILD || PASS == PASS_AFF || PASS == PASS_STEP || PASS == PASS_UPBUILD);
        constexpr bool all_rows = (PASS == PASS_PRESOLVE || PASS == PASS_VERIFY || PASS == PASS_CAND_GEO || PASS == PASS_CAND);
        const __attribute__((address_space(3))) SweepMeta* mt = blk_pass ? (const __attribute__((address_space(3))) SweepMeta*)c.meta : nullptr;
        int grp, cnt_near, cnt_all, fb;
        size_t base;
        if (blk_pass && mt) {  // (uniform) the look-ups from LDS
            const int rk = wi / 6;
            grp = mt->grp[rk], cnt_near = mt->near[rk], cnt_all = mt->all[rk], fb = mt->fbase[rk];
            base = (size_t)mt->tile_base[wi >> 6] + (wi & 63);
        } else {
            grp = w.fperm[wi / 6];
            cnt_near = (all_rows && PASS != PASS_CAND) ? 0 : w.fnear[grp], cnt_all = all_rows ? w.fcnt[grp] : cnt_near, fb = w.fbase[grp];
            base = (size_t)w.tile_base[wi >> 6] + (wi & 63);
        }
        const int a = grp / M, seg = grp - a * M, i = wi % 6, j6 = 6 * seg + i, it = a * oq + j6;
        const bool pinned = (j6 < 3 || j6 >= oq - 3);
        if (pinned != pinned_only) continue;
        const int qa = d.first + a;
        double xa[3], da[3], dd[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (blk_pass) {
                xa[k] = QGC(c.ctrl)[((size_t)qa * 3 + k) * oq + j6];
                da[k] = need_da ? QGC(w.dxa)[((size_t)a * 3 + k) * oq + j6] : 0.0;
                dd[k] = need_dd ? QGC(w.dx)[((size_t)a * 3 + k) * oq + j6] : 0.0;
            } else {
                xa[k] = c.ctrl[((size_t)qa * 3 + k) * oq + j6];
                da[k] = need_da ? w.dxa[((size_t)a * 3 + k) * oq + j6] : 0.0;
                dd[k] = need_dd ? w.dx[((size_t)a * 3 + k) * oq + j6] : 0.0;
            }
        }
        double S[6] = {0, 0, 0, 0, 0, 0}, yv[3] = {0, 0, 0}, gz[3] = {0, 0, 0};
        const int cnt = all_rows ? cnt_all : cnt_near;
        const float* nr = w.nrm + (size_t)fb * 3;
        const size_t r0 = base + (size_t)d.ncol0 * 64;
        // (QP_ROW_BLK) the first block of the frozen-row stream is requested here, with everything else the control point starts from
        constexpr bool rd_sz_b = pass_reads_sz(PASS);
        constexpr int BB = QP_ROW_BLK > 0 ? QP_ROW_BLK : 1;
        double cs[BB], cz[BB], ch[BB];
        float cn[BB][3];
        if (blk_pass && cnt > 0) {
#pragma unroll
            for (int u = 0; u < BB; ++u) {
                const int ix = u < cnt ? u : cnt - 1;
                const size_t rx = r0 + (size_t)ix * 64;
                cs[u] = rd_sz_b ? QGC(w.s)[rx] : 0.0, cz[u] = rd_sz_b ? QGC(w.z)[rx] : 0.0, ch[u] = QGC(w.rh)[rx];
#pragma unroll
                for (int e = 0; e < 3; ++e) cn[u][e] = QGF(nr)[3 * ix + e];
            }
        }
        // ---- bound rows (idx 0..5)
        // (QP_ROW_BLK: their (s, z) are requested together up front -- in the update sweep every row's stores stand between it and the
        // next row's loads, which the compiler must not move across them)
        double bs[6] = {0, 0, 0, 0, 0, 0}, bz[6] = {0, 0, 0, 0, 0, 0};
        if (pre_b) {
#pragma unroll
            for (int e = 0; e < 6; ++e) bs[e] = QGC(w.s)[base + (size_t)e * 64], bz[e] = QGC(w.z)[base + (size_t)e * 64];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double hi = blk_pass ? QGC(w.boxhi)[((size_t)a * M + seg) * 3 + k] : w.boxhi[((size_t)a * M + seg) * 3 + k];
            const double lo = blk_pass ? QGC(w.boxlo)[((size_t)a * M + seg) * 3 + k] : w.boxlo[((size_t)a * M + seg) * 3 + k];
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const size_t r = base + (size_t)(2 * k + side) * 64;
                const double sg = side == 0 ? 1.0 : -1.0;
                const double slack = side == 0 ? hi - xa[k] : xa[k] - lo;
                double wgt = 0, v = 0, zo = 0;
                row_op<PASS, pre_b>(slack, sg * da[k], sg * dd[k], r, w, io, 1.0, wgt, v, zo, bs[2 * k + side], bz[2 * k + side]);
                if (cand && wgt != 0)
                    emit_cand(d, w, *c.pw, r, j6, a, -1, k == 0 ? sg : 0.0, k == 1 ? sg : 0.0, k == 2 ? sg : 0.0, slack,
                              (int)(((size_t)qa * 3 + k) * oq + j6), side == 0 ? hi : lo, wgt);
                if (accum) {
                    const int dg = k == 0 ? 0 : (k == 1 ? 3 : 5);  // diagonal slots of the packed 3x3
                    if (build) {
                        S[dg] += wgt;
                        gz[k] += sg * zo;
                        yv[k] += sg * v;
                    } else {
                        S[k] += sg * v, S[3 + k] += sg * wgt;
                    }
                }
            }
        }
        // a row with coefficient sg * n of this control point joins its accumulators
        auto accumulate = [&](double wgt, double v, double zo, double sg, double n0, double n1, double n2) {
            if (build) acc_build(S, yv, gz, wgt, v, zo, sg, n0, n1, n2);
            else if (aff) acc_aff(S, v, wgt, sg, n0, n1, n2);
        };
        // ---- in-batch pair rows (idx 6 .. 6 + nb - 2): canonical orientation n . (x_hi - x_lo) >= rr, so that the copy in the
        // other agent's column sees bit-identical inputs (pair_slack)
        auto pair_row = [&](auto pre_tag, int pb, double n0, double n1, double n2, const double (&xb)[3], const double (&fa)[3], const double (&fd)[3],
                            double rsum, double s_in, double z_in) {
            constexpr bool PRE_P = decltype(pre_tag)::value;
            const int b = pb < a ? pb : pb + 1;
            const bool a_lo = a < b;
            const size_t r = base + (size_t)(6 + pb) * 64;
            const double slack = pair_slack(a_lo, n0, n1, n2, xa[0], xa[1], xa[2], xb[0], xb[1], xb[2], rsum);
            const double gab = need_da ? pair_dot(a_lo, n0, n1, n2, da[0], da[1], da[2], fa[0], fa[1], fa[2]) : 0.0;
            const double gdb = need_dd ? pair_dot(a_lo, n0, n1, n2, dd[0], dd[1], dd[2], fd[0], fd[1], fd[2]) : 0.0;
            double wgt = 0, v = 0, zo = 0;
            row_op<PASS, PRE_P>(slack, gab, gdb, r, w, io, a_lo ? 1.0 : 0.0, wgt, v, zo, s_in, z_in);
            if (cand && wgt != 0 && a_lo) emit_cand(d, w, *c.pw, r, j6, a, b, n0, n1, n2, slack, -1, 0.0, wgt);
            if (build && a_lo) w.pwgt[(size_t)(a * nb - a * (a + 1) / 2 + (b - a - 1)) * oq + j6] = wgt;
            accumulate(wgt, v, zo, pair_sign(a_lo), n0, n1, n2);
        };
        if (pre_b && nb > 1 && nb <= 4) {
            // (QP_ROW_BLK) up to three pair rows: everything they read -- normal, the other agent's point and directions, radii, (s, z) -- is
            // requested for all of them before the first is worked on (each cost two trips to memory, one after the other).
            // A batch of one agent has no pair row, no slot 6 in its tile and, where it is the whole mission, no normal at all: it takes
            // the loop below, which then runs no round and loads nothing.
            float pn[3][3];
            double pxb[3][3], pfa[3][3], pfd[3][3], prs[3], pps[3], ppz[3];
#pragma unroll
            for (int pb = 0; pb < 3; ++pb) {
                const int pq = pb < nb - 1 ? pb : 0;  // (a row that does not exist reads row 0's operands -- nb > 1: that row exists -- and is not worked on)
                const int b = nb > 1 ? (pq < a ? pq : pq + 1) : 0;  // (nb > 1 holds here; spelt out, the register allocation is the one it was)
                const bool a_lo = a < b;
                const int qb = d.first + b;
                const size_t r = base + (size_t)(6 + pq) * 64;
                const size_t nvo = nb > 1 ? (pair_index(N, a_lo ? qa : qb, a_lo ? qb : qa) * M + seg) * 3 : 0;
#pragma unroll
                for (int e = 0; e < 3; ++e) pn[pb][e] = QGF(c.normals)[nvo + e];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    pxb[pb][k] = QGC(c.ctrl)[((size_t)qb * 3 + k) * oq + j6];
                    pfa[pb][k] = need_da ? QGC(w.dxa)[((size_t)b * 3 + k) * oq + j6] : 0.0;
                    pfd[pb][k] = need_dd ? QGC(w.dx)[((size_t)b * 3 + k) * oq + j6] : 0.0;
                }
                prs[pb] = QGC(c.radius)[qa] + QGC(c.radius)[qb];
                pps[pb] = QGC(w.s)[r], ppz[pb] = QGC(w.z)[r];
            }
#pragma unroll
            for (int pb = 0; pb < 3; ++pb)
                if (pb < nb - 1)
                    pair_row(std::true_type{}, pb, pn[pb][0], pn[pb][1], pn[pb][2], pxb[pb], pfa[pb], pfd[pb], prs[pb], pps[pb], ppz[pb]);
        } else {
            for (int pb = 0; pb < nb - 1; ++pb) {
                const int b = pb < a ? pb : pb + 1;
                const bool a_lo = a < b;
                const int qb = d.first + b;
                const float* nv = c.normals + (pair_index(N, a_lo ? qa : qb, a_lo ? qb : qa) * M + seg) * 3;
                const double n0 = nv[0], n1 = nv[1], n2 = nv[2];
                double xb[3], fa[3] = {0, 0, 0}, fd[3] = {0, 0, 0};
#pragma unroll
                for (int k = 0; k < 3; ++k) xb[k] = c.ctrl[((size_t)qb * 3 + k) * oq + j6];
                const double rsum = c.radius[qa] + c.radius[qb];
                if (need_da) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) fa[k] = w.dxa[((size_t)b * 3 + k) * oq + j6];
                }
                if (need_dd) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) fd[k] = w.dx[((size_t)b * 3 + k) * oq + j6];
                }
                pair_row(std::false_type{}, pb, n0, n1, n2, xb, fa, fd, rsum, 0.0, 0.0);
            }
        }
        // ---- frozen neighbours that survived the presolve (rows implied by the SFC box of this segment are dropped): a stream
        // over the SELL arrays; the signed normal is shared by the six rows of the group
        // PRESOLVE / VERIFY / CAND_GEO see every row; the passes of the interior-point loop the near ones (the near rows come first in a
        // group's list); CAND walks all of them to clear the far rows' candidate marks
        if constexpr (blk_pass) {
        // Under load a trip to memory takes 3-5 us and a row's arithmetic 0.1: a thread that loads a row, works on it and stores it pays the
        // trip once per row (the loads of the next row cannot move above the stores of this one, and the compiler drains the memory counter
        // wherever a loop-carried load is used).  So the stream runs in BLOCKS: the (s, z), constant and normal of the NEXT QP_ROW_BLK rows
        // are requested before the current block is worked on, and first touched -- copied -- after it: one trip per block, overlapped with
        // the block's arithmetic.  Rows past the end re-read the last row (same cache lines) and are not used.  Same rows, same order, same
        // arithmetic per row as the plain loop.
        constexpr bool rd_sz = pass_reads_sz(PASS);
        constexpr int B = BB;
        if (cnt > 0) {
            double ns[B], nz[B], nh[B];
            float nn[B][3];
            for (int i0 = 0; i0 < cnt; i0 += B) {
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    const int ix = i0 + B + u < cnt ? i0 + B + u : cnt - 1;
                    const size_t rx = r0 + (size_t)ix * 64;
                    ns[u] = rd_sz ? QGC(w.s)[rx] : 0.0, nz[u] = rd_sz ? QGC(w.z)[rx] : 0.0, nh[u] = QGC(w.rh)[rx];
#pragma unroll
                    for (int e = 0; e < 3; ++e) nn[u][e] = QGF(nr)[3 * ix + e];
                }
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    const int idx = i0 + u;
                    if (idx < cnt) {
                        const size_t r = r0 + (size_t)idx * 64;
                        if (PASS == PASS_CAND && idx >= cnt_near) {  // a far row: no (s, z); not a candidate unless a verification finds it violated
                            QG(w.cc)[r] = 0.0;
                        } else {
                            const double n0 = cn[u][0], n1 = cn[u][1], n2 = cn[u][2];
                            const double slack = ch[u] - (n0 * xa[0] + n1 * xa[1] + n2 * xa[2]);
                            double wgt = 0, v = 0, zo = 0;
                            row_op<PASS, rd_sz>(slack, n0 * da[0] + n1 * da[1] + n2 * da[2], n0 * dd[0] + n1 * dd[1] + n2 * dd[2], r, w, io, 1.0, wgt, v, zo, cs[u], cz[u]);
                            if (cand && wgt != 0) emit_cand(d, w, *c.pw, r, j6, a, -1, n0, n1, n2, slack, -1, 0.0, wgt);
                            accumulate(wgt, v, zo, 1.0, n0, n1, n2);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    cs[u] = ns[u], cz[u] = nz[u], ch[u] = nh[u];
#pragma unroll
                    for (int e = 0; e < 3; ++e) cn[u][e] = nn[u][e];
                }
            }
        }
        } else {
#if QP_ROW_PF > 0
        // Under load the stream is bound by the memory operations in flight per thread, and unrolling the (heavy) row arithmetic to get
        // more of them costs registers and instruction cache (unroll 4 measured 8 % slower than 2).  A prefetch ring decouples the two:
        // the loads of row idx + QP_ROW_PF -- (s, z), the row constant, the group normal: nine registers -- are issued while row idx is
        // worked on, the arithmetic is not replicated.
        constexpr bool rd_sz = pass_reads_sz(PASS);
        double ps[QP_ROW_PF], pz[QP_ROW_PF], ph[QP_ROW_PF];
        float pn[QP_ROW_PF][3];
#pragma unroll
        for (int u = 0; u < QP_ROW_PF; ++u) {
            const int iu = u < cnt ? u : (cnt > 0 ? cnt - 1 : 0);
            const size_t ru = r0 + (size_t)iu * 64;
            ps[u] = (rd_sz && cnt > 0) ? w.s[ru] : 0.0, pz[u] = (rd_sz && cnt > 0) ? w.z[ru] : 0.0, ph[u] = cnt > 0 ? w.rh[ru] : 0.0;
#pragma unroll
            for (int e = 0; e < 3; ++e) pn[u][e] = cnt > 0 ? nr[3 * iu + e] : 0.0f;
        }
        for (int idx = 0; idx < cnt; ++idx) {
            const size_t r = r0 + (size_t)idx * 64;
            const bool far_row = PASS == PASS_CAND && idx >= cnt_near;
            const double n0 = pn[0][0], n1 = pn[0][1], n2 = pn[0][2], rhv = ph[0], s_in = ps[0], z_in = pz[0];
#pragma unroll
            for (int u = 0; u + 1 < QP_ROW_PF; ++u) {
                ps[u] = ps[u + 1], pz[u] = pz[u + 1], ph[u] = ph[u + 1];
#pragma unroll
                for (int e = 0; e < 3; ++e) pn[u][e] = pn[u + 1][e];
            }
            {
                const int ix = idx + QP_ROW_PF < cnt ? idx + QP_ROW_PF : cnt - 1;  // (past the end: the last row again, never used)
                const size_t rx = r0 + (size_t)ix * 64;
                if (rd_sz) ps[QP_ROW_PF - 1] = w.s[rx], pz[QP_ROW_PF - 1] = w.z[rx];
                ph[QP_ROW_PF - 1] = w.rh[rx];
#pragma unroll
                for (int e = 0; e < 3; ++e) pn[QP_ROW_PF - 1][e] = nr[3 * ix + e];
            }
            if (far_row) {  // (see the plain loop below)
                w.cc[r] = 0.0;
                continue;
            }
            const double slack = rhv - (n0 * xa[0] + n1 * xa[1] + n2 * xa[2]);
            double wgt = 0, v = 0, zo = 0;
            row_op<PASS, rd_sz>(slack, n0 * da[0] + n1 * da[1] + n2 * da[2], n0 * dd[0] + n1 * dd[1] + n2 * dd[2], r, w, io, 1.0, wgt, v, zo, s_in, z_in);
            if (cand && wgt != 0) emit_cand(d, w, *c.pw, r, j6, a, -1, n0, n1, n2, slack, -1, 0.0, wgt);
            accumulate(wgt, v, zo, 1.0, n0, n1, n2);
        }
#else
#pragma unroll QP_ROW_UNROLL
        for (int idx = 0; idx < cnt; ++idx) {
            const size_t r = r0 + (size_t)idx * 64;
            if (PASS == PASS_CAND && idx >= cnt_near) {  // a far row: no (s, z); not a candidate unless a verification finds it violated
                w.cc[r] = 0.0;
                continue;
            }
            const double n0 = nr[3 * idx], n1 = nr[3 * idx + 1], n2 = nr[3 * idx + 2];
            const double slack = w.rh[r] - (n0 * xa[0] + n1 * xa[1] + n2 * xa[2]);
            double wgt = 0, v = 0, zo = 0;
            row_op<PASS>(slack, n0 * da[0] + n1 * da[1] + n2 * da[2], n0 * dd[0] + n1 * dd[1] + n2 * dd[2], r, w, io, 1.0, wgt, v, zo);
            if (cand && wgt != 0) emit_cand(d, w, *c.pw, r, j6, a, -1, n0, n1, n2, slack, -1, 0.0, wgt);
            accumulate(wgt, v, zo, 1.0, n0, n1, n2);
        }
#endif
        }
        if (accum) {
            double* acc = w.cpacc + it;
#pragma unroll
            for (int e = 0; e < 6; ++e) acc[(size_t)e * ncp] = S[e];
            if (build) {
#pragma unroll
                for (int e = 0; e < 3; ++e) acc[(size_t)(6 + e) * ncp] = yv[e], acc[(size_t)(9 + e) * ncp] = gz[e];
            }
        }
    }
}

// A sweep of the interior-point loop: a stand-alone function (own register allocation, +3 %) that reads the row context from an LDS
// copy made once per batch QP (passing the 500-byte struct by value would travel through scratch memory).
template <int PASS>
__device__ __noinline__ PassIO sweep(const RowCtx* cl, PassIO io) {
    row_pass<PASS>(*cl, io);
    return io;
}
#define SWEEP(PASS) io = sweep<PASS>(&c_lds, io)
