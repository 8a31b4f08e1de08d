// qp_newton.inc — the Newton system of an interior-point iteration: the maps between control space and reduced space (apply_FT, apply_F),
// its right-hand sides out of the sweeps' accumulators (rbase_from_acc, rhs_from_acc) and the assembly of the knot blocks (AsmArgs,
// assemble_item, assemble_knots_lds, fasm_fetch / fasm_tiles, assemble_blocks_lds, assemble_blocks).  Included by qp.hip after qp_rows.inc,
// whose RowCtx it needs, and ahead of qp_wave_factor.inc, whose companion waves call the just-in-time assembly; from qp.hip the levers
// (QP_THREADS) and QG / QGC; QpDims, QpWs, uni (qp_base.inc); kl_lds, kl_sync, KL_LD (knot_lds.inc).

// ------------------------------------------------------------------------------------------------------------
// control-space <-> reduced-space maps
// ------------------------------------------------------------------------------------------------------------
// cvec[a][k][j6] (control space)  ->  out[(j-1)*nk + (a*3+k)*3 + e] = (F' cvec)
__device__ void apply_FT(const QpDims& d, const QpWs& w, const double* cvec, double* out, double scale) {
    const int oq = d.oq, nu = 3 * d.nb;
    for (int it = threadIdx.x; it < d.nj * nu; it += QP_THREADS) {
        const int j = it / nu + 1, u = it % nu;
        const double* xr = cvec + (size_t)u * oq + 6 * j;
        const double* xl = cvec + (size_t)u * oq + 6 * (j - 1) + 3;
        const double* L = w.Lk + 9 * j;
#pragma unroll
        for (int e = 0; e < 3; ++e)
            out[(size_t)(j - 1) * d.nk + u * 3 + e] = scale * (xr[e] + L[0 + e] * xl[0] + L[3 + e] * xl[1] + L[6 + e] * xl[2]);
    }
}
// dx[a][k][j6] = F du   (pinned control points get 0).  One work item per (knot, agent, dim): its three reduced values feed the six
// control points around the knot -- 420 items with a dozen independent loads each for a batch of four, two rounds of the workgroup,
// where a loop over the 2592 control-space entries was ten rounds of one load-wait-store each (~1 us per round under load).
__device__ void apply_F(const QpDims& d, const QpWs& w, const double* du, double* dx) {
    const int oq = d.oq, nu = 3 * d.nb;
    for (int it = threadIdx.x; it < d.nj * nu; it += QP_THREADS) {
        const int j = it / nu + 1, u = it % nu;
        const double* uu = du + (size_t)(j - 1) * d.nk + u * 3;
        const double* L = w.Lk + 9 * j;
        const double u0 = uu[0], u1 = uu[1], u2 = uu[2];
        double* o = dx + (size_t)u * oq + 6 * (j - 1) + 3;  // control points 6(j-1)+3 .. 6j+2
        o[0] = L[0] * u0 + L[1] * u1 + L[2] * u2;
        o[1] = L[3] * u0 + L[4] * u1 + L[5] * u2;
        o[2] = L[6] * u0 + L[7] * u1 + L[8] * u2;
        o[3] = u0, o[4] = u1, o[5] = u2;
    }
    for (int it = threadIdx.x; it < nu * 6; it += QP_THREADS) {  // the pinned ends
        const int u = it / 6, q = it % 6;
        dx[(size_t)u * oq + (q < 3 ? q : oq - 6 + q)] = 0.0;
    }
}

// rbase = -F'(2Qx + G'z) in one pass (grad_ctrl + apply_FT fused, as in rhs_from_acc below); also returns this thread's
// share of max|rbase| and max|2Qx + G'z| for the dual-residual test
// with_rhs (uniform): the predictor's right-hand side in the same pass -- rhs = rbase + F'(G'v), rhs_from_acc(c, false, 0)'s expression on the
// value this thread has just stored, where that function walks the same items with the same thread map and reads the store back.  Both
// inputs exist once the build sweep is done.  The corrector still reads rbase.
// 256-thread build: two items per thread and round, the operands of both requested before the first is worked on: a batch of four has
// 35 * 12 = 420 items for 256 threads, and the second round's loads cannot move above the first round's stores -- one trip to memory
// per iteration instead of two.  Same items per thread, same order, same arithmetic per item.
struct RbaseItem {
    double x[12], gz[6], yv[6], sc[2], L[9];  // control points of the two segments at the knot, G'z and G'v at its six points, segsc, L_j
};
__device__ void rbase_from_acc(const RowCtx& c, double& dmax, double& gmax, bool with_rhs) {
    const QpDims& d = c.d;
    const QpWs& w = c.w;
    const int oq = d.oq, nu = 3 * d.nb, nit = d.nj * nu;
    dmax = gmax = 0;
    auto load = [&](int it, RbaseItem& t) {
        const int j = it / nu + 1, u = it % nu, a = u / 3, k = u % 3;
        const double* xs = c.ctrl + ((size_t)(d.first + a) * 3 + k) * oq + 6 * (j - 1);  // segments j - 1 and j
#pragma unroll
        for (int q = 0; q < 12; ++q) t.x[q] = xs[q];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int j6 = 6 * (j - 1) + 3 + q;
            t.gz[q] = w.cpacc[(size_t)(9 + k) * (d.nb * oq) + (size_t)a * oq + j6];  // G'z of ALL rows of this control point (bounds, pairs, frozen)
            t.yv[q] = with_rhs ? w.cpacc[(size_t)(6 + k) * (d.nb * oq) + (size_t)a * oq + j6] : 0.0;  // G'v at the same six control points
        }
        t.sc[0] = w.segsc[j - 1], t.sc[1] = w.segsc[j];
#pragma unroll
        for (int e = 0; e < 9; ++e) t.L[e] = w.Lk[9 * j + e];
    };
    auto work = [&](int it, const RbaseItem& t) {
        const int j = it / nu + 1, u = it % nu;
        double g[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int i = (3 + q) % 6, ms = (3 + q) / 6;  // control point 6 (j - 1) + 3 + q: point i of segment j - 1 + ms
            double gv = 0;
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) gv += Qbase[6 * i + jj] * t.x[6 * ms + jj];
            gv *= 2 * t.sc[ms];
            gv += t.gz[q];
            g[q] = -gv;
            gmax = fmax(gmax, fabs(gv));
        }
        const double* L = t.L;
        const size_t o0 = (size_t)(j - 1) * d.nk + u * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const double r = g[3 + e] + L[0 + e] * g[0] + L[3 + e] * g[1] + L[6 + e] * g[2];
            w.rbase[o0 + e] = r;
            dmax = fmax(dmax, fabs(r));
            if (with_rhs) w.rhs[o0 + e] = r + t.yv[3 + e] + L[0 + e] * t.yv[0] + L[3 + e] * t.yv[1] + L[6 + e] * t.yv[2];
        }
    };
    // (the 512-thread build has a thread per item of a batch of four up to M = 43: it keeps one item per round)
    constexpr int NI = QP_THREADS >= 512 ? 1 : 2;
    for (int it = threadIdx.x; it < nit; it += NI * QP_THREADS) {
        RbaseItem t[NI];
#pragma unroll
        for (int q = 0; q < NI; ++q) load(it + q * QP_THREADS < nit ? it + q * QP_THREADS : it, t[q]);  // (past the end: the first item again, not worked on)
#pragma unroll
        for (int q = 0; q < NI; ++q)
            if (it + q * QP_THREADS < nit) work(it + q * QP_THREADS, t[q]);
    }
}
// rhs = rbase + F'(G'v) in one pass: gtv_ctrl + apply_FT + the add fused (every control-space entry of G'v is used by
// exactly one reduced-space entry, so nothing is computed twice and two barriers and the cvec round trip disappear)
__device__ void rhs_from_acc(const RowCtx& c, bool corrector, double sigma_mu) {
    const QpDims& d = c.d;
    const QpWs& w = c.w;
    const int oq = d.oq, nu = 3 * d.nb;
    for (int it = threadIdx.x; it < d.nj * nu; it += QP_THREADS) {
        const int j = it / nu + 1, u = it % nu, a = u / 3, k = u % 3;
        double g[6];  // G'v at control points 6(j-1)+3 .. 6j+2 of (agent a, dim k)
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int j6 = 6 * (j - 1) + 3 + q;
            const double* ac = w.cpacc + (size_t)a * oq + j6;
            const size_t ncp = (size_t)d.nb * oq;
            const double gv = corrector ? ac[k * ncp] - sigma_mu * ac[(3 + k) * ncp] : ac[(6 + k) * ncp];
            g[q] = gv;
        }
        const double* L = w.Lk + 9 * j;
        const size_t o0 = (size_t)(j - 1) * d.nk + u * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) w.rhs[o0 + e] = w.rbase[o0 + e] + g[3 + e] + L[0 + e] * g[0] + L[3 + e] * g[1] + L[6 + e] * g[2];
    }
}

// ------------------------------------------------------------------------------------------------------------
// knot blocks:  T_j = blockdiag(D_j) + sum_p S_p (x) t_p t_p',   T_{j+1,j} = blockdiag(E_j')
// ------------------------------------------------------------------------------------------------------------
__device__ inline double sym3s(const double* S, size_t stride, int k, int l) {  // the same on a component-major array
    const int a = k < l ? k : l, b = k < l ? l : k;
    return S[(size_t)(a == 0 ? b : (a == 1 ? 2 + b : 5)) * stride];
}
__device__ inline double sym3(const double* S, int k, int l) {
    const int a = k < l ? k : l, b = k < l ? l : k;
    return S[a == 0 ? b : (a == 1 ? 2 + b : 5)];
}

// what the assembly of a knot block needs (a by-value subset of the row context: usable from the stand-alone factor function)
struct AsmArgs {
    const double *cpacc, *pwgt, *Lk, *Dk;
    const float* normals;
    double* Td;
    int N, M, nb, first, oq, ldb;
};
// (arguments of a non-kernel function arrive in vector registers: see BlkArgs)
__device__ __forceinline__ AsmArgs uni(const AsmArgs& A) {
    return AsmArgs{uni(A.cpacc), uni(A.pwgt), uni(A.Lk), uni(A.Dk), uni(A.normals), uni(A.Td), uni(A.N), uni(A.M), uni(A.nb), uni(A.first), uni(A.oq), uni(A.ldb)};
}

// one work item of the block assembly = (knot j, agent a, agent b, dim k, dim l): six 3x3-accumulator entries in, one 3x3 (e,f)
// tile of T_j out.  r = ((a * nb + b) * 3 + k) * 3 + l.  Ssum: LDS copy of the per-control-point weight sums [nb*oq][6] or nullptr.
// Off-diagonal (a != b) blocks carry -wgt n n' of the pair row (a, b): the weight was left in pwgt by the sweep (8 bytes per
// row, one independent load -- not a stored 3x3, not a chain of index loads)
// lower_only (wave path): lane r of a factor chain loads T[k][r] for every k but only ever uses k <= r (T is symmetric, ldl_rows works
// on the lower triangle), so the other half is neither computed nor written: half of the assembly work and of T's write traffic.  (The
// chain still LOADS whole rows: predicating its 36 loads and stores costs the dependent chain more than the bytes are worth, measured.)
__device__ __forceinline__ void assemble_load(const AsmArgs& A, const double* Ssum, int j, int a, int b, int k, int l, double (&Sv)[6]) {
    const int nb = A.nb, oq = A.oq;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const int j6 = 6 * (j - 1) + 3 + p;
        double sv;
        if (a == b) {
            sv = Ssum ? sym3(Ssum + ((size_t)a * oq + j6) * 6, k, l) : sym3s(A.cpacc + (size_t)a * oq + j6, (size_t)nb * oq, k, l);
        } else {
            const int lo = a < b ? a : b, hi = a < b ? b : a, seg = j6 / 6;
            const float* nv = A.normals + (pair_index(A.N, A.first + lo, A.first + hi) * A.M + seg) * 3;
            sv = -A.pwgt[(size_t)(lo * nb - lo * (lo + 1) / 2 + (hi - lo - 1)) * oq + j6] * (double)nv[k] * (double)nv[l];
        }
        Sv[p] = sv;
    }
}
__device__ __forceinline__ void assemble_store(const AsmArgs& A, int j, int a, int b, int k, int l, const double (&Sv)[6], bool lower_only) {
    const int lb = A.ldb;
    const double* L = A.Lk + 9 * j;
    double* out = A.Td + (size_t)(j - 1) * lb * lb + (size_t)(a * 9 + k * 3) * lb + b * 9 + l * 3;
#pragma unroll
    for (int e = 0; e < 3; ++e)
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            double acc = Sv[0] * L[e] * L[f] + Sv[1] * L[3 + e] * L[3 + f] + Sv[2] * L[6 + e] * L[6 + f];
            if (e == f) acc += Sv[3 + e];
            if (a == b && k == l) acc += A.Dk[9 * j + 3 * e + f];
            if (!(lower_only && a == b && k == l && e > f)) out[(size_t)e * lb + f] = acc;
        }
}
__device__ __forceinline__ void assemble_item(const AsmArgs& A, const double* Ssum, int j, int r, bool lower_only = false) {
    const int nb = A.nb;
    const int a = r / (nb * 9), b = (r / 9) % nb, k = (r / 3) % 3, l = r % 3;
    if (lower_only && (a > b || (a == b && k > l))) return;
    double Sv[6];
    assemble_load(A, Ssum, j, a, b, k, l, Sv);
    assemble_store(A, j, a, b, k, l, Sv, lower_only);
}

// The knot blocks through the LDS, one wave per knot (r03): a knot's inputs -- the weight sums of its six control points for every batch agent,
// the pair weights, the pairs' normals of the two segments -- are fetched with coalesced loads into the wave's LDS scratch, the tiles are
// computed from there into a symmetric LDS image of the block, and the image leaves as whole rows (16 bytes per lane, 1 KB per store
// instruction).  Tile by tile from / to global memory a knot costs ~10^4 scattered 8-byte transactions, this way ~10^2 line requests --
// and under load the memory system is bound by transactions (see the row sweeps).  lds: QP_THREADS / 64 scratch areas of ASML_DOUBLES.
#define ASML_DOUBLES(nk, nb) ((nk) * KL_LD + (nb) * 36 + 3 * (nb) * ((nb) - 1) + 3 * (nb) * ((nb) - 1) + 8)
// One wave, a sequence of knots: next() returns the next knot (0-based) or -1, done(j) is called when T_j is on its way to global memory.
// scratch: ASML_DOUBLES(nk, nb) doubles of LDS of the wave's own.
// TO_GLOBAL = false: the block stays in the wave's scratch as a full symmetric image (rows KL_LD apart) for a reader in the same
// workgroup -- the 512-thread build's chains, see twisted_factor -- and next() must not return before that reader is done with the
// previous image.
template <bool TO_GLOBAL, class NextFn, class DoneFn>
__device__ __forceinline__ void assemble_knots_lds(const AsmArgs& A, double* scratch, NextFn next, DoneFn done) {
    const int nb = A.nb, oq = A.oq, nk = 9 * nb, npb = nb * (nb - 1) / 2, n3 = 3 * nb, per = n3 * (n3 + 1) / 2;
    const int lane = threadIdx.x & 63;
    const size_t ncp = (size_t)nb * oq;
    kl_lds* Timg = (kl_lds*)scratch;
    kl_lds* Sin = Timg + nk * KL_LD;  // [a][sym][p]
    kl_lds* Pw = Sin + nb * 36;      // [pair][p]
    kl_lds* Nr = Pw + 6 * npb;       // [pair][left / right segment][3]
    // this lane's tiles of a block's upper half (the same for every knot)
    int tA[2], tB[2], ntile = 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = lane + 64 * u, tc = t < per ? t : 0;
        int ai = (int)(((2 * n3 + 1) - sqrtf((float)((2 * n3 + 1) * (2 * n3 + 1) - 8 * tc))) * 0.5f);
        if (ai * n3 - ai * (ai - 1) / 2 > tc) ai--;
        if ((ai + 1) * n3 - (ai + 1) * ai / 2 <= tc) ai++;
        tA[u] = ai, tB[u] = ai + tc - (ai * n3 - ai * (ai - 1) / 2);
        if (t < per) ntile = u + 1;
    }
    const int row0 = (2 * lane) / nk, col0 = (2 * lane) % nk, drow = 128 / nk, dcol = 128 % nk;  // see the row copy below
    size_t nr_off = 0;  // this lane's entry of the pairs' normals (pair, left / right segment, component): the same for every knot
    if (lane < 6 * npb) {
        const int pw = lane / 6, sg = (lane / 3) % 2, c3 = lane % 3;
        int lo = 0, rest = pw;  // pair pw = (lo, hi) in the order lo * nb - lo (lo + 1) / 2 + (hi - lo - 1)
        while (rest >= nb - 1 - lo) rest -= nb - 1 - lo, lo++;
        const int hi = lo + 1 + rest;
        nr_off = (pair_index(A.N, A.first + lo, A.first + hi) * A.M + sg) * 3 + c3;
    }
    for (int j = next(); j >= 0; j = next()) {
        const int jn = j + 1, j60 = 6 * j + 3;  // first control point of the knot
        for (int idx = lane; idx < nb * 36; idx += 64) {
            const int a = idx / 36, e = (idx / 6) % 6, pp = idx % 6;
            Sin[idx] = A.cpacc[(size_t)e * ncp + (size_t)a * oq + j60 + pp];
        }
        for (int idx = lane; idx < 6 * npb; idx += 64) Pw[idx] = A.pwgt[(size_t)(idx / 6) * oq + j60 + idx % 6];
        if (lane < 6 * npb) Nr[lane] = (double)A.normals[nr_off + (size_t)j * 3];  // (6 npb <= 36: one entry per lane)
        double L[9], Dk[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) L[e] = A.Lk[9 * jn + e], Dk[e] = A.Dk[9 * jn + e];
        kl_sync();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u < ntile) {
                const int Ai = tA[u], Bi = tB[u], a = Ai / 3, k = Ai % 3, b = Bi / 3, l = Bi % 3;
                double Sv[6];
                if (a == b) {
                    const int kk = k < l ? k : l, ll = k < l ? l : k, sym = kk == 0 ? ll : (kk == 1 ? 2 + ll : 5);
#pragma unroll
                    for (int pp = 0; pp < 6; ++pp) Sv[pp] = Sin[(a * 6 + sym) * 6 + pp];
                } else {  // a < b
                    const int pw = a * nb - a * (a + 1) / 2 + (b - a - 1);
#pragma unroll
                    for (int pp = 0; pp < 6; ++pp) Sv[pp] = -Pw[pw * 6 + pp] * Nr[(pw * 2 + (pp >= 3)) * 3 + k] * Nr[(pw * 2 + (pp >= 3)) * 3 + l];
                }
#pragma unroll
                for (int e = 0; e < 3; ++e)
#pragma unroll
                    for (int f = 0; f < 3; ++f) {
                        double acc = Sv[0] * L[e] * L[f] + Sv[1] * L[3 + e] * L[3 + f] + Sv[2] * L[6 + e] * L[6 + f];
                        if (e == f) acc += Sv[3 + e];
                        if (Ai == Bi) acc += Dk[3 * e + f];
                        Timg[(3 * Ai + e) * KL_LD + 3 * Bi + f] = acc;
                        Timg[(3 * Bi + f) * KL_LD + 3 * Ai + e] = acc;
                    }
            }
        }
        kl_sync();
        if (TO_GLOBAL) {
            double* Tg = A.Td + (size_t)j * nk * nk;
            if ((nk & 1) == 0) {
                // (the factorisation uses the entries (r, k >= r) only: knot_ldl.  Row and column of a lane's pair advance by 128 elements
                // per round: carried along, not divided out -- nk is not a compile-time constant here, and two integer divisions per pair
                // were more instructions than everything else in this loop)
                int r = row0, k2 = col0;
                for (int idx = lane; idx < nk * nk / 2; idx += 64) {
                    if (k2 + 1 >= r) *(kl_d2*)(Tg + 2 * idx) = *(const kl_lds2*)(Timg + r * KL_LD + k2);
                    r += drow, k2 += dcol;
                    if (k2 >= nk) k2 -= nk, r++;
                }
            } else {
                for (int idx = lane; idx < nk * nk; idx += 64) Tg[idx] = Timg[(idx / nk) * KL_LD + idx % nk];
            }
        }
        done(j);
        kl_sync();
    }
}
// ---- just-in-time assembly by the chains' companion waves (256-thread build, round 6; see twisted_factor ROLE 2) --------------------------
// Two out-of-line steps per block, so that the companion's column loop keeps its registers and its stack frame to itself:
//   fasm_fetch   the block's inputs -- weight sums of its six control points per batch agent, pair weights, the pairs' normals -- travel from
//                global memory into the wave's LDS scratch by global_load_lds (4 bytes per lane and instruction, no registers, nobody waits):
//                issued right after the PREVIOUS block's tiles, they land while the companion follows that block's factorisation;
//   fasm_tiles   the 3 x 3 tiles from the LDS inputs into the symmetric LDS image the chain reads (the arithmetic of assemble_knots_lds).
// Scratch layout as in assemble_knots_lds (image | Sin | Pw | Nr), except that Nr holds the normals as the floats they are.
__device__ __noinline__ void fasm_fetch(AsmArgs Av, double* scratch_v, int jv) {
    typedef __attribute__((address_space(1))) const void gvoid;
    typedef __attribute__((address_space(3))) void lvoid;
    typedef __attribute__((address_space(3))) char lchar;
    const AsmArgs A = uni(Av);
    double* scratch = uni(scratch_v);
    const int j = __builtin_amdgcn_readfirstlane(jv);
    const int nb = A.nb, oq = A.oq, nk = 9 * nb, npb = nb * (nb - 1) / 2, lane = threadIdx.x & 63, j60 = 6 * j + 3;
    const size_t ncp = (size_t)nb * oq;
    lchar* Sin = (lchar*)((kl_lds*)scratch + nk * KL_LD);
    lchar* Pw = Sin + (size_t)nb * 36 * 8;
    lchar* Nr = Pw + (size_t)6 * npb * 8;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the previous block's tiles have read their inputs)
    for (int c = 0; c * 64 < nb * 72; ++c) {  // Sin[a][sym][p], 8 bytes each, as dwords
        const int dw = c * 64 + lane, idx = dw >> 1, a = idx / 36, e = (idx / 6) % 6, pp = idx % 6;
        if (dw < nb * 72)
            __builtin_amdgcn_global_load_lds((gvoid*)((const unsigned*)(A.cpacc + (size_t)e * ncp + (size_t)a * oq + j60 + pp) + (dw & 1)), (lvoid*)(Sin + c * 256), 4, 0, 0);
    }
    for (int c = 0; c * 64 < npb * 12; ++c) {  // Pw[pair][p]
        const int dw = c * 64 + lane, idx = dw >> 1;
        if (dw < npb * 12)
            __builtin_amdgcn_global_load_lds((gvoid*)((const unsigned*)(A.pwgt + (size_t)(idx / 6) * oq + j60 + idx % 6) + (dw & 1)), (lvoid*)(Pw + c * 256), 4, 0, 0);
    }
    if (lane < 6 * npb) {  // Nr[pair][left / right segment][3] (floats)
        const int pw = lane / 6, sg = (lane / 3) % 2, c3 = lane % 3;
        int lo = 0, rest = pw;  // pair pw = (lo, hi) in the order lo * nb - lo (lo + 1) / 2 + (hi - lo - 1)
        while (rest >= nb - 1 - lo) rest -= nb - 1 - lo, lo++;
        const int hi = lo + 1 + rest;
        const size_t off = (pair_index(A.N, A.first + lo, A.first + hi) * A.M + sg + j) * 3 + c3;
        __builtin_amdgcn_global_load_lds((gvoid*)(A.normals + off), (lvoid*)Nr, 4, 0, 0);
    }
}
__device__ __noinline__ void fasm_tiles(AsmArgs Av, double* scratch_v, int jv) {
    const AsmArgs A = uni(Av);
    double* scratch = uni(scratch_v);
    const int j = __builtin_amdgcn_readfirstlane(jv);
    const int nb = A.nb, nk = 9 * nb, npb = nb * (nb - 1) / 2, n3 = 3 * nb, per = n3 * (n3 + 1) / 2, lane = threadIdx.x & 63, jn = j + 1;
    kl_lds* Timg = (kl_lds*)scratch;
    const kl_lds* Sin = Timg + nk * KL_LD;
    const kl_lds* Pw = Sin + nb * 36;
    const __attribute__((address_space(3))) float* Nr = (const __attribute__((address_space(3))) float*)(Pw + 6 * npb);
    double L[9], Dk[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) L[e] = A.Lk[9 * jn + e], Dk[e] = A.Dk[9 * jn + e];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the inputs have landed (fasm_fetch was issued a block ago: nothing to wait for)
    kl_sync();
    for (int u = 0; u * 64 < per; ++u) {
        const int t = lane + 64 * u;
        if (t < per) {
            int Ai = (int)(((2 * n3 + 1) - sqrtf((float)((2 * n3 + 1) * (2 * n3 + 1) - 8 * t))) * 0.5f);
            if (Ai * n3 - Ai * (Ai - 1) / 2 > t) Ai--;
            if ((Ai + 1) * n3 - (Ai + 1) * Ai / 2 <= t) Ai++;
            const int Bi = Ai + t - (Ai * n3 - Ai * (Ai - 1) / 2);
            const int a = Ai / 3, k = Ai % 3, b = Bi / 3, l = Bi % 3;
            double Sv[6];
            if (a == b) {
                const int kk = k < l ? k : l, ll = k < l ? l : k, sym = kk == 0 ? ll : (kk == 1 ? 2 + ll : 5);
#pragma unroll
                for (int pp = 0; pp < 6; ++pp) Sv[pp] = Sin[(a * 6 + sym) * 6 + pp];
            } else {  // a < b
                const int pw = a * nb - a * (a + 1) / 2 + (b - a - 1);
#pragma unroll
                for (int pp = 0; pp < 6; ++pp)
                    Sv[pp] = -Pw[pw * 6 + pp] * (double)Nr[(pw * 2 + (pp >= 3)) * 3 + k] * (double)Nr[(pw * 2 + (pp >= 3)) * 3 + l];
            }
#pragma unroll
            for (int e = 0; e < 3; ++e)
#pragma unroll
                for (int f = 0; f < 3; ++f) {
                    double acc = Sv[0] * L[e] * L[f] + Sv[1] * L[3 + e] * L[3 + f] + Sv[2] * L[6 + e] * L[6 + f];
                    if (e == f) acc += Sv[3 + e];
                    if (Ai == Bi) acc += Dk[3 * e + f];
                    Timg[(3 * Ai + e) * KL_LD + 3 * Bi + f] = acc;
                    Timg[(3 * Bi + f) * KL_LD + 3 * Ai + e] = acc;
                }
        }
    }
    kl_sync();
}
// all knots up front, one wave per knot in turn (256-thread build).  lds: QP_THREADS / 64 scratch areas.
__device__ void assemble_blocks_lds(const AsmArgs& A, int nj, double* lds) {
    const int wave = threadIdx.x >> 6, NW = QP_THREADS / 64;
    int j = wave - NW;
    assemble_knots_lds<true>(A, lds + (size_t)wave * ASML_DOUBLES(9 * A.nb, A.nb), [&] { j += NW; return j < nj ? j : -1; }, [](int) {});
}

__device__ inline AsmArgs asm_args(const RowCtx& c) {
    return AsmArgs{c.w.cpacc, c.w.pwgt, c.w.Lk, c.w.Dk, c.normals, c.w.Td, c.d.N, c.d.M, c.d.nb, c.d.first, c.d.oq, c.d.ldb};
}

// whole-workgroup assembly of all knot blocks (tiled path; the wave path assembles block by block BEHIND the factorisation
// chains, see twisted_factor)
__device__ void assemble_blocks(const RowCtx& c, double* lds) {
    const QpDims& d = c.d;
    const QpWs& w = c.w;
    const int nk = d.nk, oq = d.oq, nb = d.nb, lb = d.ldb;
    const AsmArgs A = asm_args(c);
    // stage 1: per (agent, control point) the 3x3 weight sum of ALL its rows (bounds, in-batch pairs, frozen neighbours) as the
    // sweep left it in cpacc, parked in LDS when it fits (every entry is read by nine (k, l) work items)
    const bool in_lds = nb * oq * 6 <= c.lds_avail;
    if (in_lds) {
        for (int it = threadIdx.x; it < nb * oq * 6; it += QP_THREADS) lds[it] = w.cpacc[(size_t)(it % 6) * (nb * oq) + it / 6];
        __syncthreads();
    }
    const int per_knot = nb * nb * 9;
    for (int it = threadIdx.x; it < d.nj * per_knot; it += QP_THREADS) assemble_item(A, in_lds ? lds : nullptr, it / per_knot + 1, it % per_knot);
    // the wave-register path and the LDS-resident tiled path build their coupling blocks from Ek directly
    if (d.nj > 1 && nk > 36 && 3 * lb * (lb + 2) > c.lds_avail) {
        const size_t noff = (size_t)(d.nj - 1) * lb * lb;
        for (size_t it = threadIdx.x; it < noff; it += QP_THREADS) {
            const int j = (int)(it / ((size_t)lb * lb)) + 1;  // couples knot j (cols) and j+1 (rows)
            const int rr = (int)(it % ((size_t)lb * lb)) / lb, cc = (int)(it % ((size_t)lb * lb)) % lb;
            double v = 0;
            if (rr / 3 == cc / 3 && rr < nk && cc < nk) v = w.Ek[9 * j + 3 * (cc % 3) + (rr % 3)];  // E_j' : rows u_{j+1}, cols u_j
            w.To[it] = v;
        }
    }
}
