// qp_polish.inc — active-set polish ("crossover") of the interior-point answer: the algorithms.  Included by qp.hip, once, behind
// qp_entries.inc; needs its records (qp_polish_types.inc), uni, uni_words (qp_base.inc), row_pass (qp_rows.inc) and apply_F, apply_FT (qp_newton.inc).
//
// Same mathematics as the CPU checker's polish, re-implemented for one workgroup (DESIGN.md "Polish"):
//   candidates C  = rows with dominant multiplier or slack < 1e-6 at the interior-point iterate
//   K0            = reduced Hessian F'(2Q)F (block tridiagonal, no barrier terms; the same for every agent and dim), factorised and
//                   inverted once per MISSION (k0_mission_tables): it depends on the segment times alone
//   v0            = K0^{-1} g              one thread per (agent, dim) 3x3-block chain, solved with the mission's factor (only d needs it)
//   dual QP       min 1/2 z'Sz - d'z, z >= 0 with S = J_C K0^{-1} J_C', d = -J_C v0 - slack_C   -> Lawson-Hanson in wave 0
//                   (S from the 3x3 blocks of the mission's table G = K0^{-1}: a row touches one knot; no column of K0^{-1} J_C' is formed)
//   x_new         = x - F K0^{-1} (g + J_P' z): the sum first, then ONE product with G; refined against the actual residuals of the active rows
// The result is taken only if it satisfies the KKT conditions of the full QP (every row feasible to 1e-9, all
// multipliers >= 0); otherwise the interior-point answer stands.  It removes the O(sqrt(mu)) bias of the
// interior-point answer in the weakly curved directions (reduced-Hessian condition number ~1e9).

// which (agent, dim) subsystems of K0 a candidate row lives in: agents a | (b + 1) << 8, dims << 16
__device__ __forceinline__ int cand_meta(const Cand& c) {
    return c.a | ((c.b + 1) << 8) | ((c.n[0] != 0.0) << 16) | ((c.n[1] != 0.0) << 17) | ((c.n[2] != 0.0) << 18);
}
// sign of the row's coefficient on (agent, dim k): +1 the row's own agent, -1 the other agent of a pair row, 0 not in the row
__device__ __forceinline__ int meta_sign(int meta, int agent, int k) {
    if (!(((meta >> 16) >> k) & 1)) return 0;
    return agent == (meta & 255) ? 1 : (agent == ((meta >> 8) & 255) - 1 ? -1 : 0);
}
// g_c . vec  for a reduced vector vec[(knot-1)*nk + (agent*3+k)*3 + e]
__device__ __forceinline__ double cand_dot(const Cand& c, const double* vec, int nk) {
    const double* blk = vec + (size_t)(c.knot - 1) * nk;
    double s = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (c.n[k] == 0.0) continue;
        const double* pa = blk + (c.a * 3 + k) * 3;
        double ta = c.t[0] * pa[0] + c.t[1] * pa[1] + c.t[2] * pa[2];
        if (c.b >= 0) {
            const double* pb = blk + (c.b * 3 + k) * 3;
            ta -= c.t[0] * pb[0] + c.t[1] * pb[1] + c.t[2] * pb[2];
        }
        s += c.n[k] * ta;
    }
    return s;
}

// K0 = F'(2Q)F does not couple agents or dimensions: for every (agent, dim) it is the SAME block-tridiagonal matrix
// with 3x3 blocks  D_j = Dk[j]  and  T_{j+1,j} = Ek[j]'  (assemble_blocks without the barrier terms), and Dk, Ek come from the mission's
// segment times alone.  So it is factorised and inverted ONCE per mission, here, and not in every polish:
//   fd[jj*18 + 0..8]  = L_jj (lower, row-major),  fd[jj*18 + 9..17] = B_jj = T_{jj+1,jj} L_jj^{-T}     (k0_factor_step in dd, one thread's chain)
//   G = K0^-1, lower block triangle, one thread per unit column (k0_inverse_column), then symmetrised
// A candidate row touches one knot with three coefficients t per (agent, dim) it involves, so every product of K0^-1 with candidate rows
// -- S = J K0^-1 J', the primal step K0^-1 J_P' z -- is a contraction of t's with 3x3 blocks of G, and the gradient column K0^-1 g is a
// product of the table with g + J_P' z: no column of K0^-1 J' is ever formed.  The one solve left is the gradient column v0 = K0^-1 g (for
// d = -J v0 - slack), with the factor in double that is kept beside the table (k0f).
// (The primal step multiplies the table with the SUM g + J_P' z, which is nearly zero at the interior-point iterate, never with its two
// parts one after the other: a product with an explicit inverse of condition number 1e10 is only good to eps |G| |g| ~ 1e-6 m, and the
// two large parts do not share that error.  Measured: v0 from the solve or from the table and the rows' part from the table, added up
// afterwards, left control points 3e-6 m off the certified optimum on some of the 50 maps, where 2e-6 is the test's tolerance.)
// lds: 54 nj doubles (both factors).  pw.Sg holds the table's low halves between the two passes (no batch QP is running yet).
__device__ void k0_mission_tables(int nj, const QpWs& w, const PolishWs& pw, double* lds) {
    double* f3 = lds;               // the factor in double, as the polish's k0_solve3 wants it
    dd* fd = (dd*)(lds + 18 * nj);  // the factor in dd, for the table
    for (int it = threadIdx.x; it < 18 * nj; it += QP_THREADS) {
        const int jj = it / 18, e = it % 18, j = jj + 1;
        const double v = e < 9 ? w.Dk[9 * j + e] : (jj + 1 < nj ? w.Ek[9 * j + (e - 9)] : 0.0);
        f3[it] = v, fd[it] = dd(v);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int ok = 1;
        double Bp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int jj = 0; jj < nj; ++jj)
            if (!k0_factor_step(f3 + 18 * jj, Bp, jj == 0)) ok = 0;
        *(int*)(pw.k0f + 18 * (size_t)nj) = !ok;
    }
    if (threadIdx.x == 64) {  // (a wave of its own: the two chains run side by side)
        int ok = 1;
        dd Bd[9];
        for (int jj = 0; jj < nj; ++jj)
            if (!k0_factor_step(fd + 18 * jj, Bd, jj == 0)) ok = 0;
        *((int*)(pw.k0f + 18 * (size_t)nj) + 1) = !ok;  // (the polish looks at both words)
    }
    __syncthreads();
    for (int it = threadIdx.x; it < 18 * nj; it += QP_THREADS) pw.k0f[it] = f3[it];
    for (int col = threadIdx.x; col < 3 * nj; col += QP_THREADS) k0_inverse_column((const dd*)fd, nj, col / 3, col % 3, pw.G, pw.Sg);
    __threadfence_block();
    __syncthreads();
    for (int jj = threadIdx.x; jj < nj; jj += QP_THREADS) k0g_symmetrise(pw.G + k0g_block(jj, jj));
}

// one (column, agent*3+dim) subsystem:  y <- K0^{-1} y,  y_j at col[jj*nk + sub*3 + e]
// (round 6) The column lives in global memory and the recurrence walks it knot by knot, forward and back: written as load - compute - store
// per knot, every one of the 2 nj steps paid a trip to memory (the next knot's load may not pass this knot's store), 70 trips of 3-5 us under
// load for a few dozen multiply-adds each.  Now the knots travel in BLOCKS of K0_BLK: the next block is requested before the current one is
// worked on (second register set, first touched after the block), results leave per block -- a dozen trips.  Same arithmetic, same order.
__device__ __forceinline__ void k0_solve3(const double* f3g, int nj, int nk, double* col, int sub) {
    typedef __attribute__((address_space(1))) double gdb;
    const kl_lds* f3 = (const kl_lds*)f3g;  // (the factor is in LDS)
    gdb* y = QG(col) + sub * 3;
    constexpr int B = K0_BLK;
    double cur[B][3], nxt[B][3];
    double p[3] = {0, 0, 0};
#pragma unroll
    for (int u = 0; u < B; ++u) {
        const int jx = u < nj ? u : nj - 1;
#pragma unroll
        for (int e = 0; e < 3; ++e) cur[u][e] = y[(size_t)jx * nk + e];
    }
    for (int j0 = 0; j0 < nj; j0 += B) {
#pragma unroll
        for (int u = 0; u < B; ++u) {
            const int jx = j0 + B + u < nj ? j0 + B + u : nj - 1;
#pragma unroll
            for (int e = 0; e < 3; ++e) nxt[u][e] = y[(size_t)jx * nk + e];
        }
#pragma unroll
        for (int u = 0; u < B; ++u) {
            const int jj = j0 + u;
            if (jj < nj) {
                k0_forward_step(f3 + 18 * jj, jj > 0, cur[u], p);
                y[(size_t)jj * nk] = p[0] = cur[u][0], y[(size_t)jj * nk + 1] = p[1] = cur[u][1], y[(size_t)jj * nk + 2] = p[2] = cur[u][2];
            }
        }
#pragma unroll
        for (int u = 0; u < B; ++u)
#pragma unroll
            for (int e = 0; e < 3; ++e) cur[u][e] = nxt[u][e];
    }
    // backward, blocks from the last knot down (block u of a round = knot jtop - u)
#pragma unroll
    for (int u = 0; u < B; ++u) {
        const int jx = nj - 1 - u >= 0 ? nj - 1 - u : 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) cur[u][e] = y[(size_t)jx * nk + e];
    }
    for (int jt = nj - 1; jt >= 0; jt -= B) {
#pragma unroll
        for (int u = 0; u < B; ++u) {
            const int jx = jt - B - u >= 0 ? jt - B - u : 0;
#pragma unroll
            for (int e = 0; e < 3; ++e) nxt[u][e] = y[(size_t)jx * nk + e];
        }
#pragma unroll
        for (int u = 0; u < B; ++u) {
            const int jj = jt - u;
            if (jj >= 0) {
                k0_backward_step(f3 + 18 * jj, jj + 1 < nj, cur[u], p);
                y[(size_t)jj * nk] = p[0] = cur[u][0], y[(size_t)jj * nk + 1] = p[1] = cur[u][1], y[(size_t)jj * nk + 2] = p[2] = cur[u][2];
            }
        }
#pragma unroll
        for (int u = 0; u < B; ++u)
#pragma unroll
            for (int e = 0; e < 3; ++e) cur[u][e] = nxt[u][e];
    }
}

// the gradient column v0 = K0^-1 F'(2Qx): one thread per (agent, dim) subsystem, with the mission's factor (in LDS)
// (a function of its own since round 6: the blocked recurrence wants ~40 registers the polish around it does not have to spare)
__device__ __noinline__ void v0_solve3_fn(int nj_v, int nk_v, int nb_v, double* v0_v, const double* f3_v) {
    const int nj = __builtin_amdgcn_readfirstlane(nj_v), nk = __builtin_amdgcn_readfirstlane(nk_v), nb = __builtin_amdgcn_readfirstlane(nb_v);
    double* v0 = uni(v0_v);
    const double* f3 = uni(f3_v);
    for (int it = threadIdx.x; it < nb * 3; it += QP_THREADS) k0_solve3(f3, nj, nk, v0, it);
}

// out = -K0^-1 u from the table, u dense: a thread owns the three values of one (knot jj, agent, dim) and adds G[jj][kb] u_kb over all knots
// kb -- independent loads, PB blocks per trip, no recurrence.  (A function of its own: ~100 registers the polish does not have to spare.)
__device__ __noinline__ void table_product_fn(int nj_v, int nk_v, int nb_v, const double* G_v, const double* u_v, double* out_v) {
    typedef __attribute__((address_space(1))) const double gcd;
    const int nj = __builtin_amdgcn_readfirstlane(nj_v), nk = __builtin_amdgcn_readfirstlane(nk_v), nsub = 3 * __builtin_amdgcn_readfirstlane(nb_v);
    gcd* G = QGC(uni(G_v));
    gcd* uv = QGC(uni(u_v));
    double* out = uni(out_v);
    constexpr int PB = 4;
    for (int it = threadIdx.x; it < nj * nsub; it += QP_THREADS) {
        const int jj = it / nsub, sub = it % nsub;
        double acc[3] = {0, 0, 0};
        for (int k0 = 0; k0 < nj; k0 += PB) {
            double g[PB][9], x[PB][3];
#pragma unroll
            for (int u = 0; u < PB; ++u) {
                const int kb = k0 + u < nj ? k0 + u : nj - 1;
                gcd* blk = G + (jj >= kb ? k0g_block(jj, kb) : k0g_block(kb, jj));
#pragma unroll
                for (int e = 0; e < 9; ++e) g[u][e] = blk[e];
#pragma unroll
                for (int e = 0; e < 3; ++e) x[u][e] = uv[(size_t)kb * nk + sub * 3 + e];
            }
#pragma unroll
            for (int u = 0; u < PB; ++u) {
                if (k0 + u >= nj) continue;
                if (jj >= k0 + u) {  // the stored block is G[jj][kb]
                    acc[0] += g[u][0] * x[u][0] + g[u][1] * x[u][1] + g[u][2] * x[u][2];
                    acc[1] += g[u][3] * x[u][0] + g[u][4] * x[u][1] + g[u][5] * x[u][2];
                    acc[2] += g[u][6] * x[u][0] + g[u][7] * x[u][1] + g[u][8] * x[u][2];
                } else {  // G[jj][kb] = G[kb][jj]'
                    acc[0] += g[u][0] * x[u][0] + g[u][3] * x[u][1] + g[u][6] * x[u][2];
                    acc[1] += g[u][1] * x[u][0] + g[u][4] * x[u][1] + g[u][7] * x[u][2];
                    acc[2] += g[u][2] * x[u][0] + g[u][5] * x[u][1] + g[u][8] * x[u][2];
                }
            }
        }
        const size_t i = (size_t)jj * nk + sub * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) out[i + e] = -acc[e];
    }
}

// S_ab = J_a K0^-1 J_b' of two candidate rows from the table: the bilinear form t_a' G[knot_a][knot_b] t_b is the same for every
// (agent, dim) the rows share, so it is formed once and multiplied by  sum_k n_a[k] n_b[k]  and by the agents' signs: + for a/a and b/b, - for
// a/b.  ma, mb: the rows' cand_meta.  Rows that share no agent, or one agent along different axes, give exactly 0 and load nothing.
__device__ __forceinline__ double s_from_table(const Cand* cand, const double* G, int ci, int cj, int ma, int mb) {
    const int aa = ma & 255, ab = ((ma >> 8) & 255) - 1, ba = mb & 255, bb = ((mb >> 8) & 255) - 1;
    const int sg = (aa == ba) - (bb >= 0 && aa == bb) - (ab >= 0 && ab == ba) + (ab >= 0 && ab == bb);
    bool share = aa == ba || (bb >= 0 && aa == bb) || (ab >= 0 && (ab == ba || ab == bb));
    // ... nor rows of one agent along different axes (two box faces)
    if (share && ab < 0 && bb < 0) share = ((ma & mb) >> 16) != 0;
    if (!share || sg == 0) return 0.0;
    const Cand& ca = cand[ci];
    const Cand& cb = cand[cj];
    const bool a_first = ca.knot >= cb.knot;
    const double* blk = G + k0g_block((a_first ? ca.knot : cb.knot) - 1, (a_first ? cb.knot : ca.knot) - 1);
    return (double)sg * (ca.n[0] * cb.n[0] + ca.n[1] * cb.n[1] + ca.n[2] * cb.n[2]) * k0g_bilinear(blk, a_first, ca.t, cb.t);
}

// v_readlane of a double; lane: wave-uniform
__device__ __forceinline__ double rl_dyn(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

#include "lh_inverse.inc"  // the dual solve's linear algebra: products with the inverse factor W = L^-1 of S_PP

// Lawson-Hanson on  min 1/2 z'Sz - d'z, z >= 0  (n <= PL_NC candidates).  Wave 0 only.  returns nP, or -1 on failure.
// resume_nP >= 0 (round 6): the candidate set has GROWN since the previous call (rows outside it came out violated) -- the old
// candidates keep their indices, their S entries and their d, so the factor W, the active set P and W d_P the previous call ended with are
// still what they were: the iteration goes on from there (n_prev: candidates of the previous call) instead of appending the ~60 active rows
// again one by one, which was half of all the appends of a mission.  shared_int[1] carries "W d_P is valid" from one call to the next.
__device__ int lh_wave(int n, const double* Sg, int ldS, const double* dv, double* zc, double* tv, double* yv, double* wv, int* P, int* inP,
                       int* banned, double* Lc, int* shared_int, int pmax, double* str, bool big, double* stats = nullptr, int resume_nP = -1,
                       int n_prev = 0) {
    const int lane = threadIdx.x & 63;
    kl_lds* Wl = big ? nullptr : (kl_lds*)Lc;  // the factor W = L^-1 through its own address space (ds_read), or in global memory
    double* Wg = big ? Lc : nullptr;
    int* rem = (int*)tv;  // tv is scratch of the append step only
    int nP = 0;
    double dmax = 0;
    const bool resume = resume_nP >= 0;
    for (int a = lane; a < n; a += 64) {
        if (!resume || a >= n_prev)
            zc[a] = 0;
        else
            zc[a] = fmax(zc[a], 0.0);  // (a refinement round of the primal step may have pushed a multiplier a hair below zero)
        inP[a] = 0, banned[a] = 0;
        dmax = fmax(dmax, fabs(dv[a]));
    }
    dmax = wave_red(dmax, 1);
    const double wtol = 1e-12 * fmax(1.0, dmax);
    if (resume) {
        nP = resume_nP;
        WSYNC();
        for (int b = lane; b < nP; b += 64) inP[P[b]] = 1;  // (the primal step used inP as scratch)
    } else {
        lh_reset(Wl, Wg, pmax);
    }
    WSYNC();
    // WARM START (str != nullptr): the rows the interior-point iterate marks as clearly active (z/s > 100) enter the
    // factor first, strongest first, without the gradient pass and the re-solve an ordinary Lawson-Hanson step costs;
    // then one solve, rows with a non-positive multiplier leave (the inner loop below, started from z = 0, drops exactly
    // those), and the ordinary iteration takes over.  It is still Lawson-Hanson: any feasible active set is a valid start.
    bool warming = str != nullptr && !resume;
    // wv = W d_P is kept up to date across appended rows (one more entry per row: a dot product), so a solve of S_PP y = d_P
    // is ONE product (y = W' wv), not two; only a deletion invalidates it
    bool w_valid = resume ? shared_int[1] != 0 : true;
    bool first_resumed = resume && nP > 0;  // a resumed call starts with a solve on the carried-over active set (no row to append yet)
    if (stats && lane == 0) stats[7] += 1.0;
    for (int itn = 0; itn < 6 * n + 20; ++itn) {
        long long lt0 = stats ? wall_clock64() : 0;
        double best = wtol;
        int bidx = -1;
        bool do_append = true;
        if (first_resumed) {
            first_resumed = false, do_append = false;
        } else if (warming) {
            best = 100.0;
            for (int a = lane; a < n; a += 64)
                if (str[a] > best) best = str[a], bidx = a;
            wave_argmax(best, bidx);
            if (bidx >= 0 && lane == 0) str[bidx] = 0.0;
            WSYNC();
            if (bidx < 0 || nP >= pmax - 8) {
                warming = false, do_append = false;
                if (nP == 0) continue;
            }
        } else {
            // g = d - S[:, P] z_P for every candidate.  Lane l owns candidates l, l + 64, ... (an accumulator each); the active
            // rows are walked together: their index and multiplier travel by readlane from per-lane copies, so the S loads of four
            // rows x four candidates are in flight at once and nothing but the multiply-adds is dependent.  (One candidate at a time
            // with the index chain P[b] -> S -> z through LDS took 23 k cycles per pass, the largest part of the dual solve.)
            double acc[4] = {0, 0, 0, 0};
            for (int q0 = 0; q0 < nP; q0 += 64) {
                const int pl = q0 + lane < nP ? P[q0 + lane] : -1;
                const double zl = pl >= 0 ? zc[pl] : 0.0;
                const int nb = nP - q0 < 64 ? nP - q0 : 64;
                for (int b0 = 0; b0 < nb; b0 += 4) {
                    double sv[4][4], zb[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int bb = b0 + u < nb ? b0 + u : nb - 1;
                        const int pb = __builtin_amdgcn_readlane(pl, bb);
                        zb[u] = b0 + u < nb ? rl_dyn(zl, bb) : 0.0;
                        const double* row = Sg + (size_t)pb * ldS;
#pragma unroll
                        for (int v = 0; v < 4; ++v) sv[u][v] = lane + 64 * v < n ? row[lane + 64 * v] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v) acc[v] += sv[u][v] * zb[u];
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int a = lane + 64 * v;
                if (a < n) {
                    const double s = dv[a] - acc[v];
                    if (!inP[a] && !banned[a] && s > best) best = s, bidx = a;
                }
            }
            wave_argmax(best, bidx);
            if (stats && lane == 0) { const long long t_ = wall_clock64(); stats[0] += (double)(t_ - lt0); lt0 = t_; stats[4] += 1.0; }
            if (bidx < 0) break;
        }
        const int j = bidx;
        if (do_append) {
            if (nP >= pmax) return -1;
            // append row j: l = W S[P, j]; new row of W = (-W'l, 1) / sqrt(s_jj - |l|^2)
            double sr[LH_H], lr[LH_H], wr[LH_H], tr[LH_H];
#pragma unroll
            for (int h = 0; h < LH_H; ++h) sr[h] = lane + 64 * h < nP ? Sg[(size_t)P[lane + 64 * h] * ldS + j] : 0.0;
            lh_rows(Wl, Wg, sr, lr, nP, lane);
            lhv_load(wv, wr, nP, lane);
            double ll = 0, lw = 0;
#pragma unroll
            for (int h = 0; h < LH_H; ++h) ll += lr[h] * lr[h], lw += w_valid ? lr[h] * wr[h] : 0.0;
            ll = wave_red(ll, 0);
            const double sjj = Sg[(size_t)j * ldS + j];
            const double djj = sjj - ll;
            if (!(djj > 1e-13 * fmax(1e-30, sjj))) {  // (numerically) dependent on the rows already active
                if (lane == 0) banned[j] = 1;
                WSYNC();
                continue;
            }
            lw = wave_red(lw, 0);
            lh_cols(Wl, Wg, lr, tr, nP, lane);
            const double ir = fast_rsqrt(djj);
            {
                const int rowo = lhp_row(nP), len = lhp_len(nP >> 3);
#pragma unroll
                for (int h = 0; h < LH_H; ++h) {
                    const int cq = lane + 64 * h;
                    if (cq < len) Lc[rowo + cq] = cq < nP ? -ir * tr[h] : (cq == nP ? ir : 0.0);  // (zeros right of the diagonal)
                }
            }
            if (lane == 0) {
                P[nP] = j;
                inP[j] = 1;
                wv[nP] = (dv[j] - lw) * ir;
            }
            nP++;
            WSYNC();
            if (stats && lane == 0) { const long long t_ = wall_clock64(); stats[1] += (double)(t_ - lt0); lt0 = t_; stats[5] += 1.0; }
        }
        if (warming) continue;
        for (int inner = 0; inner < 2 * pmax; ++inner) {
            {
                double wr[LH_H], yr[LH_H];
                if (!w_valid) {
                    double dr[LH_H];
#pragma unroll
                    for (int h = 0; h < LH_H; ++h) dr[h] = lane + 64 * h < nP ? dv[P[lane + 64 * h]] : 0.0;
                    lh_rows(Wl, Wg, dr, wr, nP, lane);
                    lhv_store(wv, wr, nP, lane);
                    w_valid = true;
                } else
                    lhv_load(wv, wr, nP, lane);
                lh_cols(Wl, Wg, wr, yr, nP, lane);
                lhv_store(yv, yr, nP, lane);
                WSYNC();
                if (stats && lane == 0) stats[6] += 1.0;
            }
            double ymin = 1e300;
            for (int b = lane; b < nP; b += 64) ymin = fmin(ymin, yv[b]);
            ymin = wave_red(ymin, 2);
            if (ymin > 0) {
                for (int b = lane; b < nP; b += 64) zc[P[b]] = yv[b];
                WSYNC();
                if (stats && lane == 0) { const long long t_ = wall_clock64(); stats[2] += (double)(t_ - lt0); lt0 = t_; }
                break;
            }
            double alpha = 1e300;
            for (int b = lane; b < nP; b += 64)
                if (yv[b] <= 0) alpha = fmin(alpha, zc[P[b]] / (zc[P[b]] - yv[b]));
            alpha = wave_red(alpha, 2);
            if (stats && lane == 0) { const long long t_ = wall_clock64(); stats[2] += (double)(t_ - lt0); lt0 = t_; }
            if (!(alpha >= 0)) alpha = 0;
            for (int b = lane; b < nP; b += 64) zc[P[b]] += alpha * (yv[b] - zc[P[b]]);
            WSYNC();
            if (lane == 0) {  // positions (in P) of the rows that leave the active set, ascending, into rem[]
                int nrem = 0, worst = 0;
                for (int b = 1; b < nP; ++b)
                    if (yv[b] < yv[worst]) worst = b;
                for (int b = 0; b < nP; ++b) {
                    const int ia = P[b];
                    if (yv[b] <= 0 && zc[ia] <= 1e-14 * fmax(1.0, fabs(yv[b]))) rem[nrem++] = b;
                }
                if (nrem == 0) rem[nrem++] = worst;  // numerical safety: drop the most negative target
                *shared_int = nrem;
            }
            WSYNC();
            const int nrem = *shared_int;
            for (int q = nrem - 1; q >= 0; --q) {  // descending positions keep the earlier ones valid
                const int pos = rem[q];
                lh_delete(Wl, Wg, yv, nP, pos, lane);  // (tv holds rem[]; yv is recomputed by the next solve)
                if (lane == 0) {
                    const int ia = P[pos];
                    zc[ia] = 0, inP[ia] = 0;
                    for (int b = pos; b < nP - 1; ++b) P[b] = P[b + 1];
                }
                nP--;
                WSYNC();
            }
            for (int a = lane; a < n; a += 64) banned[a] = 0;
            w_valid = false;  // rows left the factor
            WSYNC();
            if (stats && lane == 0) { const long long t_ = wall_clock64(); stats[3] += (double)(t_ - lt0); lt0 = t_; }
            if (nP == 0) break;
        }
    }
    if (lane == 0) shared_int[1] = w_valid ? 1 : 0;
    return nP;
}

// called by every thread of the workgroup after the interior-point loop converged.  Returns 0 if the polished point was
// accepted (control points of the batch agents overwritten), else the reason: 1 too many candidates, 2 K0 not positive
// definite, 3 dual solve failed, 4 KKT verification failed.
// mode: 0 = candidates from the interior-point iterate, 1 = from the geometry (polish-first of later Gauss-Seidel passes),
//       2 = as 0 with capacity PL_PBIG for the dual solve, its packed factor in global memory (slow, rare).
__device__ __forceinline__ int polish_qp(RowCtx& c, PassIO& io, const PolishWs& pw, double* lds, double* red, int* flag, int mode) {
    const bool geometric = mode == 1, big = mode == 2;
    const QpDims& d = c.d;
    const QpWs& w = c.w;
    const int tid = threadIdx.x, NK = d.nk;
    double* ctrl = const_cast<double*>(c.ctrl);
    // LDS carve
    const int pmax = big ? PL_PBIG : polish_pmax(NK);    // rows simultaneously active in the dual solve
    double* Lc = big ? pw.Lbig : lds;                    // lhp_size(pmax): the inverse factor W (lh_inverse.inc)
    double* zc = big ? lds : lds + lhp_size(pmax);       // PL_NC
    double* dv = zc + PL_NC;                             // PL_NC
    double* tv = dv + PL_NC;                             // pmax
    double* yv = tv + pmax;                              // pmax
    double* wv = yv + pmax;                              // pmax: W d_P, kept across appended rows
    int* P = (int*)(wv + pmax);                          // pmax
    int* inP = P + pmax;                                 // PL_NC
    int* banned = inP + PL_NC;                           // PL_NC
    int* sint = banned + PL_NC;                          // 4
    double* str = (double*)(sint + 4);                   // PL_NC: warm-start strengths
    double* f3 = str + PL_NC;                            // 18 * nj: factor of K0's 3x3-block tridiagonal

#ifdef QP_LHSTATS
#define QP_PPROF_ON 0
#else
#define QP_PPROF_ON 1
#endif
#ifdef QP_PROFILE
    double* pscal = c.scal + 20;
    long long pt0 = wall_clock64();
#define PPROF(i)                                       \
    do {                                               \
        __syncthreads();                               \
        const long long t_ = wall_clock64();           \
        if (tid == 0 && QP_PPROF_ON) pscal[i] += (double)(t_ - pt0);  \
        pt0 = t_;                                      \
    } while (0)
#else
#define PPROF(i)
#endif
    // ---- candidates
    if (tid == 0) pw.ncand[0] = 0;
    __threadfence_block();
    __syncthreads();
    if (geometric)
        row_pass<PASS_CAND_GEO>(c, io);
    else
        row_pass<PASS_CAND>(c, io);
    __threadfence_block();
    __syncthreads();
    if (pw.ncand[0] > PL_NC) return 1;

    // ---- K0 = reduced Hessian without barrier terms: blockdiag(D_j) + E couplings, one 3x3-block chain for all: the mission's table
    {
        const int* k0bad = (const int*)(pw.k0f + 18 * (size_t)d.nj);  // the double factor's flag, the dd factor's
        if (k0bad[0] | k0bad[1]) return 2;
    }
    for (int it = tid; it < 18 * d.nj; it += QP_THREADS) f3[it] = pw.k0f[it];

    // column 0 = K0^{-1} F'(2Qx)
    for (int it0 = tid; it0 < d.nb * 3 * d.oq; it0 += 4 * QP_THREADS) {  // (four entries per thread and round, loads ahead of the stores)
        double xq[4][6], sc4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int it = it0 + q * QP_THREADS < d.nb * 3 * d.oq ? it0 + q * QP_THREADS : it0;
            const int a = it / (3 * d.oq), k = (it / d.oq) % 3, j6 = it % d.oq, m = j6 / 6;
            const double* xs = ctrl + ((size_t)(d.first + a) * 3 + k) * d.oq + 6 * m;
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) xq[q][jj] = xs[jj];
            sc4[q] = w.segsc[m];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int it = it0 + q * QP_THREADS;
            if (it < d.nb * 3 * d.oq) {
                const int i = (it % d.oq) % 6;
                double g = 0;
#pragma unroll
                for (int jj = 0; jj < 6; ++jj) g += Qbase[6 * i + jj] * xq[q][jj];
                w.cvec[it] = 2 * sc4[q] * g;
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    double* gred = pw.v0 + (size_t)d.nj * NK;   // F'(2Qx), kept for the primal step
    double* usum = gred + (size_t)d.nj * NK;    // g + J_P' z of a refinement round
    apply_FT(d, w, w.cvec, gred, 1.0);
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < d.nj * NK; i += QP_THREADS) pw.v0[i] = gred[i];
    __threadfence_block();
    __syncthreads();
    v0_solve3_fn(d.nj, d.nk, d.nb, pw.v0, f3);
    __threadfence_block();
    __syncthreads();

    PPROF(0);
    bool accepted = false;
    int n_done = 0, nP = 0;
    for (int outer = 0; outer < 8 && !accepted; ++outer) {
        const int n = pw.ncand[0];
        if (n > PL_NC) return 1;
        const int n_prev = n_done;  // candidates of the previous round
#ifndef QP_PROFILE
        if (outer > 0 && tid == 0) c.scal[SC_PROF0 + 4] += 1;  // diagnostic: dual solves resumed on a grown candidate set (S extended)
#endif
        const int first_new = n_done;
        // The sweeps append candidates with an atomic counter, i.e. in the order the hardware happens to schedule the threads; the
        // dual solve breaks ties by position and rounds in the order it meets the rows, so two runs of the same QP could end 1e-8 m
        // apart (both KKT-certified).  Put the new candidates into a defined order -- ascending row slot, which is unique -- so that
        // the answer is reproducible bit for bit whatever else runs on the CU.
        {
            const int n_new = n - first_new;
            for (int i = tid; i < n_new; i += QP_THREADS) inP[i] = pw.cand[first_new + i].row;
            __syncthreads();
            Cand mine;
            int rank = 0;
            if (tid < n_new) {
                mine = pw.cand[first_new + tid];
                for (int j = 0; j < n_new; ++j) rank += inP[j] < mine.row;
            }
            __syncthreads();
            if (tid < n_new) pw.cand[first_new + rank] = mine;
            __threadfence_block();
            __syncthreads();
        }
        // which (agent, dim) subsystems a candidate lives in, for all candidates (inP is idle until the dual solve)
        for (int ci = tid; ci < n; ci += QP_THREADS) inP[ci] = cand_meta(pw.cand[ci]);
        n_done = n;
        __syncthreads();
        // ---- S = J K0^-1 J' from the mission's table (symmetric by construction: one value per pair), d = -J v0 - slack
        // (K0 couples neither agents nor dimensions: S_ij = 0 exactly for rows that share no batch agent, or one agent along different
        // axes -- most pairs of box rows; rounds > 0 only compute what is new)
        for (int it = tid; it < n * n; it += QP_THREADS) {
            const int ci = it / n, cj = it % n;
            if (cj > ci || ci < first_new) continue;
            const double sv = s_from_table(pw.cand, pw.G, ci, cj, inP[ci], inP[cj]);
            pw.Sg[(size_t)ci * PL_NC + cj] = sv;
            pw.Sg[(size_t)cj * PL_NC + ci] = sv;
        }
        for (int ci = tid; ci < n; ci += QP_THREADS) dv[ci] = -cand_dot(pw.cand[ci], pw.v0, NK) - pw.cand[ci].slack;
        // warm start of the dual solve: first round the rows the interior-point iterate marks as active (strength = z/s); a later round
        // (rows outside the candidate set came out violated and joined it) starts from the active set the previous round ended with --
        // zc still holds it (multiplier > 0) -- instead of from nothing: without it every such round repeated the whole build-up, one gradient pass
        // and one solve per row
        for (int ci = tid; ci < n; ci += QP_THREADS)
            str[ci] = outer == 0 ? pw.cand[ci].strength : (ci < n_prev && zc[ci] > 0 ? 1e3 + zc[ci] : 0.0);
        __threadfence_block();
        __syncthreads();
        // the dual solve reads S a few thousand times with a dependent access pattern: keep it in LDS when it fits
        const double* Suse = pw.Sg;
        int ldS = PL_NC;
        {
            double* Sl = f3 + 18 * d.nj;
            if ((int)(Sl - lds) + n * n <= c.lds_avail) {
                for (int it = tid; it < n * n; it += QP_THREADS) Sl[it] = pw.Sg[(size_t)(it / n) * PL_NC + it % n];
                Suse = Sl, ldS = n;
                __syncthreads();
            }
        }
        PPROF(1);
        // ---- dual active-set solve (wave 0)
        if (tid < 64) {
            __builtin_amdgcn_s_setprio(QP_CHAIN_PRIO);  // one wave, one dependent chain (see twisted_factor in qp_wave_factor.inc)
            const int res_nP = (outer > 0 && nP > 0) ? nP : -1;
#ifdef QP_LHSTATS
            const int r = lh_wave(n, Suse, ldS, dv, zc, tv, yv, wv, P, inP, banned, Lc, sint + 2, pmax, str, big, c.scal + 20, res_nP, n_prev);
#else
            const int r = lh_wave(n, Suse, ldS, dv, zc, tv, yv, wv, P, inP, banned, Lc, sint + 2, pmax, str, big, nullptr, res_nP, n_prev);
#endif
            __builtin_amdgcn_s_setprio(0);
            if (tid == 0) sint[1] = r;
        }
        __syncthreads();
        nP = sint[1];
        PPROF(2);
        if (nP < 0) return 3;
        // ---- primal step, refinement against the actual residual of the active rows, verification
        // The active rows are listed per (agent, dim) subsystem of K0 once per dual solve -- the refinement rounds below change z, not the
        // active set -- (tv, banned, inP, str are idle outside the dual solve): pmeta[b] the row's agents and axes, off[sub] where a
        // subsystem's entries start in ptab, in the order of P -- an entry's place is counted, not claimed, so the sums are formed in a
        // fixed order.  An entry: knot * 1024 + position in P, then sgn n_k t[0..2]; the multiplier joins it per round.
        int* pmeta = inP;        // [nP]   (the dual solve is over: its membership flags are not needed any more)
        int* off = banned;       // [3 nb + 1]
        const int nsub = 3 * d.nb;
        for (int b = tid; b < nP; b += QP_THREADS) pmeta[b] = cand_meta(pw.cand[P[b]]);
        __syncthreads();
        for (int sub = tid; sub < nsub; sub += QP_THREADS) {
            int cnt = 0;
            for (int b = 0; b < nP; ++b) cnt += meta_sign(pmeta[b], sub / 3, sub % 3) != 0;
            ((int*)str)[sub] = cnt;
        }
        __syncthreads();
        for (int sub = tid; sub <= nsub; sub += QP_THREADS) {
            int o = 0;
            for (int q = 0; q < sub; ++q) o += ((int*)str)[q];
            off[sub] = o;
        }
        __syncthreads();
        for (int it = tid; it < nP * 6; it += QP_THREADS) {
            const int b = it / 6, side = (it % 6) / 3, k = it % 3;
            const int meta = pmeta[b], ag = side == 0 ? (meta & 255) : ((meta >> 8) & 255) - 1;
            if (ag < 0 || !(((meta >> 16) >> k) & 1)) continue;
            int rank = 0;
            for (int q = 0; q < b; ++q) rank += meta_sign(pmeta[q], ag, k) != 0;
            const Cand& cd = pw.cand[P[b]];
            const double sn = side == 0 ? cd.n[k] : -cd.n[k];
            double* en = pw.ptab + 4 * (size_t)(off[ag * 3 + k] + rank);
            en[0] = (double)((cd.knot - 1) * 1024 + b), en[1] = sn * cd.t[0], en[2] = sn * cd.t[1], en[3] = sn * cd.t[2];
        }
        __threadfence_block();
        __syncthreads();
        for (int round = 0; round < 4; ++round) {
            // x-space step -K0^-1 (g + J_P' z) from the table
            for (int b = tid; b < nP; b += QP_THREADS) tv[b] = zc[P[b]];
            __syncthreads();
            // g + J_P' z, the sum first (see k0_mission_tables): a thread owns one (knot, agent, dim) and adds its subsystem's entries on that knot
            for (int it = tid; it < d.nj * nsub; it += QP_THREADS) {
                const int kb = it / nsub, sub = it % nsub;
                const size_t i = (size_t)kb * NK + sub * 3;
                double u0 = gred[i], u1 = gred[i + 1], u2 = gred[i + 2];
                for (int o = off[sub]; o < off[sub + 1]; ++o) {
                    const double* en = pw.ptab + 4 * (size_t)o;
                    const int key = (int)en[0];
                    if ((key >> 10) == kb) {
                        const double zb = tv[key & 1023];
                        u0 += zb * en[1], u1 += zb * en[2], u2 += zb * en[3];
                    }
                }
                usum[i] = u0, usum[i + 1] = u1, usum[i + 2] = u2;
            }
            __threadfence_block();
            __syncthreads();
            table_product_fn(d.nj, NK, d.nb, pw.G, usum, w.rhs);
            __threadfence_block();
            __syncthreads();
            apply_F(d, w, w.rhs, w.dx);
            __threadfence_block();
            __syncthreads();
            io.vmax = 0;
            row_pass<PASS_VERIFY>(c, io);  // rows outside the candidate set that come out violated join it
            const double vmax = block_reduce(io.vmax, 1, red);
            __threadfence_block();
            __syncthreads();
            if (pw.ncand[0] > n) break;  // new candidates: extend V, S and solve the dual again
            double emax = 0, zmin = 0, zmax = 0;
            for (int b = tid; b < nP; b += QP_THREADS) {
                const double e = w.ds[pw.cand[P[b]].row];
                yv[b] = -e;
                emax = fmax(emax, fabs(e));
                zmin = fmin(zmin, zc[P[b]]), zmax = fmax(zmax, zc[P[b]]);
            }
            emax = block_reduce(emax, 1, red);
            zmin = block_reduce(zmin, 2, red);
            zmax = block_reduce(zmax, 1, red);
#ifdef QP_POLSTATS
            if (tid == 0) {
                double* ps = c.scal + 20;
                ps[0] = vmax, ps[1] = zmin, ps[2] = zmax, ps[3] = emax + 1000.0 * round + 1e6 * outer + 1e8 * nP + 1e12 * n;
            }
#endif
            // feasibility 5e-9: rows that are numerically dependent on the active ones (lattice-aligned SFC faces against
            // r_i + r_j rows) can stay inconsistent at the 1e-9 level whatever the active set
            if (vmax <= 5e-9 && zmin >= -1e-9 * fmax(1.0, zmax) && (emax < 1e-12 || round == 3)) {
                accepted = true;
                if (tid == 0) red[12] = fmax(fmax(vmax, 0.0), fmax(0.0, -zmin) / fmax(1.0, zmax));  // KKT residual of the accepted point
                break;
            }
            if (round == 3) break;
            if (tid < 64 && nP > 0) {  // S_PP dz = -e  with the factor left by the dual solve
                const int lane = tid;
                double er[LH_H], ur[LH_H], yr[LH_H];
                kl_lds* Wl = big ? nullptr : (kl_lds*)Lc;
                double* Wg = big ? Lc : nullptr;
                lhv_load(yv, er, nP, lane);
                lh_rows(Wl, Wg, er, ur, nP, lane);
                lh_cols(Wl, Wg, ur, yr, nP, lane);
#pragma unroll
                for (int h = 0; h < LH_H; ++h)
                    if (lane + 64 * h < nP) zc[P[lane + 64 * h]] += yr[h];
            }
            __syncthreads();
        }
        PPROF(3);
        if (!accepted && pw.ncand[0] <= n) break;  // verification failed without new candidates
    }
    if (!accepted) return 4;
    {
        double* xb = ctrl + (size_t)d.first * 3 * d.oq;  // the batch agents' control points are contiguous
        const int nx = d.nb * 3 * d.oq;
        for (int i0 = tid; i0 < nx; i0 += 4 * QP_THREADS) {
            double xv[4], dv4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + q * QP_THREADS;
                xv[q] = i < nx ? xb[i] : 0.0, dv4[q] = i < nx ? w.dx[i] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i0 + q * QP_THREADS < nx) xb[i0 + q * QP_THREADS] = xv[q] + dv4[q];
        }
    }
    __threadfence_block();
    __syncthreads();
    // control points with an ACTIVE SFC bound sit exactly on the face (keeps the next batch's rows consistent)
    for (int b = tid; b < nP; b += QP_THREADS) {
        const Cand& cd = pw.cand[P[b]];
        if (cd.snap_idx >= 0 && zc[P[b]] > 0) ctrl[cd.snap_idx] = cd.snap_val;
    }
    __threadfence_block();
    __syncthreads();
    return 0;
}

// stand-alone entry (own copy of the row context, own reduction scratch): see BlkArgs and uni_words in qp_base.inc
__device__ __noinline__ int polish_entry(RowCtx c_in, PolishWs pw_in, double* lds, double* red, int* flag, int mode) {
    PassIO io = {};
    RowCtx c = uni_words(c_in);
    PolishWs pw = uni_words(pw_in);
    c.pw = &pw;
    return polish_qp(c, io, pw, uni(lds), uni(red), uni(flag), uni(mode));
}
