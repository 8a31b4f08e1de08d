// jqp_polish.inc — active-set polish ("crossover") of the grid-wide joint QP: the kernels.  Included by jqp.hip, once, behind its tile sweep;
// its records (Pol, PolLayout, pol_carve, pol_emit, PC_*, PS_*) are jqp_polish_types.inc, which jqp.hip includes ahead of its sweeps.
//
// Same mathematics as qp_polish.inc (one workgroup, <= 256 candidate rows, Lawson-Hanson in one wave), re-shaped for active sets of
// thousands of rows and many workgroups:
//   candidates C  = rows with dominant multiplier or slack < 1e-6 at the interior-point iterate (sweep PASS_CAND), sorted by row id
//   K0^-1         = inverse of the reduced Hessian without barrier terms.  K0 couples neither agents nor dimensions and is the SAME
//                   3x3-block tridiagonal matrix for every (agent, dim): ONE dense inverse R (3 nj x 3 nj) per mission
//   S = J_C K0^-1 J_C'  in closed form:  S_rs = (sum over shared agents of sigma_r sigma_s) (n_r . n_s) (t_r' R[j_r, j_s] t_s)
//   dual QP  min 1/2 z'Sz - d'z, z >= 0  by BLOCK PRINCIPAL PIVOTING (Judice & Pires): the active set A is exchanged in blocks -- rows
//                   with z_i < 0 leave, rows with (Sz - d)_i < 0 enter -- with a finite single-exchange fallback; every round needs
//                   S_AA^-1, computed by the tile sweep of the knot matrices (jq_pivot0 / jq_panel / jq_update, kind 1)
//   x_new = x + F du,  du = -K0^-1 (F'2Qx + J_A' z),  refined against the actual residuals of the active rows
// The point is taken only if every row of the QP is feasible to 5e-9 and all multipliers are >= -1e-9 max(1, z_max) (the acceptance test
// of qp_polish.inc); rows outside the candidate set that come out violated join it and the dual solve is repeated.

#define POL_GATE(state_needed)                                                         \
    if (w.st[ST_STATE] != 0.0 || w.st[ST_GO] == 0.0 || w.st[ST_PSTATE] != (double)(state_needed)) return

// start of a polish attempt: counters, and (once per run) R = K0^-1 of one (agent, dim) chain
__global__ __launch_bounds__(256) void jp_begin(JArgs A) {
    const int mission = blockIdx.x, tid = threadIdx.x;
    const Ws w = carve(A, mission);
    if (w.st[ST_STATE] != 0.0 || w.st[ST_GO] == 0.0) return;
    const Pol p = pol_carve(A, mission);
    const JDims d = jdims(A.S.N, A.S.Mk[mission]);
    const int nj = d.nj, nr = 3 * nj;
    if (tid < PC_N) p.cnt[tid] = 0;
    if (tid == 0) p.cnt[PC_BEST] = 0x7fffffff, w.st[ST_PSTATE] = PS_SOLVE, w.st[ST_PTAU] = 1.0;
    if (w.st[ST_RDONE] != 0.0) return;
    // factor of the 3x3-block tridiagonal K0 chain (common/ipm_rows.h), 18 doubles per knot
    extern __shared__ double f3[];  // 18 * nj
    for (int it = tid; it < 18 * nj; it += 256) {
        const int jj = it / 18, e = it % 18, j = jj + 1;
        f3[it] = e < 9 ? w.Dk[9 * j + e] : (jj + 1 < nj ? w.Ek[9 * j + (e - 9)] : 0.0);
    }
    __syncthreads();
    if (tid == 0) {
        double Bp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int jj = 0; jj < nj; ++jj) (void)k0_factor_step(f3 + 18 * jj, Bp, jj == 0);  // (a pivot that is not positive shows in the KKT check)
    }
    __syncthreads();
    // column c of R: solve K0 y = e_c  (R is symmetric: stored as row c)
    for (int c = tid; c < nr; c += 256) {
        double* y = p.R + (size_t)c * nr;
        for (int i = 0; i < nr; ++i) y[i] = i == c ? 1.0 : 0.0;
        double p[3] = {0, 0, 0};
        for (int jj = 0; jj < nj; ++jj) {
            double yk[3] = {y[3 * jj], y[3 * jj + 1], y[3 * jj + 2]};
            k0_forward_step((const double*)f3 + 18 * jj, jj > 0, yk, p);
            y[3 * jj] = p[0] = yk[0], y[3 * jj + 1] = p[1] = yk[1], y[3 * jj + 2] = p[2] = yk[2];
        }
        for (int jj = nj - 1; jj >= 0; --jj) {
            double yk[3] = {y[3 * jj], y[3 * jj + 1], y[3 * jj + 2]};
            k0_backward_step((const double*)f3 + 18 * jj, jj + 1 < nj, yk, p);
            y[3 * jj] = p[0] = yk[0], y[3 * jj + 1] = p[1] = yk[1], y[3 * jj + 2] = p[2] = yk[2];
        }
    }
    if (tid == 0) w.st[ST_RDONE] = 1.0;
}

// c0 = F'(2Qx): one thread per (knot, agent, dim)
__global__ __launch_bounds__(256) void jp_c0(JArgs A) {
    const DevSession& S = A.S;
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_SOLVE);
    const Pol p = pol_carve(A, mission);
    const int N = S.N, M = S.Mk[mission], MS = S.M;
    const JDims d = jdims(N, M);
    const int nu = 3 * N, it = blockIdx.x * 256 + threadIdx.x;
    if (it >= d.nj * nu) return;
    const int j = it / nu + 1, u = it % nu;
    const double* ctrl = S.ctrl + (size_t)mission * N * 3 * 6 * MS + (size_t)u * d.oq;
    const double* L = w.Lk + 9 * j;
    double g[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int j6 = 6 * (j - 1) + 3 + q, m = j6 / 6, i = j6 % 6;
        double gv = 0;
#pragma unroll
        for (int jj = 0; jj < 6; ++jj) gv += Qbase[6 * i + jj] * ctrl[6 * m + jj];
        g[q] = 2 * w.segsc[m] * gv;
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) p.c0[(size_t)(j - 1) * d.nkp + u * 3 + e] = g[3 + e] + L[0 + e] * g[0] + L[3 + e] * g[1] + L[6 + e] * g[2];
}

// out = sign * R (x) in  per (agent, dim) chain (+ add):  out[(jj, u, e)] = add[(jj, u, e)] * addsign + sign * sum R[(jj, e), (jj', e')] in[(jj', u, e')]
// which: 0: v0 = R c0     1: du = -v0 - R jz
__global__ __launch_bounds__(256) void jp_chain_mv(JArgs A, int which) {
    const DevSession& S = A.S;
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(which == 0 ? PS_SOLVE : PS_PRIMAL);
    const Pol p = pol_carve(A, mission);
    const JDims d = jdims(S.N, S.Mk[mission]);
    const int nu = 3 * S.N, it = blockIdx.x * 256 + threadIdx.x, nr = 3 * d.nj;
    if (it >= d.nj * nu * 3) return;
    const int e = it % 3, u = (it / 3) % nu, jj = it / (3 * nu);
    const double* in = which == 0 ? p.c0 : p.jz;
    const double* Rr = p.R + (size_t)(3 * jj + e) * nr;
    double acc = 0;
    for (int j2 = 0; j2 < d.nj; ++j2) {
        const double* v = in + (size_t)j2 * d.nkp + u * 3;
        acc += Rr[3 * j2] * v[0] + Rr[3 * j2 + 1] * v[1] + Rr[3 * j2 + 2] * v[2];
    }
    const size_t o = (size_t)jj * d.nkp + u * 3 + e;
    if (which == 0)
        p.v0[o] = acc;
    else
        p.du[o] = -p.v0[o] - acc;
}

// new raw candidates -> sorted list (ascending row id among the new ones: reproducible whatever the sweep's scheduling was)
__global__ __launch_bounds__(256) void jp_sort(JArgs A) {
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_SOLVE);
    const Pol p = pol_carve(A, mission);
    const JDims d = jdims(A.S.N, A.S.Mk[mission]);
    const int nraw = p.cnt[PC_NRAW], nc = p.cnt[PC_NCAND];
    if (nraw + nc > p.ncmax) return;  // (jp_sort_fin fails the attempt)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nraw) return;
    const int row = p.r_row[i];
    int rank = 0;
    for (int j = 0; j < nraw; ++j) rank += p.r_row[j] < row;
    const int q = nc + rank, j6 = p.r_j6[i], m = j6 / 6, ii = j6 % 6;
    p.c_row[q] = row, p.c_a[q] = p.r_a[i], p.c_b[q] = p.r_b[i], p.c_snap[q] = p.r_snap[i];
    for (int e = 0; e < 3; ++e) p.c_n[3 * q + e] = p.r_n[3 * i + e];
    p.c_slack[q] = p.r_slack[i], p.c_str[q] = p.r_str[i], p.c_snapv[q] = p.r_snapv[i];
    if (ii < 3) {
        p.c_knot[q] = m - 1;  // 0-based knot: control points 6m .. 6m+2 are u_m itself
        for (int e = 0; e < 3; ++e) p.c_t[3 * q + e] = e == ii ? 1.0 : 0.0;
    } else {
        p.c_knot[q] = m;
        for (int e = 0; e < 3; ++e) p.c_t[3 * q + e] = w.Lk[9 * (m + 1) + 3 * (ii - 3) + e];
    }
    p.pos[row] = q;
    // initial active set: the rows the interior-point iterate marks as active (z > s).  Rows a verification found violated join the
    // candidates INACTIVE: the exchange below lets them in by violation, a limited number at a time
    p.inA[q] = (p.cnt[PC_OUTER] == 0 && p.r_str[i] >= 1.0) ? 1 : 0;
    p.flip[q] = 0;
    p.mark[q] = 0;
    p.z[q] = 0.0, p.y[q] = 0.0;
    (void)d;
}
__global__ void jp_sort_fin(JArgs A) {
    const int mission = blockIdx.x;
    const Ws w = carve(A, mission);
    POL_GATE(PS_SOLVE);
    const Pol p = pol_carve(A, mission);
    if (threadIdx.x != 0) return;
    const int nraw = p.cnt[PC_NRAW], nc = p.cnt[PC_NCAND];
    if (nraw + nc > p.ncmax) {
        w.st[ST_PSTATE] = PS_FAILED, p.cnt[PC_REASON] = 1;  // too many candidates
        return;
    }
    p.cnt[PC_FIRSTNEW] = nc, p.cnt[PC_NCAND] = nc + nraw, p.cnt[PC_NRAW] = 0, p.cnt[PC_NNEW] = nraw;
}

// S (new rows / columns) and d
__global__ __launch_bounds__(256) void jp_S(JArgs A) {
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_SOLVE);
    const Pol p = pol_carve(A, mission);
    const JDims d = jdims(A.S.N, A.S.Mk[mission]);
    const int nc = p.cnt[PC_NCAND], first_new = p.cnt[PC_FIRSTNEW], nr = 3 * d.nj;
    const size_t it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= (size_t)nc * nc) return;
    const int r = (int)(it / nc), s = (int)(it % nc);
    if (s > r || r < first_new) return;
    const int ar = p.c_a[r], br = p.c_b[r], as = p.c_a[s], bs = p.c_b[s];
    double sg = 0;
    if (ar == as) sg += 1;
    if (ar == bs) sg -= 1;
    if (br >= 0 && br == as) sg -= 1;
    if (br >= 0 && br == bs) sg += 1;
    double sv = 0;
    if (sg != 0) {
        const double nn = p.c_n[3 * r] * p.c_n[3 * s] + p.c_n[3 * r + 1] * p.c_n[3 * s + 1] + p.c_n[3 * r + 2] * p.c_n[3 * s + 2];
        if (nn != 0) {
            const double* Rb = p.R + (size_t)(3 * p.c_knot[r]) * nr + 3 * p.c_knot[s];
            double tt = 0;
#pragma unroll
            for (int e = 0; e < 3; ++e)
#pragma unroll
                for (int f = 0; f < 3; ++f) tt += p.c_t[3 * r + e] * Rb[(size_t)e * nr + f] * p.c_t[3 * s + f];
            sv = sg * nn * tt;
        }
    }
    p.S[(size_t)r * p.ncmax + s] = sv;
    p.S[(size_t)s * p.ncmax + r] = sv;
    if (s == 0) {  // d_r = -J_r v0 - slack_r
        const double* blk = p.v0 + (size_t)p.c_knot[r] * d.nkp;
        double jv = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double nk_ = p.c_n[3 * r + k];
            if (nk_ == 0.0) continue;
            const double* pa = blk + (ar * 3 + k) * 3;
            double ta = p.c_t[3 * r] * pa[0] + p.c_t[3 * r + 1] * pa[1] + p.c_t[3 * r + 2] * pa[2];
            if (br >= 0) {
                const double* pb = blk + (br * 3 + k) * 3;
                ta -= p.c_t[3 * r] * pb[0] + p.c_t[3 * r + 1] * pb[1] + p.c_t[3 * r + 2] * pb[2];
            }
            jv += nk_ * ta;
        }
        p.dv[r] = -jv - p.c_slack[r];
    }
}

// TWINS.  The last control point of a segment and the first of the next are the same point (position continuity: both are u_0 of the
// knot), and where the two segments' SFC boxes share a face -- or a pair's planes coincide -- the two rows are ONE constraint of the reduced
// problem written twice: identical row of S, identical right-hand side.  Either copy alone is a perfectly good active row; both together
// make S_AA exactly singular, the Tikhonov term then splits the multiplier at random and the exchange (block pivoting as well as
// Lawson-Hanson) keeps letting the second copy in and throwing it out again -- at 256 agents ten such pairs ate the round budget, and each
// "dependent" row that was finally banned had been a twin.  twin[i] = the first candidate i is a copy of (or -1); copies never enter A.
// Their slack at any point equals their original's, so the verification sees them satisfied whenever the original is.
__global__ __launch_bounds__(256) void jp_twin(JArgs A) {
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_SOLVE);
    const Pol p = pol_carve(A, mission);
    const int nc = p.cnt[PC_NCAND], i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const double* Si = p.S + (size_t)i * p.ncmax;
    const double sii = Si[i], di = p.dv[i];
    int tw = -1;
    for (int j = 0; j < i && tw < 0; ++j) {
        const double sij = Si[j], sjj = p.S[(size_t)j * p.ncmax + j];
        if (sij > 0.0 && sij * sij >= (1.0 - 1e-12) * sii * sjj && fabs(sii - sjj) <= 1e-12 * sii && fabs(di - p.dv[j]) <= 1e-9 * (1.0 + fabs(di))) tw = j;
    }
    p.twin[i] = tw;
    if (tw >= 0) p.inA[i] = 0;
}

#define JP_LH_REENTRIES 2
// Block principal pivoting control.  mode 0: first active set of a dual solve; mode 1: after z_A and g: infeasibilities, exchange.
// Then the active set is compacted (ascending candidate index) into Aidx.  One workgroup per mission.
__global__ __launch_bounds__(256) void jp_bpp(JArgs A, int mode) {
    const int mission = blockIdx.x, tid = threadIdx.x;
    const Ws w = carve(A, mission);
    POL_GATE(PS_SOLVE);
    const Pol p = pol_carve(A, mission);
    __shared__ double red[8];
    __shared__ int scan[257];
    __shared__ int sh_mode;
    if (p.cnt[PC_BPPDONE]) return;
    const int nc = p.cnt[PC_NCAND];
    if (mode == 0) {
        // Tikhonov term of the dual QP: S_AA is singular whenever active rows are dependent (SFC faces and r_i + r_j planes live on one
        // 0.1 m lattice), and block pivoting needs a P-matrix.  rho z relaxes a row by rho z_i metres -- 1e-9 of the row's own scale,
        // below the 5e-9 the acceptance test allows -- and the primal refinement of jp_check works against the unrelaxed rows
        double smax = 0;
        for (int i = tid; i < nc; i += 256) smax = fmax(smax, p.S[(size_t)i * p.ncmax + i]);
        smax = block_reduce(smax, 1, red);
        if (tid == 0) p.scal[0] = 1e-9 * fmax(smax, 1e-300);
    }
    if (mode == 1 && p.cnt[PC_MODE] == 1) {
        // BLOCK LAWSON-HANSON (from the best iterate block pivoting reached, when that did not converge): z stays feasible and the dual
        // objective falls monotonically, whatever the rank of S_AA.  y = the subspace minimiser on A (jp_z), g = S y - d (jp_g).
        //   y >= 0:  z = y; no inactive row with g < -tol -> done, otherwise the `room` most violated rows enter with z = 0.  A row that has
        //            entered JP_LH_REENTRIES + 1 times and was stepped out again each time is numerically dependent on the active ones
        //            (its subspace multiplier comes out <= 0 although its gradient says "enter": Lawson-Hanson's classic stall at a
        //            degenerate vertex, here 16 of the 20 refused maps of the 64-agent sweep ended that way with ONE such row): it stays
        //            out, and whether the point is acceptable without it is for the verification to say
        //   else  :  step back z += alpha (y - z) with the largest alpha that keeps z >= 0; every row that reaches zero leaves A
        double zmax = 0, ymin = 0;
        for (int i = tid; i < nc; i += 256)
            if (p.inA[i]) zmax = fmax(zmax, fmax(fabs(p.z[i]), fabs(p.y[i]))), ymin = fmin(ymin, p.y[i]);
        zmax = block_reduce(zmax, 1, red), ymin = block_reduce(ymin, 2, red);
        const double tolz = 1e-10 * fmax(1.0, zmax), tolg = 5e-10;
        if (tid == 0) {
            p.cnt[PC_LHIT] += 1, p.cnt[PC_BPPIT] += 1;
            if (p.cnt[PC_LHIT] > (w.st[ST_FINAL] != 0.0 ? (int)A.pol_lh_final : (int)A.pol_lh_early)) w.st[ST_PSTATE] = PS_FAILED, p.cnt[PC_REASON] = 3, p.cnt[PC_BPPDONE] = 1;
        }
        if (ymin >= -tolz) {
            double nviol = 0;
            for (int i = tid; i < nc; i += 256) {
                if (p.inA[i]) p.z[i] = fmax(p.y[i], 0.0);
                nviol += (!p.inA[i] && p.twin[i] < 0 && p.flip[i] <= JP_LH_REENTRIES && p.g[i] < -tolg) ? 1.0 : 0.0;
            }
            nviol = block_reduce(nviol, 0, red);
            if (tid == 0) p.cnt[PC_NINF] = (int)nviol;
            if (nviol == 0.0) {
                if (tid == 0) {
                    p.cnt[PC_BPPDONE] = 1;
                    if (w.st[ST_PSTATE] == (double)PS_SOLVE) w.st[ST_PSTATE] = PS_PRIMAL, p.cnt[PC_ROUND] = 0, p.cnt[PC_REFINE] = 0;
                }
                return;
            }
            // few violated rows left: ONE row per round, the classic Lawson-Hanson step, for which the entering row's subspace multiplier is
            // positive in exact arithmetic -- a row that entered alone and was stepped out again is what the re-entry count is about (rows
            // that enter in a block can come out negative legitimately, and do: banning those refused 11 maps with real violations)
            const bool single = nviol <= 8.0 || p.cnt[PC_LHIT] > 40;  // (... or block entries have gone round in circles: 256 agents, 17 -> 11 -> 6 rows in and out with period three)
            const int room = single ? 1 : max(8, p.cnt[PC_NA] / 16);
            for (int i = tid; i < nc; i += 256) {
                if (p.inA[i] || p.twin[i] >= 0 || p.flip[i] > JP_LH_REENTRIES || !(p.g[i] < -tolg)) continue;
                const double gi = p.g[i];
                int rank = 0;
                for (int j = 0; j < nc && rank < room; ++j)
                    if (!p.inA[j] && p.twin[j] < 0 && p.flip[j] <= JP_LH_REENTRIES && p.g[j] < -tolg && (p.g[j] < gi || (p.g[j] == gi && j < i))) rank++;
                if (rank < room) p.mark[i] = 1;
            }
            __syncthreads();
            for (int i = tid; i < nc; i += 256)
                if (p.mark[i]) p.inA[i] = 1, p.mark[i] = 0, p.z[i] = 0.0, p.flip[i] += single ? 1 : 0;
        } else {
            double alpha = 1.0;
            for (int i = tid; i < nc; i += 256)
                if (p.inA[i] && p.y[i] < -tolz) alpha = fmin(alpha, p.z[i] / (p.z[i] - p.y[i]));
            alpha = block_reduce(alpha, 2, red);
            if (!(alpha >= 0)) alpha = 0;
            double nout = 0;
            for (int i = tid; i < nc; i += 256) {
                if (!p.inA[i]) continue;
                const double zn = p.z[i] + alpha * (p.y[i] - p.z[i]);
                if (p.y[i] < -tolz && zn <= 1e-14 * fmax(1.0, zmax))
                    p.inA[i] = 0, p.z[i] = 0.0, nout += 1.0;
                else
                    p.z[i] = fmax(zn, 0.0);
            }
            nout = block_reduce(nout, 0, red);
            if (tid == 0) p.cnt[PC_NINF] = (int)nout;
        }
        __syncthreads();
    } else if (mode == 1) {
        double zmax = 0, dmax = 0;
        for (int i = tid; i < nc; i += 256) zmax = fmax(zmax, p.inA[i] ? fabs(p.z[i]) : 0.0), dmax = fmax(dmax, fabs(p.dv[i]));
        zmax = block_reduce(zmax, 1, red), dmax = block_reduce(dmax, 1, red);
        // tolerances a decade inside the acceptance test of jp_check (multipliers >= -1e-9 max(1, z_max); g is the row's slack at the
        // primal step, accepted down to -5e-9 m): tighter ones make the exchange chase the rounding noise of dependent rows
        const double tolz = 1e-10 * fmax(1.0, zmax), tolg = 5e-10;
        (void)dmax;
        double ninf_d = 0;
        int last_inf = -1;
        // a row that has changed sides more than six times is numerically dependent on the active ones (Lawson-Hanson's "banned" rows in
        // qp_polish.inc): it stays out; if that leaves a real violation the verification refuses the point
        for (int i = tid; i < nc; i += 256) {
            if (p.flip[i] > 6 || p.twin[i] >= 0) {
                p.inA[i] = 0;
                continue;
            }
            const bool inf = p.inA[i] ? p.z[i] < -tolz : p.g[i] < -tolg;
            if (inf) ninf_d += 1.0, last_inf = i;
        }
        const int ninf = (int)block_reduce(ninf_d, 0, red);
        const int imax = (int)block_reduce((double)last_inf, 1, red);
        if (tid == 0) {
            int m = 0;  // 0 converged, 1 block exchange, 2 single exchange (largest index)
            p.cnt[PC_NINF] = ninf, p.cnt[PC_BPPIT] += 1;
            if (ninf == 0)
                m = 0;
            else if (ninf < p.cnt[PC_BEST])
                p.cnt[PC_BEST] = ninf, p.cnt[PC_PLEFT] = 6, m = 3;   // (3: a new best iterate, kept for the fallback below; then as 1)
            else if (p.cnt[PC_PLEFT] > 0)
                p.cnt[PC_PLEFT] -= 1, m = 1;
            else
                m = 4;   // no progress for six rounds (the exchange oscillates on dependent rows): block Lawson-Hanson from the best iterate
            if (p.cnt[PC_BPPIT] > 40 && m != 0) m = 4;
            sh_mode = m;
        }
        __syncthreads();
        int m = sh_mode;
        if (m == 3) {
            for (int i = tid; i < nc; i += 256) p.bestA[i] = p.inA[i], p.bestz[i] = p.z[i];
            m = 1;
        }
        if (m == 4) {
            for (int i = tid; i < nc; i += 256) {
                const bool in = p.bestA[i] != 0 && p.bestz[i] > 0.0;
                p.inA[i] = in, p.z[i] = in ? p.bestz[i] : 0.0, p.y[i] = p.z[i], p.flip[i] = 0;  // (flip now counts entries into A)
            }
            if (tid == 0) p.cnt[PC_MODE] = 1, p.cnt[PC_LHIT] = 0;
            __syncthreads();
            m = 5;  // (straight to the compaction)
        }
        if (m == 0) {
            if (tid == 0) {
                p.cnt[PC_BPPDONE] = 1;
                if (w.st[ST_PSTATE] == (double)PS_SOLVE) w.st[ST_PSTATE] = PS_PRIMAL, p.cnt[PC_ROUND] = 0, p.cnt[PC_REFINE] = 0;
            }
            return;
        }
        // block exchange: every active row with a negative multiplier leaves; of the violated inactive rows only the `room` MOST violated
        // enter (a verification can return a thousand violated rows of which a few dozen belong to the active set: letting all of
        // them in at once makes S_AA singular, Lawson-Hanson's one-at-a-time rule is the other extreme)
        if (m != 5) {
        const int room = max(32, p.cnt[PC_NA] / 8);
        double nent_d = 0;  // (the ranking below is O(candidates) per row: only when the violated rows do not all fit)
        for (int i = tid; i < nc; i += 256) nent_d += (!p.inA[i] && p.twin[i] < 0 && p.flip[i] <= 6 && p.g[i] < -tolg) ? 1.0 : 0.0;
        const bool must_rank = block_reduce(nent_d, 0, red) > (double)room;
        for (int i = tid; i < nc; i += 256) {
            if (p.flip[i] > 6 || p.twin[i] >= 0) continue;
            const bool act = p.inA[i] != 0;
            const bool inf = act ? p.z[i] < -tolz : p.g[i] < -tolg;
            if (!inf || !(m == 1 || i == imax)) continue;
            if (!act && m == 1 && must_rank) {  // rank among the entering candidates (ties by index)
                const double gi = p.g[i];
                int rank = 0;
                for (int j = 0; j < nc && rank < room; ++j)
                    if (!p.inA[j] && p.twin[j] < 0 && p.flip[j] <= 6 && p.g[j] < -tolg && (p.g[j] < gi || (p.g[j] == gi && j < i))) rank++;
                if (rank >= room) continue;
            }
            p.flip[i] += 1;
            p.mark[i] = 1;  // (marked; applied after every thread has ranked against the OLD membership)
        }
        __syncthreads();
        for (int i = tid; i < nc; i += 256)
            if (p.mark[i]) p.inA[i] = !p.inA[i], p.mark[i] = 0;
        __syncthreads();
        }
    }
    // compaction
    const int per = (nc + 255) / 256, i0 = tid * per, i1 = min(nc, i0 + per);
    int cntl = 0;
    for (int i = i0; i < i1; ++i) cntl += p.inA[i] != 0;
    scan[tid + 1] = cntl;
    if (tid == 0) scan[0] = 0;
    __syncthreads();
    if (tid == 0)
        for (int i = 1; i <= 256; ++i) scan[i] += scan[i - 1];
    __syncthreads();
    int o = scan[tid];
    const bool lh = p.cnt[PC_MODE] == 1;
    for (int i = i0; i < i1; ++i) {
        if (p.inA[i]) p.Aidx[o++] = i;
        if (!lh) p.z[i] = 0.0;   // (block pivoting: the next solve writes z; Lawson-Hanson: z is the feasible iterate, the solve writes y)
    }
    if (tid == 0) {
        const int nA = scan[256];
        p.cnt[PC_NA] = nA, p.cnt[PC_NBLK] = (nA + JT - 1) / JT;
        if (nA == 0) {
            p.cnt[PC_BPPDONE] = 1;
            if (w.st[ST_PSTATE] == (double)PS_SOLVE) w.st[ST_PSTATE] = PS_PRIMAL, p.cnt[PC_ROUND] = 0, p.cnt[PC_REFINE] = 0;
        }
    }
}

// W[p0] <- S_AA + rho I (tiles I >= J feed the sweep), G <- the same with both triangles (kept for the iterative refinement of the dual
// solves), tile-major, identity padding.  One workgroup per tile of the full square.
__global__ __launch_bounds__(256) void jp_gather(JArgs A) {
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_SOLVE);
    const Pol p = pol_carve(A, mission);
    if (p.cnt[PC_BPPDONE]) return;
    const int nA = p.cnt[PC_NA], nblk = p.cnt[PC_NBLK];
    if ((int)blockIdx.x >= nblk * nblk) return;
    const int I = blockIdx.x / nblk, J = blockIdx.x % nblk;
    double* X = (nblk & 1) ? p.W1 : p.W0;
    const size_t to = ((size_t)I * nblk + J) * JTT;
    const double rho = p.scal[0];
    for (int i = threadIdx.x; i < JTT; i += 256) {
        const int r = 64 * I + (i >> 6), c = 64 * J + (i & 63);
        double v;
        if (r < nA && c < nA) {
            v = p.S[(size_t)p.Aidx[r] * p.ncmax + p.Aidx[c]];
            if (r == c) v += rho;
        } else
            v = r == c ? 1.0 : 0.0;
        p.G[to + i] = v;
        if (I >= J) X[to + i] = v;
    }
}

// products with the gathered matrices in the compact index space of the active set.  One workgroup per 16-row slab; dynamic LDS: the
// input vector.   mode 0: z_A = W d_A     1: r_A = d_A - G z_A     2: z_A += W r_A     3: z_A += W (-e_A)  (primal refinement)
__global__ __launch_bounds__(256) void jp_z(JArgs A, int mode) {
    const int mission = blockIdx.y, tid = threadIdx.x;
    const Ws w = carve(A, mission);
    if (w.st[ST_STATE] != 0.0 || w.st[ST_GO] == 0.0) return;
    const Pol p = pol_carve(A, mission);
    if (mode == 3) {
        if (w.st[ST_PSTATE] != (double)PS_PRIMAL || !p.cnt[PC_REFINE]) return;
    } else if (w.st[ST_PSTATE] != (double)PS_SOLVE || p.cnt[PC_BPPDONE])
        return;
    const int nA = p.cnt[PC_NA], nblk = p.cnt[PC_NBLK], nAp = nblk * JT;
    if ((int)blockIdx.x * 16 >= nAp) return;
    extern __shared__ double vsh[];
    double* sol = (mode != 3 && p.cnt[PC_MODE] == 1) ? p.y : p.z;  // the dual solves' output: the iterate itself (pivoting) / the subspace minimiser
    for (int i = tid; i < nAp; i += 256) {
        double v = 0;
        if (i < nA) v = mode == 0 ? p.dv[p.Aidx[i]] : (mode == 1 ? sol[p.Aidx[i]] : (mode == 2 ? p.rA[i] : -p.e[p.Aidx[i]]));
        vsh[i] = v;
    }
    __syncthreads();
    const int row = blockIdx.x * 16 + (tid >> 4), l16 = tid & 15;
    const double* Mx = mode == 1 ? p.G : p.W0;
    const double* rp = Mx + ((size_t)(row >> 6) * nblk) * JTT + (size_t)(row & 63) * JT + 4 * l16;
    double acc = 0;
    for (int Jt = 0; Jt < nblk; ++Jt) {
        const d4 m = *reinterpret_cast<const d4*>(rp + (size_t)Jt * JTT);
        const double* vv = vsh + 64 * Jt + 4 * l16;
        acc += m[0] * vv[0] + m[1] * vv[1] + m[2] * vv[2] + m[3] * vv[3];
    }
    acc += __shfl_xor(acc, 8), acc += __shfl_xor(acc, 4), acc += __shfl_xor(acc, 2), acc += __shfl_xor(acc, 1);
    if (l16 == 0 && row < nA) {
        const int q = p.Aidx[row];
        if (mode == 0)
            sol[q] = acc;
        else if (mode == 1)
            p.rA[row] = p.dv[q] - acc;
        else
            sol[q] += acc;
    }
}

// g_i = sum_{b in A} S[i][b] z_b - d_i for every candidate: one wave per candidate
__global__ __launch_bounds__(256) void jp_g(JArgs A) {
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_SOLVE);
    const Pol p = pol_carve(A, mission);
    if (p.cnt[PC_BPPDONE]) return;
    const int nc = p.cnt[PC_NCAND], nA = p.cnt[PC_NA];
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nc) return;
    const double* Sr = p.S + (size_t)i * p.ncmax;
    const double* sol = p.cnt[PC_MODE] == 1 ? p.y : p.z;
    double acc = 0;
    for (int b = lane; b < nA; b += 64) {
        const int q = p.Aidx[b];
        acc += Sr[q] * sol[q];
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) p.g[i] = acc - p.dv[i];
}

// jz = J_A' z in reduced space: one thread per (knot, agent, dim), a pass over the active rows (fixed order: reproducible)
__global__ __launch_bounds__(256) void jp_jz(JArgs A) {
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_PRIMAL);
    const Pol p = pol_carve(A, mission);
    const JDims d = jdims(A.S.N, A.S.Mk[mission]);
    const int nu = 3 * A.S.N, it = blockIdx.x * 256 + threadIdx.x;
    if (it >= d.nj * nu) return;
    const int jj = it / nu, u = it % nu, x = u / 3, k = u % 3;
    const int nA = p.cnt[PC_NA];
    double a0 = 0, a1 = 0, a2 = 0;
    for (int b = 0; b < nA; ++b) {
        const int q = p.Aidx[b];
        if (p.c_knot[q] != jj) continue;
        const double sg = p.c_a[q] == x ? 1.0 : (p.c_b[q] == x ? -1.0 : 0.0);
        if (sg == 0.0) continue;
        const double cf = sg * p.c_n[3 * q + k] * p.z[q];
        a0 += cf * p.c_t[3 * q], a1 += cf * p.c_t[3 * q + 1], a2 += cf * p.c_t[3 * q + 2];
    }
    double* o = p.jz + (size_t)jj * d.nkp + u * 3;
    o[0] = a0, o[1] = a1, o[2] = a2;
}

// dx = F du (control space, into w.dx: free while the polish runs), and the raw candidate counter cleared for the verification
__global__ __launch_bounds__(256) void jp_dx(JArgs A) {
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_PRIMAL);
    const Pol p = pol_carve(A, mission);
    const JDims d = jdims(A.S.N, A.S.Mk[mission]);
    const int nu = 3 * A.S.N, it = blockIdx.x * 256 + threadIdx.x;
    if (it == 0) p.cnt[PC_NRAW] = 0;
    if (it >= d.nj * nu) return;
    const int j = it / nu + 1, u = it % nu;
    const double* uu = p.du + (size_t)(j - 1) * d.nkp + u * 3;
    const double* L = w.Lk + 9 * j;
    const double u0 = uu[0], u1 = uu[1], u2 = uu[2];
    double* o = w.dx + (size_t)u * d.oq + 6 * (j - 1) + 3;
    o[0] = L[0] * u0 + L[1] * u1 + L[2] * u2;
    o[1] = L[3] * u0 + L[4] * u1 + L[5] * u2;
    o[2] = L[6] * u0 + L[7] * u1 + L[8] * u2;
    o[3] = u0, o[4] = u1, o[5] = u2;
}

// after the verification sweep: accept / refine the multipliers / extend the candidate set / give up
__global__ __launch_bounds__(256) void jp_check(JArgs A) {
    const int mission = blockIdx.x, tid = threadIdx.x;
    const Ws w = carve(A, mission);
    POL_GATE(PS_PRIMAL);
    const Pol p = pol_carve(A, mission);
    __shared__ double red[8];
    const JDims d = jdims(A.S.N, A.S.Mk[mission]);
    const int nsw = A.S.N * d.nch;
    const double vmax = red_final(red_slot(w, A.L, RS_VERIFY, 0), nsw, 1, 0.0, red);
    const int nA = p.cnt[PC_NA], nnew = p.cnt[PC_NRAW];
    double emax = 0, zmin = 0, zmax = 0;
    for (int b = tid; b < nA; b += 256) {
        const int q = p.Aidx[b];
        emax = fmax(emax, fabs(p.e[q])), zmin = fmin(zmin, p.z[q]), zmax = fmax(zmax, p.z[q]);
    }
    emax = block_reduce(emax, 1, red), zmin = block_reduce(zmin, 2, red), zmax = block_reduce(zmax, 1, red);
    double bad = 0;  // anything not finite in the multipliers or the step: the attempt is void (comparisons with NaN would "accept")
    for (int b = tid; b < nA; b += 256) bad += (p.z[p.Aidx[b]] - p.z[p.Aidx[b]] != 0.0) ? 1.0 : 0.0;
    for (int i = tid; i < d.nj * d.nkp; i += 256) bad += (p.du[i] - p.du[i] != 0.0) ? 1.0 : 0.0;
    bad = block_reduce(bad, 0, red);
    if (tid != 0) return;
    p.cnt[PC_REFINE] = 0;
    const int round = p.cnt[PC_ROUND];
    if (bad != 0.0) {
        w.st[ST_PSTATE] = PS_FAILED, p.cnt[PC_REASON] = 7;
        return;
    }
    if (nnew > 0) {  // rows outside the candidate set came out violated: extend S and solve the dual again
        // ... unless they are MANY: the candidate set of this iterate is far from the active set (an early attempt), the interior-point
        // method goes on and the next attempt starts from a better one
        if (p.cnt[PC_OUTER] >= 8 || nnew + p.cnt[PC_NCAND] > p.ncmax)
            w.st[ST_PSTATE] = PS_FAILED, p.cnt[PC_REASON] = 4;
        else
            w.st[ST_PSTATE] = PS_SOLVE, p.cnt[PC_OUTER] += 1, p.cnt[PC_BPPDONE] = 0, p.cnt[PC_BEST] = 0x7fffffff, p.cnt[PC_PLEFT] = 10;
        // (a dual solve that the Lawson-Hanson rounds have just finished gets a fresh share of the round budget for the few new rows,
        // staying with single entries: the 256-agent mission converged at round 148 of 160, found 12 new rows and ran out at 160)
        if (p.cnt[PC_MODE] == 1 && p.cnt[PC_LHIT] > 41) p.cnt[PC_LHIT] = 41;
        return;
    }
    if (vmax <= (round == 3 ? A.pol_vtol : 5e-9) && zmin >= -1e-9 * fmax(1.0, zmax) && (emax < 1e-12 || round == 3)) {
        w.st[ST_PSTATE] = PS_ACCEPTED;
        w.st[ST_KKT] = fmax(fmax(vmax, 0.0), fmax(0.0, -zmin) / fmax(1.0, zmax));
        return;
    }
    if (A.trace && round == 3) {
        printf("[jqp]   check mission %d: vmax %.3e zmin %.3e zmax %.3e emax %.3e nA %d ptau %.1e outer %d\n", mission, vmax, zmin, zmax, emax, nA, w.st[ST_PTAU], p.cnt[PC_OUTER]);
        int t = -1;
        for (int q = 0; q < p.cnt[PC_NCAND]; ++q)
            if (t < 0 || p.e[q] < p.e[t]) t = q;
        if (t >= 0)
            printf("[jqp]     worst candidate %d of %d: row %d a %d b %d knot %d inA %d twin %d flip %d e %.3e g %.3e z %.3e S_tt %.3e\n", t, p.cnt[PC_NCAND], p.c_row[t],
                   p.c_a[t], p.c_b[t], p.c_knot[t], p.inA[t], p.twin[t], p.flip[t], p.e[t], p.g[t], p.z[t], p.S[(size_t)t * p.ncmax + t]);
    }
    if (vmax <= 5e-9 && (emax < 1e-12 || round == 3) && p.cnt[PC_OUTER] < 8) {
        // feasible, but the refinement against the actual residuals has turned a few multipliers negative (by more than the test allows):
        // those rows leave the active set and the dual is solved again from this (otherwise feasible) iterate by the Lawson-Hanson rounds
        const double zt = -1e-9 * fmax(1.0, zmax);
        for (int b = 0; b < nA; ++b) {
            const int q = p.Aidx[b];
            if (p.z[q] < zt) p.inA[q] = 0, p.z[q] = 0.0;
            else p.z[q] = fmax(p.z[q], 0.0), p.y[q] = p.z[q];
        }
        int o = 0;
        const int nc = p.cnt[PC_NCAND];
        for (int i = 0; i < nc; ++i)
            if (p.inA[i]) p.Aidx[o++] = i;
        p.cnt[PC_NA] = o, p.cnt[PC_NBLK] = (o + JT - 1) / JT;
        p.cnt[PC_MODE] = 1, p.cnt[PC_BPPDONE] = 0, p.cnt[PC_OUTER] += 1;
        if (p.cnt[PC_LHIT] > 41) p.cnt[PC_LHIT] = 41;
        w.st[ST_PSTATE] = PS_SOLVE;
        return;
    }
    if (round == 3 && p.cnt[PC_OUTER] < 8) {
        // MODEL AND MEASUREMENT DISAGREE.  The exchange decides with g = S z - d, the slack of a row at the primal step as the dual model
        // predicts it (S = J K0^-1 J' from the explicit inverse R of the K0 chain); the verification MEASURES that slack (e) at the step
        // the chain factor produced.  Two roundings of K0^-1 -- K0's condition number grows with the number of knots -- differ by ~1e-7
        // relative, i.e. by micrometres where the multipliers are of order one: an inactive row can be violated by 1e-6 m while the model
        // holds it satisfied by 5e-6 m, and then nothing ever lets it in (missions with M = 39..41: mission_64agents_20.json).  The
        // refinement of the active rows is iterative refinement against the measurement; the same correction applied to the INACTIVE
        // candidates' right-hand side, d_q += g_q - e_q, makes the model agree with the measurement at this point, and the Lawson-Hanson
        // rounds go on from here with rows that are really violated entering.
        int nfix = 0;
        const int nc = p.cnt[PC_NCAND];
        for (int q = 0; q < nc; ++q)
            if (!p.inA[q] && p.twin[q] < 0 && p.e[q] < -5e-9 && p.g[q] - p.e[q] > 1e-9) nfix++;
        if (nfix > 0) {
            for (int q = 0; q < nc; ++q)
                if (!p.inA[q] && p.twin[q] < 0) p.dv[q] += p.g[q] - p.e[q], p.flip[q] = 0;
            for (int b = 0; b < nA; ++b) {
                const int q = p.Aidx[b];
                p.z[q] = fmax(p.z[q], 0.0), p.y[q] = p.z[q];
            }
            p.cnt[PC_MODE] = 1, p.cnt[PC_BPPDONE] = 0, p.cnt[PC_OUTER] += 1;
            if (p.cnt[PC_LHIT] > 41) p.cnt[PC_LHIT] = 41;
            w.st[ST_PSTATE] = PS_SOLVE;
            return;
        }
    }
    if (A.pol_adtau && round == 3 && (emax > 5e-9 || vmax > A.pol_vtol) && w.st[ST_PTAU] > 1e-5 && p.cnt[PC_OUTER] < 8) {
        // an ACTIVE row keeps a residual that three refinement steps do not touch: the rank-revealing inverse has deleted it as a linear
        // combination of the rows before it (pivot below pol_tau of its diagonal), but it is not consistent with them to the acceptance
        // tolerance -- it was only NEARLY dependent.  The deletion threshold of this mission is tightened by two orders of magnitude and
        // the dual is solved again from the same active set (the row now takes part in the elimination; if its multiplier comes out
        // negative it leaves by the Lawson-Hanson rounds).  The threshold so adapts to the problem instead of being a constant that has
        // to suit every map: a row is treated as dependent only while that is harmless.
        // The same holds for a row the Lawson-Hanson rounds have BANNED (it entered alone, was deleted by the inverse -- multiplier zero --
        // and stepped out again, three times) and that is violated at the point found without it: with the tighter threshold it is
        // eliminated like any other row when it enters, its multiplier is the subspace minimiser's, and the ratio test of the step back
        // drops the row it really replaces.  Every ban is lifted.
        w.st[ST_PTAU] *= 1e-2;
        for (int b = 0; b < nA; ++b) {
            const int q = p.Aidx[b];
            p.z[q] = fmax(p.z[q], 0.0), p.y[q] = p.z[q];
        }
        for (int q = 0; q < p.cnt[PC_NCAND]; ++q) p.flip[q] = 0;
        p.cnt[PC_MODE] = 1, p.cnt[PC_BPPDONE] = 0, p.cnt[PC_OUTER] += 1;
        if (p.cnt[PC_LHIT] > 41) p.cnt[PC_LHIT] = 41;
        w.st[ST_PSTATE] = PS_SOLVE;
        return;
    }
    if (round == 3 && zmin >= -1e-9 * fmax(1.0, zmax) && p.cnt[PC_OUTER] < 8) {
        // multipliers fine, but a candidate row the dual solve kept OUT is violated: it was banned as dependent on the active rows (its
        // subspace multiplier came out negative every time it entered).  Where it is nearly parallel to ONE active row (correlation above
        // 0.99 in the K0^-1 metric: the neighbouring control point under an almost identical plane), the two are alternatives, and the
        // exchange picked the wrong one: swap them and solve again.
        const int nc = p.cnt[PC_NCAND];
        int t = -1;
        for (int q = 0; q < nc; ++q)
            if (!p.inA[q] && p.twin[q] < 0 && p.e[q] < -5e-9 && (t < 0 || p.e[q] < p.e[t])) t = q;
        if (t >= 0) {
            int sbest = -1;
            double cbest = 0.99;
            const double stt = p.S[(size_t)t * p.ncmax + t];
            for (int b = 0; b < nA; ++b) {
                const int q = p.Aidx[b];
                const double stq = p.S[(size_t)t * p.ncmax + q];
                const double cc = stq > 0.0 ? stq * stq / (stt * p.S[(size_t)q * p.ncmax + q]) : 0.0;
                if (cc > cbest) cbest = cc, sbest = q;
            }
            if (sbest >= 0) {
                p.inA[t] = 1, p.z[t] = fmax(p.z[sbest], 0.0), p.y[t] = p.z[t], p.flip[t] = 0;
                p.inA[sbest] = 0, p.z[sbest] = 0.0, p.y[sbest] = 0.0, p.flip[sbest] = JP_LH_REENTRIES + 1;
                for (int b = 0; b < nA; ++b) {
                    const int q = p.Aidx[b];
                    if (p.inA[q]) p.z[q] = fmax(p.z[q], 0.0), p.y[q] = p.z[q];
                }
                int o = 0;
                for (int i = 0; i < nc; ++i)
                    if (p.inA[i]) p.Aidx[o++] = i;
                p.cnt[PC_NA] = o, p.cnt[PC_NBLK] = (o + JT - 1) / JT;
                p.cnt[PC_MODE] = 1, p.cnt[PC_BPPDONE] = 0, p.cnt[PC_OUTER] += 1;
                if (p.cnt[PC_LHIT] > 41) p.cnt[PC_LHIT] = 41;
                w.st[ST_PSTATE] = PS_SOLVE;
                return;
            }
        }
    }
    if (round == 3) {
        w.st[ST_PSTATE] = PS_FAILED, p.cnt[PC_REASON] = 5;
        return;
    }
    p.cnt[PC_ROUND] = round + 1, p.cnt[PC_REFINE] = 1;
}

// accepted: x += dx, control points with an active SFC bound snapped onto their faces
__global__ __launch_bounds__(256) void jp_apply(JArgs A, int phase) {
    const DevSession& S = A.S;
    const int mission = blockIdx.y;
    const Ws w = carve(A, mission);
    POL_GATE(PS_ACCEPTED);
    const Pol p = pol_carve(A, mission);
    const int N = S.N, M = S.Mk[mission], MS = S.M;
    double* ctrl = S.ctrl + (size_t)mission * N * 3 * 6 * MS;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (phase == 0) {
        if (i < N * 3 * 6 * M) ctrl[i] += w.dx[i];
    } else if (i < p.cnt[PC_NA]) {
        const int q = p.Aidx[i];
        if (p.c_snap[q] >= 0 && p.z[q] > 0) ctrl[p.c_snap[q]] = p.c_snapv[q];
    }
}

// end of a polish attempt
__global__ void jp_end(JArgs A) {
    const int mission = blockIdx.x;
    const Ws w = carve(A, mission);
    if (threadIdx.x != 0 || w.st[ST_STATE] != 0.0 || w.st[ST_GO] == 0.0) return;
    const Pol p = pol_carve(A, mission);
    if (w.st[ST_PSTATE] == (double)PS_ACCEPTED)
        w.st[ST_STATE] = 1.0, w.st[ST_POLISHED] = 1.0;
    else if (w.st[ST_FINAL] != 0.0) {
        if (w.st[ST_CONT] < (double)JQ_MAX_CONT && w.st[ST_ITER] < JQ_MAX_ITERS - 1)
            w.st[ST_CONT] += 1.0, w.st[ST_FINAL] = 0.0;  // refused: another decade of the interior-point method, then again (jq_ctrl(1))
        else
            w.st[ST_STATE] = 1.0, w.st[ST_REASON] = 100.0 + p.cnt[PC_REASON];  // converged, not polished (why)
    }
    w.st[ST_GO] = 0.0, w.st[ST_PSTATE] = PS_IDLE;
}
