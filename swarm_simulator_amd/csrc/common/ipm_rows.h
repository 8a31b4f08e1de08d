// ipm_rows.h — the arithmetic of ONE inequality row g . x <= h of the primal-dual interior-point method, stated once for the batch QP
// (kernels/qp.hip, qp_polish.inc) and the grid-wide joint QP (kernels/jqp.hip, jqp_polish.inc): the Newton weight, the
// predictor / affine / corrected (Mehrotra, Gondzio) pieces of a row, its accumulation into a control point's packed 3x3, the two copies of
// a pair row, the polish's candidate rule, and the 3x3-block tridiagonal K0 chain of the polish.  Pure functions of scalars and small
// arrays: where (s, z) come from, where results go and what is reduced stays with the sweeps.  Plain C++17, no HIP runtime include.
// IPM_ROW functions are host + device functions under hipcc and inline functions under g++ (tests/ipm_rows/rows_main.cpp).
//
// Floating point, said here and nowhere else: these rules are judged by tolerance.  Multiply-adds may fuse -- clang gets
// `#pragma clang fp contract(fast)` below, which holds for the rest of the translation unit --, so only qp.hip, jqp.hip and their .inc
// files include this header; ecbs.hip, edt.hip, corridor.hip and the contract(off) region of traj.hip never do.  Every formula keeps
// its order of operations: the planned control points are compared bit for bit across builds.
//
// A row's state is (s, z) > 0 with residual rg = s - slack (slack = h - g . x), ga = g . dx_aff, gd = g . dx, dreg the dual
// regularisation.  The Newton system of a row (the CPU checker of the tests states the same system independently):
//   affine      z dsa + s dza = -s z                          ga + dsa - dreg dza = -rg
//   corrected   s dz  + z ds  = -(s z + cc - sigma_mu - tt)   gd + ds  - dreg dz  = -rg        cc = dsa dza, tt = the row's target shift
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define IPM_ROW __host__ __device__ inline __attribute__((always_inline))
#define IPM_TABLE __constant__
#else
#define IPM_ROW inline
#define IPM_TABLE const
#endif
#if defined(__clang__)
#pragma clang fp contract(fast)
#endif

namespace ipm {

// Q_base (rbp_planner.hpp:330-335) = int_0^1 B'''_i B'''_j
static IPM_TABLE double Qbase[36] = {720,  -1800, 1200,  0,     0,     -120, -1800, 4800,  -3600, 0,     600,   0,
                                     1200, -3600, 3600,  -1200, 0,     0,    0,     0,     -1200, 3600,  -3600, 1200,
                                     0,    600,   0,     -3600, 4800,  -1800, -120, 0,     0,     1200,  -1800, 720};
// the pair (qi < qj) of N agents in the order of the RSFC arrays
IPM_ROW size_t pair_index(int N, int qi, int qj) { return (size_t)qi * N - (size_t)qi * (qi + 1) / 2 + (qj - qi - 1); }

// 1/x for the row arithmetic: v_rcp_f64 plus two Newton steps in device code (relative error ~1e-16 for normal x > 0; an IEEE division
// costs three times as many instructions: div_scale, div_fmas, div_fixup), the division itself on the host
IPM_ROW double fast_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
#else
    return 1.0 / x;
#endif
}

// ---- the row -------------------------------------------------------------------------------------------------------------
IPM_ROW double weight(double s, double z, double dreg) { return z * fast_rcp(s + dreg * z); }  // = 1 / (s/z + dreg)

// BUILD: Newton weight, the predictor's right-hand-side scalar v (rc / z = s) and the primal residual of the row
struct Build {
    double wgt, v, rg;
};
IPM_ROW Build build(double s, double z, double slack, double dreg) {
    Build b;
    b.rg = s - slack;
    b.wgt = weight(s, z, dreg);
    b.v = -b.wgt * (b.rg - s);
    return b;
}

// step-length term of a direction: max(-ds/s, -dz/z) (the caller takes the reciprocal of the sweep's maximum: no data-dependent division)
IPM_ROW double step_limit(double s, double z, double ds, double dz) { return fmax(-ds * fast_rcp(s), -dz * fast_rcp(z)); }

// AFF: the affine direction of the row, cc = dsa dza, and the corrector's right-hand side, which is affine in sigma mu (only known after
// the sweep's reductions):  v_corr = -wgt (rg - (s z + cc - sigma mu) / z) = v - sigma mu * wz   with wz = wgt / z
struct Affine {
    double dza, dsa, cc, v, wz, lim;
};
IPM_ROW Affine affine(double s, double z, double slack, double ga, double dreg) {
    Affine a;
    const double rg = s - slack;
    const double iz = fast_rcp(z);
    const double wgt = weight(s, z, dreg);
    a.dza = wgt * (ga + rg - s);
    a.dsa = -s - s * a.dza * iz;  // (-s z - s dza) / z
    a.cc = a.dsa * a.dza;
    a.lim = step_limit(s, z, a.dsa, a.dza);
    a.v = -wgt * (rg - s - a.cc * iz);
    a.wz = wgt * iz;
    return a;
}

// the corrected direction of the row, a function of (s, z, ga, gd) alone: the STEP, UPBUILD and GOND sweeps recompute it (and cc with it)
// instead of reading it back.  slack_old: the slack at the point the state belongs to; tt: the row's target shift (0.0: none, exact)
struct Dir {
    double dz, ds;
};
IPM_ROW Dir direction(double s, double z, double slack_old, double ga, double gd, double dreg, double sigma_mu, double tt) {
    Dir d;
    const double rg = s - slack_old;
    const double iz = fast_rcp(z);
    const double w0 = weight(s, z, dreg);
    const double dza = w0 * (ga + rg - s);
    const double cc = (-s - s * dza * iz) * dza;
    const double rcc = s * z + cc - sigma_mu - tt;
    d.dz = w0 * (gd + rg - rcc * iz);
    d.ds = -(rcc + s * d.dz) * iz;
    return d;
}

// UPBUILD: the state after the step, and its complementarity product for the wide-neighbourhood test
struct State {
    double s, z, sz;
};
IPM_ROW State step_state(double s, double z, Dir d, double alpha) {
    State n;
    n.s = s + alpha * d.ds, n.z = z + alpha * d.dz;
    n.sz = n.s * n.z;
    return n;
}

// GOND, Gondzio's centrality corrector: at the trial step length atr the complementarity product of the Mehrotra direction is projected
// onto [0.1, 10] mut; the shift t = projected - actual (not below -10 mut) moves the row's target, and the direction is solved for again
// with rcc - t instead of rcc, i.e. the right-hand side changes by -G'(W t / z): v
struct Gondzio {
    double t, v;
};
IPM_ROW Gondzio gondzio(double s, double z, Dir d, double dreg, double atr, double mut) {
    Gondzio g;
    const double pr = (s + atr * d.ds) * (z + atr * d.dz);
    const double lo = 0.1 * mut, hi = 10.0 * mut;
    g.t = (pr < lo ? lo : (pr > hi ? hi : pr)) - pr;
    g.t = fmax(g.t, -hi);
    g.v = -weight(s, z, dreg) * g.t * fast_rcp(z);
    return g;
}

// KMUL: the row's part of J'W J d, with the weight this iteration's Newton matrix was assembled with
IPM_ROW double kmul(double s, double z, double dreg, double gd) { return weight(s, z, dreg) * gd; }

// ---- polish --------------------------------------------------------------------------------------------------------------
// a row is a candidate for the active set when its multiplier dominates or its slack is gone; the value (> 0) orders the warm start
IPM_ROW double cand_strength(double s, double z) { return (z > s || s < 1e-6) ? fmax(z / s, 1e-300) : 0.0; }
// a row whose slack at the trial point is below this is violated: it joins the candidates and the dual is solved again
constexpr double VERIFY_TOL = -1e-11;

// ---- accumulation of a row with coefficient sg * n of this control point into its packed 3x3 (slots 00, 01, 02, 11, 12, 22) -----------
// (frozen rows carry their sign in n: sg = 1.0, and the multiplication by it folds away exactly)
IPM_ROW void acc_build(double (&S)[6], double (&yv)[3], double (&gz)[3], double wgt, double v, double zo, double sg, double n0, double n1,
                       double n2) {
    S[0] += wgt * n0 * n0, S[1] += wgt * n0 * n1, S[2] += wgt * n0 * n2;
    S[3] += wgt * n1 * n1, S[4] += wgt * n1 * n2, S[5] += wgt * n2 * n2;
    const double zz = sg * zo, vv = sg * v;
    gz[0] += zz * n0, gz[1] += zz * n1, gz[2] += zz * n2;
    yv[0] += vv * n0, yv[1] += vv * n1, yv[2] += vv * n2;
}
// AFF: S[0..2] / S[3..5] hold the two parts of the corrector's right-hand side (v, wz of affine())
IPM_ROW void acc_aff(double (&S)[6], double v, double wz, double sg, double n0, double n1, double n2) {
    const double vv = sg * v, ww = sg * wz;
    S[0] += vv * n0, S[1] += vv * n1, S[2] += vv * n2;
    S[3] += ww * n0, S[4] += ww * n1, S[5] += ww * n2;
}
// KMUL, GOND: G'v alone
IPM_ROW void acc_kmul(double (&S)[6], double v, double sg, double n0, double n1, double n2) {
    const double vv = sg * v;
    S[0] += vv * n0, S[1] += vv * n1, S[2] += vv * n2;
}

// ---- pair rows -----------------------------------------------------------------------------------------------------------
// The row of a pair (lo < hi) is  n . x_lo - n . x_hi <= -rr  and is worked on twice, once per agent's column (a_lo: this side is lo).
// Canonical orientation e = x_hi - x_lo, so that both copies see bit-identical inputs and produce bit-identical slacks (and with them
// bit-identical states).  xa / d: this side's point / direction, xb / f: the other side's.
IPM_ROW double pair_sign(bool a_lo) { return a_lo ? 1.0 : -1.0; }  // the coefficient of x_a in the row is pair_sign * n
// (scalars by value: with the points behind references the compiler selects the operands first and the sweeps need more registers)
IPM_ROW double pair_slack(bool a_lo, double n0, double n1, double n2, double xa0, double xa1, double xa2, double xb0, double xb1, double xb2,
                          double rsum) {
    const double e0 = a_lo ? xb0 - xa0 : xa0 - xb0, e1 = a_lo ? xb1 - xa1 : xa1 - xb1, e2 = a_lo ? xb2 - xa2 : xa2 - xb2;
    return n0 * e0 + n1 * e1 + n2 * e2 - rsum;
}
IPM_ROW double pair_dot(bool a_lo, double n0, double n1, double n2, double d0, double d1, double d2, double f0, double f1, double f2) {  // g . d
    return a_lo ? n0 * (d0 - f0) + n1 * (d1 - f1) + n2 * (d2 - f2) : n0 * (f0 - d0) + n1 * (f1 - d1) + n2 * (f2 - d2);
}

// ---- the K0 chain of the polish ------------------------------------------------------------------------------------------
// K0 = F'(2Q)F per (agent, dim): block tridiagonal with 3x3 blocks D_j and T_{j+1,j} = E_j'.  Its factor, 18 values per knot:
//   f[0..8] = L_jj (lower, row-major) with RECIPROCAL pivots in the diagonal slots (the solves multiply),  f[9..17] = B_jj = T_{j+1,j} L_jj^-T
// The chain is written for a value type T: double for the factor the polish solves its gradient column with, dd (below) for the table of
// the inverse, whose entries must be good to the last bit of a double.
//
// dd: an unevaluated sum h + l of two doubles, |l| <= ulp(h) / 2 (Dekker; error-free sums and fma products, ~106 bits)
struct dd {
    double h, l;
    IPM_ROW dd() : h(0), l(0) {}
    IPM_ROW dd(double x) : h(x), l(0) {}
    IPM_ROW dd(double hh, double ll) : h(hh), l(ll) {}
};
IPM_ROW dd dd_quick(double a, double b) {  // |a| >= |b|
    const double s = a + b;
    return dd(s, b - (s - a));
}
IPM_ROW dd dd_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return dd(s, (a - (s - bb)) + (b - bb));
}
IPM_ROW dd operator+(dd a, dd b) {
    dd s = dd_sum(a.h, b.h);
    const dd t = dd_sum(a.l, b.l);
    s = dd_quick(s.h, s.l + t.h);
    return dd_quick(s.h, s.l + t.l);
}
IPM_ROW dd operator-(dd a) { return dd(-a.h, -a.l); }
IPM_ROW dd operator-(dd a, dd b) { return a + (-b); }
IPM_ROW dd operator*(dd a, dd b) {
    const double p = a.h * b.h;
    return dd_quick(p, fma(a.h, b.h, -p) + (a.h * b.l + a.l * b.h));
}
IPM_ROW dd operator/(dd a, dd b) {
    const double q1 = a.h / b.h;
    dd r = a - b * dd(q1);
    const double q2 = r.h / b.h;
    r = r - b * dd(q2);
    const double q3 = r.h / b.h;
    return dd_quick(q1, q2) + dd(q3);
}
IPM_ROW dd& operator-=(dd& a, dd b) { return a = a - b; }
IPM_ROW bool operator>(dd a, dd b) { return a.h > b.h || (a.h == b.h && a.l > b.l); }
IPM_ROW double k0_sqrt(double a) { return sqrt(a); }
IPM_ROW dd k0_sqrt(dd a) {  // one Newton step on the double's root (a > 0)
    const double x = 1.0 / sqrt(a.h), ax = a.h * x;
    return dd_sum(ax, (a - dd(ax) * dd(ax)).h * (x * 0.5));
}

// k0_factor_step: on entry f = (D_j, E_j) (E_j zero behind the last knot) and Bp = B_{j-1} (zero in front of the first); on exit the
// factor of the knot in f and B_j in Bp.  Returns false when a pivot is not positive.
template <class T>
IPM_ROW bool k0_factor_step(T* f, T (&Bp)[9], bool first) {
    bool ok = true;
    T A[9], Ej[9];
    for (int e = 0; e < 9; ++e) A[e] = f[e], Ej[e] = f[9 + e];
    if (!first)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) A[3 * r + c] -= Bp[3 * r] * Bp[3 * c] + Bp[3 * r + 1] * Bp[3 * c + 1] + Bp[3 * r + 2] * Bp[3 * c + 2];
    const T zero = T(0.0), one = T(1.0);
    if (!(A[0] > zero)) ok = false;
    const T l00 = k0_sqrt(A[0]), l10 = A[3] / l00, l20 = A[6] / l00;
    const T d11 = A[4] - l10 * l10;
    if (!(d11 > zero)) ok = false;
    const T l11 = k0_sqrt(d11), l21 = (A[7] - l20 * l10) / l11;
    const T d22 = A[8] - l20 * l20 - l21 * l21;
    if (!(d22 > zero)) ok = false;
    const T l22 = k0_sqrt(d22);
    f[0] = one / l00, f[1] = zero, f[2] = zero, f[3] = l10, f[4] = one / l11, f[5] = zero, f[6] = l20, f[7] = l21, f[8] = one / l22;
    for (int r = 0; r < 3; ++r) {
        const T o0 = Ej[r], o1 = Ej[3 + r], o2 = Ej[6 + r];  // T_{j+1,j}[r][c] = E_j[3c + r]
        const T x0 = o0 / l00, x1 = (o1 - x0 * l10) / l11, x2 = (o2 - x0 * l20 - x1 * l21) / l22;
        f[9 + 3 * r] = Bp[3 * r] = x0, f[10 + 3 * r] = Bp[3 * r + 1] = x1, f[11 + 3 * r] = Bp[3 * r + 2] = x2;
    }
    return ok;
}
// one knot of L y = b (forward) and of L' x = y (backward): y holds the knot's three values on entry and the result on exit, p the result
// of the knot before (forward) / behind (backward), link whether there is one.  f: the knot's factor (a pointer of any address space).
template <class F, class T>
IPM_ROW void k0_forward_step(F f, bool link, T (&y)[3], const T (&p)[3]) {
    if (link) {
        const F Bm = f - 9;  // B_{j-1}
        y[0] -= Bm[0] * p[0] + Bm[1] * p[1] + Bm[2] * p[2];
        y[1] -= Bm[3] * p[0] + Bm[4] * p[1] + Bm[5] * p[2];
        y[2] -= Bm[6] * p[0] + Bm[7] * p[1] + Bm[8] * p[2];
    }
    y[0] = y[0] * f[0];
    y[1] = (y[1] - f[3] * y[0]) * f[4];
    y[2] = (y[2] - f[6] * y[0] - f[7] * y[1]) * f[8];
}
template <class F, class T>
IPM_ROW void k0_backward_step(F f, bool link, T (&y)[3], const T (&p)[3]) {
    if (link) {
        const F Bm = f + 9;  // y_j -= B_j' y_{j+1}
        y[0] -= Bm[0] * p[0] + Bm[3] * p[1] + Bm[6] * p[2];
        y[1] -= Bm[1] * p[0] + Bm[4] * p[1] + Bm[7] * p[2];
        y[2] -= Bm[2] * p[0] + Bm[5] * p[1] + Bm[8] * p[2];
    }
    y[2] = y[2] * f[8];
    y[1] = (y[1] - f[7] * y[2]) * f[4];
    y[0] = (y[0] - f[3] * y[1] - f[6] * y[2]) * f[0];
}

// ---- G = K0^-1, formed once per mission ------------------------------------------------------------------------------------
// K0 depends on the segment times alone, and everything the polish wants from K0^-1 J' is a contraction of a row's three coefficients with
// 3x3 blocks of G.  Stored: the lower block triangle, block (ja, jb) with ja >= jb row-major at k0g_block(ja, jb); G[jb][ja] = G[ja][jb]'.
IPM_ROW size_t k0g_block(int ja, int jb) { return 9 * ((size_t)ja * (ja + 1) / 2 + jb); }
IPM_ROW size_t k0g_doubles(int nj) { return k0g_block(nj, 0); }
// element (3 ja + r, 3 jb + c) of G, any ja and jb
template <class P>
IPM_ROW double k0g_at(P G, int ja, int r, int jb, int c) {
    return ja >= jb ? G[k0g_block(ja, jb) + 3 * r + c] : G[k0g_block(jb, ja) + 3 * c + r];
}
// t_a' G[ja][jb] t_b, any ja and jb; blk: the stored block of the pair (the larger knot first)
template <class P>
IPM_ROW double k0g_bilinear(P blk, bool a_first, const double (&ta)[3], const double (&tb)[3]) {
    const double (&tr)[3] = a_first ? ta : tb;  // rows of the stored block belong to the larger knot
    const double (&tc)[3] = a_first ? tb : ta;
    return tr[0] * (blk[0] * tc[0] + blk[1] * tc[1] + blk[2] * tc[2]) + tr[1] * (blk[3] * tc[0] + blk[4] * tc[1] + blk[5] * tc[2]) +
           tr[2] * (blk[6] * tc[0] + blk[7] * tc[1] + blk[8] * tc[2]);
}
// Column c of block column jb, rows ja >= jb, solved in place in the table (f: the dd factor of k0_factor_step, G: the table, lo: a
// second array of the table's shape that holds the low halves between the two passes).  The right-hand side is a unit vector: the
// forward pass starts at knot jb (everything in front of it stays zero) and only stores; the backward pass stops at knot jb and fetches
// its knots in blocks of K0_BLK, the next block requested before the current one is worked on, so that a column costs a handful of trips
// to memory and not one per knot.
// Why dd: K0's condition number is 1e10 .. 1e11 at 35 knots.  A column solved in double has a small residual K0 g - e, but its entries
// are only good to ~1e-8 of the largest, and a SYMMETRIC table takes the part above the diagonal from other columns: assembled from
// double solves its residual max|K0 G - I| came out a thousand times that of the columns themselves (3e-5 against 3e-8, unit times).
// With the chain in dd every stored entry is the correctly rounded one, and the table's residual is that of the rounding alone.
constexpr int K0_BLK = 6;
template <class F, class P>
IPM_ROW void k0_inverse_column(F f, int nj, int jb, int c, P G, P lo) {
    dd p[3];
    for (int ja = jb; ja < nj; ++ja) {
        dd y[3];
        if (ja == jb) y[0] = dd(c == 0 ? 1.0 : 0.0), y[1] = dd(c == 1 ? 1.0 : 0.0), y[2] = dd(c == 2 ? 1.0 : 0.0);
        k0_forward_step(f + 18 * ja, ja > jb, y, p);
        const size_t o = k0g_block(ja, jb) + c;
        for (int e = 0; e < 3; ++e) p[e] = y[e], G[o + 3 * e] = y[e].h, lo[o + 3 * e] = y[e].l;
    }
    constexpr int B = K0_BLK;
    dd cur[B][3], nxt[B][3];
    for (int u = 0; u < B; ++u) {
        const int jx = nj - 1 - u >= jb ? nj - 1 - u : jb;
        const size_t o = k0g_block(jx, jb) + c;
        for (int e = 0; e < 3; ++e) cur[u][e] = dd(G[o + 3 * e], lo[o + 3 * e]);
    }
    for (int jt = nj - 1; jt >= jb; jt -= B) {
        for (int u = 0; u < B; ++u) {
            const int jx = jt - B - u >= jb ? jt - B - u : jb;
            const size_t o = k0g_block(jx, jb) + c;
            for (int e = 0; e < 3; ++e) nxt[u][e] = dd(G[o + 3 * e], lo[o + 3 * e]);
        }
        for (int u = 0; u < B; ++u) {
            const int jj = jt - u;
            if (jj >= jb) {
                k0_backward_step(f + 18 * jj, jj + 1 < nj, cur[u], p);
                const size_t o = k0g_block(jj, jb) + c;
                for (int e = 0; e < 3; ++e) p[e] = cur[u][e], G[o + 3 * e] = cur[u][e].h;
            }
        }
        for (int u = 0; u < B; ++u)
            for (int e = 0; e < 3; ++e) cur[u][e] = nxt[u][e];
    }
}
// the diagonal blocks are the only entries the table holds twice: both copies get their mean, and the table is symmetric exactly
template <class P>
IPM_ROW void k0g_symmetrise(P blk) {
    const double a = 0.5 * (blk[1] + blk[3]), b = 0.5 * (blk[2] + blk[6]), c = 0.5 * (blk[5] + blk[7]);
    blk[1] = blk[3] = a, blk[2] = blk[6] = b, blk[5] = blk[7] = c;
}

}  // namespace ipm
