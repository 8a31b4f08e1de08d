// The row arithmetic of common/ipm_rows.h as g++ compiles it, checked against the EQUATIONS it solves (tests/test_ipm_rows.py builds this
// program with the sanitizers and runs it).  No formula of the header is written out again: each check puts the header's outputs into the
// row's Newton system (the header's preamble; oracle/planner.c states the same system independently) and evaluates the residual in long double.
//
// Bound on a residual, derived, not measured:  k * 2^-52 * (sum of the absolute values of the equation's terms),  k = the number of
// rounded double operations on the longest path from the inputs to the outputs that enter the residual (counted beside each check; on the
// host nothing fuses and fast_rcp is one division).  2^-52 is twice the unit roundoff: (1 + u)^k - 1 <= 2 k u for every k here.
//
// The grid: s and z over 1e-9 .. 1e3 in all combinations (s << z and z << s included), dreg 0 and 1e-9, sigma_mu from 0 to s z, the target
// shift tt of both signs, ga and gd of both signs, the row feasible, strictly inside and violated (slack = s, s / 2, 5 s / 4).
// ga and slack are given in units of s.  Reason: the corrected step takes ds from the FIRST equation, ds = -(rcc + s dz) / z, so the second
// equation's residual carries the rounding of cc / z = dsa dza / z, which is (1 + |ga - slack| / s) times that equation's own terms.  A bound
// of the form above can therefore only hold where |ga - slack| = O(s) (here <= 1.95 s); further out the residual of the second equation is
// a property of the elimination order (the oracle's too), not of these functions.
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "common/ipm_rows.h"

using namespace ipm;
typedef long double ld;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (failures < 20) std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static const ld EPS = 0x1p-52L;
static ld A(ld x) { return x < 0 ? -x : x; }
static double worst[16];  // largest residual / bound per equation (printed: how much of its bound each check uses)
// |res| <= k * 2^-52 * terms
#define BOUND(slot, res, k, terms)                                \
    do {                                                          \
        const ld r_ = A(res), b_ = (k) * EPS * (terms);           \
        if (b_ > 0 && (double)(r_ / b_) > worst[slot]) worst[slot] = (double)(r_ / b_); \
        CHECK(r_ <= b_);                                          \
    } while (0)

static void row_equations() {
    const double sv[] = {1e-9, 1e-6, 1e-3, 1.0, 1e3};
    const double dregs[] = {0.0, 1e-9}, sig[] = {0.0, 0.1, 1.0}, tts[] = {-0.5, 0.0, 0.5}, gas[] = {-0.7, 0.3}, gds[] = {-0.7, 1e-4, 0.3};
    const double slk[] = {1.0, 0.5, 1.25}, alphas[] = {0.25, 0.997};
    for (double s : sv) for (double z : sv) for (double dreg : dregs) for (double sl : slk) for (double gau : gas) {
        const double slack = sl * s, ga = gau * s;
        const ld S = s, Z = z, DR = dreg;
        // weight: wgt (s/z + dreg) = 1.   k = 4: dreg * z, s + ., the reciprocal, z * .
        const double wgt = weight(s, z, dreg);
        BOUND(0, wgt * (S / Z + DR) - 1, 4, wgt * (S / Z) + wgt * DR + 1);
        // BUILD: rg = s - slack (k = 1);  predictor v (s/z + dreg) = -(rg - s) (k = 7: the weight 4, rg, rg - s, the product)
        const Build b = build(s, z, slack, dreg);
        CHECK(b.wgt == wgt);
        BOUND(1, b.rg - (S - slack), 1, S + A(slack));
        BOUND(2, b.v * (S / Z + DR) + (b.rg - S), 7, A(b.v) * (S / Z + DR) + A(b.rg) + S);
        // AFF.  first equation  z dsa + s dza = -s z:  k = 4 (s * dza, the reciprocal of z, their product, -s - .), dza as given
        const Affine a = affine(s, z, slack, ga, dreg);
        BOUND(3, Z * a.dsa + S * a.dza + S * Z, 4, A(Z * a.dsa) + A(S * a.dza) + S * Z);
        // second equation  ga + dsa - dreg dza = -rg, rg = s - slack:  k = 12 (rg, ga + rg, . - s, the weight 4, dza, then dsa 4)
        BOUND(4, ga + a.dsa - DR * a.dza + (S - slack), 12, A(ga) + A(a.dsa) + DR * A(a.dza) + S + A(slack));
        // cc = dsa dza (k = 1); the corrector's right-hand side  v (s/z + dreg) = -(rg - s - cc / z)  (k = 11: weight 4, rg, - s, 1 / z,
        // cc / z, the difference, the product, cc itself);  wz z = wgt (k = 6: weight 4, 1 / z, the product)
        BOUND(5, a.cc - (ld)a.dsa * a.dza, 1, A((ld)a.dsa * a.dza));
        BOUND(6, a.v * (S / Z + DR) + (S - slack) - S - a.cc / Z, 11, A(a.v) * (S / Z + DR) + 2 * S + A(slack) + A(a.cc) / Z);
        BOUND(7, a.wz * Z - wgt, 6, A(a.wz) * Z + wgt);
        // step-length term: max(-dsa / s, -dza / z), each k = 2 (the reciprocal, the product)
        {
            const ld l0 = -a.dsa / S, l1 = -a.dza / Z, m = l0 > l1 ? l0 : l1;
            BOUND(8, a.lim - m, 2, A(m));
        }
        for (double sg : sig) for (double ttu : tts) for (double gd : gds) {
            const double sigma_mu = sg * s * z, tt = ttu * s * z;
            // corrected step.  first equation  s dz + z ds = -(s z + cc - sigma_mu - tt):  k = 8 (s z, + cc, - sigma_mu, - tt, s dz, the sum, 1 / z,
            // the product; cc is bit for bit AFF's: the same operations on the same inputs)
            const Dir d = direction(s, z, slack, ga, gd, dreg, sigma_mu, tt);
            BOUND(9, S * d.dz + Z * d.ds + (S * Z + a.cc - sigma_mu - tt), 8, A(S * d.dz) + A(Z * d.ds) + S * Z + A(a.cc) + A(sigma_mu) + A(tt));
            // second equation  gd + ds - dreg dz = -rg:  k = 24 (rg, 1 / z, weight 4, dza 3, cc 4, rcc 4, rcc / z, gd + rg, the difference, dz,
            // s dz, rcc + ., the product with 1 / z)
            BOUND(10, gd + d.ds - DR * d.dz + (S - slack), 24, A(gd) + A(d.ds) + DR * A(d.dz) + S + A(slack));
            // tt = 0.0 is exact: the row without a shift
            if (tt == 0.0) {
                const Dir d0 = direction(s, z, slack, ga, gd, dreg, sigma_mu, 0.0);
                CHECK(d0.dz == d.dz && d0.ds == d.ds);
            }
            // STEP's limit (k = 2 as above)
            {
                const ld l0 = -d.ds / S, l1 = -d.dz / Z, m = l0 > l1 ? l0 : l1;
                BOUND(8, step_limit(s, z, d.ds, d.dz) - m, 2, A(m));
            }
            for (double alpha : alphas) {
                // UPBUILD: new state = old + alpha (ds, dz) (k = 2 each), its product (k = 1)
                const State n = step_state(s, z, d, alpha);
                BOUND(11, n.s - (S + (ld)alpha * d.ds), 2, S + A((ld)alpha * d.ds));
                BOUND(11, n.z - (Z + (ld)alpha * d.dz), 2, Z + A((ld)alpha * d.dz));
                BOUND(11, n.sz - (ld)n.s * n.z, 1, A((ld)n.s * n.z));
                // Gondzio at the trial length alpha: pr + t within [0.1, 10] mut, or t = -10 mut where the floor binds;  k = 6 (atr ds, s + .,
                // atr dz, z + ., the product, projected - pr) on |pr|'s terms
                const double mut = sigma_mu > 1e-3 * s * z ? sigma_mu : 1e-3 * s * z;
                const Gondzio g = gondzio(s, z, d, dreg, alpha, mut);
                const ld ps = S + (ld)alpha * d.ds, pz = Z + (ld)alpha * d.dz, pr = ps * pz;
                const ld tol = 6 * EPS * ((S + A((ld)alpha * d.ds)) * (Z + A((ld)alpha * d.dz)) + 10 * (ld)mut);
                CHECK(g.t >= -10.0 * mut);
                if (g.t == -10.0 * mut) CHECK(pr + g.t >= 10 * (ld)mut - tol);  // (the floor binds only above the window)
                else CHECK(pr + g.t >= 0.1 * (ld)mut - tol && pr + g.t <= 10 * (ld)mut + tol);
                // its right-hand side  v = -w0 t / z:  v z + w0 t = 0, k = 7 (weight 4, the product, 1 / z, the product)
                BOUND(12, g.v * Z + wgt * (ld)g.t, 7, A(g.v) * Z + A(wgt * (ld)g.t));
            }
        }
        // KMUL: v (s/z + dreg) = gd (k = 5)
        for (double gd : gds) BOUND(13, kmul(s, z, dreg, gd) * (S / Z + DR) - gd, 5, A(kmul(s, z, dreg, gd)) * (S / Z + DR) + A(gd));
    }
}

// UPBUILD ends in BUILD at the new state: the sweeps call build() itself on step_state()'s output, nothing to compare but the state; here the
// chain on one row by hand -- the new residual is the new s minus the slack at the new point
static void upbuild_is_build_at_the_new_state() {
    const double s = 0.3, z = 0.02, slack_new = 0.27, gd = 0.05, ga = 0.04, alpha = 0.5, dreg = 1e-9, dregn = 0.0;
    const State n = step_state(s, z, direction(s, z, slack_new + alpha * gd, ga, gd, dreg, 1e-3, 0.0), alpha);
    const Build b = build(n.s, n.z, slack_new, dregn);
    CHECK(b.wgt == weight(n.s, n.z, dregn) && b.rg == n.s - slack_new);
    BOUND(2, b.v * ((ld)n.s / n.z + dregn) + (b.rg - (ld)n.s), 7, A(b.v) * ((ld)n.s / n.z + dregn) + A(b.rg) + n.s);
}

static void candidates() {
    CHECK(cand_strength(1e-7, 0.0) == 1e-300);
    CHECK(cand_strength(0.25, 0.75) == 0.75 / 0.25);
    CHECK(cand_strength(1e-9, 1e3) == 1e3 / 1e-9);
    CHECK(cand_strength(1.0, 0.5) == 0.0);
    CHECK(cand_strength(1e-6, 0.0) == 0.0);  // (the slack test is strict)
    CHECK(VERIFY_TOL == -1e-11);
}

static void accumulators() {
    // normals of distinct primes: every slot's product is a different integer, exact in double
    const double n0 = 2, n1 = 3, n2 = 5, wgt = 7, v = 11, zo = 13;
    for (double sg : {1.0, -1.0}) {
        double S[6] = {100, 200, 300, 400, 500, 600}, yv[3] = {1, 2, 3}, gz[3] = {4, 5, 6};
        acc_build(S, yv, gz, wgt, v, zo, sg, n0, n1, n2);
        CHECK(S[0] == 100 + 7 * 4 && S[1] == 200 + 7 * 6 && S[2] == 300 + 7 * 10 && S[3] == 400 + 7 * 9 && S[4] == 500 + 7 * 15 && S[5] == 600 + 7 * 25);
        CHECK(yv[0] == 1 + sg * 22 && yv[1] == 2 + sg * 33 && yv[2] == 3 + sg * 55);
        CHECK(gz[0] == 4 + sg * 26 && gz[1] == 5 + sg * 39 && gz[2] == 6 + sg * 65);
        double T[6] = {100, 200, 300, 400, 500, 600};
        acc_aff(T, v, wgt, sg, n0, n1, n2);
        CHECK(T[0] == 100 + sg * 22 && T[1] == 200 + sg * 33 && T[2] == 300 + sg * 55 && T[3] == 400 + sg * 14 && T[4] == 500 + sg * 21 && T[5] == 600 + sg * 35);
        double K[6] = {100, 200, 300, 400, 500, 600};
        acc_kmul(K, v, sg, n0, n1, n2);
        CHECK(K[0] == 100 + sg * 22 && K[1] == 200 + sg * 33 && K[2] == 300 + sg * 55 && K[3] == 400 && K[4] == 500 && K[5] == 600);
    }
}

static void pair_rows() {
    // values whose differences and products round: the two copies must still agree to the bit
    const double xlo[3] = {0.1, -2.7, 1.3}, xhi[3] = {1.9, 0.3, 0.7}, dlo[3] = {0.013, -0.7, 0.11}, dhi[3] = {-0.29, 0.031, 0.57};
    const double n0 = 0.6f, n1 = -0.64f, n2 = 0.48f, rsum = 0.15 + 0.15;
    const double s_lo = pair_slack(true, n0, n1, n2, xlo[0], xlo[1], xlo[2], xhi[0], xhi[1], xhi[2], rsum), s_hi = pair_slack(false, n0, n1, n2, xhi[0], xhi[1], xhi[2], xlo[0], xlo[1], xlo[2], rsum);
    CHECK(s_lo == s_hi);
    const double g_lo = pair_dot(true, n0, n1, n2, dlo[0], dlo[1], dlo[2], dhi[0], dhi[1], dhi[2]), g_hi = pair_dot(false, n0, n1, n2, dhi[0], dhi[1], dhi[2], dlo[0], dlo[1], dlo[2]);
    CHECK(g_lo == g_hi);
    // the row is n . x_lo - n . x_hi <= -rr: slack = n . (x_hi - x_lo) - rr (k = 9: 3 differences, 3 products, 2 sums, - rr), g . d likewise (k = 8)
    ld e = 0, ea = 0, g = 0, gabs = 0;
    const double nn[3] = {n0, n1, n2};
    for (int k = 0; k < 3; ++k) {
        e += (ld)nn[k] * ((ld)xhi[k] - xlo[k]), ea += A(nn[k]) * (A(xhi[k]) + A(xlo[k]));
        g += (ld)nn[k] * ((ld)dlo[k] - dhi[k]), gabs += A(nn[k]) * (A(dlo[k]) + A(dhi[k]));
    }
    BOUND(14, s_lo - (e - rsum), 9, ea + rsum);
    BOUND(14, g_lo - g, 8, gabs);
    // opposite coefficients: what the two sides add to their control points cancels
    CHECK(pair_sign(true) == 1.0 && pair_sign(false) == -1.0);
    double Slo[6] = {0, 0, 0, 0, 0, 0}, Shi[6] = {0, 0, 0, 0, 0, 0};
    acc_kmul(Slo, 0.37, pair_sign(true), n0, n1, n2), acc_kmul(Shi, 0.37, pair_sign(false), n0, n1, n2);
    for (int k = 0; k < 3; ++k) CHECK(Slo[k] == -Shi[k] && Slo[k] != 0.0);
    CHECK(pair_index(4, 0, 1) == 0 && pair_index(4, 0, 3) == 2 && pair_index(4, 1, 2) == 3 && pair_index(4, 2, 3) == 5);
}

static void k0_chain() {
    // two knots of a hand-made chain: D (SPD), E = T' between them, a second diagonal block
    const double D1[9] = {4, 1, 0.5, 1, 3, 0.25, 0.5, 0.25, 2}, E1[9] = {0.3, -0.2, 0.1, 0.05, 0.4, -0.1, 0.2, 0.1, 0.3};
    const double D2[9] = {5, -1, 0.2, -1, 4, 0.3, 0.2, 0.3, 3};
    double f[36], Bp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = 0; e < 9; ++e) f[e] = D1[e], f[9 + e] = E1[e], f[18 + e] = D2[e], f[27 + e] = 0.0;
    CHECK(k0_factor_step(f, Bp, true));
    CHECK(k0_factor_step(f + 18, Bp, false));
    ld L[2][9], B[9];
    for (int j = 0; j < 2; ++j)
        for (int e = 0; e < 9; ++e) L[j][e] = (e == 0 || e == 4 || e == 8) ? 1 / (ld)f[18 * j + e] : (ld)f[18 * j + e];  // (reciprocal pivots)
    for (int e = 0; e < 9; ++e) B[e] = f[9 + e];
    CHECK(f[1] == 0 && f[2] == 0 && f[5] == 0);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            ld ll = 0, la = 0, bb = 0, ba = 0, bl = 0, bla = 0;
            for (int k = 0; k < 3; ++k) {
                ll += L[0][3 * r + k] * L[0][3 * c + k], la += A(L[0][3 * r + k] * L[0][3 * c + k]);
                bb += B[3 * r + k] * B[3 * c + k], ba += A(B[3 * r + k] * B[3 * c + k]);
                bl += B[3 * r + k] * L[0][3 * c + k], bla += A(B[3 * r + k] * L[0][3 * c + k]);
            }
            // L L' = D:  k = 10, the path to the last pivot (l00, l20, l10, l10^2, d11, l11 | l20 l10, A7 - ., l21 | l21^2, d22's two
            // differences, the root, the reciprocal)
            BOUND(15, ll - D1[3 * r + c], 10, la + A(D1[3 * r + c]));
            // B L' = T, T[r][c] = E[3c + r]:  k = 8 (the pivots' roots and quotients 5, then two products and differences and a quotient)
            BOUND(15, bl - E1[3 * c + r], 8, bla + A(E1[3 * c + r]));
            // second knot: L L' + B B' = D  (k = 16: the update's three products, two sums and difference on top)
            ld l2 = 0, l2a = 0;
            for (int k = 0; k < 3; ++k) l2 += L[1][3 * r + k] * L[1][3 * c + k], l2a += A(L[1][3 * r + k] * L[1][3 * c + k]);
            BOUND(15, l2 + bb - D2[3 * r + c], 16, l2a + ba + A(D2[3 * r + c]));
        }
    // one knot of the substitutions: L y = b - B p  and  L' x = y - B_next' p, residual of a triangular solve (k = 10: three products and sums
    // of the link, up to two products, two differences and the product with the reciprocal pivot per row)
    const double b[3] = {0.7, -1.1, 0.4}, p[3] = {0.2, 0.9, -0.3};
    double y[3] = {b[0], b[1], b[2]};
    k0_forward_step((const double*)f + 18, true, y, p);
    for (int r = 0; r < 3; ++r) {
        ld acc = 0, ab = A(b[r]);
        for (int k = 0; k < 3; ++k) acc += L[1][3 * r + k] * y[k] * (k <= r) + B[3 * r + k] * p[k], ab += A(L[1][3 * r + k] * y[k]) * (k <= r) + A(B[3 * r + k] * p[k]);
        BOUND(15, acc - b[r], 10, ab);
    }
    double x[3] = {b[0], b[1], b[2]};
    k0_backward_step((const double*)f, true, x, p);
    for (int r = 0; r < 3; ++r) {
        ld acc = 0, ab = A(b[r]);
        for (int k = 0; k < 3; ++k) acc += L[0][3 * k + r] * x[k] * (k >= r) + B[3 * k + r] * p[k], ab += A(L[0][3 * k + r] * x[k]) * (k >= r) + A(B[3 * k + r] * p[k]);
        BOUND(15, acc - b[r], 10, ab);
    }
    double y0[3] = {b[0], b[1], b[2]}, y1[3] = {b[0], b[1], b[2]};
    const double zero[3] = {0, 0, 0};
    k0_forward_step((const double*)f + 18, false, y0, p), k0_forward_step((const double*)f + 18, true, y1, zero);  // (no link: p is not read)
    CHECK(y0[0] == y1[0] && y0[1] == y1[1] && y0[2] == y1[2]);
    // a pivot that is not positive clears the flag: the first, and one that only the elimination turns negative
    double g1[18] = {-1, 0, 0, 0, 1, 0, 0, 0, 1}, g2[18] = {1, 2, 0, 2, 1, 0, 0, 0, 1}, g3[18] = {1, 0, 0, 0, 1, 0, 0, 0, 0};
    double Bq[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(!k0_factor_step(g1, Bq, true));
    CHECK(!k0_factor_step(g2, Bq, true));
    CHECK(!k0_factor_step(g3, Bq, true));
}

int main() {
    row_equations();
    upbuild_is_build_at_the_new_state();
    candidates();
    accumulators();
    pair_rows();
    k0_chain();
    static const char* name[16] = {"weight", "build rg", "build v", "affine eq 1", "affine eq 2", "cc", "corrector rhs", "wz", "step limit", "corrected eq 1",
                                   "corrected eq 2", "state update", "gondzio rhs", "kmul", "pair row", "k0 chain"};
    for (int i = 0; i < 16; ++i) std::printf("%-16s largest residual / bound %.3f\n", name[i], worst[i]);
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("ipm rows ok\n");
    return 0;
}
