// separation_rules.h — a certified interval for the smallest safety ratio of a plan in CONTINUOUS time: not at the samples t = j * dt
// of report_rules.h but at every instant of every segment.  Stated once for the host entry (host/validate.cpp rbp_separation_host, g++)
// and the device kernels (kernels/separation.hip, hipcc).  Plain C++, <math.h> and <stdint.h> only (through report_rules.h, which this
// file includes and leaves as it is).
//
// An ITEM is a pair qi < qj and a segment m.  On the segment the downwash-scaled relative position r(t) = (p_qj - p_qi) (z over the
// downwash, the scaling of report_rules::safety_ratio) is a polynomial of degree 5 per axis in t in [0, h], h = Ts[m+1] - Ts[m], and
// |r(t)|^2 one of degree 10.  A polynomial in Bernstein form lies above its smallest coefficient and passes through its first and last
// one, so of a PIECE of the segment
//     lower_sq = max(0, min_k q_k - err)        <=  min |r|^2 on the piece  <=        upper_sq = min(q_0, q_10) + err,
// where q_0 .. q_10 are the computed Bernstein coefficients of |r|^2 on the piece and err bounds what rounding did to them.  Halving a
// piece (de Casteljau at 1/2) brings the two sides together fourfold.  The ratios are the square roots over the sum of the radii.
//
// The steps, each of them a function below, every operation an IEEE double operation rounded on its own, in the order written:
//   relative_coefficients  alpha_i = c_qj[5-i] - c_qi[5-i] (ascending powers), the z axis then rule_div(., downwash)
//   bernstein_form         g_0 = alpha_0, g_i = alpha_i * hp_i with hp_1 = h, hp_i = hp_(i-1) * h;
//                          beta_k = g_0 + w(k,1) g_1 + ... + w(k,k) g_k, summed from the left, w(k,i) = C(k,i) / C(5,i) one correctly
//                          rounded quotient of two small integers (a constant: both compilers fold it)
//   halve                  five rounds of b_i = (b_i + b_(i+1)) * 0.5; the left half is the first point of every round, the right half
//                          what stands in place at the end
//   piece_points           piece p of depth D, [p / 2^D, (p+1) / 2^D] of the segment: D halvings that follow the bits of p from the
//                          most significant (0: left), so a piece's bits do not depend on how anyone walks the pieces
//   squared_norm           q_k = sum over a + b = k, a ascending, of W(a,b) * ((bx_a bx_b + by_a by_b) + bz_a bz_b),
//                          W(a,b) = C(5,a) C(5,b) / C(10,a+b), one correctly rounded quotient of two integers
//   error_term             err = c u S, u = 2^-53, S = Ax^2 + Ay^2 + Az^2, A = |alpha_0| + |alpha_1 h| + ... + |alpha_5 h^5|
//   piece_bounds           the two ratios, moved outwards by RBP_SEPARATION_ULPS
//
// The constant c.  "Exact" is the polynomial the double inputs define: exact differences, the exact quotient by the downwash, the exact
// h of the two scaled doubles.  Count roundings, (1 + u)^n - 1 <= n u / (1 - n u) =: y(n), and note that every exact weight row sums to
// 1 with weights in [0, 1], so every exact control point of an axis is at most A in size, on every piece, and every exact q_k at most S.
//   alpha_i        2 roundings (difference, quotient; x and y have 1)
//   hp_i           the computed h carries 1, so h^i carries i, and the i - 1 products as many:            2 i - 1
//   g_i            alpha, hp and the product:                                                             2 i + 2   (g_0: 2)
//   beta_k         the weight 1, the product 1, the k - i + 1 sums a term goes through:   i + k + 5 <= 15  -> |computed - exact| <= y(15) A
//   a halving      a point goes through at most 5 sums per level ((a + b) * 0.5: the product is exact):   5 D more -> y(15 + 5 D) A
//   a product of two points squares that, and rounds:                                                     2 (15 + 5 D) + 1
//   the sum of the three axes 2, the weight 1, its product 1, at most 5 sums of terms:                    9 more
//   q_k            |computed - exact| <= y(40 + 10 D) S
// S itself is computed with at most 37 roundings, and y(n) exceeds n u by n^2 u^2: 8 more units of u cover both with room to spare, so
//     c = 48 + 10 D     (at most 128 for D = 8: err <= 2^-46 S).
// The bound holds while nothing overflows and no product of two coefficients falls under 2^-1022 (plans in metres and seconds do
// neither).  A NaN in an item makes S, err and the item's ratios NaN, and a NaN is never a minimum; an infinity makes err infinite or
// NaN: the lower ratio is 0 or NaN, the upper one infinite or NaN -- nothing certified, nothing proven.
//
// The ratios.  rule_sqrt and rule_div are correctly rounded, so sqrt(.) / radius_sum is off by a factor within (1 + u)^2 of the exact
// one: less than 3 units in the last place.  The lower ratio is moved RBP_SEPARATION_ULPS = 3 doubles towards zero (never past it), the
// upper one 3 doubles away from it (a ratio of exactly 0 stays: the root and the quotient of 0 are exact).  The promise of a piece: lower ratio <= the exact minimum of the safety ratio on it <= upper ratio.
//
// Refinement is fixed, not adaptive: an item is evaluated at depth 0; where its lower ratio there is >= refine_below it stays, otherwise
// all 2^depth pieces of depth `depth` are evaluated and the depth-0 bounds are dropped.  The decision is the item's own: no incumbent,
// no order, the same bits under every schedule.
//
// Floating point: as report_rules.h says (`#pragma clang fp contract(off)` below holds for the rest of the translation unit; a g++
// target with FMA is refused).
#pragma once
#include "common/report_rules.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__FMA__)
#error "separation_rules.h: g++ fuses a * b + c on a target with FMA; build this file without -mfma / -march=native (every product and sum rounds on its own)"
#endif

#ifndef RBP_SEPARATION_MAX_DEPTH /* (include/rbp.h says the same) */
#define RBP_SEPARATION_MAX_DEPTH 8
#endif
#define RBP_SEPARATION_ULPS 3 /* how far a ratio is moved outwards for its square root and its division */

namespace separation_rules {

using report_rules::rule_div;
using report_rules::rule_sqrt;

// C(5,i) and C(10,k)
REPORT_RULE double binomial5(int i) { return (i == 0 || i == 5) ? 1.0 : (i == 1 || i == 4) ? 5.0 : 10.0; }
REPORT_RULE double binomial10(int k) {
    const int j = k > 5 ? 10 - k : k;
    return j == 0 ? 1.0 : j == 1 ? 10.0 : j == 2 ? 45.0 : j == 3 ? 120.0 : j == 4 ? 210.0 : 252.0;
}
// C(k,i), k <= 5
REPORT_RULE double binomial(int k, int i) {
    const int j = i > k - i ? k - i : i;
    return j == 0 ? 1.0 : j == 1 ? (double)k : (k == 4 ? 6.0 : 10.0);
}
// w(k,i) = C(k,i) / C(5,i) and W(a,b) = C(5,a) C(5,b) / C(10,a+b): one rounding each (the product of two binomials is exact)
REPORT_RULE double bernstein_weight(int k, int i) { return rule_div(binomial(k, i), binomial5(i)); }
REPORT_RULE double product_weight(int a, int b) { return rule_div(binomial5(a) * binomial5(b), binomial10(a + b)); }

// the relative coefficients of one axis in ascending powers, from the six descending-power coefficients of both agents
REPORT_RULE void relative_coefficients(const double* ci, const double* cj, bool z_axis, double downwash, double* alpha) {
    for (int i = 0; i < 6; ++i) {
        const double d = cj[5 - i] - ci[5 - i];
        alpha[i] = z_axis ? rule_div(d, downwash) : d;
    }
}

// hp[i] = h^i as the rule forms it (hp[0] is not used in a product)
REPORT_RULE void powers_of(double h, double* hp) {
    hp[0] = 1.0, hp[1] = h;
    for (int i = 2; i < 6; ++i) hp[i] = hp[i - 1] * h;
}

// the six control points of one axis on [0, h]
REPORT_RULE void bernstein_form(const double* alpha, const double* hp, double* beta) {
    double g[6];
    g[0] = alpha[0];
    for (int i = 1; i < 6; ++i) g[i] = alpha[i] * hp[i];
    for (int k = 0; k < 6; ++k) {
        double s = g[0];
        for (int i = 1; i <= k; ++i) {
            const double t = bernstein_weight(k, i) * g[i];
            s = s + t;
        }
        beta[k] = s;
    }
}

// A = |alpha_0| + |alpha_1 h| + ... of one axis, summed from the left (|h^i|: times that do not ascend must not shrink the bound)
REPORT_RULE double axis_size(const double* alpha, const double* hp) {
    double s = fabs(alpha[0]);
    for (int i = 1; i < 6; ++i) {
        const double t = fabs(alpha[i]) * fabs(hp[i]);
        s = s + t;
    }
    return s;
}
REPORT_RULE double size_squared(double ax, double ay, double az) {
    const double xx = ax * ax, yy = ay * ay, zz = az * az;
    const double xy = xx + yy;
    return xy + zz;
}

// one halving of the six control points b of one axis, in place: the left half (right = false) or the right half
REPORT_RULE void halve(double* b, bool right) {
    double left[6];
    left[0] = b[0];
    for (int r = 1; r < 6; ++r) {
        for (int i = 0; i + r < 6; ++i) b[i] = (b[i] + b[i + 1]) * 0.5;
        left[r] = b[0];
    }
    for (int i = 0; i < 6; ++i) b[i] = right ? b[i] : left[i];
}

// the control points of piece p of depth D from those of the whole segment, in place (three axes of six)
REPORT_RULE void piece_points(double* b, int32_t depth, int32_t p) {
    for (int32_t l = 0; l < depth; ++l) {
        const bool right = ((p >> (depth - 1 - l)) & 1) != 0;
        halve(b, right), halve(b + 6, right), halve(b + 12, right);
    }
}

// the eleven Bernstein coefficients of |r|^2 on a piece from its control points b [3][6]
REPORT_RULE void squared_norm(const double* b, double* q) {
    for (int k = 0; k <= 10; ++k) {
        const int a0 = k > 5 ? k - 5 : 0, a1 = k < 5 ? k : 5;
        double s = 0.0;
        for (int a = a0; a <= a1; ++a) {
            const int c = k - a;
            const double xx = b[a] * b[c], yy = b[6 + a] * b[6 + c], zz = b[12 + a] * b[12 + c];
            const double xy = xx + yy;
            const double t = product_weight(a, c) * (xy + zz);
            s = (a == a0) ? t : s + t;
        }
        q[k] = s;
    }
}

// err of a piece of depth D: c u S
REPORT_RULE double error_constant(int32_t depth) { return (double)(48 + 10 * depth); }
REPORT_RULE double error_term(int32_t depth, double S) { return (error_constant(depth) * 1.1102230246251565e-16 /* 2^-53 */) * S; }

// a non-negative ratio moved n doubles towards zero (never past it) or away from it; a NaN, an infinity and, upwards, a zero stay
REPORT_RULE double ratio_down(double v, int n) {
    if (!(v < INFINITY)) return v;
    int64_t bits;
    __builtin_memcpy(&bits, &v, 8);
    bits = bits > (int64_t)n ? bits - (int64_t)n : 0;
    __builtin_memcpy(&v, &bits, 8);
    return v;
}
REPORT_RULE double ratio_up(double v, int n) {
    if (!(v < INFINITY) || v == 0.0) return v;
    int64_t bits;
    __builtin_memcpy(&bits, &v, 8);
    const int64_t infinity = 0x7FF0000000000000LL;
    bits = bits + (int64_t)n < infinity ? bits + (int64_t)n : infinity;  // (beyond the largest double lies infinity, an upper bound too)
    __builtin_memcpy(&v, &bits, 8);
    return v;
}

// the two ratios of a piece from its q and err
struct Bounds {
    double lower, upper;
};
REPORT_RULE Bounds piece_bounds(const double* q, double err, double radius_sum) {
    double mn = q[0];
    for (int k = 1; k <= 10; ++k)
        if (q[k] < mn || q[k] != q[k]) mn = q[k];  // (a NaN stays)
    const double lo = mn - err;
    const double lower_sq = lo <= 0.0 ? 0.0 : lo;  // (a NaN stays; -0 becomes 0)
    const double ends = q[10] < q[0] || q[10] != q[10] ? q[10] : q[0];
    const double upper_sq = ends + err;
    Bounds r;
    r.lower = ratio_down(rule_div(rule_sqrt(lower_sq), radius_sum), RBP_SEPARATION_ULPS);
    r.upper = ratio_up(rule_div(rule_sqrt(upper_sq), radius_sum), RBP_SEPARATION_ULPS);
    return r;
}

// What an item needs of its inputs once: the control points of the whole segment and S.
struct Item {
    double b[18];  // [3][6]
    double S;
};
REPORT_RULE Item item_of(const double* coef, int32_t M, const double* T, double ts, int32_t qi, int32_t qj, int32_t m, double downwash) {
    Item it;
    const double h = report_rules::scaled_time(T[m + 1], ts) - report_rules::scaled_time(T[m], ts);
    double hp[6], size[3];
    powers_of(h, hp);
    for (int k = 0; k < 3; ++k) {
        double alpha[6];
        relative_coefficients(report_rules::coef_of(coef, M, qi, k, m), report_rules::coef_of(coef, M, qj, k, m), k == 2, downwash, alpha);
        bernstein_form(alpha, hp, it.b + 6 * k);
        size[k] = axis_size(alpha, hp);
    }
    it.S = size_squared(size[0], size[1], size[2]);
    return it;
}
// the bounds of piece p of depth D of an item
REPORT_RULE Bounds item_piece(const Item& it, int32_t depth, int32_t p, double radius_sum) {
    double b[18], q[11];
    for (int i = 0; i < 18; ++i) b[i] = it.b[i];
    piece_points(b, depth, p);
    squared_norm(b, q);
    return piece_bounds(q, error_term(depth, it.S), radius_sum);
}
// whether an item whose depth-0 lower ratio is `lower0` goes to `depth` (a NaN goes, and stays a NaN there)
REPORT_RULE bool is_refined(double lower0, double refine_below) { return !(lower0 >= refine_below); }

// A minimum and where it was found: the smallest ratio, and among equal ratios the lexicographically first (segment, piece, qi, qj); a
// ratio of 1e9 or more, or a NaN, is never taken.  `take` keeps that minimum whatever the order candidates arrive in, which is what
// lets lanes, wavefronts and kernels each keep their own and merge.  depth: that of the piece (0 or the call's depth; -1: none).
struct Minimum {
    double ratio;
    int32_t segment, piece, qi, qj, depth;
};
REPORT_RULE Minimum no_minimum() { return Minimum{RBP_REPORT_NO_RATIO, -1, -1, -1, -1, -1}; }
REPORT_RULE bool precedes(const Minimum& c, const Minimum& m) {
    if (c.ratio < m.ratio) return true;
    if (!(c.ratio == m.ratio)) return false;
    if (c.segment != m.segment) return c.segment < m.segment;
    if (c.piece != m.piece) return c.piece < m.piece;
    if (c.qi != m.qi) return c.qi < m.qi;
    return c.qj < m.qj;
}
REPORT_RULE void take(Minimum* m, const Minimum& c) {
    if (precedes(c, *m)) *m = c;
}

// what a mission's pieces add up to (rbp_separation of include/rbp.h, besides the end time and the status)
struct Tally {
    Minimum lower, upper;
    int64_t uncertified, colliding, refined;  // items
};
REPORT_RULE Tally empty_tally() { return Tally{no_minimum(), no_minimum(), 0, 0, 0}; }
REPORT_RULE void merge(Tally* t, const Tally& o) {
    take(&t->lower, o.lower), take(&t->upper, o.upper);
    t->uncertified += o.uncertified, t->colliding += o.colliding, t->refined += o.refined;
}

// one piece's bounds into the tally's minima and into the item's own two minima (from 1e9: a NaN moves neither)
REPORT_RULE void take_piece(Tally* t, double* item_lower, double* item_upper, const Bounds& bd, int32_t depth, int32_t p, int32_t m, int32_t qi,
                            int32_t qj) {
    take(&t->lower, Minimum{bd.lower, m, p, qi, qj, depth});
    take(&t->upper, Minimum{bd.upper, m, p, qi, qj, depth});
    if (bd.lower < *item_lower) *item_lower = bd.lower;
    if (bd.upper < *item_upper) *item_upper = bd.upper;
}
// the pieces p0 <= p < p1 of depth D of an item
REPORT_RULE void take_pieces(Tally* t, double* item_lower, double* item_upper, const Item& it, int32_t depth, int32_t p0, int32_t p1,
                             double radius_sum, int32_t m, int32_t qi, int32_t qj) {
    for (int32_t p = p0; p < p1; ++p) take_piece(t, item_lower, item_upper, item_piece(it, depth, p, radius_sum), depth, p, m, qi, qj);
}
// an item's counts once all its pieces are in
REPORT_RULE void count_item(Tally* t, double item_lower, double item_upper, bool refined) {
    if (item_lower < 1.0) ++t->uncertified;
    if (item_upper < 1.0) ++t->colliding;
    if (refined) ++t->refined;
}

// the index of pair (qi < qj) of N agents, the order of rbp_plan (include/rbp.h)
REPORT_RULE int64_t pair_index(int32_t N, int32_t qi, int32_t qj) { return (int64_t)qi * N - ((int64_t)qi * (qi + 1)) / 2 + (qj - qi - 1); }

// One item, whole: depth 0, then `depth` where the rule says so.  Its smallest lower ratio is returned (1e9: none was a number below 1e9).
REPORT_RULE double take_item(Tally* t, const double* coef, int32_t M, const double* T, double ts, int32_t qi, int32_t qj, int32_t m,
                             double downwash, double radius_sum, int32_t depth, double refine_below) {
    const Item it = item_of(coef, M, T, ts, qi, qj, m, downwash);
    const Bounds b0 = item_piece(it, 0, 0, radius_sum);
    const bool refined = is_refined(b0.lower, refine_below);
    double item_lower = RBP_REPORT_NO_RATIO, item_upper = RBP_REPORT_NO_RATIO;
    if (refined)
        take_pieces(t, &item_lower, &item_upper, it, depth, 0, (int32_t)1 << depth, radius_sum, m, qi, qj);
    else
        take_piece(t, &item_lower, &item_upper, b0, 0, 0, m, qi, qj);
    count_item(t, item_lower, item_upper, refined);
    return item_lower;
}

// Everything, one item after the other: the loop of the host entry, and the meaning of every shortcut the device takes.
// T [M+1] unscaled, coef [N][3][6M], radius [N]; pair_lower [N (N-1) / 2] or null: every pair's smallest lower ratio over its segments
// (1e9 where none is a number).  depth in 0 .. RBP_SEPARATION_MAX_DEPTH, refine_below > 0.  No pair: 1e9, -1 and zeros.
REPORT_RULE Tally separation_sequential(int32_t N, int32_t M, const double* T, double ts, const double* coef, const double* radius,
                                        double downwash, int32_t depth, double refine_below, double* pair_lower) {
    Tally t = empty_tally();
    for (int32_t qi = 0; qi < N; ++qi)
        for (int32_t qj = qi + 1; qj < N; ++qj) {
            const double radius_sum = radius[qi] + radius[qj];
            double pl = RBP_REPORT_NO_RATIO;
            for (int32_t m = 0; m < M; ++m) {
                const double lo = take_item(&t, coef, M, T, ts, qi, qj, m, downwash, radius_sum, depth, refine_below);
                if (lo < pl) pl = lo;
            }
            if (pair_lower) pair_lower[pair_index(N, qi, qj)] = pl;
        }
    return t;
}

}  // namespace separation_rules
