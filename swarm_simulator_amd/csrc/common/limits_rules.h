// limits_rules.h — certified intervals for the largest velocity and the largest acceleration of a plan, as fractions of the agents' limits,
// in CONTINUOUS time: not at the samples t = j * dt of state_rules.h but at every instant of every segment.  Stated once for the host entry
// (host/limits.cpp rbp_limits_host, g++) and the device kernels (kernels/limits.hip, hipcc).  Plain C++, <math.h> and <stdint.h> only
// (through state_rules.h and separation_rules.h, which this file includes and leaves as they are).
//
// An ITEM is an agent a and a segment m.  On the segment the velocity of an axis is a polynomial of degree n = 4 and the acceleration one of
// degree n = 3 in t in [0, h], h = Ts[m+1] - Ts[m].  A polynomial in Bernstein form lies in the hull of its control points and passes
// through the first and the last one, so of a PIECE of the segment, per axis k and derivative X,
//     lower = max(0, max(|b_0|, |b_n|) - err) / limit   <=   sup |X_k(t)| / limit on the piece   <=   upper = (max_i |b_i| + err) / limit,
// where b_0 .. b_n are the computed control points of the piece and err bounds what rounding did to them.  Halving a piece (de Casteljau
// at 1/2) brings the two sides together.
//
// The steps, each of them a function below, every operation an IEEE double operation rounded on its own, in the order written:
//   derivative_coefficients  the ascending monomial coefficients gamma_j of the derivative from the six descending-power coefficients c of
//                            the position: (double)(5 - i) * c[i] (velocity, j = 4 - i) and (double)((5 - i) * (4 - i)) * c[i] (acceleration,
//                            j = 3 - i) -- the very products state_rules::velocity / acceleration form, so the rule and rbp_dynamics
//                            differentiate the same numbers.  Differences of the quintic's control points are NOT taken: they cancel, and
//                            the error would scale with the size of the position
//   bernstein_form           g_0 = gamma_0, g_i = gamma_i * hp_i, hp of separation_rules::powers_of (h as separation_rules::item_of forms
//                            it); b_k = g_0 + w(k,1) g_1 + ... + w(k,k) g_k summed from the left, w(k,i) = C(k,i) / C(n,i) one correctly
//                            rounded quotient of two small integers (a constant: both compilers fold it)
//   halve                    n rounds of b_i = (b_i + b_(i+1)) * 0.5; the left half is the first point of every round, the right half what
//                            stands in place at the end
//   piece_points             piece p of depth D, [p / 2^D, (p+1) / 2^D] of the segment: D halvings that follow the bits of p from the most
//                            significant (0: left) -- the convention of separation_rules::piece_points, with degree 4 and 3
//   error_term               err = (c_D * 2^-53) * V,  V = |gamma_0| + |gamma_1| |hp_1| + ... summed from the left
//   piece_bounds             the two quotients by the limit, moved outwards by RBP_LIMITS_ULPS doubles
//
// The constant c_D.  "Exact" is the polynomial the double inputs define: the exact products (5 - i) c[i], the exact h of the two scaled
// doubles.  Count roundings, (1 + u)^r - 1 <= r u / (1 - r u) =: y(r), u = 2^-53, and note that every exact weight row sums to 1 with
// weights in [0, 1], so every exact control point is at most V in size, on every piece (V here the exact sum of |gamma_i| h^i).
//   gamma_i    1 rounding (the integer factor is exact)
//   hp_i       the computed h carries 1, so h^i carries i, and the i - 1 products as many:          2 i - 1   (at most 7, i <= 4)
//   g_i        gamma, hp and the product:                                                           2 i + 1   (g_0: 1)
//   b_k        the weight 1, its product 1, the k - i + 1 sums a term goes through:   i + k + 4 <= 2 n + 4 <= 12  -> |computed - exact| <= y(12) V
//   a halving  a point goes through at most n <= 4 sums per level ((a + b) * 0.5: the product is exact):   4 D more -> y(12 + 4 D) V
//   computed V |gamma_i| (1) times |hp_i| (7), the product (1), at most 4 sums: at most 13 roundings: computed V >= V (1 - 13 u)
//   err        c_D * 2^-53 is exact (a small integer times a power of two); its product with the computed V rounds once:
//              err >= c_D u V (1 - 14 u)
//   max + err, ends - err   one rounding each, of a number at most (1 + y(12 + 4 D)) V + err in size: it moves the bound inwards by less
//              than u V (1 + 2^-40)
// so the exact control points lie within the computed bounds if c_D u V (1 - 14 u) >= y(12 + 4 D) V + u V (1 + 2^-40), that is if
// c_D >= 13 + 4 D and a fraction (second-order terms, together far less than 2^-40 units of u).  Three units on top:
//     c_D = 16 + 4 D     (at most 48 for D = 8: err <= 2^-47 V).
// The bound holds while nothing overflows and no product falls under 2^-1022 (plans in metres and seconds do neither).
//
// The ratios.  rule_div is correctly rounded and the limit is an input, so a quotient is off by less than one unit in the last place.
// The lower ratio is moved RBP_LIMITS_ULPS = 2 doubles towards zero (never past it), the upper one 2 doubles away from it (a ratio of
// exactly 0 stays: an agent at rest has the ratios 0, 0).  A limit that is not a positive number bounds nothing: the quotient is formed
// and both ratios are then no number.  A ratio that is no number (a NaN coefficient; an infinite one, where err is infinite and the lower
// numerator inf - inf) certifies nothing and proves nothing: the item counts as uncertified, never as violating, and is never a peak.
//
// The promise, for the polynomials the double coefficients define and positive limits:
//     lower_X_ratio <= sup over agents, axes and instants of |X_k(t)| / max_X[a][k] <= upper_X_ratio,      X = vel, acc.
// upper <= 1 certifies the limit, lower > 1 proves a violation.  Counts, in items: UNCERTIFIED where some evaluated piece has an upper
// ratio, vel or acc, that is not <= 1 (a NaN and an infinity count, so that uncertified == 0 certifies); VIOLATING where some piece's
// lower ratio is > 1; REFINED where the item went to `depth`.
//
// Refinement is fixed, not adaptive: an item is evaluated at depth 0; where all six upper ratios there are <= refine_above it stays,
// otherwise (a NaN goes too) all 2^depth pieces of depth `depth` are evaluated and the depth-0 bounds are dropped.  The decision is the
// item's own: no incumbent, no order, the same bits under every schedule.  With depth = 0 a refined item is evaluated again on its one
// piece of depth 0: the same bits, counted as refined.
//
// Floating point: as report_rules.h says (`#pragma clang fp contract(off)` below holds for the rest of the translation unit; a g++
// target with FMA is refused).  A maximum has no rounding, so the order pieces arrive in does not matter.
#pragma once
#include "common/state_rules.h"
#include "common/separation_rules.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__FMA__)
#error "limits_rules.h: g++ fuses a * b + c on a target with FMA; build this file without -mfma / -march=native (every product and sum rounds on its own)"
#endif

#ifndef RBP_LIMITS_MAX_DEPTH /* (include/rbp.h says the same) */
#define RBP_LIMITS_MAX_DEPTH 8
#endif
#define RBP_LIMITS_ULPS 2 /* how far a ratio is moved outwards for its division */

namespace limits_rules {

using report_rules::rule_div;
using separation_rules::ratio_down;
using separation_rules::ratio_up;

// the ascending coefficients of the derivative of degree n (4: velocity, 3: acceleration) from the position's six descending ones
template <int n>
REPORT_RULE void derivative_coefficients(const double* c, double* gamma) {
    static_assert(n == 4 || n == 3, "velocity or acceleration");
    for (int j = 0; j <= n; ++j) {
        const int i = n - j;  // the coefficient's place in c
        gamma[j] = (n == 4) ? (double)(5 - i) * c[i] : (double)((5 - i) * (4 - i)) * c[i];
    }
}

// w(k,i) = C(k,i) / C(n,i): one rounding
template <int n>
REPORT_RULE double bernstein_weight(int k, int i) {
    return rule_div(separation_rules::binomial(k, i), separation_rules::binomial(n, i));
}

// the n + 1 control points on [0, h]
template <int n>
REPORT_RULE void bernstein_form(const double* gamma, const double* hp, double* beta) {
    double g[n + 1];
    g[0] = gamma[0];
    for (int i = 1; i <= n; ++i) g[i] = gamma[i] * hp[i];
    for (int k = 0; k <= n; ++k) {
        double s = g[0];
        for (int i = 1; i <= k; ++i) {
            const double t = bernstein_weight<n>(k, i) * g[i];
            s = s + t;
        }
        beta[k] = s;
    }
}

// V = |gamma_0| + |gamma_1| |h| + ..., summed from the left
template <int n>
REPORT_RULE double poly_size(const double* gamma, const double* hp) {
    double s = fabs(gamma[0]);
    for (int i = 1; i <= n; ++i) {
        const double t = fabs(gamma[i]) * fabs(hp[i]);
        s = s + t;
    }
    return s;
}

// one halving of the n + 1 control points, in place: the left half (right = false) or the right half
template <int n>
REPORT_RULE void halve(double* b, bool right) {
    double left[n + 1];
    left[0] = b[0];
    for (int r = 1; r <= n; ++r) {
        for (int i = 0; i + r <= n; ++i) b[i] = (b[i] + b[i + 1]) * 0.5;
        left[r] = b[0];
    }
    for (int i = 0; i <= n; ++i) b[i] = right ? b[i] : left[i];
}

// the control points of piece p of depth D from those of the whole segment, in place
template <int n>
REPORT_RULE void piece_points(double* b, int32_t depth, int32_t p) {
    for (int32_t l = 0; l < depth; ++l) halve<n>(b, ((p >> (depth - 1 - l)) & 1) != 0);
}

// err of a piece of depth D: (c_D u) V
REPORT_RULE double error_constant(int32_t depth) { return (double)(16 + 4 * depth); }
REPORT_RULE double error_term(int32_t depth, double V) { return (error_constant(depth) * 1.1102230246251565e-16 /* 2^-53 */) * V; }

// a non-negative numerator over its limit; no number where the limit is not positive
REPORT_RULE double ratio_of(double value, double limit) {
    const double q = rule_div(value, limit);
    return limit > 0.0 ? q : (double)NAN;
}

// the two ratios of a piece from its control points, err and the limit (a NaN stays)
struct Bounds {
    double lower, upper;
};
template <int n>
REPORT_RULE Bounds piece_bounds(const double* b, double err, double limit) {
    double mx = fabs(b[0]);
    for (int i = 1; i <= n; ++i) {
        const double x = fabs(b[i]);
        if (x > mx || x != x) mx = x;
    }
    const double first = fabs(b[0]), last = fabs(b[n]);
    const double ends = last > first || last != last ? last : first;
    const double lo = ends - err;
    const double lower_num = lo <= 0.0 ? 0.0 : lo;  // (a NaN stays; -0 becomes 0)
    const double upper_num = mx + err;
    Bounds r;
    r.lower = ratio_down(ratio_of(lower_num, limit), RBP_LIMITS_ULPS);
    r.upper = ratio_up(ratio_of(upper_num, limit), RBP_LIMITS_ULPS);
    return r;
}

// A peak and where it was found: the largest ratio, and among equal ratios the lexicographically first (segment, piece, agent, axis); a
// ratio of 0, a negative one or a NaN is never taken (state_rules::Peak's rule).  `take` keeps that peak whatever the order candidates
// arrive in, which is what lets lanes, wavefronts and kernels each keep their own and merge.  depth: that of the piece (0 or the call's
// depth; -1: none).
struct Peak {
    double ratio;
    int32_t segment, piece, agent, axis, depth, pad;
};
REPORT_RULE Peak no_peak() { return Peak{0.0, -1, -1, -1, -1, -1, 0}; }
// (one decision and six selects under it, not a chain of early returns around a struct copy: every field of the peak moves together)
REPORT_RULE bool precedes(const Peak& c, const Peak& m) {
    const bool more = c.ratio > m.ratio, equal = c.ratio == m.ratio;
    const bool first = c.segment != m.segment ? c.segment < m.segment
                                              : (c.piece != m.piece ? c.piece < m.piece : (c.agent != m.agent ? c.agent < m.agent : c.axis < m.axis));
    return more || (equal && first);
}
REPORT_RULE void take(Peak* m, const Peak& c) {
    const bool p = precedes(c, *m);
    m->ratio = p ? c.ratio : m->ratio;
    m->segment = p ? c.segment : m->segment, m->piece = p ? c.piece : m->piece;
    m->agent = p ? c.agent : m->agent, m->axis = p ? c.axis : m->axis, m->depth = p ? c.depth : m->depth;
}

// what a mission's pieces add up to (rbp_limits of include/rbp.h, besides the end time and the status)
struct Tally {
    Peak lower_vel, upper_vel, lower_acc, upper_acc;
    int64_t uncertified, violating, refined;  // items
};
REPORT_RULE Tally empty_tally() { return Tally{no_peak(), no_peak(), no_peak(), no_peak(), 0, 0, 0}; }
REPORT_RULE void merge(Tally* t, const Tally& o) {
    take(&t->lower_vel, o.lower_vel), take(&t->upper_vel, o.upper_vel), take(&t->lower_acc, o.lower_acc), take(&t->upper_acc, o.upper_acc);
    t->uncertified += o.uncertified, t->violating += o.violating, t->refined += o.refined;
}

// what the evaluated pieces of one item leave: its largest upper ratios (0: none; +infinity stands for an upper ratio that is no number,
// an upper bound too, so that the bits do not depend on which NaN a machine forms) and its flags
#define RBP_LIMITS_UNCERTIFIED 1
#define RBP_LIMITS_VIOLATING 2
#define RBP_LIMITS_NOT_A_NUMBER 4
struct ItemState {
    double upper_vel, upper_acc;
    int32_t flags;
};
REPORT_RULE ItemState empty_item() { return ItemState{0.0, 0.0, 0}; }
REPORT_RULE void merge_item(ItemState* s, const ItemState& o) {
    s->upper_vel = o.upper_vel > s->upper_vel ? o.upper_vel : s->upper_vel;
    s->upper_acc = o.upper_acc > s->upper_acc ? o.upper_acc : s->upper_acc;
    s->flags |= o.flags;
}

// one piece's bounds of one axis and one derivative into the tally's peaks and into the item's state
template <bool acc>
REPORT_RULE void take_bounds(Tally* t, ItemState* s, const Bounds& bd, int32_t depth, int32_t p, int32_t m, int32_t a, int32_t k) {
    take(acc ? &t->lower_acc : &t->lower_vel, Peak{bd.lower, m, p, a, k, depth, 0});
    take(acc ? &t->upper_acc : &t->upper_vel, Peak{bd.upper, m, p, a, k, depth, 0});
    const bool nan = bd.upper != bd.upper;
    const double up = nan ? (double)INFINITY : bd.upper;
    if (acc)
        s->upper_acc = up > s->upper_acc ? up : s->upper_acc;
    else
        s->upper_vel = up > s->upper_vel ? up : s->upper_vel;
    s->flags |= (!(bd.upper <= 1.0) ? RBP_LIMITS_UNCERTIFIED : 0) | (bd.lower > 1.0 ? RBP_LIMITS_VIOLATING : 0) | (nan ? RBP_LIMITS_NOT_A_NUMBER : 0);
}

// the pieces p0, p0 + step, ... < p1 of depth D of one axis and one derivative of an item: c the axis' six coefficients on the segment
template <int n>
REPORT_RULE void take_poly(Tally* t, ItemState* s, const double* c, const double* hp, double limit, int32_t depth, int32_t p0, int32_t p1,
                           int32_t step, int32_t m, int32_t a, int32_t k) {
    double gamma[n + 1], whole[n + 1];
    derivative_coefficients<n>(c, gamma);
    bernstein_form<n>(gamma, hp, whole);
    const double err = error_term(depth, poly_size<n>(gamma, hp));
    for (int32_t p = p0; p < p1; p += step) {
        double b[n + 1];
        for (int i = 0; i <= n; ++i) b[i] = whole[i];
        piece_points<n>(b, depth, p);
        take_bounds<n == 3>(t, s, piece_bounds<n>(b, err, limit), depth, p, m, a, k);
    }
}

// the pieces p0, p0 + step, ... < p1 of depth D of an item, one polynomial at a time.  max_vel / max_acc: the agent's three limits.
REPORT_RULE void take_pieces(Tally* t, ItemState* s, const double* coef, int32_t M, const double* T, double ts, int32_t a, int32_t m,
                             const double* max_vel, const double* max_acc, int32_t depth, int32_t p0, int32_t p1, int32_t step) {
    const double h = report_rules::scaled_time(T[m + 1], ts) - report_rules::scaled_time(T[m], ts);
    double hp[6];
    separation_rules::powers_of(h, hp);
    for (int k = 0; k < 3; ++k) {
        const double* c = report_rules::coef_of(coef, M, a, k, m);
        take_poly<4>(t, s, c, hp, max_vel[k], depth, p0, p1, step, m, a, k);
        take_poly<3>(t, s, c, hp, max_acc[k], depth, p0, p1, step, m, a, k);
    }
}

// whether an item goes to `depth`, from the state its depth-0 piece leaves
REPORT_RULE bool is_refined(const ItemState& s0, double refine_above) {
    return (s0.flags & RBP_LIMITS_NOT_A_NUMBER) != 0 || !(s0.upper_vel <= refine_above) || !(s0.upper_acc <= refine_above);
}
// an item's counts once all its pieces are in
REPORT_RULE void count_item(Tally* t, const ItemState& s, bool refined) {
    if (s.flags & RBP_LIMITS_UNCERTIFIED) ++t->uncertified;
    if (s.flags & RBP_LIMITS_VIOLATING) ++t->violating;
    if (refined) ++t->refined;
}

// One item, whole: depth 0, then `depth` where the rule says so.  The state of the pieces that count is returned.
REPORT_RULE ItemState take_item(Tally* t, const double* coef, int32_t M, const double* T, double ts, int32_t a, int32_t m, const double* max_vel,
                                const double* max_acc, int32_t depth, double refine_above) {
    Tally t0 = empty_tally();
    ItemState s0 = empty_item();
    take_pieces(&t0, &s0, coef, M, T, ts, a, m, max_vel, max_acc, 0, 0, 1, 1);
    if (!is_refined(s0, refine_above)) {
        merge(t, t0);
        count_item(t, s0, false);
        return s0;
    }
    ItemState s = empty_item();
    take_pieces(t, &s, coef, M, T, ts, a, m, max_vel, max_acc, depth, 0, (int32_t)1 << depth, 1);
    count_item(t, s, true);
    return s;
}

// Everything, one item after the other: the loop of the host entry, and the meaning of every shortcut the device takes.
// T [M+1] unscaled, coef [N][3][6M], max_vel / max_acc [N][3]; agent_upper [N][2] or null: every agent's largest upper velocity ratio and
// largest upper acceleration ratio over its segments and axes (0 where none; +infinity where one is no number).  depth in
// 0 .. RBP_LIMITS_MAX_DEPTH, refine_above a number.
REPORT_RULE Tally limits_sequential(int32_t N, int32_t M, const double* T, double ts, const double* coef, const double* max_vel,
                                    const double* max_acc, int32_t depth, double refine_above, double* agent_upper) {
    Tally t = empty_tally();
    for (int32_t a = 0; a < N; ++a) {
        ItemState au = empty_item();
        for (int32_t m = 0; m < M; ++m)
            merge_item(&au, take_item(&t, coef, M, T, ts, a, m, max_vel + 3 * (int64_t)a, max_acc + 3 * (int64_t)a, depth, refine_above));
        if (agent_upper) agent_upper[2 * (int64_t)a] = au.upper_vel, agent_upper[2 * (int64_t)a + 1] = au.upper_acc;
    }
    return t;
}

}  // namespace limits_rules
