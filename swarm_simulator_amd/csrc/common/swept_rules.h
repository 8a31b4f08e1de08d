// swept_rules.h — a certified interval for the smallest clearance of a plan to the obstacles in CONTINUOUS time: not at the samples
// t = j * dt of clearance_rules.h but at every instant of every segment.  Stated once for the host entry (host/validate.cpp
// rbp_swept_clearance_host, g++) and the device kernels (kernels/swept.hip, hipcc).  Plain C++, <math.h> and <stdint.h> only (through
// clearance_rules.h and separation_rules.h, which this file includes and leaves as they are).
//
// An ITEM is an agent a and a segment m.  On the segment every axis of the agent's position is a polynomial of degree 5 in t in [0, h],
// h = Ts[m+1] - Ts[m].  A polynomial in Bernstein form lies between its smallest and its largest control point, so a PIECE of the segment
// lies in the box of its control points.  The lookup of clearance_rules.h is MONOTONE per axis: rounding to float, the product with
// rf = 1 / res and floor all preserve order (rf > 0).  So the keys of the box's two corners enclose the key of every point of the piece, and
// the smallest grid value among the cells of that box of keys bounds every reading on the piece from below.
//
// The steps, each of them a function below, every operation an IEEE double operation rounded on its own, in the order written:
//   item_of         h as separation_rules::item_of forms it; alpha_i = c[5 - i] of report_rules::coef_of (ascending powers: no difference, no
//                   downwash, no rounding); separation_rules::powers_of, bernstein_form and axis_size per axis: the six control points b_k
//                   of the whole segment and A_k = |alpha_0| + |alpha_1 h| + ...
//   piece_box       piece p of depth D by separation_rules::piece_points; per axis lo_k = min_i b_k[i] - e_k, hi_k = max_i b_k[i] + e_k,
//                   e_k = (c_D * 2^-53) * A_k
//   box_keys        kd = floor(rf * (double)(float)x) of lo_k and hi_k (the arithmetic of clearance_rules::axis_index).  OUTSIDE: on any axis
//                   !(kd_lo >= key_min && kd_hi < key_min + dim), decided on the doubles, so a NaN or an infinity is outside.  The cell count
//                   is the product of kd_hi - kd_lo + 1 in 64 bits; OVER BUDGET: more than RBP_SWEPT_MAX_CELLS
//   box_minimum     the smallest (double)dist[cell] over the box, z fastest as the grid lies; a NaN cell is never taken (a box of nothing
//                   but NaN reads +infinity, which is no minimum and no hit)
//   piece_readings  d_lo: -1 (RBP_CLEARANCE_OUTSIDE) for a piece that is outside or over budget -- nothing is scanned then -- otherwise
//                   box_minimum.  d_up: the smaller of the two lookups clearance_rules::cell_of / distance_of at the piece's first and at
//                   its last control point (a NaN stays).  The clearances are d_lo - radius and d_up - radius.
//
// The constant c_D.  "Exact" is the polynomial the double inputs define, with the exact h of the two scaled doubles.  Count roundings,
// (1 + u)^n - 1 <= n u / (1 - n u) =: y(n), u = 2^-53.  separation_rules.h's table gives, for a control point after D halvings,
//     |computed - exact| <= y(15 + 5 D) A,     A the exact |alpha_0| + |alpha_1| h + ... + |alpha_5| h^5
// (its count allows alpha two roundings; here alpha carries none, so the count has room).  On top of that:
//   the computed A   |alpha_i| * |hp_i| (hp_i carries 2 i - 1 <= 9, the product 1) through at most 5 sums: at most 15 roundings, so the
//                    computed A is at least A / (1 + u)^15 >= A (1 - 15 u)
//   e                c_D * 2^-53 is exact (a small integer times a power of two); its product with the computed A rounds once:
//                    e >= c_D u A (1 - 16 u)
//   lo - e, hi + e   one rounding each, of a number at most (1 + y(15 + 5 D)) A + e in size: it moves the corner inwards by less than
//                    u A (1 + 2^-40)
// so the exact control points lie in [lo, hi] if c_D u A (1 - 16 u) >= y(15 + 5 D) A + u A (1 + 2^-40), that is if c_D >= 16 + 5 D and a
// fraction (second-order terms: y(n) exceeds n u by n^2 u^2, (16 + 5 D) 16 u^2, together less than 2^-40 units of u).  Four units on top:
//     c_D = 20 + 5 D     (at most 60 for D = 8: e <= 2^-47 A).
// The bound holds while nothing overflows and no product falls under 2^-1022 (plans in metres and seconds do neither).  A NaN coefficient
// makes the control points, A, e and the corners NaN; an infinite one makes e infinite and the corners infinite or NaN: the piece is
// outside either way.
//
// Counts.  An item counts as UNCERTIFIED where clearance_rules::is_hit(d_lo, radius) on any of its evaluated pieces, as HITTING where
// is_hit(d_up, radius) on any, as OUTSIDE where any is outside, as OVER BUDGET where any is over budget, as REFINED where it went to `depth`.
//
// Refinement is fixed, not adaptive: an item is evaluated at depth 0; where that piece is inside, within the budget and its lower clearance
// is >= refine_below the item stays, otherwise all 2^depth pieces of depth `depth` are evaluated and the depth-0 readings and flags are
// dropped.  A NaN goes to `depth`, and so does every depth-0 box that is outside or over budget, whatever refine_below is (a box too large
// to scan says nothing about the plan).  The decision is the item's own: no incumbent, no order, the same bits under every schedule.  With
// depth = 0 a refined item is evaluated again on its one piece of depth 0: the same bits, counted as refined.
//
// The promise, for the polynomials the double coefficients define and a grid whose values are >= -1: every reading
// lookup(p_a(t)) - radius_a, at every instant t of [0, Ts[M]], is >= lower_clearance; lower_clearance > -1e-6 -- uncertified == 0 -- certifies
// the plan against the reference's own hit test.  upper_clearance is a reading at a point the rule COMPUTED on the curve, within e of it: a
// witness (hitting > 0: the rule found a point of the curve, up to e, whose cell is a hit), not a bound on the exact polynomial.  The lookup
// is a step function of the position, so a point within e of a cell face may read either cell and nothing stronger can be claimed.
//
// Floating point: as report_rules.h says (`#pragma clang fp contract(off)` below holds for the rest of the translation unit; a g++
// target with FMA is refused).  A minimum of floats has no rounding, so the scan's order does not matter.
#pragma once
#include "common/clearance_rules.h"
#include "common/separation_rules.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__FMA__)
#error "swept_rules.h: g++ fuses a * b + c on a target with FMA; build this file without -mfma / -march=native (every product and sum rounds on its own)"
#endif

#ifndef RBP_SWEPT_MAX_DEPTH /* (include/rbp.h says the same) */
#define RBP_SWEPT_MAX_DEPTH 8
#endif
#ifndef RBP_SWEPT_MAX_CELLS
#define RBP_SWEPT_MAX_CELLS 4096
#endif

namespace swept_rules {

// What an item needs of its inputs once: the control points of the whole segment and the sizes A_k.
struct Item {
    double b[18];  // [3][6]
    double A[3];
};
REPORT_RULE Item item_of(const double* coef, int32_t M, const double* T, double ts, int32_t a, int32_t m) {
    Item it;
    const double h = report_rules::scaled_time(T[m + 1], ts) - report_rules::scaled_time(T[m], ts);
    double hp[6];
    separation_rules::powers_of(h, hp);
    for (int k = 0; k < 3; ++k) {
        const double* c = report_rules::coef_of(coef, M, a, k, m);
        double alpha[6];
        for (int i = 0; i < 6; ++i) alpha[i] = c[5 - i];
        separation_rules::bernstein_form(alpha, hp, it.b + 6 * k);
        it.A[k] = separation_rules::axis_size(alpha, hp);
    }
    return it;
}

// e_k of a piece of depth D: (c_D u) A_k
REPORT_RULE double error_constant(int32_t depth) { return (double)(20 + 5 * depth); }
REPORT_RULE double error_term(int32_t depth, double A) { return (error_constant(depth) * 1.1102230246251565e-16 /* 2^-53 */) * A; }

// the widened interval of one axis of a piece from its six control points (a NaN stays)
REPORT_RULE void axis_interval(const double* b, double e, double* lo, double* hi) {
    double mn = b[0], mx = b[0];
    for (int i = 1; i < 6; ++i) {
        if (b[i] < mn || b[i] != b[i]) mn = b[i];
        if (b[i] > mx || b[i] != b[i]) mx = b[i];
    }
    *lo = mn - e, *hi = mx + e;
}

// the key of a coordinate as a double: clearance_rules::axis_index's arithmetic without the test
REPORT_RULE double key_of(double rf, double x) {
    const float xf = (float)x;
    return floor(rf * (double)xf);
}

// the box of a piece in cells: first index and count per axis
struct Box {
    int64_t i0[3], n[3];
    bool outside, over_budget;
};
REPORT_RULE Box box_keys(const int32_t* dim, const int32_t* key_min, double rf, const double* lo, const double* hi) {
    Box bx;
    bx.outside = false, bx.over_budget = false;
    for (int k = 0; k < 3; ++k) {
        const double kl = key_of(rf, lo[k]), kh = key_of(rf, hi[k]);
        const double first = (double)key_min[k], end = first + (double)dim[k];  // (sums of two int32: exact)
        if (!(kl >= first && kh < end)) {                                       // (a NaN fails)
            bx.outside = true;
            bx.i0[k] = 0, bx.n[k] = 0;
        } else {  // (kl and kh are integers within int32 here, and kl <= kh: lo <= hi and the key is monotone)
            bx.i0[k] = (int64_t)kl - (int64_t)key_min[k];
            bx.n[k] = (int64_t)kh - (int64_t)kl + 1;
        }
    }
    if (!bx.outside) {  // (each count is at most 2^31, so the product of two cannot overflow, nor can a third on top of at most 4096)
        const int64_t xy = bx.n[0] * bx.n[1];
        bx.over_budget = xy > (int64_t)RBP_SWEPT_MAX_CELLS || xy * bx.n[2] > (int64_t)RBP_SWEPT_MAX_CELLS;
    }
    return bx;
}

// the smallest value of the grid over a box that is inside and within the budget, z fastest; +infinity where every cell is a NaN.
// G: a pointer to const float (the device passes one in the global address space)
template <class G>
REPORT_RULE double box_minimum(G dist, const int32_t* dim, const Box& bx) {
    float mn = INFINITY;
    for (int64_t ix = bx.i0[0]; ix < bx.i0[0] + bx.n[0]; ++ix)
        for (int64_t iy = bx.i0[1]; iy < bx.i0[1] + bx.n[1]; ++iy) {
            const int64_t row = ((ix * (int64_t)dim[1]) + iy) * (int64_t)dim[2] + bx.i0[2];
            for (int64_t iz = 0; iz < bx.n[2]; ++iz) {
                const float v = dist[row + iz];
                if (v < mn) mn = v;  // (a NaN is never taken)
            }
        }
    return (double)mn;
}

// what a piece reads
struct Readings {
    double d_lo, d_up;
    bool outside, over_budget;
};
template <class G>
REPORT_RULE Readings piece_readings(const Item& it, int32_t depth, int32_t p, const int32_t* dim, const int32_t* key_min, double rf, G dist) {
    double b[18], lo[3], hi[3];
    for (int i = 0; i < 18; ++i) b[i] = it.b[i];
    separation_rules::piece_points(b, depth, p);
    for (int k = 0; k < 3; ++k) axis_interval(b + 6 * k, error_term(depth, it.A[k]), lo + k, hi + k);
    const Box bx = box_keys(dim, key_min, rf, lo, hi);
    Readings r;
    r.outside = bx.outside, r.over_budget = bx.over_budget;
    r.d_lo = (bx.outside || bx.over_budget) ? RBP_CLEARANCE_OUTSIDE : box_minimum(dist, dim, bx);
    const double first[3] = {b[0], b[6], b[12]}, last[3] = {b[5], b[11], b[17]};
    const int64_t c0 = clearance_rules::cell_of(dim, key_min, rf, first), c1 = clearance_rules::cell_of(dim, key_min, rf, last);
    const double d0 = clearance_rules::distance_of(c0, c0 >= 0 ? dist[c0] : 0.0f);
    const double d1 = clearance_rules::distance_of(c1, c1 >= 0 ? dist[c1] : 0.0f);
    r.d_up = d1 < d0 || d1 != d1 ? d1 : d0;  // (a NaN stays)
    return r;
}

// whether an item goes to `depth`, from its depth-0 piece
REPORT_RULE bool is_refined(const Readings& r0, double radius, double refine_below) {
    return r0.outside || r0.over_budget || !(clearance_rules::clearance(r0.d_lo, radius) >= refine_below);
}

// A minimum and where it was found: the smallest clearance, and among equal clearances the lexicographically first (segment, piece, agent);
// a clearance of 1e9 or more, or a NaN, is never taken.  `take` keeps that minimum whatever the order candidates arrive in.  dist: the
// reading at the minimum; depth: that of the piece (0 or the call's depth; -1: none).
struct Minimum {
    double clearance, dist;
    int32_t segment, piece, agent, depth;
};
REPORT_RULE Minimum no_minimum() { return Minimum{RBP_CLEARANCE_NONE, 0.0, -1, -1, -1, -1}; }
// (one decision and six selects under it, not a chain of early returns around a struct copy: every field of the minimum moves together)
REPORT_RULE bool precedes(const Minimum& c, const Minimum& m) {
    const bool less = c.clearance < m.clearance, equal = c.clearance == m.clearance;
    const bool first = c.segment != m.segment ? c.segment < m.segment : (c.piece != m.piece ? c.piece < m.piece : c.agent < m.agent);
    return less || (equal && first);
}
REPORT_RULE void take(Minimum* m, const Minimum& c) {
    const bool p = precedes(c, *m);
    m->clearance = p ? c.clearance : m->clearance, m->dist = p ? c.dist : m->dist;
    m->segment = p ? c.segment : m->segment, m->piece = p ? c.piece : m->piece;
    m->agent = p ? c.agent : m->agent, m->depth = p ? c.depth : m->depth;
}

// what a mission's pieces add up to (rbp_swept_clearance of include/rbp.h, besides the end time and the status)
struct Tally {
    Minimum lower, upper;
    int64_t uncertified, hitting, outside, over_budget, refined;  // items
};
REPORT_RULE Tally empty_tally() { return Tally{no_minimum(), no_minimum(), 0, 0, 0, 0, 0}; }
REPORT_RULE void merge(Tally* t, const Tally& o) {
    take(&t->lower, o.lower), take(&t->upper, o.upper);
    t->uncertified += o.uncertified, t->hitting += o.hitting, t->outside += o.outside, t->over_budget += o.over_budget, t->refined += o.refined;
}

// what the evaluated pieces of one item leave: its smallest lower clearance (1e9: none was a number below 1e9) and its flags
#define RBP_SWEPT_UNCERTIFIED 1
#define RBP_SWEPT_HITTING 2
#define RBP_SWEPT_OUTSIDE 4
#define RBP_SWEPT_OVER_BUDGET 8
struct ItemState {
    double lower;
    int32_t flags;
};
REPORT_RULE ItemState empty_item() { return ItemState{RBP_CLEARANCE_NONE, 0}; }
REPORT_RULE void merge_item(ItemState* s, const ItemState& o) {
    if (o.lower < s->lower) s->lower = o.lower;
    s->flags |= o.flags;
}

// one piece's readings into the tally's minima and into the item's state
REPORT_RULE void take_piece(Tally* t, ItemState* s, const Readings& r, double radius, int32_t depth, int32_t p, int32_t m, int32_t a) {
    const double lower = clearance_rules::clearance(r.d_lo, radius), upper = clearance_rules::clearance(r.d_up, radius);
    take(&t->lower, Minimum{lower, r.d_lo, m, p, a, depth});
    take(&t->upper, Minimum{upper, r.d_up, m, p, a, depth});
    if (lower < s->lower) s->lower = lower;
    if (clearance_rules::is_hit(r.d_lo, radius)) s->flags |= RBP_SWEPT_UNCERTIFIED;
    if (clearance_rules::is_hit(r.d_up, radius)) s->flags |= RBP_SWEPT_HITTING;
    if (r.outside) s->flags |= RBP_SWEPT_OUTSIDE;
    if (r.over_budget) s->flags |= RBP_SWEPT_OVER_BUDGET;
}
// an item's counts once all its pieces are in
REPORT_RULE void count_item(Tally* t, const ItemState& s, bool refined) {
    if (s.flags & RBP_SWEPT_UNCERTIFIED) ++t->uncertified;
    if (s.flags & RBP_SWEPT_HITTING) ++t->hitting;
    if (s.flags & RBP_SWEPT_OUTSIDE) ++t->outside;
    if (s.flags & RBP_SWEPT_OVER_BUDGET) ++t->over_budget;
    if (refined) ++t->refined;
}

// One item, whole: depth 0, then `depth` where the rule says so.  Its smallest lower clearance is returned.
template <class G>
REPORT_RULE double take_item(Tally* t, const double* coef, int32_t M, const double* T, double ts, int32_t a, int32_t m, double radius,
                             const int32_t* dim, const int32_t* key_min, double rf, G dist, int32_t depth, double refine_below) {
    const Item it = item_of(coef, M, T, ts, a, m);
    const Readings r0 = piece_readings(it, 0, 0, dim, key_min, rf, dist);
    const bool refined = is_refined(r0, radius, refine_below);
    ItemState s = empty_item();
    if (refined)
        for (int32_t p = 0; p < ((int32_t)1 << depth); ++p) take_piece(t, &s, piece_readings(it, depth, p, dim, key_min, rf, dist), radius, depth, p, m, a);
    else
        take_piece(t, &s, r0, radius, 0, 0, m, a);
    count_item(t, s, refined);
    return s.lower;
}

// Everything, one item after the other: the loop of the host entry, and the meaning of every shortcut the device takes.
// T [M+1] unscaled, coef [N][3][6M], radius [N]; the grid dist [dim0][dim1][dim2] with key_min and res.  agent_lower [N] or null: every
// agent's smallest lower clearance over its segments (1e9 where none is a number).  depth in 0 .. RBP_SWEPT_MAX_DEPTH, refine_below a number.
REPORT_RULE Tally swept_sequential(int32_t N, int32_t M, const double* T, double ts, const double* coef, const double* radius,
                                   const int32_t* dim, const int32_t* key_min, double res, const float* dist, int32_t depth,
                                   double refine_below, double* agent_lower) {
    Tally t = empty_tally();
    const double rf = clearance_rules::resolution_factor(res);
    for (int32_t a = 0; a < N; ++a) {
        double al = RBP_CLEARANCE_NONE;
        for (int32_t m = 0; m < M; ++m) {
            const double lo = take_item(&t, coef, M, T, ts, a, m, radius[a], dim, key_min, rf, dist, depth, refine_below);
            if (lo < al) al = lo;
        }
        if (agent_lower) agent_lower[a] = al;
    }
    return t;
}

}  // namespace swept_rules
