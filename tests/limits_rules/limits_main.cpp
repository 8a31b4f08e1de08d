// The rule of common/limits_rules.h as g++ compiles it for rbp_limits_host, checked on hand-computed cases (tests/test_limits_rules.py
// builds this program over the header ALONE, with the sanitizers, and runs it).  Trajectories are of low degree on segments of one second,
// so every expected control point can be worked out by hand.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "common/limits_rules.h"

namespace W = limits_rules;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static const double U = std::ldexp(1.0, -53);
static const double INF = std::numeric_limits<double>::infinity();
static const double QNAN = std::numeric_limits<double>::quiet_NaN();

struct Plan {
    int N, M;
    std::vector<double> c, T, max_vel, max_acc;
    Plan(int N_, int M_, double h = 1.0) : N(N_), M(M_), c((size_t)N_ * 3 * 6 * M_, 0.0), T((size_t)M_ + 1), max_vel((size_t)N_ * 3, 1.0), max_acc((size_t)N_ * 3, 1.0) {
        for (int m = 0; m <= M; ++m) T[m] = h * m;
    }
    double* axis(int a, int k, int m) { return &c[((size_t)a * 3 + k) * 6 * M + 6 * m]; }
    W::Tally run(int depth, double refine_above, double* agents = nullptr) {
        return W::limits_sequential(N, M, T.data(), 1.0, c.data(), max_vel.data(), max_acc.data(), depth, refine_above, agents);
    }
};
static bool none(const W::Peak& p) { return p.ratio == 0.0 && p.segment == -1 && p.piece == -1 && p.agent == -1 && p.axis == -1 && p.depth == -1; }
static bool at(const W::Peak& p, int segment, int piece, int agent, int axis, int depth) {
    return p.segment == segment && p.piece == piece && p.agent == agent && p.axis == axis && p.depth == depth;
}
static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

static void an_agent_at_rest() {
    Plan p(1, 2);
    for (int m = 0; m < 2; ++m) p.axis(0, 0, m)[5] = 1.2, p.axis(0, 1, m)[5] = -3.0, p.axis(0, 2, m)[5] = 0.7;
    for (int depth : {0, 1, 8})
        for (double above : {-1.0, 0.5, 1e9}) {
            double agents[2] = {7, 7};
            const W::Tally t = p.run(depth, above, agents);
            CHECK(none(t.lower_vel) && none(t.upper_vel) && none(t.lower_acc) && none(t.upper_acc));
            CHECK(t.uncertified == 0 && t.violating == 0 && t.refined == (above < 0 ? 2 : 0));
            CHECK(agents[0] == 0.0 && agents[1] == 0.0);
        }
}

static void a_constant_velocity() {
    Plan p(1, 1);
    p.axis(0, 1, 0)[4] = -0.5, p.axis(0, 1, 0)[5] = 1.0;  // y = 1 - 0.5 t
    p.max_vel[1] = 2.0;
    CHECK(W::error_constant(0) == 16.0 && W::error_constant(8) == 48.0);
    CHECK(W::error_term(0, 0.5) == 16.0 * U * 0.5 && W::error_term(8, 0.5) == 48.0 * U * 0.5);
    for (int depth = 0; depth <= 8; ++depth) {
        const W::Tally t = p.run(depth, -1.0);
        const double err = W::error_term(depth, 0.5);  // V = |gamma_0| = 0.5
        CHECK(t.lower_vel.ratio <= 0.25 && 0.25 <= t.upper_vel.ratio);
        CHECK(t.upper_vel.ratio - t.lower_vel.ratio <= 2 * err / 2.0 + 8 * U);  // within err of each other, the four doubles moved outwards besides
        CHECK(at(t.lower_vel, 0, 0, 0, 1, depth) && at(t.upper_vel, 0, 0, 0, 1, depth));  // every piece has the same bounds: the first one is named
        CHECK(none(t.lower_acc) && none(t.upper_acc));
        CHECK(t.uncertified == 0 && t.violating == 0 && t.refined == 1);
    }
}

// x(t) = -1.6 t^3 + 2.4 t^2 on one second: v = 4.8 t (1 - t), control points 0, 1.2, 1.6, 1.2, 0; a = 4.8 - 9.6 t, control points 4.8,
// 1.6, -1.6, -4.8.  The samples t = 0, 0.4, 0.8 see no more than 1.152 of a limit of 1.17; the peak is 1.2 at t = 0.5.
static void the_parabola_the_samples_miss() {
    Plan p(1, 1);
    p.axis(0, 0, 0)[2] = -1.6, p.axis(0, 0, 0)[3] = 2.4;
    p.max_vel[0] = 1.17, p.max_acc[0] = 10.0;
    double gamma[5], hp[6], b[5];
    separation_rules::powers_of(1.0, hp);
    W::derivative_coefficients<4>(p.axis(0, 0, 0), gamma);
    CHECK(gamma[0] == 0.0 && gamma[1] == 2.0 * 2.4 && gamma[2] == 3.0 * -1.6 && gamma[3] == 0.0 && gamma[4] == 0.0);
    W::bernstein_form<4>(gamma, hp, b);
    const double want_v[5] = {0, 1.2, 1.6, 1.2, 0};
    for (int i = 0; i < 5; ++i) CHECK(near(b[i], want_v[i], 8 * U * 9.6));
    W::derivative_coefficients<3>(p.axis(0, 0, 0), gamma);
    CHECK(gamma[0] == 2.0 * 2.4 && gamma[1] == 6.0 * -1.6 && gamma[2] == 0.0 && gamma[3] == 0.0);
    W::bernstein_form<3>(gamma, hp, b);
    const double want_a[4] = {4.8, 1.6, -1.6, -4.8};
    for (int i = 0; i < 4; ++i) CHECK(near(b[i], want_a[i], 8 * U * 14.4));
    {
        const W::Tally t = p.run(0, 1e9);
        CHECK(near(t.upper_vel.ratio, 1.6 / 1.17, 1e-13) && t.upper_vel.ratio >= 1.2 / 1.17);
        CHECK(none(t.lower_vel));  // both ends are at rest
        CHECK(near(t.upper_acc.ratio, 0.48, 1e-13) && near(t.lower_acc.ratio, 0.48, 1e-13) && t.lower_acc.ratio <= t.upper_acc.ratio);
        CHECK(t.uncertified == 1 && t.violating == 0 && t.refined == 0);
    }
    for (int depth = 1; depth <= 8; ++depth) {
        const W::Tally t = p.run(depth, 0.5);
        CHECK(near(t.lower_vel.ratio, 1.2 / 1.17, 1e-13) && t.lower_vel.ratio > 1.0 && t.lower_vel.ratio <= 1.2 / 1.17);
        CHECK(t.upper_vel.ratio >= 1.2 / 1.17 && t.upper_vel.ratio >= t.lower_vel.ratio && t.upper_vel.ratio < 1.6 / 1.17);
        // the witness is the end of the piece before t = 0.5, which is also the start of the next: the first of the two is named
        CHECK(at(t.lower_vel, 0, (1 << (depth - 1)) - 1, 0, 0, depth));
        CHECK(t.uncertified == 1 && t.violating == 1 && t.refined == 1);
    }
}

// x(t) = t^2: v = 2 t with control points 0, 0.5, 1, 1.5, 2 (exact), a = 2.  Left half 0 .. 1, right half 1 .. 2.
static void both_halves_of_a_segment() {
    Plan p(1, 1);
    p.axis(0, 0, 0)[3] = 1.0;
    p.max_vel[0] = 4.0, p.max_acc[0] = 4.0;
    double gamma[5], hp[6], whole[5];
    separation_rules::powers_of(1.0, hp);
    W::derivative_coefficients<4>(p.axis(0, 0, 0), gamma);
    W::bernstein_form<4>(gamma, hp, whole);
    CHECK(W::poly_size<4>(gamma, hp) == 2.0);
    for (int i = 0; i < 5; ++i) CHECK(whole[i] == 0.5 * i);
    for (int half = 0; half < 2; ++half) {
        double b[5];
        std::copy(whole, whole + 5, b);
        W::piece_points<4>(b, 1, half);
        for (int i = 0; i < 5; ++i) CHECK(b[i] == half + 0.25 * i);
        const W::Bounds bd = W::piece_bounds<4>(b, W::error_term(1, 2.0), 4.0);
        const double end = half ? 0.5 : 0.25;
        CHECK(bd.lower <= end && end <= bd.upper && bd.upper - bd.lower <= 2 * 20 * U * 2.0 / 4.0 + 8 * U);
    }
    {  // the third of four quarters: 1 .. 1.5
        double b[5];
        std::copy(whole, whole + 5, b);
        W::piece_points<4>(b, 2, 2);
        for (int i = 0; i < 5; ++i) CHECK(b[i] == 1.0 + 0.125 * i);
    }
    const W::Tally t = p.run(1, -1.0);
    CHECK(at(t.upper_vel, 0, 1, 0, 0, 1) && at(t.lower_vel, 0, 1, 0, 0, 1) && near(t.upper_vel.ratio, 0.5, 1e-14) && near(t.lower_vel.ratio, 0.5, 1e-14));
    CHECK(at(t.upper_acc, 0, 0, 0, 0, 1) && near(t.upper_acc.ratio, 0.5, 1e-14) && near(t.lower_acc.ratio, 0.5, 1e-14));
    CHECK(t.uncertified == 0 && t.violating == 0);
}

static void no_numbers() {
    for (int which = 0; which < 2; ++which) {
        Plan p(2, 1);
        p.axis(1, 2, 0)[4] = which ? INF : QNAN;
        p.axis(0, 0, 0)[4] = 0.5;
        double agents[4] = {7, 7, 7, 7};
        const W::Tally t = p.run(3, 1e9, agents);  // (only what is no number below 1e9 is refined: the second agent's item)
        CHECK(t.uncertified == 1 && t.violating == 0 && t.refined == 1);
        if (which)
            CHECK(t.upper_vel.ratio == INF && at(t.upper_vel, 0, 0, 1, 2, 3));  // (an infinite upper ratio is a peak; the lower one is no number)
        else
            CHECK(at(t.upper_vel, 0, 0, 0, 0, 0) && near(t.upper_vel.ratio, 0.5, 1e-14));  // a NaN is never a peak
        CHECK(at(t.lower_vel, 0, 0, 0, 0, 0) && none(t.lower_acc) && none(t.upper_acc));
        CHECK(near(agents[0], 0.5, 1e-14) && agents[1] == 0.0 && agents[2] == INF && agents[3] == 0.0);
    }
    for (double limit : {QNAN, 0.0, -1.0}) {
        Plan p(1, 1);
        p.axis(0, 0, 0)[4] = 0.5;
        p.max_vel[0] = limit;
        double agents[2] = {7, 7};
        const W::Tally t = p.run(2, 0.5, agents);
        CHECK(t.uncertified == 1 && t.violating == 0 && t.refined == 1);
        CHECK(none(t.lower_vel) && none(t.upper_vel) && none(t.lower_acc) && none(t.upper_acc));
        CHECK(agents[0] == INF && agents[1] == 0.0);
        p.axis(0, 0, 0)[4] = 0.0;  // at rest, and still nothing is certified of that axis
        CHECK(p.run(2, 0.5).uncertified == 1);
    }
}

static void ties_in_every_order() {
    std::vector<W::Peak> c = {{0.75, 1, 2, 3, 1, 4, 0}, {0.75, 1, 2, 3, 0, 4, 0}, {0.75, 1, 2, 2, 2, 4, 0}, {0.75, 1, 1, 5, 2, 4, 0},
                              {0.75, 0, 9, 9, 2, 0, 0}, {0.5, 0, 0, 0, 0, 4, 0},  {0.0, 0, 0, 0, 0, 4, 0},  {-1.0, 0, 0, 0, 0, 4, 0},
                              {QNAN, 0, 0, 0, 0, 4, 0}};
    std::vector<int> order(c.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    int seen = 0;
    do {
        W::Peak m = W::no_peak();
        for (int i : order) W::take(&m, c[(size_t)i]);
        CHECK(m.ratio == 0.75 && at(m, 0, 9, 9, 2, 0));
        ++seen;
    } while (std::next_permutation(order.begin(), order.end()) && seen < 40320);
    W::Peak m = W::no_peak();
    for (size_t i = 5; i < c.size(); ++i) W::take(&m, c[i]);
    CHECK(m.ratio == 0.5 && at(m, 0, 0, 0, 0, 4));
    m = W::no_peak();
    for (size_t i = 6; i < c.size(); ++i) W::take(&m, c[i]);
    CHECK(none(m));
    // merge in both orders
    W::Tally x = W::empty_tally(), y = W::empty_tally();
    x.upper_vel = c[0], x.lower_acc = c[5], x.uncertified = 1, x.refined = 2;
    y.upper_vel = c[1], y.lower_vel = c[3], y.violating = 3, y.refined = 5;
    W::Tally xy = x, yx = y;
    W::merge(&xy, y), W::merge(&yx, x);
    for (const W::Tally* t : {&xy, &yx}) {
        CHECK(at(t->upper_vel, 1, 2, 3, 0, 4) && at(t->lower_vel, 1, 1, 5, 2, 4) && at(t->lower_acc, 0, 0, 0, 0, 4) && none(t->upper_acc));
        CHECK(t->uncertified == 1 && t->violating == 3 && t->refined == 7);
    }
    // two identical agents and two identical segments: the first segment, the first agent
    Plan p(2, 2);
    for (int a = 0; a < 2; ++a)
        for (int seg = 0; seg < 2; ++seg) p.axis(a, 1, seg)[3] = 0.25, p.axis(a, 1, seg)[4] = 0.125;
    for (double above : {-1.0, 1e9}) {
        const W::Tally t = p.run(2, above);
        const int d = above < 0 ? 2 : 0;
        CHECK(at(t.upper_vel, 0, d ? 3 : 0, 0, 1, d) && at(t.lower_vel, 0, d ? 3 : 0, 0, 1, d));
        CHECK(at(t.upper_acc, 0, 0, 0, 1, d) && at(t.lower_acc, 0, 0, 0, 1, d));
    }
}

static void refine_above_at_the_depth_0_ratio() {
    Plan p(1, 1);
    p.axis(0, 0, 0)[3] = 1.0;
    p.max_vel[0] = 4.0, p.max_acc[0] = 8.0;
    const double upper0 = p.run(0, 1e9).upper_vel.ratio;
    CHECK(near(upper0, 0.5, 1e-14));
    CHECK(p.run(3, upper0).refined == 0 && p.run(3, upper0).upper_vel.depth == 0);
    CHECK(p.run(3, std::nextafter(upper0, 0.0)).refined == 1 && p.run(3, std::nextafter(upper0, 0.0)).upper_vel.depth == 3);
    CHECK(p.run(3, INF).refined == 0 && p.run(3, -INF).refined == 1);
}

static void the_ratios_move_outwards() {
    CHECK(W::ratio_of(1.0, 4.0) == 0.25 && W::ratio_of(0.0, 4.0) == 0.0 && W::ratio_of(1.0, 0.0) != W::ratio_of(1.0, 0.0));
    const double b[5] = {-3.0, 1.0, -5.0, 2.0, 4.0};
    const W::Bounds bd = W::piece_bounds<4>(b, 0.0, 2.0);
    CHECK(bd.upper == std::nextafter(std::nextafter(2.5, 3.0), 3.0) && bd.lower == std::nextafter(std::nextafter(2.0, 0.0), 0.0));
    const double z[4] = {0.0, 0.0, 0.0, 0.0};
    const W::Bounds bz = W::piece_bounds<3>(z, 0.0, 2.0);
    CHECK(bz.upper == 0.0 && bz.lower == 0.0);
}

int main() {
    an_agent_at_rest();
    a_constant_velocity();
    the_parabola_the_samples_miss();
    both_halves_of_a_segment();
    no_numbers();
    ties_in_every_order();
    refine_above_at_the_depth_0_ratio();
    the_ratios_move_outwards();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("limits rules ok\n");
    return 0;
}
