// The rule of common/separation_rules.h as g++ compiles it for rbp_separation_host, checked on hand-computed cases
// (tests/test_separation_rules.py builds this program over the header ALONE, with the sanitizers, and runs it).  Trajectories are constant,
// linear or a fixed quintic whose values a long double Horner gives, so every expected number can be worked out by hand.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "common/separation_rules.h"

namespace S = separation_rules;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static const double U = std::ldexp(1.0, -53);
static double ulp(double v) { return std::nextafter(v, INFINITY) - v; }

struct Coef {
    int N, M;
    std::vector<double> c;
    Coef(int N_, int M_) : N(N_), M(M_), c((size_t)N_ * 3 * 6 * M_, 0.0) {}
    double* axis(int qi, int k, int m) { return &c[((size_t)qi * 3 + k) * 6 * M + 6 * m]; }
    void line(int qi, int k, int m, double slope, double offset) { axis(qi, k, m)[4] = slope, axis(qi, k, m)[5] = offset; }
    void stay(int qi, double x, double y, double z) {
        for (int m = 0; m < M; ++m) line(qi, 0, m, 0, x), line(qi, 1, m, 0, y), line(qi, 2, m, 0, z);
    }
};
static std::vector<double> unit_times(int M, double h = 1.0) {
    std::vector<double> T((size_t)M + 1);
    for (int m = 0; m <= M; ++m) T[m] = h * m;
    return T;
}
static S::Tally run(Coef& c, const std::vector<double>& T, const std::vector<double>& radius, double downwash, int depth, double refine_below,
                    double* pairs = nullptr) {
    return S::separation_sequential(c.N, c.M, T.data(), 1.0, c.c.data(), radius.data(), downwash, depth, refine_below, pairs);
}
// err of the item (0, 1, m) at `depth`, in squared metres
static double err_of(Coef& c, const std::vector<double>& T, int m, double downwash, int depth) {
    return S::error_term(depth, S::item_of(c.c.data(), c.M, T.data(), 1.0, 0, 1, m, downwash).S);
}

static void a_constant_offset() {
    Coef c(2, 1);
    c.stay(0, 1.0, 1.0, 1.0), c.stay(1, 4.0, 5.0, 1.0);  // (3, 4, 0)
    const std::vector<double> T = unit_times(1), radius = {0.5, 0.5};
    const int depths[3] = {0, 1, 8};
    for (int depth : depths) {
        const S::Item it = S::item_of(c.c.data(), 1, T.data(), 1.0, 0, 1, 0, 1.0);
        CHECK(it.S == 25.0);
        const double err = S::error_term(depth, it.S);
        CHECK(err == (48.0 + 10.0 * depth) * U * 25.0);
        for (int p = 0; p < (1 << depth); p += (depth == 8 ? 51 : 1)) {
            double b[18], q[11];
            for (int i = 0; i < 18; ++i) b[i] = it.b[i];
            S::piece_points(b, depth, p);
            for (int i = 0; i < 6; ++i) CHECK(b[i] == 3.0 && b[6 + i] == 4.0 && b[12 + i] == 0.0);
            S::squared_norm(b, q);
            for (int k = 0; k <= 10; ++k) CHECK(std::fabs(q[k] - 25.0) <= 8 * U * 25.0);  // (rounded weights, their products, at most five sums)
        }
        const S::Tally t = run(c, T, radius, 1.0, depth, 1e9);
        // sqrt(25 -+ 2 err) is 5 -+ err / 5, and the ratio is moved by 3 doubles on top of the two roundings
        CHECK(t.lower.ratio <= 5.0 && 5.0 - t.lower.ratio <= 2 * err / 10.0 + 5 * ulp(5.0));
        CHECK(t.upper.ratio >= 5.0 && t.upper.ratio - 5.0 <= 2 * err / 10.0 + 5 * ulp(5.0));
        CHECK(t.uncertified == 0 && t.colliding == 0 && t.refined == 1 && t.lower.depth == depth && t.upper.depth == depth);
        CHECK(t.lower.segment == 0 && t.lower.qi == 0 && t.lower.qj == 1 && t.upper.piece >= 0);
    }
}

static void a_vertical_offset_under_the_downwash() {
    Coef c(2, 2);
    c.stay(0, 1.0, 1.0, 0.5), c.stay(1, 1.0, 1.0, 2.5);  // (0, 0, 2), downwash 2: distance 1
    const std::vector<double> T = unit_times(2, 0.7), radius = {0.25, 0.75};
    for (int depth = 0; depth <= 3; ++depth) {
        const double err = err_of(c, T, 0, 2.0, depth);
        const S::Tally t = run(c, T, radius, 2.0, depth, 1e9);
        CHECK(t.lower.ratio <= 1.0 && 1.0 - t.lower.ratio <= 2 * err / 2.0 + 5 * ulp(1.0));
        CHECK(t.upper.ratio >= 1.0 && t.upper.ratio - 1.0 <= 2 * err / 2.0 + 5 * ulp(1.0));
        CHECK(t.colliding == 0);
    }
}

static void a_straight_pass() {
    // agent 0 rests at the origin; agent 1 flies (-1 + t, 0.5, 0) for h = 2: closest at the midpoint, 0.5 away
    Coef c(2, 1);
    c.stay(0, 0.0, 0.0, 0.0);
    c.line(1, 0, 0, 1.0, -1.0), c.line(1, 1, 0, 0.0, 0.5);
    const std::vector<double> T = unit_times(1, 2.0), radius = {0.5, 0.5};
    double before = -1.0, err_before = 0.0;
    for (int depth = 0; depth <= 8; ++depth) {
        const double err = err_of(c, T, 0, 2.0, depth);
        const S::Tally t = run(c, T, radius, 2.0, depth, 1e9);
        const double lower_sq = t.lower.ratio * t.lower.ratio, upper_sq = t.upper.ratio * t.upper.ratio;
        CHECK(t.lower.ratio <= 0.5 && t.upper.ratio >= 0.5);
        if (depth >= 1) {  // the midpoint is a piece end: pieces 2^(depth-1) - 1 (its last point) and 2^(depth-1) (its first)
            CHECK(upper_sq - 0.25 <= 2 * err + 16 * ulp(0.25));
            CHECK(t.upper.piece == (1 << (depth - 1)) - 1 || t.upper.piece == (1 << (depth - 1)));
        } else {
            CHECK(std::fabs(upper_sq - 1.25) <= 2 * err + 8 * ulp(1.25));  // both ends of the segment: 1 + 0.25
        }
        CHECK(lower_sq >= before - err - err_before - 16 * ulp(0.25));
        before = lower_sq, err_before = err;
        CHECK(t.uncertified == 1 && t.colliding == (depth >= 1 ? 1 : 0));
    }
    CHECK(0.25 - before <= 1e-5);  // 256 pieces: the gap closes fourfold per level
}

static void two_identical_agents() {
    Coef c(2, 3);
    for (int qi = 0; qi < 2; ++qi)
        for (int k = 0; k < 3; ++k)
            for (int m = 0; m < 3; ++m)
                for (int i = 0; i < 6; ++i) c.axis(qi, k, m)[i] = 0.25 * (i + 1) - 0.5 * k + m;
    const std::vector<double> T = unit_times(3), radius = {0.15, 0.15};
    const int depths[3] = {0, 2, 8};
    for (int depth : depths) {
        double pair = -1.0;
        const S::Tally t = run(c, T, radius, 2.0, depth, 2.0, &pair);
        CHECK(t.lower.ratio == 0.0 && t.upper.ratio == 0.0 && !std::signbit(t.lower.ratio) && pair == 0.0);
        CHECK(t.colliding == 3 && t.uncertified == 3 && t.refined == 3);
        CHECK(t.lower.segment == 0 && t.lower.piece == 0 && t.upper.segment == 0 && t.upper.piece == 0 && t.lower.depth == depth);
    }
}

static long double horner(const double* c, long double t) {
    long double v = c[0];
    for (int i = 1; i < 6; ++i) v = v * t + c[i];
    return v;
}
static void the_ends_of_a_piece_are_values_of_the_polynomial() {
    Coef c(2, 1);
    const double quintic[3][6] = {{0.03, -0.11, 0.07, 0.2, -0.4, 1.5}, {-0.02, 0.05, 0.13, -0.3, 0.25, -0.75}, {0.01, 0.0, -0.09, 0.17, 0.6, 2.0}};
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 6; ++i) c.axis(1, k, 0)[i] = quintic[k][i], c.axis(0, k, 0)[i] = 0.125 * (k + 1) * (i == 5);
    const std::vector<double> T = {0.0, 1.7};
    const double downwash = 2.0;
    const S::Item it = S::item_of(c.c.data(), 1, T.data(), 1.0, 0, 1, 0, downwash);
    const double err = S::error_term(3, it.S);
    CHECK(err <= std::ldexp(it.S, -40) && err > 0);
    for (int p = 0; p < 8; ++p) {
        double b[18], q[11];
        for (int i = 0; i < 18; ++i) b[i] = it.b[i];
        S::piece_points(b, 3, p);
        S::squared_norm(b, q);
        for (int end = 0; end < 2; ++end) {
            const long double t = (long double)T[1] * (p + end) / 8.0L;  // (h is the double)
            long double sq = 0;
            for (int k = 0; k < 3; ++k) {
                long double d = horner(c.axis(1, k, 0), t) - horner(c.axis(0, k, 0), t);
                if (k == 2) d /= downwash;
                sq += d * d;
            }
            CHECK(std::fabs((double)((long double)q[end ? 10 : 0] - sq)) <= err);
        }
    }
}

static void the_refinement_threshold() {
    Coef c(2, 1);
    c.stay(0, 0.0, 0.0, 0.0);
    c.line(1, 0, 0, 1.0, -1.0), c.line(1, 1, 0, 0.0, 0.5);
    const std::vector<double> T = unit_times(1, 2.0), radius = {0.5, 0.5};
    const S::Tally at0 = run(c, T, radius, 2.0, 0, 1e9);
    const double lower0 = at0.lower.ratio;
    CHECK(lower0 > 0.0 && lower0 < 0.5);
    const S::Tally stays = run(c, T, radius, 2.0, 3, lower0);  // lower0 >= refine_below: it stays
    CHECK(stays.refined == 0 && stays.lower.depth == 0 && stays.upper.depth == 0 && stays.lower.ratio == lower0 && stays.upper.ratio == at0.upper.ratio);
    const S::Tally goes = run(c, T, radius, 2.0, 3, std::nextafter(lower0, INFINITY));
    CHECK(goes.refined == 1 && goes.lower.depth == 3 && goes.upper.depth == 3 && goes.lower.ratio > lower0 && goes.upper.ratio < at0.upper.ratio);
    CHECK(S::is_refined(std::nan(""), 2.0) && !S::is_refined(2.0, 2.0) && S::is_refined(1.0, RBP_REPORT_NO_RATIO));
}

static void equal_minima_name_the_first() {
    const S::Minimum cands[5] = {{0.5, 1, 0, 0, 1, 3}, {0.5, 0, 2, 1, 2, 3}, {0.5, 0, 1, 2, 3, 3}, {0.5, 0, 1, 1, 4, 3}, {0.5, 0, 1, 1, 3, 3}};
    const int orders[4][5] = {{0, 1, 2, 3, 4}, {4, 3, 2, 1, 0}, {2, 4, 0, 3, 1}, {3, 0, 4, 1, 2}};
    for (const auto& order : orders) {
        S::Minimum m = S::no_minimum();
        for (int i : order) S::take(&m, cands[i]);
        CHECK(m.segment == 0 && m.piece == 1 && m.qi == 1 && m.qj == 3);
    }
    S::Minimum m = S::no_minimum();
    S::take(&m, S::Minimum{std::nan(""), 0, 0, 0, 1, 0});
    S::take(&m, S::Minimum{RBP_REPORT_NO_RATIO, 0, 0, 0, 1, 0});
    CHECK(m.ratio == RBP_REPORT_NO_RATIO && m.segment == -1 && m.depth == -1);
    // a mission of three agents at rest in one point and four segments: every bound equal; the first item is (segment 0, piece 0, 0, 1)
    Coef c(3, 4);
    for (int qi = 0; qi < 3; ++qi) c.stay(qi, 1.0, 2.0, 3.0);
    const S::Tally t = run(c, unit_times(4), {0.1, 0.1, 0.1}, 2.0, 2, 2.0);
    CHECK(t.lower.segment == 0 && t.lower.piece == 0 && t.lower.qi == 0 && t.lower.qj == 1 && t.colliding == 12);
}

static void a_nan_is_never_a_minimum() {
    Coef c(3, 2);
    c.stay(0, 0.0, 0.0, 1.0), c.stay(1, 1.0, 0.0, 1.0), c.stay(2, 0.0, 3.0, 1.0);
    const std::vector<double> T = unit_times(2), radius = {0.25, 0.25, 0.25};
    const double nan = std::nan("");
    for (int where = 0; where < 6; ++where) {
        Coef d = c;
        d.axis(0, 1, 1)[where] = nan;  // agent 0, y, second segment: its items there are NaN, every other item is a number
        double pairs[3] = {-1, -1, -1};
        const S::Tally t = run(d, T, radius, 2.0, 2, 1e9, pairs);
        CHECK(std::fabs(t.lower.ratio - 2.0) < 1e-9 && t.lower.qi == 0 && t.lower.qj == 1 && t.lower.segment == 0);
        CHECK(std::fabs(t.upper.ratio - 2.0) < 1e-9 && t.upper.segment == 0);
        CHECK(std::fabs(pairs[0] - 2.0) < 1e-9 && std::fabs(pairs[1] - 6.0) < 1e-9 && pairs[2] > 6.0 && pairs[2] < 6.4);
        CHECK(t.uncertified == 0 && t.colliding == 0 && t.refined == 6);
    }
    Coef d = c;
    for (int m = 0; m < 2; ++m) d.axis(0, 0, m)[5] = nan, d.axis(1, 0, m)[5] = nan, d.axis(2, 0, m)[5] = nan;
    double pairs[3] = {-1, -1, -1};
    const S::Tally t = run(d, T, radius, 2.0, 1, 2.0, pairs);
    CHECK(t.lower.ratio == RBP_REPORT_NO_RATIO && t.lower.segment == -1 && t.upper.ratio == RBP_REPORT_NO_RATIO && t.upper.qj == -1);
    CHECK(pairs[0] == RBP_REPORT_NO_RATIO && pairs[2] == RBP_REPORT_NO_RATIO && t.refined == 6 && t.uncertified == 0);
    Coef e = c;
    e.stay(2, 0.0, 3.0, 3.0);
    e.axis(2, 2, 0)[0] = INFINITY;  // an infinite coefficient: S and err are infinite, nothing is certified, nothing is proven
    const S::Tally ti = run(e, T, radius, 2.0, 1, 2.0);
    CHECK(ti.lower.ratio == 0.0 && ti.lower.segment == 0 && ti.lower.qi == 0 && ti.lower.qj == 2 && ti.uncertified == 2 && ti.colliding == 0);
    CHECK(std::fabs(ti.upper.ratio - 2.0) < 1e-9);
}

static void one_agent_has_no_pair() {
    Coef c(1, 2);
    c.stay(0, 1.0, 1.0, 1.0);
    const S::Tally t = run(c, unit_times(2), {0.15}, 2.0, 4, 2.0);
    CHECK(t.lower.ratio == 1e9 && t.upper.ratio == 1e9);
    CHECK(t.lower.segment == -1 && t.lower.piece == -1 && t.lower.qi == -1 && t.lower.qj == -1 && t.lower.depth == -1);
    CHECK(t.upper.segment == -1 && t.upper.piece == -1 && t.upper.qi == -1 && t.upper.qj == -1);
    CHECK(t.uncertified == 0 && t.colliding == 0 && t.refined == 0);
}

static void the_small_things() {
    CHECK(S::bernstein_weight(4, 2) == 6.0 / 10.0 && S::bernstein_weight(5, 3) == 1.0 && S::bernstein_weight(1, 1) == 1.0 / 5.0);
    CHECK(S::product_weight(0, 0) == 1.0 && S::product_weight(5, 5) == 1.0 && S::product_weight(2, 3) == 100.0 / 252.0);
    for (int k = 0; k <= 10; ++k) {
        double s = 0;
        for (int a = (k > 5 ? k - 5 : 0); a <= (k < 5 ? k : 5); ++a) s += S::product_weight(a, k - a);
        CHECK(std::fabs(s - 1.0) <= 6 * U);
    }
    CHECK(S::ratio_down(0.0, 3) == 0.0 && S::ratio_down(std::numeric_limits<double>::denorm_min(), 3) == 0.0);
    CHECK(S::ratio_down(1.0, 3) == 1.0 - 3 * U && S::ratio_up(1.0, 3) == 1.0 + 6 * U && S::ratio_up(0.0, 3) == 0.0);
    CHECK(std::isnan(S::ratio_down(std::nan(""), 3)) && std::isnan(S::ratio_up(std::nan(""), 3)) && S::ratio_up(INFINITY, 3) == INFINITY);
    CHECK(std::isinf(S::ratio_up(std::numeric_limits<double>::max(), 3)));
    CHECK(S::pair_index(5, 0, 1) == 0 && S::pair_index(5, 0, 4) == 3 && S::pair_index(5, 1, 2) == 4 && S::pair_index(5, 3, 4) == 9);
    double b[6] = {0, 0, 0, 0, 0, 32}, r[6] = {0, 0, 0, 0, 0, 32};  // t^5 * 32 on [0, 1]
    S::halve(b, false), S::halve(r, true);
    CHECK(b[5] == 1.0 && b[0] == 0.0 && r[0] == 1.0 && r[5] == 32.0 && r[4] == 16.0);
}

int main() {
    a_constant_offset();
    a_vertical_offset_under_the_downwash();
    a_straight_pass();
    two_identical_agents();
    the_ends_of_a_piece_are_values_of_the_polynomial();
    the_refinement_threshold();
    equal_minima_name_the_first();
    a_nan_is_never_a_minimum();
    one_agent_has_no_pair();
    the_small_things();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("separation rules ok\n");
    return 0;
}
