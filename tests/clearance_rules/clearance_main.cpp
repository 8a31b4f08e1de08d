// The rule of common/clearance_rules.h as g++ compiles it for rbp_clearance_host, checked on hand-computed cases (tests/test_clearance_rules.py
// builds this program over the header ALONE, with the sanitizers, and runs it).  The grid is 4 x 3 x 2 with key_min (-2, -1, 0): x keys
// -2 .. 1, y keys -1 .. 1, z keys 0 .. 1; cell c holds c / 8 (exact in float), so a lookup names its cell.  Trajectories are constant or
// linear, so every expected number can be worked out by hand: an axis of a segment is c[4] * tseg + c[5].
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "common/clearance_rules.h"

namespace C = clearance_rules;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static const int32_t DIM[3] = {4, 3, 2}, KEY_MIN[3] = {-2, -1, 0};
static std::vector<float> grid() {
    std::vector<float> g(24);
    for (int c = 0; c < 24; ++c) g[c] = (float)c * 0.125f;
    return g;
}
static int64_t cell(double res, double x, double y, double z) {
    const double p[3] = {x, y, z};
    return C::cell_of(DIM, KEY_MIN, C::resolution_factor(res), p);
}
static int64_t at(int ix, int iy, int iz) { return ((int64_t)ix * 3 + iy) * 2 + iz; }

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
static C::Result run(Coef& c, const std::vector<double>& T, double ts, const std::vector<double>& radius, double res, double dt, double* agents) {
    const std::vector<float> g = grid();
    return C::clearance_sequential(c.N, c.M, T.data(), ts, c.c.data(), radius.data(), DIM, KEY_MIN, res, g.data(), dt, agents);
}

static void a_coordinate_on_a_cell_boundary() {
    // res 0.25: rf = 4, everything exact; p = k * res lies in the cell of key k, the upper one
    CHECK(C::resolution_factor(0.25) == 4.0);
    CHECK(cell(0.25, 0.25, 0.0, 0.0) == at(3, 1, 0));
    CHECK(cell(0.25, -0.25, 0.25, 0.25) == at(1, 2, 1));
    CHECK(cell(0.25, -0.5, -0.25, 0.0) == at(0, 0, 0));
    // res 0.1: rf = 1 / 0.1 rounds to 10; the coordinate is rounded to FLOAT first: 0.1f = 0.100000001490116 > 0.1, so 1 * 0.1 has key 1,
    // but -0.1f = -0.100000001490116 has key floor(-1.0000000149) = -2, not -1; 0.7f = 0.699999988 has key 6, not 7
    CHECK(C::resolution_factor(0.1) == 10.0);
    CHECK(cell(0.1, 0.1, 0.0, 0.0) == at(3, 1, 0));
    CHECK(cell(0.1, -0.1, 0.1, 0.1) == at(0, 2, 1));
    int64_t i = -1;
    CHECK(C::axis_index(10.0, 0.7, 0, 10, &i) && i == 6);
    CHECK(C::axis_index(10.0, 3 * 0.1, 0, 10, &i) && i == 3);  // 0.30000000000000004 -> 0.3f = 0.300000012
}

static void floor_is_not_truncation() {
    CHECK(cell(0.25, -1e-9, 0.0, 0.0) == at(1, 1, 0));  // key floor(-4e-9) = -1 (truncation: 0)
    CHECK(cell(0.25, 1e-9, 0.0, 0.0) == at(2, 1, 0));
    CHECK(cell(0.25, 0.0, -1e-9, 0.0) == at(2, 0, 0));
    CHECK(cell(0.25, 0.0, 0.0, -1e-9) == -1);            // z key -1: below the grid
}

static void the_float_cast_matters() {
    const double p = 0.25 - 1e-12;  // a double below the boundary whose nearest float IS the boundary (floats near 0.25 are 1.5e-8 apart)
    CHECK(p < 0.25 && floor(4.0 * p) == 0.0 && (float)p == 0.25f);
    CHECK(cell(0.25, p, 0.0, 0.0) == at(3, 1, 0));  // key 1, where the double alone would give key 0
    CHECK(cell(0.25, 0.0, 0.0, 0.5 - 1e-12) == -1);  // ... and across the grid's edge: z key 2
}

static void one_step_outside_on_each_side() {
    CHECK(cell(0.25, -0.5, 0.0, 0.0) == at(0, 1, 0) && cell(0.25, -0.51, 0.0, 0.0) == -1);   // x key -2 | -3
    CHECK(cell(0.25, 0.49, 0.0, 0.0) == at(3, 1, 0) && cell(0.25, 0.5, 0.0, 0.0) == -1);     // x key 1 | 2
    CHECK(cell(0.25, 0.0, -0.25, 0.0) == at(2, 0, 0) && cell(0.25, 0.0, -0.26, 0.0) == -1);  // y key -1 | -2
    CHECK(cell(0.25, 0.0, 0.49, 0.0) == at(2, 2, 0) && cell(0.25, 0.0, 0.5, 0.0) == -1);     // y key 1 | 2
    CHECK(cell(0.25, 0.0, 0.0, 0.0) == at(2, 1, 0) && cell(0.25, 0.0, 0.0, -0.01) == -1);    // z key 0 | -1
    CHECK(cell(0.25, 0.0, 0.0, 0.49) == at(2, 1, 1) && cell(0.25, 0.0, 0.0, 0.5) == -1);     // z key 1 | 2
    CHECK(C::distance_of(-1, 0.0f) == -1.0 && C::distance_of(5, 0.625f) == 0.625);
}

static void positions_that_are_no_numbers_are_outside() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double bad : {nan, inf, -inf, 1e300, -1e300, 3e9, -3e9, 1e38}) {  // (3e9 * 4 is beyond int; 1e38 is a finite float)
        CHECK(cell(0.25, bad, 0.0, 0.0) == -1);
        CHECK(cell(0.25, 0.0, bad, 0.0) == -1);
        CHECK(cell(0.25, 0.0, 0.0, bad) == -1);
    }
    const int32_t wide[3] = {2147483647, 1, 1}, low[3] = {-2147483647 - 1, 0, 0};
    const double p[3] = {1e300, 0.0, 0.0}, q[3] = {-2147483648.0, 0.0, 0.0};
    CHECK(C::cell_of(wide, low, 1.0, p) == -1);
    CHECK(C::cell_of(wide, low, 1.0, q) == 0);  // the lowest key an int holds: index 0, no overflow on the way
}

static void the_hit_threshold() {
    const double r = 0.15, thr = r - 1e-6;
    CHECK(!C::is_hit(thr, r));                       // d == r - 1e-6: not a hit
    CHECK(C::is_hit(std::nextafter(thr, -1.0), r));  // one ulp below: a hit
    CHECK(!C::is_hit(std::nextafter(thr, 1.0), r));
    CHECK(C::is_hit(-1.0, 0.0) && C::is_hit(-1.0, -0.5) && !C::is_hit(-1.0, -1.0));  // outside is a hit for any radius above -1 + 1e-6
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(!C::is_hit(0.0, nan));
    CHECK(C::clearance(0.625, 0.5) == 0.125 && C::clearance(-1.0, 0.5) == -1.5);
}

static void equal_clearances_report_the_first_sample_then_agent() {
    const C::Minimum c[4] = {{0.5, 0.75, 3, 1}, {0.5, 0.75, 2, 5}, {0.5, 0.75, 2, 4}, {0.75, 1.0, 0, 0}};
    const int orders[4][4] = {{0, 1, 2, 3}, {3, 2, 1, 0}, {2, 0, 3, 1}, {1, 3, 0, 2}};
    for (const auto& o : orders) {
        C::Minimum m = C::no_minimum();
        for (int i : o) C::take(&m, c[i]);
        CHECK(m.clearance == 0.5 && m.sample == 2 && m.agent == 4 && m.dist == 0.75);
    }
    C::Minimum m = C::no_minimum();
    CHECK(m.clearance == 1e9 && m.dist == 0.0 && m.sample == -1 && m.agent == -1);
    C::take(&m, C::Minimum{std::numeric_limits<double>::quiet_NaN(), 0.0, 0, 0});
    C::take(&m, C::Minimum{1e9, 0.0, 0, 0});
    C::take(&m, C::Minimum{2e9, 0.0, 0, 0});
    CHECK(m.clearance == 1e9 && m.sample == -1 && m.agent == -1);  // a NaN, 1e9 or more: never taken
    C::take(&m, C::Minimum{-std::numeric_limits<double>::infinity(), -1.0, 7, 7});
    C::take(&m, C::Minimum{std::numeric_limits<double>::quiet_NaN(), 0.0, 0, 0});
    CHECK(m.sample == 7 && m.agent == 7);
}

static void the_whole_loop() {
    // two agents at rest, three samples (floor(0.375 / 0.1)); agent 0 in cell (2, 1, 0) = 14 -> 1.75, agent 1 at (-0.3, 0.3, 0.3):
    // keys floor(-1.2000000477) = -2, 1, 1 -> cell (0, 2, 1) = 5 -> 0.625
    Coef c(2, 1);
    c.stay(0, 0.1, 0.1, 0.1), c.stay(1, -0.3, 0.3, 0.3);
    double agents[2] = {-7.0, -7.0};
    C::Result r = run(c, {0, 0.375}, 1.0, {0.5, 0.7}, 0.25, 0.1, agents);
    CHECK(r.samples == 3 && r.end_time == 0.375 && r.hits == 3 && r.outside == 0);  // 0.625 < 0.7 - 1e-6 at every sample
    CHECK(r.min.clearance == 0.625 - 0.7 && r.min.dist == 0.625 && r.min.sample == 0 && r.min.agent == 1);
    CHECK(agents[0] == 1.25 && agents[1] == 0.625 - 0.7);
    // agent 0 now flies along x at 2 m/s: 0.1 (key 0), 0.3 (key 1), 0.5 (key 2: outside) -- d = -1 at sample 2, a hit and the minimum
    c.line(0, 0, 0, 2.0, 0.1);
    r = run(c, {0, 0.375}, 1.0, {0.5, 0.7}, 0.25, 0.1, agents);
    CHECK(r.hits == 4 && r.outside == 1 && r.min.clearance == -1.5 && r.min.dist == -1.0 && r.min.sample == 2 && r.min.agent == 0);
    CHECK(agents[0] == -1.5 && agents[1] == 0.625 - 0.7);
    // a time scale of 2 doubles the end time: seven samples (floor(0.75 / 0.1)), agent 0 outside from sample 2 on
    r = run(c, {0, 0.375}, 2.0, {0.5, 0.7}, 0.25, 0.1, nullptr);
    CHECK(r.samples == 7 && r.end_time == 0.75 && r.outside == 5 && r.hits == 7 + 5 && r.min.sample == 2 && r.min.agent == 0);
    // ties: both agents in one cell with one radius at every sample -> (sample 0, agent 0)
    Coef t(2, 1);
    t.stay(0, 0.1, 0.1, 0.1), t.stay(1, 0.2, 0.2, 0.2);
    r = run(t, {0, 0.375}, 1.0, {0.5, 0.5}, 0.25, 0.1, agents);
    CHECK(r.min.clearance == 1.25 && r.min.sample == 0 && r.min.agent == 0 && r.hits == 0 && agents[0] == 1.25 && agents[1] == 1.25);
}

static void a_nan_radius_is_never_the_minimum() {
    Coef c(2, 1);
    c.stay(0, -0.3, 0.3, 0.3), c.stay(1, 0.1, 0.1, 0.1);  // agent 0 would be the minimum (0.625 against 1.75)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double agents[2] = {-7.0, -7.0};
    C::Result r = run(c, {0, 0.375}, 1.0, {nan, 0.5}, 0.25, 0.1, agents);
    CHECK(r.min.agent == 1 && r.min.sample == 0 && r.min.clearance == 1.25 && r.hits == 0 && r.outside == 0);
    CHECK(agents[0] == 1e9 && agents[1] == 1.25);
    r = run(c, {0, 0.375}, 1.0, {nan, nan}, 0.25, 0.1, agents);
    CHECK(r.min.clearance == 1e9 && r.min.dist == 0.0 && r.min.sample == -1 && r.min.agent == -1 && agents[0] == 1e9 && agents[1] == 1e9);
    // a NaN coefficient: the position is no number, the lookup outside, the item a hit
    c.axis(1, 2, 0)[5] = nan;
    r = run(c, {0, 0.375}, 1.0, {0.5, 0.5}, 0.25, 0.1, agents);
    CHECK(r.outside == 3 && r.hits == 3 && r.min.agent == 1 && r.min.sample == 0 && r.min.dist == -1.0 && r.min.clearance == -1.5);
}

static void no_sample_and_too_many() {
    Coef c(2, 1);
    c.stay(0, 0.1, 0.1, 0.1), c.stay(1, 0.1, 0.1, 0.1);
    double agents[2] = {-7.0, -7.0};
    C::Result r = run(c, {0, 0.05}, 1.0, {0.5, 0.5}, 0.25, 0.1, agents);
    CHECK(r.samples == 0 && r.min.clearance == 1e9 && r.min.dist == 0.0 && r.min.sample == -1 && r.min.agent == -1 && r.hits == 0 && r.outside == 0);
    CHECK(agents[0] == 1e9 && agents[1] == 1e9);
    agents[0] = agents[1] = -7.0;
    r = run(c, {0, 2000.0}, 1.0, {0.5, 0.5}, 0.25, 1e-3, agents);
    CHECK(r.samples == -1 && r.end_time == 2000.0 && r.min.clearance == 1e9 && r.min.sample == -1 && r.hits == 0);
    CHECK(agents[0] == -7.0 && agents[1] == -7.0);  // not evaluated: left untouched
}

int main() {
    a_coordinate_on_a_cell_boundary();
    floor_is_not_truncation();
    the_float_cast_matters();
    one_step_outside_on_each_side();
    positions_that_are_no_numbers_are_outside();
    the_hit_threshold();
    equal_clearances_report_the_first_sample_then_agent();
    the_whole_loop();
    a_nan_radius_is_never_the_minimum();
    no_sample_and_too_many();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("clearance rules ok\n");
    return 0;
}
