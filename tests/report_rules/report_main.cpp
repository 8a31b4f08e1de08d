// The rule of common/report_rules.h as g++ compiles it for rbp_report_host, checked on hand-computed cases (tests/test_report_rules.py
// builds this program over the header ALONE, with the sanitizers, and runs it).  Trajectories are piecewise linear or constant, so every
// expected number can be worked out by hand: an axis of a segment is c[4] * tseg + c[5].
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "common/report_rules.h"

namespace R = report_rules;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// coef [N][3][6M], all zero; line() makes axis k of agent qi in segment m the line slope * tseg + offset
struct Coef {
    int N, M;
    std::vector<double> c;
    Coef(int N_, int M_) : N(N_), M(M_), c((size_t)N_ * 3 * 6 * M_, 0.0) {}
    double* at(int qi, int k, int m) { return &c[((size_t)qi * 3 + k) * 6 * M + 6 * m]; }
    void line(int qi, int k, int m, double slope, double offset) { at(qi, k, m)[4] = slope, at(qi, k, m)[5] = offset; }
    void stay(int qi, double x, double y, double z) {
        for (int m = 0; m < M; ++m) line(qi, 0, m, 0, x), line(qi, 1, m, 0, y), line(qi, 2, m, 0, z);
    }
};

static R::Result run(Coef& c, const std::vector<double>& T, double ts, const std::vector<double>& radius, double downwash, double dt) {
    std::vector<double> scratch((size_t)7 * c.N);
    return R::report_sequential(c.N, c.M, T.data(), ts, c.c.data(), radius.data(), downwash, dt, scratch.data());
}

static void horner_and_elements() {
    const double c[6] = {1, 2, 3, 4, 5, 6};
    CHECK(R::position(c, 2.0) == 120.0);  // 32 + 32 + 24 + 16 + 10 + 6
    CHECK(R::position(c, 0.0) == 6.0);
    const double a[3] = {0, 0, 0}, b[3] = {0, 0, 2}, d[3] = {3, 4, 0};
    CHECK(R::safety_ratio(a, b, 2.0, 0.3) == 1.0 / 0.3);  // dz = 2 / downwash = 1
    CHECK(R::safety_ratio(a, d, 2.0, 0.5) == 10.0);       // 5 / 0.5
    CHECK(R::step_length(a, d) == 5.0 && R::step_length(d, a) == 5.0);
    CHECK(R::step_length(a, b) == 2.0);                   // no downwash in a step
}

static void a_sample_on_a_knot_belongs_to_the_earlier_segment() {
    const std::vector<double> T = {0, 1, 2};
    CHECK(10 * 0.1 == 1.0);
    CHECK(R::sample_time(10, 0.1) == 1.0);
    CHECK(R::segments_before(T.data(), 2, 1.0, R::sample_time(0, 0.1), 0) == 0);   // t = 0: nothing begins before it, segment 0, tseg = t
    CHECK(R::segments_before(T.data(), 2, 1.0, R::sample_time(1, 0.1), 0) == 1);
    CHECK(R::segments_before(T.data(), 2, 1.0, R::sample_time(10, 0.1), 0) == 1);  // Ts[1] = 1.0 < 1.0 is false
    CHECK(R::segments_before(T.data(), 2, 1.0, R::sample_time(11, 0.1), 0) == 2);
    CHECK(R::segments_before(T.data(), 2, 1.0, R::sample_time(11, 0.1), 1) == 2);  // ... continued from an earlier count
    CHECK(R::segments_before(T.data(), 2, 1.0, 100.0, 0) == 2);                    // Ts[M] itself starts no segment
    CHECK(R::segment_index(0) == 0 && R::segment_index(1) == 0 && R::segment_index(2) == 1);
    Coef c(1, 2);
    c.line(0, 0, 0, 1.0, 0.0), c.line(0, 0, 1, 1.0, 100.0);  // x = tseg, then 100 + tseg
    double p[3];
    R::agent_position(c.c.data(), 2, T.data(), 1.0, 0, 1.0, 1, p);
    CHECK(p[0] == 1.0 && p[1] == 0.0 && p[2] == 0.0);        // still the first segment, at its end
    R::agent_position(c.c.data(), 2, T.data(), 1.0, 0, R::sample_time(11, 0.1), 2, p);
    CHECK(p[0] == 100.0 + (11 * 0.1 - 1.0));
    R::agent_position(c.c.data(), 2, T.data(), 1.0, 0, 0.0, 0, p);
    CHECK(p[0] == 0.0);
}

static void three_tenths_lie_just_past_0_3() {
    const std::vector<double> T = {0, 0.3, 1};
    CHECK(3 * 0.1 > 0.3);
    CHECK(R::segments_before(T.data(), 2, 1.0, R::sample_time(3, 0.1), 0) == 2);  // segment 1, tseg = one rounding error
    CHECK(R::segment_time(T.data(), 1.0, R::sample_time(3, 0.1), 2) == 3 * 0.1 - 0.3);
    CHECK(R::segment_time(T.data(), 1.0, R::sample_time(3, 0.1), 2) > 0 && R::segment_time(T.data(), 1.0, R::sample_time(3, 0.1), 2) < 1e-16);
    CHECK(R::segments_before(T.data(), 2, 1.0, R::sample_time(2, 0.1), 0) == 1);
}

static void samples_are_a_floor_and_few_samples_give_no_distance() {
    CHECK(R::sample_count(0.97, 0.1) == 9);  // 9.7: a floor, not a round
    CHECK(R::sample_count(1.0, 0.1) == 10);
    CHECK(R::sample_count(0.05, 0.1) == 0 && R::sample_count(0.0, 0.1) == 0 && R::sample_count(-1.0, 0.1) == 0);
    CHECK(R::sample_count(std::numeric_limits<double>::quiet_NaN(), 0.1) == 0);
    CHECK(R::sample_count(0.15, 0.1) == 1);
    const std::vector<double> radius = {0.15, 0.15};
    for (double end : {0.05, 0.15}) {
        Coef c(2, 1);
        c.line(0, 0, 0, 1.0, 0.0), c.line(0, 1, 0, 0.0, 0.0);  // agent 0 moves along x
        c.stay(1, 0.0, 3.0, 0.0);
        const R::Result r = run(c, {0, end}, 1.0, radius, 2.0, 0.1);
        CHECK(r.samples == (end < 0.1 ? 0 : 1) && r.end_time == end && r.total_flight_distance == 0.0);
        if (r.samples == 0)
            CHECK(r.min_safety_ratio == 1e9 && r.min_sample == -1 && r.min_qi == -1 && r.min_qj == -1);
        else
            CHECK(r.min_safety_ratio == 10.0 && r.min_sample == 0 && r.min_qi == 0 && r.min_qj == 1);  // 3 / 0.3
    }
}

static void one_agent_has_no_ratio_but_a_distance() {
    Coef c(1, 1);
    c.line(0, 0, 0, 3.0, 1.0), c.line(0, 1, 0, 4.0, -1.0);  // speed 5
    const R::Result r = run(c, {0, 1}, 1.0, {0.15}, 2.0, 0.25);
    CHECK(r.samples == 4);  // t = 0, 0.25, 0.5, 0.75: three steps of 1.25, all exact in binary
    CHECK(r.total_flight_distance == 3.75);
    CHECK(r.min_safety_ratio == 1e9 && r.min_sample == -1 && r.min_qi == -1 && r.min_qj == -1);
}

static void the_distance_is_a_sum_per_agent_then_over_agents() {
    // agent 0 walks 5e15 per step, agents 1 and 2 walk 1 per step, two steps: per agent 1e16, 2, 2, then (1e16 + 2) + 2 = 1e16 + 4;
    // one running sum over all steps would lose every 1 against 1e16 (half an ulp there, and the tie goes to the even 1e16) and end at 1e16
    Coef c(3, 1);
    c.line(0, 0, 0, 5e15, 0.0), c.line(1, 1, 0, 1.0, 0.0), c.line(2, 2, 0, 1.0, 0.0);
    c.line(1, 0, 0, 0.0, -5.0), c.line(2, 0, 0, 0.0, -9.0);
    const R::Result r = run(c, {0, 3}, 1.0, {0.1, 0.1, 0.1}, 2.0, 1.0);
    CHECK(r.samples == 3);
    CHECK(r.total_flight_distance == 1e16 + 4 && 1e16 + 4 != 1e16);
    CHECK(1e16 + 1 == 1e16);
}

static void equal_ratios_report_the_smaller_index() {
    Coef c(3, 2);
    c.stay(0, 0, 0, 0), c.stay(1, 1, 0, 0), c.stay(2, 2, 0, 0);
    const R::Result r = run(c, {0, 1, 2}, 1.0, {0.2, 0.2, 0.2}, 2.0, 0.1);
    CHECK(r.samples == 20);
    CHECK(r.min_safety_ratio == 2.5 && r.min_sample == 0 && r.min_qi == 0 && r.min_qj == 1);  // (1, 2) and every later sample tie
    CHECK(r.total_flight_distance == 0.0);
    // the same minimum whatever the order candidates arrive in
    const R::Minimum cand[4] = {{2.5, 3, 1, 2}, {2.5, 3, 0, 2}, {2.5, 1, 1, 2}, {3.0, 0, 0, 1}};
    for (int rot = 0; rot < 4; ++rot) {
        R::Minimum m = R::no_minimum();
        for (int i = 0; i < 4; ++i) R::take(&m, cand[(i + rot) % 4]);
        CHECK(m.ratio == 2.5 && m.sample == 1 && m.qi == 1 && m.qj == 2);
    }
    R::Minimum m = R::no_minimum();
    R::take(&m, R::Minimum{1e9, 0, 0, 1});  // `r < 1e9` is false: never taken
    CHECK(m.sample == -1 && m.qi == -1 && m.qj == -1 && m.ratio == 1e9);
    R::take(&m, R::Minimum{2e9, 0, 0, 1});
    CHECK(m.sample == -1);
}

static void a_nan_is_never_the_minimum() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Coef c(3, 1);
    c.stay(0, 0, 0, 0), c.stay(1, 1, 0, 0), c.stay(2, 3, 0, 0);
    c.at(0, 0, 0)[2] = nan;  // every position of agent 0 is NaN, and so are its two ratios
    R::Result r = run(c, {0, 1}, 1.0, {0.2, 0.2, 0.2}, 2.0, 0.5);
    CHECK(r.samples == 2 && r.min_safety_ratio == 5.0 && r.min_sample == 0 && r.min_qi == 1 && r.min_qj == 2);
    CHECK(std::isnan(r.total_flight_distance));  // (the distance does say that a number is missing)
    R::Minimum m = R::Minimum{4.0, 7, 0, 1};
    R::take(&m, R::Minimum{nan, 0, 0, 1});
    CHECK(m.ratio == 4.0 && m.sample == 7);
    Coef d(2, 1);
    d.stay(0, nan, 0, 0), d.stay(1, 1, 0, 0);
    r = run(d, {0, 1}, 1.0, {0.2, 0.2}, 2.0, 0.5);
    CHECK(r.min_safety_ratio == 1e9 && r.min_sample == -1 && r.min_qi == -1 && r.min_qj == -1);
}

static void more_samples_than_the_limit_are_not_evaluated() {
    CHECK(RBP_REPORT_MAX_SAMPLES == 1048576);
    CHECK(R::sample_count(1048576.0, 1.0) == 1048576);
    CHECK(R::sample_count(1048577.0, 1.0) == -1);
    CHECK(R::sample_count(1e300, 1e-300) == -1);  // the quotient overflows
    CHECK(R::sample_count(1.0, 0.0) == -1);       // (entries refuse dt <= 0; the rule itself stays bounded)
    Coef c(2, 1);
    c.stay(0, 0, 0, 0), c.stay(1, 1, 0, 0);
    const R::Result r = run(c, {0, 2000.0}, 1.0, {0.2, 0.2}, 2.0, 1e-3);  // 2e6 samples
    CHECK(r.samples == -1 && r.end_time == 2000.0);
    CHECK(r.min_safety_ratio == 1e9 && r.total_flight_distance == 0.0 && r.min_sample == -1 && r.min_qi == -1 && r.min_qj == -1);
}

static void the_time_scale_multiplies_the_times_as_the_download_does() {
    const double ts = 1.1;
    CHECK(R::scaled_time(0.7, 1.0) == 0.7 && R::scaled_time(0.7, ts) == 0.7 * 1.1 && R::scaled_time(3.0, 1.4641) == 3.0 * 1.4641);
    const std::vector<double> T = {0, 1, 2};
    Coef c(2, 2);
    c.line(0, 0, 0, 1.0, 0.0), c.line(0, 0, 1, 1.0, 100.0);
    c.stay(1, 0.0, 1000.0, 0.0);
    const R::Result r = run(c, T, ts, {0.5, 0.5}, 2.0, 0.1);
    CHECK(r.end_time == 2 * 1.1 && r.samples == 22);  // 2.2 / 0.1 = 22.000000000000004
    // the second segment begins at 1 * 1.1: sample 11 (11 * 0.1 == 1.1 in doubles) is still in the first, sample 12 in the second
    CHECK(11 * 0.1 == 1.1);
    CHECK(R::segments_before(T.data(), 2, ts, R::sample_time(11, 0.1), 0) == 1);
    CHECK(R::segments_before(T.data(), 2, ts, R::sample_time(12, 0.1), 0) == 2);
    CHECK(R::segment_time(T.data(), ts, R::sample_time(12, 0.1), 2) == 12 * 0.1 - 1.1);
    CHECK(R::segments_before(T.data(), 2, 1.0, R::sample_time(11, 0.1), 0) == 2);  // (without the scale it would be)
    // ... which the distance sees: 11 steps of about 0.1, the jump of 100 + 0.1 - 1.1 between samples 11 and 12, 9 steps of about 0.1
    CHECK(std::fabs(r.total_flight_distance - (1.1 + 99.0 + 0.9)) < 1e-12);
    CHECK(r.min_safety_ratio == 1000.0 && r.min_sample == 0 && r.min_qi == 0 && r.min_qj == 1);  // agent 0 starts right below agent 1
}

int main() {
    horner_and_elements();
    a_sample_on_a_knot_belongs_to_the_earlier_segment();
    three_tenths_lie_just_past_0_3();
    samples_are_a_floor_and_few_samples_give_no_distance();
    one_agent_has_no_ratio_but_a_distance();
    the_distance_is_a_sum_per_agent_then_over_agents();
    equal_ratios_report_the_smaller_index();
    a_nan_is_never_the_minimum();
    more_samples_than_the_limit_are_not_evaluated();
    the_time_scale_multiplies_the_times_as_the_download_does();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("report rules ok\n");
    return 0;
}
