// The rule of common/state_rules.h as g++ compiles it for rbp_dynamics_host (tests/test_state_rules.py builds this program over the header
// ALONE, with the sanitizers, and runs it).  Without an argument: hand-computed cases.  With `eval`: one mission is read from standard
// input (hexadecimal doubles, so nothing is lost on the way), states_sequential runs on it, and everything it returned is printed the same
// way -- for the exact restatement of tests/synth_states.py to judge.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "common/state_rules.h"

namespace R = report_rules;
namespace S = state_rules;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static unsigned long long lcg_state = 12345;
static double rnd() {  // uniform in [-1, 1), seeded: the same on every run
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(lcg_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

struct Plan {
    int N, M;
    std::vector<double> T, c, radius, max_vel, max_acc;
    Plan(int N_, int M_) : N(N_), M(M_), T(M_ + 1), c((size_t)N_ * 3 * 6 * M_, 0.0), radius(N_, 0.2), max_vel((size_t)3 * N_, 1.0), max_acc((size_t)3 * N_, 1.0) {
        for (int m = 0; m <= M; ++m) T[m] = m;
    }
    double* at(int qi, int k, int m) { return &c[((size_t)qi * 3 + k) * 6 * M + 6 * m]; }
    void line(int qi, int k, int m, double slope, double offset) { at(qi, k, m)[4] = slope, at(qi, k, m)[5] = offset; }
    void stay(int qi, double x, double y, double z) {
        for (int m = 0; m < M; ++m) line(qi, 0, m, 0, x), line(qi, 1, m, 0, y), line(qi, 2, m, 0, z);
    }
    void randomise() {
        for (double& v : c) v = rnd();
    }
    S::Result run(double dt, double* states, double* curves, int S_stride, double ts = 1.0, double downwash = 2.0) {
        std::vector<double> scratch((size_t)3 * N);
        return S::states_sequential(N, M, T.data(), ts, c.data(), radius.data(), max_vel.data(), max_acc.data(), downwash, dt, states, curves, S_stride,
                                    scratch.data());
    }
};

static void derivatives_by_horner() {
    const double c[6] = {1, 2, 3, 4, 5, 6};
    CHECK(S::velocity(c, 2.0) == 201.0);      // 5*16 + 8*8 + 9*4 + 8*2 + 5
    CHECK(S::acceleration(c, 2.0) == 300.0);  // 20*8 + 24*4 + 18*2 + 8
    CHECK(S::velocity(c, 0.0) == 5.0 && S::acceleration(c, 0.0) == 8.0);
    // every product and sum rounds on its own, the integer factor on the coefficient first: said again, operation by operation
    for (int n = 0; n < 200; ++n) {
        double d[6];
        for (double& v : d) v = rnd() * 3;
        const double t = rnd() * 2;
        volatile double v = 5.0 * d[0], p, q;
        for (int i = 1; i < 5; ++i) p = v * t, q = (double)(5 - i) * d[i], v = p + q;
        CHECK(same_bits(S::velocity(d, t), v));
        volatile double a = 20.0 * d[0];
        const double f[4] = {20, 12, 6, 2};
        for (int i = 1; i < 4; ++i) p = a * t, q = f[i] * d[i], a = p + q;
        CHECK(same_bits(S::acceleration(d, t), a));
    }
}

static void position_rows_are_the_reports_bits() {
    Plan pl(3, 4);
    pl.randomise();
    pl.T = {0, 0.5, 2.2, 3.0, 4.7};
    for (int n = 0; n < 300; ++n) {
        const double t = (rnd() + 1.0) * 2.35, ts = n % 2 ? 1.0 : 1.1;
        const int before = R::segments_before(pl.T.data(), 4, ts, t, 0), qi = n % 3;
        double s[9], p[3];
        S::agent_state(pl.c.data(), 4, pl.T.data(), ts, qi, t, before, s);
        R::agent_position(pl.c.data(), 4, pl.T.data(), ts, qi, t, before, p);
        for (int k = 0; k < 3; ++k) CHECK(same_bits(s[k], p[k]));
    }
}

static void a_sample_on_a_knot_belongs_to_the_earlier_segment() {
    Plan pl(2, 2);
    pl.randomise();  // (random coefficients: velocity and acceleration differ across the knot)
    CHECK(R::sample_time(10, 0.1) == 1.0);
    double s[9], e[9], l[9];
    const int before = R::segments_before(pl.T.data(), 2, 1.0, 1.0, 0);
    CHECK(before == 1);
    for (int qi = 0; qi < 2; ++qi) {
        S::agent_state(pl.c.data(), 2, pl.T.data(), 1.0, qi, 1.0, before, s);
        for (int k = 0; k < 3; ++k) {
            S::axis_state(pl.at(qi, k, 0), 1.0, &e[k], &e[3 + k], &e[6 + k]);  // the earlier segment at its end
            S::axis_state(pl.at(qi, k, 1), 0.0, &l[k], &l[3 + k], &l[6 + k]);  // the later one at its start
        }
        for (int r = 0; r < 9; ++r) CHECK(same_bits(s[r], e[r]) && s[r] != l[r]);
    }
    // ... and the whole loop stores exactly that at sample 10, the later segment from sample 11 on
    std::vector<double> st((size_t)2 * 9 * 20, -7.0);
    const S::Result r = pl.run(0.1, st.data(), nullptr, 20);
    CHECK(r.samples == 20 && r.stored == 1);
    for (int row = 0; row < 9; ++row) CHECK(same_bits(st[((size_t)1 * 9 + row) * 20 + 10], s[row]));
    double n11[3];
    S::axis_state(pl.at(1, 0, 1), R::sample_time(11, 0.1) - 1.0, &n11[0], &n11[1], &n11[2]);
    CHECK(same_bits(st[((size_t)1 * 9 + 3) * 20 + 11], n11[1]) && same_bits(st[((size_t)1 * 9 + 6) * 20 + 11], n11[2]));
}

static void peaks_report_the_first_among_equals() {
    const S::Peak cand[4] = {{2.5, 1, 1, 3, 1, 2, 0}, {2.5, 1, 1, 3, 0, 2, 0}, {2.5, -1, 1, 1, 1, 2, 0}, {2.0, 1, 1, 0, 0, 1, 0}};
    for (int rot = 0; rot < 4; ++rot) {
        S::Peak m = S::no_peak();
        for (int i = 0; i < 4; ++i) S::take(&m, cand[(i + rot) % 4]);
        CHECK(m.ratio == 2.5 && m.sample == 1 && m.agent == 1 && m.axis == 2 && m.value == -1);
    }
    const S::Peak axes[2] = {{2.5, 1, 1, 1, 1, 2, 0}, {2.5, 1, 1, 1, 1, 0, 0}};
    for (int rot = 0; rot < 2; ++rot) {
        S::Peak m = S::no_peak();
        for (int i = 0; i < 2; ++i) S::take(&m, axes[(i + rot) % 2]);
        CHECK(m.axis == 0);
    }
    // the whole loop: agents 0 and 1 move alike along y and z from the first sample on -- the peak is (0, 0, 1)
    Plan pl(2, 2);
    for (int m = 0; m < 2; ++m) pl.line(0, 1, m, 0.5, 0), pl.line(0, 2, m, -0.5, 0), pl.line(1, 1, m, 0.5, 3), pl.line(1, 2, m, -0.5, 3);
    const S::Result r = pl.run(0.25, nullptr, nullptr, 0);
    CHECK(r.samples == 8 && r.stored == 0);
    CHECK(r.vel.ratio == 0.5 && r.vel.value == 0.5 && r.vel.limit == 1.0 && r.vel.sample == 0 && r.vel.agent == 0 && r.vel.axis == 1);
    CHECK(r.acc.ratio == 0.0 && r.acc.sample == -1 && r.acc.agent == -1 && r.acc.axis == -1 && r.acc.value == 0.0 && r.acc.limit == 0.0);  // no acceleration anywhere
    // a tighter limit on a later axis wins by ratio, and the raw value keeps its sign
    pl.max_vel[3 * 1 + 2] = 0.25;
    const S::Result q = pl.run(0.25, nullptr, nullptr, 0);
    CHECK(q.vel.ratio == 2.0 && q.vel.value == -0.5 && q.vel.limit == 0.25 && q.vel.sample == 0 && q.vel.agent == 1 && q.vel.axis == 2);
}

static void zero_nan_and_negative_ratios_are_never_peaks() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    S::Peak m = S::no_peak();
    S::take(&m, S::Peak{0.0, 0, 1, 0, 0, 0, 0});
    CHECK(m.sample == -1);
    S::take(&m, S::Peak{nan, nan, 1, 0, 0, 0, 0});
    CHECK(m.sample == -1 && m.ratio == 0.0);
    S::take(&m, S::Peak{-2.0, 2, -1, 0, 0, 0, 0});  // (a negative limit)
    CHECK(m.sample == -1);
    S::take(&m, S::Peak{1.5, 3, 2, 4, 0, 0, 0});
    S::take(&m, S::Peak{nan, nan, 1, 0, 0, 0, 0});
    CHECK(m.ratio == 1.5 && m.sample == 4);
    S::take(&m, S::Peak{inf, 1, 0, 9, 0, 0, 0});  // (a limit of 0 does say that the plan breaks it)
    CHECK(m.ratio == inf && m.sample == 9);
    CHECK(S::limit_ratio(-3.0, 2.0) == 1.5 && S::limit_ratio(0.0, 2.0) == 0.0 && std::isnan(S::limit_ratio(nan, 2.0)));
    // a NaN coefficient of one agent: its candidates are skipped, the other agent's peak stands
    Plan pl(2, 1);
    pl.line(0, 0, 0, nan, 0), pl.line(1, 0, 0, 0.25, 3);
    const S::Result r = pl.run(0.5, nullptr, nullptr, 0);
    CHECK(r.samples == 2 && r.vel.ratio == 0.25 && r.vel.agent == 1 && r.vel.sample == 0 && r.vel.axis == 0);
}

static void curves_keep_the_smallest_and_the_largest_ratio_of_a_sample() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Plan pl(3, 1);
    pl.stay(0, 0, 0, 0), pl.stay(1, 1, 0, 0), pl.stay(2, 3, 0, 0);
    std::vector<double> cu(2 * 4, -7.0);
    S::Result r = pl.run(0.5, nullptr, cu.data(), 4);
    CHECK(r.samples == 2 && r.stored == 1);
    CHECK(cu[0] == 2.5 && cu[1] == 7.5 && cu[2] == 2.5 && cu[3] == 7.5);  // 1 / 0.4, 3 / 0.4 (and 2 / 0.4 between)
    CHECK(cu[4] == -7.0 && cu[5] == -7.0 && cu[6] == -7.0 && cu[7] == -7.0);  // beyond the samples: untouched
    pl.at(0, 0, 0)[2] = nan;  // every ratio of agent 0 is NaN: neither curve moves for them
    r = pl.run(0.5, nullptr, cu.data(), 4);
    CHECK(cu[0] == 5.0 && cu[1] == 5.0);
    S::Curve c = S::no_curve();
    S::curve_take(&c, nan);
    CHECK(c.min_ratio == 1e9 && c.max_ratio == 0.0);
    S::curve_take(&c, 2e9);  // (above 1e9: the largest, never the smallest)
    CHECK(c.min_ratio == 1e9 && c.max_ratio == 2e9);
    Plan one(1, 1);
    one.stay(0, 1, 1, 1);
    r = one.run(0.5, nullptr, cu.data(), 4);
    CHECK(cu[0] == 1e9 && cu[1] == 0.0 && cu[2] == 1e9 && cu[3] == 0.0);  // no pair
}

static void a_row_too_short_stores_nothing() {
    Plan pl(2, 1);
    pl.randomise();
    std::vector<double> st((size_t)2 * 9 * 9, -7.0), cu(2 * 9, -7.0);
    const S::Result full = pl.run(0.1, nullptr, nullptr, 0);
    S::Result r = pl.run(0.1, st.data(), cu.data(), 9);  // ten samples
    CHECK(r.samples == 10 && r.stored == 0);
    for (double v : st) CHECK(v == -7.0);
    for (double v : cu) CHECK(v == -7.0);
    CHECK(same_bits(r.vel.ratio, full.vel.ratio) && r.vel.sample == full.vel.sample && same_bits(r.acc.ratio, full.acc.ratio) && r.acc.ratio > 0);
    std::vector<double> st11((size_t)2 * 9 * 11, -7.0);
    r = pl.run(0.1, st11.data(), nullptr, 11);
    CHECK(r.stored == 1);
    for (int row = 0; row < 18; ++row) CHECK(st11[(size_t)row * 11 + 10] == -7.0 && st11[(size_t)row * 11 + 9] != -7.0);
    pl.T[1] = 2000.0;  // 2e6 samples: more than are evaluated
    r = pl.run(1e-3, st.data(), cu.data(), 9);
    CHECK(r.samples == -1 && r.stored == 0 && r.end_time == 2000.0 && r.vel.sample == -1 && r.vel.ratio == 0.0 && r.acc.sample == -1);
    pl.T[1] = 0.05;  // no sample: stored, for there is nothing that does not fit
    r = pl.run(0.1, st.data(), nullptr, 9);
    CHECK(r.samples == 0 && r.stored == 1 && r.vel.sample == -1);
}

static bool read(std::vector<double>& v) {
    for (double& x : v)
        if (std::scanf("%la", &x) != 1) return false;
    return true;
}
static void print(const char* name, const double* v, size_t n) {
    std::printf("%s", name);
    for (size_t i = 0; i < n; ++i) std::printf(" %a", v[i]);
    std::printf("\n");
}

static int eval() {
    int N, M, S_stride;
    std::vector<double> head(3);  // dt, time scale, downwash
    if (std::scanf("%d %d %d", &N, &M, &S_stride) != 3 || N < 1 || M < 1 || S_stride < 1 || !read(head)) return 2;
    Plan pl(N, M);
    if (!read(pl.T) || !read(pl.c) || !read(pl.radius) || !read(pl.max_vel) || !read(pl.max_acc)) return 2;
    std::vector<double> st((size_t)N * 9 * S_stride, 0.0), cu((size_t)2 * S_stride, 0.0);
    const S::Result r = pl.run(head[0], st.data(), cu.data(), S_stride, head[1], head[2]);
    std::printf("samples %d stored %d\n", r.samples, r.stored);
    std::printf("vel %d %d %d %a %a %a\n", r.vel.sample, r.vel.agent, r.vel.axis, r.vel.ratio, r.vel.value, r.vel.limit);
    std::printf("acc %d %d %d %a %a %a\n", r.acc.sample, r.acc.agent, r.acc.axis, r.acc.ratio, r.acc.value, r.acc.limit);
    print("end_time", &r.end_time, 1);
    print("states", st.data(), st.size());
    print("curves", cu.data(), cu.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "eval") == 0) return eval();
    derivatives_by_horner();
    position_rows_are_the_reports_bits();
    a_sample_on_a_knot_belongs_to_the_earlier_segment();
    peaks_report_the_first_among_equals();
    zero_nan_and_negative_ratios_are_never_peaks();
    curves_keep_the_smallest_and_the_largest_ratio_of_a_sample();
    a_row_too_short_stores_nothing();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("state rules ok\n");
    return 0;
}
