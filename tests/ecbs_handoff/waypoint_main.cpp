// The per-element rules of the plan writer (common/ecbs_rules.h: plan_time, plan_waypoint) as g++ compiles them, checked against
// hand-computed values and against write_plan, the loop over them that the host search returns (tests/test_ecbs_handoff_rules.py builds
// this program with the sanitizers and runs it).  kernels/handoff.hip evaluates the same two functions, one element per lane.
#include <cstdio>
#include <cstring>
#include <vector>

#include "common/ecbs_rules.h"
#include "rbp.h"

namespace R = ecbs_rules;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Cell {
    int cx, cy, cz;
    int x() const { return cx; }
    int y() const { return cy; }
    int z() const { return cz; }
};
typedef std::vector<std::vector<Cell>> Paths;

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// every element of write_plan's output is the rule's value, and nothing beyond index M is touched
static void rule_is_write_plan(const Paths& sol, const std::vector<double>& start, const std::vector<double>& goal, const double gmin[3],
                               const double gres[3], double time_step, size_t extra) {
    const int N = (int)sol.size();
    auto len_of = [&](int a) { return (int)sol[a].size(); };
    auto cell_at = [&](int a, int p) { return sol[a][p]; };
    int32_t makespan = -1, sum_cost = -1;
    const int M = R::plan_segments(N, len_of, &makespan, &sum_cost);
    const size_t stride = (size_t)M + 1 + extra;
    std::vector<double> T(stride, -7.0);
    std::vector<float> tr((size_t)N * stride * 3, -7.0f);
    R::write_plan(M, N, len_of, cell_at, start.data(), goal.data(), gmin, gres, time_step, stride, T.data(), tr.data());
    for (size_t i = 0; i < stride; ++i) CHECK(same_bits(T[i], (int)i <= M ? R::plan_time((int)i, time_step) : -7.0));
    for (int a = 0; a < N; ++a)
        for (size_t n = 0; n < stride; ++n)
            for (int axis = 0; axis < 3; ++axis) {
                const float want = (int)n <= M ? R::plan_waypoint((int)n, axis, len_of(a), [&](int p) { return sol[a][p]; }, &start[9 * a], &goal[9 * a], gmin, gres)
                                               : -7.0f;
                CHECK(same_bits(tr[((size_t)a * stride + n) * 3 + axis], want));
            }
}

static void hand_computed() {
    const double gmin[3] = {-5.0, -5.0, 1.0}, gres[3] = {0.5, 0.5, 1.0};
    // times: 0.5 and 1
    CHECK(R::plan_time(0, 0.5) == 0.0 && R::plan_time(3, 0.5) == 1.5 && R::plan_time(7, 1.0) == 7.0 && R::plan_time(4, 0.25) == 1.0);
    // one agent, a path of three cells
    const std::vector<Cell> path = {{10, 10, 0}, {11, 10, 0}, {12, 10, 1}};
    double start[9] = {0.01, 0.02, 1.03, 9, 9, 9, 9, 9, 9}, goal[9] = {1.01, 0.02, 1.97, 8, 8, 8, 8, 8, 8};
    auto cell = [&](int p) { return path[p]; };
    auto wp = [&](int n, int axis) { return R::plan_waypoint(n, axis, 3, cell, start, goal, gmin, gres); };
    CHECK(wp(0, 0) == 0.01f && wp(0, 1) == 0.02f && wp(0, 2) == 1.03f);           // the start state's position, not its velocity
    CHECK(wp(1, 0) == 0.0f && wp(1, 1) == 0.0f && wp(1, 2) == 1.0f);               // cell 0
    CHECK(wp(2, 0) == 0.5f && wp(3, 0) == 1.0f && wp(3, 2) == 2.0f);               // cells 1, 2
    for (int n = 4; n <= 9; ++n) CHECK(wp(n, 0) == 1.01f && wp(n, 1) == 0.02f && wp(n, 2) == 1.97f);  // the goal from len + 1 on
    // a path of its start cell only (len 1): start, the cell, then the goal
    const std::vector<Cell> one = {{3, 4, 1}};
    auto wp1 = [&](int n, int axis) { return R::plan_waypoint(n, axis, 1, [&](int p) { return one[p]; }, start, goal, gmin, gres); };
    CHECK(wp1(0, 1) == 0.02f && wp1(1, 0) == -3.5f && wp1(1, 1) == -3.0f && wp1(1, 2) == 2.0f && wp1(2, 0) == 1.01f && wp1(3, 2) == 1.97f);

    // a product that is not exact in double: cell 7 on a lattice of step 0.3 from -4.8 (Param's defaults: grid/xy_res 0.3).
    // The exact product of 7 and the double 0.3 is 2.09999999999999992228...; it rounds to the double 2.1 (0x4000CCCCCCCCCCCD), and
    // 2.1 + -4.8 rounds to -2.6999999999999997 (0xC005999999999999), which is NOT the double nearest -2.7 (0xC00599999999999A): the rule's
    // result is the former, then its float.
    const double g3min[3] = {-4.8, -4.8, 0.6}, g3res[3] = {0.3, 0.3, 0.6};
    const std::vector<Cell> seven = {{7, 7, 1}};
    const double prod = 7 * 0.3, sum = prod + -4.8;
    unsigned long long bits;
    std::memcpy(&bits, &prod, 8);
    CHECK(bits == 0x4000CCCCCCCCCCCDull);
    std::memcpy(&bits, &sum, 8);
    CHECK(bits == 0xC005999999999999ull && sum != -2.7);
    const float got = R::plan_waypoint(1, 0, 1, [&](int p) { return seven[p]; }, start, goal, g3min, g3res);
    CHECK(same_bits(got, (float)sum));
    CHECK(same_bits(R::plan_waypoint(1, 2, 1, [&](int p) { return seven[p]; }, start, goal, g3min, g3res), (float)(1 * 0.6 + 0.6)));
}

static void against_write_plan() {
    const double gmin[3] = {-5.0, -5.0, 1.0}, gres[3] = {0.5, 0.5, 1.0};
    const double g3min[3] = {-4.8, -4.8, 0.6}, g3res[3] = {0.3, 0.3, 0.6};
    auto states = [](int N, double base) {
        std::vector<double> s((size_t)N * 9);
        for (size_t i = 0; i < s.size(); ++i) s[i] = base + 0.37 * (double)i;
        return s;
    };
    const Paths single = {{{1, 2, 0}, {2, 2, 0}, {2, 3, 0}, {2, 3, 1}}};                                   // N = 1
    const Paths ragged = {{{10, 10, 0}, {11, 10, 0}, {12, 10, 0}, {12, 11, 0}, {12, 12, 0}}, {{3, 4, 1}},   // makespan 4; len 1; shorter agents
                          {{7, 7, 1}, {7, 8, 1}}, {{0, 0, 0}, {0, 1, 0}, {0, 2, 0}}};
    for (const Paths* sol : {&single, &ragged})
        for (double time_step : {0.5, 1.0})
            for (size_t extra : {(size_t)0, (size_t)3, (size_t)60}) {   // stride M + 1, and strides above it (a batch's max_M + 1)
                const int N = (int)sol->size();
                rule_is_write_plan(*sol, states(N, -3.0), states(N, 1.5), gmin, gres, time_step, extra);
                rule_is_write_plan(*sol, states(N, -3.0), states(N, 1.5), g3min, g3res, time_step, extra);
            }
}

int main() {
    hand_computed();
    against_write_plan();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    else std::puts("ecbs handoff rules ok");
    return failures ? 1 : 0;
}
