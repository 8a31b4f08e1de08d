// The rule of common/swept_rules.h as g++ compiles it for rbp_swept_clearance_host, checked on hand-computed cases
// (tests/test_swept_rules.py builds this program over the header ALONE, with the sanitizers, and runs it).  Trajectories are constant or
// linear and the grids have cells of 0.5 m (rf = 2 exactly), so every expected key and reading can be worked out by hand.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "common/swept_rules.h"

namespace W = swept_rules;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static const double U = std::ldexp(1.0, -53);

struct Coef {
    int N, M;
    std::vector<double> c;
    Coef(int N_, int M_) : N(N_), M(M_), c((size_t)N_ * 3 * 6 * M_, 0.0) {}
    double* axis(int a, int k, int m) { return &c[((size_t)a * 3 + k) * 6 * M + 6 * m]; }
    void line(int a, int k, int m, double slope, double offset) { axis(a, k, m)[4] = slope, axis(a, k, m)[5] = offset; }
    void stay(int a, double x, double y, double z) {
        for (int m = 0; m < M; ++m) line(a, 0, m, 0, x), line(a, 1, m, 0, y), line(a, 2, m, 0, z);
    }
};
struct Grid {
    int32_t dim[3], key_min[3];
    double res;
    std::vector<float> d;
    Grid(int nx, int ny, int nz, int kx, int ky, int kz, float fill) : dim{nx, ny, nz}, key_min{kx, ky, kz}, res(0.5), d((size_t)nx * ny * nz, fill) {}
    float& at(int ix, int iy, int iz) { return d[((size_t)ix * dim[1] + iy) * dim[2] + iz]; }
};
static std::vector<double> unit_times(int M, double h = 1.0) {
    std::vector<double> T((size_t)M + 1);
    for (int m = 0; m <= M; ++m) T[m] = h * m;
    return T;
}
static W::Tally run(Coef& c, const std::vector<double>& T, const std::vector<double>& radius, Grid& g, int depth, double refine_below,
                    double* agents = nullptr) {
    return W::swept_sequential(c.N, c.M, T.data(), 1.0, c.c.data(), radius.data(), g.dim, g.key_min, g.res, g.d.data(), depth, refine_below, agents);
}
static W::Box box_of(Coef& c, const std::vector<double>& T, Grid& g, int a, int m, int depth, int p) {
    const W::Item it = W::item_of(c.c.data(), c.M, T.data(), 1.0, a, m);
    double b[18], lo[3], hi[3];
    for (int i = 0; i < 18; ++i) b[i] = it.b[i];
    separation_rules::piece_points(b, depth, p);
    for (int k = 0; k < 3; ++k) W::axis_interval(b + 6 * k, W::error_term(depth, it.A[k]), lo + k, hi + k);
    return W::box_keys(g.dim, g.key_min, 2.0, lo, hi);
}

static void an_agent_at_rest_in_one_cell() {
    Coef c(1, 1);
    c.stay(0, 1.2, 1.3, 0.7);  // keys floor(2.4), floor(2.6), floor(1.4) = 2, 2, 1
    Grid g(10, 6, 4, 0, 0, 0, 1.0f);
    g.at(2, 2, 1) = 0.75f;
    const std::vector<double> T = unit_times(1), radius = {0.25};
    const W::Item it = W::item_of(c.c.data(), 1, T.data(), 1.0, 0, 0);
    CHECK(it.A[0] == 1.2 && it.A[1] == 1.3 && it.A[2] == 0.7);
    for (int i = 0; i < 6; ++i) CHECK(it.b[i] == 1.2 && it.b[6 + i] == 1.3 && it.b[12 + i] == 0.7);
    CHECK(W::error_term(0, 1.2) == 20.0 * U * 1.2 && W::error_term(8, 1.2) == 60.0 * U * 1.2);
    const W::Box bx = box_of(c, T, g, 0, 0, 0, 0);
    CHECK(!bx.outside && !bx.over_budget && bx.i0[0] == 2 && bx.i0[1] == 2 && bx.i0[2] == 1 && bx.n[0] == 1 && bx.n[1] == 1 && bx.n[2] == 1);
    double agents[1] = {-7.0};
    W::Tally t = run(c, T, radius, g, 4, -2.0, agents);
    CHECK(t.lower.clearance == 0.5 && t.upper.clearance == 0.5 && t.lower.dist == 0.75 && t.upper.dist == 0.75);
    CHECK(t.lower.segment == 0 && t.lower.piece == 0 && t.lower.agent == 0 && t.lower.depth == 0 && t.upper.depth == 0);
    CHECK(t.uncertified == 0 && t.hitting == 0 && t.outside == 0 && t.over_budget == 0 && t.refined == 0 && agents[0] == 0.5);
    t = run(c, T, radius, g, 3, 1e9, agents);  // everything refined: eight equal pieces, the first is named
    CHECK(t.lower.clearance == 0.5 && t.upper.clearance == 0.5 && t.lower.piece == 0 && t.upper.piece == 0 && t.lower.depth == 3 && t.refined == 1);
    t = run(c, T, radius, g, 0, 1e9, agents);  // depth 0: refined, evaluated again on its one piece
    CHECK(t.lower.clearance == 0.5 && t.lower.depth == 0 && t.refined == 1 && agents[0] == 0.5);
    // refine_below exactly at the depth-0 lower clearance: the item stays; one double above: it goes
    CHECK(run(c, T, radius, g, 2, 0.5, nullptr).refined == 0 && run(c, T, radius, g, 2, std::nextafter(0.5, 1.0), nullptr).refined == 1);
    // a hit by the reference's test: d < radius - 1e-6
    const std::vector<double> fat = {0.75 + 2e-6}, touching = {0.75 + 5e-7};
    CHECK(run(c, T, fat, g, 0, -2.0).uncertified == 1 && run(c, T, fat, g, 0, -2.0).hitting == 1);
    CHECK(run(c, T, touching, g, 0, -2.0).uncertified == 0 && run(c, T, touching, g, 0, -2.0).hitting == 0);
}

static void a_straight_line_along_x() {
    Coef c(1, 1);
    c.line(0, 0, 0, 4.0, 0.25), c.line(0, 1, 0, 0.0, 1.3), c.line(0, 2, 0, 0.0, 0.7);  // x from 0.25 to 4.25: keys 0 .. 8
    Grid g(10, 6, 4, 0, 0, 0, 1.0f);
    for (int ix = 0; ix < 10; ++ix) g.at(ix, 2, 1) = 0.5f + 0.03125f * (float)ix;
    g.at(6, 2, 1) = 0.125f;  // the row's smallest, between the ends
    g.at(9, 2, 1) = 0.0f;    // beyond the line: never read
    g.at(6, 3, 1) = 0.0f;    // beside the line: never read
    const std::vector<double> T = unit_times(1), radius = {0.25};
    const W::Item it = W::item_of(c.c.data(), 1, T.data(), 1.0, 0, 0);
    CHECK(it.b[0] == 0.25 && it.b[5] == 4.25 && it.A[0] == 4.25);
    W::Box bx = box_of(c, T, g, 0, 0, 0, 0);
    CHECK(!bx.outside && bx.i0[0] == 0 && bx.n[0] == 9 && bx.i0[1] == 2 && bx.n[1] == 1 && bx.i0[2] == 1 && bx.n[2] == 1);
    W::Tally t = run(c, T, radius, g, 0, -2.0);
    CHECK(t.lower.dist == 0.125 && t.lower.clearance == -0.125 && t.upper.dist == 0.5 && t.upper.clearance == 0.25);
    CHECK(t.uncertified == 1 && t.hitting == 0 && t.refined == 0);
    // both halves: the point in the middle is 2.25 (key 4), give or take a rounding that does not reach a face
    bx = box_of(c, T, g, 0, 0, 1, 0);
    CHECK(!bx.outside && bx.i0[0] == 0 && bx.n[0] == 5 && bx.n[1] == 1 && bx.n[2] == 1);
    bx = box_of(c, T, g, 0, 0, 1, 1);
    CHECK(!bx.outside && bx.i0[0] == 4 && bx.n[0] == 5 && bx.n[1] == 1 && bx.n[2] == 1);
    double agents[1];
    t = run(c, T, radius, g, 1, 1e9, agents);
    CHECK(t.lower.dist == 0.125 && t.lower.piece == 1 && t.lower.depth == 1 && t.refined == 1 && agents[0] == -0.125);
    CHECK(t.upper.dist == 0.5 && t.upper.piece == 0);  // the ends read cells 0 | 4 and 4 | 8: 0.5 is the smallest
    // depth 3: eight pieces of 0.5 m, the ends at 0.25 + 0.5 p: piece 5 spans keys 5 .. 6 and piece 6 keys 6 .. 7; the first is named
    t = run(c, T, radius, g, 3, 1e9);
    CHECK(t.lower.dist == 0.125 && t.lower.piece == 5 && t.upper.dist == 0.125 && t.upper.piece == 5 && t.hitting == 1 && t.uncertified == 1);
}

static void a_coordinate_on_a_cell_face() {
    Grid g(10, 6, 4, 0, 0, 0, 1.0f);
    g.at(2, 2, 1) = 0.25f, g.at(3, 2, 1) = 0.75f;
    const std::vector<double> T = unit_times(1), radius = {0.25};
    // x = 1.5 exactly: key 3.  lo = 1.5 - e is below 1.5 as a double and rounds to 1.5f as a float, so the box is cell 3 alone
    Coef c(1, 1);
    c.stay(0, 1.5, 1.3, 0.7);
    CHECK(1.5 - W::error_term(0, 1.5) < 1.5 && (float)(1.5 - W::error_term(0, 1.5)) == 1.5f);
    W::Box bx = box_of(c, T, g, 0, 0, 0, 0);
    CHECK(!bx.outside && bx.i0[0] == 3 && bx.n[0] == 1);
    CHECK(run(c, T, radius, g, 0, -2.0).lower.dist == 0.75 && run(c, T, radius, g, 0, -2.0).upper.dist == 0.75);
    // x a double below the face that the float cast puts on it: the lookup reads cell 3, and so does the box
    c.stay(0, 1.5 - 1e-9, 1.3, 0.7);
    bx = box_of(c, T, g, 0, 0, 0, 0);
    CHECK(bx.i0[0] == 3 && bx.n[0] == 1 && run(c, T, radius, g, 0, -2.0).upper.dist == 0.75);
    // x one float below the face: cell 2
    c.stay(0, (double)std::nextafter(1.5f, 0.0f), 1.3, 0.7);
    bx = box_of(c, T, g, 0, 0, 0, 0);
    CHECK(bx.i0[0] == 2 && bx.n[0] == 1 && run(c, T, radius, g, 0, -2.0).lower.dist == 0.25);
    // a negative key_min: x = -0.75 is key -2, the second cell of a grid that starts at key -3
    Grid n(10, 6, 4, -3, 0, 0, 1.0f);
    n.at(1, 2, 1) = 0.5f;
    c.stay(0, -0.75, 1.3, 0.7);
    bx = box_of(c, T, n, 0, 0, 0, 0);
    CHECK(!bx.outside && bx.i0[0] == 1 && bx.n[0] == 1 && run(c, T, radius, n, 0, -2.0).lower.dist == 0.5);
}

static void outside_on_each_side() {
    Grid g(10, 6, 4, 0, 0, 0, 1.0f);  // x in [0, 5), y in [0, 3), z in [0, 2)
    const std::vector<double> T = unit_times(1), radius = {0.25};
    const double at[6][3] = {{-0.1, 1.3, 0.7}, {5.0, 1.3, 0.7}, {1.2, -0.1, 0.7}, {1.2, 3.0, 0.7}, {1.2, 1.3, -0.1}, {1.2, 1.3, 2.0}};
    for (int s = 0; s < 6; ++s) {
        Coef c(1, 1);
        c.stay(0, at[s][0], at[s][1], at[s][2]);
        CHECK(box_of(c, T, g, 0, 0, 0, 0).outside);
        double agents[1];
        const W::Tally t = run(c, T, radius, g, 2, -2.0, agents);  // (outside always goes to `depth`)
        CHECK(t.outside == 1 && t.refined == 1 && t.uncertified == 1 && t.hitting == 1 && t.over_budget == 0);
        CHECK(t.lower.dist == -1.0 && t.lower.clearance == -1.25 && t.upper.dist == -1.0 && t.lower.depth == 2 && t.lower.piece == 0 && agents[0] == -1.25);
    }
    // a line that leaves through the far x side only in its second half
    Coef c(1, 1);
    c.line(0, 0, 0, 4.0, 2.25), c.line(0, 1, 0, 0.0, 1.3), c.line(0, 2, 0, 0.0, 0.7);  // x from 2.25 to 6.25
    CHECK(box_of(c, T, g, 0, 0, 0, 0).outside && !box_of(c, T, g, 0, 0, 1, 0).outside && box_of(c, T, g, 0, 0, 1, 1).outside);
    const W::Tally t = run(c, T, radius, g, 1, -2.0);
    CHECK(t.outside == 1 && t.lower.piece == 1 && t.lower.dist == -1.0 && t.upper.piece == 1 && t.upper.dist == -1.0);
}

static void nan_and_infinite_coefficients() {
    Grid g(10, 6, 4, 0, 0, 0, 1.0f);
    const std::vector<double> T = unit_times(1), radius = {0.25};
    const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), INFINITY, -INFINITY};
    for (double v : bad)
        for (int k = 0; k < 3; ++k)
            for (int power = 0; power < 6; power += 5) {
                Coef c(1, 1);
                c.stay(0, 1.2, 1.3, 0.7);
                c.axis(0, k, 0)[power] = v;
                CHECK(box_of(c, T, g, 0, 0, 0, 0).outside && box_of(c, T, g, 0, 0, 3, 5).outside);
                const W::Tally t = run(c, T, radius, g, 3, 0.1);
                CHECK(t.outside == 1 && t.refined == 1 && t.uncertified == 1 && t.hitting == 1 && t.lower.dist == -1.0 && t.lower.clearance == -1.25);
            }
    // a NaN cell is never taken, and a NaN radius is no minimum and no hit
    Coef c(1, 1);
    c.line(0, 0, 0, 1.0, 0.25), c.line(0, 1, 0, 0.0, 1.3), c.line(0, 2, 0, 0.0, 0.7);  // keys 0 .. 2
    g.at(1, 2, 1) = std::numeric_limits<float>::quiet_NaN(), g.at(2, 2, 1) = 0.5f;
    W::Tally t = run(c, T, radius, g, 0, -2.0);
    CHECK(t.lower.dist == 0.5 && t.upper.dist == 0.5 && t.outside == 0);
    const std::vector<double> nan_radius = {std::numeric_limits<double>::quiet_NaN()};
    double agents[1];
    t = run(c, T, nan_radius, g, 2, 0.1, agents);
    CHECK(t.lower.segment == -1 && t.upper.segment == -1 && t.lower.clearance == 1e9 && t.uncertified == 0 && t.hitting == 0 && t.refined == 1 && agents[0] == 1e9);
}

static void an_over_budget_box() {
    Grid g(20, 20, 20, 0, 0, 0, 1.0f);
    g.at(3, 3, 3) = 0.25f;
    Coef c(1, 1);
    for (int k = 0; k < 3; ++k) c.line(0, k, 0, 9.0, 0.25);  // the diagonal from 0.25 to 9.25: keys 0 .. 18, 19^3 = 6859 cells
    const std::vector<double> T = unit_times(1), radius = {0.25};
    W::Box bx = box_of(c, T, g, 0, 0, 0, 0);
    CHECK(!bx.outside && bx.over_budget && bx.n[0] == 19 && bx.n[1] == 19 && bx.n[2] == 19);
    W::Tally t = run(c, T, radius, g, 0, -2.0);  // refined, but depth 0 is all there is
    CHECK(t.over_budget == 1 && t.outside == 0 && t.refined == 1 && t.uncertified == 1 && t.lower.dist == -1.0 && t.upper.dist == 1.0 && t.hitting == 0);
    bx = box_of(c, T, g, 0, 0, 1, 0);  // 0.25 .. 4.75: keys 0 .. 9, 1000 cells
    CHECK(!bx.outside && !bx.over_budget && bx.n[0] == 10);
    t = run(c, T, radius, g, 1, -2.0);  // over budget at depth 0 always goes to `depth`
    CHECK(t.over_budget == 0 && t.refined == 1 && t.lower.dist == 0.25 && t.lower.piece == 0 && t.lower.depth == 1 && t.uncertified == 0);
    // exactly at the budget: 16 x 16 x 16
    Coef d(1, 1);
    for (int k = 0; k < 3; ++k) d.line(0, k, 0, 7.5, 0.25);  // keys 0 .. 15
    bx = box_of(d, T, g, 0, 0, 0, 0);
    CHECK(!bx.over_budget && bx.n[0] == 16 && bx.n[1] == 16 && bx.n[2] == 16);
    CHECK(run(d, T, radius, g, 0, -2.0).lower.dist == 0.25 && run(d, T, radius, g, 0, -2.0).over_budget == 0);
}

static void the_order_on_ties() {
    // two agents at rest in cells of equal value, two segments: every piece ties; (segment, piece, agent) decides
    Grid g(10, 6, 4, 0, 0, 0, 1.0f);
    Coef c(2, 2);
    c.stay(0, 1.2, 1.3, 0.7), c.stay(1, 3.2, 1.3, 0.7);
    const std::vector<double> T = unit_times(2), radius = {0.25, 0.25};
    W::Tally t = run(c, T, radius, g, 2, 1e9);
    CHECK(t.lower.clearance == 0.75 && t.lower.segment == 0 && t.lower.piece == 0 && t.lower.agent == 0 && t.upper.segment == 0 && t.upper.agent == 0);
    g.at(6, 2, 1) = 0.5f;  // agent 1 alone is closer: it is named, in its first segment and piece
    t = run(c, T, radius, g, 2, 1e9);
    CHECK(t.lower.clearance == 0.25 && t.lower.segment == 0 && t.lower.piece == 0 && t.lower.agent == 1);
    // candidates in every order of arrival
    std::vector<W::Minimum> cand = {{0.5, 0.75, 1, 0, 0, 2}, {0.5, 0.75, 0, 3, 1, 2}, {0.5, 0.75, 0, 2, 5, 2}, {0.5, 0.75, 0, 2, 4, 2}, {0.75, 1.0, 0, 0, 0, 2},
                                    {std::numeric_limits<double>::quiet_NaN(), 0.0, 0, 0, 0, 0}, {1e9, 0.0, 0, 0, 0, 0}};
    std::vector<int> order = {0, 1, 2, 3, 4, 5, 6};
    do {
        W::Minimum m = W::no_minimum();
        for (int i : order) W::take(&m, cand[(size_t)i]);
        CHECK(m.clearance == 0.5 && m.segment == 0 && m.piece == 2 && m.agent == 4);
    } while (std::next_permutation(order.begin(), order.end()));
    W::Minimum none = W::no_minimum();
    W::take(&none, cand[5]), W::take(&none, cand[6]);
    CHECK(none.clearance == 1e9 && none.segment == -1 && none.piece == -1 && none.agent == -1 && none.depth == -1);
}

static void merge_in_both_orders() {
    W::Tally a = W::empty_tally(), b = W::empty_tally();
    a.lower = W::Minimum{0.5, 0.75, 1, 0, 0, 2}, a.upper = W::Minimum{0.75, 1.0, 0, 1, 3, 2}, a.uncertified = 1, a.hitting = 2, a.outside = 3, a.over_budget = 4, a.refined = 5;
    b.lower = W::Minimum{0.5, 0.75, 0, 7, 9, 2}, b.upper = W::Minimum{0.875, 1.0, 0, 0, 0, 0}, b.uncertified = 10, b.hitting = 20, b.outside = 30, b.over_budget = 40, b.refined = 50;
    W::Tally ab = a, ba = b;
    W::merge(&ab, b), W::merge(&ba, a);
    const W::Tally* both[2] = {&ab, &ba};
    for (const W::Tally* t : both) {
        CHECK(t->lower.segment == 0 && t->lower.piece == 7 && t->lower.agent == 9 && t->upper.clearance == 0.75 && t->upper.agent == 3);
        CHECK(t->uncertified == 11 && t->hitting == 22 && t->outside == 33 && t->over_budget == 44 && t->refined == 55);
    }
    W::Tally e = W::empty_tally();
    W::merge(&e, W::empty_tally());
    CHECK(e.lower.clearance == 1e9 && e.lower.segment == -1 && e.refined == 0);
    // a mission splits into its agents: the tallies of the parts merge to the whole's, in both orders
    Grid g(10, 6, 4, 0, 0, 0, 1.0f);
    g.at(6, 2, 1) = 0.5f;
    Coef c(2, 2), c0(1, 2), c1(1, 2);
    c.stay(0, 1.2, 1.3, 0.7), c.stay(1, 3.2, 1.3, 0.7), c0.stay(0, 1.2, 1.3, 0.7), c1.stay(0, 3.2, 1.3, 0.7);
    const std::vector<double> T = unit_times(2), radius = {0.25, 0.25};
    const W::Tally whole = run(c, T, radius, g, 1, 0.6);
    W::Tally p0 = run(c0, T, radius, g, 1, 0.6), p1 = run(c1, T, radius, g, 1, 0.6);
    p1.lower.agent = 1, p1.upper.agent = 1;
    W::Tally m01 = p0, m10 = p1;
    W::merge(&m01, p1), W::merge(&m10, p0);
    const W::Tally* parts[2] = {&m01, &m10};
    for (const W::Tally* t : parts) {
        CHECK(t->lower.clearance == whole.lower.clearance && t->lower.agent == whole.lower.agent && t->lower.depth == whole.lower.depth);
        CHECK(t->upper.clearance == whole.upper.clearance && t->upper.agent == whole.upper.agent && t->refined == whole.refined && whole.refined == 2);
    }
}

int main() {
    an_agent_at_rest_in_one_cell();
    a_straight_line_along_x();
    a_coordinate_on_a_cell_face();
    outside_on_each_side();
    nan_and_infinite_coefficients();
    an_over_budget_box();
    the_order_on_ties();
    merge_in_both_orders();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("swept rules ok\n");
    return 0;
}
