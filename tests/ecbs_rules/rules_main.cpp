// The rules of common/ecbs_rules.h as g++ compiles them for the host search, checked on hand-computed cases (tests/test_ecbs_rules.py builds
// this program with the sanitizers and runs it).  The lattice is that of Param.test_sweep(): world (-5, -5, 0.3) .. (5, 5, 2.5), grid 0.5 / 1.0.
#include <cmath>
#include <cstdio>
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
    bool operator==(const Cell& o) const { return cx == o.cx && cy == o.cy && cz == o.cz; }
};

static rbp_param sweep_param() {
    rbp_param p = rbp_param();
    p.world_min[0] = -5, p.world_min[1] = -5, p.world_min[2] = 0.3;
    p.world_max[0] = 5, p.world_max[1] = 5, p.world_max[2] = 2.5;
    p.grid_xy_res = 0.5, p.grid_z_res = 1.0, p.time_step = 1.0;
    return p;
}

static void lattice() {
    rbp_param p = sweep_param();
    double gmin[3], gmax[3], gres[3];
    int32_t dim[3];
    CHECK(R::planning_lattice(&p, 65535, gmin, gmax, gres, dim));
    CHECK(dim[0] == 21 && dim[1] == 21 && dim[2] == 2);
    CHECK(gmin[0] == -5.0 && gmin[1] == -5.0 && gmin[2] == 1.0);  // tests/synth_ecbs.py: cell z = 0 at 1 m, x = 10 at 0 m
    CHECK(gmax[0] == 5.0 && gmax[1] == 5.0 && gmax[2] == 2.0);
    CHECK(gres[0] == 0.5 && gres[1] == 0.5 && gres[2] == 1.0);

    // what is no lattice
    for (double bad : {0.0, -0.5, (double)NAN}) {
        rbp_param q = sweep_param();
        q.grid_xy_res = bad;
        CHECK(!R::planning_lattice(&q, 65535, gmin, gmax, gres, dim));
        q = sweep_param(), q.grid_z_res = bad;
        CHECK(!R::planning_lattice(&q, 65535, gmin, gmax, gres, dim));
    }
    rbp_param wide = sweep_param();
    wide.grid_xy_res = 1.0, wide.world_min[0] = 0, wide.world_max[0] = 65535;  // 65536 cells along x
    CHECK(!R::planning_lattice(&wide, 65535, gmin, gmax, gres, dim));
    wide.world_max[0] = 65534;
    CHECK(R::planning_lattice(&wide, 65535, gmin, gmax, gres, dim) && dim[0] == 65535);
    rbp_param empty = sweep_param();
    empty.world_min[2] = 1.2, empty.world_max[2] = 1.8;  // no multiple of 1.0 inside
    CHECK(!R::planning_lattice(&empty, 65535, gmin, gmax, gres, dim));

    // positions
    CHECK(R::planning_lattice(&p, 65535, gmin, gmax, gres, dim));
    CHECK(R::position_to_cell(-5.0, gmin[0], gres[0], dim[0]) == 0 && R::position_to_cell(5.0, gmin[0], gres[0], dim[0]) == 20);
    CHECK(R::position_to_cell(0.2, gmin[0], gres[0], dim[0]) == 10 && R::position_to_cell(0.3, gmin[0], gres[0], dim[0]) == 11);
    CHECK(R::position_to_cell(1.0, gmin[2], gres[2], dim[2]) == 0 && R::position_to_cell(2.0, gmin[2], gres[2], dim[2]) == 1);
    CHECK(R::position_to_cell(5.5, gmin[0], gres[0], dim[0]) == -1 && R::position_to_cell(-5.5, gmin[0], gres[0], dim[0]) == -1);
    for (double off : {1e300, -1e300, (double)NAN, (double)INFINITY})
        for (int a = 0; a < 3; ++a) CHECK(R::position_to_cell(off, gmin[a], gres[a], dim[a]) == -1);

    // samples
    std::vector<float> pos[3];
    std::vector<int> cell[3];
    R::lattice_samples(gmin, gmax, gres, dim, pos, cell);
    for (int a = 0; a < 3; ++a) {
        CHECK((int)pos[a].size() == dim[a] && cell[a].size() == pos[a].size());
        for (size_t i = 0; i < cell[a].size(); ++i) CHECK(cell[a][i] == (int)i);
    }
    double acc = gmin[0];  // the accumulating loop, not gmin + i * gres
    for (size_t i = 0; i < pos[0].size(); ++i, acc += gres[0]) CHECK(pos[0][i] == (float)acc);
    CHECK(pos[2][0] == 1.0f && pos[2][1] == 2.0f);
}

static void conflicts() {
    const double grid = 0.5;
    const Cell o{5, 5, 0}, px{6, 5, 0}, pxx{7, 5, 0}, pxxx{8, 5, 0}, py{5, 6, 0}, pxy{6, 6, 0}, pz{5, 5, 1};
    // the three regimes of tests/synth_ecbs.py: r 0.10, 0.15, 0.35 -> rr 0.2 < grid / 2 <= 0.3 < grid <= 0.7
    const double regime[3] = {0.1 + 0.1, 0.15 + 0.15, 0.35 + 0.35};
    CHECK(regime[0] < grid / 2 && grid / 2 <= regime[1] && regime[1] < grid && grid <= regime[2]);
    for (int k = 0; k < 3; ++k) {
        const double rr = regime[k];
        // vertex: below the grid only the same cell; at rr 0.7 a neighbour at 0.5 m too, the diagonal at 0.7071 m not
        CHECK(R::vertex_conflict(rr, grid, o, o));
        CHECK(R::vertex_conflict(rr, grid, o, px) == (k == 2));
        CHECK(R::vertex_conflict(rr, grid, px, o) == (k == 2));
        CHECK(R::vertex_conflict(rr, grid, o, pz) == (k == 2));
        CHECK(!R::vertex_conflict(rr, grid, o, pxy));
        CHECK(!R::vertex_conflict(rr, grid, o, pxx));
        // edge: a swap conflicts in every regime (the relative motion passes through the origin)
        CHECK(R::edge_conflict(rr, grid, o, px, px, o));
        CHECK(R::edge_conflict(rr, grid, o, pz, pz, o));
        // head-on into one cell: the exchange rule does not see it, the closest approach is 0
        CHECK(R::edge_conflict(rr, grid, o, px, pxx, px) == (k >= 1));
        // head-on with a cell between them afterwards: closest approach 0.5 m
        CHECK(R::edge_conflict(rr, grid, o, px, pxxx, pxx) == (k == 2));
        // side by side, one cell apart all along: 0.5 m
        CHECK(R::edge_conflict(rr, grid, o, px, py, pxy) == (k == 2));
        // one waits, the other leaves from the next cell: never closer than 0.5 m
        CHECK(R::edge_conflict(rr, grid, o, o, px, pxx) == (k == 2));
        // crossing paths: o -> px while py -> o.  The relative motion (0, 1, 0) -> (-1, 0, 0) comes within sqrt(1/2) cells = 0.3536 m
        CHECK(R::edge_conflict(rr, grid, o, px, py, o) == (k == 2));
        // far apart
        CHECK(!R::edge_conflict(rr, grid, o, px, Cell{9, 9, 1}, Cell{9, 8, 1}));
    }
    // the bound is inclusive for edges (<=) and exclusive for vertices (<): rr = 0.5 exactly, one cell apart
    CHECK(!R::vertex_conflict(0.5, grid, o, px) && R::edge_conflict(0.5, grid, o, px, py, pxy));
}

static void plan() {
    rbp_param p = sweep_param();
    double gmin[3], gmax[3], gres[3];
    int32_t dim[3];
    CHECK(R::planning_lattice(&p, 65535, gmin, gmax, gres, dim));
    const std::vector<std::vector<Cell>> sol = {{{10, 10, 0}, {11, 10, 0}, {12, 10, 0}}, {{3, 4, 1}}};  // costs 2 and 0
    double start[18] = {0}, goal[18] = {0};
    start[0] = 0.01, start[1] = 0.02, start[2] = 1.03, goal[0] = 1.01, goal[1] = 0.02, goal[2] = 0.97;
    start[9] = -3.49, start[10] = -3.01, start[11] = 2.0, goal[9] = -3.5, goal[10] = -3.0, goal[11] = 2.125;
    auto len_of = [&](int a) { return (int)sol[a].size(); };
    auto cell_at = [&](int a, int i) { return sol[a][i]; };
    int32_t makespan = -1, sum_cost = -1;
    const int M = R::plan_segments(2, len_of, &makespan, &sum_cost);
    CHECK(M == 4 && makespan == 2 && sum_cost == 2);
    for (size_t stride : {(size_t)5, (size_t)8}) {  // the host's M + 1, and a batch's max_M + 1
        std::vector<double> T(stride, -1.0);
        std::vector<float> tr(2 * stride * 3, -1.0f);
        R::write_plan(M, 2, len_of, cell_at, start, goal, gmin, gres, 0.5, stride, T.data(), tr.data());
        for (size_t i = 0; i < stride; ++i) CHECK(T[i] == (i <= 4 ? 0.5 * i : -1.0));
        auto at = [&](int a, int i, float x, float y, float z) {
            const float* q = &tr[((size_t)a * stride + i) * 3];
            return q[0] == x && q[1] == y && q[2] == z;
        };
        CHECK(at(0, 0, 0.01f, 0.02f, 1.03f));
        CHECK(at(0, 1, 0.0f, 0.0f, 1.0f) && at(0, 2, 0.5f, 0.0f, 1.0f) && at(0, 3, 1.0f, 0.0f, 1.0f));
        CHECK(at(0, 4, 1.01f, 0.02f, 0.97f));
        CHECK(at(1, 0, -3.49f, -3.01f, 2.0f));
        CHECK(at(1, 1, -3.5f, -3.0f, 2.0f));
        for (int i = 2; i <= 4; ++i) CHECK(at(1, i, -3.5f, -3.0f, 2.125f));  // the goal repeated to index M
        for (int a = 0; a < 2; ++a)
            for (size_t i = 5; i < stride; ++i) CHECK(at(a, (int)i, -1.0f, -1.0f, -1.0f));  // nothing past M
    }
}

int main() {
    lattice();
    conflicts();
    plan();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    else std::puts("ecbs rules ok");
    return failures ? 1 : 0;
}
