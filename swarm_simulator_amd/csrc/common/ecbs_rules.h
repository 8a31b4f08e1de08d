// ecbs_rules.h — the rules of the ECBS front-end that decide its bits, each stated once for the host search (host/ecbs.cpp, g++) and the
// device search (kernels/ecbs.hip, kernels/edt.hip, kernels/handoff.hip, hipcc): the planning lattice, position -> cell, the lattice samples
// of the obstacle mask, the two conflict predicates and the writer of T / init_traj, per element and as the host's loop.  Everything else
// in either search is integer arithmetic on queues.
// Plain C++17, no HIP runtime include.  ECBS_RULE functions are host + device functions under hipcc and inline functions under g++.
//
// Floating point, said here and nowhere else: both sides must round every operation of these rules alike, one IEEE double operation at
// a time.  No multiply and add may be fused: clang gets `#pragma clang fp contract(off)` below, which holds for the rest of the
// translation unit that includes this file; g++ on x86-64 does not contract without -mfma (or an -march that implies it), and
// csrc/Makefile gives neither.  Square roots and divisions go through rule_sqrt / rule_div: the correctly rounded __dsqrt_rn / __ddiv_rn
// in device code (where plain sqrt and / may become faster, less exact sequences), std::sqrt and / on the host, correctly rounded by IEEE 754.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "rbp.h"

#if defined(__HIPCC__)
#define ECBS_RULE __host__ __device__ inline __attribute__((always_inline))
#else
#define ECBS_RULE inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ecbs_rules {

constexpr double EPSILON = 1e-9;  // SP_EPSILON (sp_const.hpp:3)

#if defined(__HIP_DEVICE_COMPILE__)
ECBS_RULE double rule_sqrt(double v) { return __dsqrt_rn(v); }
ECBS_RULE double rule_div(double a, double b) { return __ddiv_rn(a, b); }
#else
ECBS_RULE double rule_sqrt(double v) { return std::sqrt(v); }
ECBS_RULE double rule_div(double a, double b) { return a / b; }
#endif

// the planning lattice (init_traj_planner.hpp:19-29): per axis the first and last sample, the step and the cell count.
// false when a step is not positive or an axis has no cell or more than max_cells.
ECBS_RULE bool planning_lattice(const rbp_param* param, int max_cells, double gmin[3], double gmax[3], double gres[3], int32_t dim[3]) {
    gres[0] = gres[1] = param->grid_xy_res, gres[2] = param->grid_z_res;
    for (int a = 0; a < 3; ++a) {
        if (!(gres[a] > 0)) return false;
        gmin[a] = std::ceil((param->world_min[a] - EPSILON) / gres[a]) * gres[a];
        gmax[a] = std::floor((param->world_max[a] + EPSILON) / gres[a]) * gres[a];
        const double n = std::round((gmax[a] - gmin[a]) / gres[a]) + 1;
        if (!(n > 0) || n > max_cells) return false;
        dim[a] = (int32_t)n;
    }
    return true;
}

// the lattice cell of a position along one axis (ecbs_planner.hpp:112-136), -1 when it is off the lattice (or not a number)
ECBS_RULE int position_to_cell(double v, double gmin, double gres, int dim) {
    const double c = std::round((v - gmin) / gres);
    return c >= 0 && c < dim ? (int)c : -1;
}

// the samples of the obstacle mask along each axis, by the reference's own accumulating loop (ecbs_planner.hpp:80-109): the sample as
// float (octomap::point3d) and the mask cell it sets (-1: none).  The sum `i += gres` is what the reference evaluates; gmin + n * gres is not.
inline void lattice_samples(const double gmin[3], const double gmax[3], const double gres[3], const int32_t dim[3], std::vector<float> pos[3],
                            std::vector<int> cell[3]) {
    for (int a = 0; a < 3; ++a)
        for (double i = gmin[a]; i < gmax[a] + EPSILON; i += gres[a])
            pos[a].push_back((float)i), cell[a].push_back(position_to_cell(i, gmin[a], gres[a], dim[a]));
}

// The conflict rules of two agents with radii summing to rr on a lattice of step `grid` (the only floating point of the search); a Cell
// has x(), y(), z() and ==.  environment.hpp:656-664
template <class Cell>
ECBS_RULE bool vertex_conflict(double rr, double grid, const Cell& a, const Cell& b) {
    if (rr < grid) return a == b;
    const double dx = b.x() - a.x(), dy = b.y() - a.y(), dz = b.z() - a.z();
    return rule_sqrt(dx * dx + dy * dy + dz * dz) * grid < rr;
}

// environment.hpp:69-93 (closest approach of the relative motion to the origin) and :666-681
template <class Cell>
ECBS_RULE bool edge_conflict(double rr, double grid, const Cell& a1, const Cell& b1, const Cell& a2, const Cell& b2) {
    if (rr < grid * 0.5) return a1 == b2 && b1 == a2;
    const double ax = a2.x() - a1.x(), ay = a2.y() - a1.y(), az = a2.z() - a1.z();
    const double bx = b2.x() - b1.x(), by = b2.y() - b1.y(), bz = b2.z() - b1.z();
    double md = rule_sqrt(ax * ax + ay * ay + az * az);
    if (!(ax == bx && ay == by && az == bz)) {
        double d = rule_sqrt(bx * bx + by * by + bz * bz);
        if (md > d) md = d;
        double nx = bx - ax, ny = by - ay, nz = bz - az;
        const double nn = rule_sqrt(nx * nx + ny * ny + nz * nz);
        nx = rule_div(nx, nn), ny = rule_div(ny, nn), nz = rule_div(nz, nn);
        const double adn = ax * nx + ay * ny + az * nz;
        const double px = ax - nx * adn, py = ay - ny * adn, pz = az - nz * adn;
        d = rule_sqrt(px * px + py * py + pz * pz);
        if ((px - ax) * (px - bx) + (py - ay) * (py - by) + (pz - az) * (pz - bz) < 0 && md > d) md = d;
    }
    return md * grid <= rr;
}

// What a found solution becomes (ecbs_planner.hpp:34-70).  len_of(a): cells of agent a's path; cell_at(a, p): its cell p.
// The longest path cost, the sum of the path costs; returns the segment count M = makespan + 2.
template <class LenOf>
inline int plan_segments(int N, LenOf len_of, int32_t* makespan, int32_t* sum_cost) {
    *makespan = *sum_cost = 0;
    for (int a = 0; a < N; ++a) *makespan = std::max(*makespan, len_of(a) - 1), *sum_cost += len_of(a) - 1;
    return *makespan + 2;
}

// One element of what write_plan writes, for the host loop below and for the kernel that writes a plan where the search left its paths
// (kernels/handoff.hip).  The time of waypoint i:
ECBS_RULE double plan_time(int i, double time_step) { return i * time_step; }

// Coordinate `axis` of waypoint n of an agent whose path has `len` cells (path_cell(p): its cell p): waypoint 0 is the start state,
// 1..len are the path cells (in double, then octomap::point3d's float), everything after them is the goal.  start / goal: the agent's [9] states.
template <class PathCell>
ECBS_RULE float plan_waypoint(int n, int axis, int len, PathCell path_cell, const double* start, const double* goal, const double gmin[3],
                              const double gres[3]) {
    if (n == 0) return (float)start[axis];
    if (n > len) return (float)goal[axis];
    const auto c = path_cell(n - 1);
    const int ci = axis == 0 ? c.x() : axis == 1 ? c.y() : c.z();
    return (float)(ci * gres[axis] + gmin[axis]);
}

// T[0..M] and init_traj[N][stride][3], stride >= M + 1: per agent the start, its waypoints and the goal up to index M.
// start / goal: the mission's [N][9] states.
template <class LenOf, class CellAt>
inline void write_plan(int M, int N, LenOf len_of, CellAt cell_at, const double* start, const double* goal, const double gmin[3],
                       const double gres[3], double time_step, size_t stride, double* T, float* init_traj) {
    for (int i = 0; i <= M; ++i) T[i] = plan_time(i, time_step);
    for (int a = 0; a < N; ++a) {
        float* tr = init_traj + (size_t)a * stride * 3;
        const int len = len_of(a);
        auto path_cell = [&](int p) { return cell_at(a, p); };
        for (int n = 0; n <= M; ++n)
            for (int axis = 0; axis < 3; ++axis) tr[3 * n + axis] = plan_waypoint(n, axis, len, path_cell, start + 9 * a, goal + 9 * a, gmin, gres);
    }
}

}  // namespace ecbs_rules
