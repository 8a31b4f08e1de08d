// clearance_rules.h — how close a plan comes to the obstacles: the distance grid's value under every agent at every sample t = j * dt,
// less the agent's radius; the smallest such clearance and where it lies, how many (sample, agent) items hit an obstacle by the
// reference's own test (rbp_corridor.hpp:67: getDistance < radius - SP_EPSILON_FLOAT) and how many fell outside the grid.  Stated once for
// the host entry (host/validate.cpp rbp_clearance_host, g++) and the device kernels (kernels/clearance.hip, hipcc).  Plain C++, <math.h> and
// <stdint.h> only (through report_rules.h, which this file includes and leaves as it is).
//
// From report_rules.h, unchanged: scaled_time, sample_count, sample_time, segments_before, agent_position (Horner), rule_div -- so the
// times, the segment of a sample and the positions are the report's, bit for bit.
//
// The lookup of a position is DynamicEDTOctomap::getDistance(octomap::point3d) as include/rbp.h (rbp_world) describes it and the
// corridor's CPU checker restates it, said here and nowhere else (kernels/corridor.hip keeps its own key code): every coordinate is rounded to float
// (point3d is float32), the key is kd = floor(rf * (double)pf) with rf = rule_div(1.0, res), and whether the key lies in the grid is decided
// ON THE DOUBLES, kd >= key_min && kd < key_min + dim -- a NaN, an infinity or a key beyond int is then simply outside, and no
// out-of-range conversion to int ever happens.  Inside, the cell is ((ix * ny) + iy) * nz + iz in 64 bits and d = (double)dist[cell];
// outside, d = -1.0, which is a hit for every radius above -1 + 1e-6, as it is in the reference.
//
// Floating point: as report_rules.h says.  Every product and every sum rounds on its own (`#pragma clang fp contract(off)` below holds
// for the rest of the translation unit; a g++ target with FMA is refused); divisions go through rule_div.
#pragma once
#include "common/report_rules.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__FMA__)
#error "clearance_rules.h: g++ fuses a * b + c on a target with FMA; build this file without -mfma / -march=native (every product and sum rounds on its own)"
#endif

#define RBP_CLEARANCE_NONE 1e9        /* the clearance of a mission, or an agent, without a sample */
#define RBP_CLEARANCE_OUTSIDE (-1.0)  /* what a lookup outside the grid reads */
#define RBP_CLEARANCE_EPSILON 1e-6    /* SP_EPSILON_FLOAT (sp_const.hpp:4) */

namespace clearance_rules {

using report_rules::rule_div;

// octomap's resolution_factor
REPORT_RULE double resolution_factor(double res) { return rule_div(1.0, res); }

// one axis of the lookup: the index of coordinate p along an axis of `dim` cells whose first has key key_min; false: outside
REPORT_RULE bool axis_index(double rf, double p, int32_t key_min, int32_t dim, int64_t* index) {
    const float pf = (float)p;
    const double kd = floor(rf * (double)pf);
    const double lo = (double)key_min, hi = lo + (double)dim;  // (sums of two int32: exact)
    if (!(kd >= lo && kd < hi)) return false;                  // (a NaN fails both)
    *index = (int64_t)kd - (int64_t)key_min;                   // (kd is an integer within int32 here)
    return true;
}
// the cell of position p[3] in a grid [nx][ny][nz], z fastest; -1: outside
REPORT_RULE int64_t cell_of(const int32_t* dim, const int32_t* key_min, double rf, const double* p) {
    int64_t ix = 0, iy = 0, iz = 0;
    const bool in_x = axis_index(rf, p[0], key_min[0], dim[0], &ix);
    const bool in_y = axis_index(rf, p[1], key_min[1], dim[1], &iy);
    const bool in_z = axis_index(rf, p[2], key_min[2], dim[2], &iz);
    if (!(in_x && in_y && in_z)) return -1;
    return ((ix * (int64_t)dim[1]) + iy) * (int64_t)dim[2] + iz;
}
// the distance a lookup reads: the cell's float, or -1 outside (the caller loads dist[cell] where cell >= 0)
REPORT_RULE double distance_of(int64_t cell, float value) { return cell >= 0 ? (double)value : RBP_CLEARANCE_OUTSIDE; }

REPORT_RULE double clearance(double d, double radius) { return d - radius; }
// rbp_corridor.hpp:67
REPORT_RULE bool is_hit(double d, double radius) { return d < radius - RBP_CLEARANCE_EPSILON; }

// A minimum and where it was found.  The sequential rule is `if (c < min) min = c` from 1e9 over the samples, then the agents: the smallest
// clearance, and among equal clearances the lexicographically first (sample, agent); a clearance of 1e9 or more, or a NaN (a NaN radius),
// is never taken.  `take` keeps that minimum whatever the order candidates arrive in, which is what lets lanes and agents each keep their
// own and merge.  dist: the grid's value at the minimum.
struct Minimum {
    double clearance, dist;
    int32_t sample, agent;
};
REPORT_RULE Minimum no_minimum() { return Minimum{RBP_CLEARANCE_NONE, 0.0, -1, -1}; }
REPORT_RULE bool precedes(const Minimum& c, const Minimum& m) {
    if (c.clearance < m.clearance) return true;
    if (!(c.clearance == m.clearance)) return false;
    if (c.sample != m.sample) return c.sample < m.sample;
    return c.agent < m.agent;
}
REPORT_RULE void take(Minimum* m, const Minimum& c) {
    if (precedes(c, *m)) *m = c;
}

// what rbp_clearance (include/rbp.h) holds besides the mission's status
struct Result {
    Minimum min;
    double end_time;
    int64_t hits, outside;  // (sample, agent) items
    int32_t samples;
};
REPORT_RULE Result empty_result(double end_time, int32_t samples) { return Result{no_minimum(), end_time, 0, 0, samples}; }

// one (sample, agent) item: its candidate into *m, its counts into *hits / *outside
REPORT_RULE void take_item(Minimum* m, int64_t* hits, int64_t* outside, double d, bool inside, double radius, int32_t sample, int32_t agent) {
    take(m, Minimum{clearance(d, radius), d, sample, agent});
    if (is_hit(d, radius)) ++*hits;
    if (!inside) ++*outside;
}

// Everything, one sample after the other: the loop of the host entry, and the meaning of every shortcut the device takes.
// T [M+1] unscaled, coef [N][3][6M], radius [N]; the grid dist [dim0][dim1][dim2] with key_min and res.  agent_clearance [N] or null: every
// agent's smallest clearance over its samples (1e9 without one), written only where the samples are evaluated (samples >= 0).
REPORT_RULE Result clearance_sequential(int32_t N, int32_t M, const double* T, double ts, const double* coef, const double* radius,
                                        const int32_t* dim, const int32_t* key_min, double res, const float* dist, double dt,
                                        double* agent_clearance) {
    const double end_time = report_rules::scaled_time(T[M], ts);
    Result r = empty_result(end_time, report_rules::sample_count(end_time, dt));
    if (r.samples < 0) return r;
    const double rf = resolution_factor(res);
    if (agent_clearance)
        for (int32_t a = 0; a < N; ++a) agent_clearance[a] = RBP_CLEARANCE_NONE;
    int32_t before = 0;
    for (int32_t j = 0; j < r.samples; ++j) {
        const double t = report_rules::sample_time(j, dt);
        before = report_rules::segments_before(T, M, ts, t, before);
        for (int32_t a = 0; a < N; ++a) {
            double p[3];
            report_rules::agent_position(coef, M, T, ts, a, t, before, p);
            const int64_t cell = cell_of(dim, key_min, rf, p);
            const double d = distance_of(cell, cell >= 0 ? dist[cell] : 0.0f);
            take_item(&r.min, &r.hits, &r.outside, d, cell >= 0, radius[a], j, a);
            if (agent_clearance && clearance(d, radius[a]) < agent_clearance[a]) agent_clearance[a] = clearance(d, radius[a]);
        }
    }
    return r;
}

}  // namespace clearance_rules
