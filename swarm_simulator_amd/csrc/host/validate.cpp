// Validation metrics and the crazyswarm CSV writer — the reference's own acceptance signals.
//   sampler            rbp_publisher.hpp:50-54 (t = i*0.1, floor(T.back()/dt) samples), :169-194 (timeMatrix), :670-683
//   flight distance    rbp_publisher.hpp:685-695
//   safety ratio       rbp_publisher.hpp:769-798   (downwash-scaled distance / (r_i + r_j); should be >= 1)
//   coef CSV           rbp_planner.hpp:295-324
#include "rbp_host.h"

#include "common/clearance_rules.h"
#include "common/report_rules.h"
#include "common/separation_rules.h"
#include "common/state_rules.h"
#include "common/swept_rules.h"

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

extern "C" int rbp_validate(const rbp_mission* mission, const rbp_param* param, int32_t M, const double* T,
                            const double* coef, double dt, double* min_safety_ratio, double* total_flight_distance) {
    if (!mission || !param || !T || !coef || M <= 0 || dt <= 0) return RBP_ERR_BAD_ARGUMENT;
    const int N = mission->N, n = 5;
    const int nt = (int)std::floor(T[M] / dt);
    std::vector<double> pos((size_t)N * nt * 3);
    for (int j = 0; j < nt; ++j) {
        double t = j * dt;
        // rbp_publisher.hpp:173-183: last segment whose start time is strictly before t (segment 0 at t=0)
        int index = 0;
        double tseg = 0;
        for (int m = 0; m < M; ++m) {
            if (T[m] < t) {
                tseg = T[m];
                index = m;
            } else
                break;
        }
        tseg = t - tseg;
        for (int qi = 0; qi < N; ++qi)
            for (int k = 0; k < 3; ++k) {
                const double* c = coef + ((size_t)qi * 3 + k) * 6 * M + 6 * index;  // descending powers
                double v = 0;
                for (int i = 0; i <= n; ++i) v += c[i] * std::pow(tseg, n - i);
                pos[((size_t)qi * nt + j) * 3 + k] = v;
            }
    }
    double len = 0;
    for (int qi = 0; qi < N; ++qi)
        for (int j = 0; j + 1 < nt; ++j) {
            const double* a = &pos[((size_t)qi * nt + j) * 3];
            const double* b = a + 3;
            len += std::sqrt((b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1]) + (b[2] - a[2]) * (b[2] - a[2]));
        }
    double ratio_min = 1e9;  // SP_INFINITY
    for (int j = 0; j < nt; ++j)
        for (int qi = 0; qi < N; ++qi)
            for (int qj = qi + 1; qj < N; ++qj) {
                const double* a = &pos[((size_t)qi * nt + j) * 3];
                const double* b = &pos[((size_t)qj * nt + j) * 3];
                double dz = (a[2] - b[2]) / param->downwash;
                double r = std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + dz * dz) /
                           (mission->radius[qi] + mission->radius[qj]);
                if (r < ratio_min) ratio_min = r;
            }
    if (min_safety_ratio) *min_safety_ratio = ratio_min;
    if (total_flight_distance) *total_flight_distance = len;
    return RBP_OK;
}

// The same two signals by the rule of common/report_rules.h, which the device's report kernels (kernels/report.hip) share: Horner
// positions, one sum of step lengths per agent, and where the minimum is.  T arrives scaled (a downloaded plan's), so the scale is 1.
extern "C" int rbp_report_host(const rbp_mission* mission, const rbp_param* param, int32_t M, const double* T, const double* coef,
                               double dt, rbp_report* out) {
    if (!mission || !param || !T || !coef || !out || !mission->radius || mission->N <= 0 || M <= 0 || !(dt > 0)) return RBP_ERR_BAD_ARGUMENT;
    std::vector<double> scratch((size_t)7 * mission->N);
    const report_rules::Result r =
        report_rules::report_sequential(mission->N, M, T, 1.0, coef, mission->radius, param->downwash, dt, scratch.data());
    out->min_safety_ratio = r.min_safety_ratio, out->total_flight_distance = r.total_flight_distance, out->end_time = r.end_time;
    out->samples = r.samples, out->min_sample = r.min_sample, out->min_qi = r.min_qi, out->min_qj = r.min_qj;
    out->status = 0, out->reserved = 0;
    return RBP_OK;
}

// The sampled states, limit peaks and ratio curves by the rule of common/state_rules.h, which the device's dynamics kernels
// (kernels/dynamics.hip) share.  T arrives scaled, so the scale is 1.
extern "C" int rbp_dynamics_host(const rbp_mission* mission, const rbp_param* param, int32_t M, const double* T, const double* coef,
                                 double dt, rbp_dynamics* out, double* states, double* curves, int32_t S_stride) {
    if (!mission || !param || !T || !coef || !out || !mission->radius || !mission->max_vel || !mission->max_acc || mission->N <= 0 || M <= 0 ||
        !(dt > 0) || ((states || curves) && S_stride < 1))
        return RBP_ERR_BAD_ARGUMENT;
    std::vector<double> scratch((size_t)3 * mission->N);
    const state_rules::Result r = state_rules::states_sequential(mission->N, M, T, 1.0, coef, mission->radius, mission->max_vel, mission->max_acc,
                                                                 param->downwash, dt, states, curves, S_stride, scratch.data());
    out->peak_vel_ratio = r.vel.ratio, out->peak_vel = r.vel.value, out->peak_vel_limit = r.vel.limit;
    out->peak_acc_ratio = r.acc.ratio, out->peak_acc = r.acc.value, out->peak_acc_limit = r.acc.limit;
    out->end_time = r.end_time, out->samples = r.samples;
    out->vel_sample = r.vel.sample, out->vel_agent = r.vel.agent, out->vel_axis = r.vel.axis;
    out->acc_sample = r.acc.sample, out->acc_agent = r.acc.agent, out->acc_axis = r.acc.axis;
    out->stored = r.stored, out->status = 0;
    return RBP_OK;
}

// The plan's clearance to the obstacles of its world by the rule of common/clearance_rules.h, which the device's clearance kernels
// (kernels/clearance.hip) share.  T arrives scaled, so the scale is 1.
extern "C" int rbp_clearance_host(const rbp_world* world, const rbp_mission* mission, int32_t M, const double* T, const double* coef, double dt,
                                  rbp_clearance* out, double* agent_clearance) {
    if (!world || !mission || !T || !coef || !out || !world->dist || !mission->radius || mission->N <= 0 || M <= 0 || !(dt > 0) || !(world->res > 0) ||
        world->dim[0] <= 0 || world->dim[1] <= 0 || world->dim[2] <= 0)
        return RBP_ERR_BAD_ARGUMENT;
    const clearance_rules::Result r = clearance_rules::clearance_sequential(mission->N, M, T, 1.0, coef, mission->radius, world->dim, world->key_min,
                                                                            world->res, world->dist, dt, agent_clearance);
    out->min_clearance = r.min.clearance, out->min_dist = r.min.dist, out->end_time = r.end_time;
    out->hits = r.hits, out->outside = r.outside;
    out->samples = r.samples, out->min_sample = r.min.sample, out->min_agent = r.min.agent, out->status = 0;
    return RBP_OK;
}

// The certified interval of the plan's smallest safety ratio in continuous time by the rule of common/separation_rules.h, which the
// device's separation kernels (kernels/separation.hip) share.  T arrives scaled, so the scale is 1.
extern "C" int rbp_separation_host(const rbp_mission* mission, const rbp_param* param, int32_t M, const double* T, const double* coef,
                                   int32_t depth, double refine_below, rbp_separation* out, double* pair_lower) {
    if (!mission || !param || !T || !coef || !out || !mission->radius || mission->N <= 0 || M <= 0 || depth < 0 ||
        depth > RBP_SEPARATION_MAX_DEPTH || !(refine_below > 0))
        return RBP_ERR_BAD_ARGUMENT;
    const separation_rules::Tally t = separation_rules::separation_sequential(mission->N, M, T, 1.0, coef, mission->radius, param->downwash,
                                                                              depth, refine_below, pair_lower);
    out->lower_ratio = t.lower.ratio, out->upper_ratio = t.upper.ratio, out->end_time = T[M];
    out->uncertified = t.uncertified, out->colliding = t.colliding, out->refined = t.refined;
    out->lower_segment = t.lower.segment, out->lower_piece = t.lower.piece, out->lower_qi = t.lower.qi, out->lower_qj = t.lower.qj;
    out->upper_segment = t.upper.segment, out->upper_piece = t.upper.piece, out->upper_qi = t.upper.qi, out->upper_qj = t.upper.qj;
    out->lower_depth = t.lower.depth, out->upper_depth = t.upper.depth;
    out->status = 0, out->reserved = 0;
    return RBP_OK;
}

// The certified interval of the plan's smallest clearance to the obstacles in continuous time by the rule of common/swept_rules.h, which
// the device's swept kernels (kernels/swept.hip) share.  T arrives scaled, so the scale is 1.
extern "C" int rbp_swept_clearance_host(const rbp_world* world, const rbp_mission* mission, int32_t M, const double* T, const double* coef,
                                        int32_t depth, double refine_below, rbp_swept_clearance* out, double* agent_lower) {
    if (!world || !mission || !T || !coef || !out || !world->dist || !mission->radius || mission->N <= 0 || M <= 0 || depth < 0 ||
        depth > RBP_SWEPT_MAX_DEPTH || refine_below != refine_below || !(world->res > 0) || world->dim[0] <= 0 || world->dim[1] <= 0 ||
        world->dim[2] <= 0)
        return RBP_ERR_BAD_ARGUMENT;
    const swept_rules::Tally t = swept_rules::swept_sequential(mission->N, M, T, 1.0, coef, mission->radius, world->dim, world->key_min, world->res,
                                                               world->dist, depth, refine_below, agent_lower);
    out->lower_clearance = t.lower.clearance, out->upper_clearance = t.upper.clearance;
    out->lower_dist = t.lower.dist, out->upper_dist = t.upper.dist, out->end_time = T[M];
    out->uncertified = t.uncertified, out->hitting = t.hitting, out->outside = t.outside, out->over_budget = t.over_budget, out->refined = t.refined;
    out->lower_segment = t.lower.segment, out->lower_piece = t.lower.piece, out->lower_agent = t.lower.agent, out->lower_depth = t.lower.depth;
    out->upper_segment = t.upper.segment, out->upper_piece = t.upper.piece, out->upper_agent = t.upper.agent, out->upper_depth = t.upper.depth;
    out->status = 0, out->reserved = 0;
    return RBP_OK;
}

extern "C" int rbp_write_coef_csv(const char* dir, int32_t N, int32_t M, const double* T, const double* coef) {
    if (!dir || !T || !coef) return RBP_ERR_BAD_ARGUMENT;
    const int n = 5;
    for (int qi = 0; qi < N; ++qi) {
        std::string path = std::string(dir) + "/coef" + std::to_string(qi + 1) + ".csv";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) return RBP_ERR_BAD_ARGUMENT;
        fprintf(f, "duration");
        for (const char* ax : {"x", "y", "z", "yaw"})
            for (int i = 0; i < 8; ++i) fprintf(f, ",%s^%d", ax, i);
        fprintf(f, "\n");
        for (int m = 0; m < M; ++m) {
            fprintf(f, "%g,", T[m + 1] - T[m]);
            for (int k = 0; k < 3; ++k) {
                const double* c = coef + ((size_t)qi * 3 + k) * 6 * M + 6 * m;
                for (int i = n; i >= 0; --i) fprintf(f, "%g,", c[i]);  // ascending powers
                for (int i = 0; i < 7 - n; ++i) fprintf(f, "0,");
            }
            for (int i = 0; i < 8; ++i) fprintf(f, "0,");
            fprintf(f, "\n");
        }
        fclose(f);
    }
    return RBP_OK;
}
