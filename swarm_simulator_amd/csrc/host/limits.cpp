// The host's certified velocity and acceleration limits in continuous time.  A file of its own, not a part of validate.cpp: it holds no
// arithmetic, only the loop of common/limits_rules.h and the copy of its tally into the C struct.
#include "rbp_host.h"

#include "common/limits_rules.h"

// The certified intervals of the plan's largest velocity and acceleration ratios in continuous time by the rule of common/limits_rules.h,
// which the device's limits kernels (kernels/limits.hip) share.  T arrives scaled, so the scale is 1.
extern "C" int rbp_limits_host(const rbp_mission* mission, int32_t M, const double* T, const double* coef, int32_t depth, double refine_above,
                               rbp_limits* out, double* agent_upper) {
    if (!mission || !T || !coef || !out || !mission->max_vel || !mission->max_acc || mission->N <= 0 || M <= 0 || depth < 0 ||
        depth > RBP_LIMITS_MAX_DEPTH || refine_above != refine_above)
        return RBP_ERR_BAD_ARGUMENT;
    const limits_rules::Tally t =
        limits_rules::limits_sequential(mission->N, M, T, 1.0, coef, mission->max_vel, mission->max_acc, depth, refine_above, agent_upper);
    out->lower_vel_ratio = t.lower_vel.ratio, out->upper_vel_ratio = t.upper_vel.ratio;
    out->lower_acc_ratio = t.lower_acc.ratio, out->upper_acc_ratio = t.upper_acc.ratio, out->end_time = T[M];
    out->uncertified = t.uncertified, out->violating = t.violating, out->refined = t.refined;
    out->lower_vel_segment = t.lower_vel.segment, out->lower_vel_piece = t.lower_vel.piece, out->lower_vel_agent = t.lower_vel.agent;
    out->lower_vel_axis = t.lower_vel.axis, out->lower_vel_depth = t.lower_vel.depth;
    out->upper_vel_segment = t.upper_vel.segment, out->upper_vel_piece = t.upper_vel.piece, out->upper_vel_agent = t.upper_vel.agent;
    out->upper_vel_axis = t.upper_vel.axis, out->upper_vel_depth = t.upper_vel.depth;
    out->lower_acc_segment = t.lower_acc.segment, out->lower_acc_piece = t.lower_acc.piece, out->lower_acc_agent = t.lower_acc.agent;
    out->lower_acc_axis = t.lower_acc.axis, out->lower_acc_depth = t.lower_acc.depth;
    out->upper_acc_segment = t.upper_acc.segment, out->upper_acc_piece = t.upper_acc.piece, out->upper_acc_agent = t.upper_acc.agent;
    out->upper_acc_axis = t.upper_acc.axis, out->upper_acc_depth = t.upper_acc.depth;
    out->status = 0, out->reserved = 0;
    return RBP_OK;
}
