// state_rules.h — what the reference's publisher samples of a plan besides the two numbers of report_rules.h (rbp_publisher.hpp:670-683
// update_quad_state, :697-767 plot_quad_dynamics, :769-798 update_safety_margin_ratio): position, velocity and acceleration of every agent
// at every sample t = j * dt, the largest velocity and acceleration as fractions of the agents' limits and where they lie, and the
// smallest and largest safety ratio of every sample.  Stated once for the host entry (host/validate.cpp rbp_dynamics_host, g++) and the
// device kernels (kernels/dynamics.hip, hipcc).  Plain C++, <math.h> and <stdint.h> only (through report_rules.h, which this file
// includes and leaves as it is).
//
// From report_rules.h, unchanged: scaled_time, sample_count, sample_time, segments_before, segment_index, segment_time, position,
// coef_of, safety_ratio, rule_div -- so the times, the segment of a sample (one on a knot belongs to the earlier segment) and the
// position rows are the report's, bit for bit.
//
// Floating point: as report_rules.h says.  Every product and every sum rounds on its own (`#pragma clang fp contract(off)` below holds
// for the rest of the translation unit; a g++ target with FMA is refused); divisions go through rule_div.
#pragma once
#include "common/report_rules.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__FMA__)
#error "state_rules.h: g++ fuses a * b + c on a target with FMA; build this file without -mfma / -march=native (every product and sum rounds on its own)"
#endif

namespace state_rules {

using report_rules::rule_div;

// d/dt of the quintic with descending-power coefficients c[0..5]: Horner over 5 c0, 4 c1, 3 c2, 2 c3, c4.  The integer factor is
// applied to the coefficient first (a product of its own), then the running value times tseg, then the sum.
REPORT_RULE double velocity(const double* c, double tseg) {
    double v = 5.0 * c[0];
    for (int i = 1; i < 5; ++i) {
        const double p = v * tseg;
        const double q = (double)(5 - i) * c[i];
        v = p + q;
    }
    return v;
}
// d2/dt2: Horner over 20 c0, 12 c1, 6 c2, 2 c3
REPORT_RULE double acceleration(const double* c, double tseg) {
    double v = 20.0 * c[0];
    for (int i = 1; i < 4; ++i) {
        const double p = v * tseg;
        const double q = (double)((5 - i) * (4 - i)) * c[i];
        v = p + q;
    }
    return v;
}

// position, velocity and acceleration of one axis of one segment at tseg
REPORT_RULE void axis_state(const double* c, double tseg, double* p, double* v, double* a) {
    *p = report_rules::position(c, tseg);
    *v = velocity(c, tseg);
    *a = acceleration(c, tseg);
}

// The state of agent qi at sample time t, whose count of segments begun is `before`: nine doubles in the reference's row order,
// row / 3 = derivative, row % 3 = axis: p_x p_y p_z v_x v_y v_z a_x a_y a_z.  Rows 0..2 are report_rules::agent_position.
REPORT_RULE void agent_state(const double* coef, int32_t M, const double* T, double ts, int32_t qi, double t, int32_t before, double* s) {
    const int32_t m = report_rules::segment_index(before);
    const double tseg = report_rules::segment_time(T, ts, t, before);
    for (int k = 0; k < 3; ++k) axis_state(report_rules::coef_of(coef, M, qi, k, m), tseg, s + k, s + 3 + k, s + 6 + k);
}

// |value| as a fraction of its limit: above 1 the plan breaks the limit at this sample
REPORT_RULE double limit_ratio(double value, double limit) { return rule_div(fabs(value), limit); }

// A peak and where it was found.  The sequential rule is `if (r > max) max = r` from 0 over the samples, then the agents, then the axes:
// the largest ratio, and among equal ratios the lexicographically smallest (sample, agent, axis); a ratio of 0, a negative one or a NaN is
// never taken.  `take` keeps that peak whatever the order candidates arrive in.  value: the velocity or acceleration itself, with its
// sign; limit: what it was divided by.
struct Peak {
    double ratio, value, limit;
    int32_t sample, agent, axis, pad;
};
REPORT_RULE Peak no_peak() { return Peak{0.0, 0.0, 0.0, -1, -1, -1, 0}; }
REPORT_RULE bool precedes(const Peak& c, const Peak& m) {
    if (c.ratio > m.ratio) return true;
    if (!(c.ratio == m.ratio)) return false;
    if (c.sample != m.sample) return c.sample < m.sample;
    if (c.agent != m.agent) return c.agent < m.agent;
    return c.axis < m.axis;
}
REPORT_RULE void take(Peak* m, const Peak& c) {
    if (precedes(c, *m)) *m = c;
}
// the two candidates of one axis of a state: its velocity into *vel, its acceleration into *acc
REPORT_RULE void take_axis(Peak* vel, Peak* acc, double v, double a, double lim_v, double lim_a, int32_t sample, int32_t agent, int32_t axis) {
    take(vel, Peak{limit_ratio(v, lim_v), v, lim_v, sample, agent, axis, 0});
    take(acc, Peak{limit_ratio(a, lim_a), a, lim_a, sample, agent, axis, 0});
}
// the six candidates of one state.  lim_v / lim_a: the agent's three limits.
REPORT_RULE void take_state(Peak* vel, Peak* acc, const double* s, const double* lim_v, const double* lim_a, int32_t sample, int32_t agent) {
    for (int k = 0; k < 3; ++k) take_axis(vel, acc, s[3 + k], s[6 + k], lim_v[k], lim_a[k], sample, agent, k);
}

// The ratio curves of one sample: the minimum from 1e9 and the maximum from 0 of the pairs' safety ratios, by the reference's two
// comparisons -- a NaN changes neither.  Only values are kept, so partial curves merge by the same two comparisons in any order.
struct Curve {
    double min_ratio, max_ratio;
};
REPORT_RULE Curve no_curve() { return Curve{RBP_REPORT_NO_RATIO, 0.0}; }
REPORT_RULE void curve_take(Curve* c, double r) {
    if (r < c->min_ratio) c->min_ratio = r;
    if (r > c->max_ratio) c->max_ratio = r;
}
REPORT_RULE void curve_merge(Curve* c, const Curve& o) {
    if (o.min_ratio < c->min_ratio) c->min_ratio = o.min_ratio;
    if (o.max_ratio > c->max_ratio) c->max_ratio = o.max_ratio;
}

// what rbp_dynamics (include/rbp.h) holds besides the mission's status
struct Result {
    Peak vel, acc;
    double end_time;
    int32_t samples, stored;
};
// whether the states and curves of a mission of `samples` samples are written: a buffer was given and a row of S_stride holds them
REPORT_RULE bool stores(int32_t samples, bool buffer_given, int32_t S_stride) { return buffer_given && samples >= 0 && samples <= S_stride; }

// Everything, one sample after the other: the loop of the host entry, and the meaning of every shortcut the device takes.
// T [M+1] unscaled, coef [N][3][6M], radius [N], max_vel / max_acc [N][3]; states [N][9][S_stride] or null, curves [S_stride][2] or null:
// written for samples <= S_stride only, entries beyond `samples` left as they are.  scratch: 3 N doubles (a sample's positions).
REPORT_RULE Result states_sequential(int32_t N, int32_t M, const double* T, double ts, const double* coef, const double* radius,
                                     const double* max_vel, const double* max_acc, double downwash, double dt, double* states,
                                     double* curves, int32_t S_stride, double* scratch) {
    Result r;
    r.vel = no_peak(), r.acc = no_peak();
    r.end_time = report_rules::scaled_time(T[M], ts);
    r.samples = report_rules::sample_count(r.end_time, dt);
    const bool store = stores(r.samples, states || curves, S_stride);
    r.stored = store ? 1 : 0;
    if (r.samples < 0) return r;
    int32_t before = 0;
    for (int32_t j = 0; j < r.samples; ++j) {
        const double t = report_rules::sample_time(j, dt);
        before = report_rules::segments_before(T, M, ts, t, before);
        for (int32_t qi = 0; qi < N; ++qi) {
            double s[9];
            agent_state(coef, M, T, ts, qi, t, before, s);
            take_state(&r.vel, &r.acc, s, max_vel + 3 * (int64_t)qi, max_acc + 3 * (int64_t)qi, j, qi);
            for (int k = 0; k < 3; ++k) scratch[3 * (int64_t)qi + k] = s[k];
            if (store && states)
                for (int row = 0; row < 9; ++row) states[((int64_t)qi * 9 + row) * S_stride + j] = s[row];
        }
        if (store && curves) {
            Curve c = no_curve();
            for (int32_t qi = 0; qi < N; ++qi)
                for (int32_t qj = qi + 1; qj < N; ++qj)
                    curve_take(&c, report_rules::safety_ratio(scratch + 3 * (int64_t)qi, scratch + 3 * (int64_t)qj, downwash, radius[qi] + radius[qj]));
            curves[2 * (int64_t)j] = c.min_ratio, curves[2 * (int64_t)j + 1] = c.max_ratio;
        }
    }
    return r;
}

}  // namespace state_rules
