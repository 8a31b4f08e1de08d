// report_rules.h — a mission's two acceptance signals, the sampled safety ratio over all pairs and the total flight distance
// (rbp_publisher.hpp:685-695, 769-798), stated once for the host entry (host/validate.cpp rbp_report_host, g++) and the device kernels
// (kernels/report.hip, hipcc): the scaled times, the number of samples, the segment of a sample, the position, the ratio of a pair,
// the order in which a minimum is kept, the step length, and the whole report as the host's loop (report_sequential).
// Plain C++, <math.h> and <stdint.h> only.  REPORT_RULE functions are host + device functions under hipcc and inline functions under g++.
//
// This is NOT the arithmetic of rbp_validate (host/validate.cpp), which stays as it is: that function raises tseg to its powers with
// std::pow (not correctly rounded, and not the same on a GPU) and keeps ONE running sum of step lengths over all agents, which fixes an order
// no parallel evaluation can keep.  Here a position is Horner's scheme and the distance is a sum per agent, then a sum over agents.
//
// Floating point, said here and nowhere else: both sides round every operation of these rules alike, one IEEE double operation at a time.
// No multiply and add may be fused: clang gets `#pragma clang fp contract(off)` below, which holds for the rest of the translation unit
// that includes this file; g++ contracts only where the target has FMA instructions, and such a build is refused below.  Square roots and
// divisions go through rule_sqrt / rule_div: the correctly rounded __dsqrt_rn / __ddiv_rn in device code, sqrt and / on the host.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define REPORT_RULE __host__ __device__ inline __attribute__((always_inline))
#else
#define REPORT_RULE inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__FMA__)
#error "report_rules.h: g++ fuses a * b + c on a target with FMA; build this file without -mfma / -march=native (every product and sum rounds on its own)"
#endif

#ifndef RBP_REPORT_MAX_SAMPLES           /* (include/rbp.h says the same) */
#define RBP_REPORT_MAX_SAMPLES (1 << 20) /* more samples than this are not evaluated: samples = -1 */
#endif
#define RBP_REPORT_NO_RATIO 1e9          /* SP_INFINITY: the ratio of a mission without a pair or without a sample */

namespace report_rules {

#if defined(__HIP_DEVICE_COMPILE__)
REPORT_RULE double rule_sqrt(double v) { return __dsqrt_rn(v); }
REPORT_RULE double rule_div(double a, double b) { return __ddiv_rn(a, b); }
#else
REPORT_RULE double rule_sqrt(double v) { return sqrt(v); }
REPORT_RULE double rule_div(double a, double b) { return a / b; }
#endif

// Ts[m]: the product rbp_session_download forms of a segment time and the mission's time scale (none for a scale of exactly 1)
REPORT_RULE double scaled_time(double T, double ts) { return (ts != 1.0) ? T * ts : T; }

// floor(Ts[M] / dt) samples (rbp_publisher.hpp:50-54); -1: more than RBP_REPORT_MAX_SAMPLES; an end time that is negative or no number: none
REPORT_RULE int32_t sample_count(double end_time, double dt) {
    const double q = floor(rule_div(end_time, dt));
    if (q > (double)RBP_REPORT_MAX_SAMPLES) return -1;
    if (!(q >= 1.0)) return 0;
    return (int32_t)q;
}

REPORT_RULE double sample_time(int32_t j, double dt) { return (double)j * dt; }

// The segment of time t (rbp_publisher.hpp:173-183, validate.cpp:21-31): how many of Ts[0], Ts[1], ... Ts[M-1], from the front, lie strictly
// before t.  The sample's segment is that count minus one (segment 0 when the count is 0) -- for ascending times the largest m with
// Ts[m] < t.  `from`: a count already known for an earlier time t' <= t (0 for none); the count only grows with t.
REPORT_RULE int32_t segments_before(const double* T, int32_t M, double ts, double t, int32_t from) {
    int32_t n = from;
    while (n < M && scaled_time(T[n], ts) < t) ++n;
    return n;
}
REPORT_RULE int32_t segment_index(int32_t before) { return before > 0 ? before - 1 : 0; }
// tseg = t - Ts[m], and t itself where no segment starts before t
REPORT_RULE double segment_time(const double* T, double ts, double t, int32_t before) {
    return before > 0 ? t - scaled_time(T[before - 1], ts) : t;
}

// Horner over the six descending-power coefficients c[0..5] of one axis of one segment (rbp_plan.coef)
REPORT_RULE double position(const double* c, double tseg) {
    double v = c[0];
    for (int i = 1; i < 6; ++i) {
        const double p = v * tseg;
        v = p + c[i];
    }
    return v;
}
// the six coefficients of agent qi, axis k, segment m in a mission's coef [N][3][6M]
REPORT_RULE const double* coef_of(const double* coef, int32_t M, int32_t qi, int32_t k, int32_t m) {
    return coef + ((int64_t)qi * 3 + k) * 6 * M + 6 * m;
}

// the safety ratio of two positions (validate.cpp:53-55): downwash-scaled distance over the sum of the radii
REPORT_RULE double safety_ratio(const double* a, const double* b, double downwash, double radius_sum) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = rule_div(a[2] - b[2], downwash);
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    return rule_div(rule_sqrt(xy + zz), radius_sum);
}

// the length of the step from position a to position b, the next sample's (validate.cpp:43-45)
REPORT_RULE double step_length(const double* a, const double* b) {
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    return rule_sqrt(xy + zz);
}

// A minimum and where it was found.  The sequential rule is `if (r < min) min = r` from 1e9 over the samples, then qi, then qj: the
// smallest ratio, and among equal ratios the lexicographically smallest (sample, qi, qj); a ratio of 1e9 or more, or a NaN, is never taken.
// `take` keeps that minimum whatever the order candidates arrive in, which is what lets lanes and blocks each keep their own and merge.
struct Minimum {
    double ratio;
    int32_t sample, qi, qj;
};
REPORT_RULE Minimum no_minimum() { return Minimum{RBP_REPORT_NO_RATIO, -1, -1, -1}; }
REPORT_RULE bool precedes(const Minimum& c, const Minimum& m) {
    if (c.ratio < m.ratio) return true;
    if (!(c.ratio == m.ratio)) return false;
    if (c.sample != m.sample) return c.sample < m.sample;
    if (c.qi != m.qi) return c.qi < m.qi;
    return c.qj < m.qj;
}
REPORT_RULE void take(Minimum* m, const Minimum& c) {
    if (precedes(c, *m)) *m = c;
}

// what a report holds besides the mission's status (rbp_report of include/rbp.h)
struct Result {
    double min_safety_ratio, total_flight_distance, end_time;
    int32_t samples, min_sample, min_qi, min_qj;
};
// a report of which nothing has been computed yet: no pair, no sample, no distance
REPORT_RULE Result empty_result(double end_time, int32_t samples) {
    return Result{RBP_REPORT_NO_RATIO, 0.0, end_time, samples, -1, -1, -1};
}

// position of agent qi at sample time t, whose count of segments begun is `before`
REPORT_RULE void agent_position(const double* coef, int32_t M, const double* T, double ts, int32_t qi, double t, int32_t before, double* p) {
    const int32_t m = segment_index(before);
    const double tseg = segment_time(T, ts, t, before);
    for (int k = 0; k < 3; ++k) p[k] = position(coef_of(coef, M, qi, k, m), tseg);
}

// The whole report, one sample after the other: the loop of the host entry, and the meaning of every shortcut the device takes.
// T [M+1] unscaled, coef [N][3][6M], radius [N]; scratch: 7 N doubles (this and the previous sample's positions, the agents' sums).
REPORT_RULE Result report_sequential(int32_t N, int32_t M, const double* T, double ts, const double* coef, const double* radius,
                                     double downwash, double dt, double* scratch) {
    const double end_time = scaled_time(T[M], ts);
    const int32_t samples = sample_count(end_time, dt);
    Result r = empty_result(end_time, samples);
    if (samples < 0) return r;
    double *pos = scratch, *prev = scratch + 3 * (int64_t)N, *len = scratch + 6 * (int64_t)N;
    for (int32_t qi = 0; qi < N; ++qi) len[qi] = 0.0;
    Minimum best = no_minimum();
    int32_t before = 0;
    for (int32_t j = 0; j < samples; ++j) {
        const double t = sample_time(j, dt);
        before = segments_before(T, M, ts, t, before);
        for (int32_t qi = 0; qi < N; ++qi) agent_position(coef, M, T, ts, qi, t, before, pos + 3 * (int64_t)qi);
        for (int32_t qi = 0; qi < N; ++qi)
            for (int32_t qj = qi + 1; qj < N; ++qj)
                take(&best, Minimum{safety_ratio(pos + 3 * (int64_t)qi, pos + 3 * (int64_t)qj, downwash, radius[qi] + radius[qj]), j, qi, qj});
        if (j > 0)
            for (int32_t qi = 0; qi < N; ++qi) len[qi] = len[qi] + step_length(prev + 3 * (int64_t)qi, pos + 3 * (int64_t)qi);
        double* swap = pos;
        pos = prev, prev = swap;
    }
    double total = 0.0;
    for (int32_t qi = 0; qi < N; ++qi) total = total + len[qi];
    r.min_safety_ratio = best.ratio, r.min_sample = best.sample, r.min_qi = best.qi, r.min_qj = best.qj;
    r.total_flight_distance = total;
    return r;
}

}  // namespace report_rules
