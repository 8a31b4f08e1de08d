"""rbp_limits_host (host/limits.cpp over csrc/common/limits_rules.h) against tests/synth_limits.py:
  * field for field and AS BITS, agent_upper included, against the pure Python restatement in floats: seeded synthetic plans
    (tests/synth_report.py) with seeded per-axis limits on both sides of the plans' derivatives, N in {1, 3}, M in {1, 2, 5}, depth in
    {0, 1, 4, 8}, refine_above that refines everything, nothing and a part, scaled times; NaN and infinite coefficients, a NaN limit;
  * containment in fractions.Fraction, on segments of 0.5, 1.7 and 4 s (times a scale of 1.21), coefficients up to 1e3: every computed
    control point of every piece lies within err of the exact one -- which is what pins the constant 16 + 4 D --, the exact hull
    max |b_k| is >= |X(t)| at rational points of the piece, and so lower * limit <= an exact value on the piece <= upper * limit;
  * the peak the samples miss; the shapes tests/test_gpu_limits.py runs, whose partial refine_above must leave both kinds of item in the
    first wavefront; bad arguments.
CPU only."""
import ctypes as C
from fractions import Fraction as F

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host
from tests import synth_limits as X
from tests import synth_report as S


def same(rec, ref):
    assert rec.bits() == ref.bits(), (rec, ref)


def test_the_counted_constant_is_within_the_rule_s():
    assert [X.counted_constant(d) for d in (0, 1, 4, 8)] == [14, 18, 30, 46]
    assert all(X.counted_constant(d, 3) <= X.counted_constant(d) <= X.rule_constant(d) <= X.counted_constant(d) + 4 for d in range(9))


CASES = [(1, 1, "unit", 1.0), (1, 5, "nonunit", 1.21), (3, 2, "alternating", 1.0), (3, 1, "nonunit", 1.7), (1, 2, "unit", 1.21), (3, 5, "nonunit", 1.0)]


# (depth 8 on the 15 items of the last case: a pass over 256 pieces of 90 polynomials in Python adds seconds and no path)
@pytest.mark.parametrize("refine", ["all", "none", "part"])
@pytest.mark.parametrize("N,M,kind,ts,depth", [c + (d,) for c in CASES for d in (0, 1, 4, 8) if not (d == 8 and c[0] * c[1] > 6)])
def test_the_host_entry_equals_the_restatement(N, M, kind, ts, depth, refine):
    plans = S.make(31 * N + M, N, [M], kind, [ts], spread=0.6)
    mv, ma = X.random_limits(5 * N + M, 1, N)
    mission = X.mission_of(plans, 0, mv, ma)
    coarse, upper0 = host.limits(mission, plans.plan(0), 0, 1e9, per_agent=True)
    above = {"all": -1.0, "none": 1e9, "part": float(np.median(upper0.max(axis=1)))}[refine]
    rec, agents = host.limits(mission, plans.plan(0), depth, above, per_agent=True)
    ref, ref_agents = X.restate(plans.scaled_T(0), plans.coefs[0], mv[0], ma[0], depth, above)
    same(rec, ref)
    assert np.array_equal(agents.view(np.uint64), ref_agents.view(np.uint64))
    assert rec.end_time == plans.scaled_T(0)[M] and rec.refined == {"all": N * M, "none": 0}.get(refine, rec.refined)
    assert 0 < rec.lower_vel_ratio <= rec.upper_vel_ratio < np.inf and 0 < rec.lower_acc_ratio <= rec.upper_acc_ratio < np.inf
    assert coarse.refined == 0 and coarse.lower_vel_ratio <= coarse.upper_vel_ratio
    assert rec.upper_vel_ratio == agents[:, 0].max() and rec.upper_acc_ratio == agents[:, 1].max()
    assert rec.violating <= rec.uncertified <= N * M


@pytest.mark.parametrize("what", ["nan coefficient", "infinite coefficient", "nan limit", "zero limit"])
def test_no_numbers_equal_the_restatement(what):
    plans = S.make(77, 3, [2], "nonunit", [1.21], spread=0.6)
    mv, ma = X.random_limits(9, 1, 3)
    if what == "nan coefficient":
        plans.coefs[0].reshape(3, 3, 12)[1, 2, 7] = np.nan
    elif what == "infinite coefficient":
        plans.coefs[0].reshape(3, 3, 12)[1, 2, 7] = -np.inf
    elif what == "nan limit":
        ma[0, 2, 1] = np.nan
    else:
        mv[0, 0, 0] = 0.0
    for depth, above in ((0, 1e9), (3, 1e9), (3, -1.0)):
        rec, agents = host.limits(X.mission_of(plans, 0, mv, ma), plans.plan(0), depth, above, per_agent=True)
        ref, ref_agents = X.restate(plans.scaled_T(0), plans.coefs[0], mv[0], ma[0], depth, above)
        same(rec, ref)
        assert np.array_equal(agents.view(np.uint64), ref_agents.view(np.uint64))
        assert rec.uncertified >= 1 and np.isinf(agents).any() and not np.isnan(agents).any()
        assert rec.refined >= 1   # (what is no number below 1e9 goes to `depth`)
        assert all(np.isfinite(getattr(rec, n)) or what == "infinite coefficient" for n in rec.FIELDS[:4])


def big_plans():
    """three agents, three segments of 0.5, 1.7 and 4 s, coefficients up to 1e3 (agent 2) and of ordinary size (agents 0 and 1)"""
    rng = np.random.default_rng(2024)
    T = np.array([0.0, 0.5, 2.2, 6.2])
    c = S.random_coefs(rng, 3, 3)
    c[2] = rng.uniform(-1e3, 1e3, (3, 18))
    c[1] *= rng.choice([1e-3, 1.0, 30.0], (3, 18))
    return T, c


@pytest.mark.parametrize("ts", [1.0, 1.21])
@pytest.mark.parametrize("depth", [0, 1, 4, 8])
def test_the_bounds_contain_the_exact_polynomial(depth, ts):
    T, c = big_plans()
    T = T * ts if ts != 1.0 else T
    only = list(range(1 << depth)) if depth < 8 else list(range(0, 256, 37)) + [255]
    u, checked, worst = F(1, 2 ** 53), 0, F(0)
    for a in range(3):
        for m in range(3):
            assert float(T[m + 1]) - float(T[m]) == pytest.approx((0.5, 1.7, 4.0)[m] * ts)
            for k in range(3):
                for kind in ("vel", "acc"):
                    computed, err = X.pieces(T, c[a][k], m, kind, depth)
                    exact, V = X.exact_pieces(T, c[a][k], m, kind, depth, only)
                    limit = 0.37 + 0.5 * k
                    for p, eb in zip(only, exact):
                        cb = computed[p]
                        for x, y in zip(cb, eb):
                            assert abs(F(x) - y) <= F(err), (a, m, k, kind, p)
                            worst = max(worst, abs(F(x) - y) / (u * V))
                        lower, upper = X._bounds(cb, err, limit)
                        hull, ends = max(abs(y) for y in eb), max(abs(eb[0]), abs(eb[-1]))
                        # the exact hull bounds the derivative at rational points of the piece (s: a fraction of the segment)
                        for j in range(8):
                            s = (F(p) + F(j, 7)) / (1 << depth)
                            assert abs(X.exact_value(T, c[a][k], m, kind, s)) <= hull
                        # ends is a value |X| takes on the piece, the hull bounds the supremum: lower <= ends <= sup <= hull <= upper
                        assert F(lower) * F(limit) <= ends <= hull <= F(upper) * F(limit), (a, m, k, kind, p)
                        # ... and not by much: twice err and the four doubles the ratios are moved
                        assert F(upper) * F(limit) - hull <= 2 * F(err) + 8 * u * (hull + V)
                        checked += 1
    assert checked == 27 * 2 * len(only)
    print(f"depth {depth} ts {ts}: the largest |computed - exact| of a control point is {float(worst):.2f} * 2^-53 * V; err is {X.rule_constant(depth)}")
    assert worst <= X.counted_constant(depth)


def test_the_peak_the_samples_miss():
    """v(t) = 4.8 t (1 - t) against max_vel = 1.17, sampled at dt = 0.4: no sample sees more than 1.152; the peak 1.2 lies at t = 0.5"""
    from swarm_simulator_amd.types import Param
    mission, plan = X.parabola()
    sampled = host.dynamics(mission, Param.test_sweep(), plan, 0.4)
    sampled = sampled[0] if isinstance(sampled, tuple) else sampled
    print(f"sampled peak {sampled.peak_vel_ratio!r} of {sampled.samples} samples")
    assert 0 < sampled.peak_vel_ratio < 1
    coarse = host.limits(mission, plan, 0, 1e9)
    print(f"depth 0: [{coarse.lower_vel_ratio!r}, {coarse.upper_vel_ratio!r}]")
    assert coarse.upper_vel_ratio >= coarse.lower_vel_ratio and coarse.uncertified == 1 and coarse.violating == 0
    for depth in range(1, 9):
        rec = host.limits(mission, plan, depth, 0.5)
        print(f"depth {depth}: [{rec.lower_vel_ratio!r}, {rec.upper_vel_ratio!r}]")
        assert rec.lower_vel_ratio > 1 and rec.upper_vel_ratio >= rec.lower_vel_ratio and rec.violating == 1 and rec.refined == 1
        same(rec, X.restate(plan.T, plan.coef, mission.max_vel, mission.max_acc, depth, 0.5)[0])


@pytest.mark.parametrize("name", sorted(X.GPU_SHAPES))
def test_the_partial_refinement_of_the_gpu_shapes_leaves_both_kinds_in_the_first_wavefront(name):
    """what tests/test_gpu_limits.py relies on for its partial-ballot case: 0 < refined < items, among the first 64 item slots too"""
    plans, mv, ma, above = X.gpu_case(name)
    if above is None:
        assert plans.N * plans.S == 1   # (one item cannot be of both kinds)
        return
    recs, _ = X.host_limits(plans, mv, ma, 4, above)
    for k, rec in enumerate(recs):
        items = plans.N * int(plans.M[k])
        assert (0 < rec.refined < items) or items == 1, (k, rec.refined, items)
    first = X.first_wave_refined(plans, mv, ma, above)
    assert 0 < sum(first) < len(first), first


def test_bad_arguments_are_refused():
    mission, plan = X.parabola()
    ms = mission.c_struct()
    out = A.rbp_limits()
    P = lambda a: A.ptr(a, A.c_double_p)
    f = host.lib().rbp_limits_host

    def call(depth=4, above=0.5, M=1, T=P(plan.T), coef=P(plan.coef), o=C.byref(out), m=C.byref(ms)):
        return f(m, M, T, coef, depth, above, o, None)
    assert call() == 0
    for kw in (dict(depth=-1), dict(depth=9), dict(above=float("nan")), dict(M=0), dict(T=None), dict(coef=None), dict(o=None), dict(m=None)):
        assert call(**kw) == A.RBP_ERR_BAD_ARGUMENT, kw
    assert call(depth=8) == 0 and call(depth=0) == 0 and call(above=-2.0) == 0 and call(above=1e9) == 0 and call(above=float("inf")) == 0
    with pytest.raises(ValueError):
        host.limits(mission, plan, depth=9)
    assert A.RBP_SIZEOF_LIMITS == 13 and C.sizeof(A.rbp_limits) == 152
