"""The test of the test: tests/synth_traj.py's cases keep their promises, and the C oracle -- run with plan/sequential = true,
batch_iter = 0, the QP-free path -- agrees with the exact reference.  CPU only; test_gpu_traj_synthetic.py runs the same cases through
kernels/traj.hip.

Conditions on the cases (asserted here, enforced by the generator, no case left out):
  (a) every comparison of every 1.1 ladder is at least relative 1e-9 away from its limit
  (b) every region of limits is hit at least twice, for velocity and for acceleration: inside the hull shortcut, between the shortcut and
      the peak, below the peak by 1, 2, 4 and >= 8 rungs
  (c) at least four cases whose acceleration-limited factor > 1 is a single value, at least two with a set of two values
  (d) under rule 1 the C oracle and the numpy restatement agree (on the exact coefficients and on the oracle's own)
"""
from collections import Counter

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import synth_traj as ST

ALL = [(N, idx) for N in ST.NS for idx in range(ST.K_CASES)]


def test_shapes_times_and_waypoints_cover_what_they_claim():
    cs = [ST.case(N, idx) for N, idx in ALL]
    assert len(cs) == 36 and {(1, 2), (3, 5), (7, 23)} <= {(c.N, c.M) for c in cs}
    assert max(c.N for c in cs) <= 7 and max(c.M for c in cs) <= 23 and min(c.M for c in cs) == 2
    for N in ST.NS:
        assert len({c.M for c in ST.cases(N)}) > 1   # every session is ragged
    dts = [np.diff(c.T) for c in cs]
    for dt in (1.0, 0.5, 1.7, 0.125):
        assert sum(1 for d in dts if np.allclose(d, dt, rtol=1e-12, atol=0)) >= 3
    assert sum(1 for d in dts if not np.allclose(d, d[0], rtol=1e-12, atol=0) and d.min() >= 0.3 and d.max() <= 2.5) >= 12
    assert any(np.any(np.isclose(d[1:] / d[:-1], 8.0)) for d in dts)
    delta = [np.diff(c.init_traj.astype(np.float64), axis=1) for c in cs]
    assert sum(int(np.sum(np.all(d == 0, axis=2))) for d in delta) >= 20       # hovering: the all-zero polynomial
    assert sum(int(np.sum(np.sum(d != 0, axis=2) == 1)) for d in delta) >= 50  # one axis at a time
    assert sum(int(np.sum(np.sum(d != 0, axis=2) >= 2)) for d in delta) >= 50  # diagonal
    assert max(float(np.abs(d).max()) for d in delta) <= 1.5 + 1e-6
    assert sum(1 for c in cs if np.abs(c.init_traj[:, :, 0]).min() >= 48.0) == 3   # agents near |x| = 50
    for c in cs:
        assert len(set(c.max_vel.reshape(-1)) | set(c.max_acc.reshape(-1))) == 6 * c.N, c.name   # every limit its own
        assert np.array_equal(ST.dummy_ctrl(c.init_traj), O.build_dummy(c.init_traj)), c.name


def test_conditions_a_to_d():
    hits, single, double = Counter(), 0, 0
    deciders = {N: [] for N in ST.NS}
    for N, idx in ALL:
        c = ST.case(N, idx)
        ts = c.ts
        assert ts["margin"] >= ST.MARGIN, (c.name, ts["margin"])                                   # (a)
        for name, region, rungs in c.ref.regions(c.max_vel, c.max_acc):                             # (b)
            hits[name, region if region != "below" else ("below", min(rungs, 8))] += 1
        if ts["decider"] is not None and ts["decider"][0] == "acc":                                 # (c)
            assert min(ts["sets"][0]) > 1.0
            single += len(ts["sets"][0]) == 1
            double += len(ts["sets"][0]) == 2
        oc = ST.oracle_coef(c)                                                                      # (d)
        assert len(ts["vel1"]) == 1 and ST.oracle_rule1_velocity(c, oc, c.max_vel) == ts["vel1"][0], c.name
        assert ts["sets"][1] is not None
        if ts["decider"] is not None:
            deciders[N].append(ts["decider"][1:3])
    print(f"\nregions hit: {dict(hits)}; acceleration-limited cases: {single} single-valued, {double} two-valued")
    for name in ("vel", "acc"):
        for region in ("hull", "between", ("below", 1), ("below", 2), ("below", 4), ("below", 8)):
            assert hits[name, region] >= 2, (name, region, hits)
    assert single >= 4 and double >= 2
    for N in (3, 7):   # the deciding (agent, axis) moves from case to case
        assert all(a != b for a, b in zip(deciders[N], deciders[N][1:])), deciders[N]
        assert len({d[0] for d in deciders[N]}) >= 3 and len({d[1] for d in deciders[N]}) == 3


def test_exchanging_the_deciding_limit_changes_the_factor():
    """the index max_vel[(mission * N + qi) * 3 + k]: with the deciding limit exchanged with ANY other entry of its array the expected set
    is another one, so a kernel that swaps agents or axes cannot pass"""
    n = 0
    for N, idx in ALL:
        c = ST.case(N, idx)
        if c.ts["decider"] is None:
            continue
        assert ST.swaps_change_the_factor(c) is True, c.name
        n += 1
    assert n == 30


@pytest.mark.parametrize("rule", [0, 1])
def test_oracle_agrees_with_the_exact_reference(rule):
    """oracle_planner_update on the QP-free path: ctrl bit for bit, coef within the counted bound, time_scale inside the admissible set"""
    worst = {True: 0.0, False: 0.0}
    for N, idx in ALL:
        c = ST.case(N, idx)
        rc, cor = ST.corridor(N, idx)
        assert rc == 0
        pl = cor.clone()
        rc, rep = O.planner_update(c.mission(), ST.make_param(N, rule), pl)
        assert rc == 0 and rep["n_qp"] == 0
        r = ST.check_plan(c, pl, rule, f"{c.name} rule {rule}")
        worst[pl.time_scale == 1.0] = max(worst[pl.time_scale == 1.0], r)
    print(f"\noracle, rule {rule}: worst coefficient error {worst[True]:.2f} (factor 1, bound {ST.B_UNSCALED}) / {worst[False]:.2f} "
          f"(rescaled, bound {ST.B_SCALED}) units of 2^-53 S_k")


def test_oracle_with_time_scale_off():
    worst = 0.0
    for N, idx in ALL:
        c = ST.case(N, idx)
        pl = ST.corridor(N, idx)[1].clone()
        assert O.planner_update(c.mission(), ST.make_param(N, 0, time_scale=False), pl)[0] == 0
        worst = max(worst, ST.check_plan(c, pl, 0, c.name, time_scale_on=False))
    print(f"\noracle, time_scale off: worst coefficient error {worst:.2f} units of 2^-53 S_k (bound {ST.B_UNSCALED})")


def test_the_reference_notices_a_wrong_exponent_and_a_wrong_time():
    """the exact coefficients against deliberately wrong ones: pow(inv, 4 - c) and a neighbour's dt break the bound by orders of magnitude"""
    c = ST.case(3, 6)
    good = ST.oracle_coef(c)
    assert c.ref.coef_bound_ratio(good, 1.0) <= ST.B_UNSCALED
    dts = np.repeat(np.diff(c.T), 6)
    wrong_exp = good * dts          # one power of inv short
    assert c.ref.coef_bound_ratio(wrong_exp, 1.0) > 1e6
    T2 = c.T.copy()
    T2[1:-1] = 0.5 * (T2[:-2] + T2[2:]) + 0.01   # other segment times
    assert c.ref.coef_bound_ratio(O.ctrl_to_coef(T2, c.ref.ctrl), 1.0) > 1e6
