"""The trajectory kernels (kernels/traj.hip: dummy_kernel, coef_kernel, timescale_kernel) and rbp_session_download's scaling against an
EXACT reference (tests/synth_traj.py), on non-unit segment times and limits of their own per (agent, axis).  Needs an MI355X.

plan/sequential = true with batch_iter = 0 solves no QP: launch_planner_prologue writes the `dummy` control points and
launch_planner_epilogue runs on exactly those, so nothing stands between the chosen init_traj / T / limits and the three kernels.
Every other GPU test feeds them T[i] = i, the mission file's limits (the same on every axis) and, in ragged sessions, only a QP's answer.

What is compared, per case (synth_traj.check_plan):
  ctrl                          bit for bit; qp_solves == 0
  time_scale, time_scale_alt    inside the admissible set of their rule (a `dummy` segment's |acceleration| has two exactly equal
                                peaks; which one the ladder climbs through hangs on the last bit -- synth_traj's docstring)
  T, sfc_time, rsfc_time        the uploaded / the oracle corridor's values times time_scale, one IEEE product each: ==
  coef                          |coef - c_k ts^-(5-k)| <= B 2^-53 S_k ts^-(5-k) against the Fraction coefficients, B = 16 where ts == 1
                                and 22 otherwise: the count of operations stands in check_plan's docstring

  test_ragged_session[N-rule]        12 cases of N agents, each with its own M, in one session
  test_solo_sessions...              the same cases alone: slot strides MS / PS against M / P
  test_second_run...                 only coef is rescaled on the device: a second run without reset gives the same bits
  test_failed_corridor_in_company    the status != 0 exits of coef_kernel and timescale_kernel
  test_time_scale_off                rbp_param.time_scale = 0
  test_joint_schedule_iteration_zero plan/sequential = false with iteration = 0: the other QP-free route (abi/session.hip)
"""
import functools

import numpy as np
import pytest

from swarm_simulator_amd import planner
from tests import synth_traj as ST

pytestmark = pytest.mark.gpu

ARRAYS = ("ctrl", "coef", "T", "sfc_count", "sfc_box", "sfc_time", "rsfc_time")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def session(cs, param, opts=None):
    plans = [c.plan() for c in cs]
    return planner.Session([c.world for c in cs], [c.mission() for c in cs], param, plans, opts=opts), plans


def run(cs, param, opts=None):
    """one session over the cases, corridor and planner: (statuses, plans)"""
    s, plans = session(cs, param, opts)
    s.run()
    st = s.download()
    s.close()
    return st, plans


@functools.lru_cache(maxsize=None)
def ragged(N, rule):
    """the ragged session of all N-agent cases under a rule (run once per process, never written to)"""
    return run(ST.cases(N), ST.make_param(N, rule))


def assert_same_bits(a, b, tag):
    for name in ARRAYS:
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), (tag, name)
    assert a.time_scale == b.time_scale and a.time_scale_alt == b.time_scale_alt, tag
    assert np.array_equal(bits(a.rsfc_normal), bits(b.rsfc_normal)), tag


def check_all(cs, plans, rule, tag, time_scale_on=True):
    worst = {True: 0.0, False: 0.0}
    for c, pl in zip(cs, plans):
        assert pl.qp_solves == 0 and pl.qp_iterations == 0, c.name
        r = ST.check_plan(c, pl, rule, f"{c.name} {tag}", time_scale_on)
        worst[pl.time_scale == 1.0] = max(worst[pl.time_scale == 1.0], r)
    print(f"\n{tag}: worst coefficient error {worst[True]:.2f} (factor 1, bound {ST.B_UNSCALED}) / {worst[False]:.2f} (rescaled, bound "
          f"{ST.B_SCALED}) units of 2^-53 S_k; factors {[pl.time_scale for pl in plans]}")


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("N", ST.NS)
def test_ragged_session(N, rule):
    cs = ST.cases(N)
    assert len({c.M for c in cs}) > 1
    st, plans = ragged(N, rule)
    assert st == [0] * len(cs)
    check_all(cs, plans, rule, f"N={N} rule {rule}")
    for c, pl in zip(cs, plans):   # where both sets are single values, the two factors are exactly those
        s0, s1 = c.ts["sets"][rule], c.ts["sets"][1 - rule]
        if len(s0) == 1 and len(s1) == 1:
            assert (pl.time_scale, pl.time_scale_alt) == (s0[0], s1[0]), c.name


@pytest.mark.parametrize("N", ST.NS)
def test_solo_sessions_give_the_bits_of_the_ragged_session(N):
    """one mission per session: the slot strides are the mission's own M and P there, the session's maxima in the ragged one"""
    cs = ST.cases(N)
    st, plans = ragged(N, 0)
    assert st == [0] * len(cs)
    for c, pl in zip(cs, plans):
        st1, solo = run([c], ST.make_param(N, 0))
        assert st1 == [0], c.name
        assert_same_bits(solo[0], pl, c.name)


@pytest.mark.parametrize("N", ST.NS)
def test_second_run_without_reset_is_bit_identical(N):
    """timescale_kernel rescales only coef, which coef_kernel writes anew; T and the corridor times stay as uploaded on the device"""
    cs = ST.cases(N)
    s, plans = session(cs, ST.make_param(N, 0))
    s.run()
    assert s.download() == [0] * len(cs)
    first = [pl.clone() for pl in plans]
    for f, pl in zip(first, plans):
        f.time_scale_alt = pl.time_scale_alt
    s.run()
    assert s.download() == [0] * len(cs)
    s.close()
    assert any(pl.time_scale != 1.0 for pl in plans)
    for c, f, pl, r in zip(cs, first, plans, ragged(N, 0)[1]):
        assert_same_bits(f, pl, c.name + " (second run)")
        assert_same_bits(r, pl, c.name + " (vs the ragged session)")


@pytest.mark.parametrize("N", [3, 7])
def test_failed_corridor_in_company(N):
    """a mission whose first waypoint lies in an obstacle fails its corridor stage: status != 0, and the epilogue leaves it alone while
    the others get the bits they had without it"""
    cs = ST.cases(N)
    bad = ST.blocked(cs[6])   # (the longest mission of the 7-agent session)
    from tests import oracle_lib as O
    from swarm_simulator_amd import _abi as A
    assert O.corridor_update(bad.world, bad.mission(), ST.make_param(N), bad.plan())[0] == A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ
    mixed = cs[:4] + [bad] + cs[4:]
    st, plans = run(mixed, ST.make_param(N, 0))
    assert st == [0] * 4 + [A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ] + [0] * (len(cs) - 4)
    assert not np.any(plans[4].coef)   # never written
    for c, pl, r in zip(cs, plans[:4] + plans[5:], ragged(N, 0)[1]):
        assert_same_bits(r, pl, c.name)


@pytest.mark.parametrize("N", ST.NS)
def test_time_scale_off(N):
    """rbp_param.time_scale = 0: factor 1, alt 1, the unscaled coefficients within B = 16, whatever the limits"""
    cs = ST.cases(N)
    st, plans = run(cs, ST.make_param(N, 0, time_scale=False))
    assert st == [0] * len(cs)
    check_all(cs, plans, 0, f"N={N} time_scale off", time_scale_on=False)


@pytest.mark.parametrize("min_agents", [16, 2])
def test_joint_schedule_iteration_zero(min_agents):
    """plan/sequential = false with iteration = 0: rbp_session_run skips the QP of the one-workgroup path (min_agents 16: N = 3 stays
    below it) and of the grid-wide joint solver (joint_wide_min_agents = 2) alike, and the epilogue runs on the prologue's control
    points.  (The oracle, like the reference, builds `dummy` only for the sequential schedule and publishes zeros here, so this route has
    no CPU twin: the exact reference judges it.)"""
    cs = ST.cases(3)
    st, plans = run(cs, ST.make_param(3, 0, sequential=False, iteration=0), planner.solver_opts(joint_wide_min_agents=min_agents))
    assert st == [0] * len(cs)
    check_all(cs, plans, 0, f"joint schedule, iteration 0, joint_wide_min_agents {min_agents}")
    for c, pl, r in zip(cs, plans, ragged(3, 0)[1]):
        assert_same_bits(r, pl, c.name)
