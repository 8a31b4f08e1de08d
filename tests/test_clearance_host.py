"""rbp_clearance_host (host/validate.cpp over csrc/common/clearance_rules.h) against the pure Python restatement of tests/synth_clearance.py,
field for field and AS BITS, agent_clearance included: seeded synthetic plans (tests/synth_report.py) on seeded grids of different
resolution, shape and key_min -- grids the plans stay inside, grids they leave on every side, the smallest grid 3 x 2 x 1 -- with scaled
times and sample steps on and off the knots; then the golden small cases on their own worlds.

What the host function reports of the golden plans (tests/common.SMALL_CASES, each on the world of its case, dt = 0.1), on the CPU:
hits == 0 and outside == 0 for every one of them, which test_the_golden_plans_hit_nothing asserts.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host
from tests import synth_clearance as L
from tests import synth_report as S
from tests.common import SMALL_CASES, Case

# (seed, N, Ms, times, time scales, dt, grid shape, key_min, res): synthetic agents rest near (a % side, a // side, 0.5 .. 2) and wander a few decimetres
CASES = [
    (1, 2, [1], "unit", None, 0.1, (40, 40, 30), (-10, -10, 0), 0.1),                  # inside throughout
    (2, 3, [2], "nonunit", None, 0.25, (9, 7, 5), (-2, -1, 1), 0.25),                  # leaves a small non-cubic grid
    (3, 4, [3, 1], "alternating", [1.1, 1.4641], 0.07, (16, 12, 10), (-3, -2, 0), 0.2),  # two missions, scaled times, off the knots
    (4, 6, [2], "unit", [1.4641], 0.1, (3, 2, 1), (0, 0, 5), 0.3),                      # the smallest grid: nearly everything outside
    (5, 1, [2], "unit", None, 0.1, (30, 30, 30), (-15, -15, -5), 0.1),
    (6, 9, [5], "nonunit", None, 0.1, (25, 31, 12), (-1, -4, 2), 0.125),
]
IDS = ["N2_inside", "N3_small_grid_dt025", "N4_two_missions_ts_dt007", "N6_grid_3x2x1", "N1", "N9_M5_res0125"]


def same(rec, ref):
    assert rec.bits() == ref.bits(), (rec, ref)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_host_entry_equals_the_python_restatement_as_bits(case):
    seed, N, Ms, kind, ts, dt, shape, key_min, res = case
    plans = S.make(seed, N, Ms, kind, ts)
    worlds = [L.grid(seed + k, shape, key_min, res) for k in range(plans.K)]
    got, got_agents = L.host_clearances(plans, worlds, dt)
    ref, ref_agents = L.restate_plans(plans, worlds, dt)
    for g, r in zip(got, ref):
        same(g, r)
        assert g.samples > 0 and g.status == 0
    assert np.array_equal(got_agents.view(np.uint64), ref_agents.view(np.uint64))
    assert all(g.min_clearance == got_agents[k].min() and got_agents[k, g.min_agent] == g.min_clearance for k, g in enumerate(got))


def test_the_cases_cover_inside_outside_and_hits():
    seen = {}
    for seed, N, Ms, kind, ts, dt, shape, key_min, res in CASES:
        plans = S.make(seed, N, Ms, kind, ts)
        recs, _ = L.host_clearances(plans, [L.grid(seed + k, shape, key_min, res) for k in range(plans.K)], dt)
        seen[seed] = [(r.outside, r.hits, r.samples * N) for r in recs]
    assert seen[1] == [(0, 0, 20)]                                                    # inside throughout, clear of every obstacle
    assert all(o == 0 and 0 < h < n for o, h, n in seen[3] + seen[5])                 # inside throughout, hits
    assert all(0 < o < h < n for o, h, n in seen[2] + seen[6])                        # partly outside, and hits inside too
    assert all(h >= o for v in seen.values() for o, h, n in v)                        # an outside is a hit (radius 0.15 > -1 + 1e-6)
    assert seen[4][0][0] > seen[4][0][2] // 2                                         # the smallest grid: mostly outside


def test_host_python_wrapper_and_per_agent():
    plans = S.make(7, 5, [3])
    w = L.grid(7, (40, 40, 30), (-10, -10, 0), 0.1)
    rec, agents = host.clearance(w, plans.mission(0), plans.plan(0), 0.1, per_agent=True)
    ref, ref_agents = L.restate(plans.scaled_T(0), plans.coefs[0], plans.radius[0], w, 0.1)
    same(rec, ref)
    assert np.array_equal(agents.view(np.uint64), ref_agents.view(np.uint64))
    same(host.clearance(w, plans.mission(0), plans.plan(0), 0.1), ref)


def test_no_sample_too_many_samples_and_a_nan_radius():
    plans = S.make(8, 3, [1])
    w = L.grid(8, (40, 40, 30), (-10, -10, 0), 0.1)
    plans.T[0, 1] = 0.05
    (rec,), agents = L.host_clearances(plans, [w], 0.1)
    assert rec.bits() == L.restate(plans.scaled_T(0), plans.coefs[0], plans.radius[0], w, 0.1)[0].bits()
    assert (rec.min_clearance, rec.min_dist, rec.samples, rec.min_sample, rec.min_agent, rec.hits, rec.outside) == (1e9, 0.0, 0, -1, -1, 0, 0)
    assert np.all(agents == 1e9)
    plans.T[0, 1] = 2000.0
    (rec,), agents = L.host_clearances(plans, [w], 1e-3)
    assert (rec.min_clearance, rec.samples, rec.min_sample, rec.min_agent, rec.end_time) == (1e9, -1, -1, -1, 2000.0) and np.all(agents == -7.0)
    plans.T[0, 1] = 1.0
    plans.radius[0, :] = np.nan
    (rec,), agents = L.host_clearances(plans, [w], 0.1)
    assert (rec.min_clearance, rec.min_sample, rec.min_agent, rec.hits, rec.samples) == (1e9, -1, -1, 0, 10) and np.all(agents == 1e9)


def test_bad_arguments():
    plans = S.make(9, 2, [1])
    w = L.grid(9, (4, 4, 4), (0, 0, 0), 0.5)
    mission, plan = plans.mission(0), plans.plan(0)
    out = A.rbp_clearance()
    P = lambda a: A.ptr(a, A.c_double_p)
    f = host.lib().rbp_clearance_host

    def call(ws=None, ms=None, M=plan.M, T=P(plan.T), coef=P(plan.coef), dt=0.1, o=C.byref(out)):
        ws = w.c_struct() if ws is None else ws
        ms = mission.c_struct() if ms is None else ms
        return f(C.byref(ws), C.byref(ms), M, T, coef, dt, o, None)
    assert call() == 0
    bad_res, bad_dim, no_grid, no_radius = w.c_struct(), w.c_struct(), w.c_struct(), mission.c_struct()
    bad_res.res, bad_dim.dim[1], no_grid.dist, no_radius.radius = 0.0, 0, None, None
    for kw in (dict(ws=bad_res), dict(ws=bad_dim), dict(ws=no_grid), dict(ms=no_radius), dict(M=0), dict(T=None), dict(coef=None), dict(dt=0.0), dict(dt=float("nan")),
               dict(o=None)):
        assert call(**kw) == A.RBP_ERR_BAD_ARGUMENT, kw
    assert f(None, None, 1, None, None, 0.1, None, None) == A.RBP_ERR_BAD_ARGUMENT


def golden_plan(c):
    pr = c.inputs()
    pr.coef[:], pr.T[:] = c.g["coef"], c.g["T"]
    return pr


@pytest.mark.parametrize("name", SMALL_CASES)
def test_a_golden_plan_on_its_world_equals_the_restatement(name):
    c = Case(name)
    pr = golden_plan(c)
    rec, agents = host.clearance(c.world, c.mission, pr, 0.1, per_agent=True)
    ref, ref_agents = L.restate(pr.T, pr.coef, c.mission.radius, c.world, 0.1)
    same(rec, ref)
    assert np.array_equal(agents.view(np.uint64), ref_agents.view(np.uint64)) and rec.samples > 0
    print(f"{name}: minimum clearance {rec.min_clearance!r} (agent {rec.min_agent}, sample {rec.min_sample}), hits {rec.hits}, outside {rec.outside}")


def test_the_golden_plans_hit_nothing():
    """(the module docstring: what the host function reports of the golden plans)"""
    for name in SMALL_CASES:
        c = Case(name)
        rec = host.clearance(c.world, c.mission, golden_plan(c), 0.1)
        assert (rec.hits, rec.outside) == (0, 0), (name, rec)
