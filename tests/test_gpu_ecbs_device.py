"""The ECBS search on the GPU (kernels/ecbs.hip; rbp_dev_ecbs_plan_masks, rbp_dev_worlds_ecbs_plan) against the host library's search
(csrc/host/ecbs.cpp), whose bits it returns: the initial trajectories as uint32, T, M, makespan, sum_cost and BOTH expansion counters --
the counters are what catches a search that drifts and still ends valid.  The synthetic cases are tests/synth_ecbs.py's."""
import functools

import numpy as np
import pytest

from swarm_simulator_amd import host, planner, sweep_device
from swarm_simulator_amd.types import Param
from tests import synth_ecbs as S

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_is_the_hosts(got, ref):
    assert got is not None
    assert got.M == ref.M and got.init_traj.shape == ref.init_traj.shape
    assert np.array_equal(bits(got.init_traj), bits(ref.init_traj)) and np.array_equal(got.T, ref.T)
    assert got.ecbs_stats == ref.ecbs_stats   # makespan, sum_cost, high_level, low_level


@functools.lru_cache(maxsize=None)
def synthetic():
    """every synthetic case with the host's answer (computed once), and the device's: one call per distinct (N, w)"""
    cases = [S.case(name, r, w) for name, r, w, *_ in S.CASES]
    refs = [S.host_plan(mask, m, p) for mask, m, p in cases]
    got = [None] * len(cases)
    status = np.zeros(len(cases), np.int32)
    groups = {}
    for i, (mask, m, p) in enumerate(cases):
        groups.setdefault((m.qn, p.ecbs_w), []).append(i)
    for idx in groups.values():
        plans = planner.ecbs_plan_masks([cases[i][0] for i in idx], [cases[i][1] for i in idx], cases[idx[0]][2], max_nodes=S.BUDGET, max_M=S.MAX_M)
        for i, pr, st in zip(idx, plans, plans.status):
            got[i], status[i] = pr, st
    return refs, got, status


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=[f"{c[0]}-r{c[1]}-w{c[2]}" for c in S.CASES])
def test_synthetic_cases_are_the_hosts_bit_for_bit(i):
    refs, got, status = synthetic()
    print("status", status[i], "host", refs[i].ecbs_stats, "device", got[i] and got[i].ecbs_stats)
    assert status[i] == 0
    assert_is_the_hosts(got[i], refs[i])


def test_host_failure_codes():
    """a wall with one hole and budget 4: the host gives up (2); a start on a blocked cell: 1 -- and a good mission beside them is unaffected"""
    mask, m, p = S.case("gap1", 0.35, 1.5)
    with pytest.raises(RuntimeError, match="ECBS Failed"):
        S.host_plan(mask, m, p, 4)
    good_mask, good_m, _ = S.case("gap2", 0.15, 1.5)
    blocked = mask.copy()
    blocked[6, 11, 0] = 1   # the start (-2, 0.5, 1) of agent 0
    with pytest.raises(RuntimeError, match="occluded"):
        S.host_plan(blocked, m, p, 4)
    plans = planner.ecbs_plan_masks([mask, good_mask, blocked], [m, good_m, m], p, max_nodes=4, max_M=S.MAX_M)
    assert list(plans.status) == [2, 0, 1]
    assert plans[0] is None and plans[2] is None
    assert_is_the_hosts(plans[1], S.host_plan(good_mask, good_m, p, 4))


def test_a_device_capacity_is_status_3_and_leaves_the_other_missions_alone():
    mask, m, p = S.case("circle8", 0.10, 1.0)
    ref = S.host_plan(mask, m, p)
    assert ref.M > 8
    # one call cannot mix capacities, so the unaffected neighbours are missions whose paths fit: a mission of 8 agents that needs 3 steps
    s = np.array([(x, y) for x in (-4.0, -3.0) for y in (-4.0, -3.0, -2.0, -1.0)])
    short = S.mission(s, s + (1.5, 0.0), 0.10)
    ref_short = S.host_plan(mask, short, p)
    assert ref_short.M <= 8
    mixed = planner.ecbs_plan_masks([mask] * 3, [short, m, short], p, max_nodes=S.BUDGET, max_M=8)
    assert list(mixed.status) == [0, 3, 0] and mixed[1] is None
    o = mixed.out   # a mission without a result has zeros everywhere
    assert not o.init_traj[1].any() and not o.T[1].any() and (o.M[1], o.makespan[1], o.sum_cost[1], o.high_level[1], o.low_level[1]) == (0, 0, 0, 0, 0)
    assert_is_the_hosts(mixed[0], ref_short)
    assert_is_the_hosts(mixed[2], ref_short)


MAPS8 = ["map5.bt", "map3.bt", "empty.bt"]
MAPS16 = ["map3.bt", "map6.bt"]


@functools.lru_cache(maxsize=None)
def host_world(name):
    keys, res, _ = host.load_octomap(name)
    return host.build_world(keys, res, Param.test_sweep())


def device_worlds(names):
    trees = [host.load_octomap(n) for n in names]
    return planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], Param.test_sweep())


@pytest.mark.parametrize("names,mission", [(MAPS8, "mission_8agents_15.json"), (MAPS16, "mission_16agents_15.json"), (["map1.bt"], "mission_64agents_15.json")],
                         ids=["8agents", "16agents", "64agents"])
def test_resident_worlds_are_searched_like_the_host_worlds(names, mission):
    p, m = Param.test_sweep(), host.load_mission(mission)
    ws = device_worlds(names)
    try:
        plans = planner.ecbs_plan_batch(ws, list(range(len(names))), [m] * len(names), p, max_nodes=S.BUDGET, max_M=S.MAX_M)
    finally:
        ws.close()
    assert list(plans.status) == [0] * len(names)
    for name, got in zip(names, plans):
        ref = host.ecbs_plan(host_world(name), m, p, S.BUDGET)
        print(name, ref.ecbs_stats)
        assert_is_the_hosts(got, ref)


def test_a_planning_lattice_outside_the_resident_grid_is_status_1_and_world_indices_are_checked():
    m = host.load_mission("mission_8agents_15.json")
    wide = Param.test_sweep(world_x_min=-8.0, world_x_max=8.0)   # lattice samples beyond the grid, which is built for +-5
    ws = device_worlds(["empty.bt"])
    try:
        plans = planner.ecbs_plan_batch(ws, [0], [m], wide, max_nodes=S.BUDGET, max_M=S.MAX_M)
        assert list(plans.status) == [1] and plans[0] is None
        with pytest.raises(ValueError, match="world index out of range"):
            planner.ecbs_plan_batch(ws, [1], [m], wide, max_nodes=S.BUDGET, max_M=S.MAX_M)
        with pytest.raises(ValueError, match="world index out of range"):
            planner.ecbs_plan_batch(ws, [-1], [m], wide, max_nodes=S.BUDGET, max_M=S.MAX_M)
    finally:
        ws.close()


def test_forty_copies_in_one_call_are_forty_times_the_single_answer():
    mask, m, p = S.case("cross4", 0.15, 1.0)
    one = planner.ecbs_plan_masks([mask], [m], p, max_nodes=S.BUDGET, max_M=S.MAX_M)
    assert list(one.status) == [0]
    assert_is_the_hosts(one[0], S.host_plan(mask, m, p))
    plans = planner.ecbs_plan_masks([mask] * 40, [m] * 40, p, max_nodes=S.BUDGET, max_M=S.MAX_M)
    assert list(plans.status) == [0] * 40
    for pr in plans:
        assert_is_the_hosts(pr, one[0])


def test_a_wave_that_takes_several_missions_starts_each_from_clean_workspace():
    """the grid is four waves per CU, 1024 on the MI355X: 1100 missions make waves take a second one, alternately on two masks -- stale node
    pools, paths and seen bits of the mission before would show in the counters"""
    mask, m, p = S.case("cross4", 0.15, 1.1)
    other_mask, other_m, _ = S.case("gap2", 0.15, 1.1)
    refs = [S.host_plan(mask, m, p), S.host_plan(other_mask, other_m, p)]
    K = 1100
    plans = planner.ecbs_plan_masks([(mask, other_mask)[k % 2] for k in range(K)], [(m, other_m)[k % 2] for k in range(K)], p, max_nodes=S.BUDGET,
                                    max_M=S.MAX_M)
    assert not plans.status.any()
    for k in range(K):
        assert_is_the_hosts(plans[k], refs[k % 2])


def test_sweep_device_reports_the_same_with_the_device_search(capsys):
    argv = ["--device-worlds", "--maps", "5", "--mode", "batched", "--mission", "mission_8agents_15.json"]
    lines = []
    for extra in ([], ["--device-ecbs"]):
        assert sweep_device.main(argv[:1] + extra + argv[1:]) == 0
        out = capsys.readouterr().out
        lines.append([l for l in out.splitlines() if l.startswith("map5:")])
        assert ("in one device search" in out) == bool(extra)
    assert len(lines[0]) == 1 and lines[0] == lines[1]
