"""A session that outlives its missions (rbp_session_create_reserved, rbp_session_refill_from_ecbs, kernels/handoff.hip
session_refill_kernel; planner.Session.reserved / refill / capacity, sweep_device --stream).  The yardstick is the constructor: a
Session.from_ecbs of the same search, run once.  The rule under test is that after a refill and a run every output bit equals that fresh
session's -- whatever the slots held before: a longer or shorter mission, more or fewer missions, another world -- so every comparison is
equality of bits; there is no tolerance.  mission_4agents_15.json has M = 20, 26, 26 on the three maps (tests/test_gpu_ecbs_handoff.py),
which shrinks and grows M and K' for free."""
import dataclasses

import pytest

from swarm_simulator_amd import host, planner, sweep_device
from swarm_simulator_amd.types import Mission, Param
from tests import synth_ecbs as S
from tests.test_gpu_ecbs_handoff import MAPS, OUTPUTS, SCALARS, device_worlds, same_bits

pytestmark = pytest.mark.gpu

MAX_M = 64
VARIANTS = [(dict(sequential=True, batch_size=2), None), (dict(sequential=False), None), (dict(sequential=True, batch_size=2), 16)]
IDS = ["sequential-batch2", "joint-one-workgroup", "max_boxes16"]


def mission4():
    return host.load_mission("mission_4agents_15.json")


def off_the_lattice(m):
    bad = Mission(m.start.copy(), m.goal.copy(), m.radius.copy(), m.max_vel.copy(), m.max_acc.copy())
    bad.start[0, 0] = 5.6   # one cell beyond the lattice: status 1 (tests/test_ecbs_rules.py)
    return bad


def search_on(ws, idx, p, missions=None):
    m = mission4()
    return planner.ecbs_search_batch(ws, idx, missions or [m] * len(idx), p, max_nodes=S.BUDGET, max_M=MAX_M)


def snapshot(sess):
    """run + download of a session: per mission its OUTPUTS (copies) and SCALARS"""
    sess.run(planner.A.RBP_STAGE_ALL)
    assert sess.download() == [0] * sess.K
    return [({n: getattr(pl, n).copy() for n in OUTPUTS}, {n: getattr(pl, n) for n in SCALARS}) for pl in sess.plans]


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for k, ((ga, gs), (wa, ws_)) in enumerate(zip(got, want)):
        for n in OUTPUTS:
            assert same_bits(ga[n], wa[n]), (what, k, n)
        for n in SCALARS:
            assert gs[n] == ws_[n], (what, k, n)
        assert gs["qp_iterations"] > 0 and gs["total_cost"] > 0, (what, k)


def bits(records):
    return [tuple(v.hex() if isinstance(v, float) else v for v in dataclasses.astuple(r)) for r in records]


def fresh(search, p, max_boxes=None, records=False):
    """the yardstick: a session built by the constructor from the same search, run once"""
    s = planner.Session.from_ecbs(search, p, max_boxes=max_boxes)
    try:
        snap = snapshot(s)
        return (snap, bits(s.report()), bits(s.limits()[0])) if records else snap
    finally:
        s.close()


@pytest.mark.parametrize("kw,max_boxes", VARIANTS, ids=IDS)
def test_refill_equals_fresh(kw, max_boxes):
    """A = maps [0, 1, 2] (M 20, 26, 26); B = maps [2, 0]: K' shrinks, slot 0 grows from M = 20 to 26, slot 1 shrinks from 26 to 20; A
    again: K' grows back and the last slot is reused after a gap"""
    p = Param.test_sweep(**kw)
    with device_worlds(p) as ws:
        A, B = search_on(ws, [0, 1, 2], p), search_on(ws, [2, 0], p)
        assert list(A.M) == [20, 26, 26] and list(B.M) == [26, 20] and not A.status.any() and not B.status.any()
        fresh_A = fresh(A, p, max_boxes)
        fresh_B, rep_B, lim_B = fresh(B, p, max_boxes, records=True)
        sess = planner.Session.reserved(ws, 3, 4, 64, 64, p)
        assert sess.capacity == (3, 4, 64, 64) and sess.K == 0
        sess.refill(A, max_boxes=max_boxes)
        assert sess.K == 3 and list(sess.slot_of) == [0, 1, 2] and [pl.M for pl in sess.plans] == [20, 26, 26]
        first = snapshot(sess)
        assert_same(first, fresh_A, "first refill")
        sess.refill(B, max_boxes=max_boxes)
        assert sess.K == 2 and list(sess.slot_of) == [0, 1] and [pl.M for pl in sess.plans] == [26, 20]
        assert_same(snapshot(sess), fresh_B, "shrunk")
        assert bits(sess.report()) == rep_B and bits(sess.limits()[0]) == lim_B
        sess.refill(A, max_boxes=max_boxes)
        again = snapshot(sess)
        assert_same(again, fresh_A, "grown back")
        assert_same(again, first, "the first run's bits")
        assert sess.capacity == (3, 4, 64, 64)
        sess.close()
        A.close(), B.close()


def test_a_failed_mission_in_the_middle():
    p, m = Param.test_sweep(), mission4()
    bad = off_the_lattice(m)
    with device_worlds(p) as ws:
        twin = search_on(ws, [0, 2], p)
        fresh_twin = fresh(twin, p)
        twin.close()
        mixed = search_on(ws, [0, 1, 2], p, [m, bad, m])
        assert list(mixed.status) == [0, 1, 0]
        sess = planner.Session.reserved(ws, 3, 4, 64, 64, p)
        sess.refill(mixed)
        assert list(sess.slot_of) == [0, -1, 1] and sess.K == 2
        before = snapshot(sess)
        assert_same(before, fresh_twin, "the two survivors")
        none = search_on(ws, [0, 1, 2], p, [bad] * 3)
        assert list(none.status) == [1, 1, 1]
        with pytest.raises(ValueError, match="no mission of the search has status 0"):
            sess.refill(none)
        assert sess.K == 2 and list(sess.slot_of) == [0, -1, 1]
        sess.reset()
        assert_same(snapshot(sess), before, "after the refused refill")
        sess.close()
        mixed.close(), none.close()


def test_refusals_leave_the_session_as_it_was():
    p, m = Param.test_sweep(), mission4()
    with device_worlds(p) as ws, device_worlds(p) as other:
        two = search_on(ws, [0, 0], p)                       # M = 20, 20
        sess = planner.Session.reserved(ws, 2, 4, 22, 22, p)
        sess.refill(two)
        before = snapshot(sess)
        too_many = search_on(ws, [0, 0, 0], p)              # K' = 3 above the capacity's 2
        too_long = search_on(ws, [0, 1], p)                 # M = 26 above the stride 22
        two_agents = search_on(ws, [0, 0], p, [m.subset([0, 1])] * 2)
        elsewhere = search_on(other, [0, 0], p)             # a second DeviceWorlds
        for search, why in ((too_many, "capacity"), (too_long, "exceed the session's strides"), (two_agents, "agents"), (elsewhere, "another set of worlds")):
            assert not search.status.any()
            with pytest.raises(ValueError, match=why):
                sess.refill(search)
            assert sess.K == 2 and [pl.M for pl in sess.plans] == [20, 20]
            sess.reset()
            assert_same(snapshot(sess), before, why)
            search.close()
        with pytest.raises(ValueError, match="exceed the session's strides"):   # a box capacity above the stride
            sess.refill(two, max_boxes=23)
        sess.reset()
        assert_same(snapshot(sess), before, "max_boxes")
        sess.close()
        two.close()


def test_an_empty_reserved_session_refuses():
    p = Param.test_sweep()
    with device_worlds(p) as ws:
        sess = planner.Session.reserved(ws, 3, 4, 64, 64, p)
        with pytest.raises(RuntimeError, match="holds no mission"):
            sess.run()
        with pytest.raises(ValueError, match="holds no mission"):
            sess.download()
        with pytest.raises(ValueError, match="holds no mission"):
            sess.report()
        A = search_on(ws, [0, 1, 2], p)
        sess.refill(A)
        with pytest.raises(ValueError, match="did not include the PLANNER stage"):
            sess.report()
        snapshot(sess)
        assert len(sess.report()) == 3
        sess.refill(A)                                       # ... and again after every refill
        with pytest.raises(ValueError, match="did not include the PLANNER stage"):
            sess.report()
        sess.close()
        A.close()


def test_no_allocation_in_the_steady_state():
    import torch
    p = Param.test_sweep()
    with device_worlds(p) as ws:
        A, B = search_on(ws, [0, 1, 2], p), search_on(ws, [2, 0], p)
        sess = planner.Session.reserved(ws, 3, 4, 64, 64, p)

        def cycle(search):
            sess.refill(search)
            sess.run()
            assert [r.status for r in sess.report()] == [0] * sess.K
            assert [r.status for r in sess.separation()[0]] == [0] * sess.K

        cycle(A), cycle(B)
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info(0)[0]
        cycle(A), cycle(B)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free_before
        sess.close()
        A.close(), B.close()


def test_a_session_from_the_constructor_is_refillable():
    """within its own capacity (K = 3, M = 26, max_boxes = 26): B brings fewer missions and M = 26 into the slot that held M = 20"""
    p = Param.test_sweep(sequential=True, batch_size=2)
    with device_worlds(p) as ws:
        A, B = search_on(ws, [0, 1, 2], p), search_on(ws, [2, 0], p)
        fresh_A, fresh_B = fresh(A, p), fresh(B, p)
        sess = planner.Session.from_ecbs(A, p)
        assert sess.capacity == (3, 4, 26, 26)
        assert_same(snapshot(sess), fresh_A, "as constructed")
        sess.refill(B)
        assert_same(snapshot(sess), fresh_B, "refilled")
        sess.refill(A)
        assert_same(snapshot(sess), fresh_A, "refilled back")
        sess.close()
        # a session of host plans on host grids has no set of worlds to be refilled from
        inits = planner.ecbs_plan_batch(ws, [0], [mission4()], p, max_nodes=S.BUDGET, max_M=MAX_M)
        w = host.load_world(MAPS[0], p)
        hosted = planner.Session([w], [mission4()], p, [inits[0].clone_inputs()])
        with pytest.raises(ValueError, match="not those of the search's set of worlds"):
            hosted.refill(A)
        hosted.close()
        A.close(), B.close()


def test_sweep_device_streams_the_maps_through_one_session(capsys):
    argv = ["--device-worlds", "--device-ecbs", "--device-handoff", "--maps", "3,5,7", "--mode", "batched", "--mission", "mission_8agents_15.json"]
    lines = []
    for extra in ([], ["--stream", "2"]):
        assert sweep_device.main(argv + extra) == 0
        out = capsys.readouterr().out
        lines.append([l for l in out.splitlines() if l.startswith("map")])
    assert [l.split(":")[0] for l in lines[0]] == ["map3", "map5", "map7"] and lines[0] == lines[1]
