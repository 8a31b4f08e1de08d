"""A session refilled from a caller's own plans (rbp_session_refill_from_plans, rbp_session_reserve_plan_stage, rbp_plan_stage_bytes,
kernels/handoff.hip session_refill_plans_kernel, csrc/common/plan_stage.h; planner.Session.refill_plans / reserve_plan_stage,
planner.plan_stage_bytes, sweep_device --stream-plans).  The yardstick is the constructor: planner.Session(worlds, missions, param, plans)
of the same host plans, run once.  The rule under test is that of tests/test_gpu_session_refill.py -- after a refill and a run every
output bit equals that fresh session's, whatever the slots held before and however many rounds the staging block needed -- so every
comparison is equality of bits; there is no tolerance.  mission_4agents_15.json has M = 20, 26, 26 on the three maps."""
import numpy as np
import pytest

from swarm_simulator_amd import host, planner, sweep_device
from swarm_simulator_amd.types import Mission, Param, PlanResult
from tests import synth_ecbs as S
from tests.test_gpu_ecbs_handoff import MAPS, device_worlds
from tests.test_gpu_session_refill import IDS, MAX_M, VARIANTS, assert_same, bits, mission4, search_on, snapshot
from tests.test_gpu_session_refill import fresh as fresh_from_search

pytestmark = pytest.mark.gpu

CAP = (3, 4, 64, 64)


@pytest.fixture(scope="module")
def env():
    """the worlds on the device and the host plans of the mission on each of them: computed once, never written"""
    p = Param.test_sweep()
    with device_worlds(p) as ws:
        inits = planner.ecbs_plan_batch(ws, [0, 1, 2], [mission4()] * 3, p, max_nodes=S.BUDGET, max_M=MAX_M)
        assert [pl.M for pl in inits] == [20, 26, 26] and not any(inits.status)
        yield ws, list(inits)


def batch(env, idx, max_boxes=None, missions=None):
    """(worlds, missions, plans) of the mission on the maps idx: fresh copies of the plans' inputs"""
    ws, inits = env
    plans = [PlanResult(inits[i].init_traj.copy(), inits[i].T.copy(), max_boxes) if max_boxes else inits[i].clone_inputs() for i in idx]
    return [ws[i] for i in idx], missions or [mission4()] * len(idx), plans


def fresh(env, p, idx, max_boxes=None, records=False, missions=None, edit=None):
    """the yardstick: a session built by the constructor from the same host plans, run once"""
    w, m, plans = batch(env, idx, max_boxes, missions)
    if edit:
        edit(plans)
    s = planner.Session(w, m, p, plans)
    try:
        snap = snapshot(s)
        return (snap, bits(s.report()), bits(s.limits()[0])) if records else snap
    finally:
        s.close()


@pytest.mark.parametrize("kw,max_boxes", VARIANTS, ids=IDS)
def test_refill_equals_fresh(env, kw, max_boxes):
    """A = maps [0, 1, 2] (M 20, 26, 26); B = maps [2, 0]: K shrinks, slot 0 grows from M = 20 to 26, slot 1 shrinks from 26 to 20; A again"""
    p = Param.test_sweep(**kw)
    fresh_A = fresh(env, p, [0, 1, 2], max_boxes)
    fresh_B, rep_B, lim_B = fresh(env, p, [2, 0], max_boxes, records=True)
    sess = planner.Session.reserved(env[0], *CAP, p)
    sess.refill_plans(*batch(env, [0, 1, 2], max_boxes))
    assert sess.K == 3 and sess.slot_of is None and [pl.M for pl in sess.plans] == [20, 26, 26]
    first = snapshot(sess)
    assert_same(first, fresh_A, "first refill")
    sess.refill_plans(*batch(env, [2, 0], max_boxes))
    assert sess.K == 2 and [pl.M for pl in sess.plans] == [26, 20]
    assert_same(snapshot(sess), fresh_B, "shrunk")
    assert bits(sess.report()) == rep_B and bits(sess.limits()[0]) == lim_B
    sess.refill_plans(*batch(env, [0, 1, 2], max_boxes))
    again = snapshot(sess)
    assert_same(again, fresh_A, "grown back")
    assert_same(again, first, "the first run's bits")
    assert sess.capacity == CAP
    sess.close()


def test_content_goes_where_it_belongs(env):
    """one batch of the mission as it is, one with radii scaled and max_vel halved, and one plan whose T is multiplied by 1.7: T is copied,
    not regenerated from time_step, and every mission array lands in its own slot"""
    p, m = Param.test_sweep(), mission4()
    other = Mission(m.start.copy(), m.goal.copy(), m.radius * 0.8, m.max_vel * 0.5, m.max_acc.copy())
    missions = [m, other, m]

    def stretch(plans):
        plans[2].T *= 1.7

    want = fresh(env, p, [0, 1, 2], missions=missions, edit=stretch)
    plain = fresh(env, p, [0, 1, 2])
    for k in (1, 2):   # (the variations do change the plan)
        assert want[k][0]["coef"].tobytes() != plain[k][0]["coef"].tobytes()
    assert want[2][0]["T"][-1] == pytest.approx(1.7 * plain[2][0]["T"][-1] * want[2][1]["time_scale"] / plain[2][1]["time_scale"])
    sess = planner.Session.reserved(env[0], *CAP, p)
    w, _, plans = batch(env, [0, 1, 2])
    stretch(plans)
    sess.refill_plans(w, missions, plans)
    assert_same(snapshot(sess), want, "mixed batch")
    sess.close()


def partition(Ms, block):
    """the greedy partition of csrc/common/plan_stage.h, from the bytes of each mission's own shape"""
    rounds, used = [0], 0
    for M in Ms:
        b = planner.plan_stage_bytes((1, 4, M, 1), 1)
        assert b <= block
        if used + b > block:
            rounds.append(0)
            used = 0
        rounds[-1] += 1
        used += b
    return rounds


def test_rounds(env):
    """Staging blocks that split A = (M 20, 26, 26) into rounds give the bits of one round.  Missions are packed tightly, so the two shorter
    ones together take less than ONE mission of the capacity's shape (M = 64): plan_stage_bytes(CAP, 1) gives the rounds 2 + 1 and
    plan_stage_bytes(CAP, 2) a single round.  The blocks of one and of two missions of the shape M = 26 give what is wanted: three rounds
    of one mission, and a round of two with a short last round.  The partitions are asserted, not assumed."""
    p = Param.test_sweep()
    fresh_A = fresh(env, p, [0, 1, 2])
    shape26 = (3, 4, 26, 64)
    blocks = [(planner.plan_stage_bytes(shape26, 1), [1, 1, 1]), (planner.plan_stage_bytes(shape26, 2), [2, 1]),
              (planner.plan_stage_bytes(CAP, 1), [2, 1]), (planner.plan_stage_bytes(CAP, 2), [3]), (0, [3])]
    for block, rounds in blocks:
        assert partition([20, 26, 26], block or planner.plan_stage_bytes(CAP, 3)) == rounds
        sess = planner.Session.reserved(env[0], *CAP, p)
        if block and block < planner.plan_stage_bytes(CAP, 1):   # less than one mission of the capacity's shape is refused
            with pytest.raises(ValueError, match="less than one mission"):
                sess.reserve_plan_stage(block)
            sess.close()
            sess = planner.Session.reserved(env[0], 3, 4, 26, 64, p)   # ... a session whose stride is 26 takes the block
        sess.reserve_plan_stage(block)
        sess.reserve_plan_stage(block)                         # the same size again is no error
        with pytest.raises(ValueError, match="has been reserved"):
            sess.reserve_plan_stage(block + 8 if block else 8 * planner.plan_stage_bytes(CAP, 3))
        sess.refill_plans(*batch(env, [0, 1, 2]))
        assert_same(snapshot(sess), fresh_A, f"block of {block} bytes")
        sess.refill_plans(*batch(env, [2, 0]))                 # a shorter batch through the same block, then the first again
        snapshot(sess)
        sess.refill_plans(*batch(env, [0, 1, 2]))
        assert_same(snapshot(sess), fresh_A, f"block of {block} bytes, again")
        sess.close()


def test_both_sources_in_one_session(env):
    p = Param.test_sweep(sequential=True, batch_size=2)
    ws = env[0]
    A = search_on(ws, [0, 1, 2], p)
    from_search = fresh_from_search(A, p)
    from_plans = fresh(env, p, [2, 0])
    sess = planner.Session.reserved(ws, *CAP, p)
    sess.refill(A)
    assert_same(snapshot(sess), from_search, "from the search")
    sess.refill_plans(*batch(env, [2, 0]))
    assert sess.slot_of is None
    assert_same(snapshot(sess), from_plans, "from plans")
    sess.refill(A)
    assert list(sess.slot_of) == [0, 1, 2]
    assert_same(snapshot(sess), from_search, "from the search again")
    sess.close()
    A.close()


def test_refusals_leave_the_session_as_it_was(env):
    p, m = Param.test_sweep(), mission4()
    ws, inits = env
    sess = planner.Session.reserved(ws, 2, 4, 22, 22, p)
    with pytest.raises(ValueError, match="less than one mission"):   # a stage smaller than one mission of the capacity's shape
        sess.reserve_plan_stage(planner.plan_stage_bytes((2, 4, 22, 22), 1) - 8)
    sess.refill_plans(*batch(env, [0, 0]))                  # M = 20, 20
    before = snapshot(sess)
    kept = sess.plans
    two_agents = [PlanResult(inits[0].init_traj[:2].copy(), inits[0].T.copy()) for _ in range(2)]
    w0 = batch(env, [0, 0])
    cases = [(batch(env, [0, 0, 0]), "3 missions, the session's capacity is 2"),
             (batch(env, [0, 1]), r"mission 1: plan\.M = 26 outside"),
             (batch(env, [0, 0], max_boxes=23), r"mission 0: plan\.max_boxes = 23 outside"),
             ((w0[0], [m.subset([0, 1])] * 2, two_agents), r"mission 0: plan\.N = 2"),
             ((w0[0], [m, m.subset([0, 1])], w0[2]), r"mission 1: mission\.N = 2"),
             (([ws[0], host.load_world(MAPS[0], p)], w0[1], w0[2]), r"mission 1: world\.dist is a host pointer")]
    for args, why in cases:
        with pytest.raises(ValueError, match=why):
            sess.refill_plans(*args)
        assert sess.K == 2 and sess.plans is kept and [pl.M for pl in sess.plans] == [20, 20]
        sess.reset()
        assert_same(snapshot(sess), before, why)
    with pytest.raises(ValueError, match="less than one mission"):   # ... and with the block reserved
        sess.reserve_plan_stage(64)
    sess.reset()
    assert_same(snapshot(sess), before, "stage")
    sess.close()


def test_no_allocation(env):
    import torch
    p = Param.test_sweep()
    A, B = batch(env, [0, 1, 2]), batch(env, [2, 0])
    other = planner.Session.reserved(env[0], *CAP, p)      # (the runtime loads a kernel's code object when it is first launched)
    other.refill_plans(*A)
    other.close()
    sess = planner.Session.reserved(env[0], *CAP, p)
    sess.reserve_plan_stage()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    sess.refill_plans(*A)                                  # the first refill itself: the block was reserved up front
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free_before

    def cycle(b):
        sess.refill_plans(*b)
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


def test_a_session_from_the_constructor_is_refillable(env):
    """within its own capacity (K = 3, M = 26, max_boxes = 26): B brings fewer missions and M = 26 into the slot that held M = 20"""
    p = Param.test_sweep(sequential=True, batch_size=2)
    fresh_A, fresh_B = fresh(env, p, [0, 1, 2]), fresh(env, p, [2, 0])
    w, m, plans = batch(env, [0, 1, 2])
    sess = planner.Session(w, m, p, plans)
    assert sess.capacity == (3, 4, 26, 26)
    assert_same(snapshot(sess), fresh_A, "as constructed")
    sess.refill_plans(*batch(env, [2, 0]))
    assert_same(snapshot(sess), fresh_B, "refilled")
    sess.refill_plans(*batch(env, [0, 1, 2]))
    assert_same(snapshot(sess), fresh_A, "refilled back")
    sess.close()


@pytest.mark.parametrize("front_end", [[], ["--device-ecbs"]], ids=["host-search", "device-search"])
def test_sweep_device_streams_host_plans_through_one_session(capsys, front_end):
    argv = ["--device-worlds", "--maps", "3,5,7", "--mode", "batched", "--mission", "mission_8agents_15.json"] + front_end
    lines = []
    for extra in ([], ["--stream-plans", "2"]):
        assert sweep_device.main(argv + extra) == 0
        out = capsys.readouterr().out
        lines.append([l for l in out.splitlines() if l.startswith("map")])
    assert [l.split(":")[0] for l in lines[0]] == ["map3", "map5", "map7"] and lines[0] == lines[1]
