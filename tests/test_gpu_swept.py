"""The swept clearance kernels (kernels/swept.hip) against rbp_swept_clearance_host, BIT FOR BIT: both read one text,
csrc/common/swept_rules.h, and these tests are what hold the device compiler to the host's reading of it -- every field of the struct,
indices and counters included, every agent's lower clearance, and every row the kernels must NOT touch (the agents' arrays are pre-filled
with a sentinel on both sides and compared whole).

rbp_dev_swept_clearance on synthetic seeded coefficients (tests/synth_report.py) over seeded grids (tests/synth_clearance.py) at the smallest
shapes where the kernels change path: items per mission around one wavefront and around 64 and 65 x 5 (N in 1, 2, 3, 64, 65 x M in 1, 2, 5),
(depth, refine_below) in (0, 1e9), (3, 0.3), (6, 1e9), (8, 1e9), (4, -2) -- one lane per item, 8 lanes, 64 lanes, 64 lanes walking four pieces
each, and only what is outside or over budget --, three ragged missions under one stride on three grids of different shape, resolution and
negative key_min (one 7 x 11 x 5) under time scales 1 and 1.7, plans that leave the grid on each side, NaN and infinite coefficients, a fast
diagonal whose depth-0 box is over the budget while its depth-4 pieces are not, ties between agents and between pieces, the minimum in the
last piece of the last item, a host grid against the same grid as a device tensor, a host against a device agent_lower, and the wall the
samples miss.  rbp_session_swept_clearance on real small sessions against host.swept_clearance of the downloaded plans.  The refusals that
need no device run in the CPU leg too (they carry no gpu mark)."""
import ctypes as C

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import DeviceWorld, Param, PlanResult, SweptClearance, World
from tests import synth_clearance as L
from tests import synth_report as S
from tests import synth_swept as X
from tests.common import SMALL_CASES, Case

gpu = pytest.mark.gpu
SENTINEL = -7.0
PAIRS = [(0, 1e9), (3, 0.3), (6, 1e9), (8, 1e9), (4, -2.0)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_records(dev, ref):
    assert len(dev) == len(ref)
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert d.bits() == r.bits(), (k, d, r)


def check(plans, worlds, depth, refine_below, dev_worlds=None):
    """rbp_dev_swept_clearance into a sentinel-filled host array against rbp_swept_clearance_host into one filled alike: records, and the
    array whole.  Returns (device records, agents [K][N])."""
    ref, ref_agents = X.host_swept(plans, worlds, depth, refine_below, SENTINEL)
    dev_agents = np.full((plans.K, plans.N), SENTINEL)
    dev = planner.swept_clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, dev_worlds or worlds, depth, refine_below, plans.time_scale, dev_agents)
    same_records(dev, ref)
    assert np.array_equal(bits(dev_agents), bits(ref_agents))
    without = planner.swept_clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, dev_worlds or worlds, depth, refine_below, plans.time_scale)
    same_records(without, ref)
    return dev, dev_agents


def forest(seed):
    """30 x 30 x 12 cells of 0.25 m from (-0.5, -0.5, 0): the synthetic agents (tests/synth_report.py: near (a % side, a // side, 0.5 .. 2),
    wandering a few decimetres) lie inside up to 7 x 7 of them, beyond that partly outside"""
    return L.grid(seed, (30, 30, 12), (-2, -2, 0), 0.25)


def at_rest(N, M, where=(0.1, 0.1, 0.1), radius=0.25):
    """N agents at rest in one point, M unit segments"""
    c = np.zeros((N, 3, M, 6))
    c[:, 0, :, 5], c[:, 1, :, 5], c[:, 2, :, 5] = where
    return S.Plans([M], S.times("unit", M)[None, :], [c.reshape(N, 3, 6 * M)], np.full((1, N), radius))


def test_the_shapes_below_are_the_ones_the_kernels_take_other_paths_at():
    assert sorted({(N * M + 63) // 64 for N in (1, 2, 3, 64, 65) for M in (1, 2, 5)}) == [1, 2, 3, 5, 6]   # wavefronts of items: one, full ones, one over
    assert [min(1 << d, 64) for d, _ in PAIRS] == [1, 8, 64, 64, 16] and [(1 << d) // min(1 << d, 64) for d, _ in PAIRS] == [1, 1, 1, 4, 1]


@gpu
@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 64, 65])
def test_agent_counts_segment_counts_depths_and_thresholds(N, M):
    plans, w = S.make(100 * N + M, N, [M]), [forest(N + M)]
    for depth, below in PAIRS:
        dev, agents = check(plans, w, depth, below)
        r = dev[0]
        assert r.lower_segment >= 0 and agents[0, r.lower_agent] == r.lower_clearance == agents[0].min() and r.lower_depth in (0, depth)
        assert (r.outside > 0) == (N >= 64) and r.refined <= N * M
        if below == 1e9:
            assert r.refined == N * M
        if below == -2.0:
            assert r.refined >= r.outside   # (nothing but what is outside or over budget at depth 0 goes on)


@gpu
@pytest.mark.parametrize("ts", [1.0, 1.7])
def test_three_grids_ragged_missions_and_scaled_times(ts):
    """K = 3 under one stride above every M: M = 1, 5, 2; unit, 0.5 / 1.7 and alternating times.  First on three different grids -- a
    non-cubic 7 x 11 x 5 one, one with a negative key_min and a third resolution --, then with one grid shared by two missions."""
    plans = S.make(70, 6, [1, 5, 2], ["unit", "nonunit", "alternating"], [ts] * 3, stride=7)
    small, slab, fine = L.grid(1, (7, 11, 5), (-1, -2, 1), 0.3), L.grid(2, (21, 9, 14), (-3, -1, 2), 0.2), L.grid(3, (48, 40, 30), (-8, -8, 0), 0.1)
    for depth, below in ((4, 0.3), (6, 1e9), (0, -2.0)):
        dev, _ = check(plans, [small, slab, fine], depth, below)
        assert [d.end_time for d in dev] == [plans.scaled_T(k)[-1] for k in range(3)]
        assert dev[0].outside > 0 and dev[1].outside > 0 and dev[0].lower_dist == -1.0
        shared, _ = check(plans, [fine, small, fine], depth, below)
        assert shared[2].bits() == dev[2].bits()


@gpu
def test_plans_that_leave_the_grid_on_each_side():
    """six agents start at the middle of an 8 x 6 x 4 grid of 0.25 m cells around the origin and fly at 1 m/s along +x, -x, +y, -y, +z, -z for
    two seconds; a seventh stays"""
    N, M = 7, 2
    c = np.zeros((N, 3, M, 6))
    c[:, 2, :, 5] = 0.5
    for a in range(6):
        k, sign = a // 2, 1.0 - 2.0 * (a % 2)
        c[a, k, :, 4] = sign
        c[a, k, 1, 5] += sign   # the second segment goes on where the first ended
    plans = S.Plans([M], S.times("unit", M)[None, :], [c.reshape(N, 3, 6 * M)], np.full((1, N), 0.125))
    w = World(np.full((8, 6, 4), 0.5, np.float32), (-4, -3, 0), 0.25)
    for depth, below in PAIRS:
        dev, agents = check(plans, [w], depth, below)
        assert np.all(agents[0, :6] == -1.125) and agents[0, 6] == 0.375
        assert (dev[0].lower_clearance, dev[0].lower_dist, dev[0].upper_clearance, dev[0].upper_dist) == (-1.125, -1.0, -1.125, -1.0)
        # +-z (z = 0.5 +- t against [0, 1)) and +-y (against [-0.75, 0.75)) leave in their first segment, +x reaches x = 1, the first key
        # beyond the grid, at its end, and -x reaches -1, the first key inside: all twelve items but that one have a piece outside
        assert dev[0].uncertified == dev[0].outside == dev[0].hitting == 11 and dev[0].over_budget == 0 and dev[0].refined == (14 if below == 1e9 else 11)
        # the first piece outside in segment 0: the whole of agent 0's at depth 0, otherwise +z's, the one that ends at t = 0.5
        assert (dev[0].lower_segment, dev[0].lower_piece, dev[0].lower_agent) == ((0, 0, 0) if depth == 0 else (0, (1 << (depth - 1)) - 1, 4))


@gpu
def test_nan_and_infinite_coefficients_are_outside():
    plans = S.make(13, 5, [2])
    plans.coefs[0][0, 1, 6 + 3] = np.nan    # agent 0, y, second segment
    plans.coefs[0][3, 0, 2] = np.inf        # agent 3, x, first segment
    plans.coefs[0][4, 2, 5] = 1e300         # agent 4, z, first segment
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    for depth, below in PAIRS:
        dev, agents = check(plans, [forest(5)], depth, below)
        assert dev[0].outside >= 3 and dev[0].lower_dist == -1.0 and np.isfinite(dev[0].lower_clearance) and np.all(np.isfinite(agents))
    plans.radius[0, 1] = np.nan             # ... and a NaN radius is never the minimum
    dev, agents = check(plans, [forest(5)], 4, 1e9)
    assert agents[0, 1] == 1e9 and dev[0].lower_agent != 1 and dev[0].upper_agent != 1


@gpu
def test_a_fast_diagonal_over_the_budget_at_depth_0_and_within_it_at_depth_4():
    """one agent crosses a 40 x 40 x 8 grid of 0.1 m cells from (0.25, 0.25, 0.05) to (3.65, 3.65, 0.75) in one segment: 35 x 35 x 8 = 9800
    cells at depth 0; four others rest.  (4, -2) refines that item alone"""
    N = 5
    c = np.zeros((N, 3, 1, 6))
    c[:, 0, 0, 5], c[:, 1, 0, 5], c[:, 2, 0, 5] = 0.25, 0.25, 0.05
    c[1:, 0, 0, 5] += 0.3 * np.arange(1, N)
    c[0, 0, 0, 4], c[0, 1, 0, 4], c[0, 2, 0, 4] = 3.4, 3.4, 0.7
    plans = S.Plans([1], S.times("unit", 1)[None, :], [c.reshape(N, 3, 6)], np.full((1, N), 0.15))
    w = L.grid(9, (40, 40, 8), (0, 0, 0), 0.1)
    dev, agents = check(plans, [w], 0, -2.0)
    assert (dev[0].over_budget, dev[0].refined, dev[0].outside, agents[0, 0]) == (1, 1, 0, -1.15)
    dev, agents = check(plans, [w], 4, -2.0)
    assert (dev[0].over_budget, dev[0].refined, dev[0].outside) == (0, 1, 0) and agents[0, 0] > -1.0
    dev, _ = check(plans, [w], 1, 1e9)   # halves of 18 x 18 x 4 = 1296 cells
    assert (dev[0].over_budget, dev[0].refined) == (0, N)
    for depth, below in PAIRS:
        check(plans, [w], depth, below)


@gpu
@pytest.mark.parametrize("N", [4, 65])
def test_ties_between_agents_and_between_pieces_report_the_first(N):
    """every agent rests in one cell with one radius through two segments: every piece of every item ties, in every lane, wavefront and
    kernel; the first is segment 0, piece 0, agent 0"""
    plans = at_rest(N, 2)
    w = World(np.full((4, 4, 4), 0.75, np.float32), (-2, -2, -2), 0.25)
    for depth, below in PAIRS + [(3, 0.5), (3, 0.6)]:   # (0.5 is the clearance itself: nothing refined; 0.6: everything)
        dev, agents = check(plans, [w], depth, below)
        r = dev[0]
        assert (r.lower_clearance, r.lower_dist, r.lower_segment, r.lower_piece, r.lower_agent) == (0.5, 0.75, 0, 0, 0)
        assert (r.upper_clearance, r.upper_dist, r.upper_segment, r.upper_piece, r.upper_agent) == (0.5, 0.75, 0, 0, 0)
        assert (r.uncertified, r.hitting, r.outside, r.over_budget) == (0, 0, 0, 0) and np.all(agents == 0.5)
        assert r.refined == (2 * N if below > 0.5 else 0) and r.lower_depth == (depth if below > 0.5 else 0)
    plans.radius[:] = 1.0   # ... and with the radius above the grid's value: every item uncertified and hitting
    dev, _ = check(plans, [w], 3, 0.3)
    assert (dev[0].uncertified, dev[0].hitting, dev[0].refined, dev[0].lower_clearance, dev[0].lower_agent) == (2 * N, 2 * N, 2 * N, -0.25, 0)


@gpu
@pytest.mark.parametrize("N", [64, 65])
def test_the_minimum_in_the_last_piece_of_the_last_item(N):
    """the last agent flies x = 0.1 + 32 t through its last segment over cells of 0.25 m and meets the only low cell, key 128, in
    [32.0, 32.1]: in piece 63 of 64 and in piece 255 of 256 alone"""
    M = 5
    c = np.zeros((N, 3, M, 6))
    c[:, :, :, 5] = 0.1
    c[N - 1, 0, M - 1, 4] = 32.0
    plans = S.Plans([M], S.times("unit", M)[None, :], [c.reshape(N, 3, 6 * M)], np.full((1, N), 0.25))
    d = np.full((130, 2, 2), 1.0, np.float32)
    d[128, 0, 0] = 0.5
    w = [World(d, (0, 0, 0), 0.25)]
    for depth in (6, 8):
        dev, agents = check(plans, w, depth, 1e9)
        r = dev[0]
        assert (r.lower_segment, r.lower_piece, r.lower_agent, r.lower_clearance, r.lower_dist, r.lower_depth) == (M - 1, (1 << depth) - 1, N - 1, 0.25, 0.5, depth)
        assert (r.upper_segment, r.upper_piece, r.upper_agent, r.upper_clearance) == (M - 1, (1 << depth) - 1, N - 1, 0.25)
        assert np.all(agents[0, :N - 1] == 0.75) and agents[0, N - 1] == 0.25 and (r.uncertified, r.hitting, r.outside) == (0, 0, 0)
    dev, _ = check(plans, w, 4, 0.6)   # the last item alone is refined
    assert (dev[0].refined, dev[0].lower_piece, dev[0].lower_depth, dev[0].upper_depth) == (1, 15, 4, 4)


@gpu
def test_a_host_grid_and_the_same_grid_as_a_device_tensor_give_the_same_bytes():
    import torch
    plans = S.make(23, 65, [5, 2])
    ws = [forest(8), forest(9)]
    dev_host, agents_host = check(plans, ws, 4, 0.3)
    tensors = [torch.from_numpy(w.dist).to("cuda:0") for w in ws]
    torch.cuda.synchronize()
    dws = [DeviceWorld.from_tensor(t, w.key_min, w.res) for t, w in zip(tensors, ws)]
    dev_dev, agents_dev = check(plans, ws, 4, 0.3, dev_worlds=dws)
    assert [d.bits() for d in dev_dev] == [d.bits() for d in dev_host] and np.array_equal(bits(agents_dev), bits(agents_host))
    mixed, agents_mixed = check(plans, ws, 4, 0.3, dev_worlds=[dws[0], ws[1]])   # one of each
    assert np.array_equal(bits(agents_mixed), bits(agents_host))


@gpu
def test_a_host_and_a_device_agent_lower_give_the_same_bytes():
    import torch
    plans = S.make(24, 65, [5, 1, 2])
    ws = [forest(8), forest(9), forest(10)]
    for depth, below in ((4, 0.3), (8, 1e9)):
        _, agents_host = check(plans, ws, depth, below)
        t = torch.full((3, 65), SENTINEL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        dev = planner.swept_clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, ws, depth, below, None, t)
        same_records(dev, X.host_swept(plans, ws, depth, below)[0])
        assert np.array_equal(bits(t.cpu().numpy()), bits(agents_host))


@gpu
def test_the_wall_the_samples_miss():
    """the behavioural case: the sampled call says clear, the swept call proves the hit"""
    world, mission, pr = X.wall()
    plans = S.Plans([1], pr.T[None, :], [pr.coef.reshape(1, 3, 6)], mission.radius[None, :])
    sampled = planner.clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, [world], 0.1)
    assert sampled[0].hits == 0 and sampled[0].min_clearance == 1.0 - 0.15
    dev, _ = check(plans, [world], 0, 1e9)
    assert dev[0].uncertified == 1 and dev[0].hitting == 0
    dev, agents = check(plans, [world], 8, 1e9)
    assert dev[0].hitting == 1 and dev[0].upper_clearance == 0.0 - 0.15 and agents[0, 0] == 0.0 - 0.15


# ---- sessions ------------------------------------------------------------------------------------------------------------------
def session_check(worlds, missions, param, plans, run="run"):
    """plan, bound the clearance, and compare with host.swept_clearance of the downloaded plans on the same grids"""
    sess = planner.Session(worlds, missions, param, plans)
    getattr(sess, run)(A.RBP_STAGE_ALL)
    records, agents = sess.swept_clearance(per_agent=True)   # (after run_async: waits for the solve)
    plain, none = sess.swept_clearance()
    on_dev, agents_dev = sess.swept_clearance(per_agent=True, device_out=True)
    every, _ = sess.swept_clearance(depth=8, refine_below=1e9)
    status = sess.download()
    sess.close()
    assert status == [0] * len(plans) and [r.status for r in records] == status and none is None
    ref = [host.swept_clearance(w, m, p, per_agent=True) for w, m, p in zip(worlds, missions, plans)]
    same_records(records, [r for r, _ in ref])
    same_records(plain, records), same_records(on_dev, records)
    same_records(every, [host.swept_clearance(w, m, p, 8, 1e9) for w, m, p in zip(worlds, missions, plans)])
    assert np.array_equal(bits(agents), bits(np.stack([a for _, a in ref]))) and np.array_equal(bits(agents_dev.cpu().numpy()), bits(agents))
    assert all(r.end_time == p.T[-1] and r.lower_segment >= 0 and r.lower_clearance <= r.upper_clearance for r, p in zip(records, plans))
    return records


@gpu
@pytest.mark.parametrize("name", SMALL_CASES)
def test_session_swept_clearance_equals_the_host_s_of_the_download(name):
    c = Case(name)
    (r,) = session_check([c.world], [c.mission], c.param, [c.inputs()])
    assert (r.uncertified, r.hitting, r.outside, r.over_budget) == (0, 0, 0, 0)


@gpu
def test_session_swept_clearance_with_a_time_scale_above_one():
    c = Case("s4_map1_seq2")
    c.mission.max_vel = c.mission.max_vel * 0.25
    plans = [c.inputs()]
    session_check([c.world], [c.mission], c.param, plans)
    assert plans[0].time_scale > 1.0


@gpu
def test_session_swept_clearance_waits_for_an_asynchronous_joint_solve():
    """16 agents, plan/sequential = false: the grid-wide solver, whose run_async returns while the solve proceeds"""
    c = Case("c2_16agents_map3")
    session_check([c.world], [c.mission], Param.test_sweep(sequential=False), [c.inputs()], run="run_async")


@gpu
def test_a_failed_mission_in_the_middle_is_flagged_and_left_alone():
    """a waypoint inside an obstacle (the way tests/test_gpu_report.py builds that error) between two copies of the healthy mission"""
    import torch
    c = Case("s4_map1_seq2")
    w, param, first, last = c.world, c.param, c.inputs(), c.inputs()
    t = first.init_traj.copy()
    t[2, 5] = ((np.array(w.key_min) + np.argwhere(w.dist == 0)[0] + 0.5) * w.res).astype(np.float32)
    plans = [first, PlanResult(t, first.T), last]
    sess = planner.Session([w] * 3, [c.mission] * 3, param, plans)
    sess.run()
    st = sess.download()
    out, out2 = (A.rbp_swept_clearance * 3)(), (A.rbp_swept_clearance * 3)()
    host_a = np.full((3, 4), SENTINEL)
    assert planner.lib().rbp_session_swept_clearance(sess._h, 4, 0.5, out, C.c_void_p(host_a.ctypes.data), None) == A.RBP_OK
    dev_a = torch.full((3, 4), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert planner.lib().rbp_session_swept_clearance(sess._h, 4, 0.5, out2, C.c_void_p(dev_a.data_ptr()), None) == A.RBP_OK
    sess.close()
    assert st == [0, A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    assert [getattr(out[1], n) for n, _ in A.rbp_swept_clearance._fields_] == [0.0] * 5 + [0] * 5 + [-1] * 8 + [A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    ref_a = np.full((3, 4), SENTINEL)
    for k in (0, 2):
        ref, ref_a[k] = host.swept_clearance(w, c.mission, plans[k], 4, 0.5, per_agent=True)
        assert SweptClearance.from_c(out[k]).bits() == ref.bits() and out[k].lower_segment >= 0
    assert np.array_equal(bits(host_a), bits(ref_a)) and np.array_equal(bits(dev_a.cpu().numpy()), bits(ref_a))
    assert [SweptClearance.from_c(o).bits() for o in out2] == [SweptClearance.from_c(o).bits() for o in out]


@gpu
def test_a_session_built_from_a_device_search_on_resident_worlds():
    """Session.from_ecbs: the grids are the resident ones of a DeviceWorlds, referenced in place"""
    p, m = Param.test_sweep(), host.load_mission("mission_4agents_15.json")
    trees = [host.load_octomap(n) for n in ("empty.bt", "map5.bt", "map3.bt")]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    try:
        search = planner.ecbs_search_batch(ws, [0, 1, 2], [m] * 3, p)
        assert list(search.status) == [0, 0, 0]
        sess = planner.Session.from_ecbs(search, p)
        search.close()
        sess.run()
        records, agents = sess.swept_clearance(per_agent=True)
        assert sess.download() == [0, 0, 0]
        ref = [host.swept_clearance(ws[k].download(), m, sess.plans[k], per_agent=True) for k in range(3)]
        sess.close()
    finally:
        ws.close()
    same_records(records, [r for r, _ in ref])
    assert np.array_equal(bits(agents), bits(np.stack([a for _, a in ref]))) and all(r.uncertified == 0 and r.lower_segment >= 0 for r in records)


@gpu
def test_refusals_of_a_session():
    c = Case("c1_4agents_empty_seq2")
    sess = planner.Session([c.world], [c.mission], c.param, [c.inputs()])
    out = (A.rbp_swept_clearance * 1)()
    f = planner.lib().rbp_session_swept_clearance
    assert f(sess._h, 4, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT       # nothing has run
    sess.run(A.RBP_STAGE_CORRIDOR)
    with pytest.raises(ValueError, match="PLANNER"):
        sess.swept_clearance()                                                  # a CORRIDOR-only run
    sess.run(A.RBP_STAGE_ALL)
    assert f(sess._h, 9, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT and f(sess._h, -1, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 4, float("nan"), out, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 4, 0.5, None, None, None) == A.RBP_ERR_BAD_ARGUMENT
    with pytest.raises(ValueError, match="depth"):
        sess.swept_clearance(depth=9)
    with pytest.raises(ValueError, match="refine_below"):
        sess.swept_clearance(refine_below=float("nan"))
    assert f(sess._h, 4, 0.5, out, None, None) == A.RBP_OK and out[0].lower_segment >= 0 and out[0].status == 0
    assert f(sess._h, 0, -2.0, out, None, None) == A.RBP_OK and out[0].refined == 0 and out[0].lower_depth == 0
    sess.run(A.RBP_STAGE_CORRIDOR)
    assert f(sess._h, 4, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT       # ... and again after one
    sess.close()


@gpu
def test_the_sweep_driver_prints_the_swept_clearance_lines_of_one_call(capsys, monkeypatch):
    """sweep_device --device-swept-clearance on three maps: the report lines of the default run, then one line per map, from ONE
    Session.swept_clearance(); the lines say what host.swept_clearance says of the downloaded plans on the downloaded grids"""
    from swarm_simulator_amd import sweep_device
    base = ["--device-worlds", "--device-ecbs", "--mission", "mission_16agents_15.json", "--maps", "2-4", "--mode", "batched"]
    calls = {"swept_clearance": 0, "download": 0}
    seen = []
    for name in calls:
        orig = getattr(planner.Session, name)
        monkeypatch.setattr(planner.Session, name, lambda self, *a, _o=orig, _n=name, **k: (calls.__setitem__(_n, calls[_n] + 1), seen.append(self), _o(self, *a, **k))[2])
    assert sweep_device.main(base) == 0
    plain = [l for l in capsys.readouterr().out.splitlines() if l.startswith("map")]
    assert len(plain) == 3 and calls == {"swept_clearance": 0, "download": 1}
    assert sweep_device.main(base + ["--device-swept-clearance"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("map")]
    assert calls == {"swept_clearance": 1, "download": 2} and lines[0::2] == plain and len(lines) == 6
    m, p = host.load_mission("mission_16agents_15.json"), Param.test_sweep()
    for line, i, plan in zip(lines[1::2], (2, 3, 4), seen[-1].plans):
        r = host.swept_clearance(host.load_world(f"map{i}.bt", p), m, plan)
        assert line == (f"map{i}: continuous clearance in [{r.lower_clearance:.5f} (agent {r.lower_agent} segment {r.lower_segment} piece {r.lower_piece}/{1 << r.lower_depth}), "
                        f"{r.upper_clearance:.5f} (agent {r.upper_agent} segment {r.upper_segment} piece {r.upper_piece}/{1 << r.upper_depth})]  "
                        f"uncertified {r.uncertified}  hitting {r.hitting}  outside {r.outside}  over budget {r.over_budget}  refined {r.refined}")
    with pytest.raises(SystemExit):
        sweep_device.main(["--device-worlds", "--device-swept-clearance", "--mode", "serial"])
    capsys.readouterr()


# ---- refusals that need no device (these run in the CPU leg too) ---------------------------------------------------------------
def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    plans = S.make(1, 2, [1])
    w = L.grid(1, (4, 4, 4), (0, 0, 0), 0.5)
    out = (A.rbp_swept_clearance * 1)()
    P = lambda a: A.ptr(a, A.c_double_p)
    ts = P(np.array([-1.0]))

    def worlds(**kw):
        s = w.c_struct()
        for k, v in kw.items():
            if k == "dim":
                s.dim[1] = v
            else:
                setattr(s, k, v)
        return (A.rbp_world * 1)(s)
    f = planner.lib().rbp_dev_swept_clearance
    good = dict(device=0, K=1, N=2, M=A.ptr(plans.M, A.c_int32_p), S=1, T=P(plans.T), ts=None, coef=P(plans.coef), rad=P(plans.radius), ws=worlds(), depth=4, below=0.5,
                out=out)
    for change in (dict(M=None), dict(T=None), dict(coef=None), dict(rad=None), dict(ws=None), dict(out=None), dict(depth=-1), dict(depth=9), dict(below=float("nan")),
                   dict(K=0), dict(N=0), dict(S=0), dict(ts=ts), dict(ws=worlds(res=0.0)), dict(ws=worlds(res=float("nan"))), dict(ws=worlds(dim=0)),
                   dict(ws=worlds(dim=-3)), dict(ws=worlds(dist=None))):
        a = dict(good, **change)
        rc = f(a["device"], a["K"], a["N"], a["M"], a["S"], a["T"], a["ts"], a["coef"], a["rad"], a["ws"], a["depth"], a["below"], a["out"], None)
        assert rc == A.RBP_ERR_BAD_ARGUMENT, change
        assert "rbp_dev_swept_clearance" in planner.last_error()
    g = planner.lib().rbp_session_swept_clearance
    assert g(None, 4, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT and g(None, 9, 0.5, None, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert "rbp_session_swept_clearance" in planner.last_error()
    with pytest.raises(ValueError):
        planner.swept_clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, [w], depth=9)
    with pytest.raises(ValueError):
        planner.swept_clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, [w], agent_lower=np.zeros(7))
    with pytest.raises(ValueError):
        planner.swept_clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, [w, w])
    assert planner.lib().rbp_sizeof(A.RBP_SIZEOF_SWEPT_CLEARANCE) == C.sizeof(A.rbp_swept_clearance) == 120
    assert planner.lib().rbp_abi_version() == 6 and {"rbp_session_swept_clearance", "rbp_dev_swept_clearance"} <= set(planner.EXPORTED_SYMBOLS)
