"""The clearance kernels (kernels/clearance.hip) against rbp_clearance_host, BIT FOR BIT: both read one text, csrc/common/clearance_rules.h,
and these tests are what hold the device compiler to the host's reading of it -- every field of the struct, indices and counters included,
every agent's clearance, and every row the kernels must NOT touch (the agents' arrays are pre-filled with a sentinel on both sides and
compared whole).

rbp_dev_clearance on synthetic seeded coefficients (tests/synth_report.py) over seeded grids (tests/synth_clearance.py) at the smallest shapes
where the kernels can still go wrong: agent counts around the four wavefronts of a workgroup (1 .. 5, 64, 65), 1 / 2 / 5 segments, sample
counts around the 64 lanes of a chunk (0, 1, 63, 64, 65, 129) and more than are evaluated, three sample steps under time scales 1 and 1.7,
three different grids in one call (the smallest 3 x 2 x 1, a non-cubic one with a negative key_min) and one grid shared by two missions,
plans that leave the grid through each of its six sides, ties between agents and between samples, the minimum in the last lane of the last
chunk of the last agent, NaN and infinite coefficients, a host grid against the same grid as a device tensor, a host against a device
agent_clearance.  rbp_session_clearance on real small sessions against host.clearance of the downloaded plans.  The refusals that need no
device run in the CPU leg too (they carry no gpu mark)."""
import ctypes as C

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import Clearance, DeviceWorld, Param, PlanResult, World
from tests import synth_clearance as L
from tests import synth_report as S
from tests.common import SMALL_CASES, Case

gpu = pytest.mark.gpu
SENTINEL = -7.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_records(dev, ref):
    assert len(dev) == len(ref)
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert d.bits() == r.bits(), (k, d, r)


def check(plans, worlds, dt, dev_worlds=None):
    """rbp_dev_clearance into a sentinel-filled host array against rbp_clearance_host into one filled alike: records, and the array whole.
    Returns (device records, agents [K][N])."""
    ref, ref_agents = L.host_clearances(plans, worlds, dt, SENTINEL)
    dev_agents = np.full((plans.K, plans.N), SENTINEL)
    dev = planner.clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, dev_worlds or worlds, dt, plans.time_scale, dev_agents)
    same_records(dev, ref)
    assert np.array_equal(bits(dev_agents), bits(ref_agents))
    without = planner.clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, dev_worlds or worlds, dt, plans.time_scale)
    same_records(without, ref)
    return dev, dev_agents


def forest(seed):
    """30 x 30 x 12 cells of 0.25 m from (-0.5, -0.5, 0): the synthetic agents (tests/synth_report.py: near (a % side, a // side, 0.5 .. 2),
    wandering a few decimetres) lie inside up to 7 x 7 of them, beyond that partly outside"""
    return L.grid(seed, (30, 30, 12), (-2, -2, 0), 0.25)


def at_rest(N, M, T_end, where=(0.1, 0.1, 0.1), radius=0.25):
    """N agents at rest in one point, M segments up to T_end"""
    c = np.zeros((N, 3, M, 6))
    c[:, 0, :, 5], c[:, 1, :, 5], c[:, 2, :, 5] = where
    T = np.linspace(0.0, T_end, M + 1)[None, :]
    return S.Plans([M], T, [c.reshape(N, 3, 6 * M)], np.full((1, N), radius))


def test_the_shapes_below_are_the_ones_the_kernels_take_other_paths_at():
    assert [(N + 3) // 4 for N in (1, 2, 3, 4, 5, 64, 65)] == [1, 1, 1, 1, 2, 16, 17]      # workgroups of four agents: short, full, one over
    assert [int(np.floor(e / 0.25)) for e in (0.125, 0.25, 15.75, 16.0, 16.25, 32.25)] == [0, 1, 63, 64, 65, 129]   # chunks of 64 samples


@gpu
@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 64, 65])
def test_agent_counts_and_segment_counts(N, M):
    dev, agents = check(S.make(100 * N + M, N, [M]), [forest(N + M)], 0.1)
    assert dev[0].samples == 10 * M and dev[0].min_sample >= 0 and agents[0, dev[0].min_agent] == dev[0].min_clearance == agents[0].min()
    assert (dev[0].outside > 0) == (N >= 64)


@gpu
@pytest.mark.parametrize("end,samples", [(0.125, 0), (0.25, 1), (15.75, 63), (16.0, 64), (16.25, 65), (32.25, 129)])
def test_sample_counts_around_a_chunk(end, samples):
    """5 agents (a full workgroup and a short one), slow quintics so that half a minute of flight stays near the grid"""
    plans = S.make(11, 5, [1])
    plans.coefs[0].reshape(5, 3, 1, 6)[..., :5] *= 1e-6
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    plans.T[0, 1] = end
    dev, agents = check(plans, [forest(3)], 0.25)
    assert dev[0].samples == samples
    if samples == 0:
        assert (dev[0].min_clearance, dev[0].min_dist, dev[0].min_sample, dev[0].min_agent, dev[0].hits, dev[0].outside) == (1e9, 0.0, -1, -1, 0, 0)
        assert np.all(agents == 1e9)
    else:
        assert dev[0].outside < samples * 5 and np.all(agents < 1e9)


@gpu
def test_more_samples_than_are_evaluated():
    plans = S.make(12, 3, [1, 1])
    plans.T[0, 1] = 2000.0
    dev, agents = check(plans, [forest(1), forest(2)], 1e-3)
    assert A.RBP_REPORT_MAX_SAMPLES < 2000000
    assert (dev[0].samples, dev[0].min_clearance, dev[0].min_sample, dev[0].min_agent, dev[0].hits, dev[0].end_time, dev[0].status) == (-1, 1e9, -1, -1, 0, 2000.0, 0)
    assert dev[1].samples == 1000 and np.all(agents[0] == SENTINEL) and np.all(agents[1] != SENTINEL)


@gpu
@pytest.mark.parametrize("ts", [1.0, 1.7])
@pytest.mark.parametrize("dt", [0.1, 0.25, 0.07])
def test_three_grids_ragged_missions_scaled_times_and_sample_steps(dt, ts):
    """K = 3 under one stride above every M: M = 1, 5, 2; unit, 0.5 / 1.7 and alternating times.  First on three different grids -- the
    smallest 3 x 2 x 1, a non-cubic one with a negative key_min, a third resolution --, then with one grid shared by two missions."""
    plans = S.make(70, 6, [1, 5, 2], ["unit", "nonunit", "alternating"], [ts] * 3, stride=7)
    tiny, slab, fine = L.grid(1, (3, 2, 1), (0, 0, 4), 0.3), L.grid(2, (21, 9, 14), (-3, -1, 2), 0.2), L.grid(3, (48, 40, 30), (-8, -8, 0), 0.1)
    dev, _ = check(plans, [tiny, slab, fine], dt)
    ends = [plans.scaled_T(k)[-1] for k in range(3)]
    assert [d.end_time for d in dev] == ends and [d.samples for d in dev] == [int(np.floor(e / dt)) for e in ends]
    assert dev[0].outside > 0 and dev[1].outside > 0 and dev[0].min_dist == -1.0
    shared, _ = check(plans, [fine, tiny, fine], dt)
    assert shared[2].bits() == dev[2].bits()
    if ts == 1.0:   # (unscaled, no segment lasts long enough for a quintic to leave the third grid)
        assert dev[2].outside == 0 and shared[0].outside == 0


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
    dev, agents = check(plans, [w], 0.1)
    assert np.all(agents[0, :6] == -1.125) and agents[0, 6] == 0.375
    assert (dev[0].min_clearance, dev[0].min_dist, dev[0].min_agent, dev[0].min_sample) == (-1.125, -1.0, 4, 5)   # +z leaves first: z = 0.5 + 0.5 at t = 0.5
    assert dev[0].hits == dev[0].outside and dev[0].outside > 6 * 9   # each of the six is outside for the last second at least


@gpu
@pytest.mark.parametrize("N", [4, 65])
def test_ties_between_agents_and_between_samples_report_the_first(N):
    """every agent rests in one cell with one radius through 70 samples: N x 70 equal clearances, in every lane, chunk, wavefront and
    workgroup; the first is sample 0, agent 0"""
    plans = at_rest(N, 2, 7.0)
    w = World(np.full((4, 4, 4), 0.75, np.float32), (-2, -2, -2), 0.25)
    dev, agents = check(plans, [w], 0.1)
    assert (dev[0].samples, dev[0].min_clearance, dev[0].min_dist, dev[0].min_sample, dev[0].min_agent, dev[0].hits, dev[0].outside) == (70, 0.5, 0.75, 0, 0, 0, 0)
    assert np.all(agents == 0.5)
    # ... and with the radius above the grid's value: every item a hit
    plans.radius[:] = 1.0
    dev, _ = check(plans, [w], 0.1)
    assert (dev[0].hits, dev[0].min_sample, dev[0].min_agent, dev[0].min_clearance) == (70 * N, 0, 0, -0.25)


@gpu
@pytest.mark.parametrize("N", [64, 65])
def test_the_minimum_in_the_last_lane_of_the_last_chunk_of_the_last_agent(N):
    """128 samples = two full chunks; the last agent flies along x at one cell per sample and meets the only low cell at sample 127"""
    c = np.zeros((N, 3, 1, 6))
    c[:, :, 0, 5] = 0.1
    c[N - 1, 0, 0, 4] = 1.0   # x = 0.1 + t: key floor(4 (0.1 + 0.25 j)) = j
    plans = S.Plans([1], np.array([[0.0, 32.0]]), [c.reshape(N, 3, 6)], np.full((1, N), 0.25))
    d = np.full((130, 2, 2), 1.0, np.float32)
    d[127, 0, 0] = 0.5
    dev, agents = check(plans, [World(d, (0, 0, 0), 0.25)], 0.25)
    assert (dev[0].samples, dev[0].min_sample, dev[0].min_agent, dev[0].min_clearance, dev[0].min_dist) == (128, 127, N - 1, 0.25, 0.5)
    assert np.all(agents[0, :N - 1] == 0.75) and agents[0, N - 1] == 0.25 and dev[0].hits == 0 and dev[0].outside == 0


@gpu
def test_nan_and_infinite_coefficients_are_outside():
    plans = S.make(13, 5, [2])
    plans.coefs[0][0, 1, 6 + 3] = np.nan    # agent 0, y, second segment
    plans.coefs[0][3, 0, 2] = np.inf        # agent 3, x, first segment
    plans.coefs[0][4, 2, 5] = 1e300         # agent 4, z, first segment
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    dev, agents = check(plans, [forest(5)], 0.1)
    assert dev[0].outside >= 9 + 10 + 11 and dev[0].min_dist == -1.0 and np.isfinite(dev[0].min_clearance) and np.all(np.isfinite(agents))
    plans.radius[0, 1] = np.nan             # ... and a NaN radius is never the minimum
    dev, agents = check(plans, [forest(5)], 0.1)
    assert agents[0, 1] == 1e9 and dev[0].min_agent != 1


@gpu
def test_a_host_grid_and_the_same_grid_as_a_device_tensor_give_the_same_bytes():
    import torch
    plans = S.make(23, 65, [5, 2])
    ws = [forest(8), forest(9)]
    dev_host, agents_host = check(plans, ws, 0.1)
    tensors = [torch.from_numpy(w.dist).to("cuda:0") for w in ws]
    torch.cuda.synchronize()
    dws = [DeviceWorld.from_tensor(t, w.key_min, w.res) for t, w in zip(tensors, ws)]
    dev_dev, agents_dev = check(plans, ws, 0.1, dev_worlds=dws)
    assert [d.bits() for d in dev_dev] == [d.bits() for d in dev_host] and np.array_equal(bits(agents_dev), bits(agents_host))
    mixed, agents_mixed = check(plans, ws, 0.1, dev_worlds=[dws[0], ws[1]])   # one of each
    assert np.array_equal(bits(agents_mixed), bits(agents_host))


@gpu
def test_a_host_and_a_device_agent_clearance_give_the_same_bytes():
    import torch
    plans = S.make(24, 65, [5, 1, 2])
    plans.T[1, 1] = 2000.0   # the middle mission: 20000 samples at dt = 0.1, not evaluated at dt = 1e-3 (its row keeps the sentinel)
    ws = [forest(8), forest(9), forest(10)]
    for dt in (0.1, 1e-3):
        _, agents_host = check(plans, ws, dt)
        t = torch.full((3, 65), SENTINEL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        dev = planner.clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, ws, dt, None, t)
        same_records(dev, L.host_clearances(plans, ws, dt)[0])
        assert np.array_equal(bits(t.cpu().numpy()), bits(agents_host))
    assert np.all(agents_host[1] == SENTINEL)


# ---- sessions ------------------------------------------------------------------------------------------------------------------
def session_check(worlds, missions, param, plans, run="run"):
    """plan, look the clearance up, and compare with host.clearance of the downloaded plans on the same grids"""
    sess = planner.Session(worlds, missions, param, plans)
    getattr(sess, run)(A.RBP_STAGE_ALL)
    records, agents = sess.clearance(per_agent=True)   # (after run_async: waits for the solve)
    plain, none = sess.clearance()
    on_dev, agents_dev = sess.clearance(per_agent=True, device_out=True)
    status = sess.download()
    sess.close()
    assert status == [0] * len(plans) and [r.status for r in records] == status and none is None
    ref = [host.clearance(w, m, p, 0.1, per_agent=True) for w, m, p in zip(worlds, missions, plans)]
    same_records(records, [r for r, _ in ref])
    same_records(plain, records), same_records(on_dev, records)
    assert np.array_equal(bits(agents), bits(np.stack([a for _, a in ref]))) and np.array_equal(bits(agents_dev.cpu().numpy()), bits(agents))
    assert all(r.samples > 0 and r.end_time == p.T[-1] and r.min_sample >= 0 for r, p in zip(records, plans))
    return records


@gpu
@pytest.mark.parametrize("name", SMALL_CASES)
def test_session_clearance_equals_the_host_clearance_of_the_download(name):
    c = Case(name)
    (r,) = session_check([c.world], [c.mission], c.param, [c.inputs()])
    assert (r.hits, r.outside) == (0, 0)


@gpu
def test_session_clearance_with_a_time_scale_above_one():
    c = Case("s4_map1_seq2")
    c.mission.max_vel = c.mission.max_vel * 0.25
    plans = [c.inputs()]
    session_check([c.world], [c.mission], c.param, plans)
    assert plans[0].time_scale > 1.0


@gpu
def test_session_clearance_of_three_missions_of_different_M():
    c = Case("s4_map1_seq2")
    worlds = [host.load_world(f"map{i}.bt", c.param) for i in (1, 2, 4)]
    plans = [host.ecbs_plan(w, c.mission, c.param) for w in worlds]
    assert [p.M for p in plans] == [26, 27, 25]
    session_check(worlds, [c.mission] * 3, c.param, plans)


@gpu
def test_session_clearance_waits_for_an_asynchronous_joint_solve():
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
    out, out2 = (A.rbp_clearance * 3)(), (A.rbp_clearance * 3)()
    host_a = np.full((3, 4), SENTINEL)
    assert planner.lib().rbp_session_clearance(sess._h, 0.1, out, C.c_void_p(host_a.ctypes.data), None) == A.RBP_OK
    dev_a = torch.full((3, 4), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert planner.lib().rbp_session_clearance(sess._h, 0.1, out2, C.c_void_p(dev_a.data_ptr()), None) == A.RBP_OK
    sess.close()
    assert st == [0, A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    assert [getattr(out[1], n) for n, _ in A.rbp_clearance._fields_] == [0.0, 0.0, 0.0, 0, 0, 0, -1, -1, A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ]
    ref_a = np.full((3, 4), SENTINEL)
    for k in (0, 2):
        ref, ref_a[k] = host.clearance(w, c.mission, plans[k], 0.1, per_agent=True)
        assert Clearance.from_c(out[k]).bits() == ref.bits() and out[k].samples > 0
    assert np.array_equal(bits(host_a), bits(ref_a)) and np.array_equal(bits(dev_a.cpu().numpy()), bits(ref_a))
    assert [Clearance.from_c(o).bits() for o in out2] == [Clearance.from_c(o).bits() for o in out]


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
        records, agents = sess.clearance(per_agent=True)
        assert sess.download() == [0, 0, 0]
        ref = [host.clearance(ws[k].download(), m, sess.plans[k], 0.1, per_agent=True) for k in range(3)]
        sess.close()
    finally:
        ws.close()
    same_records(records, [r for r, _ in ref])
    assert np.array_equal(bits(agents), bits(np.stack([a for _, a in ref]))) and all(r.hits == 0 and r.samples > 0 for r in records)


@gpu
def test_refusals_of_a_session():
    c = Case("c1_4agents_empty_seq2")
    sess = planner.Session([c.world], [c.mission], c.param, [c.inputs()])
    out = (A.rbp_clearance * 1)()
    f = planner.lib().rbp_session_clearance
    assert f(sess._h, 0.1, out, None, None) == A.RBP_ERR_BAD_ARGUMENT       # nothing has run
    sess.run(A.RBP_STAGE_CORRIDOR)
    with pytest.raises(ValueError, match="PLANNER"):
        sess.clearance()                                                     # a CORRIDOR-only run
    sess.run(A.RBP_STAGE_ALL)
    assert f(sess._h, 0.0, out, None, None) == A.RBP_ERR_BAD_ARGUMENT and f(sess._h, -0.1, out, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 0.1, None, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 0.1, out, None, None) == A.RBP_OK and out[0].samples > 0 and out[0].status == 0
    sess.run(A.RBP_STAGE_CORRIDOR)
    assert f(sess._h, 0.1, out, None, None) == A.RBP_ERR_BAD_ARGUMENT       # ... and again after one
    sess.close()


@gpu
def test_the_sweep_driver_prints_the_clearance_lines_of_one_call(capsys, monkeypatch):
    """sweep_device --device-clearance on three maps: the report lines of the default run, then one clearance line per map, from ONE
    Session.clearance(); the lines say what host.clearance says of the downloaded plans on the downloaded grids"""
    from swarm_simulator_amd import sweep_device
    base = ["--device-worlds", "--device-ecbs", "--mission", "mission_16agents_15.json", "--maps", "2-4", "--mode", "batched"]
    calls = {"clearance": 0, "download": 0}
    seen = []
    for name in calls:
        orig = getattr(planner.Session, name)
        monkeypatch.setattr(planner.Session, name, lambda self, *a, _o=orig, _n=name, **k: (calls.__setitem__(_n, calls[_n] + 1), seen.append(self), _o(self, *a, **k))[2])
    assert sweep_device.main(base) == 0
    plain = [l for l in capsys.readouterr().out.splitlines() if l.startswith("map")]
    assert len(plain) == 3 and calls == {"clearance": 0, "download": 1}
    assert sweep_device.main(base + ["--device-clearance"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("map")]
    assert calls == {"clearance": 1, "download": 2} and lines[0::2] == plain and len(lines) == 6
    m, p = host.load_mission("mission_16agents_15.json"), Param.test_sweep()
    for line, i, plan in zip(lines[1::2], (2, 3, 4), seen[-1].plans):
        r = host.clearance(host.load_world(f"map{i}.bt", p), m, plan)
        assert line == f"map{i}: minimum clearance {r.min_clearance:.4f} (agent {r.min_agent} sample {r.min_sample})  hits {r.hits}  outside {r.outside}  samples {r.samples}"
    with pytest.raises(SystemExit):
        sweep_device.main(["--device-worlds", "--device-clearance", "--mode", "serial"])
    capsys.readouterr()


# ---- refusals that need no device (these run in the CPU leg too) ---------------------------------------------------------------
def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    plans = S.make(1, 2, [1])
    w = L.grid(1, (4, 4, 4), (0, 0, 0), 0.5)
    out = (A.rbp_clearance * 1)()
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
    f = planner.lib().rbp_dev_clearance
    good = dict(device=0, K=1, N=2, M=A.ptr(plans.M, A.c_int32_p), S=1, T=P(plans.T), ts=None, coef=P(plans.coef), rad=P(plans.radius), ws=worlds(), dt=0.1, out=out)
    for change in (dict(M=None), dict(T=None), dict(coef=None), dict(rad=None), dict(ws=None), dict(out=None), dict(dt=0.0), dict(dt=-0.1), dict(dt=float("nan")),
                   dict(K=0), dict(N=0), dict(S=0), dict(ts=ts), dict(ws=worlds(res=0.0)), dict(ws=worlds(res=float("nan"))), dict(ws=worlds(dim=0)),
                   dict(ws=worlds(dim=-3)), dict(ws=worlds(dist=None))):
        a = dict(good, **change)
        rc = f(a["device"], a["K"], a["N"], a["M"], a["S"], a["T"], a["ts"], a["coef"], a["rad"], a["ws"], a["dt"], a["out"], None)
        assert rc == A.RBP_ERR_BAD_ARGUMENT, change
        assert "rbp_dev_clearance" in planner.last_error()
    g = planner.lib().rbp_session_clearance
    assert g(None, 0.1, out, None, None) == A.RBP_ERR_BAD_ARGUMENT and g(None, 0.0, None, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert "rbp_session_clearance" in planner.last_error()
    with pytest.raises(ValueError):
        planner.clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, [w], dt=0.0)
    with pytest.raises(ValueError):
        planner.clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, [w], agent_clearance=np.zeros(7))
    with pytest.raises(ValueError):
        planner.clearance_coefs(plans.M, plans.T, plans.coef, plans.radius, [w, w])
    assert planner.lib().rbp_sizeof(A.RBP_SIZEOF_CLEARANCE) == C.sizeof(A.rbp_clearance) == 56
    assert planner.lib().rbp_abi_version() == 6 and {"rbp_session_clearance", "rbp_dev_clearance"} <= set(planner.EXPORTED_SYMBOLS)
