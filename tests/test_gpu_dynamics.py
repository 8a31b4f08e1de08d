"""The dynamics kernels (kernels/dynamics.hip) against rbp_dynamics_host, BIT FOR BIT: both read one text, csrc/common/state_rules.h, and
these tests are what hold the device compiler to the host's reading of it -- every field of the struct, every stored state and every curve
entry, and every byte the kernels must NOT touch (buffers are pre-filled with a sentinel on both sides and compared whole).

rbp_dev_dynamics on synthetic seeded coefficients (tests/synth_report.py) with seeded limits (tests/synth_states.py) at the smallest shapes
where the kernels can still go wrong: no pair (curves 1e9 / 0), one pair, the wave boundary of the curve kernel's pair lanes, agent counts
that are no multiple of the 64 chunks the state kernel's wavefronts stride over (3, 65, 70), curve tiles (21 samples at 64 and 65 agents, 19
at 70, 5 at 256) and state chunks (64 samples) that the samples fill exactly, by one more, or not once, ragged missions under one stride with
scaled times, no sample and one, rows that hold exactly the samples, one more and one fewer, more samples than are evaluated, states only /
curves only / neither, a device destination against a host destination, planted ties between agents, axes and samples, a peak in the last
sample of the last tile, a NaN.  rbp_session_dynamics on real small sessions against host.dynamics of the downloaded plans.  The refusals that
need no device run in the CPU leg too (they carry no gpu mark)."""
import ctypes as C

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import Param, PlanResult
from tests import synth_report as S
from tests import synth_states as X
from tests.common import SMALL_CASES, Case

gpu = pytest.mark.gpu
SENTINEL = -7.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_records(dev, ref):
    assert len(dev) == len(ref)
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert d.bits() == r.bits(), (k, d, r)


def check(plans, dt, seed=0, S_stride=None, states=True, curves=True, limits=None, nan_ok=False):
    """rbp_dev_dynamics into sentinel-filled host buffers against rbp_dynamics_host into buffers filled alike: records, and both buffers
    whole.  S_stride: default the largest number of samples (at least 1).  Returns (device records, states, curves)."""
    max_vel, max_acc = limits if limits is not None else X.limits(seed, plans.K, plans.N)
    if S_stride is None:
        S_stride = max([1] + [r.samples for r in plans.host_reports(dt)])
    shape_s, shape_c = (plans.K, plans.N, 9, S_stride), (plans.K, S_stride, 2)
    ref_s, ref_c = (np.full(shape_s, SENTINEL) if states else None), (np.full(shape_c, SENTINEL) if curves else None)
    dev_s, dev_c = (np.full(shape_s, SENTINEL) if states else None), (np.full(shape_c, SENTINEL) if curves else None)
    ref = X.host_dynamics(plans, dt, max_vel, max_acc, ref_s, ref_c)
    dev = planner.dynamics_coefs(plans.M, plans.T, plans.coef, plans.radius, max_vel, max_acc, plans.downwash, dt, plans.time_scale, dev_s, dev_c, S_stride)
    same_records(dev, ref)
    for d, r in ((dev_s, ref_s), (dev_c, ref_c)):
        if d is not None:
            if nan_ok:   # (a NaN's payload and sign are not part of the rule)
                assert np.array_equal(np.isnan(d), np.isnan(r))
                d, r = np.nan_to_num(d, nan=0.0), np.nan_to_num(r, nan=0.0)
            assert np.array_equal(bits(d), bits(r))
    return dev, dev_s, dev_c


def static_grid(N, M, moves=(), radius=0.25):
    """N agents at rest on the unit grid; moves: (agent, axis, segment, slope)"""
    side = int(np.ceil(np.sqrt(N)))
    c = np.zeros((N, 3, M, 6))
    c[:, 0, :, 5], c[:, 1, :, 5], c[:, 2, :, 5] = (np.arange(N) % side)[:, None], (np.arange(N) // side)[:, None], 1.0
    for a, k, m, slope in moves:
        c[a, k, m, 4] = slope
    return S.Plans([M], S.times("unit", M)[None, :], [c.reshape(N, 3, 6 * M)], np.full((1, N), radius))


def test_the_shapes_below_are_the_ones_the_kernels_take_other_paths_at():
    assert [S.tile_of(N) for N in (1, 2, 3, 64, 65, 70, 256, 1365, 1366)] == [64, 64, 64, 21, 21, 19, 5, 1, 0]   # the curve kernel's tiles
    assert 64 * 0.25 == 16.0 and 65 * 0.25 == 16.25 and 21 * 0.25 == 5.25 and 22 * 0.25 == 5.5                  # ends of exactly that many samples
    assert [N * (N - 1) // 2 % 64 for N in (3, 65, 70)] == [3, 32, 47]                                           # pairs against a wavefront's lanes


@gpu
@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 64, 65, 70])
def test_agent_counts_and_segment_counts(N, M):
    dev, st, cu = check(S.make(100 * N + M, N, [M]), 0.1, seed=N + M)
    assert dev[0].samples == 10 * M and dev[0].stored == 1 and dev[0].vel_sample >= 0 and dev[0].acc_sample >= 0
    if N == 1:
        assert np.all(cu[0, :, 0] == 1e9) and np.all(cu[0, :, 1] == 0.0)   # no pair
    else:
        assert np.all(cu[0, :, 0] <= cu[0, :, 1]) and np.all(cu[0, :, 0] < 1e9)


@gpu
@pytest.mark.parametrize("dt", [0.1, 0.25, 0.07])
@pytest.mark.parametrize("N", [3, 64])
def test_ragged_missions_scaled_times_and_sample_steps(N, dt):
    """K = 3 under one stride above every M: M = 1, 5, 2; unit, 0.5 / 1.7 and alternating times; time scales 1, 1.1, 1.1^4.  The rows hold
    the longest mission's samples: the shorter ones leave the rest of theirs untouched."""
    plans = S.make(7 * N, N, [1, 5, 2], ["unit", "nonunit", "alternating"], [1.0, 1.1, 1.4641], stride=7)
    dev, st, cu = check(plans, dt, seed=N)
    ends = [plans.T[0, 1], plans.T[1, 5] * 1.1, plans.T[2, 2] * 1.4641]
    assert [d.end_time for d in dev] == ends and [d.samples for d in dev] == [int(np.floor(e / dt)) for e in ends]
    assert all(d.stored == 1 for d in dev) and np.all(st[0, :, :, dev[0].samples:] == SENTINEL) and np.all(cu[2, dev[2].samples:] == SENTINEL)


@gpu
@pytest.mark.parametrize("end,samples", [(0.125, 0), (0.25, 1), (5.25, 21), (5.5, 22), (16.0, 64), (16.25, 65)])
def test_no_sample_one_sample_and_samples_around_a_tile_and_a_chunk(end, samples):
    """64 agents: curve tiles of 21 samples, state chunks of 64"""
    plans = S.make(11, 64, [1])
    plans.T[0, 1] = end
    dev, st, cu = check(plans, 0.25, seed=3)
    assert dev[0].samples == samples and dev[0].stored == 1
    if samples == 0:
        assert (dev[0].peak_vel_ratio, dev[0].peak_vel, dev[0].peak_vel_limit, dev[0].vel_sample, dev[0].vel_agent, dev[0].vel_axis) == (0.0, 0.0, 0.0, -1, -1, -1)
        assert np.all(st == SENTINEL) and np.all(cu == SENTINEL)


@gpu
def test_256_agents_take_tiles_of_five_samples():
    dev, st, cu = check(S.make(14, 256, [2]), 0.1, seed=4)
    assert dev[0].samples == 20 and np.all(cu[0, :, 0] < cu[0, :, 1])


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("extra", [0, 1, -1])
def test_rows_that_hold_the_samples_exactly_one_more_and_one_fewer(extra):
    """two missions of 50 and 20 samples, 5 agents: with rows of 49 the first is not stored (stored = 0, untouched) and the second is"""
    plans = S.make(21, 5, [5, 2])
    dev, st, cu = check(plans, 0.1, seed=5, S_stride=50 + extra)
    assert [d.samples for d in dev] == [50, 20] and [d.stored for d in dev] == [0 if extra < 0 else 1, 1]
    if extra < 0:
        assert np.all(st[0] == SENTINEL) and np.all(cu[0] == SENTINEL) and dev[0].vel_sample >= 0   # ... and its peaks are still reported
    assert np.all(st[1, :, :, 20:] == SENTINEL) and np.all(st[1, :, :, :20] != SENTINEL)


@gpu
def test_more_samples_than_are_evaluated():
    plans = S.make(12, 3, [1, 1])
    plans.T[0, 1] = 2000.0
    dev, st, cu = check(plans, 1e-3, seed=6, S_stride=1000)
    assert A.RBP_REPORT_MAX_SAMPLES < 2000000
    assert (dev[0].samples, dev[0].stored, dev[0].vel_sample, dev[0].acc_sample, dev[0].peak_vel_ratio, dev[0].end_time) == (-1, 0, -1, -1, 0.0, 2000.0)
    assert (dev[1].samples, dev[1].stored) == (1000, 1) and np.all(st[0] == SENTINEL) and np.all(cu[0] == SENTINEL)


@gpu
@pytest.mark.parametrize("states,curves", [(True, False), (False, True), (False, False)])
def test_states_only_curves_only_and_neither(states, curves):
    dev, st, cu = check(S.make(22, 6, [2, 3]), 0.1, seed=7, states=states, curves=curves)
    both, _, _ = check(S.make(22, 6, [2, 3]), 0.1, seed=7)
    assert [d.stored for d in dev] == [1 if (states or curves) else 0] * 2
    assert [d.bits()[:-2] for d in dev] == [d.bits()[:-2] for d in both]


@gpu
def test_a_device_destination_and_a_host_destination_give_the_same_bytes():
    import torch
    plans = S.make(23, 65, [5, 2])
    mv, ma = X.limits(8, 2, 65)
    _, host_s, host_c = check(plans, 0.1, limits=(mv, ma), S_stride=51)
    dev_s = torch.full((2, 65, 9, 51), SENTINEL, dtype=torch.float64, device="cuda:0")
    dev_c = torch.full((2, 51, 2), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dev = planner.dynamics_coefs(plans.M, plans.T, plans.coef, plans.radius, mv, ma, plans.downwash, 0.1, None, dev_s, dev_c, 51)
    same_records(dev, X.host_dynamics(plans, 0.1, mv, ma, np.zeros((2, 65, 9, 51)), None))
    assert np.array_equal(bits(dev_s.cpu().numpy()), bits(host_s)) and np.array_equal(bits(dev_c.cpu().numpy()), bits(host_c))
    # one of each: states on the device, curves on the host
    mix_c = np.full((2, 51, 2), SENTINEL)
    dev_s.fill_(SENTINEL)
    torch.cuda.synchronize()
    planner.dynamics_coefs(plans.M, plans.T, plans.coef, plans.radius, mv, ma, plans.downwash, 0.1, None, dev_s, mix_c, 51)
    assert np.array_equal(bits(dev_s.cpu().numpy()), bits(host_s)) and np.array_equal(bits(mix_c), bits(host_c))


@gpu
def test_a_host_destination_larger_than_the_staging_goes_in_chunks_of_missions():
    """five missions under rows of 4000 samples: 18.5 MB of states and curves each against RBP_DYNAMICS_STAGE_BYTES = 64 MiB, so the
    missions are staged three and two at a time; only each mission's own samples come back, the rest of the rows keeps the sentinel"""
    per = 8 * (64 * 9 + 2) * 4000
    assert A.RBP_DYNAMICS_STAGE_BYTES // per == 3 and 5 * per > A.RBP_DYNAMICS_STAGE_BYTES
    dev, st, cu = check(S.make(31, 64, [2, 1, 3, 2, 1]), 0.1, seed=10, S_stride=4000)
    assert [d.samples for d in dev] == [20, 10, 30, 20, 10] and all(d.stored == 1 for d in dev)
    assert all(np.all(st[k, :, :, d.samples:] == SENTINEL) and np.all(cu[k, d.samples:] == SENTINEL) for k, d in enumerate(dev))


# ---- peaks -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [4, 66])
def test_ties_between_agents_axes_and_samples_report_the_first(N):
    """every agent moves alike along y and z through all five segments under equal limits: 3 N x 50 equal ratios, in every chunk, wavefront
    and workgroup; the first is sample 0, agent 0, axis 1.  A steady acceleration ties the same way."""
    moves = [(a, k, m, 0.5) for a in range(N) for k in (1, 2) for m in range(5)]
    plans = static_grid(N, 5, moves)
    plans.coefs[0].reshape(N, 3, 5, 6)[:, 2, :, 3] = 0.125   # z: + 0.125 t^2 per segment, acceleration 0.25
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    dev, st, cu = check(plans, 0.1, limits=(np.ones((1, N, 3)), np.ones((1, N, 3))))
    d = dev[0]
    assert (d.peak_acc_ratio, d.peak_acc, d.acc_sample, d.acc_agent, d.acc_axis) == (0.25, 0.25, 0, 0, 2)
    assert (d.vel_agent, d.vel_axis) == (0, 2) and d.peak_vel_ratio == st[0, 0, 5, d.vel_sample]   # z is faster than y wherever t > 0 ...
    assert np.all(st[0, :, 4, :] == 0.5) and d.peak_vel_ratio > 0.5                              # ... and y ties everywhere at 0.5


@gpu
def test_velocity_ties_report_sample_agent_axis_in_that_order():
    moves = [(a, k, m, -0.5) for a in range(70) for k in (1, 2) for m in range(5)]
    dev, st, cu = check(static_grid(70, 5, moves), 0.1, limits=(np.ones((1, 70, 3)), np.ones((1, 70, 3))))
    d = dev[0]
    assert (d.peak_vel_ratio, d.peak_vel, d.peak_vel_limit, d.vel_sample, d.vel_agent, d.vel_axis) == (0.5, -0.5, 1.0, 0, 0, 1)
    assert (d.peak_acc_ratio, d.acc_sample, d.acc_agent, d.acc_axis) == (0.0, -1, -1, -1)   # no acceleration anywhere: none


@gpu
def test_a_peak_in_the_last_sample_of_the_last_tile():
    """agent 63 accelerates along x during the last segment only: its velocity peaks at sample 49, the last of the mission"""
    plans = static_grid(64, 5)
    plans.coefs[0].reshape(64, 3, 5, 6)[63, 0, 4, 3] = -0.5
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    dev, st, cu = check(plans, 0.1, limits=(np.ones((1, 64, 3)), np.ones((1, 64, 3))))
    d = dev[0]
    assert (d.samples, d.vel_sample, d.vel_agent, d.vel_axis) == (50, 49, 63, 0) and d.peak_vel < 0
    assert (d.acc_sample, d.acc_agent, d.acc_axis, d.peak_acc) == (40 + 1, 63, 0, -1.0)   # (sample 40 lies on the knot: the earlier segment)


@gpu
def test_a_nan_coefficient_is_never_a_peak_and_never_moves_a_curve():
    plans = S.make(13, 5, [2])
    plans.coefs[0][0, 1, 6 + 3] = np.nan   # agent 0, y, second segment
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    dev, st, cu = check(plans, 0.1, seed=9, nan_ok=True)
    d = dev[0]
    assert np.isnan(st[0, 0, 1, 15]) and np.isnan(st[0, 0, 4, 15]) and np.isfinite(st[0, 0, 1, 5])
    assert np.isfinite(d.peak_vel_ratio) and np.isfinite(d.peak_acc_ratio) and d.vel_sample >= 0 and np.all(np.isfinite(cu[0]))
    assert not (d.vel_agent == 0 and d.vel_axis == 1 and d.vel_sample > 10)


# ---- sessions ------------------------------------------------------------------------------------------------------------------
def session_check(worlds, missions, param, plans, run="run"):
    """plan, sample, and compare with host.dynamics of the downloaded plans"""
    sess = planner.Session(worlds, missions, param, plans)
    getattr(sess, run)(A.RBP_STAGE_ALL)
    records, st, cu = sess.dynamics(states=True, curves=True)   # (after run_async: waits for the solve)
    peaks_only = sess.dynamics()[0]
    status = sess.download()
    sess.close()
    assert status == [0] * len(plans) and [r.status for r in records] == status
    ref_s, ref_c = np.zeros_like(st), np.zeros_like(cu)
    ref = [host.dynamics(m, param, p, 0.1, ref_s[k], ref_c[k]) for k, (m, p) in enumerate(zip(missions, plans))]
    same_records(records, ref)
    assert np.array_equal(bits(st), bits(ref_s)) and np.array_equal(bits(cu), bits(ref_c))
    assert st.shape[3] == max(r.samples for r in records) and all(r.stored == 1 and r.samples > 0 and r.end_time == p.T[-1] for r, p in zip(records, plans))
    assert [r.bits()[:-2] for r in peaks_only] == [r.bits()[:-2] for r in records] and all(r.stored == 0 for r in peaks_only)
    return records


@gpu
@pytest.mark.parametrize("name", SMALL_CASES)
def test_session_dynamics_equal_the_host_dynamics_of_the_download(name):
    c = Case(name)
    session_check([c.world], [c.mission], c.param, [c.inputs()])


@gpu
def test_session_dynamics_with_a_time_scale_above_one():
    c = Case("s4_map1_seq2")
    c.mission.max_vel = c.mission.max_vel * 0.25
    plans = [c.inputs()]
    records = session_check([c.world], [c.mission], c.param, plans)
    assert plans[0].time_scale > 1.0 and records[0].peak_vel_limit == c.mission.max_vel[records[0].vel_agent, records[0].vel_axis]


@gpu
def test_session_dynamics_of_three_missions_of_different_M():
    c = Case("s4_map1_seq2")
    worlds = [host.load_world(f"map{i}.bt", c.param) for i in (1, 2, 4)]
    plans = [host.ecbs_plan(w, c.mission, c.param) for w in worlds]
    assert [p.M for p in plans] == [26, 27, 25]
    session_check(worlds, [c.mission] * 3, c.param, plans)


@gpu
def test_session_dynamics_wait_for_an_asynchronous_joint_solve():
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
    ns = max(r.samples for r in sess.report())
    out = (A.rbp_dynamics * 3)()
    host_s, host_c = np.full((3, 4, 9, ns), SENTINEL), np.full((3, ns, 2), SENTINEL)
    assert planner.lib().rbp_session_dynamics(sess._h, 0.1, out, C.c_void_p(host_s.ctypes.data), C.c_void_p(host_c.ctypes.data), ns, None) == A.RBP_OK
    dev_s = torch.full((3, 4, 9, ns), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    out2 = (A.rbp_dynamics * 3)()
    assert planner.lib().rbp_session_dynamics(sess._h, 0.1, out2, C.c_void_p(dev_s.data_ptr()), None, ns, None) == A.RBP_OK
    sess.close()
    assert st == [0, A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    bad = out[1]
    assert [getattr(bad, n) for n, _ in A.rbp_dynamics._fields_] == [0.0] * 7 + [0, -1, -1, -1, -1, -1, -1, 0, A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ]
    assert np.all(host_s[1] == SENTINEL) and np.all(host_c[1] == SENTINEL)
    ref_s, ref_c = np.full((3, 4, 9, ns), SENTINEL), np.full((3, ns, 2), SENTINEL)
    from swarm_simulator_amd.types import Dynamics
    for k in (0, 2):
        assert Dynamics.from_c(out[k]).bits() == host.dynamics(c.mission, param, plans[k], 0.1, ref_s[k], ref_c[k]).bits() and out[k].samples > 0
    assert np.array_equal(bits(host_s), bits(ref_s)) and np.array_equal(bits(host_c), bits(ref_c))
    assert np.array_equal(bits(dev_s.cpu().numpy()), bits(ref_s)) and [Dynamics.from_c(o).bits() for o in out2] == [Dynamics.from_c(o).bits() for o in out]


@gpu
def test_refusals_of_a_session():
    c = Case("c1_4agents_empty_seq2")
    sess = planner.Session([c.world], [c.mission], c.param, [c.inputs()])
    out = (A.rbp_dynamics * 1)()
    buf = np.zeros((4, 9, 4000))
    f = planner.lib().rbp_session_dynamics
    assert f(sess._h, 0.1, out, None, None, 0, None) == A.RBP_ERR_BAD_ARGUMENT       # nothing has run
    sess.run(A.RBP_STAGE_CORRIDOR)
    with pytest.raises(ValueError, match="PLANNER"):
        sess.dynamics()                                                               # a CORRIDOR-only run
    sess.run(A.RBP_STAGE_ALL)
    assert f(sess._h, 0.0, out, None, None, 0, None) == A.RBP_ERR_BAD_ARGUMENT and f(sess._h, -0.1, out, None, None, 0, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 0.1, None, None, None, 0, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 0.1, out, C.c_void_p(buf.ctypes.data), None, 0, None) == A.RBP_ERR_BAD_ARGUMENT   # a buffer without room for a sample
    assert f(sess._h, 0.1, out, None, None, 0, None) == A.RBP_OK and out[0].samples > 0 and out[0].stored == 0
    assert f(sess._h, 0.1, out, C.c_void_p(buf.ctypes.data), None, 4000, None) == A.RBP_OK and out[0].stored == 1 and out[0].samples <= 4000
    sess.run(A.RBP_STAGE_CORRIDOR)
    assert f(sess._h, 0.1, out, None, None, 0, None) == A.RBP_ERR_BAD_ARGUMENT       # ... and again after one
    sess.close()


@gpu
def test_the_sweep_driver_prints_the_peak_lines_of_one_dynamics_call(capsys, monkeypatch):
    """sweep_device --device-dynamics on three maps: the report lines of the default run, then one peak line per map, from ONE
    Session.dynamics(); the lines say what host.dynamics says of the downloaded plans"""
    from swarm_simulator_amd import sweep_device
    base = ["--device-worlds", "--device-ecbs", "--mission", "mission_16agents_15.json", "--maps", "2-4", "--mode", "batched"]
    calls = {"dynamics": 0, "download": 0}
    seen = []
    for name in calls:
        orig = getattr(planner.Session, name)
        monkeypatch.setattr(planner.Session, name, lambda self, *a, _o=orig, _n=name, **k: (calls.__setitem__(_n, calls[_n] + 1), seen.append(self), _o(self, *a, **k))[2])
    assert sweep_device.main(base) == 0
    plain = [l for l in capsys.readouterr().out.splitlines() if l.startswith("map")]
    assert len(plain) == 3 and calls == {"dynamics": 0, "download": 1}
    assert sweep_device.main(base + ["--device-dynamics"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("map")]
    assert calls == {"dynamics": 1, "download": 2} and lines[0::2] == plain and len(lines) == 6
    m, p = host.load_mission("mission_16agents_15.json"), Param.test_sweep()
    for line, i, plan in zip(lines[1::2], (2, 3, 4), seen[-1].plans):
        d = host.dynamics(m, p, plan)
        assert line == (f"map{i}: peak velocity ratio {d.peak_vel_ratio:.4f} (agent {d.vel_agent} {'xyz'[d.vel_axis]} sample {d.vel_sample})  "
                        f"peak acceleration ratio {d.peak_acc_ratio:.4f} (agent {d.acc_agent} {'xyz'[d.acc_axis]} sample {d.acc_sample})  samples {d.samples}")
    with pytest.raises(SystemExit):
        sweep_device.main(["--device-worlds", "--device-dynamics", "--mode", "serial"])
    capsys.readouterr()


# ---- refusals that need no device (these run in the CPU leg too) ---------------------------------------------------------------
def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    plans = S.make(1, 2, [1])
    mv, ma = X.limits(1, 1, 2)
    out = (A.rbp_dynamics * 1)()
    buf = np.zeros((1, 2, 9, 10))
    P = lambda a: A.ptr(a, A.c_double_p)
    ts = P(np.array([-1.0]))
    f = planner.lib().rbp_dev_dynamics
    good = dict(device=0, K=1, N=2, M=A.ptr(plans.M, A.c_int32_p), S=1, T=P(plans.T), ts=None, coef=P(plans.coef), rad=P(plans.radius), mv=P(mv), ma=P(ma),
                dw=2.0, dt=0.1, out=out, st=None, cu=None, stride=0)
    for change in (dict(M=None), dict(T=None), dict(coef=None), dict(rad=None), dict(mv=None), dict(ma=None), dict(out=None), dict(dt=0.0), dict(dt=-0.1),
                   dict(dt=float("nan")), dict(K=0), dict(N=0), dict(S=0), dict(dw=0.0), dict(ts=ts), dict(N=1366),
                   dict(st=C.c_void_p(buf.ctypes.data), stride=0), dict(cu=C.c_void_p(buf.ctypes.data), stride=-1)):
        a = dict(good, **change)
        rc = f(a["device"], a["K"], a["N"], a["M"], a["S"], a["T"], a["ts"], a["coef"], a["rad"], a["mv"], a["ma"], a["dw"], a["dt"], a["out"], a["st"], a["cu"], a["stride"])
        assert rc == A.RBP_ERR_BAD_ARGUMENT, change
        assert "rbp_dev_dynamics" in planner.last_error()
    g = planner.lib().rbp_session_dynamics
    assert g(None, 0.1, out, None, None, 0, None) == A.RBP_ERR_BAD_ARGUMENT and g(None, 0.0, None, None, None, 0, None) == A.RBP_ERR_BAD_ARGUMENT
    with pytest.raises(ValueError):
        planner.dynamics_coefs(plans.M, plans.T, plans.coef, plans.radius, mv, ma, plans.downwash, dt=0.0)
    with pytest.raises(ValueError):
        planner.dynamics_coefs(plans.M, plans.T, plans.coef, plans.radius, mv, ma, plans.downwash, states=np.zeros(7), S_stride=10)
    assert planner.lib().rbp_sizeof(A.RBP_SIZEOF_DYNAMICS) == C.sizeof(A.rbp_dynamics) == 96
    assert planner.lib().rbp_abi_version() == 6 and "rbp_session_dynamics" in planner.EXPORTED_SYMBOLS
