"""The report kernels (kernels/report.hip) against rbp_report_host, BIT FOR BIT: both read one text, csrc/common/report_rules.h, and these
tests are what hold the device compiler to the host's reading of it -- ratio bits, distance bits, end_time, samples and the three indices.

rbp_dev_report on synthetic seeded coefficients (tests/synth_report.py) at the smallest shapes where the kernels can still go wrong: no
pair, one pair, the wave boundary of the per-agent lanes (64 / 65), pair counts that are no multiple of the block (3, 2080, 2415), tiles
(21 samples at 64 and 65 agents, 19 at 70, 5 at 256: S.tile_of) that the samples fill exactly never, partly (50 = 21 + 21 + 8) or not once
(20 < 21), ragged missions under one stride, samples on knots and off them, scaled times, no sample and one, planted ties between pairs
and between samples in different tiles (which different workgroups take), a minimum in the last sample of the last tile, a NaN, more
samples than are evaluated, the reference's own 64-agent log.  rbp_session_report on real small sessions against host.report of the
downloaded plans.  The refusals that need no device run in the CPU leg too (they carry no gpu mark)."""
import ctypes as C
import os

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import Param, PlanResult
from tests import synth_report as S
from tests.common import GOLDEN_DIR, SMALL_CASES, Case

gpu = pytest.mark.gpu


def same(dev, ref, nan_distance=False):
    """bit for bit; nan_distance: the case holds a NaN, whose payload and sign are not part of the rule -- both distances must be NaN"""
    if nan_distance:
        assert np.isnan(dev.total_flight_distance) and np.isnan(ref.total_flight_distance)
        return dev.bits()[:1] + dev.bits()[2:] == ref.bits()[:1] + ref.bits()[2:]
    return dev.bits() == ref.bits()


def check(plans, dt, nan_distance=False):
    dev = planner.report_coefs(plans.M, plans.T, plans.coef, plans.radius, plans.downwash, dt, plans.time_scale)
    ref = plans.host_reports(dt)
    assert len(dev) == plans.K
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert same(d, r, nan_distance), (k, d, r)
    return dev


def static_grid(N, M, moves=()):
    """N agents at rest on the unit grid (equal radii: every neighbouring pair ties at every sample); moves: (agent, axis, segment, slope)"""
    side = int(np.ceil(np.sqrt(N)))
    c = np.zeros((N, 3, M, 6))
    c[:, 0, :, 5], c[:, 1, :, 5], c[:, 2, :, 5] = (np.arange(N) % side)[:, None], (np.arange(N) // side)[:, None], 1.0
    for a, k, m, slope in moves:
        c[a, k, m, 4] = slope
    return S.Plans([M], S.times("unit", M)[None, :], [c.reshape(N, 3, 6 * M)], np.full((1, N), 0.25))


def test_the_shapes_below_are_the_ones_the_kernel_takes_other_paths_at():
    assert [S.tile_of(N) for N in (1, 2, 3, 64, 65, 70, 256, 1365, 1366)] == [64, 64, 64, 21, 21, 19, 5, 1, 0]
    assert 50 % 21 and 50 % 19 and 20 < 21 and 50 > 2 * 21   # samples of M = 5 / M = 2 at dt = 0.1 against the tiles
    assert [N * (N - 1) // 2 % 256 for N in (3, 65, 70)] == [3, 32, 111]


@gpu
@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 64, 65, 70])
def test_agent_counts_and_segment_counts(N, M):
    dev = check(S.make(100 * N + M, N, [M]), 0.1)
    assert dev[0].samples == 10 * M and (dev[0].min_qi >= 0) == (N > 1)


@gpu
@pytest.mark.parametrize("dt", [0.1, 0.25, 0.07])
@pytest.mark.parametrize("N", [3, 64])
def test_ragged_missions_scaled_times_and_sample_steps(N, dt):
    """K = 3 under one stride: M = 1, 5, 2; unit, 0.5 / 1.7 and alternating times; time scales 1, 1.1, 1.1^4"""
    plans = S.make(7 * N, N, [1, 5, 2], ["unit", "nonunit", "alternating"], [1.0, 1.1, 1.4641])
    dev = check(plans, dt)
    ends = [plans.T[0, 1], plans.T[1, 5] * 1.1, plans.T[2, 2] * 1.4641]
    assert abs(plans.T[1, 5] - 4.9) < 1e-12 and plans.T[2, 2] == 1.5
    assert [d.end_time for d in dev] == ends
    assert [d.samples for d in dev] == [int(np.floor(e / dt)) for e in ends]


@gpu
@pytest.mark.parametrize("dt,samples", [(2.0, 0), (0.6, 1)])
def test_no_sample_and_one_sample(dt, samples):
    dev = check(S.make(11, 5, [1]), dt)
    assert dev[0].samples == samples and dev[0].total_flight_distance == 0.0
    assert (dev[0].min_safety_ratio == 1e9 and dev[0].min_sample == -1) if samples == 0 else dev[0].min_sample == 0


@gpu
def test_more_samples_than_are_evaluated():
    plans = S.make(12, 3, [1])
    plans.T[0, 1] = 2000.0
    dev = check(plans, 1e-3)
    assert (dev[0].samples, dev[0].min_safety_ratio, dev[0].total_flight_distance, dev[0].min_sample, dev[0].end_time) == (-1, 1e9, 0.0, -1, 2000.0)


@gpu
@pytest.mark.parametrize("N", [4, 66])
def test_ties_between_pairs_and_between_samples_report_the_first(N):
    """agents at rest on the unit grid: every neighbouring pair has ratio 2 at every one of 50 samples, in every tile and workgroup"""
    dev = check(static_grid(N, 5), 0.1)
    assert (dev[0].min_safety_ratio, dev[0].min_sample, dev[0].min_qi, dev[0].min_qj, dev[0].total_flight_distance) == (2.0, 0, 0, 1, 0.0)


@gpu
def test_a_minimum_in_the_last_sample_of_the_last_tile():
    """agent 5 moves towards agent 4 during the last segment only: the minimum is at sample 49, the 8th of the third tile"""
    dev = check(static_grid(64, 5, [(5, 0, 4, -0.4)]), 0.1)
    assert (dev[0].samples, dev[0].min_sample, dev[0].min_qi, dev[0].min_qj) == (50, 49, 4, 5)
    assert dev[0].min_safety_ratio < 2.0


@gpu
def test_a_nan_coefficient_is_never_the_minimum():
    plans = S.make(13, 5, [2])
    plans.coefs[0][0, 1, 6 + 3] = np.nan   # agent 0, y, second segment
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    dev = check(plans, 0.1, nan_distance=True)
    assert dev[0].min_safety_ratio < 1e9 and dev[0].min_qi >= 0


@gpu
def test_the_reference_log():
    g = np.load(os.path.join(GOLDEN_DIR, "ref_log_coef.npz"))
    coef = np.ascontiguousarray(g["coef"][..., 5::-1].transpose(0, 2, 1, 3).reshape(64, 3, 216))
    m = host.load_mission("mission_64agents_15.json")
    plans = S.Plans([36], np.arange(37.0)[None, :], [coef], m.radius[None, :])
    dev = check(plans, 0.1)
    assert abs(dev[0].min_safety_ratio - 1.0019) < 2e-3 and dev[0].samples == 360


@gpu
def test_256_agents_take_tiles_of_five_samples():
    dev = check(S.make(14, 256, [2]), 0.1)
    assert dev[0].samples == 20 and dev[0].min_qj > dev[0].min_qi >= 0


# ---- sessions ------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("T", "coef", "ctrl", "sfc_count", "sfc_box", "sfc_time", "rsfc_time")


def snapshot(plans):
    return [[getattr(p, n).copy() for n in OUTPUTS] + [p.time_scale, p.total_cost] for p in plans]


def session_check(worlds, missions, param, plans, run="run"):
    """plan, report, and compare with host.report of the downloaded plans; the download is the same before and after the report"""
    sess = planner.Session(worlds, missions, param, plans)
    getattr(sess, run)(A.RBP_STAGE_ALL)
    if run == "run":
        st = sess.download()
        before = snapshot(plans)
    reports = sess.report()   # (after run_async: waits for the solve)
    st2 = sess.download()
    if run == "run":
        assert st2 == st
        for a, b in zip(before, snapshot(plans)):
            for x, y in zip(a, b):
                assert np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(y).view(np.uint8))
    sess.close()
    assert st2 == [0] * len(plans) and [r.status for r in reports] == st2
    for m, p, r in zip(missions, plans, reports):
        assert r.bits() == host.report(m, param, p).bits()
        assert r.end_time == p.T[-1] and r.samples > 0 and r.min_safety_ratio > 0.9
    return reports


@gpu
@pytest.mark.parametrize("name", SMALL_CASES)
def test_session_report_equals_the_host_report_of_the_download(name):
    c = Case(name)
    session_check([c.world], [c.mission], c.param, [c.inputs()])


@gpu
def test_session_report_with_a_time_scale_above_one():
    c = Case("s4_map1_seq2")
    c.mission.max_vel = c.mission.max_vel * 0.25
    plans = [c.inputs()]
    session_check([c.world], [c.mission], c.param, plans)
    assert plans[0].time_scale > 1.0


@gpu
def test_session_report_of_three_missions_of_different_M():
    c = Case("s4_map1_seq2")
    worlds = [host.load_world(f"map{i}.bt", c.param) for i in (1, 2, 4)]
    plans = [host.ecbs_plan(w, c.mission, c.param) for w in worlds]
    assert [p.M for p in plans] == [26, 27, 25]
    session_check(worlds, [c.mission] * 3, c.param, plans)


@gpu
def test_a_failed_mission_is_flagged_and_leaves_the_healthy_one_intact():
    """a waypoint inside an obstacle (rbp_corridor.hpp:181-187, the way tests/test_gpu_corridor_synthetic.py builds that error) beside
    the healthy mission it was made from"""
    c = Case("s4_map1_seq2")
    w, param, healthy = c.world, c.param, c.inputs()
    t = healthy.init_traj.copy()
    t[2, 5] = ((np.array(w.key_min) + np.argwhere(w.dist == 0)[0] + 0.5) * w.res).astype(np.float32)
    plans = [PlanResult(t, healthy.T), healthy]
    sess = planner.Session([w, w], [c.mission] * 2, param, plans)
    sess.run()
    st = sess.download()
    reports = sess.report()
    sess.close()
    assert st == [A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    bad = reports[0]
    assert (bad.status, bad.min_safety_ratio, bad.total_flight_distance, bad.end_time, bad.samples, bad.min_sample, bad.min_qi, bad.min_qj) == \
        (A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0.0, 0.0, 0.0, 0, -1, -1, -1)
    assert reports[1].bits() == host.report(c.mission, param, plans[1]).bits() and reports[1].samples > 0
    assert session_check([w], [c.mission], param, [c.inputs()])[0].bits() == reports[1].bits()   # ... as alone


@gpu
def test_refusals_of_a_session():
    c = Case("c1_4agents_empty_seq2")
    sess = planner.Session([c.world], [c.mission], c.param, [c.inputs()])
    out = (A.rbp_report * 1)()
    f = planner.lib().rbp_session_report
    assert f(sess._h, 0.1, out, None) == A.RBP_ERR_BAD_ARGUMENT       # nothing has run
    sess.run(A.RBP_STAGE_CORRIDOR)
    with pytest.raises(ValueError, match="PLANNER"):
        sess.report()                                                  # a CORRIDOR-only run
    sess.run(A.RBP_STAGE_ALL)
    assert f(sess._h, 0.0, out, None) == A.RBP_ERR_BAD_ARGUMENT and f(sess._h, -0.1, out, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 0.1, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 0.1, out, None) == A.RBP_OK and out[0].samples > 0
    sess.run(A.RBP_STAGE_CORRIDOR)
    assert f(sess._h, 0.1, out, None) == A.RBP_ERR_BAD_ARGUMENT       # ... and again after one
    sess.close()


@gpu
def test_report_waits_for_an_asynchronous_joint_solve():
    """16 agents, plan/sequential = false: the grid-wide solver, whose run_async returns while the solve proceeds"""
    c = Case("c2_16agents_map3")
    p = Param.test_sweep(sequential=False)
    session_check([c.world], [c.mission], p, [c.inputs()], run="run_async")


@gpu
def test_the_sweep_driver_prints_the_same_lines_from_one_report_call(capsys, tmp_path, monkeypatch):
    """sweep_device --device-report on three maps, batched and hand-off: the report lines of the default run, to the printed digits, from
    ONE Session.report() and without a download; with --csv the coefficients come down too and the files are the default run's"""
    from swarm_simulator_amd import sweep_device
    base = ["--device-worlds", "--device-ecbs", "--mission", "mission_16agents_15.json", "--maps", "2-4", "--mode", "batched"]
    lines = lambda: [l for l in capsys.readouterr().out.splitlines() if l.startswith("map") and "QP total cost" in l]
    calls = {"report": 0, "download": 0}
    for name in calls:
        orig = getattr(planner.Session, name)
        monkeypatch.setattr(planner.Session, name, lambda self, *a, _o=orig, _n=name, **k: (calls.__setitem__(_n, calls[_n] + 1), _o(self, *a, **k))[1])
    for extra in ([], ["--device-handoff"]):
        assert sweep_device.main(base + extra) == 0
        want = lines()
        assert len(want) == 3 and calls == {"report": 0, "download": 1}
        assert sweep_device.main(base + extra + ["--device-report"]) == 0
        assert lines() == want and calls == {"report": 1, "download": 1}
        calls.update(report=0, download=0)
    assert sweep_device.main(base + ["--csv", str(tmp_path / "a")]) == 0
    assert sweep_device.main(base + ["--device-report", "--csv", str(tmp_path / "b")]) == 0
    capsys.readouterr()
    for i in (2, 3, 4):
        assert open(tmp_path / "a" / f"map{i}" / "coef1.csv").read() == open(tmp_path / "b" / f"map{i}" / "coef1.csv").read()
    with pytest.raises(SystemExit):
        sweep_device.main(["--device-worlds", "--device-report", "--mode", "serial"])
    capsys.readouterr()


# ---- refusals that need no device (these run in the CPU leg too)----------------------------------------------------------------
def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    plans = S.make(1, 2, [1])
    out = (A.rbp_report * 1)()
    M, T, coef, rad = A.ptr(plans.M, A.c_int32_p), A.ptr(plans.T, A.c_double_p), A.ptr(plans.coef, A.c_double_p), A.ptr(plans.radius, A.c_double_p)
    ts = A.ptr(np.array([-1.0]), A.c_double_p)
    f = planner.lib().rbp_dev_report
    good = dict(device=0, K=1, N=2, M=M, S=1, T=T, ts=None, coef=coef, rad=rad, dw=2.0, dt=0.1, out=out)
    for change in (dict(M=None), dict(T=None), dict(coef=None), dict(rad=None), dict(out=None), dict(dt=0.0), dict(dt=-0.1), dict(dt=float("nan")),
                   dict(K=0), dict(N=0), dict(S=0), dict(dw=0.0), dict(ts=ts), dict(N=1366)):
        a = dict(good, **change)
        rc = f(a["device"], a["K"], a["N"], a["M"], a["S"], a["T"], a["ts"], a["coef"], a["rad"], a["dw"], a["dt"], a["out"])
        assert rc == A.RBP_ERR_BAD_ARGUMENT, change
        assert "rbp_dev_report" in planner.last_error()
    g = planner.lib().rbp_session_report
    assert g(None, 0.1, out, None) == A.RBP_ERR_BAD_ARGUMENT and g(None, 0.0, None, None) == A.RBP_ERR_BAD_ARGUMENT
    with pytest.raises(ValueError):
        planner.report_coefs(plans.M, plans.T, plans.coef, plans.radius, plans.downwash, dt=0.0)
    assert planner.lib().rbp_sizeof(A.RBP_SIZEOF_REPORT) == C.sizeof(A.rbp_report) == 48
