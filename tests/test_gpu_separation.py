"""The separation kernels (kernels/separation.hip) against rbp_separation_host, BIT FOR BIT: both read one text,
csrc/common/separation_rules.h, and these tests are what hold the device compiler to the host's reading of it -- every field of the struct,
indices and counters included, every pair's lower ratio, and every row the kernels must NOT touch (the pairs' arrays are pre-filled with
a sentinel on both sides and compared whole).

rbp_dev_separation on synthetic seeded coefficients (tests/synth_report.py) at the smallest shapes where the kernels can still go wrong:
no pair (N = 1), one, three, 66 (more than the 64 lanes of a wavefront) and 253 pairs, 1 / 2 / 5 segments, depth 0, 1, 3 and 8, everything
refined, the default threshold and a threshold that sends exactly one item through the work list; three missions of different M under one
stride with time scales 1 / 1.21 / 0.9; the pairs' array on the host and as a device tensor; the crossing that the samples miss; identical
agents; NaN coefficients.  rbp_session_separation on planned sessions against host.separation of the downloaded plans.  The refusals that
need no device run in the CPU leg too (they carry no gpu mark)."""
import ctypes as C

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import Param, PlanResult, Separation
from tests import synth_report as S
from tests import synth_separation as X
from tests.common import Case

gpu = pytest.mark.gpu
SENTINEL = -7.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_records(dev, ref):
    assert len(dev) == len(ref)
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert d.bits() == r.bits(), (k, d, r)


def check(plans, depth, refine_below):
    """rbp_dev_separation into a sentinel-filled host array against rbp_separation_host into one filled alike: records, and the array
    whole.  Returns (device records, pairs [K][N (N-1) / 2])."""
    ref, ref_pairs = X.host_separations(plans, depth, refine_below, SENTINEL)
    dev_pairs = np.full(ref_pairs.shape, SENTINEL)
    dev = planner.separation_coefs(plans.M, plans.T, plans.coef, plans.radius, plans.downwash, depth, refine_below, plans.time_scale, dev_pairs)
    same_records(dev, ref)
    assert np.array_equal(bits(dev_pairs), bits(ref_pairs))
    without = planner.separation_coefs(plans.M, plans.T, plans.coef, plans.radius, plans.downwash, depth, refine_below, plans.time_scale)
    same_records(without, ref)
    return dev, dev_pairs


def gentle(plans):
    """the same missions with every coefficient but the constant one a tenth: the depth-0 bounds are then tight, positive and all different"""
    coefs = [c.copy() for c in plans.coefs]
    for c, M in zip(coefs, plans.M):
        c.reshape(plans.N, 3, M, 6)[..., :5] *= 0.1
    return S.Plans(plans.M, plans.T, coefs, plans.radius, plans.time_scale, plans.downwash)


def one_item_threshold(plans):
    """a refine_below that sends exactly the item with the smallest depth-0 lower ratio of mission 0 to `depth`: one double above it"""
    (r, *_), _ = X.host_separations(plans, 0, 1e9)
    below = float(np.nextafter(r.lower_ratio, np.inf))
    assert r.lower_ratio > 0 and X.host_separations(plans, 3, below)[0][0].refined == 1
    return below


def test_the_shapes_below_are_the_ones_the_kernels_take_other_paths_at():
    items = {(N, M): N * (N - 1) // 2 * M for N in (1, 2, 3, 12, 23) for M in (1, 2, 5)}
    assert items[(1, 5)] == 0 and items[(2, 1)] == 1 and items[(12, 1)] == 66 and items[(23, 5)] == 1265   # none, one lane, two wavefronts, five workgroups
    assert [(items[(N, 5)] + 255) // 256 for N in (3, 12, 23)] == [1, 2, 5]


@gpu
@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 12, 23])
def test_agent_counts_segment_counts_depths_and_thresholds(N, M):
    plans = S.make(100 * N + M, N, [M], "nonunit", spread=0.5)
    items = N * (N - 1) // 2 * M
    for depth in (0, 1, 3, 8):
        for below in (1e9, 2.0):
            (d,), pairs = check(plans, depth, below)
            if N == 1:
                assert (d.lower_ratio, d.upper_ratio, d.lower_segment, d.upper_qj, d.lower_depth, d.refined, d.uncertified) == (1e9, 1e9, -1, -1, -1, 0, 0)
                continue
            assert d.lower_ratio <= d.upper_ratio and d.refined == (items if below == 1e9 else d.refined) and pairs.min() == d.lower_ratio
        if N > 1:   # exactly one item through the work list
            calm = gentle(plans)
            (d,), _ = check(calm, depth, one_item_threshold(calm))
            assert d.refined == 1


@gpu
@pytest.mark.parametrize("depth,below", [(0, 1e9), (3, 2.0), (8, 1e9), (4, 1.3)])
def test_three_ragged_missions_under_one_stride_with_scaled_times(depth, below):
    plans = S.make(70, 6, [1, 5, 2], ["unit", "nonunit", "alternating"], [1.0, 1.21, 0.9], stride=7, spread=0.5)
    dev, _ = check(plans, depth, below)
    assert [d.end_time for d in dev] == [plans.scaled_T(k)[-1] for k in range(3)]
    assert [d.refined <= 15 * M for d, M in zip(dev, (1, 5, 2))] == [True] * 3 and all(d.lower_segment < M for d, M in zip(dev, (1, 5, 2)))


@gpu
def test_a_host_and_a_device_pair_lower_give_the_same_bytes():
    import torch
    plans = S.make(24, 23, [5, 1, 2], spread=0.5)
    for depth, below in ((3, 2.0), (1, 1e9)):
        _, pairs_host = check(plans, depth, below)
        t = torch.full((3, 253), SENTINEL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        dev = planner.separation_coefs(plans.M, plans.T, plans.coef, plans.radius, plans.downwash, depth, below, None, t)
        same_records(dev, X.host_separations(plans, depth, below)[0])
        assert np.array_equal(bits(t.cpu().numpy()), bits(pairs_host))


def as_plans(mission, plan, downwash=2.0):
    return S.Plans([plan.M], np.asarray(plan.T)[None, :], [plan.coef.reshape(plan.N, 3, 6 * plan.M)], mission.radius[None, :], downwash=downwash)


@gpu
def test_the_crossing_that_the_samples_miss():
    mission, plan = X.crossing()
    (d,), _ = check(as_plans(mission, plan), 4, 2.0)
    sampled = planner.report_coefs([1], np.asarray(plan.T)[None, :], plan.coef, mission.radius[None, :], 2.0, 0.1)[0]
    assert sampled.min_safety_ratio > 1.3 and d.upper_ratio < 1 and d.colliding >= 1 and d.lower_ratio <= 0.1 / 0.3 <= d.upper_ratio


@gpu
@pytest.mark.parametrize("depth", [0, 2, 8])
def test_identical_agents(depth):
    plans = S.make(5, 3, [3], "nonunit")
    plans.coefs[0][1] = plans.coefs[0][0]
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    (d,), pairs = check(plans, depth, 2.0)
    assert (d.lower_ratio, d.upper_ratio, d.colliding, d.lower_segment, d.lower_piece, d.lower_qi, d.lower_qj) == (0.0, 0.0, 3, 0, 0, 0, 1) and pairs[0, 0] == 0.0


@gpu
def test_nan_coefficients_are_never_a_minimum():
    plans = S.make(13, 5, [2], spread=0.5)
    plans.coefs[0][0, 1, 6 + 3] = np.nan    # agent 0, y, second segment
    plans.coefs[0][3, 0, 2] = np.inf        # agent 3, x, first segment
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    for depth, below in ((2, 1e9), (3, 2.0)):
        (d,), pairs = check(plans, depth, below)
        assert np.isfinite(d.lower_ratio) and np.all(np.isfinite(pairs))
    plans.coefs[0][:, 0, :] = np.nan        # ... and with nothing but NaN there is no minimum
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius)
    (d,), pairs = check(plans, 2, 2.0)
    assert (d.lower_ratio, d.upper_ratio, d.lower_qi, d.upper_piece, d.refined) == (1e9, 1e9, -1, -1, 20) and np.all(pairs == 1e9)


# ---- sessions ------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("T", "coef", "ctrl", "sfc_count", "sfc_box", "sfc_time", "rsfc_time")


def snapshot(plans):
    return [[getattr(p, n).copy() for n in OUTPUTS] + [p.time_scale, p.total_cost] for p in plans]


@pytest.fixture(scope="module")
def smoke_mission():
    """the 8 agents of mission_64agents_15 on map1 that __graft_entry__.smoke plans"""
    p = Param.test_sweep()
    m = host.load_mission("mission_64agents_15.json").subset([0, 16, 32, 48, 8, 24, 40, 56])
    w = host.load_world("map1.bt", p)
    return w, m, p, host.ecbs_plan(w, m, p)


@gpu
@pytest.mark.parametrize("variant", [2, 4])
def test_session_separation_equals_the_host_separation_of_the_download(smoke_mission, variant):
    w, m, p, init = smoke_mission
    plans = [init.clone_inputs()]
    sess = planner.Session([w], [m], p, plans, opts=planner.solver_opts(qp_variant=variant))
    sess.run(A.RBP_STAGE_ALL)
    st = sess.download()
    before = snapshot(plans)
    records, pairs = sess.separation(depth=4, per_pair=True)
    plain, none = sess.separation(depth=4)
    every, _ = sess.separation(depth=4, refine_below=1e9)
    on_dev, pairs_dev = sess.separation(depth=4, per_pair=True, device_out=True)
    sampled = [sess.report(dt)[0].min_safety_ratio for dt in (0.1, 0.037)]
    assert sess.download() == st == [0]
    sess.close()
    for a, b in zip(before, snapshot(plans)):
        for x, y in zip(a, b):
            assert np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(y).view(np.uint8))
    ref, ref_pairs = host.separation(m, p, plans[0], 4, 2.0, per_pair=True)
    same_records(records, [ref]), same_records(plain, records), same_records(on_dev, records)
    same_records(every, [host.separation(m, p, plans[0], 4, 1e9)])
    assert none is None and np.array_equal(bits(pairs[0]), bits(ref_pairs)) and np.array_equal(bits(pairs_dev.cpu().numpy()), bits(pairs))
    r = records[0]
    assert r.lower_ratio <= min(sampled) and r.lower_ratio <= r.upper_ratio and r.end_time == plans[0].T[-1] and r.status == 0
    assert every[0].refined == 28 * plans[0].M and r.refined <= every[0].refined
    print(f"variant {variant}: continuous ratio in [{r.lower_ratio!r}, {r.upper_ratio!r}], sampled {sampled}, refined {r.refined} of {every[0].refined}")


@gpu
def test_a_failed_mission_in_the_middle_is_flagged_and_left_alone():
    """a waypoint inside an obstacle (the way tests/test_gpu_clearance.py builds that error) between two copies of the healthy mission"""
    import torch
    c = Case("s4_map1_seq2")
    w, param, first, last = c.world, c.param, c.inputs(), c.inputs()
    t = first.init_traj.copy()
    t[2, 5] = ((np.array(w.key_min) + np.argwhere(w.dist == 0)[0] + 0.5) * w.res).astype(np.float32)
    plans = [first, PlanResult(t, first.T), last]
    sess = planner.Session([w] * 3, [c.mission] * 3, param, plans)
    sess.run()
    st = sess.download()
    out, out2 = (A.rbp_separation * 3)(), (A.rbp_separation * 3)()
    host_p = np.full((3, 6), SENTINEL)
    assert planner.lib().rbp_session_separation(sess._h, 3, 2.0, out, C.c_void_p(host_p.ctypes.data), None) == A.RBP_OK
    dev_p = torch.full((3, 6), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert planner.lib().rbp_session_separation(sess._h, 3, 2.0, out2, C.c_void_p(dev_p.data_ptr()), None) == A.RBP_OK
    sess.close()
    assert st == [0, A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    assert [getattr(out[1], n) for n, _ in A.rbp_separation._fields_] == [0.0, 0.0, 0.0, 0, 0, 0] + [-1] * 10 + [A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    ref_p = np.full((3, 6), SENTINEL)
    for k in (0, 2):
        ref, ref_p[k] = host.separation(c.mission, param, plans[k], 3, 2.0, per_pair=True)
        assert Separation.from_c(out[k]).bits() == ref.bits() and out[k].lower_segment >= 0
    assert np.array_equal(bits(host_p), bits(ref_p)) and np.array_equal(bits(dev_p.cpu().numpy()), bits(ref_p))
    assert [Separation.from_c(o).bits() for o in out2] == [Separation.from_c(o).bits() for o in out]


@gpu
def test_refusals_of_a_session():
    c = Case("c1_4agents_empty_seq2")
    sess = planner.Session([c.world], [c.mission], c.param, [c.inputs()])
    out = (A.rbp_separation * 1)()
    f = planner.lib().rbp_session_separation
    assert f(sess._h, 4, 2.0, out, None, None) == A.RBP_ERR_BAD_ARGUMENT       # nothing has run
    sess.run(A.RBP_STAGE_CORRIDOR)
    with pytest.raises(ValueError, match="PLANNER"):
        sess.separation()                                                       # a CORRIDOR-only run
    sess.run(A.RBP_STAGE_ALL)
    for depth, below in ((9, 2.0), (-1, 2.0), (4, 0.0), (4, -1.0), (4, float("nan"))):
        assert f(sess._h, depth, below, out, None, None) == A.RBP_ERR_BAD_ARGUMENT, (depth, below)
    assert f(sess._h, 4, 2.0, None, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 4, 2.0, out, None, None) == A.RBP_OK and out[0].lower_segment >= 0 and out[0].status == 0
    sess.run(A.RBP_STAGE_CORRIDOR)
    assert f(sess._h, 4, 2.0, out, None, None) == A.RBP_ERR_BAD_ARGUMENT       # ... and again after one
    sess.close()


@gpu
def test_the_sweep_driver_prints_the_separation_lines_of_one_call(capsys, monkeypatch):
    """sweep_device --device-separation on two maps: the report lines of the default run, then one separation line per map, from ONE
    Session.separation(); the lines say what host.separation says of the downloaded plans"""
    from swarm_simulator_amd import sweep_device
    base = ["--device-worlds", "--device-ecbs", "--mission", "mission_16agents_15.json", "--maps", "2-3", "--mode", "batched"]
    calls, seen = {"separation": 0}, []
    orig = planner.Session.separation
    monkeypatch.setattr(planner.Session, "separation", lambda self, *a, **k: (calls.__setitem__("separation", calls["separation"] + 1), seen.append(self), orig(self, *a, **k))[2])
    assert sweep_device.main(base + ["--device-separation"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("map")]
    assert calls == {"separation": 1} and len(lines) == 4
    m, p = host.load_mission("mission_16agents_15.json"), Param.test_sweep()
    for line, i, plan in zip(lines[1::2], (2, 3), seen[-1].plans):
        s = host.separation(m, p, plan)
        assert line.startswith(f"map{i}: continuous safety ratio in [{s.lower_ratio:.5f} (agents {s.lower_qi} {s.lower_qj} segment {s.lower_segment} piece {s.lower_piece}/{1 << s.lower_depth}), ")
        assert line.endswith(f"uncertified {s.uncertified}  colliding {s.colliding}  refined {s.refined}")
    with pytest.raises(SystemExit):
        sweep_device.main(["--device-worlds", "--device-separation", "--mode", "serial"])
    capsys.readouterr()


# ---- refusals that need no device (these run in the CPU leg too) ---------------------------------------------------------------
def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    plans = S.make(1, 2, [1])
    out = (A.rbp_separation * 1)()
    P = lambda a: A.ptr(a, A.c_double_p)
    ts = P(np.array([-1.0]))
    f = planner.lib().rbp_dev_separation
    good = dict(device=0, K=1, N=2, M=A.ptr(plans.M, A.c_int32_p), S=1, T=P(plans.T), ts=None, coef=P(plans.coef), rad=P(plans.radius), dw=2.0, depth=4, below=2.0, out=out)
    for change in (dict(M=None), dict(T=None), dict(coef=None), dict(rad=None), dict(out=None), dict(depth=9), dict(depth=-1), dict(below=0.0), dict(below=-2.0),
                   dict(below=float("nan")), dict(K=0), dict(N=0), dict(S=0), dict(ts=ts), dict(dw=0.0), dict(dw=float("nan"))):
        a = dict(good, **change)
        rc = f(a["device"], a["K"], a["N"], a["M"], a["S"], a["T"], a["ts"], a["coef"], a["rad"], a["dw"], a["depth"], a["below"], a["out"], None)
        assert rc == A.RBP_ERR_BAD_ARGUMENT, change
        assert "rbp_dev_separation" in planner.last_error()
    g = planner.lib().rbp_session_separation
    assert g(None, 4, 2.0, out, None, None) == A.RBP_ERR_BAD_ARGUMENT and g(None, 4, 2.0, None, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert "rbp_session_separation" in planner.last_error()
    with pytest.raises(ValueError):
        planner.separation_coefs(plans.M, plans.T, plans.coef, plans.radius, 2.0, depth=9)
    with pytest.raises(ValueError):
        planner.separation_coefs(plans.M, plans.T, plans.coef, plans.radius, 2.0, pair_lower=np.zeros(7))
    assert planner.lib().rbp_sizeof(A.RBP_SIZEOF_SEPARATION) == C.sizeof(A.rbp_separation) == 96
    assert planner.lib().rbp_abi_version() == 6 and {"rbp_session_separation", "rbp_dev_separation"} <= set(planner.EXPORTED_SYMBOLS)
    assert A.RBP_SEPARATION_MAX_DEPTH == 8
