"""The limits kernels (kernels/limits.hip) against rbp_limits_host, BIT FOR BIT: both read one text, csrc/common/limits_rules.h, and these
tests are what hold the device compiler to the host's reading of it -- every field of the struct, indices and counters included, every
agent's two upper ratios, and every row the kernels must NOT touch (the agents' arrays are pre-filled with a sentinel on both sides and
compared whole).

rbp_dev_limits on synthetic seeded coefficients (tests/synth_report.py) and seeded limits at the smallest shapes where the kernels change
path (tests/synth_limits.GPU_SHAPES): one item in one lane; N = 5 under a stride of 13 with missions of M = 13, 7 and 1 in one call (65 item
slots: inactive slots m >= M and a second wavefront of one item); N = 64, M = 2 (two full wavefronts) -- each at depth 0, 1, 3 (eight
items per round of the refine kernel), 6 (one item per wavefront) and 8 (four pieces per lane), with everything refined, nothing refined,
and a threshold that leaves both kinds of item in the first wavefront (tests/test_limits_host.py checks that on the CPU); ties between
identical agents and identical segments; NaN and infinite coefficients; a host against a device agent_upper, and none.
rbp_session_limits on a real small session against limits_coefs and host.limits of the downloaded plans, with a failed mission in the
middle, a NaN limit (the session does not refuse limits; rbp_dev_limits does), and against the peaks of Session.dynamics at dt = 0.01.  The
refusals that need no device run in the CPU leg too (they carry no gpu mark)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import Limits, PlanResult
from tests import synth_limits as X
from tests import synth_report as S
from tests.common import Case

gpu = pytest.mark.gpu
SENTINEL = -7.0
DEPTHS = [0, 1, 3, 6, 8]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_records(dev, ref):
    assert len(dev) == len(ref)
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert d.bits() == r.bits(), (k, d, r)


def check(plans, mv, ma, depth, above):
    """rbp_dev_limits into a sentinel-filled host array against rbp_limits_host into one filled alike: records, and the array whole; and
    the same records with no array.  Returns (device records, agents [K][N][2])."""
    ref, ref_agents = X.host_limits(plans, mv, ma, depth, above, SENTINEL)
    dev_agents = np.full((plans.K, plans.N, 2), SENTINEL)
    dev = planner.limits_coefs(plans.M, plans.T, plans.coef, mv, ma, depth, above, plans.time_scale, dev_agents)
    same_records(dev, ref)
    assert np.array_equal(bits(dev_agents), bits(ref_agents))
    same_records(planner.limits_coefs(plans.M, plans.T, plans.coef, mv, ma, depth, above, plans.time_scale), ref)
    return dev, dev_agents


def test_the_shapes_below_are_the_ones_the_kernels_take_other_paths_at():
    slots = {name: N * max(Ms) for name, (N, Ms, _, _) in X.GPU_SHAPES.items()}
    assert slots == {"one_lane": 1, "across_a_wave": 65, "two_full_waves": 128}
    assert [min(1 << d, 64) for d in DEPTHS] == [1, 2, 8, 64, 64] and [(1 << d) // min(1 << d, 64) for d in DEPTHS] == [1, 1, 1, 1, 4]


@gpu
@pytest.mark.parametrize("name", sorted(X.GPU_SHAPES))
def test_shapes_depths_and_thresholds(name):
    plans, mv, ma, part = X.gpu_case(name)
    for depth in DEPTHS:
        for above in [-1.0, 1e9] + ([part] if part is not None else []):
            dev, agents = check(plans, mv, ma, depth, above)
            for k, r in enumerate(dev):
                items = plans.N * int(plans.M[k])
                assert r.status == 0 and r.end_time == plans.scaled_T(k)[-1]
                assert r.upper_vel_ratio == agents[k, :, 0].max() and r.upper_acc_ratio == agents[k, :, 1].max()
                assert 0 < r.lower_vel_ratio <= r.upper_vel_ratio and 0 < r.lower_acc_ratio <= r.upper_acc_ratio
                if above == -1.0:
                    assert r.refined == items and r.upper_vel_depth == depth
                elif above == 1e9:
                    assert r.refined == 0 and r.upper_vel_depth == 0
                else:
                    assert (0 < r.refined < items) or items == 1   # (both kinds in one wavefront: the partial ballot)


@gpu
def test_ties_between_identical_agents_and_identical_segments_name_the_first():
    """two agents with the same coefficients and limits, two identical segments: y = 0.25 t^2 + 0.125 t, so the velocity 0.125 + 0.5 t peaks
    at the end of a segment (the last piece) and the acceleration 0.5 is the same on every piece (the first)"""
    N, M = 2, 2
    c = np.zeros((N, 3, M, 6))
    c[:, 1, :, 3], c[:, 1, :, 4] = 0.25, 0.125
    plans = S.Plans([M], S.times("unit", M)[None, :], [c.reshape(N, 3, 6 * M)], np.full((1, N), 0.15))
    mv, ma = np.ones((1, N, 3)), np.ones((1, N, 3))
    for depth in (1, 3, 6, 8):
        for above, D in ((-1.0, depth), (1e9, 0)):
            (r,), agents = check(plans, mv, ma, depth, above)
            last = (1 << D) - 1
            assert (r.upper_vel_segment, r.upper_vel_piece, r.upper_vel_agent, r.upper_vel_axis, r.upper_vel_depth) == (0, last, 0, 1, D)
            assert (r.lower_vel_segment, r.lower_vel_piece, r.lower_vel_agent, r.lower_vel_axis, r.lower_vel_depth) == (0, last, 0, 1, D)
            assert (r.upper_acc_segment, r.upper_acc_piece, r.upper_acc_agent, r.upper_acc_axis, r.upper_acc_depth) == (0, 0, 0, 1, D)
            assert (r.lower_acc_segment, r.lower_acc_piece, r.lower_acc_agent, r.lower_acc_axis, r.lower_acc_depth) == (0, 0, 0, 1, D)
            assert r.lower_vel_ratio <= 0.625 <= r.upper_vel_ratio and r.lower_acc_ratio <= 0.5 <= r.upper_acc_ratio
            assert (r.uncertified, r.violating) == (0, 0) and np.all(agents[0, 0] == agents[0, 1])


@gpu
def test_nan_and_infinite_coefficients_count_as_on_the_host():
    plans, mv, ma, part = X.gpu_case("across_a_wave")
    plans.coefs[0][0, 1, 6 + 3] = np.nan    # mission 0: agent 0, y, second segment
    plans.coefs[0][3, 0, 2] = np.inf        # agent 3, x, first segment
    plans.coefs[1][4, 2, 5 * 6 + 1] = -np.inf   # mission 1: agent 4, z, sixth segment
    plans = S.Plans(plans.M, plans.T, plans.coefs, plans.radius, plans.time_scale)
    for depth in DEPTHS:
        for above in (-1.0, 1e9, part):
            dev, agents = check(plans, mv, ma, depth, above)
            assert dev[0].uncertified >= 2 and dev[1].uncertified >= 1 and dev[0].refined >= 2 and dev[1].refined >= 1
            assert np.isinf(agents[0, 0]).any() and np.isinf(agents[0, 3]).any() and np.isinf(agents[1, 4]).any() and not np.isnan(agents).any()
            assert np.isinf(dev[0].upper_vel_ratio) and dev[0].upper_vel_agent == 3


@gpu
def test_a_host_and_a_device_agent_upper_give_the_same_bytes():
    import torch
    plans, mv, ma, part = X.gpu_case("across_a_wave")
    for depth, above in ((3, part), (8, -1.0)):
        _, agents_host = check(plans, mv, ma, depth, above)
        t = torch.full((plans.K, plans.N, 2), SENTINEL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        dev = planner.limits_coefs(plans.M, plans.T, plans.coef, mv, ma, depth, above, plans.time_scale, t)
        same_records(dev, X.host_limits(plans, mv, ma, depth, above)[0])
        assert np.array_equal(bits(t.cpu().numpy()), bits(agents_host))


# ---- sessions ------------------------------------------------------------------------------------------------------------------
def limits_of_plans(plans, missions, **kw):
    """limits_coefs on downloaded plans: T is scaled already, so no time scale; a mission's coefficients [N][3][6 M] at the front of its slot"""
    M = [p.M for p in plans]
    S_, N = max(M), plans[0].N
    T = np.zeros((len(plans), S_ + 1))
    coef = np.zeros((len(plans), N * 3 * 6 * S_))
    for k, p in enumerate(plans):
        T[k, :p.M + 1] = p.T
        coef[k, :N * 3 * 6 * p.M] = np.asarray(p.coef).reshape(-1)
    return planner.limits_coefs(M, T, coef, np.stack([m.max_vel for m in missions]), np.stack([m.max_acc for m in missions]), **kw)


@gpu
@pytest.mark.parametrize("rule", [0, 1])
def test_session_limits_equal_the_host_s_and_limits_coefs_of_the_download(rule):
    c = Case("s4_map1_seq2")
    c.mission.max_vel = c.mission.max_vel * 0.25   # (a time scale above one: the plans sit on the ladder)
    param = dataclasses.replace(c.param, timescale_rule=rule)
    plans = [c.inputs()]
    sess = planner.Session([c.world], [c.mission], param, plans)
    sess.run(A.RBP_STAGE_ALL)
    assert sess.download() == [0]
    before = (plans[0].coef.copy(), plans[0].T.copy(), [r.bits() for r in sess.report()])
    records, agents = sess.limits(per_agent=True)
    plain, none = sess.limits()
    on_dev, agents_dev = sess.limits(per_agent=True, device_out=True)
    every, _ = sess.limits(depth=8, refine_above=-1.0)
    coarse, _ = sess.limits(depth=0, refine_above=1e9)
    fine, _, _ = sess.dynamics(dt=0.01)
    assert sess.download() == [0]
    after = (plans[0].coef.copy(), plans[0].T.copy(), [r.bits() for r in sess.report()])
    sess.close()
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1])) and before[2] == after[2]
    assert none is None and plans[0].time_scale > 1.0
    ref, ref_agents = host.limits(c.mission, plans[0], per_agent=True)
    same_records(records, [ref]), same_records(plain, [ref]), same_records(on_dev, [ref])
    same_records(every, [host.limits(c.mission, plans[0], 8, -1.0)]), same_records(coarse, [host.limits(c.mission, plans[0], 0, 1e9)])
    same_records(limits_of_plans(plans, [c.mission]), [ref])
    assert np.array_equal(bits(agents[0]), bits(ref_agents)) and np.array_equal(bits(agents_dev.cpu().numpy()), bits(agents))
    for name, r in (("defaults", records[0]), ("depth 8, all", every[0]), ("depth 0", coarse[0])):
        print(f"rule {rule} {name}: vel [{r.lower_vel_ratio!r}, {r.upper_vel_ratio!r}] acc [{r.lower_acc_ratio!r}, {r.upper_acc_ratio!r}] sampled "
              f"{fine[0].peak_vel_ratio!r} {fine[0].peak_acc_ratio!r} uncertified {r.uncertified} violating {r.violating} refined {r.refined}")
        # the samples' peaks are values on the curve (up to Horner's own rounding, a few tens of 2^-53 V / limit)
        assert fine[0].peak_vel_ratio <= r.upper_vel_ratio + 1e-12 * max(1.0, r.upper_vel_ratio)
        assert fine[0].peak_acc_ratio <= r.upper_acc_ratio + 1e-12 * max(1.0, r.upper_acc_ratio)
        assert r.lower_vel_ratio <= r.upper_vel_ratio and r.lower_acc_ratio <= r.upper_acc_ratio
        assert r.end_time == plans[0].T[-1] and r.status == 0 and r.upper_vel_segment >= 0


@gpu
def test_a_failed_mission_in_the_middle_is_flagged_and_left_alone_and_a_nan_limit_is_not_refused():
    """a waypoint inside an obstacle (the way tests/test_gpu_swept.py builds that error) between two copies of the healthy mission, the
    last of which has a max_acc that is no number: timeScale compares with it and scales by nothing, the limits call reports it"""
    import copy
    import torch
    c = Case("s4_map1_seq2")
    w, param, first, last = c.world, c.param, c.inputs(), c.inputs()
    t = first.init_traj.copy()
    t[2, 5] = ((np.array(w.key_min) + np.argwhere(w.dist == 0)[0] + 0.5) * w.res).astype(np.float32)
    plans = [first, PlanResult(t, first.T), last]
    odd = copy.copy(c.mission)
    odd.max_acc = c.mission.max_acc.copy()
    odd.max_acc[1, 2] = np.nan
    missions = [c.mission, c.mission, odd]
    sess = planner.Session([w] * 3, missions, param, plans)
    sess.run()
    st = sess.download()
    out, out2 = (A.rbp_limits * 3)(), (A.rbp_limits * 3)()
    host_a = np.full((3, 4, 2), SENTINEL)
    assert planner.lib().rbp_session_limits(sess._h, 4, 0.5, out, C.c_void_p(host_a.ctypes.data), None) == A.RBP_OK
    dev_a = torch.full((3, 4, 2), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert planner.lib().rbp_session_limits(sess._h, 4, 0.5, out2, C.c_void_p(dev_a.data_ptr()), None) == A.RBP_OK
    sess.close()
    assert st == [0, A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    assert [getattr(out[1], n) for n, _ in A.rbp_limits._fields_] == [0.0] * 5 + [0] * 3 + [-1] * 20 + [A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ, 0]
    ref_a = np.full((3, 4, 2), SENTINEL)
    for k in (0, 2):
        ref, ref_a[k] = host.limits(missions[k], plans[k], 4, 0.5, per_agent=True)
        assert Limits.from_c(out[k]).bits() == ref.bits() and out[k].upper_vel_segment >= 0
    assert np.array_equal(bits(host_a), bits(ref_a)) and np.array_equal(bits(dev_a.cpu().numpy()), bits(ref_a))
    assert [Limits.from_c(o).bits() for o in out2] == [Limits.from_c(o).bits() for o in out]
    # the NaN limit: its agent's items are uncertified, its upper acceleration ratio stands as +infinity, and nothing of it is a peak
    assert out[2].uncertified >= plans[2].M and host_a[2, 1, 1] == np.inf and np.isfinite(out[2].upper_acc_ratio)
    with pytest.raises(ValueError, match="positive"):
        limits_of_plans([plans[2]], [odd])


@gpu
def test_refusals_of_a_session():
    c = Case("c1_4agents_empty_seq2")
    sess = planner.Session([c.world], [c.mission], c.param, [c.inputs()])
    out = (A.rbp_limits * 1)()
    f = planner.lib().rbp_session_limits
    assert f(sess._h, 4, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT       # nothing has run
    sess.run(A.RBP_STAGE_CORRIDOR)
    with pytest.raises(ValueError, match="PLANNER"):
        sess.limits()                                                           # a CORRIDOR-only run
    sess.run(A.RBP_STAGE_ALL)
    assert f(sess._h, 9, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT and f(sess._h, -1, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 4, float("nan"), out, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert f(sess._h, 4, 0.5, None, None, None) == A.RBP_ERR_BAD_ARGUMENT
    with pytest.raises(ValueError, match="depth"):
        sess.limits(depth=9)
    with pytest.raises(ValueError, match="refine_above"):
        sess.limits(refine_above=float("nan"))
    assert f(sess._h, 4, 0.5, out, None, None) == A.RBP_OK and out[0].upper_vel_segment >= 0 and out[0].status == 0
    assert f(sess._h, 0, 1e9, out, None, None) == A.RBP_OK and out[0].refined == 0 and out[0].upper_vel_depth == 0
    sess.run(A.RBP_STAGE_CORRIDOR)
    assert f(sess._h, 4, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT       # ... and again after one
    sess.close()


@gpu
def test_the_sweep_driver_prints_the_limits_lines_of_one_call(capsys, monkeypatch):
    """sweep_device --device-limits on two maps: one line per map after its report line, from ONE Session.limits(); the lines say what
    host.limits says of the downloaded plans"""
    from swarm_simulator_amd import sweep_device
    base = ["--device-worlds", "--device-ecbs", "--mission", "mission_8agents_15.json", "--maps", "2-3", "--mode", "batched"]
    calls, seen = {"limits": 0}, []
    orig = planner.Session.limits
    monkeypatch.setattr(planner.Session, "limits", lambda self, *a, **k: (calls.__setitem__("limits", calls["limits"] + 1), seen.append(self), orig(self, *a, **k))[2])
    assert sweep_device.main(base + ["--device-limits"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("map")]
    assert calls == {"limits": 1} and len(lines) == 4
    m = host.load_mission("mission_8agents_15.json")
    for line, i, plan in zip(lines[1::2], (2, 3), seen[-1].plans):
        r = host.limits(m, plan)
        assert line.startswith(f"map{i}: continuous velocity ratio in [{r.lower_vel_ratio:.5f}, {r.upper_vel_ratio:.5f} (agent {r.upper_vel_agent} axis {r.upper_vel_axis} "
                               f"segment {r.upper_vel_segment} piece {r.upper_vel_piece}/{1 << r.upper_vel_depth})]  acceleration ratio in [{r.lower_acc_ratio:.5f}, ")
        assert line.endswith(f"uncertified {r.uncertified}  violating {r.violating}  refined {r.refined}")
    with pytest.raises(SystemExit):
        sweep_device.main(["--device-worlds", "--device-limits", "--mode", "serial"])
    capsys.readouterr()


# ---- refusals that need no device (these run in the CPU leg too) ---------------------------------------------------------------
def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    plans = S.make(1, 2, [1])
    mv, ma = X.random_limits(1, 1, 2)
    out = (A.rbp_limits * 1)()
    P = lambda a: A.ptr(a, A.c_double_p)
    ts = P(np.array([-1.0]))

    def limit(value):
        a = mv.copy()
        a[0, 1, 2] = value
        return a
    keep = [limit(v) for v in (0.0, -1.0, float("nan"))]   # (kept alive: the calls below take their addresses)
    f = planner.lib().rbp_dev_limits
    good = dict(device=0, K=1, N=2, M=A.ptr(plans.M, A.c_int32_p), S=1, T=P(plans.T), ts=None, coef=P(plans.coef), mv=P(mv), ma=P(ma), depth=4, above=0.5, out=out)
    for change in (dict(M=None), dict(T=None), dict(coef=None), dict(mv=None), dict(ma=None), dict(out=None), dict(depth=-1), dict(depth=9), dict(above=float("nan")),
                   dict(K=0), dict(N=0), dict(S=0), dict(ts=ts), dict(mv=P(keep[0])), dict(ma=P(keep[1])), dict(mv=P(keep[2])), dict(ma=P(keep[2]))):
        a = dict(good, **change)
        rc = f(a["device"], a["K"], a["N"], a["M"], a["S"], a["T"], a["ts"], a["coef"], a["mv"], a["ma"], a["depth"], a["above"], a["out"], None)
        assert rc == A.RBP_ERR_BAD_ARGUMENT, change
        assert "rbp_dev_limits" in planner.last_error()
    g = planner.lib().rbp_session_limits
    assert g(None, 4, 0.5, out, None, None) == A.RBP_ERR_BAD_ARGUMENT and g(None, 9, 0.5, None, None, None) == A.RBP_ERR_BAD_ARGUMENT
    assert "rbp_session_limits" in planner.last_error()
    with pytest.raises(ValueError):
        planner.limits_coefs(plans.M, plans.T, plans.coef, mv, ma, depth=9)
    with pytest.raises(ValueError):
        planner.limits_coefs(plans.M, plans.T, plans.coef, mv, ma, agent_upper=np.zeros(7))
    header = open(A.REPO_ROOT + "/include/rbp.h").read()
    assert "RBP_SIZEOF_LIMITS = 13" in header and A.RBP_SIZEOF_LIMITS == 13
    assert planner.lib().rbp_sizeof(A.RBP_SIZEOF_LIMITS) == C.sizeof(A.rbp_limits) == 152
    assert planner.lib().rbp_abi_version() == 6 and {"rbp_session_limits", "rbp_dev_limits"} <= set(planner.EXPORTED_SYMBOLS)
