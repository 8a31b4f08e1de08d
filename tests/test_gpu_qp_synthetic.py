"""The QP kernels (kernels/qp.hip qp_batch_kernel, kernels/jqp.hip) on short missions, few agents and non-unit segment times: the cases
of tests/synth_qp.py, judged by the independent KKT certificate (tests/golden/make_kkt_reference.py) at the case's own T.  Needs an MI355X.

Every other solving test feeds the kernels whole benchmark missions with T[i] = i, M = 26 .. 37.  With unit times dt^-5 and the ratio
dl / dr at every knot are 1, so a wrong exponent or an inverted ratio passes them all; here an answer computed with the wrong times is
rejected by the certificate with a forward error above 1e-3 m (condition (e) of synth_qp, checked on the CPU by test_qp_synthetic.py).

Per mission (check_mission): status 0; qp_solves = passes x batches; every QP polished, kkt_max < 1e-8; time_scale == 1 and T as uploaded,
bit for bit; the corridor equal to the oracle's (RSFC normals by their bits); check_reports(certify_plan(...)) on the kernel's control
points at FWD_TOL / FEAS_TOL / STAT_TOL; |ctrl - oracle ctrl| <= CTRL_TOL; coef against the oracle's Bernstein -> monomial map of the
kernel's own ctrl.

  test_ragged_session[N-schedule]     one session per N and schedule over its cases, each with its own M: the batch kernel
  test_solo_sessions...               each case in a session of its own (slot strides M and P in place of the session's maxima): same bits
  test_grid_wide_joint_solver[N]      N = 2, 3, 7, 16 as joint QPs on kernels/jqp.hip (its outcome stands apart from the batch kernel's)
  test_both_kernel_builds[variant]    the N = 7 sessions on the 512-thread and the 256-thread build of qp_batch_kernel
  test_time_step_end_to_end           plan/time_step = 0.5, 1, 1.7 from the ECBS front end on: T = arange(M + 1) * time_step, certified,
                                      and the same optimum (it does not depend on a uniform scale)
  test_one_shot_route[N]              Corridor + RBPPlanner for one N = 1 and one N = 3 case; N = 1 hands over a zero-length rsfc_normal
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_kkt_reference as K  # noqa: E402

from swarm_simulator_amd import _abi as A  # noqa: E402
from swarm_simulator_amd import host, planner  # noqa: E402
from swarm_simulator_amd.types import Param  # noqa: E402
from tests import oracle_lib as O  # noqa: E402
from tests import synth_qp as SQ  # noqa: E402
from tests.test_gpu_parity import CTRL_TOL  # noqa: E402
from tests.test_kkt_reference import FWD_TOL, check_reports  # noqa: E402

pytestmark = pytest.mark.gpu

COEF_TOL = 10 * CTRL_TOL * 3 ** 5   # test_planner_vs_golden's tolerance for coef
BATCH_SESSIONS = [(N, si) for N, si in SQ.SESSIONS if SQ.SCHEDULES[N][si].name != "wide"]
WIDE_SESSIONS = [(N, si) for N, si in SQ.SESSIONS if SQ.SCHEDULES[N][si].name in ("wide", "joint")]
_sid = lambda k: f"{k[0]}-{SQ.SCHEDULES[k[0]][k[1]].name}"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def run(cs, param, opts=None):
    """one session over the cases, corridor and planner: (statuses, plans)"""
    plans = [c.plan() for c in cs]
    s = planner.Session([c.world for c in cs], [c.mission for c in cs], param, plans, opts=planner.solver_opts(**opts) if opts else None)
    s.run()
    st = s.download()
    s.close()
    return st, plans


@functools.lru_cache(maxsize=None)
def ragged(N, si, wide=None, variant=0, iteration=None):
    """the session of all cases of (N, si) (run once per process, never written to).  wide: joint_wide_min_agents in place of the schedule's"""
    cs = [c for c, _ in SQ.cases(N, si)]
    opts = SQ.SCHEDULES[N][si].opts_kw()
    if wide is not None:
        opts["joint_wide_min_agents"] = wide
    if variant:
        opts["qp_variant"] = variant
    return run(cs, cs[0].param(**({} if iteration is None else {"iteration": iteration})), opts)


def check_mission(c, f, pl, before, tag, worst):
    """see the module docstring; worst[(N, kind)] = [forward error, |ctrl - oracle|] collects the figures"""
    ref = f.oracle.plan
    assert pl.qp_solves == c.qp_solves(), (tag, pl.qp_solves)
    assert pl.qp_unpolished == 0 and pl.kkt_max < 1e-8, (tag, pl.qp_unpolished, pl.kkt_max)
    assert pl.time_scale == 1.0 and np.array_equal(bits(pl.T), bits(c.T)), tag
    assert np.array_equal(pl.sfc_count, ref.sfc_count) and np.array_equal(pl.sfc_box, ref.sfc_box) and np.array_equal(pl.sfc_time, ref.sfc_time), tag
    assert np.array_equal(pl.rsfc_time, ref.rsfc_time) and np.array_equal(bits(pl.rsfc_normal), bits(ref.rsfc_normal)), tag
    reps = SQ.certify(c, pl, pl.ctrl, before)
    fwd, dctrl = max(r["forward_error"] for r in reps), float(np.abs(pl.ctrl - ref.ctrl).max())
    w = worst.setdefault((c.N, c.kind), [0.0, 0.0])
    w[0], w[1] = max(w[0], fwd), max(w[1], dctrl)
    print(f"{tag}: forward error {fwd:.2e} m, |ctrl - oracle| {dctrl:.2e} m, viol_eq {max(r['viol_eq'] for r in reps):.1e}, stationarity "
          f"{max(r['stationarity'] for r in reps):.1e}, objective excess {min(r['objective_excess'] for r in reps):.1e}, "
          f"iterations {pl.qp_iterations}, kkt_max {pl.kkt_max:.1e}")
    check_reports(reps, FWD_TOL)
    assert dctrl <= CTRL_TOL, (tag, dctrl)
    dcoef = float(np.abs(pl.coef - O.ctrl_to_coef(pl.T, pl.ctrl)).max())
    assert dcoef < COEF_TOL, (tag, dcoef)


def check_session(N, si, st, plans, tag, before=None):
    cfs = SQ.cases(N, si)
    assert st == [0] * len(cfs), (tag, st)
    worst = {}
    print()
    for i, ((c, f), pl) in enumerate(zip(cfs, plans)):
        check_mission(c, f, pl, None if before is None else before[i].ctrl, f"{c.name} {tag}", worst)
    for (n, kind), (fwd, dctrl) in sorted(worst.items()):
        print(f"WORST {tag} N={n} {kind}: forward error {fwd:.2e} m, |ctrl - oracle| {dctrl:.2e} m")


def first_pass(N, si):
    """plan/iteration = 2: certify_plan needs the control points the second pass began from -- the answer of a one-pass run of the same session"""
    if SQ.cases(N, si)[0][0].passes() == 1:
        return None
    st, plans = ragged(N, si, iteration=1)
    assert st == [0] * len(plans)
    return plans


@pytest.mark.parametrize("key", BATCH_SESSIONS, ids=_sid)
def test_ragged_session(key):
    N, si = key
    assert len({c.M for c, _ in SQ.cases(N, si)}) > 1
    st, plans = ragged(N, si)
    check_session(N, si, st, plans, "batch kernel", first_pass(N, si))


@pytest.mark.parametrize("key", BATCH_SESSIONS, ids=_sid)
def test_solo_sessions_give_the_bits_of_the_ragged_session(key):
    """what test_session_batch_equals_single_missions asserts, per case"""
    N, si = key
    st, plans = ragged(N, si)
    assert st == [0] * len(plans)
    opts = SQ.SCHEDULES[N][si].opts_kw()
    for (c, _), pl in zip(SQ.cases(N, si), plans):
        st1, (solo,) = run([c], c.param(), opts)
        assert st1 == [0], c.name
        assert np.array_equal(solo.sfc_box, pl.sfc_box) and np.array_equal(bits(solo.rsfc_normal), bits(pl.rsfc_normal)), c.name
        assert np.array_equal(solo.ctrl, pl.ctrl) and np.array_equal(solo.coef, pl.coef), c.name


@pytest.mark.parametrize("key", WIDE_SESSIONS, ids=_sid)
def test_grid_wide_joint_solver(key):
    """plan/sequential = false with joint_wide_min_agents = 2: kernels/jqp.hip, which has its own copy of dt^-5 and dl / dr"""
    N, si = key
    st, plans = ragged(N, si, wide=2)
    check_session(N, si, st, plans, "grid-wide joint solver")


@pytest.mark.parametrize("variant", [2, 4])
def test_both_kernel_builds(variant):
    """qp_batch_kernel is built twice (512 threads / 256 threads; csrc/Makefile) and picked per launch by the number of resident missions:
    a small session never takes the second by itself"""
    for si in (0, 1):
        st, plans = ragged(7, si, variant=variant)
        check_session(7, si, st, plans, f"qp_variant {variant}")


def test_time_step_end_to_end():
    """rbp_param.time_step reaches T through the ECBS front end (csrc/common/ecbs_rules.h) and the QP through T"""
    m = host.load_mission("mission_4agents_15.json")
    out = {}
    for ts in (0.5, 1.0, 1.7):
        p = Param.test_sweep(time_step=ts, time_scale=False)
        w = host.load_world("map1.bt", p)
        init = host.ecbs_plan(w, m, p)
        assert np.array_equal(init.T, np.arange(init.M + 1) * ts)
        gpu = init.clone_inputs()
        assert planner.Corridor(w, m, p).update(False, gpu)
        pl = planner.RBPPlanner(m, p)
        assert pl.update(False, gpu), pl.last_error
        assert gpu.qp_unpolished == 0 and gpu.kkt_max < 1e-8 and gpu.time_scale == 1.0 and np.array_equal(gpu.T, init.T)
        reps = K.certify_plan(gpu.T, init.init_traj, m.start, m.goal, m.radius, gpu.sfc_box, gpu.sfc_time, gpu.sfc_count, gpu.rsfc_normal, gpu.rsfc_time,
                              gpu.ctrl, p.sequential, p.batch_size, p.batch_iter)
        print(f"\ntime_step {ts}: M {init.M}, forward error {max(r['forward_error'] for r in reps):.2e} m")
        check_reports(reps, FWD_TOL)
        out[ts] = (init, gpu)
    assert np.array_equal(out[0.5][0].init_traj, out[1.0][0].init_traj) and np.array_equal(out[1.7][0].init_traj, out[1.0][0].init_traj)
    for ts in (0.5, 1.7):
        d = float(np.abs(out[ts][1].ctrl - out[1.0][1].ctrl).max())
        print(f"time_step {ts} against 1: |ctrl difference| {d:.2e} m")
        assert d <= 2 * CTRL_TOL, (ts, d)


@pytest.mark.parametrize("key", [(1, 0, 2), (3, 0, 0)], ids=["N1", "N3"])
def test_one_shot_route(key):
    """Corridor::update + RBPPlanner::update.  A mission of one agent has no pair: its rsfc_normal is a zero-length array, which the binding
    hands over as a valid pointer -- it works; a NULL rsfc_normal is the documented RBP_ERR_BAD_ARGUMENT for every N."""
    c, f = SQ.case(*key)
    p, pl = c.param(), c.plan()
    assert pl.rsfc_normal.shape == (c.N * (c.N - 1) // 2, c.M, 3)
    assert planner.Corridor(c.world, c.mission, p).update(False, pl)
    rp = planner.RBPPlanner(c.mission, p)
    assert rp.update(False, pl), rp.last_error
    print()
    check_mission(c, f, pl, None, f"{c.name} one-shot", {})
    no_normals = pl.clone()
    no_normals.rsfc_normal = None
    rp2 = planner.RBPPlanner(c.mission, p)
    assert rp2.update(False, no_normals) is False and rp2.rc == A.RBP_ERR_BAD_ARGUMENT and "needs the corridor" in rp2.last_error
