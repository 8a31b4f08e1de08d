"""The grid-wide JOINT QP (plan/sequential = false, the reference's code default: param.hpp:67, rbp_planner.hpp:857-859; kernels/jqp.hip).
Needs an MI355X.

* 8 / 16 agents: grid-wide solver == one-workgroup solver == oracle within CTRL_TOL (three solvers, two of them sharing no linear
  algebra: tile-sweep inverses + block principal pivoting here, LDL' chains + Lawson-Hanson in kernels/qp.hip);
* 32 / 64 agents: against the committed oracle vectors tests/golden/joint32_map{7,21}.npz / joint64_map{3,12,30}.npz (the oracle needs 26 s / 300 s
  on one core: tests/golden/make_joint_golden.py); 64 agents additionally certified by the independent numpy restatement on a sub-block
  of the QP (rows and variables of eight agents, everything else fixed at the answer);
* ALL 50 maps of the reference's sweep at 64 and at 32 agents, and a HELD-OUT set no solver constant was ever tuned on (two other
  64-agent missions and another 32-agent mission on ten maps each, the ICRA world): every mission polished, within CTRL_TOL of the
  oracle's certified optimum (tests/golden/joint64_sweep.npz, joint32_sweep.npz, joint_heldout.npz);
* 256 agents (BASELINE config C4's mission, joint): solved, every constraint set of the reference satisfied;
* sessions: several joint missions in one session == the one-mission calls bit for bit; a second run of a session repeats the first.
* the look-ahead sweep with the panel in a launch of its own (sessions of 1024 tiles or more per launch) == with the panel fused into the update, bit for bit.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import Param
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

CTRL_TOL = 2e-6
FEAS_TOL = 1e-8
# the whole-sweep / held-out tests: BASELINE.md 3 "parity gate: feasibility <= 1e-7" (CPLEX's own default is 1e-6).  The joint polish accepts
# a row violated by up to 5e-8 m after its last refinement round where active rows are nearly dependent (kernels/jqp_polish.inc jp_check);
# measured: one row of one map (map45, 2.5e-8 m), everything else below 1e-11
FEAS_TOL_SWEEP = 1e-7
EQ_TOL = 5e-8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _inputs(n, map_id, **pkw):
    p = Param.test_sweep(sequential=False, **pkw)
    m = host.load_mission(f"mission_{n}agents_15.json")
    w = host.load_world(f"map{map_id}.bt", p)
    init = host.ecbs_plan(w, m, p)
    return p, m, w, init


def _certify_sub_blocks(p, m, w, init, g, blocks, block=8):
    """block-coordinate optimality of the joint answer, judged by the independent numpy restatement (tests/golden/make_kkt_reference.py):
    the QP over `block` agents with every other agent frozen AT THE ANSWER (plan/sequential = true, batch_size = block, dummy = the
    answer) must have the answer's own control points as its certified optimum -- a necessary condition of joint optimality that needs
    neither solver."""
    sys.path.insert(0, GOLDEN)
    import make_kkt_reference as K
    from swarm_simulator_amd.types import PlanResult
    pr0 = PlanResult(init.init_traj, init.T)   # corridor times before timeScale (the oracle's corridor: bit-identical to the GPU's)
    assert O.corridor_update(w, m, p, pr0)[0] == 0
    assert np.array_equal(pr0.sfc_box, g.sfc_box)
    return K.certify_plan(init.T, init.init_traj, m.start, m.goal, m.radius, g.sfc_box, pr0.sfc_time, g.sfc_count, g.rsfc_normal,
                          pr0.rsfc_time, g.ctrl, True, block, (m.qn + block - 1) // block, only_batches=blocks, ctrl_before_pass=g.ctrl)


def _plan(p, m, w, init, wide, **opts):
    """one mission through the two stage calls; wide: the grid-wide solver (rbp_solver_opts.joint_wide_min_agents = 2) / one workgroup (0)"""
    ctx = planner.Context(opts=planner.solver_opts(joint_wide_min_agents=2 if wide else 0, **opts))
    g = init.clone_inputs()
    assert planner.Corridor(w, m, p, ctx).update(False, g)
    pl = planner.RBPPlanner(m, p, ctx)
    assert pl.update(False, g), pl.last_error
    ctx.close()
    return g


@pytest.mark.parametrize("n,map_id", [(8, 5), (16, 3)])
def test_grid_wide_vs_one_workgroup_vs_oracle(n, map_id):
    p, m, w, init = _inputs(n, map_id)
    ref = init.clone_inputs()
    assert O.corridor_update(w, m, p, ref)[0] == 0
    rc, rep = O.planner_update(m, p, ref)
    assert rc == 0 and rep["n_polished"] == 1
    wide = _plan(p, m, w, init, True)
    one = _plan(p, m, w, init, False)
    assert wide.qp_solves == 1 and wide.qp_unpolished == 0 and wide.kkt_max < 1e-9
    for g in (wide, one):
        assert np.abs(ref.ctrl - g.ctrl).max() < CTRL_TOL
        assert abs(ref.total_cost - g.total_cost) <= 1e-8 * max(1.0, abs(ref.total_cost))
        obj, veq, vbox, vrs = O.evaluate_ctrl(m, g)
        assert veq < EQ_TOL and vbox < FEAS_TOL and vrs < FEAS_TOL
    assert np.abs(wide.ctrl - one.ctrl).max() < CTRL_TOL


@pytest.mark.parametrize("n,map_id", [(32, 7), (32, 21), (64, 3), (64, 12), (64, 30)])
def test_grid_wide_vs_committed_oracle_vector(n, map_id):
    gold = np.load(os.path.join(GOLDEN, f"joint{n}_map{map_id}.npz"))
    p, m, w, init = _inputs(n, map_id)
    assert hashlib.sha256(np.ascontiguousarray(init.init_traj).tobytes()).hexdigest() == str(gold["init_traj_sha256"])
    g = _plan(p, m, w, init, True)
    assert g.M == int(gold["M"]) and g.qp_solves == 1
    assert g.qp_unpolished == 0 and g.kkt_max < 1e-9
    assert np.abs(gold["ctrl"] - g.ctrl).max() < CTRL_TOL
    assert abs(float(gold["total_cost"]) - g.total_cost) <= 1e-8 * max(1.0, abs(g.total_cost))
    obj, veq, vbox, vrs = O.evaluate_ctrl(m, g)
    assert veq < EQ_TOL and vbox < FEAS_TOL and vrs < FEAS_TOL
    if n == 64 and map_id == 3:
        for rep in _certify_sub_blocks(p, m, w, init, g, [0, 3, 7]):
            tag = f"agents {8 * rep['batch']}..: " + ", ".join(f"{k}={v:.3g}" for k, v in rep.items() if isinstance(v, float))
            assert rep["x_as_viol_ineq"] < 1e-7 and rep["x_as_viol_eq"] < 1e-8 and rep["stationarity"] < 1e-7, tag
            assert rep["forward_error"] < CTRL_TOL, tag


@pytest.mark.parametrize("map_id", [41, 44])
def test_joint_64_maps_that_lose_the_dual_residual(map_id):
    """maps 41 and 44 of the sweep: past mu ~ 1e-8 one interior-point step costs the dual residual five orders of magnitude (explicit
    inverses at Newton weights of 1e9) and, depending on last-bit differences of the build, the method then crawled for a hundred
    iterations or ran out of rounds.  The safeguard of jq_ctrl(1) takes that step back and answers with the iterate before it: the
    mission is solved within a normal iteration count, feasible, with a small reported KKT residual (polished or not)."""
    p, m, w, init = _inputs(64, map_id)
    g = _plan(p, m, w, init, True)
    assert g.qp_solves == 1 and g.qp_iterations <= 60
    assert g.kkt_max < 2e-7
    obj, veq, vbox, vrs = O.evaluate_ctrl(m, g)
    assert veq < EQ_TOL and vbox < FEAS_TOL and vrs < FEAS_TOL
    assert abs(obj - g.total_cost) <= 1e-9 * max(1.0, obj)


def test_joint_centrality_corrector_saves_iterations():
    """one Gondzio corrector per iteration (on by default; rbp_solver_opts.joint_corrector = 0 switches it off): fewer iterations, the same optimum"""
    p, m, w, init = _inputs(64, 3)
    plain = _plan(p, m, w, init, True, joint_corrector=0)
    corr = _plan(p, m, w, init, True, joint_corrector=1)
    assert corr.qp_iterations < plain.qp_iterations
    assert corr.qp_unpolished == 0 and plain.qp_unpolished == 0
    assert np.abs(corr.ctrl - plain.ctrl).max() < CTRL_TOL


def test_joint_256_agents_solved_and_feasible():
    """BASELINE config C4's mission as ONE joint QP: knot blocks of order 2304 (no mission file of this size exists upstream:
    tools/make_mission_256.py).  No oracle can follow (dense LU of order ~1e5): the reference's constraint sets judge the answer."""
    p = Param.test_sweep(sequential=False, world_x_min=-5, world_y_min=-5, world_x_max=15, world_y_max=5)
    m = host.load_mission("mission_256agents_c4.json")
    w = host.load_world("map1.bt", p)
    init = host.ecbs_plan(w, m, p)
    g = init.clone_inputs()
    assert planner.Corridor(w, m, p).update(False, g)
    pl = planner.RBPPlanner(m, p)
    assert pl.update(False, g), pl.last_error
    assert g.qp_solves == 1 and g.qp_unpolished == 0 and g.kkt_max < 1e-7
    obj, veq, vbox, vrs = O.evaluate_ctrl(m, g)
    assert veq < EQ_TOL and vbox < FEAS_TOL and vrs < FEAS_TOL
    assert abs(obj - g.total_cost) <= 1e-9 * max(1.0, obj)
    # the numpy restatement on two sub-blocks of eight agents: block-coordinate optimality of the polished answer
    for rep in _certify_sub_blocks(p, m, w, init, g, [5, 20]):
        tag = ", ".join(f"{k}={v:.3g}" for k, v in rep.items() if isinstance(v, float))
        assert rep["viol_ineq"] < 1e-7 and rep["viol_eq"] < 1e-8, tag
        assert rep["x_as_viol_ineq"] < 1e-7 and rep["stationarity"] < 1e-7 and rep["forward_error"] < CTRL_TOL, tag


def test_joint_schedules_of_the_tile_sweep_agree():
    """look-ahead (default for fewer than eight resident missions), bulk with one pivot tile per pass (jq_update_bulk + a pivot launch per
    step: the default of many resident missions) and bulk with two pivot tiles per pass (jq_pivot2 / jq_panel2 / jq_update2_bulk: opt-in) on
    the same mission: the same optimum (all polished, control points within CTRL_TOL).  The first two accumulate in the same order -- in
    practice the same bits, hence the same iteration count; the double step composes two sweep steps algebraically and rounds differently."""
    p, m, w, init = _inputs(64, 7)
    look = _plan(p, m, w, init, True, joint_schedule=1)
    bulk1 = _plan(p, m, w, init, True, joint_schedule=2)
    bulk2 = _plan(p, m, w, init, True, joint_schedule=3)
    assert look.qp_unpolished == 0 and bulk1.qp_unpolished == 0 and bulk2.qp_unpolished == 0
    assert look.qp_iterations == bulk1.qp_iterations
    assert abs(look.qp_iterations - bulk2.qp_iterations) <= 2
    for b, tol in ((bulk1, 1e-10), (bulk2, 1e-8)):  # (measured: 0 and 3.6e-10; control points 0 and 7.4e-9 m)
        assert np.abs(look.ctrl - b.ctrl).max() < CTRL_TOL
        assert abs(look.total_cost - b.total_cost) <= tol * max(1.0, look.total_cost)


@pytest.mark.parametrize("n,map_id", [(8, 5), (16, 3), (32, 7)])
def test_joint_double_step_sweep_on_even_and_odd_tile_orders(n, map_id):
    """9 N = 72 / 144 / 288 unknowns per knot = 2 / 3 / 5 tiles of 64: a double pass with no panel, a double pass followed by a single
    one, two double passes and a single one -- each against the one-pivot bulk schedule on the same mission"""
    p, m, w, init = _inputs(n, map_id)
    one = _plan(p, m, w, init, True, joint_schedule=2)
    two = _plan(p, m, w, init, True, joint_schedule=3)
    assert one.qp_unpolished == 0 and two.qp_unpolished == 0
    assert np.abs(one.ctrl - two.ctrl).max() < 1e-7   # (measured <= 1.1e-8 m: the polish's own accuracy)
    assert abs(one.total_cost - two.total_cost) <= 1e-8 * max(1.0, one.total_cost)
    assert one.qp_iterations == two.qp_iterations


def test_joint_64_session_of_six_maps_is_polished():
    """six 64-agent joint missions in one session (maps 1..6): every one ends as the KKT-certified optimum of the active-set polish.  Before
    the polish knew about TWINS (the same reduced constraint written twice: last control point of a segment = first of the next under a
    shared box face; jp_twin in kernels/jqp_polish.inc) two of these six were refused."""
    p = Param.test_sweep(sequential=False)
    m = host.load_mission("mission_64agents_15.json")
    worlds = [host.load_world(f"map{i}.bt", p) for i in range(1, 7)]
    plans = [host.ecbs_plan(w, m, p).clone_inputs() for w in worlds]
    sess = planner.Session(worlds, [m] * len(worlds), p, plans)
    sess.run(A.RBP_STAGE_ALL)
    assert sess.download() == [0] * len(worlds)
    sess.close()
    for g in plans:
        assert g.qp_solves == 1 and g.qp_unpolished == 0 and g.kkt_max < 1e-9
        obj, veq, vbox, vrs = O.evaluate_ctrl(m, g)
        assert veq < EQ_TOL and vbox < FEAS_TOL and vrs < FEAS_TOL
        assert abs(obj - g.total_cost) <= 1e-9 * max(1.0, obj)


def _golden_cases(name):
    gold = np.load(os.path.join(GOLDEN, name))
    n = len(gold["cost"])
    if "mission" in gold.files:
        cases = [(str(gold["mission"][i]), str(gold["world"][i])) for i in range(n)]
    else:  # (joint64_sweep.npz, round 4: the 64-agent mission on map1..50, agents 0, 21, 42, 63)
        cases = [("mission_64agents_15.json", f"map{i + 1}.bt") for i in range(n)]
    return gold, cases


@pytest.mark.parametrize("name", ["joint64_sweep.npz", "joint32_sweep.npz", "joint_heldout.npz"])
def test_joint_every_mission_ends_at_the_oracles_optimum(name):
    """Every joint QP ends as the KKT-certified optimum of the active-set polish, within CTRL_TOL of the oracle's certified optimum (control
    points of four agents of every mission, objective to 1e-8) -- no looser branch for refused polishes: there are none.
      joint64_sweep.npz   all 50 maps of the reference's sweep, 64 agents (tests/golden/make_joint_sweep_golden.py)
      joint32_sweep.npz   the same at 32 agents                              (tests/golden/make_joint_heldout_golden.py)
      joint_heldout.npz   HELD OUT: mission_64agents_12 / _20 / mission_32agents_12 on ten maps each and the 64-agent mission on
                          ICRA2020_64agents_presentation.bt -- inputs no constant of kernels/jqp*.hip was ever tuned on (two of these
                          cases were refused when the set was first run; what they showed -- the exchange trusting a dual model that
                          disagreed with the measured slack of an inactive row -- was fixed in the algorithm, not in a constant).
    Ten missions of the 64-agent sweep are additionally certified on one sub-block of eight agents each by the independent numpy
    restatement (block-coordinate optimality with the other 56 agents frozen at the answer)."""
    gold, cases = _golden_cases(name)
    p = Param.test_sweep(sequential=False)
    by_n = {}
    for i, (mf, wf) in enumerate(cases):
        assert int(gold["rc"][i]) == 0 and int(gold["polished"][i]) == 1, cases[i]
        by_n.setdefault(int(mf.split("_")[1].replace("agents", "")), []).append(i)
    for N, idx in sorted(by_n.items()):
        missions = [host.load_mission(cases[i][0]) for i in idx]
        worlds = [host.load_world(cases[i][1], p) for i in idx]
        inits = [host.ecbs_plan(w, m, p) for w, m in zip(worlds, missions)]
        for k, i in enumerate(idx):
            assert hashlib.sha256(np.ascontiguousarray(inits[k].init_traj).tobytes()).hexdigest() == str(gold["init_traj_sha256"][i]), cases[i]
        plans = [g.clone_inputs() for g in inits]
        sess = planner.Session(worlds, missions, p, plans)
        sess.run(A.RBP_STAGE_ALL)
        assert sess.download() == [0] * len(idx)
        sess.close()
        agents = [int(a) for a in gold["agents"]] if "agents" in gold.files else [0, N // 3, (2 * N) // 3, N - 1]
        for k, i in enumerate(idx):
            g, m = plans[k], missions[k]
            assert g.M == int(gold["M"][i]) and g.qp_solves == 1, cases[i]
            assert g.qp_unpolished == 0 and g.kkt_max < 1e-7, f"{cases[i]}: unpolished {g.qp_unpolished} kkt {g.kkt_max:.3g}"
            err = np.abs(gold["ctrl"][i][:, :, :6 * g.M] - g.ctrl[agents]).max()
            rel = abs(float(gold["cost"][i]) - g.total_cost) / max(1.0, abs(g.total_cost))
            assert err < CTRL_TOL and rel < 1e-8, f"{cases[i]}: ctrl {err:.3g} cost {rel:.3g}"
            obj, veq, vbox, vrs = O.evaluate_ctrl(m, g)
            assert veq < EQ_TOL and vbox < FEAS_TOL_SWEEP and vrs < FEAS_TOL_SWEEP, f"{cases[i]}: {veq:.3g} {vbox:.3g} {vrs:.3g}"
        if name == "joint64_sweep.npz":
            for k in range(0, len(idx), 5):  # maps 1, 6, ..., 46: one sub-block of eight agents each
                for rep in _certify_sub_blocks(p, missions[k], worlds[k], inits[k], plans[k], [(k // 5) % 8]):
                    tag = f"{cases[idx[k]]} agents {8 * rep['batch']}..: " + ", ".join(f"{a}={v:.3g}" for a, v in rep.items() if isinstance(v, float))
                    assert rep["x_as_viol_ineq"] < 1e-7 and rep["x_as_viol_eq"] < 1e-8 and rep["stationarity"] < 1e-7, tag
                    assert rep["forward_error"] < CTRL_TOL, tag


def test_joint_session_matches_one_mission_calls_and_repeats():
    p = Param.test_sweep(sequential=False)
    m = host.load_mission("mission_16agents_15.json")
    maps = [3, 9, 4]  # (M = 34, 34, 36 on these maps: a ragged session)
    worlds = [host.load_world(f"map{i}.bt", p) for i in maps]
    inits = [host.ecbs_plan(w, m, p) for w in worlds]
    singles = []
    for w, init in zip(worlds, inits):
        g = init.clone_inputs()
        assert planner.Corridor(w, m, p).update(False, g)
        assert planner.RBPPlanner(m, p).update(False, g)
        singles.append(g)
    plans = [g.clone_inputs() for g in inits]
    sess = planner.Session(worlds, [m] * len(maps), p, plans)
    runs = []
    for _ in range(2):
        sess.reset()
        sess.run(A.RBP_STAGE_ALL)
        assert sess.download() == [0] * len(maps)
        runs.append([g.ctrl.copy() for g in plans])
    sess.close()
    for a, b, s in zip(runs[0], runs[1], singles):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert np.array_equal(a.view(np.uint64), s.ctrl.view(np.uint64))


@pytest.mark.parametrize("n,map_id,copies", [(16, 3, 88), (32, 7, 36)])
def test_joint_unfused_panel_gives_the_bits_of_the_fused_one(n, map_id, copies):
    """The look-ahead sweep forms the panel Y = B P in one of two places: inside jq_update while a launch is fewer than 1024 tiles (a lone
    mission), by a jq_panel launch before it otherwise.  Both are one function (panel_rows in kernels/jqp_tile.inc), so a session of `copies`
    copies of one mission -- whose two-chain knot launches are 2 x 6 x 88 = 1056 / 2 x 15 x 36 = 1080 tiles (3 / 5 tiles per side: the
    smallest odd orders above one) -- must give every copy the control points of the mission solved alone, bit for bit, in the same
    number of iterations."""
    tri = (9 * n + 63) // 64 * ((9 * n + 63) // 64 + 1) // 2
    assert 2 * tri < 1024 <= copies * 2 * tri
    p, m, w, init = _inputs(n, map_id)
    opts = planner.solver_opts(joint_wide_min_agents=2, joint_schedule=1)
    runs = {}
    for K in (1, copies):
        runs[K] = [init.clone_inputs() for _ in range(K)]
        sess = planner.Session([w] * K, [m] * K, p, runs[K], opts=opts)
        sess.run(A.RBP_STAGE_ALL)
        assert sess.download() == [0] * K
        sess.close()
    alone = runs[1][0]
    assert alone.qp_solves == 1 and alone.qp_unpolished == 0
    for g in runs[copies]:
        assert g.qp_unpolished == 0 and g.qp_iterations == alone.qp_iterations
        assert np.array_equal(g.ctrl.view(np.uint64), alone.ctrl.view(np.uint64))


def test_joint_run_async_returns_at_once_and_gives_the_same_answer():
    """rbp_session_run_async (include/rbp.h): the grid-wide solve proceeds on the session's own thread and stream; the call returns while it
    runs, `wait` / `download` wait for it, the control points are bit-identical to the synchronous `run`, and a second session solves
    concurrently."""
    import time
    p = Param.test_sweep(sequential=False)
    m = host.load_mission("mission_32agents_15.json")
    maps = [7, 21]
    worlds = [host.load_world(f"map{i}.bt", p) for i in maps]
    inits = [host.ecbs_plan(w, m, p) for w in worlds]
    plans = [g.clone_inputs() for g in inits]
    sess = planner.Session(worlds, [m] * len(maps), p, plans)
    sess.run(A.RBP_STAGE_ALL)  # (reserves the workspace, warms the kernels up)
    assert sess.download() == [0] * len(maps)
    sync_ctrl = [g.ctrl.copy() for g in plans]
    sess.reset()
    t0 = time.perf_counter()
    sess.run(A.RBP_STAGE_ALL)
    assert sess.download() == [0] * len(maps)
    t_sync = time.perf_counter() - t0
    sess.reset()
    t0 = time.perf_counter()
    sess.run_async(A.RBP_STAGE_ALL)
    t_call = time.perf_counter() - t0
    sess.wait()
    t_all = time.perf_counter() - t0
    assert sess.download() == [0] * len(maps)
    assert t_call < 0.2 * t_sync, (t_call, t_sync)   # (measured: a few hundred microseconds against ~0.15 s)
    assert t_all > 0.5 * t_sync
    for a, g in zip(sync_ctrl, plans):
        assert np.array_equal(a.view(np.uint64), g.ctrl.view(np.uint64))
    # two sessions in flight at once; download waits for its own session's solve without an explicit wait
    plans2 = [g.clone_inputs() for g in inits]
    sess2 = planner.Session(worlds, [m] * len(maps), p, plans2)
    sess.reset()
    sess.run_async(A.RBP_STAGE_ALL)
    sess2.run_async(A.RBP_STAGE_ALL)
    assert sess2.download() == [0] * len(maps)
    assert sess.download() == [0] * len(maps)
    for a, g, g2 in zip(sync_ctrl, plans, plans2):
        assert np.array_equal(a.view(np.uint64), g.ctrl.view(np.uint64))
        assert np.array_equal(a.view(np.uint64), g2.ctrl.view(np.uint64))
    # a sequential (batch) session: run_async is run
    sess2.close()
    sess.close()
    ps = Param.test_sweep(sequential=True)
    gs = inits[0].clone_inputs()
    s3 = planner.Session([worlds[0]], [m], ps, [gs])
    s3.run_async(A.RBP_STAGE_ALL)
    s3.wait()
    assert s3.download() == [0]
    s3.close()
