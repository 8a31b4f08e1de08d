"""Short missions, few agents and non-unit segment times for the QP kernels (kernels/qp.hip qp_batch_kernel, kernels/jqp.hip).
TEST INFRASTRUCTURE ONLY: a plain module imported by test_qp_synthetic.py (CPU: the cases keep their promises) and
test_gpu_qp_synthetic.py (GPU: the kernels' answers are certified optima of these cases).

Every other solving test starts from whole benchmark missions with T[i] = i, M = 26 .. 37 and the mission file's agent counts.  A case
here is CUT from a committed golden: the first M + 1 waypoints of a subset of its agents, the goal set to the last kept waypoint, planned
on the golden's own world with segment durations of the case's kind and plan/time_scale off (kernels/traj.hip has exact tests of its own,
tests/synth_traj.py).

  N and schedule   SCHEDULES: N = 1; 2 with batches of 1 and of 4; 3 with batches of 2 (a short last batch of one); 4; 7 with batches of 4
                   (4 + 3) and 8 (one batch of 7, batch_size > N); 8 with batches of 3 (3, 3, 2); 11; 16 as one joint QP on one workgroup
                   and with batches of 8 in two Gauss-Seidel passes -- nb = 1 .. 4 (rows in wave registers, the unrolled pair-row
                   prefetch), 5 .. 8 (tiles in LDS), >= 9 (tiles in global memory); N = 2, 3, 7 also as joint QPs for the grid-wide solver
  M                2, 3, 4, 5, 6, 9: 1, 2, 3, 4, 5 and 8 interior knots -- every remainder of the knot factor's 4-column panels, one full
                   panel and two
  durations        KINDS: uniform 0.5 and 1.7 (the optimum does not move under a uniform scale: these test conditioning), random in
                   [0.5, 2] and [0.5, 4], alternating 2 / 0.5.  Nothing outside [0.5, 4] and no neighbours beyond 1 : 8: past that the
                   CPU oracle stops being a reference (DESIGN.md "QP kernels on synthetic cases")

The judge is tests/golden/make_kkt_reference.py (certify_plan): independent of the oracle and of the kernels.  A case is admitted only if
    (a) the oracle's corridor and planner return 0 with every QP polished,
    (b) the certificate accepts the oracle's answer (FEAS_TOL, STAT_TOL of test_kkt_reference.py),
    (c) the oracle is within FWD_TOL / 10 of the certified optimum: the reference uses a tenth of the budget, the kernel gets the rest,
    (d) non-uniform kinds: the optimum lies at least MOVE_MIN from the oracle's optimum of the same case at T[i] = i,
    (e) non-uniform kinds: the certificate built at the case's T rejects that unit-time answer with a forward error above REJECT_MIN --
        an answer computed with the wrong times cannot pass (this stands in for a mutant build of the kernel).
A draw that misses one is replaced by the next seed (FIRST_SEED records where the search ends).
"""
import dataclasses
import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

from swarm_simulator_amd.types import Mission, PlanResult
from tests.common import Case

MS = (2, 3, 4, 5, 6, 9)
KINDS = ("u0.5", "u1.7", "rand2", "rand4", "alt")
MOVE_MIN, REJECT_MIN = 1e-2, 1e-3   # metres: conditions (d) and (e)
GOLDEN_OF = {1: "s4_map1_seq2", 2: "s4_map1_seq2", 3: "s4_map1_seq2", 4: "s4_map1_seq2", 7: "s8_map5_seq4", 8: "s8_map5_seq4",
             11: "c2_16agents_map3", 16: "c2_16agents_map3"}


@dataclass(frozen=True)
class Sched:
    """one session's schedule: rbp_param fields (batch_size, iteration, sequential) and rbp_solver_opts fields (joint_wide_min_agents)"""
    name: str
    param: tuple = ()
    opts: tuple = ()
    count: int = 6      # cases of the session
    ms: tuple = None    # their M (default: a walk through MS that starts at N)
    kinds: tuple = None

    def param_kw(self):
        return dict(self.param)

    def opts_kw(self):
        return dict(self.opts)


def _batch(bs, count=6, **kw):
    return Sched(f"bs{bs}" + "".join(f"_{k}{v}" for k, v in kw.items()), (("batch_size", bs),) + tuple(kw.items()), (), count)


def _joint(wide, **kw):
    return Sched("wide" if wide else "joint", (("sequential", False),), (("joint_wide_min_agents", 2 if wide else 0),), **kw)


_WIDE = dict(count=3, ms=(3, 6, 9), kinds=("rand2", "alt", "rand4"))
# the sessions of every N.  An N with two batch schedules splits eight cases between them; together they meet every M.
SCHEDULES = {1: (_batch(4),), 2: (_batch(1, 4), _batch(4, 4), _joint(True, **_WIDE)), 3: (_batch(2), _joint(True, **_WIDE)), 4: (_batch(4),),
             7: (_batch(4, 4), _batch(8, 4), _joint(True, **_WIDE)), 8: (_batch(3),), 11: (_batch(4),),
             16: (_joint(False, count=4), _batch(8, 4, iteration=2))}
NS = tuple(SCHEDULES)
SESSIONS = tuple((N, si) for N in NS for si in range(len(SCHEDULES[N])))
# the first seed of a case that meets (a)-(e) where it is not 0 (case() starts there and still checks; recorded to spare the search)
FIRST_SEED = {(7, 1, 2): 1, (11, 0, 2): 1, (16, 1, 3): 1}


def _kkt():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if d not in sys.path:
        sys.path.insert(0, d)
    import make_kkt_reference as K
    return K


def durations(rng, kind, M):
    if kind.startswith("u"):
        return np.full(M, float(kind[1:]))
    if kind == "alt":
        return np.where((np.arange(M) + int(rng.integers(2))) % 2 == 0, 2.0, 0.5)   # (either one first)
    return rng.uniform(0.5, 2.0 if kind == "rand2" else 4.0, M)


@dataclass(eq=False)
class QpCase:
    name: str
    golden: str
    sub: tuple              # agents of the golden
    M: int
    kind: str
    sched: Sched
    T: np.ndarray           # [M + 1]
    init_traj: np.ndarray   # [N][M + 1][3] float32
    mission: Mission
    base: Case
    seed: tuple = ()

    @property
    def N(self):
        return len(self.sub)

    @property
    def world(self):
        return self.base.world

    @property
    def uniform(self):
        return self.kind.startswith("u")

    def param(self, **kw):
        d = dict(time_scale=False, sequential=True, batch_size=4, batch_iter=-1, iteration=1)
        d.update(self.sched.param_kw())
        d.update(kw)
        return dataclasses.replace(self.base.param, **d)

    def plan(self, T=None):
        return PlanResult(self.init_traj.copy(), (self.T if T is None else np.asarray(T, np.float64)).copy())

    def passes(self):
        return self.param().iteration

    def qp_solves(self):
        """passes x batches (rbp_planner.hpp:140-203 with setBatch :849-872)"""
        p = self.param()
        return p.iteration * (-(-self.N // p.batch_size) if p.sequential else 1)


def make_case(golden, sub, M, dts, sched, kind="given", name=None, seed=()):
    """the cut of `golden`: agents `sub`, waypoints 0 .. M, the goal at waypoint M (at rest), segment durations `dts`"""
    base = Case(golden)
    sub = tuple(int(q) for q in sub)
    traj = np.ascontiguousarray(base.g["init_traj"][list(sub), :M + 1], np.float32)
    m = base.mission.subset(list(sub))
    goal = np.zeros((len(sub), 9))
    goal[:, :3] = traj[:, M].astype(np.float64)
    mission = Mission(m.start.copy(), goal, m.radius.copy(), m.max_vel.copy(), m.max_acc.copy())
    T = np.concatenate([[0.0], np.cumsum(np.asarray(dts, np.float64))])
    assert len(T) == M + 1
    return QpCase(name or f"{golden}_{'-'.join(map(str, sub))}_m{M}_{kind}_{sched.name}", golden, sub, M, kind, sched, T, traj, mission, base, seed)


def _spec(N, si, j):
    """(M, kind) of case j of session si of N"""
    sc = SCHEDULES[N][si]
    if sc.ms is not None:
        return sc.ms[j], sc.kinds[j]
    nbatch = sum(1 for s in SCHEDULES[N] if s.ms is None)
    g = j * nbatch + si   # the N's batch sessions take turns on one walk through MS and KINDS
    return MS[(g + N) % len(MS)], KINDS[(g + N) % len(KINDS)]


def _build(N, si, j, attempt):
    M, kind = _spec(N, si, j)
    rng = np.random.default_rng([N, si, j, attempt])
    n0 = Case(GOLDEN_OF[N]).g["init_traj"].shape[0]
    sub = np.sort(rng.choice(n0, N, replace=False))
    return make_case(GOLDEN_OF[N], sub, M, durations(rng, kind, M), SCHEDULES[N][si], kind, f"n{N}_{SCHEDULES[N][si].name}_{j}_m{M}_{kind}",
                     (N, si, j, attempt))


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's answer and the certificate
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class OracleRun:
    rc_corridor: int
    rc_planner: int
    report: dict
    plan: PlanResult
    before: np.ndarray = None   # plan/iteration = 2: the control points after the first pass (certify_plan's ctrl_before_pass)

    @property
    def ok(self):
        return self.rc_corridor == 0 and self.rc_planner == 0 and self.report["n_polished"] == self.report["n_qp"]


def run_oracle(c, T=None):
    from tests import oracle_lib as O
    p, pl = c.param(), c.plan(T)
    rc_c, _ = O.corridor_update(c.world, c.mission, p, pl)
    if rc_c:
        return OracleRun(rc_c, -1, {}, pl)
    before = None
    if p.iteration > 1:
        assert p.iteration == 2
        first = pl.clone()
        if O.planner_update(c.mission, c.param(iteration=1), first)[0]:
            return OracleRun(0, -1, {}, pl)
        before = first.ctrl.copy()
    rc_p, rep = O.planner_update(c.mission, p, pl)
    return OracleRun(rc_c, rc_p, rep, pl, before)


def certify(c, corridor, ctrl, before=None):
    """certify_plan of control points `ctrl` for case c at ITS T, on the corridor of plan `corridor`; one report per batch of the last pass"""
    p, m = c.param(), c.mission
    return _kkt().certify_plan(c.T, c.init_traj, m.start, m.goal, m.radius, corridor.sfc_box, corridor.sfc_time, corridor.sfc_count,
                               corridor.rsfc_normal, corridor.rsfc_time, ctrl, p.sequential, p.batch_size, p.batch_iter, ctrl_before_pass=before)


def accepted(reps, fwd_tol):
    """check_reports of test_kkt_reference.py as a predicate"""
    from tests.test_kkt_reference import check_reports
    try:
        check_reports(reps, fwd_tol)
    except AssertionError:
        return False
    return True


@dataclass
class Facts:
    """what conditions (a)-(e) were judged on"""
    oracle: OracleRun
    reports: list
    fwd: float                # the oracle's forward error
    n_implied: int
    n_active: int             # active rows that the equalities do not decide
    moved: float = None       # (d)
    unit_fwd: float = None    # (e)
    unit_accepted: bool = None


def facts(c):
    from tests.test_kkt_reference import FWD_TOL
    o = run_oracle(c)
    if not o.ok:
        return None
    reps = certify(c, o.plan, o.plan.ctrl, o.before)
    if not accepted(reps, FWD_TOL / 10):
        return None
    f = Facts(o, reps, max(r["forward_error"] for r in reps), sum(r["n_implied"] for r in reps), sum(r["n_active"] - r["n_implied"] for r in reps))
    if not c.uniform:
        u = run_oracle(c, np.arange(c.M + 1, dtype=np.float64))
        if not u.ok:
            return None
        f.moved = float(np.abs(u.plan.ctrl - o.plan.ctrl).max())
        ureps = certify(c, o.plan, u.plan.ctrl, o.before)
        f.unit_fwd, f.unit_accepted = max(r["forward_error"] for r in ureps), accepted(ureps, FWD_TOL)
        if f.moved < MOVE_MIN or f.unit_fwd <= REJECT_MIN or f.unit_accepted:
            return None
    return f


@functools.lru_cache(maxsize=None)
def case(N, si, j):
    """(case, facts) of case j of session si of N (built once per process, never written to): the first seed that meets (a)-(e)"""
    first = FIRST_SEED.get((N, si, j), 0)
    for attempt in range(first, first + 16):
        c = _build(N, si, j, attempt)
        f = facts(c)
        if f is not None:
            return c, f
    raise RuntimeError(f"no seed for case {N} {si} {j}")


def cases(N, si):
    return [case(N, si, j) for j in range(SCHEDULES[N][si].count)]


def all_keys():
    return [(N, si, j) for N, si in SESSIONS for j in range(SCHEDULES[N][si].count)]
