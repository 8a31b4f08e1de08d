"""The batch QP's polish with the mission's K0 tables (csrc/kernels/qp_polish.inc: factor and G = K0^-1 formed once per mission, S and the
primal step read from G, no column of K0^-1 J' stored), on the short missions of tests/synth_qp.py: N = 1, 2, 3, 7, non-unit segment
times, judged by check_mission of test_gpu_qp_synthetic.py -- the KKT certificate at FWD_TOL, |ctrl - oracle| <= CTRL_TOL.  Needs an MI355X.

  test_short_missions[variant-iteration-far]
      the batch sessions of N = 1, 2, 3, 7 on both builds of qp_batch_kernel (qp_variant 2: 512 threads, 4: 256 threads), with
      plan/iteration 1 and 2 -- the second pass starts polish-first, its candidates taken from the geometry --, and once more with
      qp_far_slack = 0.15 m in place of the default: the interior-point phase then leaves out most frozen-neighbour rows, verification
      finds violated ones among them, the candidate set grows, S is extended by the new rows and columns and the dual solve resumed.
      iteration 1 is check_mission as it stands; iteration 2 has no oracle answer of its own among the cases, so it is held to the
      certificate of its second pass (certify_plan with the first pass's control points as the starting point) and to the counters.
  test_eight_agents_one_batch[variant]
      one 8-agent mission at batch_size 8: nk = 72, the LDS-resident tiled path, whose polish is the same code.

Counters, as the commit before the tables gave them for these very runs (measured there, asserted here): every session of every
(variant, iteration, far) combination ended with qp_unpolished = 0 on every mission and scalars slot 11 (second attempts: a batch QP that
did not end polished on the reduced row set and was solved again with every row) = 0 on every mission, the 8-agent mission included.
That the incremental path runs at all is asserted too: scalars slot 12 counts the dual solves that were resumed on a grown candidate
set (S extended by the new rows and columns); the sessions of every combination hold one, with either radius.  The slot is new with the
tables, the parent has no such figure."""
import functools

import numpy as np
import pytest

from swarm_simulator_amd import planner
from tests import synth_qp as SQ
from tests.test_gpu_qp_synthetic import check_mission
from tests.test_kkt_reference import FWD_TOL, check_reports

pytestmark = pytest.mark.gpu

SESSIONS = [(1, 0), (2, 0), (2, 1), (3, 0), (7, 0), (7, 1)]   # the batch schedules of N = 1, 2, 3, 7
FAR = {"default": None, "far0.15": 0.15}
SECOND_ATTEMPTS = 11                                            # scalars slot: SC_PROF0 + 3
GROWN = 12                                                      # scalars slot: SC_PROF0 + 4, dual solves resumed on a grown candidate set
# the parent's counters per (variant, iteration, far): (sum of qp_unpolished, sum of second attempts) over all missions of SESSIONS
PARENT = {(v, it, far): (0, 0) for v in (2, 4) for it in (1, 2) for far in FAR}
PARENT_EIGHT = {2: (0, 0), 4: (0, 0)}


def run(cs, param, opts):
    plans = [c.plan() for c in cs]
    s = planner.Session([c.world for c in cs], [c.mission for c in cs], param, plans, opts=planner.solver_opts(**opts))
    s.run()
    st = s.download()
    sc = s.scalars(24)
    s.close()
    return st, plans, sc[:, SECOND_ATTEMPTS].copy(), sc[:, GROWN].copy()


@functools.lru_cache(maxsize=None)
def session(N, si, variant, iteration, far):
    """one session over the cases of (N, si): run once per process, never written to"""
    cs = [c for c, _ in SQ.cases(N, si)]
    opts = dict(SQ.SCHEDULES[N][si].opts_kw(), qp_variant=variant)
    if FAR[far] is not None:
        opts["qp_far_slack"] = FAR[far]
    return run(cs, cs[0].param(iteration=iteration), opts)


@pytest.mark.parametrize("far", list(FAR))
@pytest.mark.parametrize("iteration", [1, 2])
@pytest.mark.parametrize("variant", [2, 4])
def test_short_missions(variant, iteration, far):
    unpolished = second_attempts = grown = 0
    worst = {}
    print()
    for N, si in SESSIONS:
        st, plans, second, grew = session(N, si, variant, iteration, far)
        grown += int(grew.sum())
        cfs = SQ.cases(N, si)
        assert st == [0] * len(cfs), (N, si, st)
        before = None
        if iteration == 2:
            st1, before, _, _ = session(N, si, variant, 1, far)
            assert st1 == [0] * len(cfs)
        for i, ((c, f), pl) in enumerate(zip(cfs, plans)):
            tag = f"{c.name} variant {variant} iteration {iteration} {far}"
            unpolished += pl.qp_unpolished
            second_attempts += int(second[i])
            if iteration == 1:
                check_mission(c, f, pl, None, tag, worst)
                continue
            assert pl.qp_solves == 2 * c.qp_solves(), (tag, pl.qp_solves)
            assert pl.qp_unpolished == 0 and pl.kkt_max < 1e-8, (tag, pl.qp_unpolished, pl.kkt_max)
            reps = SQ.certify(c, pl, pl.ctrl, before[i].ctrl)
            print(f"{tag}: forward error {max(r['forward_error'] for r in reps):.2e} m, iterations {pl.qp_iterations}, kkt_max {pl.kkt_max:.1e}")
            check_reports(reps, FWD_TOL)
    print(f"variant {variant} iteration {iteration} {far}: qp_unpolished {unpolished}, second attempts {second_attempts}, "
          f"dual solves resumed on a grown candidate set {grown}")
    assert (unpolished, second_attempts) == PARENT[(variant, iteration, far)]
    assert grown > 0  # verification found violated rows outside the candidate set, S was extended and the dual solve resumed


@functools.lru_cache(maxsize=None)
def eight_agents():
    """agents 0 .. 7 of the 8-agent golden, M = 6, random durations in [0.5, 2], as ONE batch; admitted like every case of synth_qp"""
    rng = np.random.default_rng([8, 8])
    c = SQ.make_case(SQ.GOLDEN_OF[8], range(8), 6, SQ.durations(rng, "rand2", 6), SQ._batch(8), "rand2", "n8_bs8_m6_rand2")
    f = SQ.facts(c)
    assert f is not None, "the 8-agent case no longer meets the conditions of synth_qp"
    return c, f


@pytest.mark.parametrize("variant", [2, 4])
def test_eight_agents_one_batch(variant):
    c, f = eight_agents()
    assert c.param().batch_size == 8 and c.qp_solves() == 1
    st, (pl,), second, _ = run([c], c.param(), dict(qp_variant=variant))
    assert st == [0]
    print()
    check_mission(c, f, pl, None, f"{c.name} variant {variant}", {})
    print(f"variant {variant}: qp_unpolished {pl.qp_unpolished}, second attempts {int(second[0])}")
    assert (pl.qp_unpolished, int(second[0])) == PARENT_EIGHT[variant]
