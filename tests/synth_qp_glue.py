"""Cases for the hand-overs between the batch QP's sweeps, set-up and chains (kernels/qp_batch.inc, qp_newton.inc rbase_from_acc, qp_base.inc
block_reduce_n).  TEST INFRASTRUCTURE ONLY: imported by test_qp_glue.py (CPU: the cases are admitted) and test_gpu_qp_glue.py (GPU).

Cut from the committed goldens by tests/synth_qp.make_case, batches of four:
  N = 5, 9   a neighbour count = 1 mod 4 (the presolve's rounds of four end on a round of one) and a short last batch of ONE agent: blocks
             of order 36, which take the fused right-hand-side pass, next to a block of order 9, which must not
  M = 2, 3, 9   one, two and eight interior knots: (M - 1) * 3 nb = 12, 24, 96 right-hand-side items for the batches of four and 3, 6, 24 for the
             last one -- below one wavefront, above it; the step update has 3 nb * 6 M = 144 .. 648 entries
A case is admitted only if the oracle alone meets conditions (a)-(c) of tests/synth_qp.py: corridor and planner return 0 with every QP
polished, the KKT certificate accepts the oracle's answer, and the oracle is within FWD_TOL / 10 of the certified optimum.  A draw that
misses one is replaced by the next seed.
"""
import functools

import numpy as np

from tests import synth_qp as SQ
from tests.common import Case

NS = (5, 9)
MS = (2, 3, 9)
KIND_OF = {2: "rand2", 3: "alt", 9: "rand4"}
GOLDEN_OF = {5: "s8_map5_seq4", 9: "c2_16agents_map3"}
SCHED = SQ._batch(4, 3)


def facts_abc(c):
    """conditions (a)-(c) of tests/synth_qp.py, judged on the oracle alone; None: not admitted"""
    from tests.test_kkt_reference import FWD_TOL
    o = SQ.run_oracle(c)
    if not o.ok:
        return None
    reps = SQ.certify(c, o.plan, o.plan.ctrl, o.before)
    if not SQ.accepted(reps, FWD_TOL / 10):
        return None
    return SQ.Facts(o, reps, max(r["forward_error"] for r in reps), sum(r["n_implied"] for r in reps), sum(r["n_active"] - r["n_implied"] for r in reps))


def _build(N, M, attempt):
    kind = KIND_OF[M]
    rng = np.random.default_rng([N, M, attempt, 20261021])
    n0 = Case(GOLDEN_OF[N]).g["init_traj"].shape[0]
    sub = np.sort(rng.choice(n0, N, replace=False))
    return SQ.make_case(GOLDEN_OF[N], sub, M, SQ.durations(rng, kind, M), SCHED, kind, f"glue_n{N}_m{M}_{kind}", (N, M, attempt))


@functools.lru_cache(maxsize=None)
def case(N, M):
    """(case, facts) -- built once per process, never written to: the first seed that meets (a)-(c)"""
    for attempt in range(16):
        c = _build(N, M, attempt)
        f = facts_abc(c)
        if f is not None:
            return c, f
    raise RuntimeError(f"no seed for glue case N={N} M={M}")


def cases(N):
    return [case(N, M) for M in MS]
