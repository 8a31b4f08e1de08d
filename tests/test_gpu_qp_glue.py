"""The hand-overs between the batch QP's sweeps, set-up and chains on the cases of tests/synth_qp_glue.py: N = 5 and 9 in batches of four
(a neighbour count = 1 mod 4; a short last batch of one agent, whose block of order 9 must not take the fused right-hand-side pass that
the blocks of order 36 beside it take), M = 2, 3 and 9 (one, two and eight interior knots), on both builds of qp_batch_kernel.  Needs an MI355X.

Judged as tests/test_gpu_qp_synthetic.py judges a mission (check_mission): status 0, every QP polished, kkt_max < 1e-8, the KKT certificate
at its tolerances, |ctrl - oracle| <= CTRL_TOL.  A case is admitted on the CPU first, by the oracle alone (synth_qp_glue.facts_abc)."""
import pytest

from tests import synth_qp_glue as G
from tests.test_gpu_qp_synthetic import check_mission, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", [2, 4], ids=["512-threads", "256-threads"])
@pytest.mark.parametrize("N", G.NS)
def test_short_missions_in_batches_of_four(N, variant):
    cfs = G.cases(N)   # (admission: raises where no seed meets (a)-(c))
    assert [c.M for c, _ in cfs] == list(G.MS) and all(c.N == N and c.qp_solves() == -(-N // 4) for c, _ in cfs)
    cs = [c for c, _ in cfs]
    st, plans = run(cs, cs[0].param(), {"qp_variant": variant})
    assert st == [0] * len(cs), st
    worst = {}
    print()
    for (c, f), pl in zip(cfs, plans):
        check_mission(c, f, pl, None, f"{c.name} qp_variant {variant}", worst)
