"""The knots' inverse factors as contiguous triangles in global memory (kernels/knot_factor_layout.h; QP_LF_PACKED of kernels/qp.hip): the
block orders and chain shapes tests/test_gpu_fwd_in_factor.py does not reach.  Needs an MI355X.  The packed layout is the default of the
256-thread build (qp_variant 4): that variant is the one that takes the packed paths of the odd orders 9 and 27 here.  The 512-thread
build (qp_variant 2) keeps the square image by default and runs the same sessions through the same staging code in 8-byte units.

test_sessions_with_odd_tail_batches[N-variant]
    Product sessions cut from the 8-agent golden as tests/test_gpu_fwd_in_factor.py::cut_cases cuts them (same routine, same admission
    conditions), batches of 4 agents, every M of synth_qp.MS (nj = 1 .. 8: the middle step alone, one chain only, uneven chains), on both
    builds of the kernel:
      N = 5   a batch of order 36, then a tail of order 9 (odd: 8-byte staging units, a gap between the triangle and 1 / d);
      N = 7   a batch of order 36, then a tail of order 27 (odd, no gap);
      N = 8   two batches of order 36 (the second with frozen-neighbour rows).
    N = 4, 6 and 8 at orders 36 and 18 are the existing file's.  Certified as tests/test_gpu_qp_synthetic.py certifies (check_mission:
    its tolerances, every QP polished).  A wrong address in the factor's slot or in a stage buffer is a wrong Newton step: a QP that does
    not converge or is not polished, not a rounding.
"""
import pytest

from tests import synth_qp as SQ
from tests.test_gpu_fwd_in_factor import cut_cases
from tests.test_gpu_qp_synthetic import check_mission, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", [2, 4])
@pytest.mark.parametrize("N", [5, 7, 8])
def test_sessions_with_odd_tail_batches(N, variant):
    cfs = cut_cases(N)
    assert sorted(c.M for c, _ in cfs) == sorted(SQ.MS) and all(c.N == N and c.param().batch_size == 4 and c.param().sequential for c, _ in cfs)
    cs = [c for c, _ in cfs]
    st, plans = run(cs, cs[0].param(), {"qp_variant": variant})
    assert st == [0] * len(cs), st
    print()
    for (c, f), pl in zip(cfs, plans):
        check_mission(c, f, pl, None, f"{c.name} qp_variant {variant}", {})
