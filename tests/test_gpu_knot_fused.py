"""The rank-36 update formed in the MFMA tiles of the knot factorisation (kernels/knot_lds.inc: kl_fused_update, KL_FUSED_UPDATE) on the GPU.

tools/ubench/knot.hip, built once with -DKL_FUSED_UPDATE=0 (coupling rows, stored X and U: the other side of every A/B) and once with =1
(the default), each run once under a time limit.  The tool checks M, 1 / d and -- where X is not materialised -- the next block's Schur
complement T - X D^-1 X' against its host restatement (1e-11 * scale, relative 1e-12 for 1 / d).  The companion wave announces M before it
reads its row back: a wrong publish order is a hang, and a hang ends here, in one workgroup under a limit, instead of in the planner.

The product test plans the 8-agent mission on map1.bt with the sweep's parameters (sequential, batches of 4 agents: two batch QPs of
block order 36, the second with frozen-neighbour rows) on both builds of the QP kernel and compares the control points with the
oracle's, to the tolerance of tests/test_gpu_parity.py; every QP must have been polished."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import Param
from tests import oracle_lib as O
from tests.test_gpu_parity import CTRL_TOL, FEAS_TOL, OBJ_RTOL

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(HERE, "..", "swarm_simulator_amd", "csrc", "kernels")
UBENCH = os.path.join(HERE, "..", "tools", "ubench", "knot.hip")


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_knot_microbenchmark_passes_with_and_without_the_fused_update(fused):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to build tools/ubench/knot.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "knot")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", KERNELS, f"-DKL_FUSED_UPDATE={fused}", "-o", exe, UBENCH],
                              timeout=900)
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = run.stdout.decode()
    print(out)
    assert run.returncode == 0, out
    lines = out.strip().splitlines()
    assert lines[-1] == "PASS", out
    assert sum(1 for l in lines if l.startswith("NK ") and l.endswith(" ok")) == 8, out  # four NK at two spreads
    assert any("NK 36 panels" in l for l in lines), out
    assert any(f"KL_FUSED_UPDATE={fused}" in l for l in lines), out  # the side of the A/B that was asked for
    # the fused path checks the Schur complement of the next block, the other one the stored X
    assert any(l.startswith("NK 36 ") and ("max|next S err|" if fused else "max|X err|") in l for l in lines), out


@pytest.fixture(scope="module")
def reference():
    """8 agents, two batches of 4 on map1.bt: corridor and plan of the oracle, computed once and left unchanged"""
    p = Param.test_sweep()
    m = host.load_mission("mission_8agents_15.json")
    w = host.load_world("map1.bt", p)
    init = host.ecbs_plan(w, m, p)
    ref = init.clone_inputs()
    assert O.corridor_update(w, m, p, ref)[0] == 0
    assert O.planner_update(m, p, ref)[0] == 0
    return p, m, w, init, ref


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [2, 4])
def test_batch_qps_of_block_order_36_vs_oracle_on_both_builds(reference, variant):
    p, m, w, init, ref = reference
    assert p.sequential and p.batch_size == 4 and len(m.start) == 8  # two batch QPs, 9 coefficients x 4 agents per knot
    gpu = init.clone_inputs()
    ctx = planner.Context(opts=planner.solver_opts(qp_variant=variant))
    try:
        assert planner.Corridor(w, m, p).update(False, gpu)
        pl = planner.RBPPlanner(m, p, ctx)
        assert pl.update(False, gpu), pl.last_error
    finally:
        ctx.close()
    err = np.abs(ref.ctrl - gpu.ctrl).max()
    print(f"qp_variant {variant}: max |ctrl - oracle| {err:.3g} m, QPs {gpu.qp_solves}, iterations {gpu.qp_iterations}, unpolished {gpu.qp_unpolished}")
    assert err < CTRL_TOL
    assert abs(ref.total_cost - gpu.total_cost) < OBJ_RTOL * max(1.0, abs(ref.total_cost))
    assert gpu.qp_unpolished == 0
    obj, veq, vbox, vrs = O.evaluate_ctrl(m, gpu)
    assert veq < FEAS_TOL and vbox < FEAS_TOL and vrs < FEAS_TOL
