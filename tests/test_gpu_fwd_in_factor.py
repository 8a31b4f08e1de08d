"""The predictor's forward substitution carried along the knot factorisation (kernels/qp.hip QP_FWD_IN_FACTOR; kl_forward_step /
kl_middle_step of kernels/knot_lds.inc, the step bodies of kernels/knot_subst.h) on the GPU.  Needs an MI355X.

test_knot_microbenchmark_with_and_without_forward_steps[fwd]
    tools/ubench/knot.hip built with -DUB_FWD=0 and =1, each run once under a time limit: a chain wave and its companion in ONE workgroup,
    chains of 1, 2, 3 and 17 knots first (z_j and the last v against a host restatement on the device's own M_j and 1 / d_j, 1e-12 of the
    scale), then the tool's usual checks.  The chain now waits for its last block's M and steps in front of its wait for the next block:
    a wrong announcement order is a hang, and a hang ends here, in one workgroup under a limit, not in the planner.

test_sessions_of_block_order_36[N-variant]
    Product sessions cut from the goldens as tests/synth_qp.py cuts its cases (same routine, same admission conditions (a)-(e)), batches of
    4 agents, M = 2, 3, 4, 5, 6, 9 (nj = 1: the middle step alone; nj = 2: the left chain only; uneven chains; 8 knots), on both builds:
      N = 4   one batch QP of order 36 (synth_qp's own session);
      N = 8   a second batch of order 36 with frozen-neighbour rows;
      N = 6   a batch of 4, then a tail of order 18, which keeps the full substitution, in the same mission.
    Certified as tests/test_gpu_qp_synthetic.py certifies (check_mission: its tolerances, every QP polished).
"""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests import synth_qp as SQ
from tests.test_gpu_qp_synthetic import check_mission, run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(HERE, "..", "swarm_simulator_amd", "csrc", "kernels")
UBENCH = os.path.join(HERE, "..", "tools", "ubench", "knot.hip")
GOLDEN8 = "s8_map5_seq4"


@pytest.mark.parametrize("fwd", [0, 1])
def test_knot_microbenchmark_with_and_without_forward_steps(fwd):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to build tools/ubench/knot.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "knot")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", KERNELS, f"-DUB_FWD={fwd}", "-o", exe, UBENCH], timeout=900)
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    lines = out.strip().splitlines()
    assert lines[-1] == "PASS", out
    assert any(f"UB_FWD={fwd};" in l for l in lines), out  # the side that was asked for
    chains = [l for l in lines if l.startswith("forward steps")]
    assert len(chains) == 4 and all(l.endswith("fwd ok" if fwd else "fwd off, chain ok") for l in chains), out
    assert [int(l.split("chain of")[1].split(":")[0]) for l in chains] == [1, 2, 3, 17], out
    assert sum(1 for l in lines if l.startswith("NK ") and l.endswith(" ok")) == 8, out  # the tool's own checks: four NK at two spreads


@functools.lru_cache(maxsize=None)
def cut_cases(N):
    """(case, facts) for every M of synth_qp.MS: N agents of the 8-agent golden, batches of 4 (built once per process, never written to)"""
    sched = SQ._batch(4)
    out = []
    for j, M in enumerate(SQ.MS):
        kind = SQ.KINDS[(j + N) % len(SQ.KINDS)]
        for attempt in range(16):
            rng = np.random.default_rng([N, 36, j, attempt])
            sub = np.sort(rng.choice(8, N, replace=False))
            c = SQ.make_case(GOLDEN8, sub, M, SQ.durations(rng, kind, M), sched, kind, f"n{N}_bs4_{j}_m{M}_{kind}", (N, 36, j, attempt))
            f = SQ.facts(c)
            if f is not None:
                out.append((c, f))
                break
        else:
            raise RuntimeError(f"no seed for N {N} M {M}")
    return out


def session_cases(N):
    return SQ.cases(4, 0) if N == 4 else cut_cases(N)


@pytest.mark.parametrize("variant", [2, 4])
@pytest.mark.parametrize("N", [4, 8, 6])
def test_sessions_of_block_order_36(N, variant):
    cfs = session_cases(N)
    assert sorted(c.M for c, _ in cfs) == sorted(SQ.MS) and all(c.N == N and c.param().batch_size == 4 and c.param().sequential for c, _ in cfs)
    cs = [c for c, _ in cfs]
    st, plans = run(cs, cs[0].param(), {"qp_variant": variant})
    assert st == [0] * len(cs), st
    print()
    for (c, f), pl in zip(cfs, plans):
        check_mission(c, f, pl, None, f"{c.name} qp_variant {variant}", {})
