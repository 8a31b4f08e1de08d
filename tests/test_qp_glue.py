"""The order of operations of the batch QP's workgroup-wide reductions (csrc/common/reduce_order.h, used by kernels/qp_base.inc wave_red,
block_reduce and block_reduce_n) as the HOST compiler builds it: tests/qp_glue/glue_main.cpp includes nothing but that header, is compiled
with every warning an error and with the undefined-behaviour and address sanitizers and runs as a process of its own.  What it covers: the
header's partner map is a reduction tree (every lane of a row once); its slot / chunk map parks K values' partial results in the 16 scratch
doubles without a slot written twice, read unwritten or out of range, for 256 and 512 threads; and the test's doubles tell one order of
additions from another.  What it does NOT cover: the device code.  Both host models walk the same header, so "K together equal K apart" holds
there by construction once the slots are right; that the device's block_reduce_n gives block_reduce's bits is held by the benchmark's dumped
outputs against the parent commit (profiles/qp_glue_ab.txt) and, to the oracle, by tests/test_gpu_qp_glue.py.

The cases of tests/synth_qp_glue.py are admitted here, on the CPU, by the oracle alone."""
import os
import subprocess

import pytest

from swarm_simulator_amd import _abi as A
from tests import synth_qp_glue as G
from tests.test_kkt_reference import FWD_TOL

SRC = os.path.join(A.REPO_ROOT, "tests", "qp_glue", "glue_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qp_glue") / "glue_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_reductions_taken_together_keep_each_value_s_order_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "qp glue ok" in r.stdout


def test_the_kernel_includes_the_header():
    src = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc", "kernels")
    assert '#include "common/reduce_order.h"' in open(os.path.join(src, "qp.hip")).read()


@pytest.mark.parametrize("N", G.NS)
def test_the_glue_cases_are_admitted_by_the_oracle_alone(N):
    """conditions (a)-(c) of tests/synth_qp.py; N = 5 and 9 in batches of four end on a batch of one agent"""
    for c, f in G.cases(N):
        assert f.oracle.ok and f.oracle.report["n_qp"] == c.qp_solves() == -(-N // 4) and N % 4 == 1
        assert f.fwd <= FWD_TOL / 10, (c.name, f.fwd)
        print(f"{c.name}: seed {c.seed}, oracle forward error {f.fwd:.2e} m, active rows not decided by the equalities {f.n_active}")
