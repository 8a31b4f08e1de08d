"""The arithmetic of one inequality row that both QP solvers share (csrc/common/ipm_rows.h), as the HOST compiler builds it:
tests/ipm_rows/rows_main.cpp includes nothing but that header, is compiled with every warning an error and with the undefined-behaviour and
address sanitizers, runs as a process of its own, and checks the header against the equations it solves -- the Newton system of a row over
a grid of states (s, z from 1e-9 to 1e3), regularisations, centrality targets and shifts, each residual in long double against a bound
counted from the operations --, and bit for bit where bits matter: the two copies of a pair row, the slot order of the accumulators,
the polish's candidate rule, the flag of the K0 factor step.  (What the device compiler makes of the same text is held to the oracle by
tests/test_gpu_parity.py, test_gpu_sweep.py and test_gpu_joint.py.)"""
import os
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

SRC = os.path.join(A.REPO_ROOT, "tests", "ipm_rows", "rows_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipm_rows") / "rows_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_row_arithmetic_solves_its_equations_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ipm rows ok" in r.stdout


def test_only_the_two_qp_solvers_include_the_header():
    """its `fp contract(fast)` holds for the rest of a translation unit: the files that must round like the reference never see it"""
    src = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")
    users = sorted(f for d, _, fs in os.walk(src) for f in fs if '#include "common/ipm_rows.h"' in open(os.path.join(d, f), errors="replace").read())
    assert users == ["jqp.hip", "qp.hip"]
