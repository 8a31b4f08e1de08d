"""The per-element rules of the ECBS plan writer (csrc/common/ecbs_rules.h: plan_time, plan_waypoint) as the HOST compiler builds them:
tests/ecbs_handoff/waypoint_main.cpp includes nothing but that header and include/rbp.h, is compiled with every warning an error and with
the undefined-behaviour and address sanitizers, and checks them against hand-computed values and against write_plan -- N = 1, a path of
its start cell only, agents shorter than the makespan, strides above M + 1, time steps 0.5 and 1, and a lattice whose products are not
exact in double.  (The device compiler's reading of the same text, kernels/handoff.hip, is held to the host's bits by
tests/test_gpu_ecbs_handoff.py.)"""
import os
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

SRC = os.path.join(A.REPO_ROOT, "tests", "ecbs_handoff", "waypoint_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "include"), "-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ecbs_handoff") / "waypoint_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_waypoint_rule_is_what_write_plan_writes_under_the_sanitizers(program):
    """(on the parent commit plan_time / plan_waypoint do not exist and the program does not compile)"""
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ecbs handoff rules ok" in r.stdout
