"""The staging layout of rbp_session_refill_from_plans (csrc/common/plan_stage.h: offsets, the greedy partition into rounds, the two
element rules) on the host: tests/plan_stage/stage_main.cpp is a stand-alone program built here with g++ -fsanitize=address,undefined.
It packs ragged missions, walks every round's index space with the header's rules into an arena image and requires the image of a
direct build with every destination element written exactly once; its `capacity` lines are the packer's totals for capacity-shaped
missions, which rbp_plan_stage_bytes must answer.  The refill itself is a GPU test: tests/test_gpu_session_refill_plans.py."""
import os
import subprocess

import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import planner

SRC = os.path.join(A.REPO_ROOT, "tests", "plan_stage", "stage_main.cpp")
CSRC = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")


@pytest.fixture(scope="module")
def stage_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_stage") / "stage_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + CSRC, SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def test_rounds_write_the_image_of_a_direct_build_once(stage_output):
    assert stage_output[-1] == "ok 24 cases", stage_output[-3:]


def test_plan_stage_bytes_is_the_packers_total(stage_output):
    rows = [tuple(int(v) for v in l.split()[1:]) for l in stage_output if l.startswith("capacity ")]
    assert len(rows) == 27
    for N, M, K, total in rows:
        for cap_K, max_boxes in ((K, M), (1000, 1)):   # (neither the capacity's K nor its max_boxes enters)
            assert planner.plan_stage_bytes((cap_K, N, M, max_boxes), K) == total, (N, M, K)
    # additive in K; a shorter mission takes less
    assert planner.plan_stage_bytes((3, 4, 64, 64), 3) == 3 * planner.plan_stage_bytes((3, 4, 64, 64), 1)
    assert planner.plan_stage_bytes((3, 4, 26, 64), 1) < planner.plan_stage_bytes((3, 4, 64, 64), 1)
