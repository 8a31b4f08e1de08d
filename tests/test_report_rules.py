"""The rule of a mission's report (csrc/common/report_rules.h: safety ratio, flight distance, where the minimum lies), as the HOST compiler
builds it: tests/report_rules/report_main.cpp includes nothing but that header, is compiled with every warning an error and with the
undefined-behaviour and address sanitizers, and checks hand-computed cases: a sample on a knot belongs to the earlier segment
(10 * 0.1 == 1.0), 3 * 0.1 lies just past 0.3, the number of samples is a floor, no or one sample gives distance 0, one agent gives ratio 1e9
and indices -1, equal ratios report the smaller (sample, qi, qj) whatever the order they are met in, a NaN is never the minimum, the limit on
the number of samples, a time scale multiplies the times as rbp_session_download does, and the distance is a sum per agent and then over
agents.  (The device compiler's reading of the same text is held to the host's bits by tests/test_gpu_report.py.)"""
import os
import re
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

HEADER = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc", "common", "report_rules.h")
SRC = os.path.join(A.REPO_ROOT, "tests", "report_rules", "report_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]   # (not include/: the header stands alone)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("report_rules") / "report_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_rule_holds_on_hand_computed_cases_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "report rules ok" in r.stdout


def test_the_header_includes_nothing_but_math_and_stdint():
    assert re.findall(r"^\s*#\s*include\s*(\S+)", open(HEADER).read(), flags=re.M) == ["<math.h>", "<stdint.h>"]


def test_the_header_and_the_abi_agree_on_the_limit():
    """RBP_REPORT_MAX_SAMPLES is said in the rule's header (which cannot include rbp.h), in rbp.h and in the binding"""
    said = [re.search(r"#define RBP_REPORT_MAX_SAMPLES \(1 << (\d+)\)", open(p).read()) for p in (HEADER, os.path.join(A.REPO_ROOT, "include", "rbp.h"))]
    assert all(said) and [1 << int(m.group(1)) for m in said] == [A.RBP_REPORT_MAX_SAMPLES] * 2
