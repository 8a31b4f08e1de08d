"""The limits rule (csrc/common/limits_rules.h: the derivative's coefficients, their Bernstein form on a segment, de Casteljau halving, the
hull and the end values of a piece with the counted rounding term, the two ratios, fixed refinement, the counts and the order of the
peaks), as the HOST compiler builds it: tests/limits_rules/limits_main.cpp includes nothing but that header, is compiled with every warning
an error and with the undefined-behaviour and address sanitizers, and checks hand-computed cases: an agent at rest, a constant velocity at
every depth, the parabola whose peak the samples miss, both halves of a segment, NaN and infinite coefficients, limits that are no positive
number, the order of the peak on ties in every order of arrival, `merge` in both orders, and refine_above exactly at a depth-0 ratio.
(The device compiler's reading of the same text is held to the host's bits by tests/test_gpu_limits.py.)  CPU only."""
import os
import re
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

CSRC = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")
HEADER = os.path.join(CSRC, "common", "limits_rules.h")
SRC = os.path.join(A.REPO_ROOT, "tests", "limits_rules", "limits_main.cpp")
INC = ["-I" + CSRC]   # (not include/: the header stands alone)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("limits_rules") / "limits_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_rule_holds_on_hand_computed_cases_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "limits rules ok" in r.stdout


def test_the_header_includes_nothing_but_the_two_rules_it_stands_on():
    """... which include report_rules.h, and that <math.h> and <stdint.h> and nothing else (tests/test_report_rules.py)"""
    assert re.findall(r"^\s*#\s*include\s*(\S+)", open(HEADER).read(), flags=re.M) == ['"common/state_rules.h"', '"common/separation_rules.h"']


def test_the_header_and_the_abi_agree_on_the_depth():
    rule, abi = open(HEADER).read(), open(os.path.join(A.REPO_ROOT, "include", "rbp.h")).read()
    name = "RBP_LIMITS_MAX_DEPTH"
    assert int(re.search(r"#define " + name + r" (\d+)", rule).group(1)) == int(re.search(r"#define " + name + r" (\d+)", abi).group(1)) == A.RBP_LIMITS_MAX_DEPTH


def test_the_arithmetic_is_stated_in_the_header_and_nowhere_else():
    """the kernels and the host entry call the rule; neither differentiates, halves a control point, forms an error term or divides by a limit
    on its own"""
    for rel in (os.path.join("kernels", "limits.hip"), os.path.join("host", "limits.cpp")):
        text = open(os.path.join(CSRC, rel)).read()
        assert "limits_rules::" in text and '#include "common/limits_rules.h"' in text
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        body = code[code.index("limits"):]
        for needle in ("0.5", "fabs", "rule_div", "__ddiv", "b[", "halve", "gamma", "hp[", "ratio_up", "ratio_down", "1.11022", "16 +"):
            assert needle not in body, (rel, needle)


def test_the_host_entry_stays_out_of_the_ranges_the_sibling_rules_tests_slice():
    """tests/test_swept_rules.py, test_separation_rules.py and test_clearance_rules.py search host/validate.cpp from their own entry up to
    rbp_write_coef_csv; rbp_limits_host lives in a file of its own"""
    assert "limits" not in open(os.path.join(CSRC, "host", "validate.cpp")).read()
