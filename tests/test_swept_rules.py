"""The swept clearance rule (csrc/common/swept_rules.h: the Bernstein form of an agent's trajectory on a segment, de Casteljau halving,
the widened box of a piece's control points, its keys, the budget, the smallest cell of the box, the two end lookups, fixed refinement, the
flags and the order of the minima), as the HOST compiler builds it: tests/swept_rules/swept_main.cpp includes nothing but that header, is
compiled with every warning an error and with the undefined-behaviour and address sanitizers, and checks hand-computed cases: an agent at
rest in one cell (the box is that cell, lower equals upper), a straight line along x through a known row of cells, the boxes and keys of both
of its halves, a coordinate exactly on a cell face and one float beside it, outside on each of the six sides, NaN and infinite coefficients,
a NaN cell and a NaN radius, a box over the budget and one exactly at it, the order of the minimum on ties in every order of arrival, and
`merge` in both orders.  (The device compiler's reading of the same text is held to the host's bits by tests/test_gpu_swept.py.)  CPU only."""
import os
import re
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

HEADER = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc", "common", "swept_rules.h")
SRC = os.path.join(A.REPO_ROOT, "tests", "swept_rules", "swept_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]   # (not include/: the header stands alone)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("swept_rules") / "swept_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_rule_holds_on_hand_computed_cases_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "swept rules ok" in r.stdout


def test_the_header_includes_nothing_but_the_two_rules_it_stands_on():
    """... which include report_rules.h, and that <math.h> and <stdint.h> and nothing else (tests/test_report_rules.py)"""
    assert re.findall(r"^\s*#\s*include\s*(\S+)", open(HEADER).read(), flags=re.M) == ['"common/clearance_rules.h"', '"common/separation_rules.h"']


def test_the_header_and_the_abi_agree_on_the_constants():
    rule, abi = open(HEADER).read(), open(os.path.join(A.REPO_ROOT, "include", "rbp.h")).read()
    for name, value in (("RBP_SWEPT_MAX_DEPTH", A.RBP_SWEPT_MAX_DEPTH), ("RBP_SWEPT_MAX_CELLS", A.RBP_SWEPT_MAX_CELLS)):
        assert int(re.search(r"#define " + name + r" (\d+)", rule).group(1)) == int(re.search(r"#define " + name + r" (\d+)", abi).group(1)) == value


def test_the_arithmetic_is_stated_in_the_header_and_nowhere_else():
    """the kernels and the host entry call the rule; neither halves a control point, widens a box, forms a key or scans a box on its own"""
    csrc = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")
    for rel in (os.path.join("kernels", "swept.hip"), os.path.join("host", "validate.cpp")):
        text = open(os.path.join(csrc, rel)).read()
        assert "swept_rules::" in text and '#include "common/swept_rules.h"' in text
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        body = code[code.index("swept"):] if rel.endswith(".hip") else code[code.index("rbp_swept_clearance_host"):code.index("rbp_write_coef_csv")]
        for needle in ("0.5", "floor", "(float)", "rule_div", "__ddiv", "b[", "halve", "key_of", "1.11022"):
            assert needle not in body, (rel, needle)
