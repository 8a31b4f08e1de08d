"""The separation rule (csrc/common/separation_rules.h: the Bernstein form of a pair's relative trajectory on a segment, de Casteljau
halving, the degree-10 squared norm, the error term, the two ratios of a piece, fixed refinement, the order of the minima), as the HOST
compiler builds it: tests/separation_rules/separation_main.cpp includes nothing but that header, is compiled with every warning an error
and with the undefined-behaviour and address sanitizers, and checks hand-computed cases: a constant offset (3, 4, 0) whose every
coefficient is 25, a vertical offset under the downwash, a straight pass whose closest approach is a piece end from depth 1 on, two
identical agents, the ends of the eight pieces of depth 3 against the polynomial's values, refine_below exactly at an item's depth-0 lower
ratio and one double above, equal minima in every order of arrival, NaN and infinite coefficients, a mission of one agent.  (The device
compiler's reading of the same text is held to the host's bits by tests/test_gpu_separation.py.)  CPU only."""
import os
import re
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

HEADER = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc", "common", "separation_rules.h")
SRC = os.path.join(A.REPO_ROOT, "tests", "separation_rules", "separation_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]   # (not include/: the header stands alone)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("separation_rules") / "separation_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_rule_holds_on_hand_computed_cases_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "separation rules ok" in r.stdout


def test_the_header_includes_nothing_but_the_report_rules():
    """... which include <math.h> and <stdint.h> and nothing else (tests/test_report_rules.py)"""
    assert re.findall(r"^\s*#\s*include\s*(\S+)", open(HEADER).read(), flags=re.M) == ['"common/report_rules.h"']


def test_the_arithmetic_is_stated_in_the_header_and_nowhere_else():
    """the kernels and the host entry call the rule; neither halves a control point, forms a weight or a product of control points, takes
    a square root or moves a ratio on its own"""
    csrc = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")
    for rel in (os.path.join("kernels", "separation.hip"), os.path.join("host", "validate.cpp")):
        text = open(os.path.join(csrc, rel)).read()
        assert "separation_rules::" in text and '#include "common/separation_rules.h"' in text
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        body = code[code.index("separation"):] if rel.endswith(".hip") else code[code.index("rbp_separation_host"):code.index("rbp_write_coef_csv")]
        for needle in ("0.5", "binomial", "rule_sqrt", "rule_div", "__dsqrt", "__ddiv", "b[", "q[", "nextafter"):
            assert needle not in body, (rel, needle)
        assert not re.search(r"for\s*\([^)]*<\s*(6|11|=\s*10|=\s*5)\s*;", body), rel   # no loop over six control points or eleven coefficients
