"""The clearance rule (csrc/common/clearance_rules.h: the lookup of a position in the distance grid, clearance, hit, outside, where the
minimum lies), as the HOST compiler builds it: tests/clearance_rules/clearance_main.cpp includes nothing but that header, is compiled with
every warning an error and with the undefined-behaviour and address sanitizers, and checks hand-computed cases on a 4 x 3 x 2 grid with a
negative key_min: a coordinate exactly on a cell boundary at res 0.1 and 0.25, a negative coordinate just below zero (floor, not
truncation), a double that rounds to the next float across a boundary, one step outside on each of the six sides, NaN / inf / 1e300
positions (outside, and no conversion to int the sanitizer could object to), the hit threshold at d == r - 1e-6 and one ulp below, equal
clearances reporting the first (sample, agent) whatever the order they arrive in, a NaN radius never the minimum, no sample giving 1e9 and
-1.  (The device compiler's reading of the same text is held to the host's bits by tests/test_gpu_clearance.py.)  CPU only."""
import os
import re
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

HEADER = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc", "common", "clearance_rules.h")
SRC = os.path.join(A.REPO_ROOT, "tests", "clearance_rules", "clearance_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]   # (not include/: the header stands alone)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("clearance_rules") / "clearance_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_rule_holds_on_hand_computed_cases_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clearance rules ok" in r.stdout


def test_the_header_includes_nothing_but_the_report_rules():
    """... which include <math.h> and <stdint.h> and nothing else (tests/test_report_rules.py)"""
    assert re.findall(r"^\s*#\s*include\s*(\S+)", open(HEADER).read(), flags=re.M) == ['"common/report_rules.h"']


def test_the_lookup_is_stated_in_the_header_and_nowhere_else():
    """the kernels and the host entry call the rule; neither forms a key of its own (kernels/corridor.hip keeps its own key code, untouched)"""
    csrc = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")
    for rel in (os.path.join("kernels", "clearance.hip"), os.path.join("host", "validate.cpp")):
        text = open(os.path.join(csrc, rel)).read()
        assert "clearance_rules::" in text and '#include "common/clearance_rules.h"' in text
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        body = code[code.index("clearance"):] if rel.endswith(".hip") else code[code.index("rbp_clearance_host"):code.index("rbp_write_coef_csv")]
        assert "floor(" not in body, rel
