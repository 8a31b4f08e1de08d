"""The polish's per-mission table G = K0^-1 (csrc/common/ipm_rows.h: the dd chain, k0_inverse_column, k0g_symmetrise, k0g_at) as the HOST
compiler builds it: tests/k0_inverse/k0_main.cpp includes nothing but that header, is compiled with every warning an error and with the
undefined-behaviour and address sanitizers, and runs as a process of its own.

Shapes: nj = 1 (one block, no coupling), 2 (one coupling), 3, 7, 35 knots; unit segment times, segment lengths 0.6 .. 1.7 in mixed order,
and 0.5 / 2 alternating (knot ratios 4 and 1/4).  K0 is assembled densely in long double from D_j, E_j and inverted there.  Checked:
the table against that inverse, max|K0 G - I|, and exact symmetry of the stored table.  The bound is not a number chosen in advance:
the same two figures are computed for the route the table replaces -- the double factor's forward and backward pass on every unit
vector -- and the table may be at most 4 times worse.  Both figures are printed per case.

(Why the table's chain runs in double-double: assembled from columns solved in double, the symmetric table's residual was 3.4e-5 against
the columns' own 2.7e-8 at 35 knots and unit times -- K0's condition number is 8e9 there -- because the part above the diagonal comes from
other columns.  With correctly rounded entries it is 1.8e-8.)"""
import os
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

SRC = os.path.join(A.REPO_ROOT, "tests", "k0_inverse", "k0_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k0_inverse") / "k0_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_table_is_the_inverse_and_exactly_symmetric(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "k0 inverse ok" in r.stdout
    assert r.stdout.count("max|K0 G - I|") == 15  # five knot counts, three sets of segment times
