"""The substitution step of the wave path (csrc/kernels/knot_subst.h: the two products by pieces, the forward, middle and backward step) as
the HOST compiler builds it.  tests/knot_subst/subst_main.cpp includes the header, is compiled with every warning an error and with the
undefined-behaviour and address sanitizers, and runs as a process of its own: a block-tridiagonal system of nj knots of order 36 with
twisted elimination, M_j and 1 / d_j as the kernel stores them, solved once as solve_staged does and once split as QP_FWD_IN_FACTOR does
(forward steps in elimination order out of a chain area with NaNs where the guarded product must not look, the middle step, then backward
only).  The two agree bit for bit for nj = 1, 2, 3, 4, 5, 8, 35; the distance to a long-double solve is printed.

tools/ubench/knot.hip is cross-compiled for gfx950 with -DUB_FWD=0 and =1 (no GPU needed), so that neither side of its A/B goes stale."""
import os
import shutil
import subprocess

import pytest

from swarm_simulator_amd import _abi as A

SRC = os.path.join(A.REPO_ROOT, "tests", "knot_subst", "subst_main.cpp")
CSRC = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")
UBENCH = os.path.join(A.REPO_ROOT, "tools", "ubench", "knot.hip")


def test_split_substitution_equals_the_full_one_bit_for_bit(tmp_path):
    exe = str(tmp_path / "subst_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=undefined,address",
                        "-fno-sanitize-recover", "-pthread", "-I" + CSRC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "knot subst ok"
    sizes = [int(l.split(":")[0].split()[1]) for l in lines if l.startswith("nj ")]
    assert sizes == [1, 2, 3, 4, 5, 8, 35]
    assert all(l.split(": ")[1].startswith("0 of ") and l.endswith(" ok") for l in lines if l.startswith("nj ")), r.stdout


@pytest.mark.parametrize("fwd", [0, 1])
def test_knot_microbenchmark_builds_for_gfx950(fwd, tmp_path):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to build tools/ubench/knot.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", os.path.join(CSRC, "kernels"), f"-DUB_FWD={fwd}", "-o", str(tmp_path / "knot"),
                        UBENCH], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
