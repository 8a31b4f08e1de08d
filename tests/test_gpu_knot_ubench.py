"""tools/ubench/knot.hip on the GPU: the chain wave and its companion wave of kernels/knot_lds.inc in one workgroup, synchronised by
the progress words, checked against the host restatement inside the tool (NK = 9, 18, 27, 36, diagonal spreads 1e4 and 1e8;
|M err| and |X err| < 1e-11 * scale, relative 1/d error < 1e-12).  Both paths of the tool (-DKL_PANEL=0: the column loop for every NK,
the parent's figure of any A/B; -DKL_PANEL=1: the default of knot_lds.inc), each built once and run once under a time limit: a wrong
publish count would be a hang, and a hang ends here instead of in the planner."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(HERE, "..", "swarm_simulator_amd", "csrc", "kernels")
UBENCH = os.path.join(HERE, "..", "tools", "ubench", "knot.hip")


@pytest.mark.gpu
@pytest.mark.parametrize("panel", [0, 1])
def test_knot_microbenchmark_passes_on_the_gpu(panel):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to build tools/ubench/knot.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "knot")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", KERNELS, f"-DKL_PANEL={panel}", "-o", exe, UBENCH], timeout=900)
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = run.stdout.decode()
    print(out)
    assert run.returncode == 0, out
    lines = out.strip().splitlines()
    assert lines[-1] == "PASS", out
    assert sum(1 for l in lines if l.startswith("NK ") and l.endswith(" ok")) == 8, out  # four NK at two spreads
    assert any(("NK 36 panels" if panel else "NK 36 columns") in l for l in lines), out  # the flagship size runs the path asked for
