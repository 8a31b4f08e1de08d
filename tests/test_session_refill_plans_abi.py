"""The boundary of the refill from a caller's plans (include/rbp.h: RBP_REFILL_STAGE_BYTES, rbp_plan_stage_bytes,
rbp_session_reserve_plan_stage, rbp_session_refill_from_plans) as far as it can be checked without a GPU: the names in the header, the
library and the binding, the refusals that come before a device is looked for, the header as a C11 and a C++14 translation unit, and the
driver's argument rules for --stream-plans.  The refill itself is a GPU test: tests/test_gpu_session_refill_plans.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import planner

INC = os.path.join(A.REPO_ROOT, "include")
CALLS = ("rbp_plan_stage_bytes", "rbp_session_reserve_plan_stage", "rbp_session_refill_from_plans")


def test_the_four_names_are_declared_exported_and_bound():
    hdr = open(os.path.join(INC, "rbp.h")).read()
    assert re.search(r"#define\s+RBP_REFILL_STAGE_BYTES\s+\(64u << 20\)", hdr)
    assert A.RBP_REFILL_STAGE_BYTES == 64 << 20
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\(", hdr), name
        assert name in planner.EXPORTED_SYMBOLS and getattr(planner.lib(), name).argtypes is not None
    for name in ("refill_plans", "reserve_plan_stage"):
        assert callable(getattr(planner.Session, name))
    assert callable(planner.plan_stage_bytes)


def bad(rc):
    return rc == A.RBP_ERR_BAD_ARGUMENT


def test_argument_refusals_come_before_a_device_is_looked_for():
    """on a machine without a GPU every one of these would otherwise be RBP_ERR_NO_DEVICE (or a crash on the unreadable handle)"""
    L = planner.lib()
    sess = C.create_string_buffer(64)   # stands for a session: never looked into, a refusal comes first
    w, m, pl = (A.rbp_world * 1)(), (A.rbp_mission * 1)(), (A.rbp_plan * 1)()
    assert bad(L.rbp_session_refill_from_plans(None, 1, w, m, pl, None)) and "rbp_session_refill_from_plans" in planner.last_error()
    for K in (0, -1):
        assert bad(L.rbp_session_refill_from_plans(sess, K, w, m, pl, None)) and "K >= 1" in planner.last_error()
    assert bad(L.rbp_session_refill_from_plans(sess, 1, None, m, pl, None))
    assert bad(L.rbp_session_refill_from_plans(sess, 1, w, None, pl, None))
    assert bad(L.rbp_session_refill_from_plans(sess, 1, w, m, None, None))
    assert bad(L.rbp_session_reserve_plan_stage(None, 0)) and "rbp_session_reserve_plan_stage" in planner.last_error()
    # rbp_plan_stage_bytes: a pure function
    n = C.c_size_t(7)
    good = A.rbp_session_capacity(3, 4, 64, 64)
    assert L.rbp_plan_stage_bytes(C.byref(good), 2, C.byref(n)) == 0 and n.value > 0
    assert bad(L.rbp_plan_stage_bytes(None, 1, C.byref(n))) and n.value == 0
    assert bad(L.rbp_plan_stage_bytes(C.byref(good), 1, None))
    for K in (0, -3):
        assert bad(L.rbp_plan_stage_bytes(C.byref(good), K, C.byref(n)))
    for cap in ((0, 4, 64, 64), (3, 0, 64, 64), (3, -4, 64, 64), (3, 4, 1, 64), (3, 4, -64, 64), (3, 4, 64, 0)):
        n.value = 7
        assert bad(L.rbp_plan_stage_bytes(C.byref(A.rbp_session_capacity(*cap)), 1, C.byref(n))) and n.value == 0, cap
        with pytest.raises(ValueError, match="K >= 1, N >= 1, M >= 2, max_boxes >= 1"):
            planner.plan_stage_bytes(cap, 1)
    with pytest.raises(ValueError, match="K >= 1"):
        planner.plan_stage_bytes((3, 4, 64, 64), 0)


def test_stream_plans_argument_rules():
    from swarm_simulator_amd import sweep_device
    for argv in (["--device-worlds", "--device-ecbs", "--device-handoff", "--mode", "batched", "--stream-plans", "2"],   # with --device-handoff
                 ["--device-worlds", "--stream-plans", "2"],                                                             # not batched
                 ["--stream-plans", "2"],                                                                                # no device worlds
                 ["--device-worlds", "--mode", "batched", "--stream-plans", "-1"]):
        with pytest.raises(SystemExit):
            sweep_device.main(argv)


TU = """#include "rbp.h"
int use(rbp_session* s, const rbp_world* w, const rbp_mission* m, const rbp_plan* p) {
    rbp_session_capacity cap = {3, 4, 64, 64}; size_t bytes = RBP_REFILL_STAGE_BYTES;
    return rbp_plan_stage_bytes(&cap, 2, &bytes) + rbp_session_reserve_plan_stage(s, bytes) + rbp_session_refill_from_plans(s, 2, w, m, p, 0);
}
"""


@pytest.mark.parametrize("cc,std,ext", [("gcc", "c11", "c"), ("g++", "c++14", "cpp")])
def test_header_with_the_new_calls_is_plain_c_and_cxx(tmp_path, cc, std, ext):
    src = tmp_path / f"refill_plans_tu.{ext}"
    src.write_text(TU)
    r = subprocess.run([cc, f"-std={std}", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-c", str(src), "-o", str(tmp_path / "refill_plans_tu.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
