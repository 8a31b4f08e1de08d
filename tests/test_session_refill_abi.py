"""The boundary of the refillable session (include/rbp.h: rbp_session_capacity, rbp_session_create_reserved, rbp_session_capacity_of,
rbp_session_refill_from_ecbs) as far as it can be checked without a GPU: the struct's layout in the header and in the binding, the argument
refusals that come before a device is looked for, and the header as a C11 and a C++14 translation unit.  The refill itself is a GPU test:
tests/test_gpu_session_refill.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import planner

INC = os.path.join(A.REPO_ROOT, "include")


def test_capacity_struct_layout_agrees_with_the_header():
    hdr = open(os.path.join(INC, "rbp.h")).read()
    m = re.search(r"typedef struct rbp_session_capacity \{([^}]*)\} rbp_session_capacity;", hdr)
    assert m, "include/rbp.h lost rbp_session_capacity"
    decl = m.group(1).strip().rstrip(";")
    typ, names = decl.split(None, 1)
    assert typ == "int32_t"
    assert [n.strip() for n in names.split(",")] == [f for f, _ in A.rbp_session_capacity._fields_] == ["K", "N", "M", "max_boxes"]
    assert all(t is C.c_int32 for _, t in A.rbp_session_capacity._fields_)
    which = int(re.search(r"RBP_SIZEOF_SESSION_CAPACITY = (\d+)", hdr).group(1))
    assert which == A.RBP_SIZEOF_SESSION_CAPACITY
    assert planner.lib().rbp_sizeof(which) == C.sizeof(A.rbp_session_capacity) == 16
    for f, off in zip(("K", "N", "M", "max_boxes"), (0, 4, 8, 12)):
        assert getattr(A.rbp_session_capacity, f).offset == off


def test_the_three_calls_are_declared_exported_and_bound():
    hdr = open(os.path.join(INC, "rbp.h")).read()
    for name in ("rbp_session_create_reserved", "rbp_session_capacity_of", "rbp_session_refill_from_ecbs"):
        assert re.search(r"\bint\s+" + name + r"\(", hdr), name
        assert name in planner.EXPORTED_SYMBOLS and getattr(planner.lib(), name).argtypes is not None


def bad(rc):
    return rc == A.RBP_ERR_BAD_ARGUMENT, (rc, planner.last_error())


def test_argument_refusals_come_before_a_device_is_looked_for():
    """on a machine without a GPU every one of these would otherwise be RBP_ERR_NO_DEVICE (or a crash on the unreadable handles)"""
    L = planner.lib()
    from swarm_simulator_amd.types import Param
    p = Param.test_sweep().c_struct()
    h = C.c_void_p()
    ws = C.create_string_buffer(64)   # stands for a set of worlds: never looked into, a refusal comes first
    good = A.rbp_session_capacity(3, 4, 64, 64)
    # null arguments
    assert bad(L.rbp_session_create_reserved(None, ws, C.byref(good), C.byref(p)))[0]
    assert bad(L.rbp_session_create_reserved(C.byref(h), None, C.byref(good), C.byref(p)))[0] and "set of worlds" in planner.last_error()
    assert bad(L.rbp_session_create_reserved(C.byref(h), ws, None, C.byref(p)))[0]
    assert bad(L.rbp_session_create_reserved(C.byref(h), ws, C.byref(good), None))[0]
    assert not h.value
    # zero and negative capacities
    for K, N, M, MB in ((0, 4, 64, 64), (-1, 4, 64, 64), (3, 0, 64, 64), (3, -4, 64, 64), (3, 4, 1, 64), (3, 4, 0, 64), (3, 4, -64, 64),
                        (3, 4, 64, 0), (3, 4, 64, -1)):
        cap = A.rbp_session_capacity(K, N, M, MB)
        h.value = 1
        ok, why = bad(L.rbp_session_create_reserved(C.byref(h), ws, C.byref(cap), C.byref(p)))
        assert ok and "K >= 1, N >= 1, M >= 2, max_boxes >= 1" in why[1], ((K, N, M, MB), why)
        assert not h.value   # *out is cleared on every refusal
    # the refusals of rbp_param known from rbp_session_create
    q = Param.test_sweep().c_struct()
    q.n = 7
    assert L.rbp_session_create_reserved(C.byref(h), ws, C.byref(good), C.byref(q)) == A.RBP_ERR_UNSUPPORTED_DEGREE
    q = Param.test_sweep().c_struct()
    q.box_xy_res = 0.0
    assert bad(L.rbp_session_create_reserved(C.byref(h), ws, C.byref(good), C.byref(q)))[0]
    # capacity_of and refill: null session, null search
    cap = A.rbp_session_capacity()
    assert bad(L.rbp_session_capacity_of(None, C.byref(cap)))[0]
    assert bad(L.rbp_session_capacity_of(ws, None))[0]
    slot_of = (C.c_int32 * 4)()
    assert bad(L.rbp_session_refill_from_ecbs(None, ws, 0, slot_of, None))[0] and "rbp_session_refill_from_ecbs" in planner.last_error()
    assert bad(L.rbp_session_refill_from_ecbs(ws, None, 0, slot_of, None))[0]
    assert bad(L.rbp_session_refill_from_ecbs(None, None, 0, None, None))[0]


def test_python_refusals_without_a_device():
    from swarm_simulator_amd.types import Param
    with pytest.raises(TypeError, match="DeviceWorlds"):
        planner.Session.reserved(object(), 3, 4, 64, 64, Param.test_sweep())
    from swarm_simulator_amd import sweep_device
    with pytest.raises(SystemExit):   # --stream without --device-handoff is an argument error
        sweep_device.main(["--device-worlds", "--device-ecbs", "--mode", "batched", "--stream", "2"])
    with pytest.raises(SystemExit):
        sweep_device.main(["--stream", "2"])


TU = """#include "rbp.h"
int use(rbp_session* s, const rbp_dev_worlds* ws, const rbp_dev_ecbs* e, const rbp_param* p) {
    rbp_session_capacity cap = {3, 4, 64, 64}; int32_t slot_of[3]; rbp_session* r = 0;
    return rbp_session_create_reserved(&r, ws, &cap, p) + rbp_session_capacity_of(s, &cap) + rbp_session_refill_from_ecbs(s, e, 0, slot_of, 0);
}
"""


@pytest.mark.parametrize("cc,std,ext", [("gcc", "c11", "c"), ("g++", "c++14", "cpp")])
def test_header_with_the_new_calls_is_plain_c_and_cxx(tmp_path, cc, std, ext):
    src = tmp_path / f"refill_tu.{ext}"
    src.write_text(TU)
    r = subprocess.run([cc, f"-std={std}", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-c", str(src), "-o", str(tmp_path / "refill_tu.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
