"""The hand-off of a device search to a session (rbp_dev_worlds_ecbs_search, rbp_dev_ecbs_download, rbp_session_create_from_ecbs), the part
that needs no GPU: every argument refusal is RBP_ERR_BAD_ARGUMENT before a device is looked for, in the manner of
tests/test_ecbs_device_cases.py, and the Python calls check theirs."""
import ctypes as C

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import planner, sweep_device
from tests import synth_ecbs as S


class Search:
    """valid arguments of rbp_dev_worlds_ecbs_search for one small mission; a test breaks one of them"""

    def __init__(self, K=2):
        _, self.m, p = S.case("gap2", 0.15, 1.1)
        self.K = K
        self.missions = [self.m] * K
        self.param = p.c_struct()
        self.budget, self.max_M = S.BUDGET, S.MAX_M
        # a set of worlds cannot be made without a device.  Every refusal tested here comes before the set is looked into, so any non-null
        # pointer does; it points at zeroed memory (a set of no worlds) so that a check that went missing shows as a failed assertion
        self.worlds = C.create_string_buffer(256)

    def refused(self, why, *, K=None, missions=True, param=True, worlds=True, index=True, out=True, idx=None):
        K = self.K if K is None else K
        n = len(self.missions)
        ms = (A.rbp_mission * n)(*[m.c_struct() for m in self.missions])
        idx = np.zeros(n, np.int32) if idx is None else np.asarray(idx, np.int32)
        h = C.c_void_p(0xdead)
        rc = planner.lib().rbp_dev_worlds_ecbs_search(self.worlds if worlds else None, K, A.ptr(idx, A.c_int32_p) if index else None, ms if missions else None,
                                                      C.byref(self.param) if param else None, self.budget, self.max_M, C.byref(h) if out else None)
        assert rc == A.RBP_ERR_BAD_ARGUMENT and why in planner.last_error(), (rc, planner.last_error())
        assert not out or h.value is None   # no handle comes back from a refused call


def test_the_search_refuses_bad_arguments_before_a_device_is_looked_for():
    """(on the parent commit the symbols do not exist)"""
    Search().refused("null out", out=False)
    Search().refused("K > 0", K=0)
    Search().refused("K > 0", K=-3)
    Search().refused("missions", missions=False)
    Search().refused("param", param=False)
    Search().refused("set of worlds", worlds=False)
    Search().refused("world_index", index=False)
    c = Search()
    c.missions = [c.m, c.m.subset([0, 1])]
    c.refused("share N")
    c = Search()
    c.missions = [S.mission(np.zeros((257, 2)), np.zeros((257, 2)), 0.15)] * 2
    c.refused("N must be 1..256")
    c = Search()
    c.missions = [S.mission(np.zeros((0, 2)), np.zeros((0, 2)), 0.15)] * 2
    c.refused("N must be 1..256")
    for budget in (0, -1, A.RBP_ECBS_MAX_HIGH_LEVEL_NODES + 1):
        c = Search()
        c.budget = budget
        c.refused("max_high_level_nodes")
    for max_M in (1, 0, -5, 4097):
        c = Search()
        c.max_M = max_M
        c.refused("max_M")
    c = Search()   # a lattice beyond what the kernel packs: 2001 cells along x and y
    c.param.grid_xy_res = 0.005
    c.refused("1..1024 cells per axis")
    c = Search()   # ... and one whose time layers exceed the seen bitmap: 1001 x 1001 x 2 cells
    c.param.grid_xy_res = 0.01
    c.refused("seen bitmap")
    # the zeroed set holds no world: every index is outside it
    Search().refused("world index out of range")
    Search().refused("world index out of range", idx=[0, -1])


def test_a_null_handle_is_refused_everywhere():
    L = planner.lib()
    assert L.rbp_dev_ecbs_count(None) == 0
    L.rbp_dev_ecbs_destroy(None)   # (like free)
    arrays = planner.EcbsOut(2, 4, S.MAX_M)
    out = arrays.c_struct()
    assert L.rbp_dev_ecbs_download(None, C.byref(out)) == A.RBP_ERR_BAD_ARGUMENT and "handle" in planner.last_error()
    ps = S.case("gap2", 0.15, 1.1)[2].c_struct()
    h = C.c_void_p(0xdead)
    slot = np.full(2, 7, np.int32)
    assert L.rbp_session_create_from_ecbs(C.byref(h), None, C.byref(ps), 0, A.ptr(slot, A.c_int32_p)) == A.RBP_ERR_BAD_ARGUMENT
    assert "handle" in planner.last_error() and h.value is None and list(slot) == [7, 7]
    # (any non-null pointer stands for a handle: these refusals come before it is looked into)
    fake = C.create_string_buffer(1024)
    assert L.rbp_session_create_from_ecbs(None, fake, C.byref(ps), 0, None) == A.RBP_ERR_BAD_ARGUMENT
    assert L.rbp_session_create_from_ecbs(C.byref(h), fake, None, 0, None) == A.RBP_ERR_BAD_ARGUMENT and "param" in planner.last_error()
    assert L.rbp_dev_ecbs_download(fake, None) == A.RBP_ERR_BAD_ARGUMENT and "out" in planner.last_error()


def test_the_python_calls_check_their_arguments(capsys):
    _, m, p = S.case("gap2", 0.15, 1.1)
    with pytest.raises(TypeError):
        planner.ecbs_search_batch(None, [0], [m], p)
    with pytest.raises(TypeError):
        planner.Session.from_ecbs(None, p)
    for argv in (["--device-worlds", "--device-handoff", "--mode", "batched"], ["--device-worlds", "--device-ecbs", "--device-handoff"],
                 ["--device-worlds", "--device-ecbs", "--device-handoff", "--mode", "serial"], ["--device-handoff", "--mode", "batched"]):
        with pytest.raises(SystemExit):
            sweep_device.main(argv)
        assert "--device-handoff needs" in capsys.readouterr().err
