"""The device ECBS search (kernels/ecbs.hip), the part that needs no GPU: the synthetic cases of tests/synth_ecbs.py keep the statistics
recorded from the host search -- and so stay inside the budgets tests/test_gpu_ecbs_device.py runs them with -- and both entry points
refuse bad arguments before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import planner
from tests import synth_ecbs as S


@pytest.mark.parametrize("name,r,w,high,low,M", S.CASES, ids=[f"{c[0]}-r{c[1]}-w{c[2]}" for c in S.CASES])
def test_host_statistics_stay_as_recorded(name, r, w, high, low, M):
    mask, m, p = S.case(name, r, w)
    assert mask.shape == S.DIM
    pr = S.host_plan(mask, m, p)   # (raises if the search needs more than the GPU test's budget)
    st = pr.ecbs_stats
    assert (st["high_level"], st["low_level"], pr.M) == (high, low, M)
    assert pr.M <= S.MAX_M and high <= S.BUDGET
    grid = p.grid_xy_res
    assert (2 * r < grid / 2, grid / 2 <= 2 * r < grid, 2 * r >= grid) == (r == 0.10, r == 0.15, r == 0.35)


def test_the_radii_reach_all_three_regimes():
    assert {c[1] for c in S.CASES} == {0.10, 0.15, 0.35}


class Call:
    """valid arguments of the two calls for one small mission; a test breaks one of them"""

    def __init__(self, K=2):
        mask, self.m, p = S.case("gap2", 0.15, 1.1)
        self.K = K
        self.masks = [mask] * K
        self.missions = [self.m] * K
        self.param = p.c_struct()
        self.arrays = planner.EcbsOut(K, self.m.qn, S.MAX_M)   # (owns what self.out points at)
        self.out = self.arrays.c_struct()
        self.budget = S.BUDGET
        self.dim = (C.c_int32 * 3)(*S.DIM)
        # a set of worlds cannot be made without a device.  Every refusal tested here comes before the set is looked into, so any non-null
        # pointer does; it points at zeroed memory so that a check that went missing shows as a failed assertion
        self.worlds = C.create_string_buffer(256)

    def refused(self, why, *, K=None, dim=True, masks=True, missions=True, param=True, out=True, worlds=True, index=True, only=None):
        """both calls (or only "masks" / "worlds") return RBP_ERR_BAD_ARGUMENT and name `why`"""
        K = self.K if K is None else K
        n = len(self.missions)
        ms = (A.rbp_mission * n)(*[m.c_struct() for m in self.missions])
        u8 = C.POINTER(C.c_uint8)
        mp = (u8 * n)(*[C.cast(None, u8) if m is None else m.ctypes.data_as(u8) for m in self.masks])
        idx = np.zeros(n, np.int32)
        L = planner.lib()
        if only != "worlds":
            rc = L.rbp_dev_ecbs_plan_masks(0, K, self.dim if dim else None, mp if masks else None, ms if missions else None,
                                           C.byref(self.param) if param else None, self.budget, C.byref(self.out) if out else None)
            assert rc == A.RBP_ERR_BAD_ARGUMENT and why in planner.last_error(), (rc, planner.last_error())
        if only != "masks":
            rc = L.rbp_dev_worlds_ecbs_plan(self.worlds if worlds else None, K, A.ptr(idx, A.c_int32_p) if index else None, ms if missions else None,
                                            C.byref(self.param) if param else None, self.budget, C.byref(self.out) if out else None)
            assert rc == A.RBP_ERR_BAD_ARGUMENT and why in planner.last_error(), (rc, planner.last_error())


def test_argument_errors_come_before_a_device_is_looked_for():
    """(on the parent commit the symbols do not exist)"""
    assert planner.lib().rbp_sizeof(7) == C.sizeof(A.rbp_ecbs_out)
    assert A.RBP_ECBS_MAX_HIGH_LEVEL_NODES >= 128
    Call().refused("K > 0", K=0)
    Call().refused("K > 0", K=-3)
    Call().refused("missions", missions=False)
    Call().refused("param", param=False)
    Call().refused("out", out=False)
    Call().refused("need dim", dim=False, only="masks")
    Call().refused("the masks", masks=False, only="masks")
    Call().refused("set of worlds", worlds=False, only="worlds")
    Call().refused("world_index", index=False, only="worlds")
    c = Call()
    c.masks = [c.masks[0], None]
    c.refused("a mask is null", only="masks")
    c = Call()
    c.out.T = None
    c.refused("every array")
    c = Call()
    c.missions = [c.m, c.m.subset([0, 1])]
    c.refused("share N")
    c = Call()
    big = S.mission(np.zeros((257, 2)), np.zeros((257, 2)), 0.15)
    c.missions, c.arrays = [big] * 2, planner.EcbsOut(2, 257, 2)
    c.out = c.arrays.c_struct()
    c.refused("N must be 1..256")
    c = Call()
    none = S.mission(np.zeros((0, 2)), np.zeros((0, 2)), 0.15)
    c.missions = [none] * 2
    c.refused("N must be 1..256")
    for budget in (0, -1, A.RBP_ECBS_MAX_HIGH_LEVEL_NODES + 1):
        c = Call()
        c.budget = budget
        c.refused("max_high_level_nodes")
    for max_M in (1, 4097):
        c = Call()
        c.out.max_M = max_M
        c.refused("max_M")
    c = Call()   # a lattice beyond what the kernel packs: 2001 cells along x and y
    c.param.grid_xy_res = 0.005
    c.dim = (C.c_int32 * 3)(2001, 2001, 2)
    c.refused("1..1024 cells per axis")
    c = Call()   # ... and one whose time layers exceed the seen bitmap: 1001 x 1001 x 2 cells
    c.param.grid_xy_res = 0.01
    c.dim = (C.c_int32 * 3)(1001, 1001, 2)
    c.refused("seen bitmap")
    c = Call()   # a mask of another lattice
    c.dim = (C.c_int32 * 3)(21, 21, 3)
    c.refused("not the planning lattice", only="masks")


def test_the_python_calls_check_their_arguments():
    mask, m, p = S.case("gap2", 0.15, 1.1)
    with pytest.raises(ValueError):
        planner.ecbs_plan_masks([mask], [m, m], p)
    with pytest.raises(ValueError):
        planner.ecbs_plan_masks([mask], [m], p, max_nodes=0)
    with pytest.raises(TypeError):
        planner.ecbs_plan_batch(None, [0], [m], p)
