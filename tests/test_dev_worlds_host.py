"""Device-resident worlds, the part that needs no GPU: rbp_ecbs_plan in its two halves (the obstacle mask of ECBSPlanner::setObstacles and
the search on it) against the one call, and the argument checks of rbp_dev_worlds_create, which come before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host, planner
from swarm_simulator_amd.types import Param

PAIRS = [("mission_8agents_15.json", "map5.bt"), ("mission_16agents_15.json", "map3.bt")]   # the inputs of the committed goldens


def numpy_mask(w, m, p):
    """ecbs_planner.hpp:80-109 restated on w.dist: the accumulating sample loops, point3d's float cast, getDistance's key lookup"""
    eps, axes = 1e-9, []
    for lo, hi, gres in ((p.world_x_min, p.world_x_max, p.grid_xy_res), (p.world_y_min, p.world_y_max, p.grid_xy_res), (p.world_z_min, p.world_z_max, p.grid_z_res)):
        gmin, gmax = np.ceil((lo - eps) / gres) * gres, np.floor((hi + eps) / gres) * gres
        s, i = [], gmin
        while i < gmax + eps:
            s.append(i)
            i += gres
        s = np.array(s)
        axes.append((int(np.round((gmax - gmin) / gres)) + 1, np.round((s - gmin) / gres).astype(int), s.astype(np.float32)))
    mask = np.zeros([a[0] for a in axes], np.uint8)
    key = [np.floor((1.0 / w.res) * a[2].astype(np.float64)).astype(int) - k for a, k in zip(axes, w.key_min)]
    d = w.dist[np.ix_(*key)].astype(np.float64)
    mask[np.ix_(*[a[1] for a in axes])] = d < m.radius.max() + p.grid_margin
    return mask


@pytest.fixture(scope="module", params=PAIRS, ids=[f"{m[8:-5]}_{w[:-3]}" for m, w in PAIRS])
def case(request):
    p = Param.test_sweep()
    m = host.load_mission(request.param[0])
    w = host.load_world(request.param[1], p)
    return w, m, p, host.ecbs_obstacles(w, m, p)


def test_the_two_halves_composed_are_ecbs_plan(case):
    w, m, p, mask = case
    one = host.ecbs_plan(w, m, p)
    two = host.ecbs_plan_obstacles(mask, m, p)
    assert np.array_equal(one.init_traj.view(np.uint32), two.init_traj.view(np.uint32))
    assert np.array_equal(one.T.view(np.uint64), two.T.view(np.uint64))
    assert one.ecbs_stats["makespan"] == two.ecbs_stats["makespan"] and one.ecbs_stats["sum_cost"] == two.ecbs_stats["sum_cost"]


def test_the_mask_is_the_loop_of_set_obstacles(case):
    w, m, p, mask = case
    assert mask.dtype == np.uint8 and mask.any() and not mask.all()
    assert np.array_equal(mask, numpy_mask(w, m, p))


def test_null_obstacle_only_queries_the_shape_and_capacity_is_checked(case):
    w, m, p, mask = case
    wb, ms, ps = w.c_buf(), m.c_struct(), p.c_struct()
    dim = (C.c_int32 * 3)()
    assert host.lib().rbp_ecbs_obstacles(C.byref(wb), C.byref(ms), C.byref(ps), dim, None, 0) == 0 and tuple(dim) == mask.shape
    small = np.zeros(mask.size - 1, np.uint8)
    assert host.lib().rbp_ecbs_obstacles(C.byref(wb), C.byref(ms), C.byref(ps), dim, small.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         small.size) == A.RBP_ERR_BAD_ARGUMENT
    with pytest.raises(RuntimeError):   # a mask of another lattice is refused, not searched
        host.ecbs_plan_obstacles(mask[:-1], m, p)


def test_a_world_smaller_than_the_planning_grid_is_rc_1_from_both_routes():
    p = Param.test_sweep()
    m = host.load_mission("mission_8agents_15.json")
    keys, res, _ = host.load_octomap("map5.bt")
    w = host.build_world(keys, res, Param.test_sweep(world_x_min=-3.0, world_x_max=3.0))   # the lattice of `p` reaches x = +-5
    wb, ms, ps = w.c_buf(), m.c_struct(), p.c_struct()
    out = A.rbp_init_traj_buf()
    assert host.lib().rbp_ecbs_plan(C.byref(wb), C.byref(ms), C.byref(ps), 1000, C.byref(out)) == 1
    dim = (C.c_int32 * 3)()
    assert host.lib().rbp_ecbs_obstacles(C.byref(wb), C.byref(ms), C.byref(ps), dim, None, 0) == 0
    mask = np.zeros(tuple(dim), np.uint8)
    assert host.lib().rbp_ecbs_obstacles(C.byref(wb), C.byref(ms), C.byref(ps), dim, mask.ctypes.data_as(C.POINTER(C.c_uint8)), mask.size) == 1
    with pytest.raises(RuntimeError, match="occluded"):
        host.ecbs_obstacles(w, m, p)
    with pytest.raises(RuntimeError, match="occluded"):
        host.ecbs_plan(w, m, p)


def create(out=True, W=1, n_leaves=(0,), res=(0.1,), lo=(-5.0, -5.0, 0.3), hi=(5.0, 5.0, 2.5), max_dist=1.0):
    h = C.c_void_p()
    keys = np.zeros((4, 4), np.int32)
    n = max(len(n_leaves), 1)
    kp = (A.c_int32_p * n)(*[A.ptr(keys, A.c_int32_p)] * len(n_leaves))
    rc = planner.lib().rbp_dev_worlds_create(C.byref(h) if out else None, 0, W, kp, (C.c_int64 * n)(*n_leaves), (C.c_double * n)(*res),
                                             (C.c_double * 3)(*lo), (C.c_double * 3)(*hi), max_dist)
    if rc == 0:
        planner.lib().rbp_dev_worlds_destroy(h)
    else:
        assert not h.value
    return rc


@pytest.mark.parametrize("bad", [dict(out=False), dict(W=0), dict(W=-3), dict(n_leaves=(-1,)), dict(W=2, n_leaves=(2, -5), res=(0.1, 0.1)),
                                 dict(hi=(5.0, -5.5, 2.5)), dict(res=(0.0,)), dict(res=(-0.1,)), dict(W=2, n_leaves=(0, 0), res=(0.1, 0.0)),
                                 dict(max_dist=0.0), dict(max_dist=-1.0)],
                         ids=["null_out", "W_0", "W_negative", "n_leaves_negative", "n_leaves_negative_second", "max_below_min", "res_0", "res_negative",
                              "res_0_second", "max_dist_0", "max_dist_negative"])
def test_dev_worlds_create_refuses_bad_arguments_before_it_looks_for_a_device(bad):
    assert create(**bad) == A.RBP_ERR_BAD_ARGUMENT
    assert b"rbp_dev_worlds_create" in planner.lib().rbp_last_error()


def test_dev_worlds_create_has_no_cpu_fallback():
    if planner.lib().rbp_device_count() > 0:
        pytest.skip("a HIP device is present")
    assert create() == A.RBP_ERR_NO_DEVICE and b"no CPU fallback" in planner.lib().rbp_last_error()
    keys, res, _ = host.load_octomap("empty.bt")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        planner.DeviceWorlds([keys], [res], Param.test_sweep())


def test_dev_worlds_calls_on_a_null_set():
    L = planner.lib()
    g = A.rbp_world()
    assert L.rbp_dev_worlds_count(None) == 0
    assert L.rbp_dev_worlds_get(None, 0, C.byref(g)) == A.RBP_ERR_BAD_ARGUMENT
    assert L.rbp_dev_worlds_download(None, 0, None) == A.RBP_ERR_BAD_ARGUMENT
    L.rbp_dev_worlds_destroy(None)
