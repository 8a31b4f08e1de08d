"""Host front-end (not accelerated): mission JSON, octomap .bt -> distance grid, ECBS initial trajectories.

Thin ctypes binding of lib/librbp_host.so (include/rbp_host.h).  These are the callers/data formats either
side of the hot path (reference: mission.hpp:22-88, swarm_traj_planner_rbp_test_all.cpp:51-63,
ecbs_planner.hpp:21-136).
"""
import ctypes as C
import os

import numpy as np

from . import _abi as A
from .types import Clearance, Dynamics, Limits, Mission, Param, PlanResult, Report, Separation, SweptClearance, World

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(A.LIB_DIR, "librbp_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C swarm_simulator_amd/csrc host`")
        L = C.CDLL(path)
        L.rbp_mission_load_json.argtypes = [C.c_char_p, C.POINTER(A.rbp_mission_buf)]
        L.rbp_mission_free.argtypes = [C.POINTER(A.rbp_mission_buf)]
        L.rbp_mission_free.restype = None
        L.rbp_octomap_load_bt.argtypes = [C.c_char_p, C.POINTER(A.rbp_octomap_buf)]
        L.rbp_octomap_free.argtypes = [C.POINTER(A.rbp_octomap_buf)]
        L.rbp_octomap_free.restype = None
        L.rbp_world_build.argtypes = [C.POINTER(A.rbp_octomap_buf), C.c_double * 3, C.c_double * 3, C.c_double,
                                      C.POINTER(A.rbp_world_buf)]
        L.rbp_world_free.argtypes = [C.POINTER(A.rbp_world_buf)]
        L.rbp_world_free.restype = None
        L.rbp_ecbs_plan.argtypes = [C.POINTER(A.rbp_world_buf), C.POINTER(A.rbp_mission), C.POINTER(A.rbp_param),
                                    C.c_int64, C.POINTER(A.rbp_init_traj_buf)]
        L.rbp_ecbs_obstacles.argtypes = [C.POINTER(A.rbp_world_buf), C.POINTER(A.rbp_mission), C.POINTER(A.rbp_param), C.c_int32 * 3,
                                         C.POINTER(C.c_uint8), C.c_size_t]
        L.rbp_ecbs_plan_obstacles.argtypes = [C.c_int32 * 3, C.POINTER(C.c_uint8), C.POINTER(A.rbp_mission), C.POINTER(A.rbp_param),
                                              C.c_int64, C.POINTER(A.rbp_init_traj_buf)]
        L.rbp_init_traj_free.argtypes = [C.POINTER(A.rbp_init_traj_buf)]
        L.rbp_init_traj_free.restype = None
        L.rbp_validate.argtypes = [C.POINTER(A.rbp_mission), C.POINTER(A.rbp_param), C.c_int32, A.c_double_p,
                                   A.c_double_p, C.c_double, A.c_double_p, A.c_double_p]
        L.rbp_report_host.argtypes = [C.POINTER(A.rbp_mission), C.POINTER(A.rbp_param), C.c_int32, A.c_double_p,
                                      A.c_double_p, C.c_double, C.POINTER(A.rbp_report)]
        L.rbp_dynamics_host.argtypes = [C.POINTER(A.rbp_mission), C.POINTER(A.rbp_param), C.c_int32, A.c_double_p, A.c_double_p, C.c_double,
                                        C.POINTER(A.rbp_dynamics), C.c_void_p, C.c_void_p, C.c_int32]
        L.rbp_clearance_host.argtypes = [C.POINTER(A.rbp_world), C.POINTER(A.rbp_mission), C.c_int32, A.c_double_p, A.c_double_p, C.c_double,
                                         C.POINTER(A.rbp_clearance), A.c_double_p]
        L.rbp_separation_host.argtypes = [C.POINTER(A.rbp_mission), C.POINTER(A.rbp_param), C.c_int32, A.c_double_p, A.c_double_p, C.c_int32,
                                          C.c_double, C.POINTER(A.rbp_separation), A.c_double_p]
        L.rbp_swept_clearance_host.argtypes = [C.POINTER(A.rbp_world), C.POINTER(A.rbp_mission), C.c_int32, A.c_double_p, A.c_double_p, C.c_int32,
                                               C.c_double, C.POINTER(A.rbp_swept_clearance), A.c_double_p]
        L.rbp_limits_host.argtypes = [C.POINTER(A.rbp_mission), C.c_int32, A.c_double_p, A.c_double_p, C.c_int32, C.c_double,
                                      C.POINTER(A.rbp_limits), A.c_double_p]
        L.rbp_write_coef_csv.argtypes =[C.c_char_p, C.c_int32, C.c_int32, A.c_double_p, A.c_double_p]
        L.rbp_write_qp_lp.argtypes = [C.c_char_p, C.POINTER(A.rbp_mission), C.POINTER(A.rbp_param), C.POINTER(A.rbp_plan), C.c_int32,
                                      A.c_double_p]
        _lib = L
    return _lib


def _np(p, shape, dtype):
    n = int(np.prod(shape))
    if n == 0:
        return np.zeros(shape, dtype)
    return np.ctypeslib.as_array(p, shape=(n,)).astype(dtype, copy=True).reshape(shape)


def data_path(*parts):
    """committed input fixtures: data/missions/*.json, data/worlds/*.bt (the reference's own files)."""
    return os.path.join(A.REPO_ROOT, "data", *parts)


def load_mission(path) -> Mission:
    """Mission::setMission (mission.hpp:22-88)."""
    if not os.path.isabs(path) and not os.path.exists(path):
        path = data_path("missions", path)
    buf = A.rbp_mission_buf()
    rc = lib().rbp_mission_load_json(path.encode(), C.byref(buf))
    if rc:
        raise ValueError(f"There is no such mission file {path} (rc={rc})")
    N = buf.N
    m = Mission(_np(buf.start, (N, 9), np.float64), _np(buf.goal, (N, 9), np.float64), _np(buf.radius, (N,), np.float64),
                _np(buf.max_vel, (N, 3), np.float64), _np(buf.max_acc, (N, 3), np.float64),
                _np(buf.speed, (N,), np.float64))
    lib().rbp_mission_free(C.byref(buf))
    return m


def load_octomap(path):
    """occupied leaves of an octomap binary tree: (keys[n][4] = x,y,z,size ; res ; node count)."""
    if not os.path.isabs(path) and not os.path.exists(path):
        path = data_path("worlds", path)
    buf = A.rbp_octomap_buf()
    rc = lib().rbp_octomap_load_bt(path.encode(), C.byref(buf))
    if rc:
        raise ValueError(f"cannot read octomap {path} (rc={rc})")
    keys = _np(buf.keys, (buf.n_occupied, 4), np.int32)
    res, nodes = buf.res, buf.n_nodes
    lib().rbp_octomap_free(C.byref(buf))
    return keys, res, nodes


def build_world(keys, res, param: Param, max_dist=1.0) -> World:
    """DynamicEDTOctomap(maxDist, tree, world_min, world_max, false).update()
    (swarm_traj_planner_rbp_test_all.cpp:57-63)."""
    ob = A.rbp_octomap_buf()
    keys = np.ascontiguousarray(keys, np.int32)
    ob.res, ob.n_occupied, ob.keys, ob.n_nodes = res, len(keys), A.ptr(keys, A.c_int32_p), 0
    wb = A.rbp_world_buf()
    lo = (C.c_double * 3)(param.world_x_min, param.world_y_min, param.world_z_min)
    hi = (C.c_double * 3)(param.world_x_max, param.world_y_max, param.world_z_max)
    rc = lib().rbp_world_build(C.byref(ob), lo, hi, max_dist, C.byref(wb))
    if rc:
        raise ValueError(f"rbp_world_build failed rc={rc}")
    shape = tuple(wb.dim)
    w = World(_np(wb.dist, shape, np.float32), tuple(wb.key_min), wb.res)
    lib().rbp_world_free(C.byref(wb))
    return w


def load_world(path, param: Param) -> World:
    keys, res, _ = load_octomap(path)
    return build_world(keys, res, param)


ECBS_ERROR_TEXT = {1: "ECBSPlanner: start/goal occluded by obstacle", 2: "ECBSPlanner: ECBS Failed!"}


def _plan_result(rc, out) -> PlanResult:
    if rc:
        raise RuntimeError(ECBS_ERROR_TEXT.get(rc, f"rc={rc}"))
    N, M = out.N, out.M
    pr = PlanResult(_np(out.init_traj, (N, M + 1, 3), np.float32), _np(out.T, (M + 1,), np.float64))
    pr.ecbs_stats = dict(makespan=out.makespan, sum_cost=out.sum_cost, high_level=out.high_level_expanded,
                         low_level=out.low_level_expanded)
    lib().rbp_init_traj_free(C.byref(out))
    return pr


def ecbs_plan(world: World, mission: Mission, param: Param, max_nodes=200000) -> PlanResult:
    """ECBSPlanner::update (ecbs_planner.hpp:21-72): returns a PlanResult holding initTraj and T."""
    out = A.rbp_init_traj_buf()
    wb, ms, ps = world.c_buf(), mission.c_struct(), param.c_struct()
    return _plan_result(lib().rbp_ecbs_plan(C.byref(wb), C.byref(ms), C.byref(ps), max_nodes, C.byref(out)), out)


def obstacle_mask(call):
    """the two-step protocol of rbp_ecbs_obstacles / rbp_dev_worlds_ecbs_obstacles: call(dim, buffer or None, capacity) -> rc; returns
    (rc, mask [dimx][dimy][dimz] uint8)."""
    dim = (C.c_int32 * 3)()
    rc = call(dim, None, 0)
    if rc:
        return rc, None
    mask = np.zeros(tuple(dim), np.uint8)
    return call(dim, mask.ctypes.data_as(C.POINTER(C.c_uint8)), mask.size), mask


def ecbs_obstacles(world: World, mission: Mission, param: Param) -> np.ndarray:
    """ECBSPlanner::setObstacles (ecbs_planner.hpp:80-109): the occupancy mask [dimx][dimy][dimz] of the planning lattice.  A lattice
    sample outside the world's grid raises what ecbs_plan raises."""
    wb, ms, ps = world.c_buf(), mission.c_struct(), param.c_struct()
    rc, mask = obstacle_mask(lambda dim, buf, cap: lib().rbp_ecbs_obstacles(C.byref(wb), C.byref(ms), C.byref(ps), dim, buf, cap))
    if rc:
        raise RuntimeError(ECBS_ERROR_TEXT.get(rc, f"rc={rc}"))
    return mask


def ecbs_plan_obstacles(obstacle, mission: Mission, param: Param, max_nodes=200000) -> PlanResult:
    """the search of ecbs_plan on a mask from ecbs_obstacles (or planner.ecbs_obstacles): ecbs_plan is the two composed."""
    mask = np.ascontiguousarray(obstacle, np.uint8)
    out = A.rbp_init_traj_buf()
    ms, ps = mission.c_struct(), param.c_struct()
    rc = lib().rbp_ecbs_plan_obstacles((C.c_int32 * 3)(*mask.shape), mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(ms), C.byref(ps),
                                       max_nodes, C.byref(out))
    return _plan_result(rc, out)


def validate(mission: Mission, param: Param, plan: PlanResult, dt=0.1):
    """(min safety-margin ratio, total flight distance) — rbp_publisher.hpp:769-798, 685-695."""
    ms, ps = mission.c_struct(), param.c_struct()
    ratio, dist = C.c_double(), C.c_double()
    rc = lib().rbp_validate(C.byref(ms), C.byref(ps), plan.M, A.ptr(plan.T, A.c_double_p), A.ptr(plan.coef, A.c_double_p),
                            dt, C.byref(ratio), C.byref(dist))
    if rc:
        raise RuntimeError(f"rbp_validate rc={rc}")
    return ratio.value, dist.value


def report(mission: Mission, param: Param, plan: PlanResult, dt=0.1) -> Report:
    """the same two signals as a Report, by the rule the device shares (csrc/common/report_rules.h): what planner.Session.report /
    planner.report_coefs return for this plan, bit for bit, and where the minimum lies.  Differs from validate by rounding only."""
    ms, ps = mission.c_struct(), param.c_struct()
    out = A.rbp_report()
    rc = lib().rbp_report_host(C.byref(ms), C.byref(ps), plan.M, A.ptr(plan.T, A.c_double_p), A.ptr(plan.coef, A.c_double_p), dt, C.byref(out))
    if rc:
        raise ValueError(f"rbp_report_host rc={rc}")
    return Report.from_c(out)


def dynamics(mission: Mission, param: Param, plan: PlanResult, dt=0.1, states=None, curves=None):
    """the plan's limit peaks as a Dynamics, by the sequential loop the device shares (csrc/common/state_rules.h): what
    planner.Session.dynamics / planner.dynamics_coefs return for this plan, bit for bit.  states [N][9][S] and curves [S][2]: None or
    C-contiguous float64 arrays with one S, written in place up to the plan's samples where samples <= S (Dynamics.stored), else untouched."""
    S = 0
    for a in (states, curves):
        if a is not None and (a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]):
            raise ValueError("states / curves must be C-contiguous float64 arrays")
    if states is not None:
        S = states.shape[-1]
        if states.shape != (plan.N, 9, S):
            raise ValueError(f"states must be [N][9][S], not {states.shape}")
    if curves is not None:
        if curves.ndim != 2 or curves.shape[1] != 2 or (states is not None and curves.shape[0] != S):
            raise ValueError(f"curves must be [S][2] with the S of states, not {curves.shape}")
        S = curves.shape[0]
    ms, ps = mission.c_struct(), param.c_struct()
    out = A.rbp_dynamics()
    rc = lib().rbp_dynamics_host(C.byref(ms), C.byref(ps), plan.M, A.ptr(plan.T, A.c_double_p), A.ptr(plan.coef, A.c_double_p), dt, C.byref(out),
                                 C.c_void_p(None if states is None else states.ctypes.data), C.c_void_p(None if curves is None else curves.ctypes.data), S)
    if rc:
        raise ValueError(f"rbp_dynamics_host rc={rc}")
    return Dynamics.from_c(out)


def clearance(world: World, mission: Mission, plan: PlanResult, dt=0.1, per_agent=False):
    """the plan's clearance to the obstacles of `world` as a Clearance, by the sequential loop the device shares
    (csrc/common/clearance_rules.h): what planner.Session.clearance / planner.clearance_coefs return for this plan and grid, bit for bit.
    per_agent: returns (Clearance, [N] array of every agent's smallest clearance, 1e9 without a sample)."""
    ws, ms = world.c_struct(), mission.c_struct()
    out = A.rbp_clearance()
    agents = np.full(plan.N, 1e9) if per_agent else None
    rc = lib().rbp_clearance_host(C.byref(ws), C.byref(ms), plan.M, A.ptr(plan.T, A.c_double_p), A.ptr(plan.coef, A.c_double_p), dt, C.byref(out),
                                  A.ptr(agents, A.c_double_p))
    if rc:
        raise ValueError(f"rbp_clearance_host rc={rc}")
    return (Clearance.from_c(out), agents) if per_agent else Clearance.from_c(out)


def separation(mission: Mission, param: Param, plan: PlanResult, depth=4, refine_below=2.0, per_pair=False):
    """a certified interval for the plan's smallest safety ratio in continuous time as a Separation, by the sequential loop the device
    shares (csrc/common/separation_rules.h): what planner.Session.separation / planner.separation_coefs return for this plan, bit for bit.
    per_pair: returns (Separation, [N (N-1) / 2] array of every pair's smallest lower ratio, 1e9 where there is none)."""
    ms, ps = mission.c_struct(), param.c_struct()
    out = A.rbp_separation()
    pairs = np.full(plan.N * (plan.N - 1) // 2, 1e9) if per_pair else None
    rc = lib().rbp_separation_host(C.byref(ms), C.byref(ps), plan.M, A.ptr(plan.T, A.c_double_p), A.ptr(plan.coef, A.c_double_p), depth,
                                   refine_below, C.byref(out), A.ptr(pairs, A.c_double_p))
    if rc:
        raise ValueError(f"rbp_separation_host rc={rc}")
    return (Separation.from_c(out), pairs) if per_pair else Separation.from_c(out)


def swept_clearance(world: World, mission: Mission, plan: PlanResult, depth=4, refine_below=0.5, per_agent=False):
    """a certified interval for the plan's smallest clearance to the obstacles of `world` in continuous time as a SweptClearance, by the
    sequential loop the device shares (csrc/common/swept_rules.h): what planner.Session.swept_clearance / planner.swept_clearance_coefs
    return for this plan and grid, bit for bit.  per_agent: returns (SweptClearance, [N] array of every agent's smallest lower clearance,
    1e9 where there is none)."""
    ws, ms = world.c_struct(), mission.c_struct()
    out = A.rbp_swept_clearance()
    agents = np.full(plan.N, 1e9) if per_agent else None
    rc = lib().rbp_swept_clearance_host(C.byref(ws), C.byref(ms), plan.M, A.ptr(plan.T, A.c_double_p), A.ptr(plan.coef, A.c_double_p), depth,
                                        refine_below, C.byref(out), A.ptr(agents, A.c_double_p))
    if rc:
        raise ValueError(f"rbp_swept_clearance_host rc={rc}")
    return (SweptClearance.from_c(out), agents) if per_agent else SweptClearance.from_c(out)


def limits(mission: Mission, plan: PlanResult, depth=4, refine_above=0.5, per_agent=False):
    """certified intervals for the plan's largest velocity and acceleration, as fractions of the mission's max_vel / max_acc, in continuous
    time as a Limits, by the sequential loop the device shares (csrc/common/limits_rules.h): what planner.Session.limits /
    planner.limits_coefs return for this plan, bit for bit.  per_agent: returns (Limits, [N][2] array of every agent's largest upper
    velocity and acceleration ratio, 0 where there is none)."""
    ms = mission.c_struct()
    out = A.rbp_limits()
    agents = np.zeros((plan.N, 2)) if per_agent else None
    rc = lib().rbp_limits_host(C.byref(ms), plan.M, A.ptr(plan.T, A.c_double_p), A.ptr(plan.coef, A.c_double_p), depth, refine_above,
                               C.byref(out), A.ptr(agents, A.c_double_p))
    if rc:
        raise ValueError(f"rbp_limits_host rc={rc}")
    return (Limits.from_c(out), agents) if per_agent else Limits.from_c(out)


def write_coef_csv(directory, plan: PlanResult):
    """generateCoefCSV (rbp_planner.hpp:295-324)."""
    os.makedirs(directory, exist_ok=True)
    rc = lib().rbp_write_coef_csv(directory.encode(), plan.N, plan.M, A.ptr(plan.T, A.c_double_p), A.ptr(plan.coef, A.c_double_p))
    if rc:
        raise RuntimeError(f"rbp_write_coef_csv rc={rc}")


def write_qp_lp(path, mission: Mission, param: Param, plan: PlanResult, batch: int, dummy=None):
    """QPmodel.lp of batch `batch` (rbp_planner.hpp:150-152): `plan` holds the corridor and the UNSCALED T; `dummy` = control points
    of the frozen agents ([N][3][6M]) or None for build_dummy."""
    ms, ps, pl = mission.c_struct(), param.c_struct(), plan.c_struct()
    d = None if dummy is None else A.as_f64(dummy)
    rc = lib().rbp_write_qp_lp(path.encode(), C.byref(ms), C.byref(ps), C.byref(pl), batch, A.ptr(d, A.c_double_p))
    if rc:
        raise RuntimeError(f"rbp_write_qp_lp rc={rc}")
