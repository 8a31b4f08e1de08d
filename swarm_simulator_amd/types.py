"""Host-side data types mirroring the reference's Mission / Param / PlanResult.

reference: swarm_planner/include/mission.hpp:10-20, param.hpp:7-42, sp_const.hpp:16-28.
Each object owns numpy buffers and hands out the flat C structs of include/rbp.h.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _abi as A


@dataclass
class Mission:
    """mission.hpp:13-15: qn, startState/goalState (9 each), quad_size, max_vel, max_acc."""
    start: np.ndarray      # [N][9]
    goal: np.ndarray       # [N][9]
    radius: np.ndarray     # [N]   quad_size
    max_vel: np.ndarray    # [N][3]
    max_acc: np.ndarray    # [N][3]
    speed: np.ndarray = None

    def __post_init__(self):
        self.start = A.as_f64(self.start)
        self.goal = A.as_f64(self.goal)
        self.radius = A.as_f64(self.radius)
        self.max_vel = A.as_f64(self.max_vel)
        self.max_acc = A.as_f64(self.max_acc)

    @property
    def qn(self):
        return int(self.start.shape[0])

    N = qn

    def c_struct(self):
        m = A.rbp_mission()
        m.N = self.qn
        m.start = A.ptr(self.start, A.c_double_p)
        m.goal = A.ptr(self.goal, A.c_double_p)
        m.radius = A.ptr(self.radius, A.c_double_p)
        m.max_vel = A.ptr(self.max_vel, A.c_double_p)
        m.max_acc = A.ptr(self.max_acc, A.c_double_p)
        return m

    def subset(self, idx):
        idx = np.asarray(idx)
        return Mission(self.start[idx], self.goal[idx], self.radius[idx], self.max_vel[idx], self.max_acc[idx])


@dataclass
class Param:
    """param.hpp:44-70 — same names, same defaults."""
    log: bool = False
    world_x_min: float = -5
    world_y_min: float = -5
    world_z_min: float = 0
    world_x_max: float = 5
    world_y_max: float = 5
    world_z_max: float = 2.5
    ecbs_w: float = 1.3
    grid_xy_res: float = 0.3
    grid_z_res: float = 0.6
    grid_margin: float = 0.2
    box_xy_res: float = 0.1
    box_z_res: float = 0.1
    time_scale: bool = True
    time_step: float = 1
    downwash: float = 2.0
    n: int = 5
    phi: int = 3
    sequential: bool = False
    batch_size: int = 4
    batch_iter: int = 0
    iteration: int = 1
    timescale_rule: int = 0   # NOT a key of the reference: include/rbp.h RBP_TIMESCALE_* (0 = every real root, 1 = roots_derivative's first two eigenvalues)

    @classmethod
    def random_forest(cls, **kw):
        """launch/plan_rbp_random_forest.launch:29-66 argument defaults."""
        d = dict(world_z_min=0.3, ecbs_w=1.3, grid_xy_res=0.5, grid_z_res=1.0, grid_margin=0.2,
                 sequential=True, batch_size=4, batch_iter=-1, iteration=1)
        d.update(kw)
        return cls(**d)

    @classmethod
    def test_sweep(cls, **kw):
        """launch/plan_rbp_test.launch:27-59 (the 50-map sweep): as random_forest but ecbs_w=1.5."""
        d = dict(ecbs_w=1.5)
        d.update(kw)
        return cls.random_forest(**d)

    def c_struct(self):
        p = A.rbp_param()
        p.world_min[:] = [self.world_x_min, self.world_y_min, self.world_z_min]
        p.world_max[:] = [self.world_x_max, self.world_y_max, self.world_z_max]
        p.box_xy_res, p.box_z_res = self.box_xy_res, self.box_z_res
        p.downwash, p.time_step = self.downwash, self.time_step
        p.ecbs_w, p.grid_xy_res, p.grid_z_res, p.grid_margin = self.ecbs_w, self.grid_xy_res, self.grid_z_res, self.grid_margin
        p.n, p.phi = self.n, self.phi
        p.sequential, p.batch_size, p.batch_iter, p.iteration = int(self.sequential), self.batch_size, self.batch_iter, self.iteration
        p.time_scale, p.log = int(self.time_scale), int(self.log)
        p.timescale_rule = int(self.timescale_rule)
        return p


@dataclass
class World:
    """The distance grid DynamicEDTOctomap serves (include/rbp.h rbp_world)."""
    dist: np.ndarray            # [nx][ny][nz] float32 metres
    key_min: tuple
    res: float

    def __post_init__(self):
        self.dist = A.as_f32(self.dist)

    def c_struct(self):
        w = A.rbp_world()
        w.dim[:] = list(self.dist.shape)
        w.key_min[:] = list(self.key_min)
        w.res = self.res
        w.dist = A.ptr(self.dist, A.c_float_p)
        return w

    def c_buf(self):
        w = A.rbp_world_buf()
        w.dim[:] = list(self.dist.shape)
        w.key_min[:] = list(self.key_min)
        w.res = self.res
        w.dist = A.ptr(self.dist, A.c_float_p)
        return w


class DeviceWorld:
    """A distance grid that lives in HBM: rbp_world whose `dist` is a device pointer (include/rbp.h).  Corridor, Context.plan_update and
    Session take it in place of a World and read the grid where it is.  Items of planner.DeviceWorlds are of this type; from_tensor wraps
    a caller's own tensor."""

    def __init__(self, ptr, shape, key_min, res, device, owner=None, index=None):
        self.ptr, self.shape, self.key_min, self.res, self.device = int(ptr), tuple(int(n) for n in shape), tuple(int(k) for k in key_min), float(res), int(device)
        self._owner, self._index = owner, index   # the DeviceWorlds (or the tensor) that owns the memory: kept alive with this object

    @classmethod
    def from_tensor(cls, t, key_min, res):
        """a caller's float32 CUDA tensor [nx][ny][nz] (contiguous) as a world; the tensor is kept alive with the object"""
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()):
            raise TypeError("DeviceWorld.from_tensor needs a contiguous float32 CUDA tensor [nx][ny][nz]")
        return cls(t.data_ptr(), t.shape, key_min, res, t.device.index if t.device.index is not None else torch.cuda.current_device(), owner=t)

    def c_struct(self):
        w = A.rbp_world()
        w.dim[:] = list(self.shape)
        w.key_min[:] = list(self.key_min)
        w.res = self.res
        w.dist = C.cast(C.c_void_p(self.ptr), A.c_float_p)
        return w

    def tensor(self):
        """zero-copy torch float32 view [nx][ny][nz] of the grid"""
        import torch
        if isinstance(self._owner, torch.Tensor):
            return self._owner
        holder = type("_View", (), {})()   # __cuda_array_interface__ holder (torch on ROCm reads it like on CUDA)
        holder.__cuda_array_interface__ = {"shape": self.shape, "typestr": "<f4", "data": (self.ptr, False), "version": 2}
        holder.keepalive = self
        return torch.as_tensor(holder, device=torch.device("cuda", self.device))

    def download(self) -> World:
        """the grid as a host World"""
        if self._index is not None:
            return World(self._owner._download(self._index), self.key_min, self.res)
        return World(self._owner.detach().cpu().numpy(), self.key_min, self.res)


@dataclass
class Report:
    """rbp_report (include/rbp.h): a mission's two acceptance signals and where the smallest ratio lies.  min_safety_ratio is 1e9 and the
    three indices -1 for a mission without a pair or a sample; samples is -1 beyond RBP_REPORT_MAX_SAMPLES; status != 0: nothing computed."""
    min_safety_ratio: float
    total_flight_distance: float
    end_time: float
    samples: int
    min_sample: int
    min_qi: int
    min_qj: int
    status: int = 0

    @classmethod
    def from_c(cls, r):
        return cls(r.min_safety_ratio, r.total_flight_distance, r.end_time, r.samples, r.min_sample, r.min_qi, r.min_qj, r.status)

    def bits(self):
        """the record with its doubles as bit patterns: what two evaluations of the one rule must agree on"""
        f = np.array([self.min_safety_ratio, self.total_flight_distance, self.end_time], np.float64).view(np.uint64)
        return tuple(int(x) for x in f) + (self.samples, self.min_sample, self.min_qi, self.min_qj, self.status)


@dataclass
class Dynamics:
    """rbp_dynamics (include/rbp.h): a mission's limit peaks -- the largest |v| / max_vel and |a| / max_acc over samples, agents and axes,
    with the value itself, its limit and where it lies (-1: none) -- its end time and samples, and whether its states / curves were
    written.  status != 0: nothing computed."""
    peak_vel_ratio: float
    peak_vel: float
    peak_vel_limit: float
    peak_acc_ratio: float
    peak_acc: float
    peak_acc_limit: float
    end_time: float
    samples: int
    vel_sample: int
    vel_agent: int
    vel_axis: int
    acc_sample: int
    acc_agent: int
    acc_axis: int
    stored: int = 0
    status: int = 0

    FIELDS = ("peak_vel_ratio", "peak_vel", "peak_vel_limit", "peak_acc_ratio", "peak_acc", "peak_acc_limit", "end_time", "samples",
              "vel_sample", "vel_agent", "vel_axis", "acc_sample", "acc_agent", "acc_axis", "stored", "status")

    @classmethod
    def from_c(cls, r):
        return cls(*[getattr(r, n) for n in cls.FIELDS])

    def bits(self):
        """the record with its doubles as bit patterns: what two evaluations of the one rule must agree on"""
        f = np.array([getattr(self, n) for n in self.FIELDS[:7]], np.float64).view(np.uint64)
        return tuple(int(x) for x in f) + tuple(getattr(self, n) for n in self.FIELDS[7:])


@dataclass
class Clearance:
    """rbp_clearance (include/rbp.h): a mission's smallest clearance to the obstacles -- the distance grid's value under an agent at a
    sample less the agent's radius -- with the grid's value there (-1: outside the grid) and where it lies (-1: none, clearance 1e9), how
    many (sample, agent) items hit an obstacle by the reference's test and how many fell outside the grid, the end time and the samples.
    status != 0: nothing computed."""
    min_clearance: float
    min_dist: float
    end_time: float
    hits: int
    outside: int
    samples: int
    min_sample: int
    min_agent: int
    status: int = 0

    FIELDS = ("min_clearance", "min_dist", "end_time", "hits", "outside", "samples", "min_sample", "min_agent", "status")

    @classmethod
    def from_c(cls, r):
        return cls(*[getattr(r, n) for n in cls.FIELDS])

    def bits(self):
        """the record with its doubles as bit patterns: what two evaluations of the one rule must agree on"""
        f = np.array([getattr(self, n) for n in self.FIELDS[:3]], np.float64).view(np.uint64)
        return tuple(int(x) for x in f) + tuple(getattr(self, n) for n in self.FIELDS[3:])


@dataclass
class Separation:
    """rbp_separation (include/rbp.h): a certified interval for a mission's smallest safety ratio in continuous time --
    lower_ratio <= the smallest ratio over all pairs at every instant <= upper_ratio -- with the (segment, piece, qi, qj) and the depth
    of the piece each bound came from (-1: none, ratio 1e9), the items (pair, segment) whose lower ratio is below 1 (uncertified), whose
    upper ratio is below 1 (colliding: a proven collision) and that were refined, and the end time.  status != 0: nothing computed."""
    lower_ratio: float
    upper_ratio: float
    end_time: float
    uncertified: int
    colliding: int
    refined: int
    lower_segment: int
    lower_piece: int
    lower_qi: int
    lower_qj: int
    upper_segment: int
    upper_piece: int
    upper_qi: int
    upper_qj: int
    lower_depth: int
    upper_depth: int
    status: int = 0

    FIELDS = ("lower_ratio", "upper_ratio", "end_time", "uncertified", "colliding", "refined", "lower_segment", "lower_piece", "lower_qi",
              "lower_qj", "upper_segment", "upper_piece", "upper_qi", "upper_qj", "lower_depth", "upper_depth", "status")

    @classmethod
    def from_c(cls, r):
        return cls(*[getattr(r, n) for n in cls.FIELDS])

    def bits(self):
        """the record with its doubles as bit patterns: what two evaluations of the one rule must agree on"""
        f = np.array([getattr(self, n) for n in self.FIELDS[:3]], np.float64).view(np.uint64)
        return tuple(int(x) for x in f) + tuple(getattr(self, n) for n in self.FIELDS[3:])


@dataclass
class SweptClearance:
    """rbp_swept_clearance (include/rbp.h): a certified interval for a mission's smallest clearance to the obstacles in continuous time --
    every reading of the grid under an agent less its radius, at every instant, is >= lower_clearance; upper_clearance is a reading at a
    point the rule computed on the curve (a witness) -- with the readings there (-1: outside or over budget), the (segment, piece, agent)
    and the depth of the piece each came from (-1: none, clearance 1e9), the items (agent, segment) whose lower reading is a hit
    (uncertified), whose upper reading is a hit (hitting), that have a piece outside the grid or over the cell budget and that were
    refined, and the end time.  status != 0: nothing computed."""
    lower_clearance: float
    upper_clearance: float
    lower_dist: float
    upper_dist: float
    end_time: float
    uncertified: int
    hitting: int
    outside: int
    over_budget: int
    refined: int
    lower_segment: int
    lower_piece: int
    lower_agent: int
    lower_depth: int
    upper_segment: int
    upper_piece: int
    upper_agent: int
    upper_depth: int
    status: int = 0

    FIELDS = ("lower_clearance", "upper_clearance", "lower_dist", "upper_dist", "end_time", "uncertified", "hitting", "outside", "over_budget",
              "refined", "lower_segment", "lower_piece", "lower_agent", "lower_depth", "upper_segment", "upper_piece", "upper_agent",
              "upper_depth", "status")

    @classmethod
    def from_c(cls, r):
        return cls(*[getattr(r, n) for n in cls.FIELDS])

    def bits(self):
        """the record with its doubles as bit patterns: what two evaluations of the one rule must agree on"""
        f = np.array([getattr(self, n) for n in self.FIELDS[:5]], np.float64).view(np.uint64)
        return tuple(int(x) for x in f) + tuple(getattr(self, n) for n in self.FIELDS[5:])


@dataclass
class Limits:
    """rbp_limits (include/rbp.h): certified intervals for a mission's largest velocity and largest acceleration, as fractions of the agents'
    max_vel / max_acc, in continuous time -- lower_X_ratio <= sup |X_k(t)| / max_X[a][k] <= upper_X_ratio over agents, axes and instants
    (upper <= 1 certifies the limit, lower > 1 proves a violation) -- with the (segment, piece, agent, axis) and the depth of the piece each
    of the four peaks came from (-1: none, ratio 0), the items (agent, segment) with a piece whose upper ratio is not <= 1 (uncertified),
    with a piece whose lower ratio is > 1 (violating) and that were refined, and the end time.  status != 0: nothing computed."""
    lower_vel_ratio: float
    upper_vel_ratio: float
    lower_acc_ratio: float
    upper_acc_ratio: float
    end_time: float
    uncertified: int
    violating: int
    refined: int
    lower_vel_segment: int
    lower_vel_piece: int
    lower_vel_agent: int
    lower_vel_axis: int
    lower_vel_depth: int
    upper_vel_segment: int
    upper_vel_piece: int
    upper_vel_agent: int
    upper_vel_axis: int
    upper_vel_depth: int
    lower_acc_segment: int
    lower_acc_piece: int
    lower_acc_agent: int
    lower_acc_axis: int
    lower_acc_depth: int
    upper_acc_segment: int
    upper_acc_piece: int
    upper_acc_agent: int
    upper_acc_axis: int
    upper_acc_depth: int
    status: int = 0

    FIELDS = ("lower_vel_ratio", "upper_vel_ratio", "lower_acc_ratio", "upper_acc_ratio", "end_time", "uncertified", "violating", "refined",
              "lower_vel_segment", "lower_vel_piece", "lower_vel_agent", "lower_vel_axis", "lower_vel_depth", "upper_vel_segment", "upper_vel_piece", "upper_vel_agent", "upper_vel_axis", "upper_vel_depth", "lower_acc_segment", "lower_acc_piece", "lower_acc_agent", "lower_acc_axis", "lower_acc_depth", "upper_acc_segment", "upper_acc_piece", "upper_acc_agent", "upper_acc_axis", "upper_acc_depth", "status")

    @classmethod
    def from_c(cls, r):
        return cls(*[getattr(r, n) for n in cls.FIELDS])

    def bits(self):
        """the record with its doubles as bit patterns: what two evaluations of the one rule must agree on"""
        f = np.array([getattr(self, n) for n in self.FIELDS[:5]], np.float64).view(np.uint64)
        return tuple(int(x) for x in f) + tuple(getattr(self, n) for n in self.FIELDS[5:])


class PlanResult:
    """sp_const.hpp:21-28 as flat arrays (include/rbp.h rbp_plan)."""

    def __init__(self, init_traj, T, max_boxes=None):
        self.init_traj = A.as_f32(init_traj)          # [N][M+1][3]
        self.T = A.as_f64(T).copy()                   # [M+1]
        N, M1, _ = self.init_traj.shape
        assert M1 == self.T.shape[0]
        self.N, self.M = N, M1 - 1
        M = self.M
        self.max_boxes = int(max_boxes or M)
        self.sfc_count = np.zeros(N, np.int32)
        self.sfc_box = np.zeros((N, self.max_boxes, 6), np.float64)
        self.sfc_time = np.zeros((N, self.max_boxes), np.float64)
        self.rsfc_normal = np.zeros((A.npair(N), M, 3), np.float32)
        self.rsfc_time = np.zeros(M, np.float64)
        self.coef = np.zeros((N, 3, 6 * M), np.float64)
        self.ctrl = np.zeros((N, 3, 6 * M), np.float64)
        self.time_scale = 1.0
        self.time_scale_alt = 1.0   # the other rule's factor (rbp_param.timescale_rule)
        self.total_cost = 0.0
        self.x_size = self.eq_size = self.ineq_size = 0
        self.qp_iterations = 0
        self.qp_solves = self.qp_unpolished = 0
        self.kkt_max = 0.0
        self._c = None

    def c_struct(self):
        p = A.rbp_plan()
        p.N, p.M = self.N, self.M
        p.T = A.ptr(self.T, A.c_double_p)
        p.init_traj = A.ptr(self.init_traj, A.c_float_p)
        p.max_boxes = self.max_boxes
        p.sfc_count = A.ptr(self.sfc_count, A.c_int32_p)
        p.sfc_box = A.ptr(self.sfc_box, A.c_double_p)
        p.sfc_time = A.ptr(self.sfc_time, A.c_double_p)
        p.rsfc_normal = A.ptr(self.rsfc_normal, A.c_float_p)
        p.rsfc_time = A.ptr(self.rsfc_time, A.c_double_p)
        p.coef = A.ptr(self.coef, A.c_double_p)
        p.ctrl = A.ptr(self.ctrl, A.c_double_p)
        p.time_scale = self.time_scale
        p.total_cost = self.total_cost
        self._c = p
        return p

    def sync_from(self, p):
        """copy the scalar outputs back from the C struct after a call."""
        self.time_scale, self.total_cost = p.time_scale, p.total_cost
        self.x_size, self.eq_size, self.ineq_size = p.x_size, p.eq_size, p.ineq_size
        self.qp_iterations = p.qp_iterations
        self.qp_solves, self.qp_unpolished, self.kkt_max = p.qp_solves, p.qp_unpolished, p.kkt_max
        self.time_scale_alt = p.time_scale_alt

    def clone_inputs(self):
        return PlanResult(self.init_traj.copy(), self.T.copy(), self.max_boxes)

    def clone(self):
        q = self.clone_inputs()
        for k in ("sfc_count", "sfc_box", "sfc_time", "rsfc_normal", "rsfc_time", "coef", "ctrl"):
            getattr(q, k)[...] = getattr(self, k)
        q.time_scale, q.total_cost = self.time_scale, self.total_cost
        return q

    # ---- reference-shaped views ----------------------------------------------------------------
    def SFC(self, qi):
        """list of (box[6], end_time) like PlanResult::SFC[qi] (sp_const.hpp:17)."""
        return [(self.sfc_box[qi, b].copy(), float(self.sfc_time[qi, b])) for b in range(int(self.sfc_count[qi]))]

    def RSFC(self, qi, qj):
        """list of (normal[3] float32, time) like PlanResult::RSFC[qi][qj] (sp_const.hpp:18)."""
        p = A.pair_index(self.N, qi, qj)
        return [(self.rsfc_normal[p, m].copy(), float(self.rsfc_time[m])) for m in range(self.M)]

    def msgs_traj_info(self):
        """[N, n, T_0..T_M]   rbp_planner.hpp:270-274"""
        return np.concatenate([[self.N, 5], self.T])

    def msgs_traj_coef(self, qi):
        """data of msgs_traj_coef[qi]: column-major (6M x 3)  rbp_planner.hpp:286-289"""
        return self.coef[qi].reshape(-1)
