"""Host-side mirror of the reference's two stage classes, on top of the C ABI (lib/librbp_hip.so).

    Corridor(world, mission, param).update(log, plan)      <-> SwarmPlanning::Corridor::update    rbp_corridor.hpp:13-26
    RBPPlanner(mission, param).update(log, plan)           <-> SwarmPlanning::RBPPlanner::update  rbp_planner.hpp:21-84

Same argument meaning and error behaviour: `update` returns True/False and mutates the PlanResult in place;
`last_error` carries what the reference would have sent to ROS_ERROR.  `Session` is the device-resident batched
form bench.py times.  The HIP library is mandatory: nothing here falls back to a CPU implementation.
"""
import ctypes as C
import os

from . import _abi as A
from .types import Clearance, DeviceWorld, Dynamics, Limits, Mission, Param, PlanResult, Report, Separation, SweptClearance, World

_lib = None

ERROR_TEXT = {
    A.RBP_ERR_OBSTACLE_IN_INIT_TRAJ: "Corridor: Invalid initial trajectory. Obstacle invades initial trajectory.",
    A.RBP_ERR_UNEQUAL_TRAJ_LEN: "Corridor: size of initial trajectories must be equal",
    A.RBP_ERR_INIT_TRAJ_COLLIDE: "Corridor: initial trajectories are collided with each other",
    A.RBP_ERR_SFC_OVERFLOW: "Corridor: more SFC boxes than plan.max_boxes",
    A.RBP_ERR_QP_FAILED: "RBPPlanner: Failed to optimize QP",
    A.RBP_ERR_UNSUPPORTED_DEGREE: "RBPPlanner: n should be 5",
    A.RBP_ERR_BAD_ARGUMENT: "bad argument",
    A.RBP_ERR_NO_DEVICE: "no HIP device (the RBP path has no CPU fallback)",
    A.RBP_ERR_HIP: "HIP runtime error",
    A.RBP_ERR_EXCHANGE: "exchange between the two ranks of a sharded joint solve failed",
}


# rbp_exchange_fn of include/rbp.h: int (*)(void* user, void* send_dev, void* recv_dev, size_t bytes)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
EXCHANGE_STREAM_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)   # rbp_exchange_stream_fn (+ the stream)
EXCHANGE_ABORT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)                                                    # rbp_exchange_abort_fn


class RbpLibraryMissing(RuntimeError):
    pass


preloaded_hip_runtime = []   # torch's HIP runtime libraries loaded ahead of librbp_hip.so by lib() (empty: none)


def lib():
    """Load lib/librbp_hip.so; fails loudly if it was not built."""
    global _lib
    if _lib is None:
        path = os.environ.get("RBP_HIP_LIB") or os.path.join(A.LIB_DIR, "librbp_hip.so")  # env override: developer A/B builds
        if not os.path.exists(path):
            raise RbpLibraryMissing(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 and must find THEM when it initialises
        # (if this library's /opt/rocm runtime is in the process first, torch.cuda reports "No HIP GPUs are available"); with torch's
        # copies loaded first, both sides share one runtime whatever the import order -- which streams, events and device pointers
        # exchanged between them (bench.py, sharded.py) rely on.
        # RBP_PRELOAD_TORCH_HIP=0 switches the preload off (a process that never imports torch); what was preloaded is recorded in
        # `preloaded_hip_runtime` and a failure is reported, not swallowed.
        global preloaded_hip_runtime
        if os.environ.get("RBP_PRELOAD_TORCH_HIP", "1") != "0":
            import importlib.util
            sp = importlib.util.find_spec("torch")
            if sp is not None and sp.submodule_search_locations:
                tl = os.path.join(list(sp.submodule_search_locations)[0], "lib")
                for n in ("libhsa-runtime64.so", "libamdhip64.so"):
                    f = os.path.join(tl, n)
                    if os.path.exists(f):
                        try:
                            C.CDLL(f, mode=C.RTLD_GLOBAL)
                            preloaded_hip_runtime.append(f)
                        except OSError as e:
                            import warnings
                            warnings.warn(f"swarm_simulator_amd: could not preload torch's {n} ({e}); torch.cuda may not see the GPU "
                                          f"if it is imported after this library")
        L = C.CDLL(path)
        P = C.POINTER
        L.rbp_version.restype = C.c_char_p
        # the structs of include/rbp.h are written by the library: refuse a library built from another header
        if os.environ.get("RBP_HIP_LIB") and not hasattr(L, "rbp_abi_version"):
            pass  # (developer A/B builds of older commits predate the check)
        else:
            L.rbp_abi_version.restype = C.c_int
            L.rbp_sizeof.restype = C.c_size_t
            L.rbp_sizeof.argtypes = [C.c_int]
            if L.rbp_abi_version() != A.RBP_ABI_VERSION:
                raise RbpLibraryMissing(f"{path}: ABI version {L.rbp_abi_version()}, this binding expects {A.RBP_ABI_VERSION} (rebuild the library)")
            L.rbp_session_device_arrays.argtypes = [C.c_void_p, C.c_int32, P(A.rbp_device_arrays)]
            for which, t in enumerate((A.rbp_world, A.rbp_mission, A.rbp_param, A.rbp_plan, A.rbp_counters, A.rbp_device_arrays, A.rbp_solver_opts, A.rbp_ecbs_out)):
                if L.rbp_sizeof(which) != C.sizeof(t):
                    raise RbpLibraryMissing(f"{path}: sizeof({t.__name__}) is {L.rbp_sizeof(which)} in the library, {C.sizeof(t)} in this binding")
            L.rbp_release_thread_context.restype = None
        L.rbp_last_error.restype = C.c_char_p
        L.rbp_device_count.restype = C.c_int
        L.rbp_param_defaults.argtypes = [P(A.rbp_param)]
        L.rbp_param_defaults.restype = None
        L.rbp_corridor_update.argtypes = [P(A.rbp_world), P(A.rbp_mission), P(A.rbp_param), P(A.rbp_plan)]
        L.rbp_corridor_update_range.argtypes = [P(A.rbp_world), P(A.rbp_mission), P(A.rbp_param), P(A.rbp_plan), C.c_int32, C.c_int32]
        L.rbp_planner_update.argtypes = [P(A.rbp_mission), P(A.rbp_param), P(A.rbp_plan)]
        L.rbp_session_set_agent_range.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.rbp_session_create.argtypes = [P(C.c_void_p), C.c_int, C.c_int, P(A.rbp_world), P(A.rbp_mission), P(A.rbp_param),
                                         P(A.rbp_plan)]
        L.rbp_session_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rbp_session_run_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rbp_session_wait.argtypes = [C.c_void_p]
        L.rbp_session_shard_joint.argtypes = [C.c_void_p, C.c_int32, C.c_int32, EXCHANGE_FN, C.c_void_p]
        L.rbp_session_shard_joint_stream.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
        L.rbp_session_download.argtypes = [C.c_void_p, P(A.rbp_plan), A.c_int32_p, C.c_void_p]
        L.rbp_session_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.rbp_session_counters.argtypes = [C.c_void_p, P(A.rbp_counters), C.c_void_p]
        L.rbp_session_scalars.argtypes = [C.c_void_p, A.c_double_p, C.c_int, C.c_void_p]
        L.rbp_session_destroy.argtypes = [C.c_void_p]
        L.rbp_session_destroy.restype = None
        try:  # (developer A/B builds of older commits loaded through RBP_HIP_LIB may predate the GPU distance grid)
            L.rbp_edt_dims.argtypes = [C.c_double, C.c_double * 3, C.c_double * 3, C.c_int32 * 3, C.c_int32 * 3]
            L.rbp_edt_build.argtypes = [A.c_int32_p, C.c_int64, C.c_double, C.c_double * 3, C.c_double * 3, C.c_double, A.c_float_p]
            L.rbp_dev_worlds_create.argtypes = [P(C.c_void_p), C.c_int, C.c_int32, P(A.c_int32_p), P(C.c_int64), A.c_double_p, C.c_double * 3,
                                                C.c_double * 3, C.c_double]
            L.rbp_dev_worlds_count.argtypes = [C.c_void_p]
            L.rbp_dev_worlds_get.argtypes = [C.c_void_p, C.c_int32, P(A.rbp_world)]
            L.rbp_dev_worlds_download.argtypes = [C.c_void_p, C.c_int32, A.c_float_p]
            L.rbp_dev_worlds_destroy.argtypes = [C.c_void_p]
            L.rbp_dev_worlds_destroy.restype = None
            L.rbp_dev_worlds_ecbs_obstacles.argtypes = [C.c_void_p, C.c_int32, P(A.rbp_mission), P(A.rbp_param), C.c_int32 * 3, P(C.c_uint8), C.c_size_t]
            L.rbp_dev_ecbs_plan_masks.argtypes = [C.c_int, C.c_int32, P(C.c_int32), P(P(C.c_uint8)), P(A.rbp_mission), P(A.rbp_param), C.c_int64,
                                                  P(A.rbp_ecbs_out)]
            L.rbp_dev_worlds_ecbs_plan.argtypes = [C.c_void_p, C.c_int32, A.c_int32_p, P(A.rbp_mission), P(A.rbp_param), C.c_int64, P(A.rbp_ecbs_out)]
            L.rbp_dev_worlds_ecbs_search.argtypes = [C.c_void_p, C.c_int32, A.c_int32_p, P(A.rbp_mission), P(A.rbp_param), C.c_int64, C.c_int32, P(C.c_void_p)]
            L.rbp_dev_ecbs_count.argtypes = [C.c_void_p]
            L.rbp_dev_ecbs_download.argtypes = [C.c_void_p, P(A.rbp_ecbs_out)]
            L.rbp_dev_ecbs_destroy.argtypes = [C.c_void_p]
            L.rbp_dev_ecbs_destroy.restype = None
            L.rbp_session_create_from_ecbs.argtypes = [P(C.c_void_p), C.c_void_p, P(A.rbp_param), C.c_int32, A.c_int32_p]
            L.rbp_session_report.argtypes = [C.c_void_p, C.c_double, P(A.rbp_report), C.c_void_p]
            L.rbp_dev_report.argtypes = [C.c_int, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, A.c_double_p, A.c_double_p, A.c_double_p, A.c_double_p,
                                         C.c_double, C.c_double, P(A.rbp_report)]
            if L.rbp_sizeof(A.RBP_SIZEOF_REPORT) != C.sizeof(A.rbp_report):
                raise RbpLibraryMissing(f"{path}: sizeof(rbp_report) is {L.rbp_sizeof(A.RBP_SIZEOF_REPORT)} in the library, {C.sizeof(A.rbp_report)} in this binding")
            L.rbp_session_dynamics.argtypes = [C.c_void_p, C.c_double, P(A.rbp_dynamics), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
            L.rbp_dev_dynamics.argtypes = [C.c_int, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, A.c_double_p, A.c_double_p, A.c_double_p, A.c_double_p,
                                           A.c_double_p, A.c_double_p, C.c_double, C.c_double, P(A.rbp_dynamics), C.c_void_p, C.c_void_p, C.c_int32]
            if L.rbp_sizeof(A.RBP_SIZEOF_DYNAMICS) != C.sizeof(A.rbp_dynamics):
                raise RbpLibraryMissing(f"{path}: sizeof(rbp_dynamics) is {L.rbp_sizeof(A.RBP_SIZEOF_DYNAMICS)} in the library, {C.sizeof(A.rbp_dynamics)} in this binding")
            L.rbp_session_clearance.argtypes = [C.c_void_p, C.c_double, P(A.rbp_clearance), C.c_void_p, C.c_void_p]
            L.rbp_dev_clearance.argtypes = [C.c_int, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, A.c_double_p, A.c_double_p, A.c_double_p, A.c_double_p,
                                            P(A.rbp_world), C.c_double, P(A.rbp_clearance), C.c_void_p]
            if L.rbp_sizeof(A.RBP_SIZEOF_CLEARANCE) != C.sizeof(A.rbp_clearance):
                raise RbpLibraryMissing(f"{path}: sizeof(rbp_clearance) is {L.rbp_sizeof(A.RBP_SIZEOF_CLEARANCE)} in the library, {C.sizeof(A.rbp_clearance)} in this binding")
            L.rbp_session_separation.argtypes = [C.c_void_p, C.c_int32, C.c_double, P(A.rbp_separation), C.c_void_p, C.c_void_p]
            L.rbp_dev_separation.argtypes = [C.c_int, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, A.c_double_p, A.c_double_p, A.c_double_p, A.c_double_p,
                                             C.c_double, C.c_int32, C.c_double, P(A.rbp_separation), C.c_void_p]
            if L.rbp_sizeof(A.RBP_SIZEOF_SEPARATION) != C.sizeof(A.rbp_separation):
                raise RbpLibraryMissing(f"{path}: sizeof(rbp_separation) is {L.rbp_sizeof(A.RBP_SIZEOF_SEPARATION)} in the library, {C.sizeof(A.rbp_separation)} in this binding")
            L.rbp_session_swept_clearance.argtypes = [C.c_void_p, C.c_int32, C.c_double, P(A.rbp_swept_clearance), C.c_void_p, C.c_void_p]
            L.rbp_dev_swept_clearance.argtypes = [C.c_int, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, A.c_double_p, A.c_double_p, A.c_double_p, A.c_double_p,
                                                  P(A.rbp_world), C.c_int32, C.c_double, P(A.rbp_swept_clearance), C.c_void_p]
            if L.rbp_sizeof(A.RBP_SIZEOF_SWEPT_CLEARANCE) != C.sizeof(A.rbp_swept_clearance):
                raise RbpLibraryMissing(f"{path}: sizeof(rbp_swept_clearance) is {L.rbp_sizeof(A.RBP_SIZEOF_SWEPT_CLEARANCE)} in the library, {C.sizeof(A.rbp_swept_clearance)} in this binding")
            L.rbp_session_limits.argtypes = [C.c_void_p, C.c_int32, C.c_double, P(A.rbp_limits), C.c_void_p, C.c_void_p]
            L.rbp_dev_limits.argtypes = [C.c_int, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, A.c_double_p, A.c_double_p, A.c_double_p, A.c_double_p,
                                         A.c_double_p, C.c_int32, C.c_double, P(A.rbp_limits), C.c_void_p]
            if L.rbp_sizeof(A.RBP_SIZEOF_LIMITS) != C.sizeof(A.rbp_limits):
                raise RbpLibraryMissing(f"{path}: sizeof(rbp_limits) is {L.rbp_sizeof(A.RBP_SIZEOF_LIMITS)} in the library, {C.sizeof(A.rbp_limits)} in this binding")
            L.rbp_session_create_reserved.argtypes = [P(C.c_void_p), C.c_void_p, P(A.rbp_session_capacity), P(A.rbp_param)]
            L.rbp_session_capacity_of.argtypes = [C.c_void_p, P(A.rbp_session_capacity)]
            L.rbp_session_refill_from_ecbs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, A.c_int32_p, C.c_void_p]
            L.rbp_plan_stage_bytes.argtypes = [P(A.rbp_session_capacity), C.c_int32, P(C.c_size_t)]
            L.rbp_session_reserve_plan_stage.argtypes = [C.c_void_p, C.c_size_t]
            L.rbp_session_refill_from_plans.argtypes = [C.c_void_p, C.c_int32, P(A.rbp_world), P(A.rbp_mission), P(A.rbp_plan), C.c_void_p]
            if L.rbp_sizeof(A.RBP_SIZEOF_SESSION_CAPACITY) != C.sizeof(A.rbp_session_capacity):
                raise RbpLibraryMissing(f"{path}: sizeof(rbp_session_capacity) is {L.rbp_sizeof(A.RBP_SIZEOF_SESSION_CAPACITY)} in the library, {C.sizeof(A.rbp_session_capacity)} in this binding")
        except AttributeError:
            if not os.environ.get("RBP_HIP_LIB"):
                raise
        L.rbp_solver_opts_defaults.argtypes = [P(A.rbp_solver_opts)]
        L.rbp_solver_opts_defaults.restype = None
        L.rbp_session_set_solver_opts.argtypes = [C.c_void_p, P(A.rbp_solver_opts)]
        L.rbp_ctx_set_solver_opts.argtypes = [C.c_void_p, P(A.rbp_solver_opts)]
        L.rbp_session_reserve_workspace.argtypes = [C.c_void_p, C.c_void_p]
        L.rbp_session_workspace_bytes.argtypes = [C.c_void_p]
        L.rbp_session_workspace_bytes.restype = C.c_size_t
        L.rbp_ctx_create.argtypes = [P(C.c_void_p), C.c_int]
        L.rbp_ctx_destroy.argtypes = [C.c_void_p]
        L.rbp_ctx_destroy.restype = None
        L.rbp_ctx_corridor_update.argtypes = [C.c_void_p, P(A.rbp_world), P(A.rbp_mission), P(A.rbp_param), P(A.rbp_plan)]
        L.rbp_ctx_planner_update.argtypes = [C.c_void_p, P(A.rbp_mission), P(A.rbp_param), P(A.rbp_plan)]
        L.rbp_ctx_plan_update.argtypes = [C.c_void_p, P(A.rbp_world), P(A.rbp_mission), P(A.rbp_param), P(A.rbp_plan)]
        L.rbp_session_create_in.argtypes = [C.c_void_p, P(C.c_void_p), C.c_int, P(A.rbp_world), P(A.rbp_mission), P(A.rbp_param),
                                            P(A.rbp_plan)]
        _lib = L
    return _lib


EXPORTED_SYMBOLS = [
    "rbp_param_defaults", "rbp_corridor_update", "rbp_corridor_update_range", "rbp_planner_update", "rbp_session_create",
    "rbp_session_run", "rbp_session_run_async", "rbp_session_wait", "rbp_session_shard_joint", "rbp_session_shard_joint_stream", "rbp_session_set_agent_range",
    "rbp_session_download", "rbp_session_reset", "rbp_session_destroy", "rbp_session_counters", "rbp_session_scalars",
    "rbp_session_device_arrays",
    "rbp_version", "rbp_abi_version", "rbp_sizeof", "rbp_release_thread_context",
    "rbp_last_error", "rbp_device_count",
    "rbp_ctx_create", "rbp_ctx_destroy", "rbp_ctx_corridor_update", "rbp_ctx_planner_update", "rbp_ctx_plan_update",
    "rbp_session_create_in",
    "rbp_solver_opts_defaults", "rbp_session_set_solver_opts", "rbp_ctx_set_solver_opts", "rbp_session_workspace_bytes", "rbp_session_reserve_workspace",
    "rbp_edt_dims", "rbp_edt_build",
    "rbp_dev_worlds_create", "rbp_dev_worlds_count", "rbp_dev_worlds_get", "rbp_dev_worlds_download", "rbp_dev_worlds_destroy",
    "rbp_dev_worlds_ecbs_obstacles", "rbp_dev_ecbs_plan_masks", "rbp_dev_worlds_ecbs_plan",
    "rbp_dev_worlds_ecbs_search", "rbp_dev_ecbs_count", "rbp_dev_ecbs_download", "rbp_dev_ecbs_destroy", "rbp_session_create_from_ecbs",
    "rbp_session_report", "rbp_dev_report",
    "rbp_session_dynamics", "rbp_dev_dynamics",
    "rbp_session_clearance", "rbp_dev_clearance",
    "rbp_session_separation", "rbp_dev_separation",
    "rbp_session_swept_clearance", "rbp_dev_swept_clearance",
    "rbp_session_limits", "rbp_dev_limits",
    "rbp_session_create_reserved", "rbp_session_capacity_of", "rbp_session_refill_from_ecbs",
    "rbp_plan_stage_bytes", "rbp_session_reserve_plan_stage", "rbp_session_refill_from_plans",
]


def plan_stage_bytes(capacity, K):
    """bytes K missions of the shape (N, M) of `capacity` = (K, N, M, max_boxes) occupy in the staging block of Session.refill_plans
    (rbp_plan_stage_bytes): what Session.reserve_plan_stage takes.  A pure function; needs no device."""
    cap = A.rbp_session_capacity(*[int(v) for v in capacity])
    n = C.c_size_t()
    rc = lib().rbp_plan_stage_bytes(C.byref(cap), int(K), C.byref(n))
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"rbp_plan_stage_bytes rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"rbp_plan_stage_bytes failed rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return n.value


def last_error():
    return lib().rbp_last_error().decode()


def solver_opts(**kw):
    """rbp_solver_opts (include/rbp.h) with the library's defaults, fields overridden by keyword: polish, joint_wide_min_agents,
    joint_corrector, joint_schedule (0 auto / 1 look-ahead / 2 bulk / 3 bulk with two pivot tiles per pass), qp_schedule (0 auto / 1 one workgroup per mission; 2, the retired phase split, is refused when the planner runs),
    qp_variant (0 / 2 / 4), qp_block_order, qp_groups and qp_rounds (reserved, ignored), qp_far_slack (metres; <= 0: off).  The library reads no environment variables: these are the switches."""
    o = A.rbp_solver_opts()
    lib().rbp_solver_opts_defaults(C.byref(o))
    for k, v in kw.items():
        if k == "size" or not hasattr(o, k):
            raise TypeError(f"rbp_solver_opts has no field {k!r}")
        setattr(o, k, float(v) if k == "qp_far_slack" else int(v))
    return o


def set_default_solver_opts(opts=None, **kw):
    """solver options of the calling thread's default context: what Corridor / RBPPlanner without an explicit Context use."""
    o = opts if opts is not None else solver_opts(**kw)
    rc = lib().rbp_ctx_set_solver_opts(None, C.byref(o))
    if rc:
        raise RuntimeError(f"rbp_ctx_set_solver_opts rc={rc}: {last_error()}")


class Context:
    """rbp_ctx: device memory kept across plans (include/rbp.h).  `device=None` = the calling thread's current device.
    `opts`: rbp_solver_opts (see solver_opts()) of every session / one-shot call made in the context."""

    def __init__(self, device=None, opts=None):
        self._h = C.c_void_p()
        rc = lib().rbp_ctx_create(C.byref(self._h), -1 if device is None else int(device))
        if rc:
            raise RuntimeError(f"rbp_ctx_create failed rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
        if opts is not None:
            self.set_solver_opts(opts)

    def set_solver_opts(self, opts=None, **kw):
        o = opts if opts is not None else solver_opts(**kw)
        rc = lib().rbp_ctx_set_solver_opts(self._h, C.byref(o))
        if rc:
            raise RuntimeError(f"rbp_ctx_set_solver_opts rc={rc}: {last_error()}")

    def plan_update(self, world: World, mission: Mission, param: Param, plan: PlanResult) -> int:
        """Corridor::update && RBPPlanner::update in one call; returns the C ABI's code (0 = both true)."""
        w, m, p, pl = world.c_struct(), mission.c_struct(), param.c_struct(), plan.c_struct()
        rc = lib().rbp_ctx_plan_update(self._h, C.byref(w), C.byref(m), C.byref(p), C.byref(pl))
        plan.sync_from(pl)
        return rc

    def close(self):
        if self._h:
            lib().rbp_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Corridor:
    """rbp_corridor.hpp:11-26.  `ctx`: optional Context whose device arena the call reuses (default: the library's
    per-thread context)."""

    def __init__(self, world: World, mission: Mission, param: Param, ctx: Context = None):
        self.world, self.mission, self.param, self.ctx = world, mission, param, ctx
        self.last_error = ""
        self.rc = 0

    def update(self, log: bool, plan: PlanResult) -> bool:
        w, m, p, pl = self.world.c_struct(), self.mission.c_struct(), self.param.c_struct(), plan.c_struct()
        if self.ctx is not None:
            self.rc = lib().rbp_ctx_corridor_update(self.ctx._h, C.byref(w), C.byref(m), C.byref(p), C.byref(pl))
        else:
            self.rc = lib().rbp_corridor_update(C.byref(w), C.byref(m), C.byref(p), C.byref(pl))
        self.last_error = "" if self.rc == 0 else ERROR_TEXT.get(self.rc, str(self.rc)) + " | " + last_error()
        return self.rc == 0

    def update_range(self, plan: PlanResult, agent_begin: int, agent_end: int) -> bool:
        """one shard of an agent-sharded update (include/rbp.h rbp_corridor_update_range): only the SFC of agents
        [agent_begin, agent_end) and the RSFC rows of pairs (qi, qj) with qi in that range are valid afterwards."""
        w, m, p, pl = self.world.c_struct(), self.mission.c_struct(), self.param.c_struct(), plan.c_struct()
        self.rc = lib().rbp_corridor_update_range(C.byref(w), C.byref(m), C.byref(p), C.byref(pl), agent_begin, agent_end)
        self.last_error = "" if self.rc == 0 else ERROR_TEXT.get(self.rc, str(self.rc)) + " | " + last_error()
        return self.rc == 0


class RBPPlanner:
    """rbp_planner.hpp:19-84"""

    def __init__(self, mission: Mission, param: Param, ctx: "Context" = None):
        self.mission, self.param, self.ctx = mission, param, ctx
        self.last_error = ""
        self.rc = 0

    def update(self, log: bool, plan: PlanResult) -> bool:
        m, p, pl = self.mission.c_struct(), self.param.c_struct(), plan.c_struct()
        if self.ctx is not None:
            self.rc = lib().rbp_ctx_planner_update(self.ctx._h, C.byref(m), C.byref(p), C.byref(pl))
        else:
            self.rc = lib().rbp_planner_update(C.byref(m), C.byref(p), C.byref(pl))
        plan.sync_from(pl)
        self.last_error = "" if self.rc == 0 else ERROR_TEXT.get(self.rc, str(self.rc)) + " | " + last_error()
        return self.rc == 0


class Session:
    """K independent missions resident in HBM (e.g. the 50-map sweep of swarm_traj_planner_rbp_test_all.cpp:49-103).
    The missions share N; every plan keeps its own M (= ECBS makespan + 2) and max_boxes."""

    def __init__(self, worlds, missions, param: Param, plans, device=0, opts=None):
        K = len(plans)
        assert len(worlds) == K and len(missions) == K
        self.K, self.plans, self.param, self.device = K, plans, param, device
        self._N = plans[0].N
        self._keep = (worlds, missions)
        self._w = (A.rbp_world * K)(*[w.c_struct() for w in worlds])
        self._m = (A.rbp_mission * K)(*[m.c_struct() for m in missions])
        self._p = param.c_struct()
        self._pl = (A.rbp_plan * K)(*[p.c_struct() for p in plans])
        self._h = C.c_void_p()
        rc = lib().rbp_session_create(C.byref(self._h), device, K, self._w, self._m, C.byref(self._p), self._pl)
        if rc:
            raise RuntimeError(f"rbp_session_create failed rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
        if opts is not None:
            self.set_solver_opts(opts)

    @classmethod
    def from_ecbs(cls, dev_ecbs, param: Param, max_boxes=None, opts=None):
        """the session of the missions a device search solved (ecbs_search_batch), built on the device from what the search left there
        (rbp_session_create_from_ecbs): no trajectory comes to the host.  `slot_of[k]` is mission k's index in the session, -1 for a
        mission without a plan; `plans` are empty PlanResults of each mission's shape for download().  The DeviceEcbs may be closed
        right away; the DeviceWorlds it searched must outlive the session.  `param` is the plan's: its time_step should be the search's."""
        import numpy as np
        if not isinstance(dev_ecbs, DeviceEcbs):
            raise TypeError("Session.from_ecbs takes a DeviceEcbs")
        if not dev_ecbs._h:
            raise RuntimeError("DeviceEcbs is closed")
        self = cls.__new__(cls)
        self._p = param.c_struct()
        self._h = C.c_void_p()
        slot_of = np.zeros(dev_ecbs.K, np.int32)
        rc = lib().rbp_session_create_from_ecbs(C.byref(self._h), dev_ecbs._h, C.byref(self._p), int(max_boxes or 0), A.ptr(slot_of, A.c_int32_p))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_create_from_ecbs rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_create_from_ecbs failed rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
        self.param, self.device = param, dev_ecbs.device
        self._missions_of(dev_ecbs, slot_of, max_boxes)
        if opts is not None:
            self.set_solver_opts(opts)
        return self

    def _missions_of(self, dev_ecbs, slot_of, max_boxes):
        """what from_ecbs and refill share: slot_of, K, and the shapes of the search's missions with status 0, of which `plans` makes empty
        PlanResults for download() when they are first asked for -- a caller that only reads reports never pays for them"""
        self.slot_of = slot_of
        self._N = dev_ecbs.N
        self._shapes = [(int(M), max_boxes) for M, st in zip(dev_ecbs.M, dev_ecbs.status) if st == 0]
        self.K = len(self._shapes)
        self._keep = (dev_ecbs._worlds,)
        self._plans = self._pl = None

    @property
    def plans(self):
        if self._plans is None:
            import numpy as np
            self._plans = [PlanResult(np.zeros((self._N, M + 1, 3), np.float32), np.zeros(M + 1), mb) for M, mb in self._shapes]
            self._pl = (A.rbp_plan * self.K)(*[p.c_struct() for p in self._plans])
        return self._plans

    @plans.setter
    def plans(self, plans):
        self._plans = plans

    @classmethod
    def reserved(cls, dev_worlds, K, N, M, max_boxes, param: Param, opts=None):
        """an EMPTY session with room for K missions of N agents, M segments and max_boxes boxes per agent on the device of a DeviceWorlds
        (rbp_session_create_reserved), to be given its missions by refill().  Until then run, download and the reports raise ValueError.
        The DeviceWorlds must outlive the session."""
        if not isinstance(dev_worlds, DeviceWorlds):
            raise TypeError("Session.reserved takes a DeviceWorlds")
        if not dev_worlds._h:
            raise RuntimeError("DeviceWorlds is closed")
        self = cls.__new__(cls)
        self._p = param.c_struct()
        self._h = C.c_void_p()
        cap = A.rbp_session_capacity(int(K), int(N), int(M), int(max_boxes))
        rc = lib().rbp_session_create_reserved(C.byref(self._h), dev_worlds._h, C.byref(cap), C.byref(self._p))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_create_reserved rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_create_reserved failed rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
        self.param, self.device = param, dev_worlds.device
        self.K, self.plans, self.slot_of, self._N = 0, [], None, int(N)
        self._keep = (dev_worlds,)
        self._pl = (A.rbp_plan * 0)()
        if opts is not None:
            self.set_solver_opts(opts)
        return self

    def refill(self, search, max_boxes=None, stream=None):
        """replace the session's missions by those a device search solved (rbp_session_refill_from_ecbs): one staged copy and one kernel
        on `stream`, nothing allocated, nothing synchronised.  `plans`, `K` and `slot_of` are rebuilt as by from_ecbs; the search may be
        closed once `stream` has been synchronised (run + download or a report do).  A refusal (ValueError) leaves the session as it was."""
        import numpy as np
        if not isinstance(search, DeviceEcbs):
            raise TypeError("Session.refill takes a DeviceEcbs")
        if not search._h:
            raise RuntimeError("DeviceEcbs is closed")
        slot_of = np.zeros(search.K, np.int32)
        rc = lib().rbp_session_refill_from_ecbs(self._h, search._h, int(max_boxes or 0), A.ptr(slot_of, A.c_int32_p), C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_refill_from_ecbs rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_refill_from_ecbs failed rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
        self._missions_of(search, slot_of, max_boxes)

    def reserve_plan_stage(self, bytes=0):
        """reserve the pinned staging block of refill_plans, its device twin and its event with `bytes` of room
        (rbp_session_reserve_plan_stage); 0: the capacity's missions in one round, up to 64 MiB.  Optional: the first refill_plans does it
        with 0.  Less than one mission of the capacity's shape (plan_stage_bytes(capacity, 1)) or a second size: ValueError."""
        rc = lib().rbp_session_reserve_plan_stage(self._h, int(bytes))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_reserve_plan_stage rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_reserve_plan_stage failed rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")

    def refill_plans(self, worlds, missions, plans, stream=None):
        """replace the session's missions by a caller's own (rbp_session_refill_from_plans): host plans with T and init_traj from any
        front-end, their missions, and worlds whose grids lie on the session's device (DeviceWorlds items), which must stay alive until
        the next refill.  Staged copies and one kernel per round on `stream`, nothing allocated once the staging block exists, nothing
        synchronised.  `plans` become the session's for download(), `K` follows, `slot_of` becomes None.  A refusal (ValueError) leaves
        the session as it was."""
        K = len(plans)
        if len(worlds) != K or len(missions) != K:
            raise ValueError("refill_plans: worlds, missions and plans must have one entry per mission")
        w = (A.rbp_world * K)(*[x.c_struct() for x in worlds])
        m = (A.rbp_mission * K)(*[x.c_struct() for x in missions])
        pl = (A.rbp_plan * K)(*[p.c_struct() for p in plans])
        rc = lib().rbp_session_refill_from_plans(self._h, K, w, m, pl, C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_refill_from_plans rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_refill_from_plans failed rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
        self._keep_refill = (worlds, missions)   # (the grids are referenced in place)
        self.K, self.slot_of, self._N = K, None, plans[0].N
        self._plans, self._pl = list(plans), pl

    @property
    def capacity(self):
        """(K, N, M, max_boxes) the session's arena was laid out for (rbp_session_capacity_of): what a refill may bring"""
        cap = A.rbp_session_capacity()
        rc = lib().rbp_session_capacity_of(self._h, C.byref(cap))
        if rc:
            raise RuntimeError(f"rbp_session_capacity_of rc={rc}: {last_error()}")
        return (cap.K, cap.N, cap.M, cap.max_boxes)

    def set_solver_opts(self, opts=None, **kw):
        """rbp_solver_opts of this session (before its next run): Session.set_solver_opts(qp_schedule=2) or an object from solver_opts()"""
        o = opts if opts is not None else solver_opts(**kw)
        rc = lib().rbp_session_set_solver_opts(self._h, C.byref(o))
        if rc:
            raise RuntimeError(f"rbp_session_set_solver_opts rc={rc}: {last_error()}")

    def run(self, stages=A.RBP_STAGE_ALL, stream=None):
        self._xchg_error = None   # (an exchange hook's exception belongs to the run it happened in)
        rc = lib().rbp_session_run(self._h, stages, C.c_void_p(stream or 0))
        if rc:
            cause = getattr(self, "_xchg_error", None)
            raise RuntimeError(f"rbp_session_run rc={rc}: {last_error()}" + (f" ({cause!r})" if cause is not None else ""))

    def run_async(self, stages=A.RBP_STAGE_ALL, stream=None):
        """`run` that returns at once for a grid-wide joint session too (the solve proceeds on a library thread; `wait`, `download`
        and every other call on the session wait for it): include/rbp.h rbp_session_run_async"""
        rc = lib().rbp_session_run_async(self._h, stages, C.c_void_p(stream or 0))
        if rc:
            raise RuntimeError(f"rbp_session_run_async rc={rc}: {last_error()}")

    def wait(self):
        rc = lib().rbp_session_wait(self._h)
        if rc:
            raise RuntimeError(f"rbp_session_wait rc={rc}: {last_error()}")

    def shard_joint(self, dist, group=None):
        """make this session one rank of a PAIR that shares a joint solve (include/rbp.h rbp_session_shard_joint): rank 0 of `group`
        (default: the whole process group, which must have two ranks) eliminates the lower chain of the knots, rank 1 the upper one; the
        three exchanges per interior-point iteration are all-gathers on the library's device buffers -- RCCL over xGMI under the "nccl"
        backend, through host copies under "gloo" (tests: two ranks on one GPU).  dist=None undoes it."""
        import torch
        if dist is None:
            rc = lib().rbp_session_shard_joint(self._h, 0, 1, EXCHANGE_FN(), None)
            self._xchg = None
            self._xchg_error = None
            if rc:
                raise RuntimeError(f"rbp_session_shard_joint rc={rc}: {last_error()}")
            return
        ws, rank = dist.get_world_size(group), dist.get_rank(group)
        if ws != 2:
            raise ValueError(f"a joint solve is shared by TWO ranks (the twisted elimination has two chains); the group has {ws}")
        gloo = dist.get_backend(group) == "gloo"
        sess = self
        dev = torch.device("cuda", self.device)
        self._xchg_error = None

        class _View:
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}

        def hook(user, send_ptr, recv_ptr, nbytes):
            try:
                n = nbytes // 8
                send = torch.as_tensor(_View(send_ptr, n), device=dev)   # (the library's buffers live on the session's device)
                recv = torch.as_tensor(_View(recv_ptr, n), device=dev)
                if gloo:
                    outs = [torch.empty(n, dtype=torch.float64) for _ in range(2)]
                    dist.all_gather(outs, send.cpu(), group=group)
                    recv.copy_(outs[1 - rank])
                else:
                    out = torch.empty(2 * n, dtype=torch.float64, device=send.device)
                    dist.all_gather_into_tensor(out, send, group=group)
                    recv.copy_(out[(1 - rank) * n:(2 - rank) * n])
                torch.cuda.synchronize(dev)
                sess.exchanges += 1
                sess.exchange_bytes += nbytes
                return 0
            except BaseException as e:  # (an exception must not unwind through the C frames of the library)
                sess._xchg_error = e
                return 1

        self.exchanges, self.exchange_bytes = 0, 0
        self._xchg = EXCHANGE_FN(hook)  # (kept alive as long as the session may call it)
        rc = lib().rbp_session_shard_joint(self._h, rank, 2, self._xchg, None)
        if rc:
            raise RuntimeError(f"rbp_session_shard_joint rc={rc}: {last_error()}")

    def set_agent_range(self, agent_begin: int, agent_end: int):
        rc = lib().rbp_session_set_agent_range(self._h, agent_begin, agent_end)
        if rc:
            raise RuntimeError(f"rbp_session_set_agent_range rc={rc}: {last_error()}")

    def reset(self, stream=None):
        rc = lib().rbp_session_reset(self._h, C.c_void_p(stream or 0))
        if rc:
            raise RuntimeError(f"rbp_session_reset rc={rc}: {last_error()}")

    def download(self, stream=None):
        """copies outputs into the PlanResult objects; returns per-mission status list."""
        import numpy as np
        st = np.zeros(self.K, np.int32)
        plans = self.plans   # (made now if nobody has asked for them yet)
        rc = lib().rbp_session_download(self._h, self._pl, A.ptr(st, A.c_int32_p), C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT and self.K == 0:   # (a reserved session before its first refill; a mission's status is never this code)
            raise ValueError(f"rbp_session_download rc={rc}: {last_error()}")
        for p, c in zip(plans, self._pl):
            p.sync_from(c)
        return st.tolist()

    def report(self, dt=0.1, stream=None):
        """the missions' safety ratios and flight distances, computed where the plans lie (rbp_session_report): a list of K Report records,
        the bits host.report gives for the downloaded plans.  Nothing is downloaded and nothing of the session changes; a mission whose
        status is not 0 comes back with that status and nothing computed."""
        out = (A.rbp_report * self.K)()
        rc = lib().rbp_session_report(self._h, dt, out, C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_report rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_report rc={rc}: {last_error()}")
        return [Report.from_c(r) for r in out]

    def dynamics(self, dt=0.1, states=False, curves=False, device_out=False, stream=None):
        """the missions' limit peaks and, where asked for, their sampled states and ratio curves, computed where the plans lie
        (rbp_session_dynamics): (records, states, curves) -- K Dynamics records, the bits host.dynamics gives for the downloaded plans;
        states [K][N][9][S] (agent, row = derivative * 3 + axis, sample) and curves [K][S][2] (smallest, largest safety ratio of a sample),
        or None where not asked for.  S is the largest number of samples of a mission, from report() (at least 1); mission k's entries
        beyond records[k].samples are zero.  device_out: the two arrays are torch tensors on the session's device, written in place by
        the kernels; otherwise numpy arrays.  Nothing of the session changes; a mission whose status is not 0 comes back with that
        status, nothing computed and nothing stored."""
        import numpy as np
        S, N = 1, self._N
        if states or curves:
            S = max([1] + [r.samples for r in self.report(dt, stream)])
        out = (A.rbp_dynamics * self.K)()
        if device_out:
            import torch
            dev = torch.device("cuda", self.device)
            st = torch.zeros((self.K, N, 9, S), dtype=torch.float64, device=dev) if states else None
            cu = torch.zeros((self.K, S, 2), dtype=torch.float64, device=dev) if curves else None
            torch.cuda.synchronize(dev)   # (the zeros are written on torch's stream, the kernels run on `stream`)
            sp, cp = (st.data_ptr() if states else None), (cu.data_ptr() if curves else None)
        else:
            st = np.zeros((self.K, N, 9, S)) if states else None
            cu = np.zeros((self.K, S, 2)) if curves else None
            sp, cp = (st.ctypes.data if states else None), (cu.ctypes.data if curves else None)
        rc = lib().rbp_session_dynamics(self._h, dt, out, C.c_void_p(sp), C.c_void_p(cp), S, C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_dynamics rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_dynamics rc={rc}: {last_error()}")
        return [Dynamics.from_c(r) for r in out], st, cu

    def clearance(self, dt=0.1, per_agent=False, device_out=False, stream=None):
        """the missions' clearance to the obstacles of their worlds, computed where the plans and the grids lie (rbp_session_clearance):
        (records, agents) -- K Clearance records, the bits host.clearance gives for the downloaded plans on the downloaded grids; agents
        [K][N], every agent's smallest clearance (1e9 without a sample), or None unless per_agent.  device_out: the array is a torch tensor
        on the session's device, written in place by the kernel; otherwise a numpy array.  The row of a mission that is not computed keeps
        its 1e9.  Nothing of the session changes; a mission whose status is not 0 comes back with that status and nothing computed."""
        import numpy as np
        N = self._N
        out = (A.rbp_clearance * self.K)()
        ag, ap = None, None
        if per_agent and device_out:
            import torch
            dev = torch.device("cuda", self.device)
            ag = torch.full((self.K, N), 1e9, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)   # (the fill is written on torch's stream, the kernels run on `stream`)
            ap = ag.data_ptr()
        elif per_agent:
            ag = np.full((self.K, N), 1e9)
            ap = ag.ctypes.data
        rc = lib().rbp_session_clearance(self._h, dt, out, C.c_void_p(ap), C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_clearance rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_clearance rc={rc}: {last_error()}")
        return [Clearance.from_c(r) for r in out], ag

    def separation(self, depth=4, refine_below=2.0, per_pair=False, device_out=False, stream=None):
        """a certified interval for the missions' smallest safety ratio in continuous time, computed where the plans lie
        (rbp_session_separation): (records, pairs) -- K Separation records, the bits host.separation gives for the downloaded plans;
        pairs [K][N (N-1) / 2], every pair's smallest lower ratio in the pair order of a plan (1e9 where there is none), or None unless
        per_pair.  depth: the pieces of a refined item are 2^depth; refine_below: items whose depth-0 lower ratio is below it are
        refined.  device_out: the array is a torch tensor on the session's device, written in place by the kernels; otherwise a numpy
        array.  The row of a mission that is not computed keeps its 1e9.  Nothing of the session changes; a mission whose status is not 0
        comes back with that status and nothing computed."""
        import numpy as np
        N = self._N
        npair = N * (N - 1) // 2
        out = (A.rbp_separation * self.K)()
        pl, pp = None, None
        if per_pair and device_out:
            import torch
            dev = torch.device("cuda", self.device)
            pl = torch.full((self.K, npair), 1e9, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)   # (the fill is written on torch's stream, the kernels run on `stream`)
            pp = pl.data_ptr()
        elif per_pair:
            pl = np.full((self.K, npair), 1e9)
            pp = pl.ctypes.data
        rc = lib().rbp_session_separation(self._h, depth, refine_below, out, C.c_void_p(pp), C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_separation rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_separation rc={rc}: {last_error()}")
        return [Separation.from_c(r) for r in out], pl

    def swept_clearance(self, depth=4, refine_below=0.5, per_agent=False, device_out=False, stream=None):
        """a certified interval for the missions' smallest clearance to the obstacles in continuous time, computed where the plans and the
        grids lie (rbp_session_swept_clearance): (records, agents) -- K SweptClearance records, the bits host.swept_clearance gives for the
        downloaded plans on the downloaded grids; agents [K][N], every agent's smallest lower clearance (1e9 where there is none), or None
        unless per_agent.  depth: the pieces of a refined item are 2^depth; refine_below: items whose depth-0 lower clearance is below it,
        or whose depth-0 box leaves the grid or the cell budget, are refined (1e9: all).  device_out: the array is a torch tensor on the
        session's device, written in place by the kernels; otherwise a numpy array.  The row of a mission that is not computed keeps its
        1e9.  Nothing of the session changes; a mission whose status is not 0 comes back with that status and nothing computed."""
        import numpy as np
        N = self._N
        out = (A.rbp_swept_clearance * self.K)()
        ag, ap = None, None
        if per_agent and device_out:
            import torch
            dev = torch.device("cuda", self.device)
            ag = torch.full((self.K, N), 1e9, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)   # (the fill is written on torch's stream, the kernels run on `stream`)
            ap = ag.data_ptr()
        elif per_agent:
            ag = np.full((self.K, N), 1e9)
            ap = ag.ctypes.data
        rc = lib().rbp_session_swept_clearance(self._h, depth, refine_below, out, C.c_void_p(ap), C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_swept_clearance rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_swept_clearance rc={rc}: {last_error()}")
        return [SweptClearance.from_c(r) for r in out], ag

    def limits(self, depth=4, refine_above=0.5, per_agent=False, device_out=False, stream=None):
        """certified intervals for the missions' largest velocity and acceleration, as fractions of the agents' limits, in continuous time,
        computed where the plans lie (rbp_session_limits): (records, agents) -- K Limits records, the bits host.limits gives for the
        downloaded plans; agents [K][N][2], every agent's largest upper velocity and acceleration ratio (0 where there is none), or None
        unless per_agent.  depth: the pieces of a refined item are 2^depth; refine_above: items with a depth-0 upper ratio above it are
        refined (negative: all).  device_out: the array is a torch tensor on the session's device, written in place by the kernels;
        otherwise a numpy array.  The row of a mission that is not computed keeps its zeros.  Nothing of the session changes; a mission
        whose status is not 0 comes back with that status and nothing computed."""
        import numpy as np
        N = self._N
        out = (A.rbp_limits * self.K)()
        ag, ap = None, None
        if per_agent and device_out:
            import torch
            dev = torch.device("cuda", self.device)
            ag = torch.zeros((self.K, N, 2), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)   # (the fill is written on torch's stream, the kernels run on `stream`)
            ap = ag.data_ptr()
        elif per_agent:
            ag = np.zeros((self.K, N, 2))
            ap = ag.ctypes.data
        rc = lib().rbp_session_limits(self._h, depth, refine_above, out, C.c_void_p(ap), C.c_void_p(stream or 0))
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_session_limits rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_session_limits rc={rc}: {last_error()}")
        return [Limits.from_c(r) for r in out], ag

    def reserve_workspace(self, stream=None):
        """reserve the QP workspace now (otherwise the first PLANNER run does)"""
        rc = lib().rbp_session_reserve_workspace(self._h, C.c_void_p(stream or 0))
        if rc:
            raise RuntimeError(f"rbp_session_reserve_workspace rc={rc}: {last_error()}")

    def workspace_bytes_per_mission(self):
        return int(lib().rbp_session_workspace_bytes(self._h))

    def counters(self, stream=None):
        ct = A.rbp_counters()
        rc = lib().rbp_session_counters(self._h, C.byref(ct), C.c_void_p(stream or 0))
        if rc:
            raise RuntimeError(f"rbp_session_counters rc={rc}: {last_error()}")
        return {k: getattr(ct, k) for k, _ in ct._fields_}

    def device_arrays(self, mission=0):
        """torch tensors over mission `mission`'s corridor arrays in the session's HBM arena (no copy): dict with sfc_count [N] i32,
        sfc_box [N][MB][6] f64, sfc_time [N][MB] f64, rsfc_normal [npair][M][3] f32, rsfc_time [M] f64 (MB, M: session strides)."""
        import torch
        da = A.rbp_device_arrays()
        rc = lib().rbp_session_device_arrays(self._h, mission, C.byref(da))
        if rc:
            raise RuntimeError(f"rbp_session_device_arrays rc={rc}: {last_error()}")

        class _View:  # __cuda_array_interface__ holder (torch on ROCm reads it like on CUDA)
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2}

        dev = torch.device("cuda", da.device)
        def view(ptr, shape, typestr):
            return torch.as_tensor(_View(ptr, shape, typestr), device=dev)
        N, M, MB, npair = da.N, da.M, da.max_boxes, da.npair
        return {"sfc_count": view(da.sfc_count, (N,), "<i4"), "sfc_box": view(da.sfc_box, (N, MB, 6), "<f8"),
                "sfc_time": view(da.sfc_time, (N, MB), "<f8"), "rsfc_normal": view(da.rsfc_normal, (max(npair, 1), M, 3), "<f4")[:npair],
                "rsfc_time": view(da.rsfc_time, (M,), "<f8"), "status": view(da.status, (1,), "<i4"), "_keepalive": self}

    def scalars(self, n=24, stream=None):
        import numpy as np
        out = np.zeros((self.K, n))
        rc = lib().rbp_session_scalars(self._h, A.ptr(out, A.c_double_p), n, C.c_void_p(stream or 0))
        if rc:
            raise RuntimeError(f"rbp_session_scalars rc={rc}: {last_error()}")
        return out

    def close(self):
        if self._h:
            lib().rbp_session_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def report_coefs(M, T, coef, radius, downwash, dt=0.1, time_scale=None, device=0):
    """rbp_dev_report: the report kernels on the caller's arrays, uploaded once -- coefficients from anywhere, the reference's own log for
    one.  M [K] segments per mission; T [K][S + 1] unscaled times (S >= max M, M[k] + 1 entries of row k used); coef [K][N][3][6 S] with
    mission k's own [N][3][6 M[k]] packed at the front of its slot (a session's layout: for M[k] == S simply [N][3][6 S]); radius [K][N];
    time_scale [K] or None.  Returns K Report records, the bits host.report gives for the scaled times."""
    import numpy as np
    M = np.ascontiguousarray(M, np.int32).reshape(-1)
    K = len(M)
    T, coef, radius = A.as_f64(T).reshape(K, -1), A.as_f64(coef), A.as_f64(radius).reshape(K, -1)
    S, N = T.shape[1] - 1, radius.shape[1]
    if coef.size != K * N * 3 * 6 * S:
        raise ValueError(f"coef holds {coef.size} doubles, K * N * 3 * 6 * M_stride = {K * N * 3 * 6 * S}")
    ts = None if time_scale is None else A.as_f64(time_scale).reshape(K)
    out = (A.rbp_report * K)()
    rc = lib().rbp_dev_report(device, K, N, A.ptr(M, A.c_int32_p), S, A.ptr(T, A.c_double_p), A.ptr(ts, A.c_double_p), A.ptr(coef, A.c_double_p),
                              A.ptr(radius, A.c_double_p), downwash, dt, out)
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"rbp_dev_report rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"rbp_dev_report rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return [Report.from_c(r) for r in out]


def dynamics_coefs(M, T, coef, radius, max_vel, max_acc, downwash, dt=0.1, time_scale=None, states=None, curves=None, S_stride=0, device=0):
    """rbp_dev_dynamics: the dynamics kernels on the caller's arrays, uploaded once, in report_coefs' layout with max_vel / max_acc
    [K][N][3].  states / curves: None, a C-contiguous float64 numpy array ([K][N][9][S_stride] / [K][S_stride][2]) or a torch tensor of
    that shape on `device`, written in place -- a mission's entries up to its samples where samples <= S_stride, nothing else.
    Returns K Dynamics records, the bits host.dynamics gives for the scaled times."""
    import numpy as np
    M = np.ascontiguousarray(M, np.int32).reshape(-1)
    K = len(M)
    T, coef, radius = A.as_f64(T).reshape(K, -1), A.as_f64(coef), A.as_f64(radius).reshape(K, -1)
    S, N = T.shape[1] - 1, radius.shape[1]
    max_vel, max_acc = A.as_f64(max_vel).reshape(K, N, 3), A.as_f64(max_acc).reshape(K, N, 3)
    if coef.size != K * N * 3 * 6 * S:
        raise ValueError(f"coef holds {coef.size} doubles, K * N * 3 * 6 * M_stride = {K * N * 3 * 6 * S}")
    ts = None if time_scale is None else A.as_f64(time_scale).reshape(K)

    def address(a, count):
        if a is None:
            return None
        if isinstance(a, np.ndarray):
            if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"] or a.size != count:
                raise ValueError(f"a destination must be a C-contiguous float64 array of {count} elements")
            return a.ctypes.data
        if str(a.dtype) != "torch.float64" or not a.is_contiguous() or a.numel() != count:
            raise ValueError(f"a destination must be a contiguous float64 tensor of {count} elements")
        return a.data_ptr()

    sp, cp = address(states, K * N * 9 * S_stride), address(curves, K * S_stride * 2)
    out = (A.rbp_dynamics * K)()
    rc = lib().rbp_dev_dynamics(device, K, N, A.ptr(M, A.c_int32_p), S, A.ptr(T, A.c_double_p), A.ptr(ts, A.c_double_p), A.ptr(coef, A.c_double_p),
                                A.ptr(radius, A.c_double_p), A.ptr(max_vel, A.c_double_p), A.ptr(max_acc, A.c_double_p), downwash, dt, out,
                                C.c_void_p(sp), C.c_void_p(cp), int(S_stride))
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"rbp_dev_dynamics rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"rbp_dev_dynamics rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return [Dynamics.from_c(r) for r in out]


def clearance_coefs(M, T, coef, radius, worlds, dt=0.1, time_scale=None, agent_clearance=None, device=0):
    """rbp_dev_clearance: the clearance kernels on the caller's arrays, uploaded once, in report_coefs' layout, and K worlds (World: a host
    grid, uploaded once per distinct grid; DeviceWorld: referenced in place).  agent_clearance: None, a C-contiguous float64 numpy array
    [K][N] or a torch tensor of that shape on `device`, written in place -- the rows of the missions that are computed, nothing else.
    Returns K Clearance records, the bits host.clearance gives for the scaled times."""
    import numpy as np
    M = np.ascontiguousarray(M, np.int32).reshape(-1)
    K = len(M)
    T, coef, radius = A.as_f64(T).reshape(K, -1), A.as_f64(coef), A.as_f64(radius).reshape(K, -1)
    S, N = T.shape[1] - 1, radius.shape[1]
    if coef.size != K * N * 3 * 6 * S:
        raise ValueError(f"coef holds {coef.size} doubles, K * N * 3 * 6 * M_stride = {K * N * 3 * 6 * S}")
    if len(worlds) != K:
        raise ValueError(f"{len(worlds)} worlds for {K} missions")
    ts = None if time_scale is None else A.as_f64(time_scale).reshape(K)
    ap = None
    if isinstance(agent_clearance, np.ndarray):
        if agent_clearance.dtype != np.float64 or not agent_clearance.flags["C_CONTIGUOUS"] or agent_clearance.size != K * N:
            raise ValueError(f"agent_clearance must be a C-contiguous float64 array of {K * N} elements")
        ap = agent_clearance.ctypes.data
    elif agent_clearance is not None:
        if str(agent_clearance.dtype) != "torch.float64" or not agent_clearance.is_contiguous() or agent_clearance.numel() != K * N:
            raise ValueError(f"agent_clearance must be a contiguous float64 tensor of {K * N} elements")
        ap = agent_clearance.data_ptr()
    ws = (A.rbp_world * K)(*[w.c_struct() for w in worlds])
    out = (A.rbp_clearance * K)()
    rc = lib().rbp_dev_clearance(device, K, N, A.ptr(M, A.c_int32_p), S, A.ptr(T, A.c_double_p), A.ptr(ts, A.c_double_p), A.ptr(coef, A.c_double_p),
                                 A.ptr(radius, A.c_double_p), ws, dt, out, C.c_void_p(ap))
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"rbp_dev_clearance rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"rbp_dev_clearance rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return [Clearance.from_c(r) for r in out]


def swept_clearance_coefs(M, T, coef, radius, worlds, depth=4, refine_below=0.5, time_scale=None, agent_lower=None, device=0):
    """rbp_dev_swept_clearance: the swept clearance kernels on the caller's arrays, uploaded once, in report_coefs' layout, and K worlds
    (World: a host grid, uploaded once per distinct grid; DeviceWorld: referenced in place).  agent_lower: None, a C-contiguous float64
    numpy array [K][N] or a torch tensor of that shape on `device`, written in place.  Returns K SweptClearance records, the bits
    host.swept_clearance gives for the scaled times."""
    import numpy as np
    M = np.ascontiguousarray(M, np.int32).reshape(-1)
    K = len(M)
    T, coef, radius = A.as_f64(T).reshape(K, -1), A.as_f64(coef), A.as_f64(radius).reshape(K, -1)
    S, N = T.shape[1] - 1, radius.shape[1]
    if coef.size != K * N * 3 * 6 * S:
        raise ValueError(f"coef holds {coef.size} doubles, K * N * 3 * 6 * M_stride = {K * N * 3 * 6 * S}")
    if len(worlds) != K:
        raise ValueError(f"{len(worlds)} worlds for {K} missions")
    ts = None if time_scale is None else A.as_f64(time_scale).reshape(K)
    ap = None
    if isinstance(agent_lower, np.ndarray):
        if agent_lower.dtype != np.float64 or not agent_lower.flags["C_CONTIGUOUS"] or agent_lower.size != K * N:
            raise ValueError(f"agent_lower must be a C-contiguous float64 array of {K * N} elements")
        ap = agent_lower.ctypes.data
    elif agent_lower is not None:
        if str(agent_lower.dtype) != "torch.float64" or not agent_lower.is_contiguous() or agent_lower.numel() != K * N:
            raise ValueError(f"agent_lower must be a contiguous float64 tensor of {K * N} elements")
        ap = agent_lower.data_ptr()
    ws = (A.rbp_world * K)(*[w.c_struct() for w in worlds])
    out = (A.rbp_swept_clearance * K)()
    rc = lib().rbp_dev_swept_clearance(device, K, N, A.ptr(M, A.c_int32_p), S, A.ptr(T, A.c_double_p), A.ptr(ts, A.c_double_p),
                                       A.ptr(coef, A.c_double_p), A.ptr(radius, A.c_double_p), ws, depth, refine_below, out, C.c_void_p(ap))
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"rbp_dev_swept_clearance rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"rbp_dev_swept_clearance rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return [SweptClearance.from_c(r) for r in out]


def limits_coefs(M, T, coef, max_vel, max_acc, depth=4, refine_above=0.5, time_scale=None, agent_upper=None, device=0):
    """rbp_dev_limits: the limits kernels on the caller's arrays, uploaded once, in report_coefs' layout with max_vel / max_acc [K][N][3].
    agent_upper: None, a C-contiguous float64 numpy array [K][N][2] or a torch tensor of that shape on `device`, written in place.
    Returns K Limits records, the bits host.limits gives for the scaled times."""
    import numpy as np
    M = np.ascontiguousarray(M, np.int32).reshape(-1)
    K = len(M)
    T, coef, max_vel = A.as_f64(T).reshape(K, -1), A.as_f64(coef), A.as_f64(max_vel).reshape(K, -1, 3)
    S, N = T.shape[1] - 1, max_vel.shape[1]
    max_acc = A.as_f64(max_acc).reshape(K, N, 3)
    if coef.size != K * N * 3 * 6 * S:
        raise ValueError(f"coef holds {coef.size} doubles, K * N * 3 * 6 * M_stride = {K * N * 3 * 6 * S}")
    ts = None if time_scale is None else A.as_f64(time_scale).reshape(K)
    ap = None
    if isinstance(agent_upper, np.ndarray):
        if agent_upper.dtype != np.float64 or not agent_upper.flags["C_CONTIGUOUS"] or agent_upper.size != K * N * 2:
            raise ValueError(f"agent_upper must be a C-contiguous float64 array of {K * N * 2} elements")
        ap = agent_upper.ctypes.data
    elif agent_upper is not None:
        if str(agent_upper.dtype) != "torch.float64" or not agent_upper.is_contiguous() or agent_upper.numel() != K * N * 2:
            raise ValueError(f"agent_upper must be a contiguous float64 tensor of {K * N * 2} elements")
        ap = agent_upper.data_ptr()
    out = (A.rbp_limits * K)()
    rc = lib().rbp_dev_limits(device, K, N, A.ptr(M, A.c_int32_p), S, A.ptr(T, A.c_double_p), A.ptr(ts, A.c_double_p), A.ptr(coef, A.c_double_p),
                              A.ptr(max_vel, A.c_double_p), A.ptr(max_acc, A.c_double_p), depth, refine_above, out, C.c_void_p(ap))
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"rbp_dev_limits rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"rbp_dev_limits rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return [Limits.from_c(r) for r in out]


def separation_coefs(M, T, coef, radius, downwash, depth=4, refine_below=2.0, time_scale=None, pair_lower=None, device=0):
    """rbp_dev_separation: the separation kernels on the caller's arrays, uploaded once, in report_coefs' layout.  pair_lower: None, a
    C-contiguous float64 numpy array [K][N (N-1) / 2] or a torch tensor of that shape on `device`, written in place.  Returns K Separation
    records, the bits host.separation gives for the scaled times."""
    import numpy as np
    M = np.ascontiguousarray(M, np.int32).reshape(-1)
    K = len(M)
    T, coef, radius = A.as_f64(T).reshape(K, -1), A.as_f64(coef), A.as_f64(radius).reshape(K, -1)
    S, N = T.shape[1] - 1, radius.shape[1]
    npair = N * (N - 1) // 2
    if coef.size != K * N * 3 * 6 * S:
        raise ValueError(f"coef holds {coef.size} doubles, K * N * 3 * 6 * M_stride = {K * N * 3 * 6 * S}")
    ts = None if time_scale is None else A.as_f64(time_scale).reshape(K)
    pp = None
    if isinstance(pair_lower, np.ndarray):
        if pair_lower.dtype != np.float64 or not pair_lower.flags["C_CONTIGUOUS"] or pair_lower.size != K * npair:
            raise ValueError(f"pair_lower must be a C-contiguous float64 array of {K * npair} elements")
        pp = pair_lower.ctypes.data
    elif pair_lower is not None:
        if str(pair_lower.dtype) != "torch.float64" or not pair_lower.is_contiguous() or pair_lower.numel() != K * npair:
            raise ValueError(f"pair_lower must be a contiguous float64 tensor of {K * npair} elements")
        pp = pair_lower.data_ptr()
    out = (A.rbp_separation * K)()
    rc = lib().rbp_dev_separation(device, K, N, A.ptr(M, A.c_int32_p), S, A.ptr(T, A.c_double_p), A.ptr(ts, A.c_double_p), A.ptr(coef, A.c_double_p),
                                  A.ptr(radius, A.c_double_p), downwash, depth, refine_below, out, C.c_void_p(pp))
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"rbp_dev_separation rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"rbp_dev_separation rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return [Separation.from_c(r) for r in out]


def build_world(keys, res, param: Param, max_dist=1.0):
    """The distance grid of a world ON THE GPU (rbp_edt_build): DynamicEDTOctomap(maxDist, tree, world_min, world_max, false).update()
    (swarm_traj_planner_rbp_test_all.cpp:57-63) + getDistance on every voxel centre.  Same result, bit for bit, as host.build_world."""
    import numpy as np
    from .types import World
    keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 4)
    lo = (C.c_double * 3)(param.world_x_min, param.world_y_min, param.world_z_min)
    hi = (C.c_double * 3)(param.world_x_max, param.world_y_max, param.world_z_max)
    dim, kmin = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    rc = lib().rbp_edt_dims(res, lo, hi, dim, kmin)
    if rc:
        raise ValueError(f"rbp_edt_dims rc={rc}: {last_error()}")
    dist = np.zeros(tuple(dim), np.float32)
    rc = lib().rbp_edt_build(A.ptr(keys, A.c_int32_p), len(keys), res, lo, hi, max_dist, A.ptr(dist, A.c_float_p))
    if rc:
        raise RuntimeError(f"rbp_edt_build rc={rc}: {last_error()}")
    return World(dist, tuple(kmin), res)


def _box(param: Param):
    return ((C.c_double * 3)(param.world_x_min, param.world_y_min, param.world_z_min),
            (C.c_double * 3)(param.world_x_max, param.world_y_max, param.world_z_max))


class DeviceWorlds:
    """rbp_dev_worlds (include/rbp.h): the distance grids of a set of worlds built in one call and kept in HBM.  keys_list / res_list:
    per world what host.load_octomap returns; the box is param's.  len(), indexing (-> DeviceWorld) and close(); an item keeps the set
    alive, and a closed set's items must not be used any more.  Every grid equals host.build_world's, bit for bit."""

    def __init__(self, keys_list, res_list, param: Param, max_dist=1.0, device=0):
        import numpy as np
        W = len(keys_list)
        if len(res_list) != W:
            raise ValueError("keys_list and res_list must have one entry per world")
        keys = [np.ascontiguousarray(k, np.int32).reshape(-1, 4) for k in keys_list]
        kp = (A.c_int32_p * max(W, 1))(*[A.ptr(k, A.c_int32_p) for k in keys])
        nl = (C.c_int64 * max(W, 1))(*[len(k) for k in keys])
        res = np.ascontiguousarray(res_list, np.float64)
        lo, hi = _box(param)
        self._h = C.c_void_p()
        self.device = int(device)
        rc = lib().rbp_dev_worlds_create(C.byref(self._h), self.device, W, kp, nl, A.ptr(res, A.c_double_p), lo, hi, max_dist)
        if rc == A.RBP_ERR_BAD_ARGUMENT:
            raise ValueError(f"rbp_dev_worlds_create rc={rc}: {last_error()}")
        if rc:
            raise RuntimeError(f"rbp_dev_worlds_create rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
        self._items = []
        for w in range(W):
            g = A.rbp_world()
            rc = lib().rbp_dev_worlds_get(self._h, w, C.byref(g))
            if rc:
                raise RuntimeError(f"rbp_dev_worlds_get rc={rc}: {last_error()}")
            self._items.append(DeviceWorld(C.cast(g.dist, C.c_void_p).value, tuple(g.dim), tuple(g.key_min), g.res, self.device, owner=self, index=w))

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        if not self._h:
            raise RuntimeError("DeviceWorlds is closed")
        return self._items[i]

    def _download(self, w):
        import numpy as np
        if not self._h:
            raise RuntimeError("DeviceWorlds is closed")
        dist = np.zeros(self._items[w].shape, np.float32)
        rc = lib().rbp_dev_worlds_download(self._h, w, A.ptr(dist, A.c_float_p))
        if rc:
            raise RuntimeError(f"rbp_dev_worlds_download rc={rc}: {last_error()}")
        return dist

    def close(self):
        if self._h:
            lib().rbp_dev_worlds_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ecbs_obstacles(dev_world: DeviceWorld, mission: Mission, param: Param):
    """host.ecbs_obstacles from a grid that stays on the GPU (rbp_dev_worlds_ecbs_obstacles): one thread per sample of the planning lattice,
    and the mask [dimx][dimy][dimz] comes back instead of the grid.  `dev_world`: an item of a DeviceWorlds."""
    from . import host
    ws = dev_world._owner
    if not isinstance(ws, DeviceWorlds):
        raise TypeError("planner.ecbs_obstacles takes an item of a DeviceWorlds (rbp_dev_worlds_ecbs_obstacles addresses a world of a set)")
    if not ws._h:
        raise RuntimeError("DeviceWorlds is closed")
    ms, ps = mission.c_struct(), param.c_struct()
    rc, mask = host.obstacle_mask(lambda dim, buf, cap: lib().rbp_dev_worlds_ecbs_obstacles(ws._h, dev_world._index, C.byref(ms), C.byref(ps), dim, buf, cap))
    if rc in host.ECBS_ERROR_TEXT:
        raise RuntimeError(host.ECBS_ERROR_TEXT[rc])
    if rc:
        raise RuntimeError(f"rbp_dev_worlds_ecbs_obstacles rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return mask


def ecbs_plan(dev_world: DeviceWorld, mission: Mission, param: Param, max_nodes=200000) -> PlanResult:
    """host.ecbs_plan for a world on the GPU: the obstacle mask from the resident grid, then the host search; same result, same errors."""
    from . import host
    return host.ecbs_plan_obstacles(ecbs_obstacles(dev_world, mission, param), mission, param, max_nodes)


class EcbsOut:
    """rbp_ecbs_out (include/rbp.h) for K missions of N agents: the caller-owned arrays of one device search and their C struct"""

    def __init__(self, K, N, max_M):
        import numpy as np
        self.K, self.N, self.max_M = K, N, max_M
        self.status, self.M, self.makespan, self.sum_cost = (np.zeros(K, np.int32) for _ in range(4))
        self.high_level, self.low_level = np.zeros(K, np.int64), np.zeros(K, np.int64)
        self.T = np.zeros((K, max_M + 1), np.float64)
        self.init_traj = np.zeros((K, N, max_M + 1, 3), np.float32)

    def c_struct(self):
        o = A.rbp_ecbs_out()
        o.max_M = self.max_M
        o.status, o.M, o.makespan, o.sum_cost = (A.ptr(a, A.c_int32_p) for a in (self.status, self.M, self.makespan, self.sum_cost))
        o.high_level_expanded, o.low_level_expanded = (A.ptr(a, C.POINTER(C.c_int64)) for a in (self.high_level, self.low_level))
        o.T, o.init_traj = A.ptr(self.T, A.c_double_p), A.ptr(self.init_traj, A.c_float_p)
        return o

    def results(self):
        """one PlanResult with ecbs_stats per mission, None where the mission's status is not 0"""
        res = []
        for k in range(self.K):
            if self.status[k]:
                res.append(None)
                continue
            M = int(self.M[k])
            pr = PlanResult(self.init_traj[k, :, :M + 1].copy(), self.T[k, :M + 1].copy())
            pr.ecbs_stats = dict(makespan=int(self.makespan[k]), sum_cost=int(self.sum_cost[k]), high_level=int(self.high_level[k]),
                                 low_level=int(self.low_level[k]))
            res.append(pr)
        return res


class EcbsPlans(list):
    """what the device searches return: a list of PlanResult (None where the mission's status is not 0) with the `status` array and the
    raw arrays of the call (`out`, an EcbsOut)"""
    status = out = None


def _ecbs_missions(missions):
    missions = list(missions)
    if not missions:
        raise ValueError("need at least one mission")
    keep = [m.c_struct() for m in missions]   # (the structs point into the missions' arrays, which `missions` keeps alive)
    return missions, (A.rbp_mission * len(keep))(*keep)


def _ecbs_finish(name, rc, out):
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"{name} rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"{name} rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    plans = EcbsPlans(out.results())
    plans.status, plans.out = out.status, out
    return plans


def ecbs_plan_masks(masks, missions, param: Param, max_nodes=A.RBP_ECBS_MAX_HIGH_LEVEL_NODES, max_M=64, device=0):
    """host.ecbs_plan_obstacles for K missions in one call, searched on the GPU (rbp_dev_ecbs_plan_masks, kernels/ecbs.hip: one wavefront per
    mission): masks[k] is mission k's obstacle mask [dimx][dimy][dimz] (host.ecbs_obstacles / planner.ecbs_obstacles).  Returns a list of
    PlanResult with ecbs_stats, equal to the host search's bit for bit, None where the mission's `status` (the list's attribute) is not 0:
    1 and 2 are the host's codes, 3 (RBP_ECBS_CAPACITY) says that a capacity of the device search -- max_M, a node pool -- was exceeded;
    nothing falls back to the CPU."""
    import numpy as np
    missions, ms = _ecbs_missions(missions)
    masks = [np.ascontiguousarray(m, np.uint8) for m in masks]
    if len(masks) != len(missions) or any(m.ndim != 3 or m.shape != masks[0].shape for m in masks):
        raise ValueError("need one mask [dimx][dimy][dimz] per mission, all of one shape")
    mp = (C.POINTER(C.c_uint8) * len(masks))(*[m.ctypes.data_as(C.POINTER(C.c_uint8)) for m in masks])
    out = EcbsOut(len(missions), missions[0].qn, int(max_M))
    ps, oc = param.c_struct(), out.c_struct()
    rc = lib().rbp_dev_ecbs_plan_masks(int(device), len(missions), (C.c_int32 * 3)(*masks[0].shape), mp, ms, C.byref(ps), int(max_nodes), C.byref(oc))
    return _ecbs_finish("rbp_dev_ecbs_plan_masks", rc, out)


def ecbs_plan_batch(dev_worlds: DeviceWorlds, world_indices, missions, param: Param, max_nodes=A.RBP_ECBS_MAX_HIGH_LEVEL_NODES, max_M=64):
    """planner.ecbs_plan for K missions in one call, searched on the GPU: mission k on world world_indices[k] of the resident set; the masks
    are made on the device and never leave it (rbp_dev_worlds_ecbs_plan).  Returns what ecbs_plan_masks returns."""
    import numpy as np
    if not isinstance(dev_worlds, DeviceWorlds):
        raise TypeError("planner.ecbs_plan_batch takes a DeviceWorlds")
    if not dev_worlds._h:
        raise RuntimeError("DeviceWorlds is closed")
    missions, ms = _ecbs_missions(missions)
    idx = np.ascontiguousarray(world_indices, np.int32)
    if idx.shape != (len(missions),):
        raise ValueError("need one world index per mission")
    out = EcbsOut(len(missions), missions[0].qn, int(max_M))
    ps, oc = param.c_struct(), out.c_struct()
    rc = lib().rbp_dev_worlds_ecbs_plan(dev_worlds._h, len(missions), A.ptr(idx, A.c_int32_p), ms, C.byref(ps), int(max_nodes), C.byref(oc))
    return _ecbs_finish("rbp_dev_worlds_ecbs_plan", rc, out)


class DeviceEcbs:
    """rbp_dev_ecbs (include/rbp.h): a device search whose results stay in HBM.  `status`, `M` and `ecbs_stats` (per mission, None where the
    status is not 0) are what came back to the host; download() fetches the plans, Session.from_ecbs plans from them where they are."""

    def __init__(self, handle, dev_worlds, K, N, max_M):
        self._h, self._worlds, self.K, self.N, self.max_M, self.device = handle, dev_worlds, K, N, max_M, dev_worlds.device
        self._scalars = self._fetch(False)
        o = self._scalars
        self.status, self.M = o.status, o.M
        self.ecbs_stats = [None if o.status[k] else dict(makespan=int(o.makespan[k]), sum_cost=int(o.sum_cost[k]), high_level=int(o.high_level[k]),
                                                          low_level=int(o.low_level[k])) for k in range(K)]

    def _fetch(self, trajectories):
        if not self._h:
            raise RuntimeError("DeviceEcbs is closed")
        out = EcbsOut(self.K, self.N, self.max_M)
        oc = out.c_struct()
        if not trajectories:
            oc.T, oc.init_traj = None, None
        rc = lib().rbp_dev_ecbs_download(self._h, C.byref(oc))
        if rc:
            raise RuntimeError(f"rbp_dev_ecbs_download rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
        return out

    def download(self):
        """the EcbsPlans ecbs_plan_batch returns for the same arguments, T / init_traj written on the device and copied back once"""
        return _ecbs_finish("rbp_dev_ecbs_download", 0, self._fetch(True))

    def close(self):
        if self._h:
            lib().rbp_dev_ecbs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ecbs_search_batch(dev_worlds: DeviceWorlds, world_indices, missions, param: Param, max_nodes=A.RBP_ECBS_MAX_HIGH_LEVEL_NODES, max_M=64):
    """ecbs_plan_batch whose results stay on the device (rbp_dev_worlds_ecbs_search): returns a DeviceEcbs.  The DeviceWorlds must outlive it."""
    import numpy as np
    if not isinstance(dev_worlds, DeviceWorlds):
        raise TypeError("planner.ecbs_search_batch takes a DeviceWorlds")
    if not dev_worlds._h:
        raise RuntimeError("DeviceWorlds is closed")
    missions, ms = _ecbs_missions(missions)
    idx = np.ascontiguousarray(world_indices, np.int32)
    if idx.shape != (len(missions),):
        raise ValueError("need one world index per mission")
    ps, h = param.c_struct(), C.c_void_p()
    rc = lib().rbp_dev_worlds_ecbs_search(dev_worlds._h, len(missions), A.ptr(idx, A.c_int32_p), ms, C.byref(ps), int(max_nodes), int(max_M), C.byref(h))
    if rc == A.RBP_ERR_BAD_ARGUMENT:
        raise ValueError(f"rbp_dev_worlds_ecbs_search rc={rc}: {last_error()}")
    if rc:
        raise RuntimeError(f"rbp_dev_worlds_ecbs_search rc={rc}: {ERROR_TEXT.get(rc, '')} | {last_error()}")
    return DeviceEcbs(h, dev_worlds, len(missions), missions[0].qn, int(max_M))
