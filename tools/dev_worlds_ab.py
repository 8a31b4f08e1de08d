"""Developer tool (GPU): what it costs to get the 50 sweep worlds (map1..50.bt, the box of Param.test_sweep()) into HBM,

  (a) one rbp_dev_worlds_create: one batched build, the grids stay on the device;
  (b) the route before rbp_dev_worlds: 50 x planner.build_world (rbp_edt_build: per world allocations, a build, a blocking copy back to a
      numpy array, frees) plus the upload of those 50 grids that creating a 50-mission Session performs -- timed as 50 blocking copies of the
      same bytes from the numpy arrays into a preallocated device buffer, since a session's create also uploads everything else.

Host clock around calls that end synchronised, a warm-up of both, then --reps alternating repetitions; median and spread of each.  The grids
of both routes are compared bit for bit first.  Optional libraries built from other sources join the alternation:
  --parent-lib   a librbp_hip.so built from the parent commit: (b) with ITS rbp_edt_build (a memset and five launches per world) as (b-parent)
  --unfused-lib  this tree built with EXTRA=-DEDT_SLAB_MAX_CELLS=0: (a) through the unfused z and y passes as (a-unfused)
--profile runs (a) and (b) once each and nothing else: the command to put under `rocprofv3 --kernel-trace --stats`.

usage: python tools/dev_worlds_ab.py [--reps 9] [--parent-lib PATH] [--unfused-lib PATH] [--out profiles/dev_worlds_ab.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swarm_simulator_amd import _abi as A  # noqa: E402
from swarm_simulator_amd import host, planner  # noqa: E402
from swarm_simulator_amd.types import Param  # noqa: E402


def load(path):
    L = C.CDLL(path)
    L.rbp_edt_dims.argtypes = [C.c_double, C.c_double * 3, C.c_double * 3, C.c_int32 * 3, C.c_int32 * 3]
    L.rbp_edt_build.argtypes = [A.c_int32_p, C.c_int64, C.c_double, C.c_double * 3, C.c_double * 3, C.c_double, A.c_float_p]
    L.rbp_last_error.restype = C.c_char_p
    if hasattr(L, "rbp_dev_worlds_create"):
        P = C.POINTER
        L.rbp_dev_worlds_create.argtypes = [P(C.c_void_p), C.c_int, C.c_int32, P(A.c_int32_p), P(C.c_int64), A.c_double_p, C.c_double * 3, C.c_double * 3,
                                            C.c_double]
        L.rbp_dev_worlds_download.argtypes = [C.c_void_p, C.c_int32, A.c_float_p]
        L.rbp_dev_worlds_destroy.argtypes = [C.c_void_p]
        L.rbp_dev_worlds_destroy.restype = None
    return L


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--maps", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--unfused-lib", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    L = planner.lib()
    if L.rbp_device_count() < 1:
        raise SystemExit("dev_worlds_ab: no HIP device (this measures the GPU; there is nothing to time without one)")
    p = Param.test_sweep()
    octrees = [host.load_octomap(f"map{i}.bt") for i in range(1, args.maps + 1)]
    keys = [np.ascontiguousarray(o[0], np.int32) for o in octrees]
    res = np.array([o[1] for o in octrees], np.float64)
    W = len(keys)
    lo = (C.c_double * 3)(p.world_x_min, p.world_y_min, p.world_z_min)
    hi = (C.c_double * 3)(p.world_x_max, p.world_y_max, p.world_z_max)
    kp = (A.c_int32_p * W)(*[A.ptr(k, A.c_int32_p) for k in keys])
    nl = (C.c_int64 * W)(*[len(k) for k in keys])
    dim, kmin = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    assert L.rbp_edt_dims(res[0], lo, hi, dim, kmin) == 0 and len(set(res.tolist())) == 1   # (the sweep's maps share one resolution)
    shape = tuple(dim)
    staging = torch.empty((W,) + shape, dtype=torch.float32, device="cuda")

    def route_a(lib, keep=False):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.rbp_dev_worlds_create(C.byref(h), 0, W, kp, nl, A.ptr(res, A.c_double_p), lo, hi, 1.0)   # returns when the grids are complete
        dt = time.perf_counter() - t0
        assert rc == 0, lib.rbp_last_error()
        grids = None
        if keep:
            grids = [np.zeros(shape, np.float32) for _ in range(W)]
            for w in range(W):
                assert lib.rbp_dev_worlds_download(h, w, A.ptr(grids[w], A.c_float_p)) == 0
        lib.rbp_dev_worlds_destroy(h)
        return dt, grids

    def route_b(lib):
        t0 = time.perf_counter()
        grids = []
        for w in range(W):   # planner.build_world's body, on `lib`
            dist = np.zeros(shape, np.float32)
            rc = lib.rbp_edt_build(A.ptr(keys[w], A.c_int32_p), len(keys[w]), res[w], lo, hi, 1.0, A.ptr(dist, A.c_float_p))
            assert rc == 0, lib.rbp_last_error()
            grids.append(dist)
        t1 = time.perf_counter()
        for w in range(W):   # the grid upload of a 50-mission session: one blocking copy per grid
            staging[w].copy_(torch.from_numpy(grids[w]))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, grids

    routes = {"a": lambda: route_a(L)[0], "b": lambda: route_b(L)[0]}
    if args.unfused_lib:
        Lu = load(args.unfused_lib)
        routes["a-unfused"] = lambda: route_a(Lu)[0]
    if args.parent_lib:
        Lp = load(args.parent_lib)
        routes["b-parent"] = lambda: route_b(Lp)[0]
    if args.profile:
        route_a(L), route_b(L)
        return 0

    # warm-up and the comparison of the results
    _, ga = route_a(L, keep=True)
    _, build_only, gb = route_b(L)
    same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ga, gb))
    for name, lib in (("a-unfused", args.unfused_lib and Lu), ("b-parent", args.parent_lib and Lp)):
        if lib:
            g = route_a(lib, keep=True)[1] if name == "a-unfused" else route_b(lib)[2]
            same = same and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ga, g))
    times = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, f in routes.items():
            times[k].append(f())
    _, build_only, _ = route_b(L)
    lines = [f"# tools/dev_worlds_ab.py --reps {args.reps}: {W} worlds of {shape[0]} x {shape[1]} x {shape[2]} cells, {sum(len(k) for k in keys)} leaves, "
             f"{torch.cuda.get_device_name(0)}",
             f"grids of all routes bit-identical: {same}"]
    for k, t in times.items():
        ms = sorted(1e3 * x for x in t)
        lines.append(f"({k:10s}) median {statistics.median(ms):9.3f} ms   min {ms[0]:9.3f}   max {ms[-1]:9.3f}   ({len(ms)} alternating repetitions)")
    med = {k: statistics.median(t) for k, t in times.items()}
    lines.append(f"(b) / (a) = {med['b'] / med['a']:.2f}   [(b) of one more run: {1e3 * build_only:.3f} ms in the {W} builds, the rest in the {W} uploads]")
    for k in ("a-unfused", "b-parent"):
        if k in med:
            lines.append(f"({k}) / (a) = {med[k] / med['a']:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if same and med["a"] < med["b"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
