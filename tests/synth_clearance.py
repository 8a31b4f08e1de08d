"""A pure Python restatement of the clearance rule (csrc/common/clearance_rules.h) and seeded synthetic grids, beside tests/synth_report.py,
whose synthetic plans it reuses; shared by tests/test_clearance_host.py (CPU) and tests/test_gpu_clearance.py.

`restate` walks one mission as the rule's sequential loop does, in Python floats (IEEE doubles, one rounding per operation): the samples
floor(T[M] / dt), the double t = j * dt, the segment of a sample, Horner positions; the lookup with numpy.float32 for the cast to
octomap's point3d, math.floor for the key (a Python int: no range to leave), the in-grid test, the cell in a numpy grid, -1 outside; the
clearance d - radius, the hit d < radius - 1e-6, and the minimum under the rule's order (smallest clearance, then the first (sample,
agent); a NaN never).  Nothing is shared with the C++ text but the IEEE operations themselves, so rbp_clearance_host must equal it bit for bit.

`host_clearances(plans, worlds, dt)` gives what rbp_clearance_host says of each mission of a synth_report.Plans on its world (times scaled by
the IEEE product, as rbp_session_download hands them out) -- the reference of the GPU tests.
"""
import math

import numpy as np

from swarm_simulator_amd import host
from swarm_simulator_amd.types import Clearance, World

MAX_SAMPLES = 1 << 20   # RBP_REPORT_MAX_SAMPLES
NONE = 1e9
EPSILON = 1e-6          # SP_EPSILON_FLOAT


def grid(seed, shape, key_min, res, clamp=1.0):
    """a seeded distance grid: about a fifth of the cells obstacles (0), the rest uniform up to the clamp, a fifth of them AT the clamp"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, clamp, shape).astype(np.float32)
    kind = rng.uniform(0.0, 1.0, shape)
    d[kind < 0.2] = 0.0
    d[kind > 0.8] = clamp
    return World(d, tuple(int(k) for k in key_min), float(res))


def lookup(world, p):
    """(d, inside) of position p [3] (Python floats)"""
    rf = 1.0 / world.res
    idx = []
    for a in range(3):
        with np.errstate(over="ignore", invalid="ignore"):
            pf = float(np.float32(p[a]))
        x = rf * pf
        if math.isnan(x) or math.isinf(x):
            return -1.0, False
        kd = math.floor(x)
        if not (kd >= world.key_min[a] and kd < world.key_min[a] + world.dist.shape[a]):
            return -1.0, False
        idx.append(kd - world.key_min[a])
    return float(world.dist[idx[0], idx[1], idx[2]]), True


def restate(T, coef, radius, world, dt):
    """of ONE mission (T scaled [M + 1], coef [N][3][6 M], radius [N]): (Clearance, agents [N] or None where nothing is evaluated)"""
    T = [float(x) for x in T]
    M, N = len(T) - 1, coef.shape[0]
    c = np.asarray(coef, np.float64).reshape(N, 3, M, 6)
    end = T[M]
    q = math.floor(end / dt) if math.isfinite(end / dt) else end / dt
    if q > MAX_SAMPLES:
        return Clearance(NONE, 0.0, end, 0, 0, -1, -1, -1, 0), None
    samples = int(q) if q >= 1 else 0
    best = (NONE, 0.0, -1, -1)
    agents = [NONE] * N
    hits = outside = 0
    for j in range(samples):
        t = float(j) * dt
        before = 0
        while before < M and T[before] < t:
            before += 1
        m = max(before - 1, 0)
        tseg = t - T[before - 1] if before > 0 else t
        for a in range(N):
            p = []
            for k in range(3):
                v = float(c[a, k, m, 0])
                for i in range(1, 6):
                    v = v * tseg
                    v = v + float(c[a, k, m, i])
                p.append(v)
            d, inside = lookup(world, p)
            r = float(radius[a])
            cl = d - r
            if d < r - EPSILON:
                hits += 1
            if not inside:
                outside += 1
            if cl < best[0]:        # (samples ascend, then agents: the first among equals stays)
                best = (cl, d, j, a)
            if cl < agents[a]:
                agents[a] = cl
    return Clearance(best[0], best[1], end, hits, outside, samples, best[2], best[3], 0), np.array(agents)


def restate_plans(plans, worlds, dt):
    """`restate` of every mission of a synth_report.Plans: (records, agents [K][N] with rows of missions not evaluated left at -7)"""
    recs, agents = [], np.full((plans.K, plans.N), -7.0)
    for k in range(plans.K):
        r, ag = restate(plans.scaled_T(k), plans.coefs[k], plans.radius[k], worlds[k], dt)
        recs.append(r)
        if ag is not None:
            agents[k] = ag
    return recs, agents


def host_clearances(plans, worlds, dt, fill=-7.0):
    """rbp_clearance_host of every mission of `plans` on worlds[k] (host Worlds): (records, agents [K][N] pre-filled with `fill`)"""
    import ctypes as C
    from swarm_simulator_amd import _abi as A
    recs, agents = [], np.full((plans.K, plans.N), fill)
    for k in range(plans.K):
        mission, pl = plans.mission(k), plans.plan(k)   # (kept alive: the structs point into their arrays)
        ws, ms = worlds[k].c_struct(), mission.c_struct()
        out = A.rbp_clearance()
        rc = host.lib().rbp_clearance_host(C.byref(ws), C.byref(ms), pl.M, A.ptr(pl.T, A.c_double_p), A.ptr(pl.coef, A.c_double_p), dt, C.byref(out),
                                           A.ptr(agents[k], A.c_double_p))
        assert rc == 0, rc
        recs.append(Clearance.from_c(out))
    return recs, agents
