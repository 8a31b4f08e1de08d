"""A pure Python restatement of the swept clearance rule (csrc/common/swept_rules.h), beside tests/synth_report.py, whose synthetic plans it
reuses, and tests/synth_clearance.py, whose grids and lookup it reuses; shared by tests/test_swept_host.py (CPU) and tests/test_gpu_swept.py.

`restate` walks one mission as the rule's sequential loop does, in Python floats (IEEE doubles, one rounding per operation): h of the two
scaled times, its powers, the Bernstein form with weights C(k,i) / C(5,i) as one rounded quotient, A, de Casteljau halvings along the bits of
a piece, the box min - e / max + e with e = ((20 + 5 D) 2^-53) A, the keys with numpy.float32 for the cast and math.floor, the in-grid test,
the budget, the smallest cell of the box in a numpy grid, the two end lookups, the flags, fixed refinement, and the minima under the rule's
order.  Nothing is shared with the C++ text but the IEEE operations themselves, so rbp_swept_clearance_host must equal it bit for bit.

`exact_pieces` gives, in fractions.Fraction, the control points of every piece of the polynomial the doubles define (exact h, exact Bernstein
form, exact halvings): what the rule's widened boxes must contain.  `boxes` gives the rule's widened [lo, hi] per piece.

The widening is COUNTED here (u = 2^-53; a chain of n roundings is off by a factor within (1 + u)^n; every exact control point is at most
A = sum |alpha_i| h^i in size):
  h        Ts[m+1] - Ts[m]                                                  1 rounding
  hp_i     h^i by i - 1 products of the computed h                          i + (i - 1)
  g_i      alpha_i * hp_i, alpha a given double                             (2 i - 1) + 1
  beta_k   term i passes the weight, its product and k - i + 1 sums         2 i + 2 + (k - i + 1) <= 13
  halving  (a + b) * 0.5, five rounds per level, the product exact          5 per level
  A        |alpha_i| * |hp_i| through at most five sums                     (2 i - 1) + 1 + 5 <= 15, which shrinks e
  e        (c u) * A, the first product exact                               1, which shrinks e
  corner   min - e, max + e                                                 1, of a number of about A in size
`counted_constant(D)` walks that table: point + 1 (the corner) + 1 (what 16 roundings take from e, rounded up) -- 15 + 5 D; the header's
20 + 5 D must not be smaller.
"""
import math
from fractions import Fraction as F
from math import comb

import numpy as np

from swarm_simulator_amd import host
from swarm_simulator_amd.types import SweptClearance
from tests import synth_clearance as L

NONE = 1e9
OUTSIDE = -1.0
EPSILON = 1e-6
MAX_CELLS = 4096
U = 2.0 ** -53


def counted_constant(depth):
    hp = lambda i: i + (i - 1)
    g = lambda i: hp(i) + 1 if i else 0
    beta = max([g(0) + k for k in range(6)] + [g(i) + 2 + (k - i + 1) for k in range(6) for i in range(1, k + 1)])
    return beta + 5 * depth + 1 + 1


def rule_constant(depth):
    return 20 + 5 * depth


# ---- the rule in floats -----------------------------------------------------------------------------------------------------------
def _powers(h):
    hp = [1.0, h]
    for i in range(2, 6):
        hp.append(hp[i - 1] * h)
    return hp


def _bernstein(alpha, hp):
    g = [alpha[0]] + [alpha[i] * hp[i] for i in range(1, 6)]
    beta = []
    for k in range(6):
        s = g[0]
        for i in range(1, k + 1):
            t = (float(comb(k, i)) / float(comb(5, i))) * g[i]
            s = s + t
        beta.append(s)
    return beta


def _size(alpha, hp):
    s = abs(alpha[0])
    for i in range(1, 6):
        t = abs(alpha[i]) * abs(hp[i])
        s = s + t
    return s


def _halve(b, right):
    b = list(b)
    left = [b[0]]
    for r in range(1, 6):
        for i in range(6 - r):
            b[i] = (b[i] + b[i + 1]) * 0.5
        left.append(b[0])
    return b if right else left


def _piece(b3, depth, p):
    for l in range(depth):
        right = (p >> (depth - 1 - l)) & 1
        b3 = [_halve(b, right) for b in b3]
    return b3


def _item(T, c, m):
    """T scaled; c [3][6 M] of one agent: (control points [3][6], A [3])"""
    h = float(T[m + 1]) - float(T[m])
    hp = _powers(h)
    b3, A3 = [], []
    for k in range(3):
        alpha = [float(c[k][6 * m + 5 - i]) for i in range(6)]
        b3.append(_bernstein(alpha, hp))
        A3.append(_size(alpha, hp))
    return b3, A3


def _interval(b, e):
    mn = mx = b[0]
    for x in b[1:]:
        if x < mn or x != x:
            mn = x
        if x > mx or x != x:
            mx = x
    return mn - e, mx + e


def _key(rf, x):
    with np.errstate(over="ignore", invalid="ignore"):
        xf = float(np.float32(x))
    v = rf * xf
    return v if (math.isnan(v) or math.isinf(v)) else math.floor(v)


def piece_box(b3, A3, depth):
    """the widened [lo, hi] of a piece's three axes"""
    out = []
    for k in range(3):
        e = (float(rule_constant(depth)) * U) * A3[k]
        out.append(_interval(b3[k], e))
    return out


def readings(world, b3, A3, depth):
    """(d_lo, d_up, outside, over_budget, cells) of a piece from its control points"""
    rf = 1.0 / world.res
    box = piece_box(b3, A3, depth)
    outside, i0, n = False, [], []
    for k in range(3):
        kl, kh = _key(rf, box[k][0]), _key(rf, box[k][1])
        first, end = world.key_min[k], world.key_min[k] + world.dist.shape[k]
        if not (kl >= first and kh < end):
            outside = True
        else:
            i0.append(kl - first), n.append(kh - kl + 1)
    cells = 0 if outside else n[0] * n[1] * n[2]
    over = (not outside) and cells > MAX_CELLS
    if outside or over:
        d_lo = OUTSIDE
    else:
        sub = world.dist[i0[0]:i0[0] + n[0], i0[1]:i0[1] + n[1], i0[2]:i0[2] + n[2]]
        vals = sub[~np.isnan(sub)]
        d_lo = float(vals.min()) if vals.size else math.inf
    d0, _ = L.lookup(world, [b3[0][0], b3[1][0], b3[2][0]])
    d1, _ = L.lookup(world, [b3[0][5], b3[1][5], b3[2][5]])
    d_up = d1 if (d1 < d0 or d1 != d1) else d0
    return d_lo, d_up, outside, over, cells


def _precedes(c, m):
    """candidates (clearance, dist, segment, piece, agent, depth)"""
    if c[0] < m[0]:
        return True
    if not c[0] == m[0]:
        return False
    return (c[2], c[3], c[4]) < (m[2], m[3], m[4])


def restate(T, coef, radius, world, depth, refine_below, stats=None):
    """of ONE mission (T scaled [M + 1], coef [N][3][6 M], radius [N]): (SweptClearance, agents [N]).  stats: a list that receives the cell
    count of every depth-0 box that was scanned"""
    T = [float(x) for x in T]
    M, N = len(T) - 1, coef.shape[0]
    coef = np.asarray(coef, np.float64).reshape(N, 3, 6 * M)
    lower = upper = (NONE, 0.0, -1, -1, -1, -1)
    counts = [0, 0, 0, 0, 0]   # uncertified, hitting, outside, over budget, refined
    agents = []
    for a in range(N):
        r = float(radius[a])
        al = NONE
        for m in range(M):
            b3, A3 = _item(T, coef[a], m)
            r0 = readings(world, b3, A3, 0)
            if stats is not None and not (r0[2] or r0[3]):
                stats.append(r0[4])
            refined = r0[2] or r0[3] or not (r0[0] - r >= refine_below)
            pieces = [(depth, p, readings(world, _piece(b3, depth, p), A3, depth)) for p in range(1 << depth)] if refined else [(0, 0, r0)]
            il, flags = NONE, [False] * 4
            for D, p, (d_lo, d_up, outside, over, _) in pieces:
                lo, up = d_lo - r, d_up - r
                if _precedes((lo, d_lo, m, p, a, D), lower):
                    lower = (lo, d_lo, m, p, a, D)
                if _precedes((up, d_up, m, p, a, D), upper):
                    upper = (up, d_up, m, p, a, D)
                if lo < il:
                    il = lo
                flags = [flags[0] or d_lo < r - EPSILON, flags[1] or d_up < r - EPSILON, flags[2] or outside, flags[3] or over]
            for i in range(4):
                counts[i] += bool(flags[i])
            counts[4] += bool(refined)
            if il < al:
                al = il
        agents.append(al)
    rec = SweptClearance(lower[0], upper[0], lower[1], upper[1], T[M], counts[0], counts[1], counts[2], counts[3], counts[4],
                         lower[2], lower[3], lower[4], lower[5], upper[2], upper[3], upper[4], upper[5], 0)
    return rec, np.array(agents)


def restate_plans(plans, worlds, depth, refine_below):
    """`restate` of every mission of a synth_report.Plans: (records, agents [K][N])"""
    recs, agents = [], np.zeros((plans.K, plans.N))
    for k in range(plans.K):
        r, ag = restate(plans.scaled_T(k), plans.coefs[k], plans.radius[k], worlds[k], depth, refine_below)
        recs.append(r)
        agents[k] = ag
    return recs, agents


def boxes(T, c, m, depth):
    """the rule's widened boxes of the 2^depth pieces of segment m of one agent (c [3][6 M]): a list of [(lo, hi)] * 3, in floats"""
    b3, A3 = _item([float(x) for x in T], c, m)
    return [piece_box(_piece(b3, depth, p), A3, depth) for p in range(1 << depth)]


# ---- the exact polynomial ----------------------------------------------------------------------------------------------------------
def _exact_halve(b, right):
    left, b = [b[0]], list(b)
    for r in range(1, 6):
        b = [(b[i] + b[i + 1]) / 2 for i in range(6 - r)] + b[6 - r:]
        left.append(b[0])
    return b if right else left


def exact_pieces(T, c, m, depth, only=None):
    """the exact control points [3][6] of the pieces `only` (default: all 2^depth) of segment m of one agent, as Fractions"""
    h = F(float(T[m + 1])) - F(float(T[m]))
    b3 = []
    for k in range(3):
        alpha = [F(float(c[k][6 * m + 5 - i])) for i in range(6)]
        b3.append([sum(F(comb(kk, i), comb(5, i)) * alpha[i] * h ** i for i in range(kk + 1)) for kk in range(6)])
    out = []
    for p in (range(1 << depth) if only is None else only):
        b = b3
        for l in range(depth):
            right = (p >> (depth - 1 - l)) & 1
            b = [_exact_halve(x, right) for x in b]
        out.append(b)
    return out


def exact_position(T, c, m, s):
    """the exact position [3] at the fraction s in [0, 1] of segment m, as Fractions"""
    h = F(float(T[m + 1])) - F(float(T[m]))
    t = h * s
    return [sum(F(float(c[k][6 * m + 5 - i])) * t ** i for i in range(6)) for k in range(3)]


# ---- fixed cases -------------------------------------------------------------------------------------------------------------------
def wall():
    """the wall the samples miss: res 0.1, clamp 1.0, a one-cell-thick plane of zeros at x in [2.0, 2.1); one agent of radius 0.15 flies
    x = 0.05 + 8 t for one segment of 0.5 s, y = z = 1.05.  (world, mission, plan)"""
    from swarm_simulator_amd.types import Mission, PlanResult, World
    d = np.full((45, 21, 21), 1.0, np.float32)
    d[20, :, :] = 0.0
    world = World(d, (0, 0, 0), 0.1)
    c = np.zeros((1, 3, 6))
    c[0, 0, 4], c[0, 0, 5], c[0, 1, 5], c[0, 2, 5] = 8.0, 0.05, 1.05, 1.05
    pr = PlanResult(np.zeros((1, 2, 3), np.float32), np.array([0.0, 0.5]))
    pr.coef[:] = c
    return world, Mission(np.zeros((1, 9)), np.zeros((1, 9)), np.full(1, 0.15), np.ones((1, 3)), np.ones((1, 3))), pr


def host_swept(plans, worlds, depth, refine_below, fill=-7.0):
    """rbp_swept_clearance_host of every mission of `plans` on worlds[k] (host Worlds): (records, agents [K][N] pre-filled with `fill`)"""
    import ctypes as C
    from swarm_simulator_amd import _abi as A
    recs, agents = [], np.full((plans.K, plans.N), fill)
    for k in range(plans.K):
        mission, pl = plans.mission(k), plans.plan(k)   # (kept alive: the structs point into their arrays)
        ws, ms = worlds[k].c_struct(), mission.c_struct()
        out = A.rbp_swept_clearance()
        rc = host.lib().rbp_swept_clearance_host(C.byref(ws), C.byref(ms), pl.M, A.ptr(pl.T, A.c_double_p), A.ptr(pl.coef, A.c_double_p), depth,
                                                 refine_below, C.byref(out), A.ptr(agents[k], A.c_double_p))
        assert rc == 0, rc
        recs.append(SweptClearance.from_c(out))
    return recs, agents
