"""A pure Python restatement of the limits rule (csrc/common/limits_rules.h), beside tests/synth_report.py, whose synthetic plans it reuses;
shared by tests/test_limits_host.py (CPU) and tests/test_gpu_limits.py.

`restate` walks one mission as the rule's sequential loop does, in Python floats (IEEE doubles, one rounding per operation, no
contraction): h of the two scaled times, its powers, the derivative's coefficients as the products state_rules forms, the Bernstein form of
degree n with weights C(k,i) / C(n,i) as one rounded quotient, V, de Casteljau halvings along the bits of a piece, err = ((16 + 4 D) 2^-53) V,
the two quotients moved two doubles outwards, the flags, fixed refinement, and the peaks under the rule's order.  Nothing is shared with the
C++ text but the IEEE operations themselves, so rbp_limits_host must equal it bit for bit.

`exact_pieces` gives, in fractions.Fraction, the control points of every piece of the derivative of the polynomial the doubles define
(exact products, exact h, exact Bernstein form, exact halvings); `pieces` gives the rule's computed control points and err; `exact_value`
the derivative at a rational point.

The error term is COUNTED here (u = 2^-53; a chain of r roundings is off by a factor within (1 + u)^r; every exact control point is at most
V = sum |gamma_i| h^i in size):
  gamma_i  (5 - i) c[i]                                                     1 rounding
  h        Ts[m+1] - Ts[m]                                                  1
  hp_i     h^i by i - 1 products of the computed h                          i + (i - 1)
  g_i      gamma_i * hp_i                                                   1 + (2 i - 1) + 1
  b_k      term i passes the weight, its product and k - i + 1 sums         2 i + 1 + 2 + (k - i + 1) <= 2 n + 4
  halving  (a + b) * 0.5, n rounds per level, the product exact             n per level
  V, err   what their roundings take from err, rounded up                   1
  bound    max + err, ends - err                                            1, of a number of about V in size
`counted_constant(D)` walks that table for n = 4, the larger: 14 + 4 D; the header's 16 + 4 D must not be smaller.
"""
import math
import struct
from fractions import Fraction as F
from math import comb

import numpy as np

from swarm_simulator_amd import host
from swarm_simulator_amd.types import Limits, Mission

U = 2.0 ** -53
ULPS = 2
DEGREE = {"vel": 4, "acc": 3}


def counted_constant(depth, n=4):
    hp = lambda i: i + (i - 1)
    g = lambda i: 1 + hp(i) + 1 if i else 1
    point = max([g(0) + k for k in range(n + 1)] + [g(i) + 2 + (k - i + 1) for k in range(n + 1) for i in range(1, k + 1)])
    return point + n * depth + 1 + 1


def rule_constant(depth):
    return 16 + 4 * depth


# ---- the rule in floats -----------------------------------------------------------------------------------------------------------
def _powers(h):
    hp = [1.0, h]
    for i in range(2, 6):
        hp.append(hp[i - 1] * h)
    return hp


def _gamma(c, n):
    """ascending coefficients of the derivative of degree n from the six descending-power coefficients c"""
    out = []
    for j in range(n + 1):
        i = n - j
        out.append(float(5 - i) * c[i] if n == 4 else float((5 - i) * (4 - i)) * c[i])
    return out


def _bernstein(gamma, hp, n):
    g = [gamma[0]] + [gamma[i] * hp[i] for i in range(1, n + 1)]
    beta = []
    for k in range(n + 1):
        s = g[0]
        for i in range(1, k + 1):
            t = (float(comb(k, i)) / float(comb(n, i))) * g[i]
            s = s + t
        beta.append(s)
    return beta


def _size(gamma, hp, n):
    s = abs(gamma[0])
    for i in range(1, n + 1):
        t = abs(gamma[i]) * abs(hp[i])
        s = s + t
    return s


def _halve(b, right):
    b, n = list(b), len(b) - 1
    left = [b[0]]
    for r in range(1, n + 1):
        for i in range(n + 1 - r):
            b[i] = (b[i] + b[i + 1]) * 0.5
        left.append(b[0])
    return b if right else left


def _piece(b, depth, p):
    for l in range(depth):
        b = _halve(b, (p >> (depth - 1 - l)) & 1)
    return b


def _bits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def _of_bits(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def _down(v, n=ULPS):
    if not v < math.inf:
        return v
    b = _bits(v)
    return _of_bits(b - n if b > n else 0)


def _up(v, n=ULPS):
    if not v < math.inf or v == 0.0:
        return v
    return _of_bits(min(_bits(v) + n, 0x7FF0000000000000))


def _div(a, b):
    if b == 0.0:   # (Python raises where IEEE does not)
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _ratio(value, limit):
    q = _div(value, limit)
    return q if limit > 0.0 else math.nan


def _bounds(b, err, limit):
    mx = abs(b[0])
    for x in b[1:]:
        x = abs(x)
        if x > mx or x != x:
            mx = x
    first, last = abs(b[0]), abs(b[-1])
    ends = last if (last > first or last != last) else first
    lo = ends - err
    lower_num = 0.0 if lo <= 0.0 else lo
    return _down(_ratio(lower_num, limit)), _up(_ratio(mx + err, limit))


def _poly(T, c_axis, m, kind):
    """(control points of the whole segment, V) of one axis' derivative on segment m; c_axis [6 M]"""
    n = DEGREE[kind]
    h = float(T[m + 1]) - float(T[m])
    hp = _powers(h)
    gamma = _gamma([float(x) for x in c_axis[6 * m:6 * m + 6]], n)
    return _bernstein(gamma, hp, n), _size(gamma, hp, n)


def pieces(T, c_axis, m, kind, depth):
    """the rule's computed control points of the 2^depth pieces of one axis' derivative, and err: ([points], err) in floats"""
    whole, V = _poly(T, c_axis, m, kind)
    return [_piece(whole, depth, p) for p in range(1 << depth)], (float(rule_constant(depth)) * U) * V


def _precedes(c, m):
    """candidates (ratio, segment, piece, agent, axis, depth)"""
    if c[0] > m[0]:
        return True
    if not c[0] == m[0]:
        return False
    return c[1:5] < m[1:5]


NO_PEAK = (0.0, -1, -1, -1, -1, -1)


def restate(T, coef, max_vel, max_acc, depth, refine_above):
    """of ONE mission (T scaled [M + 1], coef [N][3][6 M], limits [N][3]): (Limits, agents [N][2])"""
    T = [float(x) for x in T]
    M, N = len(T) - 1, coef.shape[0]
    coef = np.asarray(coef, np.float64).reshape(N, 3, 6 * M)
    limit = {"vel": np.asarray(max_vel, np.float64).reshape(N, 3), "acc": np.asarray(max_acc, np.float64).reshape(N, 3)}
    peaks = {("lower", "vel"): NO_PEAK, ("upper", "vel"): NO_PEAK, ("lower", "acc"): NO_PEAK, ("upper", "acc"): NO_PEAK}
    counts = [0, 0, 0]   # uncertified, violating, refined
    agents = np.zeros((N, 2))

    def evaluate(a, m, D):
        """(candidates, state) of the 2^D pieces of item (a, m); state: upper vel, upper acc, uncertified, violating, a NaN"""
        cands, st = [], [0.0, 0.0, False, False, False]
        for k in range(3):
            for col, kind in enumerate(("vel", "acc")):
                pts, err = pieces(T, coef[a][k], m, kind, D)
                for p, b in enumerate(pts):
                    lo, up = _bounds(b, err, float(limit[kind][a][k]))
                    cands.append((("lower", kind), (lo, m, p, a, k, D)))
                    cands.append((("upper", kind), (up, m, p, a, k, D)))
                    nan = up != up
                    u = math.inf if nan else up
                    if u > st[col]:
                        st[col] = u
                    st[2], st[3], st[4] = st[2] or not up <= 1.0, st[3] or lo > 1.0, st[4] or nan
        return cands, st

    for a in range(N):
        for m in range(M):
            cands, st = evaluate(a, m, 0)
            refined = st[4] or not st[0] <= refine_above or not st[1] <= refine_above
            if refined:
                cands, st = evaluate(a, m, depth)
            for key, c in cands:
                if _precedes(c, peaks[key]):
                    peaks[key] = c
            counts[0] += bool(st[2])
            counts[1] += bool(st[3])
            counts[2] += bool(refined)
            agents[a][0], agents[a][1] = max(agents[a][0], st[0]), max(agents[a][1], st[1])
    lv, uv, la, ua = (peaks[("lower", "vel")], peaks[("upper", "vel")], peaks[("lower", "acc")], peaks[("upper", "acc")])
    rec = Limits(lv[0], uv[0], la[0], ua[0], T[M], counts[0], counts[1], counts[2], *lv[1:], *uv[1:], *la[1:], *ua[1:], 0)
    return rec, agents


# ---- the exact polynomial ----------------------------------------------------------------------------------------------------------
def exact_gamma(c_axis, m, kind):
    n = DEGREE[kind]
    c = [F(float(x)) for x in c_axis[6 * m:6 * m + 6]]
    return [((5 - (n - j)) if n == 4 else (5 - (n - j)) * (4 - (n - j))) * c[n - j] for j in range(n + 1)]


def _exact_halve(b, right):
    n = len(b) - 1
    left, b = [b[0]], list(b)
    for r in range(1, n + 1):
        b = [(b[i] + b[i + 1]) / 2 for i in range(n + 1 - r)] + b[n + 1 - r:]
        left.append(b[0])
    return b if right else left


def exact_pieces(T, c_axis, m, kind, depth, only=None):
    """(the exact control points of the pieces `only` (default: all), the exact V) of one axis' derivative on segment m, as Fractions"""
    n = DEGREE[kind]
    h = F(float(T[m + 1])) - F(float(T[m]))
    gamma = exact_gamma(c_axis, m, kind)
    whole = [sum(F(comb(k, i), comb(n, i)) * gamma[i] * h ** i for i in range(k + 1)) for k in range(n + 1)]
    out = []
    for p in (range(1 << depth) if only is None else only):
        b = whole
        for l in range(depth):
            b = _exact_halve(b, (p >> (depth - 1 - l)) & 1)
        out.append(b)
    return out, sum(abs(gamma[i]) * abs(h) ** i for i in range(n + 1))


def exact_value(T, c_axis, m, kind, s):
    """the derivative at the fraction s in [0, 1] of segment m, as a Fraction"""
    h = F(float(T[m + 1])) - F(float(T[m]))
    gamma = exact_gamma(c_axis, m, kind)
    return sum(g * (h * s) ** i for i, g in enumerate(gamma))


# ---- fixed cases and helpers -------------------------------------------------------------------------------------------------------
def random_limits(seed, K, N, low=0.05, high=0.6):
    """max_vel, max_acc [K][N][3]: of the size of the synthetic plans' derivatives, so that ratios fall on both sides of 1"""
    rng = np.random.default_rng(seed)
    return rng.uniform(low, high, (K, N, 3)), rng.uniform(2 * low, 4 * high, (K, N, 3))


def mission_of(plans, k, max_vel, max_acc):
    N = plans.N
    return Mission(np.zeros((N, 9)), np.zeros((N, 9)), plans.radius[k].copy(), np.array(max_vel[k], np.float64).reshape(N, 3),
                   np.array(max_acc[k], np.float64).reshape(N, 3))


def parabola():
    """the peak the samples miss: one agent, one segment of one second, x = -1.6 t^3 + 2.4 t^2, so v = 4.8 t (1 - t) with its peak 1.2 at
    t = 0.5; max_vel 1.17.  (mission, plan)"""
    from swarm_simulator_amd.types import PlanResult
    c = np.zeros((1, 3, 6))
    c[0, 0] = [0, 0, -1.6, 2.4, 0, 0]
    pr = PlanResult(np.zeros((1, 2, 3), np.float32), np.array([0.0, 1.0]))
    pr.coef[:] = c
    return Mission(np.zeros((1, 9)), np.zeros((1, 9)), np.full(1, 0.15), np.full((1, 3), 1.17), np.full((1, 3), 10.0)), pr


def host_limits(plans, max_vel, max_acc, depth, refine_above, fill=-7.0):
    """rbp_limits_host of every mission of `plans`: (records, agents [K][N][2] pre-filled with `fill`)"""
    import ctypes as C
    from swarm_simulator_amd import _abi as A
    recs, agents = [], np.full((plans.K, plans.N, 2), fill)
    for k in range(plans.K):
        mission, pl = mission_of(plans, k, max_vel, max_acc), plans.plan(k)   # (kept alive: the structs point into their arrays)
        ms = mission.c_struct()
        out = A.rbp_limits()
        rc = host.lib().rbp_limits_host(C.byref(ms), pl.M, A.ptr(pl.T, A.c_double_p), A.ptr(pl.coef, A.c_double_p), depth, refine_above,
                                        C.byref(out), A.ptr(agents[k], A.c_double_p))
        assert rc == 0, rc
        recs.append(Limits.from_c(out))
    return recs, agents


# ---- the shapes of tests/test_gpu_limits.py ----------------------------------------------------------------------------------------
# N, the missions' M (the stride is the largest), the kinds of their times, their time scales
GPU_SHAPES = {
    "one_lane": (1, [1], ["nonunit"], [1.21]),                                              # one lane of one wavefront
    "across_a_wave": (5, [13, 7, 1], ["nonunit", "alternating", "unit"], [1.21, 1.0, 0.7]),   # 65 slots: inactive m >= M, a second wave of one item
    "two_full_waves": (64, [2], ["alternating"], [1.3]),                                    # exactly 128 items
}


def item_upper0(plans, k, max_vel, max_acc):
    """[N][M[k]]: every item's largest depth-0 upper ratio, velocity or acceleration -- what the rule compares with refine_above"""
    T, M = plans.scaled_T(k), int(plans.M[k])
    coef = plans.coefs[k].reshape(plans.N, 3, 6 * M)
    out = np.zeros((plans.N, M))
    for a in range(plans.N):
        for m in range(M):
            for axis in range(3):
                for kind, lim in (("vel", max_vel), ("acc", max_acc)):
                    pts, err = pieces(T, coef[a][axis], m, kind, 0)
                    out[a][m] = max(out[a][m], _bounds(pts[0], err, float(lim[k][a][axis]))[1])
    return out


def gpu_case(name):
    """(plans, max_vel, max_acc, the refine_above that leaves items of both kinds in every mission -- None for a single item)"""
    from tests import synth_report as S
    N, Ms, kinds, ts = GPU_SHAPES[name]
    plans = S.make(1000 + 7 * N + len(Ms), N, Ms, kinds, ts, spread=0.6)
    mv, ma = random_limits(50 + N, len(Ms), N)
    if N * max(Ms) == 1:
        return plans, mv, ma, None
    ups = [item_upper0(plans, k, mv, ma) for k in range(plans.K)]
    # the median of the mission whose largest item is the smallest (the test on the CPU sees that it parts every mission)
    above = float(np.median(min((u for u in ups if u.size > 1), key=lambda u: float(u.max()))))
    return plans, mv, ma, above


def first_wave_refined(plans, max_vel, max_acc, above):
    """whether each active item of mission 0's first 64 slots (e = a * stride + m, m < M) goes to `depth`"""
    up = item_upper0(plans, 0, max_vel, max_acc)
    M = int(plans.M[0])
    return [not up[e // plans.S][e % plans.S] <= above for e in range(min(64, plans.N * plans.S)) if e % plans.S < M]
