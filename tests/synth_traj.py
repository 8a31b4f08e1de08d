"""Synthetic inputs and an EXACT reference for the trajectory kernels (kernels/traj.hip: dummy_kernel, coef_kernel, timescale_kernel).
TEST INFRASTRUCTURE ONLY: a plain module imported by test_traj_synthetic.py (CPU: the cases keep their promises, the C oracle agrees
with the reference) and test_gpu_traj_synthetic.py (GPU: the kernels agree with the reference).

With plan/sequential = true and batch_iter = 0 no QP is solved (rbp_planner.hpp:119-138): the prologue writes the `dummy` control points
and the epilogue runs on exactly those, so the three kernels are driven with chosen waypoints, segment times and limits.

The reference.  A `dummy` segment is w0 w0 w0 w1 w1 w1: the smoothstep w0 + D (10 s^3 - 15 s^4 + 6 s^5), s = t / dt, D = w1 - w0.
  ctrl        numpy restatement of build_dummy, bit for bit
  coef        fractions.Fraction: float32 waypoints, the integer basis and the double difference dt = T[m+1] - T[m] are rationals, so
              c_k = sum_i v_i B[i][k] / dt^(5-k) is exact; S_k = sum_i |v_i B[i][k]| / dt^(5-k) scales the rounding bound
  time_scale  |velocity| has one peak, at dt / 2.  |acceleration| has two EXACTLY equal peaks, at dt (3 -+ sqrt 3) / 6, and which one
              scale_to_max_acc keeps (`acc_max < acc`, strictly) hangs on the last bit of the evaluation -- in the reference as much as
              in any restatement.  The 1.1 ladder then evaluates acc(t_max / sc) / sc^2, which differs between the peaks.  So a segment
              has a SET of factors: one per admissible t_max (|value| within TIE of the largest), each from the ladder run in Fraction on
              the exact doubles sc = 1.0 * 1.1 * 1.1 ...  A mission's admissible set: every option v with
              max_seg min(options) <= v <= max_seg max(options).
  rule 1      (first two eigenvalues, Eigen 3.3's order) only changes the velocity candidates: that part is the numpy restatement
              make_kkt_reference.time_scale_of(..., "eigen33"); the acceleration part is shared.
"""
import dataclasses
import functools
import math
import os
import sys
from dataclasses import dataclass
from fractions import Fraction as Fr

import numpy as np

from swarm_simulator_amd.types import Mission, Param, PlanResult, World

BASIS = ((-1, 5, -10, 10, -5, 1), (5, -20, 30, -20, 5, 0), (-10, 30, -30, 10, 0, 0), (10, -20, 10, 0, 0, 0), (-5, 5, 0, 0, 0, 0),
         (1, 0, 0, 0, 0, 0))   # Bernstein -> monomial, rows = control point, columns = descending powers (rbp_planner.hpp:338-343)
U = 2.0 ** -53            # unit roundoff: the coefficient bounds are B * U * S_k
MARGIN = 1e-9             # condition (a): every ladder comparison is at least this far (relative) from the limit
TIE = 1e-12               # a candidate time is admissible if its |value| is within this (relative) of the largest
SQRT3 = Fr(math.isqrt(3 * 10 ** 80), 10 ** 40)
HUGE = 1e300

NS = (1, 3, 7)
# every session is ragged; (1, 2), (3, 5), (7, 23): N * 3 * M = 6 (less than a wavefront), 45 (less than the 256 threads), 483 (a partial
# second pass of timescale_kernel's stride loop)
M_OF = {1: (2, 3, 4, 2, 5, 3, 2, 6, 4, 3, 2, 5), 3: (5, 2, 7, 3, 5, 4, 9, 2, 6, 5, 3, 8), 7: (23, 2, 11, 5, 17, 3, 23, 8, 13, 6, 19, 4)}
K_CASES = 12
# the first seed of each case that meets the conditions (case() starts there and still checks; recorded to spare the search)
FIRST_SEED = {(1, 2): 1, (1, 4): 2, (3, 3): 1, (3, 5): 1, (3, 7): 1, (3, 9): 1, (7, 2): 19, (7, 3): 7, (7, 5): 5, (7, 6): 2, (7, 7): 1, (7, 8): 5,
              (7, 9): 1, (7, 10): 2, (7, 11): 1}
B_UNSCALED, B_SCALED = 16, 22   # coefficient bounds in units of U * S_k: see check_plan
T_KIND = ("u1", "u0.5", "u1.7", "u0.125", "rand", "rand", "rand", "rand", "rand", "rand", "ratio8", "rand")
FAR_CASE = 5              # the case whose agents live near x = 50 (cancellation in -1 5 -10 10 -5 1)
# what decides the factor of case idx: None (factor 1: every limit inside the hull shortcut / between the shortcut and the peak / mixed),
# ("vel", rungs) or ("acc", kind): the number of 1.1 rungs through the first / second peak, n1 / n2
DECIDER = (("none", "hull"), ("none", "between"), ("vel", 1), ("acc", "both2"), ("vel", 2), ("acc", "split2"), ("vel", 4), ("acc", "same"),
           ("vel", 8), ("acc", "deep"), ("acc", "both1"), ("acc", "split"))

RES = 0.25                # map and box resolution of the (empty) synthetic worlds
LANE = 3.0                # metres of y per agent: agents never meet
X_SPAN, Z_KEY, Z_DIM = 3.0, 1, 11


def _kkt():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if d not in sys.path:
        sys.path.insert(0, d)
    import make_kkt_reference as K
    return K


# ---------------------------------------------------------------------------------------------------------------------------------
# exact reference
# ---------------------------------------------------------------------------------------------------------------------------------
def dummy_ctrl(init_traj):
    """build_dummy (rbp_planner.hpp:513-549): ctrl [N][3][6M], segment m = w_m w_m w_m w_{m+1} w_{m+1} w_{m+1}"""
    w = np.transpose(np.asarray(init_traj, np.float32).astype(np.float64), (0, 2, 1))
    return np.ascontiguousarray(np.stack([w[:, :, :-1]] * 3 + [w[:, :, 1:]] * 3, axis=3).reshape(w.shape[0], 3, -1))


def exact_coef(ctrl, T):
    """(c, S): object arrays [N][3][6M] of Fraction, c_k = sum_i v_i B[i][k] / dt^(5-k) and S_k = sum_i |v_i B[i][k]| / dt^(5-k)"""
    N, _, oq = ctrl.shape
    c, S = np.empty((N, 3, oq), object), np.empty((N, 3, oq), object)
    T = np.asarray(T, np.float64)
    for m in range(oq // 6):
        dt = Fr(float(T[m + 1] - T[m]))   # the double difference, as the kernel forms it
        ip = [1 / dt ** (5 - k) for k in range(6)]
        for q in range(N):
            for a in range(3):
                v = [Fr(float(x)) for x in ctrl[q, a, 6 * m:6 * m + 6]]
                for k in range(6):
                    terms = [v[i] * BASIS[i][k] for i in range(6)]
                    c[q, a, 6 * m + k] = sum(terms) * ip[k]
                    S[q, a, 6 * m + k] = sum(abs(t) for t in terms) * ip[k]
    return c, S


def to_float(a):
    return np.array([float(x) for x in a.reshape(-1)], np.float64).reshape(a.shape)


def _poly(p, deg, t, sc=None):
    """|sum_i p[i] sc^-(5-i) t^(deg-i)|: the ladder's test value as the reference states it (:783-787, :836-840), exactly"""
    if sc is None:
        return abs(sum(p[i] * t ** (deg - i) for i in range(deg + 1)))
    return abs(sum(p[i] * t ** (deg - i) / sc ** (5 - i) for i in range(deg + 1)))


@dataclass(eq=False)
class Peak:
    """one quantity (velocity: deg 4, acceleration: deg 3) of one (agent, axis, segment)"""
    p: list          # derivative coefficients, descending powers, Fraction
    deg: int
    peak: Fr         # the largest |value| over the candidate times
    times: list      # the admissible t_max
    hull: Fr         # the hull bound of the kernel's shortcut (5 |D| / dt, 20 |D| / dt^2)

    @functools.lru_cache(maxsize=None)
    def _ladders(self, lim):
        """((factor, rungs, margin) per admissible t_max) for the double `lim`"""
        L = Fr(lim)
        out = []
        for t in self.times:
            sc, val, rungs, margin = 1.0, self.peak, 0, math.inf
            while True:
                margin = min(margin, float(abs(val - L) / L))
                if not (val > L and sc < 1e6):
                    break
                sc *= 1.1   # the exact doubles the kernel and the reference produce
                rungs += 1
                val = _poly(self.p, self.deg, t, Fr(sc))
            out.append((sc, rungs, margin))
        return tuple(out)

    def ladders(self, lim):
        lim = float(lim)
        if self.peak == 0:
            return ((1.0, 0, 1.0),)
        if self.peak <= Fr(lim):
            return ((1.0, 0, float((Fr(lim) - self.peak) / Fr(lim))),)
        return self._ladders(lim)

    def region(self, lim):
        """'still' | 'hull' (inside the kernel's shortcut) | 'between' (root path, factor 1) | 'below'"""
        if self.peak == 0:
            return "still"
        L = Fr(float(lim))
        if self.hull * (1 + Fr(MARGIN)) <= L:
            return "hull"
        return "between" if self.peak <= L else "below"


def segment_peaks(c6, dt, delta):
    """(velocity Peak, acceleration Peak) of one segment from its exact coefficients c6 (descending), dt and D = w1 - w0.  Candidate
    times are {0, dt} and the roots of the derivative in the smoothstep's closed form: dt / 2, resp. dt (3 -+ sqrt 3) / 6 (sqrt 3 to 40
    digits; the peaks are stationary, so the values are exact to ~1e-80)."""
    pv = [(5 - i) * c6[i] for i in range(5)]
    pa = [(5 - i) * (4 - i) * c6[i] for i in range(4)]
    out = []
    for p, deg, roots, hull in ((pv, 4, [dt / 2], 5 * abs(delta) / dt), (pa, 3, [dt * (3 - SQRT3) / 6, dt * (3 + SQRT3) / 6], 20 * abs(delta) / dt ** 2)):
        cand = [Fr(0), dt] + (roots if delta != 0 else [])
        vals = [_poly(p, deg, t) for t in cand]
        top = max(vals)
        times = [t for t, v in zip(cand, vals) if top > 0 and v >= top * (1 - Fr(TIE))]
        out.append(Peak(p, deg, top, times, hull))
    return out


def admissible(options_per_segment):
    """the mission's admissible set from the segments' option sets"""
    lo = max(min(o) for o in options_per_segment)
    hi = max(max(o) for o in options_per_segment)
    return sorted({v for o in options_per_segment for v in o if lo <= v <= hi})


class Reference:
    """everything about (init_traj, T) that does not depend on the limits, and time_scale for given limits"""

    def __init__(self, init_traj, T):
        self.init_traj, self.T = np.asarray(init_traj, np.float32), np.asarray(T, np.float64)
        self.N, self.M = self.init_traj.shape[0], self.init_traj.shape[1] - 1
        self.ctrl = dummy_ctrl(self.init_traj)
        self.c, self.S = exact_coef(self.ctrl, self.T)
        self.coef, self.S_f = to_float(self.c), to_float(self.S)
        self.vel, self.acc = {}, {}
        for q in range(self.N):
            for a in range(3):
                for m in range(self.M):
                    dt = Fr(float(self.T[m + 1] - self.T[m]))
                    v = self.ctrl[q, a, 6 * m:6 * m + 6]
                    assert v[0] == v[1] == v[2] and v[3] == v[4] == v[5], "not a dummy segment"
                    self.vel[q, a, m], self.acc[q, a, m] = segment_peaks(list(self.c[q, a, 6 * m:6 * m + 6]), dt, Fr(float(v[3])) - Fr(float(v[0])))

    def time_scale(self, max_vel, max_acc, coef_variants=(), rule1=True):
        """dict: sets {0: [...], 1: [...]} (admissible factors per rule), margin (smallest relative distance of a ladder comparison from
        its limit), vel0 / vel1 (the velocity-only factor per rule), acc (admissible set of the acceleration part alone),
        decider (the (quantity, agent, axis, segment) that alone reaches the top of rule 0's set, or None), rungs of the decider's ladders"""
        K = _kkt()
        margin, vel0, acc_opts, tops = math.inf, 1.0, [], []
        for key, pk in self.vel.items():
            (sc, rungs, mg), = pk.ladders(max_vel[key[0], key[1]])
            margin, vel0 = min(margin, mg), max(vel0, sc)
            tops.append((sc, sc, ("vel",) + key, (rungs,)))
        for key, pk in self.acc.items():
            lad = pk.ladders(max_acc[key[0], key[1]])
            margin = min(margin, min(l[2] for l in lad))
            acc_opts.append({l[0] for l in lad})
            tops.append((min(l[0] for l in lad), max(l[0] for l in lad), ("acc",) + key, tuple(l[1] for l in lad)))
        huge = np.full((self.N, 3), HUGE)
        sets = {0: admissible(acc_opts + [{vel0}])}
        v1 = set()
        if rule1:
            v1 = {K.time_scale_of(cf, self.T, np.asarray(max_vel, np.float64), huge, "eigen33") for cf in (self.coef,) + tuple(coef_variants)}
            sets[1] = admissible(acc_opts + [{min(v1)}]) if len(v1) == 1 else None   # (None: the restatement is not sure of Eigen's order here)
        tops.sort(key=lambda t: -t[1])
        decider = rungs = None
        if tops[0][1] > 1.0 and (len(tops) == 1 or tops[1][1] < tops[0][0]):
            decider, rungs = tops[0][2], tops[0][3]
        return dict(sets=sets, margin=margin, vel0=vel0, vel1=sorted(v1), acc=admissible(acc_opts), decider=decider, rungs=rungs)

    def regions(self, max_vel, max_acc):
        """list of ('vel' | 'acc', region, rungs) over all moving segments"""
        out = []
        for name, d, lim in (("vel", self.vel, max_vel), ("acc", self.acc, max_acc)):
            for key, pk in d.items():
                r = pk.region(lim[key[0], key[1]])
                if r != "still":
                    out.append((name, r, max(l[1] for l in pk.ladders(lim[key[0], key[1]]))))
        return out

    def coef_bound_ratio(self, coef, ts):
        """max over coefficients of |coef - c_k ts^-(5-k)| / (U S_k ts^-(5-k)), exactly (coef: doubles; ts: the factor that was applied)"""
        worst, s = Fr(0), Fr(float(ts))
        flat_c, flat_S, flat = self.c.reshape(-1), self.S.reshape(-1), np.asarray(coef, np.float64).reshape(-1)
        for i in range(flat.size):
            sk = s ** (5 - i % 6)
            if flat_S[i] == 0:
                assert flat[i] == 0.0
                continue
            worst = max(worst, abs(Fr(float(flat[i])) * sk - flat_c[i]) / (Fr(U) * flat_S[i]))
        return float(worst)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class TrajCase:
    name: str
    N: int
    M: int
    idx: int
    init_traj: np.ndarray   # [N][M + 1][3] float32
    T: np.ndarray           # [M + 1]
    max_vel: np.ndarray     # [N][3]
    max_acc: np.ndarray     # [N][3]
    world: World
    ref: Reference
    ts: dict                # Reference.time_scale at the case's limits
    seed: tuple

    def mission(self, max_vel=None, max_acc=None):
        z = np.zeros((self.N, 9))
        return Mission(z, z.copy(), np.full(self.N, 0.15), self.max_vel.copy() if max_vel is None else max_vel,
                       self.max_acc.copy() if max_acc is None else max_acc)

    def plan(self):
        return PlanResult(self.init_traj.copy(), self.T.copy())


def make_param(N, rule=0, **kw):
    """the session's world box: x in [0, 51] (the far case lives at x = 48 .. 51), one lane of y per agent; plan/sequential = true with
    batch_iter = 0: no QP"""
    d = dict(world_x_min=0.0, world_y_min=0.0, world_z_min=Z_KEY * RES, world_x_max=51.0, world_y_max=LANE * N, world_z_max=(Z_KEY + Z_DIM - 1) * RES,
             box_xy_res=RES, box_z_res=RES, sequential=True, batch_size=4, batch_iter=0, iteration=1, time_scale=True, timescale_rule=rule)
    d.update(kw)
    return Param(**d)


def make_world(N, x0, blocked_at=None):
    """an empty grid over x in [x0, x0 + 3], every lane, the whole height; blocked_at: a point whose cell (and neighbours) is an obstacle"""
    key_min = (int(round(x0 / RES)), 0, Z_KEY)
    dim = (int(X_SPAN / RES) + 1, int(LANE * N / RES) + 1, Z_DIM)
    dist = np.ones(dim, np.float32)
    if blocked_at is not None:
        k = np.floor(np.asarray(blocked_at, np.float64) / RES).astype(int) - np.array(key_min)
        lo, hi = np.maximum(k - 1, 0), np.minimum(k + 2, dim)
        dist[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 0.0
    return World(dist, key_min, RES)


def _make_T(rng, kind, M):
    if kind.startswith("u"):
        return np.arange(M + 1, dtype=np.float64) * float(kind[1:])
    dts = rng.uniform(0.3, 2.5, M)
    if kind == "ratio8":   # neighbouring segments in ratio 1 : 8
        j = int(rng.integers(0, M - 1))
        dts[j], dts[j + 1] = 0.3, 2.4
    return np.concatenate([[0.0], np.cumsum(dts)])


def _vel_rungs(r):
    """rungs of the velocity ladder when peak / limit = r (floats; the generator's aim, the exact reference judges)"""
    f = lambda s: 30 * (0.5 / s) ** 2 * (1 - 0.5 / s) ** 2 / s
    sc, n = 1.0, 0
    while f(sc) * r > f(1.0) and n < 60:
        sc *= 1.1
        n += 1
    return n


def _acc_rungs(r):
    """(n1, n2): rungs through the first / second acceleration peak when peak / limit = r"""
    a = lambda x: abs(60 * x * (1 - x) * (1 - 2 * x))
    out = []
    for tau in ((3 - math.sqrt(3)) / 6, (3 + math.sqrt(3)) / 6):
        sc, n = 1.0, 0
        while a(tau / sc) / sc ** 2 * r > a(tau) and n < 60:
            sc *= 1.1
            n += 1
        out.append(n)
    return tuple(out)


def _draw_ratio(rng, what, kind):
    for _ in range(100000):
        r = float(np.exp(rng.uniform(math.log(1.01), math.log(6.0))))
        if what == "vel":
            n = _vel_rungs(r)
            ok = (n == kind) if kind < 8 else n >= 8
            ok = ok and _vel_rungs(r * 1.002) == n and _vel_rungs(r / 1.002) == n
        else:
            n1, n2 = _acc_rungs(r)
            ok = {"both2": n1 == n2 == 2, "both1": n1 == n2 == 1, "same": n1 == n2 >= 1 and r < 1.45, "split2": n1 != n2 and 1.9 < r < 2.1,
                  "split": n1 != n2, "deep": max(n1, n2) >= 8}[kind]
            ok = ok and _acc_rungs(r * 1.002) == (n1, n2) == _acc_rungs(r / 1.002)
        if ok:
            return r
    raise RuntimeError(f"no ratio for {what} {kind}")


def _build(N, idx, attempt):
    rng = np.random.default_rng([N, idx, attempt])
    M, x0 = M_OF[N][idx], (48.0 if idx == FAR_CASE else 0.0)
    T = _make_T(rng, T_KIND[idx], M)
    dts = np.diff(T)
    what, kind = DECIDER[idx]
    dq, da, dm = (2 * idx + 1) % N, (idx + N) % 3, int(rng.integers(0, M))   # the deciding (agent, axis, segment): moves from case to case
    ratio = _draw_ratio(rng, what, kind) if what != "none" else None
    lo = np.array([x0 + 0.3, 0.3, 0.6])
    hi = np.array([x0 + X_SPAN - 0.3, LANE - 0.3, (Z_KEY + Z_DIM - 1) * RES - 0.35])
    traj = np.zeros((N, M + 1, 3), np.float64)
    for q in range(N):
        l, h = lo + (0, LANE * q, 0), hi + (0, LANE * q, 0)
        pos = rng.uniform(l + 0.2, h - 0.2)
        traj[q, 0] = pos
        dstar = rng.uniform(0.9, 1.4)
        for m in range(M):
            u = rng.random()
            d = np.zeros(3)
            if u < 0.5:     # lattice-like: one axis at a time, the others hover
                d[int(rng.integers(0, 3))] = 0.1 * int(rng.integers(1, 16))
            elif u < 0.8:   # diagonal
                ax = rng.permutation(3)[:int(rng.integers(2, 4))]
                d[ax] = rng.uniform(0.1, 1.0, len(ax))
            # (else: hover, D = 0 on every axis)
            if what != "none" and q == dq:   # the deciding segment holds the axis's largest peak by a clear factor
                p = 1 if what == "vel" else 2
                if m == dm:
                    d[da] = dstar
                else:
                    cap = dstar * (dts[m] / dts[dm]) ** p / (ratio * 1.3)
                    if d[da] > cap:
                        d[da] = cap * rng.uniform(0.3, 0.9)
            for a in range(3):
                s = 1.0 if rng.random() < 0.5 else -1.0
                if not (l[a] <= pos[a] + s * d[a] <= h[a]):
                    s = -s
                if not (l[a] <= pos[a] + s * d[a] <= h[a]):   # neither side has room for the whole move: toward the roomier side
                    s = 1.0 if h[a] - pos[a] > pos[a] - l[a] else -1.0
                    d[a] = min(d[a], (h[a] - pos[a]) if s > 0 else (pos[a] - l[a]))
                pos[a] += s * d[a]
            traj[q, m + 1] = pos
    traj = traj.astype(np.float32)
    ref = Reference(traj, T)
    # limits per (agent, axis), relative to the axis's own peaks
    max_vel, max_acc = np.zeros((N, 3)), np.zeros((N, 3))
    for q in range(N):
        for a in range(3):
            for name, d, lim, span in (("vel", ref.vel, max_vel, 2.4), ("acc", ref.acc, max_acc, 3.1)):
                peak = max(float(d[q, a, m].peak) for m in range(M))
                hull = max(float(d[q, a, m].hull) for m in range(M))
                if peak == 0:
                    lim[q, a] = rng.uniform(0.5, 2.0)
                    continue
                region = kind if what == "none" else ("hull" if rng.random() < 0.5 else "between")
                lim[q, a] = hull * rng.uniform(1.05, 3.0) if region == "hull" else peak * rng.uniform(1.1, span)
                if name == what and (q, a) == (dq, da):
                    lim[q, a] = float(d[q, a, dm].peak) / ratio
    return TrajCase(f"n{N}_{idx}", N, M, idx, traj, T, max_vel, max_acc, make_world(N, x0), ref, None, (N, idx, attempt))


def oracle_coef(c):
    from tests import oracle_lib as O
    return O.ctrl_to_coef(c.T, c.ref.ctrl)


def oracle_rule1_velocity(c, coef, max_vel):
    """the C oracle's factor under rule 1 with the acceleration limits out of the way"""
    from tests import oracle_lib as O
    pl = c.plan()
    pl.coef[...] = coef
    return O.time_scale(c.mission(np.asarray(max_vel, np.float64).copy(), np.full((c.N, 3), HUGE)), pl, 1)


def swaps_change_the_factor(c):
    """exchanging the deciding limit with any other entry of its array changes the expected sets (None: no decider)"""
    if c.ts["decider"] is None:
        return None
    what, q, a, _ = c.ts["decider"]
    for q2 in range(c.N):
        for a2 in range(3):
            if (q2, a2) == (q, a):
                continue
            mv, ma = c.max_vel.copy(), c.max_acc.copy()
            lim = mv if what == "vel" else ma
            lim[q, a], lim[q2, a2] = lim[q2, a2], lim[q, a]
            if c.ref.time_scale(mv, ma, rule1=False)["sets"][0] == c.ts["sets"][0]:
                return False
    return True


def _accept(c):
    """conditions (a), (d) and the case's own promise (DECIDER)"""
    oc = oracle_coef(c)
    c.ts = ts = c.ref.time_scale(c.max_vel, c.max_acc, (oc,))
    if ts["margin"] < MARGIN or ts["sets"][1] is None:
        return False
    if oracle_rule1_velocity(c, oc, c.max_vel) != ts["vel1"][0]:
        return False
    if len(set(c.max_vel.reshape(-1)) | set(c.max_acc.reshape(-1))) != 6 * c.N:
        return False
    what, kind = DECIDER[c.idx]
    if what == "none":
        seen = {r[1] for r in c.ref.regions(c.max_vel, c.max_acc)}
        return ts["sets"] == {0: [1.0], 1: [1.0]} and (seen == {"hull"} if kind == "hull" else "between" in seen and "below" not in seen)
    if ts["decider"] is None or ts["decider"][0] != what or ts["decider"][1:3] != ((2 * c.idx + 1) % c.N, (c.idx + c.N) % 3):
        return False
    if what == "vel":
        ok = ts["rungs"][0] == kind if kind < 8 else ts["rungs"][0] >= 8
    else:
        n1, n2 = ts["rungs"]
        ok = {"both2": n1 == n2 == 2, "both1": n1 == n2 == 1, "same": n1 == n2, "split2": n1 != n2, "split": n1 != n2, "deep": max(n1, n2) >= 8}[kind]
    return ok and swaps_change_the_factor(c) is True


@functools.lru_cache(maxsize=None)
def case(N, idx):
    """case idx of the N-agent session (built once per process, never written to): the first seed that meets the conditions"""
    first = FIRST_SEED.get((N, idx), 0)
    for attempt in range(first, first + 64):
        c = _build(N, idx, attempt)
        if _accept(c):
            return c
    raise RuntimeError(f"no seed for case n{N}_{idx}")


def cases(N):
    return [case(N, idx) for idx in range(K_CASES)]


@functools.lru_cache(maxsize=None)
def corridor(N, idx):
    """the oracle's corridor of a case at its uploaded T (never written to): (rc, plan)"""
    from tests import oracle_lib as O
    c = case(N, idx)
    pl = c.plan()
    rc, _ = O.corridor_update(c.world, c.mission(), make_param(N), pl)
    return rc, pl


def blocked(c):
    """the case with an obstacle on agent 0's first waypoint: its corridor stage fails (rbp_corridor.hpp:181-187)"""
    x0 = c.world.key_min[0] * RES
    return dataclasses.replace(c, name=c.name + "_blocked", world=make_world(c.N, x0, blocked_at=c.init_traj[0, 0]))


def check_plan(c, pl, rule, tag, time_scale_on=True):
    """a downloaded plan of case c (the product's, or the oracle's) against the exact reference; returns the worst coefficient error in
    units of U * S_k.

    The coefficient bound, counted from coef_kernel's operations for the t^5 coefficient (the longest chain), in units of U = 2^-53
    relative to S_k:  inv = 1 / dt, one rounding, raised to the 5th power: 5;  pow's own error, at most one ulp = 2 U: 2;  the product
    basis * tp: 1;  the product with the control point (0 where the multiply-add is fused): 1;  five additions of partial sums, each
    bounded by S_k: 5.  That is 14; B_UNSCALED = 16 leaves 2 for what the first-order count neglects.  The rescale
    pow(1 / ts, 5 - k) * coef adds 5 (the reciprocal's rounding through the 5th power) + 2 (pow) + 1 (product) = 8: B_SCALED = 22 = 14 + 8.
    The oracle's arithmetic is the same chain without fusion."""
    assert np.array_equal(np.ascontiguousarray(pl.ctrl).view(np.uint64), c.ref.ctrl.view(np.uint64)), tag
    if time_scale_on:
        assert pl.time_scale in c.ts["sets"][rule], (tag, pl.time_scale, c.ts["sets"][rule])
        assert pl.time_scale_alt in c.ts["sets"][1 - rule], (tag, pl.time_scale_alt, c.ts["sets"][1 - rule])
    else:
        assert pl.time_scale == 1.0 and pl.time_scale_alt == 1.0, tag
    ts = pl.time_scale
    rc, cor = corridor(c.N, c.idx)
    assert rc == 0, tag
    assert np.array_equal(pl.T, c.T * ts), tag   # one IEEE product each
    assert np.array_equal(pl.sfc_count, cor.sfc_count) and np.array_equal(pl.sfc_box, cor.sfc_box), tag
    want = cor.sfc_time.copy()
    for q in range(c.N):
        want[q, :cor.sfc_count[q]] *= ts
    assert np.array_equal(pl.sfc_time, want), tag
    assert np.array_equal(pl.rsfc_time, cor.rsfc_time * ts) and np.array_equal(cor.rsfc_time, c.T[1:]), tag
    ratio = c.ref.coef_bound_ratio(pl.coef, ts)
    assert ratio <= (B_UNSCALED if ts == 1.0 else B_SCALED), (tag, ratio, ts)
    return ratio
