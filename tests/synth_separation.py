"""An exact restatement of the separation rule (csrc/common/separation_rules.h) in fractions.Fraction, beside tests/synth_report.py, whose
synthetic plans it reuses; shared by tests/test_separation_host.py (CPU) and tests/test_gpu_separation.py.

`ExactItem` is the polynomial the double inputs of one item (a pair and a segment) define, with nothing rounded: the exact differences of
the coefficients, the exact quotient by the downwash, the exact h = Ts[m+1] - Ts[m] of the two scaled doubles.  From it come, per piece
[p / 2^D, (p+1) / 2^D] of the segment, the eleven exact Bernstein coefficients of the squared relative distance (exact Bernstein form, exact
de Casteljau halvings along the bits of p, exact product formula), the exact values at rational times, and S.

The error term is COUNTED here, from the operations as the rule writes them (u = 2^-53; a chain of n roundings is off by a factor within
(1 + u)^n, and every exact control point is at most A = sum |alpha_i| h^i in size, every exact q_k at most S = Ax^2 + Ay^2 + Az^2):

  alpha_i      c_qj - c_qi, and for z the quotient by the downwash                                    2 roundings
  h            Ts[m+1] - Ts[m]                                                                        1
  hp_i         h^i by i - 1 products of the computed h                                                i + (i - 1)
  g_i          alpha_i * hp_i                                                                         2 + (2 i - 1) + 1
  beta_k       g_0 + w(k,1) g_1 + ... from the left, w a rounded quotient: term i passes the weight,
               its product and k - i + 1 sums                                                         (2 i + 2) + 2 + (k - i + 1), i >= 1
  halving      (a + b) * 0.5, five rounds per level, the product exact                                5 per level
  product      b_a * b_c of two points                                                                2 x point + 1
  q_k          (xx + yy) + zz, W * (.), at most five sums of terms                                    2 + 2 + 5
  and 8 units for S as computed (37 roundings at most, relative) and the second-order terms.
`counted_constant(D)` walks that table; it arrives at 48 + 10 D without reading the header.

`host_separations(plans, depth, refine_below)` gives what rbp_separation_host says of each mission of a synth_report.Plans (times scaled
by the IEEE product, as rbp_session_download hands them out) -- the reference of the GPU tests.
"""
from fractions import Fraction as F
from math import comb

import numpy as np

from swarm_simulator_amd import host
from swarm_simulator_amd.types import Mission, Param, PlanResult

U = F(1, 2 ** 53)
ULPS = 3   # RBP_SEPARATION_ULPS


def counted_constant(depth):
    alpha, h = 2, 1
    hp = lambda i: i * h + (i - 1)
    g = lambda i: alpha + hp(i) + 1 if i else alpha
    beta = max([g(0) + k for k in range(6)] + [g(i) + 2 + (k - i + 1) for k in range(6) for i in range(1, k + 1)])
    point = beta + 5 * depth
    return (2 * point + 1) + 2 + 2 + 5 + 8


def ratio_slack():
    """what the square of a ratio may be off by, relative: the root and the quotient round once each (u each) and the ratio is moved by
    ULPS doubles (at most 2 u each): (1 + 8 u)^2 - 1 < 17 u"""
    return 17 * U


class ExactItem:
    def __init__(self, T, ci, cj, m, downwash):
        """T scaled [M + 1]; ci, cj [3][6 M] of the two agents (descending powers per segment)"""
        self.h = F(float(T[m + 1])) - F(float(T[m]))
        dw = F(float(downwash))
        self.alpha = []
        for k in range(3):
            a = [F(float(cj[k][6 * m + 5 - i])) - F(float(ci[k][6 * m + 5 - i])) for i in range(6)]
            self.alpha.append([x / dw for x in a] if k == 2 else a)
        self.S = sum(sum(abs(a[i] * self.h ** i) for i in range(6)) ** 2 for a in self.alpha)
        self.b = [[sum(F(comb(k, i), comb(5, i)) * a[i] * self.h ** i for i in range(k + 1)) for k in range(6)] for a in self.alpha]

    def err(self, depth):
        return counted_constant(depth) * U * self.S

    def value(self, t):
        """|r(t)|^2 at the rational time t in [0, h]"""
        return sum(sum(a[i] * t ** i for i in range(6)) ** 2 for a in self.alpha)

    @staticmethod
    def _halve(b, right):
        left, b = [b[0]], list(b)
        for r in range(1, 6):
            b = [(b[i] + b[i + 1]) / 2 for i in range(6 - r)] + b[6 - r:]
            left.append(b[0])
        return b if right else left

    def piece(self, depth, p):
        """the eleven exact Bernstein coefficients of |r|^2 on piece p of depth `depth`"""
        b = self.b
        for l in range(depth):
            right = (p >> (depth - 1 - l)) & 1
            b = [self._halve(x, right) for x in b]
        return [sum(F(comb(5, a) * comb(5, k - a), comb(10, k)) * sum(x[a] * x[k - a] for x in b) for a in range(max(0, k - 5), min(5, k) + 1))
                for k in range(11)]


def sub_plan(T, coef, radius, qi, qj, m):
    """the item (qi, qj, m) of a mission as a plan of its own: two agents, one segment, the segment's own two scaled times"""
    M = len(T) - 1
    c = np.asarray(coef, np.float64).reshape(-1, 3, M, 6)
    pr = PlanResult(np.zeros((2, 2, 3), np.float32), np.array([float(T[m]), float(T[m + 1])]))
    pr.coef[:] = np.stack([c[qi, :, m, :], c[qj, :, m, :]]).reshape(2, 3, 6)
    r = np.array([float(radius[qi]), float(radius[qj])])
    return Mission(np.zeros((2, 9)), np.zeros((2, 9)), r, np.ones((2, 3)), np.ones((2, 3))), pr


def crossing():
    """the case a sampled ratio misses: agent 0 rests at the origin, agent 1 passes it at 8 m/s, 0.1 m to the side, and is 0.4 m before
    and behind it at the samples t = 0.4 and 0.5 of dt = 0.1; radii 0.15.  (mission, plan): one segment of one second"""
    c = np.zeros((2, 3, 6))
    c[1, 0, 4], c[1, 0, 5], c[1, 1, 5] = 8.0, -3.6, 0.1
    pr = PlanResult(np.zeros((2, 2, 3), np.float32), np.array([0.0, 1.0]))
    pr.coef[:] = c
    return Mission(np.zeros((2, 9)), np.zeros((2, 9)), np.full(2, 0.15), np.ones((2, 3)), np.ones((2, 3))), pr


def host_separations(plans, depth, refine_below, fill=-7.0):
    """rbp_separation_host of every mission of `plans`: (records, pair_lower [K][N (N-1) / 2] pre-filled with `fill`)"""
    import ctypes as C
    from swarm_simulator_amd import _abi as A
    from swarm_simulator_amd.types import Separation
    p = Param.test_sweep(downwash=plans.downwash).c_struct()
    recs, pairs = [], np.full((plans.K, plans.N * (plans.N - 1) // 2), fill)
    for k in range(plans.K):
        mission, pl = plans.mission(k), plans.plan(k)   # (kept alive: the structs point into their arrays)
        ms = mission.c_struct()
        out = A.rbp_separation()
        rc = host.lib().rbp_separation_host(C.byref(ms), C.byref(p), pl.M, A.ptr(pl.T, A.c_double_p), A.ptr(pl.coef, A.c_double_p), depth, refine_below,
                                            C.byref(out), A.ptr(pairs[k], A.c_double_p) if pairs.shape[1] else None)
        assert rc == 0, rc
        recs.append(Separation.from_c(out))
    return recs, pairs
