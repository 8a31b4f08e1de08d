"""The exact restatement of the state rule (csrc/common/state_rules.h), beside tests/synth_report.py, whose synthetic plans and whose exact
positions and pair ratios it reuses; shared by tests/test_state_rules.py, tests/test_dynamics_host.py (CPU) and tests/test_gpu_dynamics.py.

`Exact` restates velocity, acceleration, the limit ratios and the ratio curves of ONE mission in fractions.Fraction, with the rule's own
DISCRETE decisions -- the number of samples, the double t = j * dt of a sample, its segment -- made in doubles as the rule makes them
(synth_report.Exact), and everything continuous exact.  With it come error bounds COUNTED from the operations (u = 2^-53,
gamma_k = k u / (1 - k u)):

  velocity      v^ = Horner over d_i = fl(k_i c_i), k = 5 4 3 2 1, at fl(t - Ts[m]).  The subtraction perturbs tseg by a factor (1 + d),
                which moves the exact derivative polynomial by at most gamma_4 V with V = sum_i k_i |c_i| |tseg|^(4-i) (the highest power
                is 4).  A term passes through its coefficient product (one rounding; exact for k = 1, 2, 4, counted all the same) and at
                most four multiply-adds (eight roundings): gamma_9 on the perturbed argument.
                |v^ - v| <= e_v = (gamma_4 + gamma_9 (1 + gamma_4)) V.
  acceleration  the same with k = 20 12 6 2, highest power 3, three multiply-adds: e_a = (gamma_3 + gamma_7 (1 + gamma_3)) A,
                A = sum_i k_i |c_i| |tseg|^(3-i).
  limit ratio   fl(|x^| / limit): one division.  |r^ - r| <= (e_x (1 + u) + u |x|) / |limit|.
  curves        the smallest / largest of the pairs' computed ratios lies within the largest bound of a pair that can attain it of the
                exact smallest / largest (synth_report.Exact.ratios carries every pair's exact ratio and bound).
Positions are not bounded again here: rows 0..2 are required to be the report's bits.

`host_dynamics(plans, dt, ...)` gives what rbp_dynamics_host says of each mission of a synth_report.Plans with the limits `max_vel` /
`max_acc` [K][N][3] -- the reference of the GPU tests.
"""
from fractions import Fraction as F

import numpy as np

from swarm_simulator_amd import host
from swarm_simulator_amd.types import Mission, Param
from tests import synth_report as S

U, gamma = S.U, S.gamma
E_VEL = gamma(4) + gamma(9) * (1 + gamma(4))
E_ACC = gamma(3) + gamma(7) * (1 + gamma(3))
K_VEL = (5, 4, 3, 2, 1)
K_ACC = (20, 12, 6, 2)


class Exact:
    """of ONE mission (T scaled): vel / acc [sample][agent * 3 + axis] as (exact value, bound); curve bounds through synth_report.Exact"""

    def __init__(self, T, coef, radius, downwash, dt, pairs=True):
        T = [float(x) for x in T]
        M, N = len(T) - 1, coef.shape[0]
        self.samples = ns = int(np.floor(T[M] / dt))
        self.N = N
        c = coef.reshape(N, 3, M, 6)
        self.vel, self.acc = [], []
        for j in range(ns):
            t = float(j) * dt
            before = 0
            while before < M and T[before] < t:
                before += 1
            m = max(before - 1, 0)
            tseg = F(t) - F(T[m]) if before > 0 else F(t)
            vrow, arow = [], []
            for a in range(N):
                for k in range(3):
                    cc = [F(float(x)) for x in c[a, k, m]]
                    v = sum(kk * ci * tseg ** (4 - i) for i, (kk, ci) in enumerate(zip(K_VEL, cc)))
                    V = sum(kk * abs(ci) * abs(tseg) ** (4 - i) for i, (kk, ci) in enumerate(zip(K_VEL, cc)))
                    ac = sum(kk * ci * tseg ** (3 - i) for i, (kk, ci) in enumerate(zip(K_ACC, cc)))
                    Ab = sum(kk * abs(ci) * abs(tseg) ** (3 - i) for i, (kk, ci) in enumerate(zip(K_ACC, cc)))
                    vrow.append((v, E_VEL * V)), arow.append((ac, E_ACC * Ab))
            self.vel.append(vrow), self.acc.append(arow)
        self.report = S.Exact(T, coef, radius, downwash, dt) if pairs else None

    def limit_ratios(self, which, limits):
        """{(sample, agent, axis): (exact ratio, bound)} of velocity ("vel") or acceleration ("acc") under limits [N][3]"""
        rows, out = getattr(self, which), {}
        for j, row in enumerate(rows):
            for i, (x, e) in enumerate(row):
                lim = abs(F(float(limits[i // 3, i % 3])))
                out[(j, i // 3, i % 3)] = (abs(x) / lim, (e * (1 + U) + U * abs(x)) / lim)
        return out

    def curve(self, j):
        """((exact min, bound), (exact max, bound)) of sample j over the pairs; None without a pair"""
        rs = [v for (jj, _, _), v in self.report.ratios.items() if jj == j]
        if not rs:
            return None
        bound = max(b for _, b in rs)   # (the computed extremum is some pair's computed ratio: the largest bound covers whichever)
        return (min(r for r, _ in rs), bound), (max(r for r, _ in rs), bound)


def peak_of(ratios):
    """(key, ratio, bound) of the exact peak under the rule's order: largest ratio, then the smallest (sample, agent, axis); None: none > 0"""
    best = None
    for key in sorted(ratios):
        r, b = ratios[key]
        if r > 0 and (best is None or r > best[1]):
            best = (key, r, b)
    return best


def peak_is_certain(ratios):
    key, r, b = peak_of(ratios)
    return all(r2 + b2 < r - b for k2, (r2, b2) in ratios.items() if k2 != key)


def limits(seed, K, N, low=0.3, high=1.5):
    """seeded max_vel, max_acc [K][N][3]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(low, high, (K, N, 3)), rng.uniform(low, high, (K, N, 3))


def mission_of(plans, k, max_vel, max_acc):
    N = plans.N
    return Mission(np.zeros((N, 9)), np.zeros((N, 9)), plans.radius[k].copy(), np.ascontiguousarray(max_vel[k]), np.ascontiguousarray(max_acc[k]))


def host_dynamics(plans, dt, max_vel, max_acc, states=None, curves=None):
    """rbp_dynamics_host of every mission of `plans` (times scaled by the IEEE product, as rbp_session_download hands them out); states
    [K][N][9][S] / curves [K][S][2] are written in place where given"""
    p = Param.test_sweep(downwash=plans.downwash)
    return [host.dynamics(mission_of(plans, k, max_vel, max_acc), p, plans.plan(k), dt, None if states is None else states[k], None if curves is None else curves[k])
            for k in range(plans.K)]
