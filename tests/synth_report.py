"""Synthetic plans for the report rule (csrc/common/report_rules.h) and its exact restatement, shared by tests/test_report_host.py (CPU)
and tests/test_gpu_report.py.

A `Plans` object holds K missions of N agents in the layout rbp_dev_report takes: M [K], T [K][S + 1] (unscaled), coef [K] slots of
N * 3 * 6 * S doubles with mission k's own [N][3][6 M[k]] packed at the front, radius [K][N], time_scale [K] or None.  `host_reports`
gives what rbp_report_host says of each mission -- of the times scaled by the IEEE product T * ts, which is what rbp_session_download
hands out.  Coefficients are seeded: agents start on a jittered grid about 1 m apart and move along random quintics.

`exact` restates the rule in fractions.Fraction (square roots in decimal, 60 digits), with the rule's own DISCRETE decisions -- the
number of samples, the double t = j * dt of a sample, its segment -- made in doubles as the rule makes them, and everything continuous
exact: tseg = t - Ts[m], the polynomial, differences, norms, quotients.  With it come error bounds COUNTED from the operations
(u = 2^-53, gamma_k = k u / (1 - k u), Higham's notation), per position, per ratio and for the distance:

  position   p^ = Horner(c, fl(t - Ts[m])).  The subtraction perturbs tseg by a factor (1 + d), |d| <= u, which moves the exact
             polynomial by at most sum_i (5 - i) |c_i| |tseg|^(5-i) ((1 + u)^5 - 1) / 5 <= gamma_5 S with S = sum_i |c_i| |tseg|^(5-i);
             Horner's five multiply-adds then err by at most gamma_10 S' on the perturbed argument, S' <= (1 + u)^5 S.
             |p^ - p| <= e_p = (gamma_5 + gamma_10 (1 + gamma_5)) S.
  difference fl(a^ - b^) = (a^ - b^)(1 + d): |.. - (a - b)| <= (e_a + e_b)(1 + u) + u |a - b|; the z difference is then divided by
             the downwash, one more factor (1 + d): e_z = ((e_a + e_b)(1 + u) + u |dz|) (1 + u) / downwash + u |dz| / downwash.
  norm       three squares (1 + d each), two sums, one square root: n^ = ||d^|| (1 + theta), |theta| <= gamma_3 (the root halves the
             relative error of its argument, gamma_3 / 2, and adds u); ||d^|| differs from ||d|| by at most ||e||_2.
  ratio      divided by fl(r_i + r_j), itself (r_i + r_j)(1 + d): two more factors.  |r^ - r| <= (||e||_2 (1 + gamma_5) + gamma_5 ||d||) / (r_i + r_j).
  distance   a step is a norm without the downwash: |s^ - s| <= ||e||_2 (1 + gamma_3) + gamma_3 ||d|| = e_s.  An agent's ns - 1 steps are
             summed one after the other, then the N sums: every step passes through at most (ns - 2) + (N - 1) + 1 additions (the first
             of them to 0.0, exact), so |D^ - D| <= sum e_s (1 + gamma_n) + gamma_n sum s with n = ns + N - 2.
rbp_validate differs: each power comes from pow (glibc: below 1 ulp = 2 u, times the product's u: gamma_3 per term) and the six terms are
summed from 0.0 (gamma_5 on top): e_p = (gamma_5 + gamma_8 (1 + gamma_5)) S; and ONE running sum over all N (ns - 1) steps: n = N (ns - 1).
"""
import decimal
from fractions import Fraction as F

import numpy as np

from swarm_simulator_amd import _abi as A
from swarm_simulator_amd import host
from swarm_simulator_amd.types import Mission, Param, PlanResult

U = F(1, 2 ** 53)
CTX = decimal.Context(prec=60)


def gamma(k):
    return k * U / (1 - k * U)


def tile_of(N):
    """samples per tile of report_pair_kernel (kernels/report.hip report_tile): what 32 KB hold at 24 bytes per agent, at most 64"""
    return min(64, 32768 // (24 * N))


BLOCKS = 16   # REPORT_BLOCKS of kernels/report.hip: workgroups per mission


class Plans:
    def __init__(self, M, T, coefs, radius, time_scale=None, downwash=2.0):
        self.M = np.asarray(M, np.int32)
        self.K, self.S = len(self.M), int(T.shape[1]) - 1
        self.T, self.radius, self.downwash = A.as_f64(T), A.as_f64(radius), float(downwash)
        self.N = self.radius.shape[1]
        self.coefs = [A.as_f64(c) for c in coefs]   # per mission [N][3][6 M[k]]
        self.time_scale = None if time_scale is None else A.as_f64(time_scale)
        self.coef = np.zeros((self.K, self.N * 3 * 6 * self.S))
        for k, c in enumerate(self.coefs):
            assert c.shape == (self.N, 3, 6 * self.M[k])
            self.coef[k, :c.size] = c.reshape(-1)

    def scaled_T(self, k):
        T = self.T[k, :self.M[k] + 1].copy()
        ts = 1.0 if self.time_scale is None else float(self.time_scale[k])
        return T * ts if ts != 1.0 else T   # (numpy's product of two doubles is the IEEE product rbp_session_download forms)

    def mission(self, k):
        N = self.N
        return Mission(np.zeros((N, 9)), np.zeros((N, 9)), self.radius[k].copy(), np.ones((N, 3)), np.ones((N, 3)))

    def plan(self, k):
        pr = PlanResult(np.zeros((self.N, self.M[k] + 1, 3), np.float32), self.scaled_T(k))
        pr.coef[:] = self.coefs[k]
        return pr

    def host_reports(self, dt):
        p = Param.test_sweep(downwash=self.downwash)
        return [host.report(self.mission(k), p, self.plan(k), dt) for k in range(self.K)]


def times(kind, M):
    """T [M + 1]: unit segments; 0.5 / 1.7 alternating; or 1 / 0.5 alternating"""
    seg = {"unit": [1.0], "nonunit": [0.5, 1.7], "alternating": [1.0, 0.5]}[kind]
    return np.concatenate([[0.0], np.cumsum([seg[m % len(seg)] for m in range(M)])])


def random_coefs(rng, N, M, spread=1.0):
    """[N][3][6 M] descending powers: agent a rests near grid point a (about `spread` apart in x / y, z in 0.5 .. 2) plus a random quintic
    of a few decimetres per segment"""
    side = int(np.ceil(np.sqrt(N)))
    c = rng.uniform(-0.05, 0.05, (N, 3, M, 6))
    base = np.stack([(np.arange(N) % side) * spread, (np.arange(N) // side) * spread, rng.uniform(0.5, 2.0, N)], 1)
    c[..., 5] = base[:, :, None] + rng.uniform(-0.2, 0.2, (N, 3, M))
    return np.ascontiguousarray(c.reshape(N, 3, 6 * M))


def make(seed, N, Ms, kinds="unit", time_scale=None, radius=0.15, spread=1.0, stride=None):
    """K = len(Ms) missions under one stride (default: the largest M)"""
    rng = np.random.default_rng(seed)
    K, S = len(Ms), stride or max(Ms)
    kinds = [kinds] * K if isinstance(kinds, str) else kinds
    T = np.zeros((K, S + 1))
    for k, M in enumerate(Ms):
        T[k, :M + 1] = times(kinds[k], M)
    rad = np.full((K, N), radius) + rng.uniform(0.0, 0.02, (K, N))
    return Plans(Ms, T, [random_coefs(rng, N, M, spread) for M in Ms], rad, time_scale)


# ---- the exact restatement --------------------------------------------------------------------------------------------------------
def _sqrt(fr):
    return CTX.sqrt(CTX.divide(decimal.Decimal(fr.numerator), decimal.Decimal(fr.denominator)))


def _dec(fr):
    return CTX.divide(decimal.Decimal(fr.numerator), decimal.Decimal(fr.denominator))


def _to_f(d):
    return F(d)   # a Decimal is a rational


class Exact:
    """of ONE mission (T scaled, as rbp_report_host takes it): positions, every ratio with its bound, the distance with its bound"""

    def __init__(self, T, coef, radius, downwash, dt, pow_terms=False):
        T = [float(x) for x in T]
        M, N = len(T) - 1, coef.shape[0]
        self.samples = ns = int(np.floor(T[M] / dt))
        c = coef.reshape(N, 3, M, 6)
        g_eval = gamma(8) if pow_terms else gamma(10)
        pos, err = [], []
        for j in range(ns):
            t = float(j) * dt                       # the rule's double
            before = 0
            while before < M and T[before] < t:     # the rule's comparison of doubles
                before += 1
            m = max(before - 1, 0)
            tseg = F(t) - F(T[m]) if before > 0 else F(t)
            pw = [tseg ** (5 - i) for i in range(6)]
            row, erow = [], []
            for a in range(N):
                for k in range(3):
                    cc = [F(float(x)) for x in c[a, k, m]]
                    row.append(sum(ci * p for ci, p in zip(cc, pw)))
                    S = sum(abs(ci) * abs(p) for ci, p in zip(cc, pw))
                    erow.append((gamma(5) + g_eval * (1 + gamma(5))) * S)
            pos.append(row), err.append(erow)
        self.pos, self.err, self.N = pos, err, N
        dw, rad = F(float(downwash)), [F(float(r)) for r in radius]
        self.ratios = {}    # (j, qi, qj) -> (exact ratio as Fraction of a 60-digit decimal, bound)
        for j in range(ns):
            for qi in range(N):
                for qj in range(qi + 1, N):
                    d, e = [], []
                    for k in range(3):
                        diff = pos[j][3 * qi + k] - pos[j][3 * qj + k]
                        ek = (err[j][3 * qi + k] + err[j][3 * qj + k]) * (1 + U) + U * abs(diff)
                        if k == 2:
                            diff, ek = diff / dw, ek * (1 + U) / dw + U * abs(diff) / dw
                        d.append(diff), e.append(ek)
                    norm = _to_f(_sqrt(sum(x * x for x in d)))
                    enorm = _to_f(_sqrt(sum(x * x for x in e))) * (1 + F(1, 10 ** 50))
                    rs = rad[qi] + rad[qj]
                    self.ratios[(j, qi, qj)] = (norm / rs, (enorm * (1 + gamma(5)) + gamma(5) * norm) / rs)
        total, etotal = F(0), F(0)
        for a in range(N):
            for j in range(ns - 1):
                d = [pos[j + 1][3 * a + k] - pos[j][3 * a + k] for k in range(3)]
                e = [(err[j + 1][3 * a + k] + err[j][3 * a + k]) * (1 + U) + U * abs(d[k]) for k in range(3)]
                norm = _to_f(_sqrt(sum(x * x for x in d)))
                enorm = _to_f(_sqrt(sum(x * x for x in e))) * (1 + F(1, 10 ** 50))
                total += norm
                etotal += enorm * (1 + gamma(3)) + gamma(3) * norm
        self.distance = total
        n = max(N * (ns - 1), 1) if pow_terms else max(ns + N - 2, 1)
        self.distance_bound = etotal * (1 + gamma(n)) + gamma(n) * total

    def minimum(self):
        """(key, ratio, bound) of the exact minimum under the rule's order, or None"""
        best = None
        for key in sorted(self.ratios):
            r, b = self.ratios[key]
            if best is None or r < best[1]:
                best = (key, r, b)
        return best

    def minimiser_is_certain(self):
        """every other candidate is further from the minimum than both bounds together: the computed minimiser must be the exact one"""
        key, r, b = self.minimum()
        return all(r2 - b2 > r + b for k2, (r2, b2) in self.ratios.items() if k2 != key)
