"""The two quantities the batch QP's polish (csrc/kernels/qp_polish.inc) takes from the mission's table G = K0^-1 instead of from explicit
columns V = K0^-1 J', restated in numpy from Cand-like records and held against the dense products:

    S_ab   = sg_ab (n_a . n_b) (t_a' G[knot_a][knot_b] t_b)              against   J K0^-1 J'
    step   = -K0^-1 (g + J_P' z): the active rows listed per (agent, dim), u = g + J_P' z formed one (knot, agent, dim) triple at a
             time from that list, then the product of the table with u over all knots                    against   the dense product

K0 is the same block-tridiagonal matrix for every (agent, dim); a row touches ONE knot with three coefficients t -- a unit vector on a
control point right of the knot, a row of L_j on one left of it -- times n[k] per dim, with sign + on its own agent and - on the other
agent of a pair row.  No GPU: this pins the algebra (signs, transposes, which block, the exact zeros), the kernels are held to the KKT
certificate by test_gpu_polish_inverse.py.

Both sides read the same table, so they differ by the order of summation alone: the bound is 64 ulps of the sum of the absolute terms.
Pairs of rows that share no agent, or one agent along different axes, must give 0.0 exactly."""
from dataclasses import dataclass

import numpy as np

QBASE = np.array([720, -1800, 1200, 0, 0, -120, -1800, 4800, -3600, 0, 600, 0, 1200, -3600, 3600, -1200, 0, 0, 0, 0, -1200, 3600, -3600, 1200,
                  0, 600, 0, -3600, 4800, -1800, -120, 0, 0, 1200, -1800, 720.0]).reshape(6, 6)
NB = 3                                                        # batch agents
T = np.concatenate([[0.0], np.cumsum([1.0, 0.5, 2.0, 1.3, 0.7, 1.9])])   # M = 6: five knots, ratios above and below 1
M, NJ = len(T) - 1, len(T) - 2
NK = 9 * NB


def continuity_maps():
    L = np.zeros((M + 1, 3, 3))
    for j in range(1, M):
        r = (T[j] - T[j - 1]) / (T[j + 1] - T[j])
        L[j] = [[(1 + r) ** 2, -2 * r * (1 + r), r * r], [1 + r, -r, 0], [1, 0, 0]]
    return L


def k0_dense(L):
    K = np.zeros((3 * NJ, 3 * NJ))
    for j in range(1, M):
        sl, sr, jj = (T[j] - T[j - 1]) ** -5.0, (T[j + 1] - T[j]) ** -5.0, j - 1
        K[3 * jj:3 * jj + 3, 3 * jj:3 * jj + 3] = 2 * (L[j].T @ (QBASE[3:, 3:] * sl) @ L[j] + QBASE[:3, :3] * sr)
        if j + 1 < M:
            E = 2 * (QBASE[:3, 3:] * sr) @ L[j + 1]
            K[3 * jj:3 * jj + 3, 3 * jj + 3:3 * jj + 6] = E
            K[3 * jj + 3:3 * jj + 6, 3 * jj:3 * jj + 3] = E.T
    return K


LK = continuity_maps()
G = np.linalg.inv(k0_dense(LK))
G = np.tril(G) + np.tril(G, -1).T          # the stored table: lower triangle, the rest by transposition


def g_block(ja, jb):
    """3x3 block (ja, jb) of the table, the way the kernel reads it: the stored lower block, transposed when ja < jb"""
    lo = G[3 * max(ja, jb):3 * max(ja, jb) + 3, 3 * min(ja, jb):3 * min(ja, jb) + 3]
    return lo if ja >= jb else lo.T


@dataclass
class Cand:
    n: tuple     # per dim
    t: tuple
    knot: int    # 1-based, as kernels count knots
    a: int
    b: int = -1


def cand(j6, n, a, b=-1):
    """knot_of: control point j6 = 6 m + i -- i < 3: right of knot m, t a unit vector; i >= 3: left of knot m + 1, t = row i - 3 of L"""
    m, i = divmod(j6, 6)
    t = np.eye(3)[i] if i < 3 else LK[m + 1][i - 3]
    return Cand(tuple(float(x) for x in n), tuple(float(x) for x in t), m if i < 3 else m + 1, a, b)


def dense_row(c):
    r = np.zeros(NJ * NK)
    for k in range(3):
        for ag, sg in ((c.a, 1.0), (c.b, -1.0)):
            if ag >= 0:
                i0 = (c.knot - 1) * NK + (ag * 3 + k) * 3
                r[i0:i0 + 3] += sg * c.n[k] * np.asarray(c.t)
    return r


def dense_inverse():
    """K0^-1 of the whole batch: the table's entry wherever agent and dim agree"""
    X = np.zeros((NJ * NK, NJ * NK))
    for ja in range(NJ):
        for jb in range(NJ):
            for sub in range(3 * NB):
                X[ja * NK + sub * 3:ja * NK + sub * 3 + 3, jb * NK + sub * 3:jb * NK + sub * 3 + 3] = g_block(ja, jb)
    return X


def s_entry(ca, cb):
    sg = int(ca.a == cb.a) - int(cb.b >= 0 and ca.a == cb.b) - int(ca.b >= 0 and ca.b == cb.a) + int(ca.b >= 0 and ca.b == cb.b)
    share = ca.a == cb.a or (cb.b >= 0 and ca.a == cb.b) or (ca.b >= 0 and ca.b in (cb.a, cb.b))
    if share and ca.b < 0 and cb.b < 0:
        share = any(x != 0 and y != 0 for x, y in zip(ca.n, cb.n))
    if not share or sg == 0:
        return 0.0
    # the bilinear form on the STORED block: its rows belong to the larger knot (ipm::k0g_bilinear)
    hi, lo = (ca, cb) if ca.knot >= cb.knot else (cb, ca)
    return sg * float(np.dot(ca.n, cb.n)) * float(np.asarray(hi.t) @ g_block(hi.knot - 1, lo.knot - 1) @ np.asarray(lo.t))


def meta_sign(c, ag, k):
    if c.n[k] == 0:
        return 0
    return 1 if ag == c.a else (-1 if ag == c.b else 0)


def primal_step(rows, z, g):
    """the kernel's route: per (agent, dim) the list of active rows in the order of P -- (knot, position, sgn n_k t) --, the sum
    u = g + J_P' z gathered per (knot, agent, dim) from that list, then -G u one (knot, agent, dim) triple at a time over ALL knots"""
    out, u = np.zeros(NJ * NK), g.copy()
    for sub in range(3 * NB):
        ag, k = divmod(sub, 3)
        lst = [(c.knot - 1, b, meta_sign(c, ag, k) * c.n[k] * np.asarray(c.t)) for b, c in enumerate(rows) if meta_sign(c, ag, k)]
        for kb in range(NJ):
            for knot, b, w in lst:
                if knot == kb:
                    u[kb * NK + sub * 3:kb * NK + sub * 3 + 3] += z[b] * w
    for sub in range(3 * NB):
        for jj in range(NJ):
            acc = np.zeros(3)
            for kb in range(NJ):
                acc += g_block(jj, kb) @ u[kb * NK + sub * 3:kb * NK + sub * 3 + 3]
            out[jj * NK + sub * 3:jj * NK + sub * 3 + 3] = -acc
    return out


ROWS = {
    "bound, right of knot 2":         cand(6 * 2 + 1, (0, -1, 0), 0),            # one agent, one dim, t a unit vector
    "bound, left of knot 3":          cand(6 * 2 + 4, (0, 0, 1), 0),             # t = a row of L_3
    "bound, other axis":              cand(6 * 2 + 1, (1, 0, 0), 0),
    "bound, agent 1":                 cand(6 * 3 + 0, (0, -1, 0), 1),
    "frozen, left of knot 1":         cand(6 * 0 + 3, (0.36, -0.48, 0.8), 0),    # one agent, three dims
    "frozen, right of knot 5":        cand(6 * 5 + 2, (-0.6, 0.0, 0.8), 2),
    "pair 0-1, left of knot 2":       cand(6 * 1 + 5, (0.48, 0.6, -0.64), 0, 1), # b >= 0: opposite signs on the two agents
    "pair 1-2, right of knot 4":      cand(6 * 4 + 0, (0.0, 0.8, 0.6), 1, 2),
    "pair 0-2, left of knot 4":       cand(6 * 3 + 4, (0.8, 0.0, -0.6), 0, 2),
}


def test_s_from_the_table_is_j_kinv_jt():
    names, cs = list(ROWS), list(ROWS.values())
    J = np.array([dense_row(c) for c in cs])
    X = dense_inverse()
    dense, bound = J @ X @ J.T, np.abs(J) @ np.abs(X) @ np.abs(J.T)
    worst = 0.0
    for i, ca in enumerate(cs):
        for j, cb in enumerate(cs):
            s = s_entry(ca, cb)
            if ca.knot != cb.knot:  # one stored block, one order of operations: the same bits either way round
                assert s == s_entry(cb, ca), (names[i], names[j])  # (rows on one knot: the kernel computes i >= j and mirrors it)
            tol = 64 * np.finfo(float).eps * bound[i, j]
            assert abs(s - dense[i, j]) <= tol, (names[i], names[j], s, dense[i, j])
            worst = max(worst, abs(s - dense[i, j]) / max(tol, 1e-300))
    print(f"\nS: largest |difference| / bound {worst:.3f} over {len(cs) ** 2} pairs")
    assert np.all(np.diag(dense) > 0)


def test_rows_that_share_nothing_give_an_exact_zero():
    r = ROWS
    for a, b in (("bound, right of knot 2", "bound, agent 1"),            # no common agent
                 ("frozen, left of knot 1", "frozen, right of knot 5"),
                 ("pair 0-1, left of knot 2", "frozen, right of knot 5"),
                 ("bound, right of knot 2", "bound, other axis"),         # one agent, different axes
                 ("bound, left of knot 3", "bound, other axis"),
                 ("bound, other axis", "pair 1-2, right of knot 4")):     # agent 0's row against a pair without agent 0
        assert s_entry(r[a], r[b]) == 0.0 and s_entry(r[b], r[a]) == 0.0, (a, b)
        assert np.dot(dense_row(r[a]), dense_inverse() @ dense_row(r[b])) == 0.0, (a, b)
    # a frozen row whose normal has a zero component shares that axis with nothing
    assert s_entry(r["frozen, right of knot 5"], cand(6 * 5 + 2, (0, 1, 0), 2)) == 0.0


def test_primal_step_from_the_table():
    rng = np.random.default_rng(5)
    cs = list(ROWS.values())
    z = rng.uniform(0.1, 3.0, len(cs))
    g = rng.normal(size=NJ * NK)
    J = np.array([dense_row(c) for c in cs])
    X = dense_inverse()
    dense = -X @ (g + J.T @ z)
    bound = np.abs(X) @ (np.abs(g) + np.abs(J.T) @ z)
    got = primal_step(cs, z, g)
    ratio = np.abs(got - dense) / (64 * np.finfo(float).eps * bound)
    print(f"\nprimal step: largest |difference| / bound {ratio.max():.3f} over {got.size} entries")
    assert np.all(ratio <= 1.0)
    # the step solves K0 step = -(g + J_P' z)  (against K0 itself, not its inverse: cond(K0) ~ 1e6 at five knots)
    K0 = np.zeros_like(X)
    K = k0_dense(LK)
    for sub in range(3 * NB):
        idx = np.array([jj * NK + sub * 3 + e for jj in range(NJ) for e in range(3)])
        K0[np.ix_(idx, idx)] = K
    res = K0 @ got + g + J.T @ z
    assert np.abs(res).max() <= 1e-9 * (np.abs(K0) @ np.abs(got)).max()
