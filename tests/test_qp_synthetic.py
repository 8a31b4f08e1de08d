"""The synthetic QP cases (tests/synth_qp.py: short missions, few agents, non-unit segment times) keep their promises, and the certificate's
repair for rows that the equalities decide.  CPU only: oracle + tests/golden/make_kkt_reference.py.

These are conditions on the INPUTS of test_gpu_qp_synthetic.py -- (a)-(e) of synth_qp's docstring -- checked here so that the GPU test
spends its time on the kernels.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_kkt_reference as K  # noqa: E402

from tests import synth_qp as SQ  # noqa: E402
from tests.common import Case  # noqa: E402
from tests.test_kkt_reference import FWD_TOL, certify_case, check_reports  # noqa: E402

KEYS = SQ.all_keys()


def test_the_case_list_covers_what_it_says():
    """every N meets every M and at least three duration kinds, two of them non-uniform; nothing outside [0.5, 4], no neighbours beyond 1 : 8;
    every session holds a dozen missions at the most"""
    assert SQ.NS == (1, 2, 3, 4, 7, 8, 11, 16)
    names = set()
    for N in SQ.NS:
        ms, kinds = set(), set()
        for si, sc in enumerate(SQ.SCHEDULES[N]):
            assert 1 <= sc.count <= 12
            for j in range(sc.count):
                c, _ = SQ.case(N, si, j)
                assert c.N == N and c.init_traj.shape == (N, c.M + 1, 3) and c.T.shape == (c.M + 1,) and c.T[0] == 0.0
                dts = np.diff(c.T)
                assert dts.min() >= 0.5 and dts.max() <= 4.0 and (dts[1:] / dts[:-1]).max(initial=1.0) <= 8.0 and (dts[:-1] / dts[1:]).max(initial=1.0) <= 8.0
                assert np.array_equal(c.mission.goal[:, :3], c.init_traj[:, c.M].astype(np.float64)) and not c.mission.goal[:, 3:].any()
                assert c.param().time_scale is False
                ms.add(c.M), kinds.add(c.kind), names.add(c.name)
        assert ms == set(SQ.MS), N
        assert len(kinds) >= 3 and len([k for k in kinds if not k.startswith("u")]) >= 2, N
    assert len(names) == len(KEYS)   # no case was left out, none stands twice
    sched = {(N, sc.name) for N in SQ.NS for sc in SQ.SCHEDULES[N]}
    assert {(1, "bs4"), (2, "bs1"), (2, "bs4"), (3, "bs2"), (4, "bs4"), (7, "bs4"), (7, "bs8"), (8, "bs3"), (11, "bs4"), (16, "joint"),
            (16, "bs8_iteration2"), (2, "wide"), (3, "wide"), (7, "wide")} <= sched


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "n%d_s%d_%d" % k)
def test_case_keeps_its_promises(key):
    c, f = SQ.case(*key)
    o = f.oracle
    assert o.rc_corridor == 0 and o.rc_planner == 0 and o.report["n_polished"] == o.report["n_qp"] == c.qp_solves()   # (a)
    check_reports(f.reports, FWD_TOL / 10)                                                                           # (b), (c)
    assert len(f.reports) == c.qp_solves() // c.passes()
    if not c.uniform:
        assert f.moved >= SQ.MOVE_MIN, f.moved                                                                       # (d)
        assert f.unit_fwd > SQ.REJECT_MIN and not f.unit_accepted, f.unit_fwd                                        # (e)
    assert c.seed[3] == SQ.FIRST_SEED.get(key, 0), f"FIRST_SEED[{key}] should be {c.seed[3]}"


def test_the_cases_have_active_rows_and_implied_rows():
    """an unconstrained QP checks only the knot solve: at least a third of the cases have active rows that the equalities do not decide;
    at least one QP has rows that they do (the certificate's repair is exercised by the cases themselves)"""
    fs = [SQ.case(*k)[1] for k in KEYS]
    assert sum(f.n_implied > 0 for f in fs) >= 1
    assert 3 * sum(f.n_active > 0 for f in fs) >= len(fs), [f.n_active for f in fs]
    worst = {}
    for k in KEYS:
        c, f = SQ.case(*k)
        worst[(c.N, c.kind)] = max(worst.get((c.N, c.kind), 0.0), f.fwd)
    print("\noracle forward error [m] per (N, kind): " + ", ".join(f"{k[0]}/{k[1]} {v:.1e}" for k, v in sorted(worst.items())))


def _opened_case():
    return SQ.make_case("s4_map1_seq2", [0, 1], 4, np.random.default_rng(30).uniform(0.5, 4.0, 4), SQ.Sched("bs4", (("batch_size", 4),)))


def test_certificate_drops_rows_that_the_equalities_decide(monkeypatch):
    """a start or goal exactly on a face of its SFC box: the box rows of the pinned control points are active with slack 0 and vanish under
    the equality elimination.  Left in, _nullspace takes its rank relative to rounding noise and the report is nonsense."""
    c = _opened_case()
    o = SQ.run_oracle(c)
    assert o.ok
    rep, = SQ.certify(c, o.plan, o.plan.ctrl)
    assert rep["n_implied"] == 3 and rep["n_active"] == 3   # nothing else is active: the largest singular value of G_A Z is noise
    check_reports([rep], 1e-10)
    assert rep["stationarity"] < 1e-10
    monkeypatch.setattr(K, "IMPLIED_RTOL", -1.0)   # the repair taken out: no row is ever dropped
    bad, = SQ.certify(c, o.plan, o.plan.ctrl)
    assert bad["n_implied"] == 0
    assert bad["forward_error"] > 1e-3 or bad["lambda_max"] > 1e12


def test_golden_reports_are_unchanged_by_the_repair(monkeypatch):
    """the reports of the five golden cases of test_oracle_goldens_are_certified_optima, with the repair and with it taken out (the path
    certify_batch took before it): the same to the last bit apart from the new key.  s4_map1_joint and batch 1 of s4_map1_seq2 hold three
    implied rows each, next to rows that do constrain: those stay in."""
    names = ["c1_4agents_empty_joint", "c1_4agents_empty_seq2", "s4_map1_joint", "s4_map1_seq2", "s8_map5_seq4"]
    now = [certify_case(Case(name), Case(name).g["ctrl"]) for name in names]
    monkeypatch.setattr(K, "IMPLIED_RTOL", -1.0)
    before = [certify_case(Case(name), Case(name).g["ctrl"]) for name in names]
    assert [r["n_implied"] for reps in now for r in reps] == [0, 0, 0, 3, 0, 3, 0, 0]
    for ra, rb in zip(now, before):
        assert len(ra) == len(rb)
        for a, b in zip(ra, rb):
            assert a.keys() == b.keys() and b["n_implied"] == 0 and a["n_implied"] < max(a["n_active"], 1)
            for k in a:
                if k != "n_implied":
                    assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
