"""The state rule (csrc/common/state_rules.h: velocity, acceleration, a sample's nine values, limit peaks, ratio curves), as the HOST compiler
builds it: tests/state_rules/state_main.cpp includes nothing but that header, is compiled with every warning an error and with the
undefined-behaviour and address sanitizers, and (1) checks hand-computed cases -- Horner over the differentiated coefficients with every
operation rounded on its own, rows 0..2 the bits of report_rules::agent_position, a sample on a knot in the earlier segment with random
coefficients on both sides, the peak order under ties between samples, agents and axes, zero / NaN / negative ratios never taken, the
curves' NaN rule, a row too short storing nothing -- and (2) evaluates seeded synthetic missions handed to it in hexadecimal, which are
judged here against the exact fractions.Fraction restatement of tests/synth_states.py within bounds counted from the operations.

Largest observed error / bound quotients (this suite's cases, x86-64 g++): velocity 0.193, acceleration 0.248, limit ratio 0.107, curves 0.064.
(The device compiler's reading of the same text is held to the host's bits by tests/test_gpu_dynamics.py.)  CPU only."""
import os
import re
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from swarm_simulator_amd import _abi as A
from tests import synth_report as S
from tests import synth_states as X

HEADER = os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc", "common", "state_rules.h")
SRC = os.path.join(A.REPO_ROOT, "tests", "state_rules", "state_main.cpp")
INC = ["-I" + os.path.join(A.REPO_ROOT, "swarm_simulator_amd", "csrc")]   # (not include/: the header stands alone)

# (seed, N, M, times, time scale, dt): samples on knots (unit times, dt 0.1 / 0.25), off them (0.07), scaled times, one agent
CASES = [(1, 2, 1, "unit", 1.0, 0.1), (2, 3, 2, "nonunit", 1.0, 0.25), (3, 4, 3, "alternating", 1.1, 0.07), (5, 1, 2, "unit", 1.4641, 0.1)]
IDS = ["N2_M1_unit", "N3_M2_nonunit_dt025", "N4_M3_alternating_ts11_dt007", "N1_M2_ts14641"]

QUOTIENTS = {}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("state_rules") / "state_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover"] + INC + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def hexes(a):
    return " ".join(float(x).hex() for x in np.asarray(a, np.float64).reshape(-1))


def evaluate(program, plans, ts, dt, max_vel, max_acc, S_stride):
    """states_sequential of mission 0 of `plans` as the program computes it: dict of samples, stored, vel, acc, end_time, states, curves"""
    N, M = plans.N, int(plans.M[0])
    text = "\n".join([f"{N} {M} {S_stride}", hexes([dt, ts, plans.downwash]), hexes(plans.T[0, :M + 1]), hexes(plans.coefs[0]), hexes(plans.radius[0]),
                      hexes(max_vel), hexes(max_acc)]) + "\n"
    r = subprocess.run([program, "eval"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        name, *w = line.split()
        if name == "samples":
            out["samples"], out["stored"] = int(w[0]), int(w[2])
        elif name in ("vel", "acc"):
            out[name] = tuple(int(x) for x in w[:3]) + tuple(float.fromhex(x) for x in w[3:])
        else:
            out[name] = np.array([float.fromhex(x) for x in w])
    out["states"] = out["states"].reshape(N, 9, S_stride)
    out["curves"] = out["curves"].reshape(S_stride, 2)
    return out


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request, program):
    seed, N, M, kind, ts, dt = request.param
    plans = S.make(seed, N, [M], kind, [ts])
    max_vel, max_acc = X.limits(seed, 1, N)
    T = plans.scaled_T(0)
    ex = X.Exact(T, plans.coefs[0], plans.radius[0], plans.downwash, dt)
    got = evaluate(program, plans, ts, dt, max_vel[0], max_acc[0], ex.samples + 2)
    return plans, ex, got, max_vel[0], max_acc[0], dt


def test_the_rule_holds_on_hand_computed_cases_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "state rules ok" in r.stdout


def test_the_header_includes_nothing_but_the_report_rules():
    """... which include <math.h> and <stdint.h> and nothing else (tests/test_report_rules.py)"""
    assert re.findall(r"^\s*#\s*include\s*(\S+)", open(HEADER).read(), flags=re.M) == ['"common/report_rules.h"']


def test_velocity_and_acceleration_lie_within_the_counted_bound_of_the_exact_values(case):
    plans, ex, got, _, _, _ = case
    assert got["samples"] == ex.samples > 0 and got["stored"] == 1 and got["end_time"][0] == plans.scaled_T(0)[-1]
    for name, base, rows in (("velocity", 3, ex.vel), ("acceleration", 6, ex.acc)):
        worst = 0.0
        for j, row in enumerate(rows):
            for i, (x, e) in enumerate(row):
                err = abs(F(float(got["states"][i // 3, base + i % 3, j])) - x)
                assert err <= e, (name, j, i, float(err), float(e))
                if e:
                    worst = max(worst, float(err / e))
        print(f"largest error / bound, {name}: {worst:.3g}")
        QUOTIENTS.setdefault(name, []).append(worst)
    assert np.all(got["states"][:, :, ex.samples:] == 0.0)   # beyond the samples: as the program's buffer was


def test_position_rows_are_the_exact_positions_within_the_reports_bound(case):
    """(that they are the report's BITS is checked inside the program, against report_rules::agent_position itself)"""
    plans, ex, got, _, _, _ = case
    for j in range(ex.samples):
        for i in range(3 * plans.N):
            assert abs(F(float(got["states"][i // 3, i % 3, j])) - ex.report.pos[j][i]) <= ex.report.err[j][i]


def test_the_peaks_lie_within_the_bound_and_where_the_exact_peaks_lie(case):
    plans, ex, got, max_vel, max_acc, _ = case
    for which, lim in (("vel", max_vel), ("acc", max_acc)):
        ratios = ex.limit_ratios(which, lim)
        key, r, b = X.peak_of(ratios)
        sample, agent, axis, ratio, value, limit = got[which]
        bound = max(b, ratios[(sample, agent, axis)][1])
        err = abs(F(ratio) - r)
        assert err <= bound
        QUOTIENTS.setdefault("limit ratio", []).append(float(err / bound))
        base = 3 if which == "vel" else 6
        assert value == got["states"][agent, base + axis, sample] and limit == lim[agent, axis] and ratio == abs(value) / limit
        assert X.peak_is_certain(ratios), "the case was chosen so that the runner-up is further away than both bounds"
        assert (sample, agent, axis) == key


def test_the_curves_lie_within_the_bound_of_the_exact_extrema(case):
    plans, ex, got, _, _, _ = case
    for j in range(ex.samples):
        c = ex.curve(j)
        if c is None:
            assert tuple(got["curves"][j]) == (1e9, 0.0)   # one agent: no pair
            continue
        for col, (r, b) in enumerate(c):
            err = abs(F(float(got["curves"][j, col])) - r)
            assert err <= b
            QUOTIENTS.setdefault("curves", []).append(float(err / b))
        assert got["curves"][j, 0] <= got["curves"][j, 1]
    assert np.all(got["curves"][ex.samples:] == 0.0)


def test_the_quotients_the_docstring_quotes():
    """prints the largest observed error / bound quotients (run with -s): they must all be at most 1, which the tests above assert"""
    for k, v in QUOTIENTS.items():
        print(f"largest error / bound, {k}: {max(v):.3g}")
    assert QUOTIENTS and all(q <= 1 for v in QUOTIENTS.values() for q in v)
