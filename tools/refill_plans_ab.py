"""A/B of loading a caller's host plans into a session (profiles/refill_plans_ab.txt).  One process, host clock around calls that end
synchronised, a warm-up of both routes, then alternating repetitions; medians with min / max.

The clock runs from "host plans exist" to "session ready to run": K host plans (planner.ecbs_plan_batch, downloaded beforehand), their
missions and the resident worlds are given, and the route ends when a run could be enqueued and everything the route put on the device
has arrived (route (a) returns synchronised; route (b) is followed by Session.scalars, which synchronises the stream).

  route (a), the parent's: rbp_session_create (planner.Session(...)): a new arena, a synchronous clear, seven blocking uploads per mission
             "+ close": with the release of the session, which a caller that plans batch after batch pays per batch on this route
  route (b), the new one:  rbp_session_refill_from_plans (Session.refill_plans) into ONE planner.Session.reserved of the capacity whose
             staging block exists (Session.reserve_plan_stage): packed rounds, one copy and one kernel per round
  "C call": the library call alone on ctypes arrays built beforehand -- (a) rbp_session_create, (b) rbp_session_refill_from_plans and
            the synchronisation; "python": the planner.Session method, which builds those arrays from the K PlanResults on both routes;
  "(b) call alone": rbp_session_refill_from_plans without the synchronisation (it only enqueues: the host's time).

Before anything is timed both routes run; at the small K their downloads are compared bit for bit, at the large K the missions' time
scales and costs (Session.scalars).

usage: python tools/refill_plans_ab.py [--reps 7] [--reps-big 5] [--maps 1-50] [--copies 40]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from swarm_simulator_amd import _abi as A  # noqa: E402
from swarm_simulator_amd import host, planner, test_all  # noqa: E402
from swarm_simulator_amd.types import Param  # noqa: E402

BUDGET, MAX_M = 128, 64
FIELDS = ("T", "coef", "ctrl", "sfc_count", "sfc_box", "sfc_time", "rsfc_normal", "rsfc_time")


def line(name, ts):
    ms = [1e3 * t for t in ts]
    print(f"({name:<44}) median {statistics.median(ms):10.3f} ms   min {min(ms):10.3f}   max {max(ms):10.3f}   ({len(ms)} alternating repetitions)", flush=True)
    return statistics.median(ms), max(ms) - min(ms)


def verdict(what, a, b):
    (ma, sa), (mb, sb) = a, b
    spread = max(sa, sb)
    v = "a gain" if ma - mb > 3 * spread else ("a LOSS" if mb - ma > 3 * spread else "inside the spread")
    print(f"{what}: (a) - (b) = {ma - mb:.3f} ms, (a) / (b) = {ma / mb:.2f}; spreads (max - min) {sa:.3f} / {sb:.3f} ms -> {v} "
          f"(the difference against three times the larger spread)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reps-big", type=int, default=5)
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--copies", type=int, default=40)
    ap.add_argument("--mission", default="mission_64agents_15.json")
    args = ap.parse_args()
    p, m = Param.test_sweep(), host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    W = len(maps)
    L = planner.lib()
    print(f"# tools/refill_plans_ab.py --reps {args.reps} --reps-big {args.reps_big}: {W} maps x copies, {m.qn} agents")
    inits = planner.ecbs_plan_batch(ws, list(range(W)), [m] * W, p, max_nodes=BUDGET, max_M=MAX_M)
    assert not any(inits.status)

    def done(sess):
        return sess.scalars(n=2)   # synchronises the stream

    ok = True
    for copies, reps in ((1, args.reps), (args.copies, args.reps_big)):
        K = W * copies
        idx = list(range(W)) * copies
        worlds, missions = [ws[i] for i in idx], [m] * K

        def plans():
            return [inits[i].clone_inputs() for i in idx]

        Ms = [inits[i].M for i in idx]
        cap = (K, m.qn, max(Ms), max(Ms))
        resident = planner.Session.reserved(ws, *cap, p)
        resident.reserve_plan_stage()
        # warm-up of both routes, and the comparison of what they plan
        fresh = planner.Session(worlds, missions, p, plans())
        fresh.run()
        resident.refill_plans(worlds, missions, plans())
        resident.run()
        if copies == 1:
            sa, sb = fresh.download(), resident.download()
            same = not any(sa) and not any(sb)
            for a, b in zip(fresh.plans, resident.plans):
                same = same and all(np.array_equal(getattr(a, f).view(np.uint8), getattr(b, f).view(np.uint8)) for f in FIELDS)
                same = same and (a.time_scale, a.total_cost, a.qp_iterations) == (b.time_scale, b.total_cost, b.qp_iterations)
            print(f"K = {K}: both routes download the same bits ({', '.join(FIELDS)}, time_scale, total_cost, qp_iterations of every mission): {same}")
        else:
            same = np.array_equal(done(fresh).view(np.uint64), done(resident).view(np.uint64))
            print(f"K = {K}: both routes plan the same time scales and costs (bits of Session.scalars(2) of every mission): {same}")
        ok = ok and same
        fresh.close()
        stage = planner.plan_stage_bytes(cap, K)
        print(f"K = {K}, M {min(Ms)}..{max(Ms)}, capacity {cap}, staged bytes of the batch {sum(planner.plan_stage_bytes((1, m.qn, M, 1), 1) for M in Ms)}, "
              f"block {min(stage, A.RBP_REFILL_STAGE_BYTES)}")
        # ctypes arrays of the batch, built once: what the C calls take
        keep = plans()
        cw = (A.rbp_world * K)(*[x.c_struct() for x in worlds])
        cm = (A.rbp_mission * K)(*[x.c_struct() for x in missions])
        cp = (A.rbp_plan * K)(*[x.c_struct() for x in keep])
        pc = p.c_struct()
        t = {k: [] for k in ("a_c", "a_c_close", "a_py", "a_py_close", "b_c", "b_call", "b_py")}
        for _ in range(reps):
            h = C.c_void_p()
            t0 = time.perf_counter()
            rc = L.rbp_session_create(C.byref(h), 0, K, cw, cm, C.byref(pc), cp)
            t1 = time.perf_counter()
            L.rbp_session_destroy(h)
            t2 = time.perf_counter()
            assert rc == 0, planner.last_error()
            t["a_c"].append(t1 - t0), t["a_c_close"].append(t2 - t0)
            t0 = time.perf_counter()
            rc = L.rbp_session_refill_from_plans(resident._h, K, cw, cm, cp, None)
            t1 = time.perf_counter()
            done(resident)
            t2 = time.perf_counter()
            assert rc == 0, planner.last_error()
            t["b_call"].append(t1 - t0), t["b_c"].append(t2 - t0)
            pl = plans()
            t0 = time.perf_counter()
            s = planner.Session(worlds, missions, p, pl)
            t1 = time.perf_counter()
            s.close()
            t2 = time.perf_counter()
            t["a_py"].append(t1 - t0), t["a_py_close"].append(t2 - t0)
            pl = plans()
            t0 = time.perf_counter()
            resident.refill_plans(worlds, missions, pl)
            done(resident)
            t["b_py"].append(time.perf_counter() - t0)
        a_c = line(f"a K={K} C call rbp_session_create", t["a_c"])
        a_cc = line(f"a K={K} C call rbp_session_create + destroy", t["a_c_close"])
        b_c = line(f"b K={K} C call refill_from_plans + sync", t["b_c"])
        line(f"b K={K} C call refill_from_plans alone", t["b_call"])
        a_py = line(f"a K={K} python Session(...)", t["a_py"])
        a_pyc = line(f"a K={K} python Session(...) + close", t["a_py_close"])
        b_py = line(f"b K={K} python refill_plans + sync", t["b_py"])
        verdict(f"K = {K} C call, ready to run", a_c, b_c)
        verdict(f"K = {K} C call, with (a)'s release", a_cc, b_c)
        verdict(f"K = {K} python, ready to run", a_py, b_py)
        verdict(f"K = {K} python, with (a)'s release", a_pyc, b_py)
        resident.close()
    ws.close()
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
