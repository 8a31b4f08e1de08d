"""A/B of planning batch after batch (profiles/refill_ab.txt).  One process, host clock around calls that end synchronised, a warm-up of
both routes, then alternating repetitions; medians with min / max.

The workload is a planning service's: batch after batch of B missions on the resident worlds, every batch a device search of its own
(planner.ecbs_search_batch).  The searches are made beforehand; the clock runs from "search handle exists" to "PLANNER run complete"
(run, then Session.scalars, which synchronises the stream and copies K x 2 doubles).

  route (a), the parent's: per batch planner.Session.from_ecbs (rbp_session_create_from_ecbs) + run + close
  route (b), the new one:  ONE planner.Session.reserved (rbp_session_create_reserved) for the capacity; per batch refill
             (rbp_session_refill_from_ecbs) + run
  Three batches in a row, the maps rotated by one from batch to batch so that every slot changes its world and its M; the second and
  the third are reported: the first pays the reservations (arena, QP workspace) on both routes.
  "ctor" / "refill" = the constructor alone (it returns synchronised) against the refill call alone (it only enqueues: the host's time).
  "close" = route (a)'s release of the session, part of its batch.

Before anything is timed both routes download the three batches' plans at the small B and the bits are compared; at the large B the
missions' time scales and costs (Session.scalars) are.

usage: python tools/refill_ab.py [--reps 5] [--reps-big 3] [--maps 1-50] [--copies 40]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from swarm_simulator_amd import host, planner, test_all  # noqa: E402
from swarm_simulator_amd.types import Param  # noqa: E402

BUDGET, MAX_M = 128, 64
FIELDS = ("T", "coef", "ctrl", "sfc_count", "sfc_box", "sfc_time", "rsfc_normal", "rsfc_time")


def line(name, ts):
    ms = [1e3 * t for t in ts]
    print(f"({name:<44}) median {statistics.median(ms):10.3f} ms   min {min(ms):10.3f}   max {max(ms):10.3f}   ({len(ms)} alternating repetitions)", flush=True)
    return statistics.median(ms), max(ms) - min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-big", type=int, default=3)
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--copies", type=int, default=40)
    ap.add_argument("--mission", default="mission_64agents_15.json")
    args = ap.parse_args()
    p, m = Param.test_sweep(), host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    W = len(maps)
    print(f"# tools/refill_ab.py --reps {args.reps} --reps-big {args.reps_big}: batches of {W} maps x copies, {m.qn} agents")

    def done(sess):
        return sess.scalars(n=2)   # synchronises the stream: the PLANNER run is complete

    def route_a(searches, t, keep=None):
        for b, search in enumerate(searches):
            t0 = time.perf_counter()
            sess = planner.Session.from_ecbs(search, p)
            t1 = time.perf_counter()
            sess.run()
            sc = done(sess)
            t2 = time.perf_counter()
            if keep is not None:
                keep.append((sess.download(), sess.plans, sc))
            t3 = time.perf_counter()
            sess.close()
            t4 = time.perf_counter()
            t[f"batch{b}"].append((t2 - t0) + (t4 - t3)), t[f"ctor{b}"].append(t1 - t0), t[f"close{b}"].append(t4 - t3)

    def route_b(searches, cap, t, keep=None):
        t0 = time.perf_counter()
        sess = planner.Session.reserved(ws, *cap, p)
        t["reserve"].append(time.perf_counter() - t0)
        for b, search in enumerate(searches):
            t0 = time.perf_counter()
            sess.refill(search)
            t1 = time.perf_counter()
            sess.run()
            sc = done(sess)
            t2 = time.perf_counter()
            if keep is not None:
                keep.append((sess.download(), sess.plans, sc))
            t[f"batch{b}"].append(t2 - t0), t[f"ctor{b}"].append(t1 - t0)
        sess.close()

    def new_times():
        return {k: [] for k in ["reserve"] + [f"{part}{b}" for part in ("batch", "ctor", "close") for b in range(3)]}

    ok = True
    for copies, reps in ((1, args.reps), (args.copies, args.reps_big)):
        B = W * copies
        searches = []
        for shift in range(3):   # batch b: the maps rotated by b
            idx = [(i + shift) % W for i in range(W)] * copies
            searches.append(planner.ecbs_search_batch(ws, idx, [m] * B, p, max_nodes=BUDGET, max_M=MAX_M))
            assert not searches[-1].status.any()
        Ms = np.concatenate([s.M for s in searches])
        cap = (B, m.qn, int(Ms.max()), int(Ms.max()))
        # warm-up of both routes, and the comparison of what they plan
        ka, kb = [], []
        route_a(searches, new_times(), ka if copies == 1 else None)
        route_b(searches, cap, new_times(), kb if copies == 1 else None)
        if copies == 1:
            same = True
            for (sa, pa, _), (sb, pb, _) in zip(ka, kb):
                same = same and not any(sa) and not any(sb) and len(pa) == len(pb)
                for a, b in zip(pa, pb):
                    same = same and all(np.array_equal(getattr(a, f).view(np.uint8), getattr(b, f).view(np.uint8)) for f in FIELDS)
                    same = same and (a.time_scale, a.total_cost, a.qp_iterations) == (b.time_scale, b.total_cost, b.qp_iterations)
            print(f"B = {B}: both routes download the same bits ({', '.join(FIELDS)}, time_scale, total_cost, qp_iterations of every mission of three batches): {same}")
        else:
            sa, sb = [], []
            sess = planner.Session.reserved(ws, *cap, p)
            for search in searches:
                f = planner.Session.from_ecbs(search, p)
                f.run()
                sa.append(done(f))
                f.close()
                sess.refill(search)
                sess.run()
                sb.append(done(sess))
            sess.close()
            same = all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(sa, sb))
            print(f"B = {B}: both routes plan the same time scales and costs (bits of Session.scalars(2) of every mission of three batches): {same}")
        ok = ok and same
        ta, tb = new_times(), new_times()
        for _ in range(reps):
            route_a(searches, ta)
            route_b(searches, cap, tb)
        # the refill as the device sees it: the call, then a synchronisation (Session.scalars), on a session whose QP workspace exists, so
        # that the staged copy, the kernel and the clear of the K' workspace blocks are all inside
        sess = planner.Session.reserved(ws, *cap, p)
        sess.refill(searches[0])
        sess.run()
        done(sess)
        per_mission = sess.workspace_bytes_per_mission()
        t_sync = []
        for _ in range(reps):
            for search in searches:
                t0 = time.perf_counter()
                sess.refill(search)
                done(sess)
                t_sync.append(time.perf_counter() - t0)
        sess.close()
        print(f"B = {B}, M {Ms.min()}..{Ms.max()}, capacity {cap}, QP workspace {cap[0]} x {per_mission} bytes")
        line(f"b B={B} refill + synchronise", t_sync)
        line(f"b B={B} reserve", tb["reserve"])
        for b in (0, 1, 2):
            med = {}
            for part, na, nb in (("batch", "from_ecbs+run+close", "refill+run"), ("ctor", "from_ecbs alone", "refill call alone")):
                med[part, "a"] = line(f"a B={B} batch {b + 1} {na}", ta[f"{part}{b}"])
                med[part, "b"] = line(f"b B={B} batch {b + 1} {nb}", tb[f"{part}{b}"])
            line(f"a B={B} batch {b + 1} close", ta[f"close{b}"])
            for part in ("batch", "ctor"):
                (a, sa_), (c, sb_) = med[part, "a"], med[part, "b"]
                spread = max(sa_, sb_)
                verdict = "a gain" if a - c > 3 * spread else ("a LOSS" if c - a > 3 * spread else "inside the spread")
                print(f"batch {b + 1} {part}: (a) - (b) = {a - c:.3f} ms, (a) / (b) = {a / c:.2f}; spreads (max - min) {sa_:.3f} / {sb_:.3f} ms -> {verdict} "
                      f"(the difference against three times the larger spread){' [first batch: pays the reservations]' if b == 0 else ''}", flush=True)
        for s in searches:
            s.close()
    ws.close()
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
