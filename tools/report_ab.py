"""A/B of a sweep's report: every downloaded plan through host.validate against one Session.report() on the resident plans
(profiles/report_ab.txt).  One process, host clock around calls that end synchronised, a warm-up of both routes, then alternating
repetitions; medians with min / max.  The session is the hand-off sweep's: worlds, searches and plans made on the device, then planned once.

  (a) Session.download() followed by host.validate per mission: today's report lines
  (b) Session.report(): two kernels and one copy of K small records, no download
  at K = 50 (64 agents x map1..50) and K = 50 x --copies (2000: bench.py's residency)

--only-report: plan, then nothing but three Session.report() calls per K -- the run to put under `rocprofv3 --kernel-trace --stats`.

usage: python tools/report_ab.py [--reps 5] [--maps 1-50] [--copies 40] [--only-report]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from swarm_simulator_amd import host, planner, test_all  # noqa: E402
from swarm_simulator_amd.types import Param  # noqa: E402


def line(name, ts, extra=""):
    ms = [1e3 * t for t in ts]
    print(f"({name:<10}) median {statistics.median(ms):10.3f} ms   min {min(ms):10.3f}   max {max(ms):10.3f}   ({len(ms)} alternating repetitions){extra}", flush=True)
    return statistics.median(ms), max(ms) - min(ms)


def planned_session(ws, W, copies, m, p):
    search = planner.ecbs_search_batch(ws, list(range(W)) * copies, [m] * (W * copies), p)
    assert not any(search.status), "a search failed"
    sess = planner.Session.from_ecbs(search, p)
    search.close()
    sess.run()
    return sess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--copies", type=int, default=40)
    ap.add_argument("--mission", default="mission_64agents_15.json")
    ap.add_argument("--only-report", action="store_true")
    args = ap.parse_args()
    p, m = Param.test_sweep(), host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    W, ok = len(maps), True
    print(f"# tools/report_ab.py --reps {args.reps} --copies {args.copies}: {W} maps x {m.qn} agents, dt 0.1")
    for copies in (1, args.copies):
        K = W * copies
        sess = planned_session(ws, W, copies, m, p)

        def route_a():
            st = sess.download()
            return st, [host.validate(m, p, pl) for pl in sess.plans]

        def route_b():
            return sess.report()

        if args.only_report:
            for _ in range(3):
                route_b()
            sess.close()
            continue
        (st, va), rb = route_a(), route_b()   # warm-up, and the comparison
        same = st == [r.status for r in rb] == [0] * K and all(r.bits() == host.report(m, p, pl).bits() for r, pl in zip(rb, sess.plans))
        dr = max(abs(r.min_safety_ratio - v[0]) for r, v in zip(rb, va))
        dd = max(abs(r.total_flight_distance - v[1]) / v[1] for r, v in zip(rb, va))
        ok = ok and same
        print(f"K = {K}: segments {min(pl.M for pl in sess.plans)}..{max(pl.M for pl in sess.plans)}, samples {min(r.samples for r in rb)}..{max(r.samples for r in rb)}; "
              f"(b) equals host.report of the downloaded plans bit for bit: {same}; against host.validate: ratio differs by at most {dr:.2e}, "
              f"distance by at most {dd:.2e} relative")
        ta, tb, td = [], [], []
        for _ in range(args.reps):
            for ts, fn in ((ta, route_a), (tb, route_b), (td, sess.download)):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
        a, sa = line(f"a K={K}", ta, f"   {1e3 * statistics.median(ta) / K:.3f} ms per mission")
        b, sb = line(f"b K={K}", tb, f"   {1e6 * statistics.median(tb) / K:.2f} us per mission")
        line(f"dl K={K}", td, "   the download alone (part of (a))")
        print(f"K = {K}: (a) / (b) = {a / b:.1f};  (a) - (b) = {a - b:.3f} ms against the larger run-to-run spread (max - min) of the two routes, {max(sa, sb):.3f} ms")
        sess.close()
    ws.close()
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
