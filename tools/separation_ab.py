"""A/B of a sweep's certified separation in continuous time: every downloaded plan through host.separation against one
Session.separation() on the resident plans (profiles/separation_ab.txt).  One process, host clock around calls that end synchronised, a
warm-up of every route, then alternating repetitions; medians with min / max.  The session is the hand-off sweep's: worlds, searches and
plans made on the device, then planned once.

  (a) Session.download() followed by host.separation per mission, depth 4, refine_below 2.0: what a caller had to do before
  (b) Session.separation(depth=4, refine_below=2.0): the coarse kernel over every item, the refine kernel over the listed ones
  (c) as (a) with everything refined (refine_below 1e9)
  (d) as (b) with everything refined: every item through the work list, 16 pieces each
  (e) as (b) with every pair's lower ratio into a host array, through the staging buffer

No speed is required of this call; the numbers are the record.  The share of items refined is printed with them.

usage: python tools/separation_ab.py [--reps 7] [--maps 1-50] [--out profiles/separation_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from swarm_simulator_amd import host, planner, test_all  # noqa: E402
from swarm_simulator_amd.types import Param  # noqa: E402

OUT = []


def say(text):
    print(text, flush=True)
    OUT.append(text)


def line(name, ts, extra=""):
    ms = [1e3 * t for t in ts]
    say(f"({name:<10}) median {statistics.median(ms):10.3f} ms   min {min(ms):10.3f}   max {max(ms):10.3f}   ({len(ms)} alternating repetitions){extra}")
    return statistics.median(ms), max(ms) - min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--mission", default="mission_64agents_15.json")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "separation_ab.txt"))
    args = ap.parse_args()
    if planner.lib().rbp_device_count() < 1:
        raise SystemExit("tools/separation_ab.py: no HIP device: nothing here is measured on a CPU")
    p, m = Param.test_sweep(), host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    K, N, D = len(maps), m.qn, args.depth
    say(f"# tools/separation_ab.py --reps {args.reps}: {K} maps x {N} agents, depth {D}")
    search = planner.ecbs_search_batch(ws, list(range(K)), [m] * K, p)
    assert not any(search.status), "a search failed"
    sess = planner.Session.from_ecbs(search, p)
    search.close()
    sess.run()

    def on_host(below):
        def route():
            st = sess.download()
            return st, [host.separation(m, p, pl, D, below, per_pair=True) for pl in sess.plans]
        return route

    routes = [("a", on_host(2.0)), ("b", lambda: sess.separation(D, 2.0)), ("c", on_host(1e9)), ("d", lambda: sess.separation(D, 1e9)),
              ("e", lambda: sess.separation(D, 2.0, per_pair=True))]
    (sta, ra), (rb, _), (stc, rc), (rd, _), (re_, pairs) = [fn() for _, fn in routes]   # warm-up, and the comparison
    same = sta == stc == [0] * K and [r.bits() for r in rb] == [r.bits() for r, _ in ra] == [r.bits() for r in re_]
    same = same and [r.bits() for r in rd] == [r.bits() for r, _ in rc]
    same = same and np.array_equal(pairs.view(np.uint64), np.stack([a for _, a in ra]).view(np.uint64))
    items = sum(N * (N - 1) // 2 * pl.M for pl in sess.plans)
    refined = sum(r.refined for r in rb)
    say(f"K = {K}: segments {min(pl.M for pl in sess.plans)}..{max(pl.M for pl in sess.plans)}, {items} (pair, segment) items, {refined} of them refined at "
        f"refine_below 2.0 ({100.0 * refined / items:.2f} %), {sum(r.refined for r in rd)} at 1e9; (b), (d), (e) equal host.separation of the downloaded plans "
        f"bit for bit: {same}")
    say(f"K = {K}: smallest lower ratio {min(r.lower_ratio for r in rb):.5f}, smallest upper ratio {min(r.upper_ratio for r in rb):.5f}, "
        f"missions certified (lower >= 1) {sum(r.lower_ratio >= 1 for r in rb)}, uncertified items {sum(r.uncertified for r in rb)}, "
        f"colliding items {sum(r.colliding for r in rb)}; sampled at dt 0.1: smallest ratio {min(r.min_safety_ratio for r in sess.report(0.1)):.5f}")
    times = {name: [] for name, _ in routes}
    for _ in range(args.reps):
        for name, fn in routes:
            t0 = time.perf_counter()
            r = fn()
            times[name].append(time.perf_counter() - t0)
            del r
    med = {name: line(f"{name} K={K}", times[name], f"   {1e3 * statistics.median(times[name]) / K:.3f} ms per mission") for name, _ in routes}
    for host_route, dev_route, what in (("a", "b", "refine_below 2.0"), ("c", "d", "everything refined"), ("a", "e", "refine_below 2.0, pairs to the host")):
        (a, spa), (b, spb) = med[host_route], med[dev_route]
        say(f"K = {K}, {what}: ({host_route}) / ({dev_route}) = {a / b:.1f};  ({host_route}) - ({dev_route}) = {a - b:.3f} ms against the run-to-run spreads "
            f"(max - min) {spa:.3f} / {spb:.3f} ms: the device call is faster by more than both spreads: {a - b > spa and a - b > spb}")
    sess.close()
    ws.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(OUT) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    raise SystemExit(main())
