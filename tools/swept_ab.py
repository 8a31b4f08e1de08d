"""A/B of a sweep's certified clearance to the obstacles in continuous time: every downloaded plan through host.swept_clearance against one
Session.swept_clearance() on the resident plans and grids (profiles/swept_ab.txt).  One process, host clock around calls that end
synchronised, a warm-up of every route, then alternating repetitions; medians with min / max.  The session is the hand-off sweep's: worlds,
searches and plans made on the device, then planned once.  The grids are downloaded once, before the clock starts.

  (a) Session.download() followed by host.swept_clearance per mission, depth 4, everything refined: what a caller had to do before
  (b) Session.swept_clearance(depth=4, refine_below=1e9): every item through the work list, 16 pieces each
  (c) as (b) with every agent's lower clearance into a host array, through the staging buffer
  (d) as (a) at the defaults (refine_below 0.5)
  (e) as (b) at the defaults: the coarse kernel over every item, the refine kernel over the listed ones

No speed is required of this call; the numbers are the record.  With them come the 50 intervals: how many maps are certified
(lower_clearance > -1e-6, uncertified == 0) and where the continuous lower bound lies below the sampled minimum of Session.clearance(0.1).

usage: python tools/swept_ab.py [--reps 7] [--maps 1-50] [--out profiles/swept_ab.txt]
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "swept_ab.txt"))
    args = ap.parse_args()
    if planner.lib().rbp_device_count() < 1:
        raise SystemExit("tools/swept_ab.py: no HIP device: nothing here is measured on a CPU")
    p, m = Param.test_sweep(), host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    K, N, D = len(maps), m.qn, args.depth
    say(f"# tools/swept_ab.py --reps {args.reps}: {K} maps x {N} agents, depth {D}")
    search = planner.ecbs_search_batch(ws, list(range(K)), [m] * K, p)
    assert not any(search.status), "a search failed"
    sess = planner.Session.from_ecbs(search, p)
    search.close()
    sess.run()
    grids = [ws[k].download() for k in range(K)]

    def on_host(below):
        def route():
            st = sess.download()
            return st, [host.swept_clearance(w, m, pl, D, below, per_agent=True) for w, pl in zip(grids, sess.plans)]
        return route

    routes = [("a", on_host(1e9)), ("b", lambda: sess.swept_clearance(D, 1e9)), ("c", lambda: sess.swept_clearance(D, 1e9, per_agent=True)),
              ("d", on_host(0.5)), ("e", lambda: sess.swept_clearance(D, 0.5))]
    (sta, ra), (rb, _), (rc, agents), (std, rd), (re_, _) = [fn() for _, fn in routes]   # warm-up, and the comparison
    same = sta == std == [0] * K and [r.bits() for r in rb] == [r.bits() for r, _ in ra] == [r.bits() for r in rc]
    same = same and [r.bits() for r in re_] == [r.bits() for r, _ in rd]
    same = same and np.array_equal(agents.view(np.uint64), np.stack([a for _, a in ra]).view(np.uint64))
    items = sum(N * pl.M for pl in sess.plans)
    say(f"K = {K}: segments {min(pl.M for pl in sess.plans)}..{max(pl.M for pl in sess.plans)}, {items} (agent, segment) items, {sum(r.refined for r in re_)} of them "
        f"refined at refine_below 0.5 ({100.0 * sum(r.refined for r in re_) / items:.2f} %), {sum(r.refined for r in rb)} at 1e9; (b), (c), (e) equal "
        f"host.swept_clearance of the downloaded plans bit for bit: {same}")
    sampled = sess.clearance(0.1)[0]
    certified = sum(r.uncertified == 0 and r.lower_clearance > -1e-6 for r in rb)
    below = [(i, r.lower_clearance, s.min_clearance) for i, r, s in zip(maps, rb, sampled) if r.lower_clearance < s.min_clearance]
    say(f"K = {K}: maps certified (uncertified == 0, lower > -1e-6) {certified}; uncertified items {sum(r.uncertified for r in rb)}, hitting {sum(r.hitting for r in rb)}, "
        f"outside {sum(r.outside for r in rb)}, over budget {sum(r.over_budget for r in rb)}; the defaults certify {sum(r.uncertified == 0 for r in re_)} maps and give "
        f"{'the same' if [(r.lower_clearance, r.upper_clearance) for r in re_] == [(r.lower_clearance, r.upper_clearance) for r in rb] else 'other'} intervals")
    say(f"K = {K}: smallest lower clearance {min(r.lower_clearance for r in rb):.5f}, smallest upper {min(r.upper_clearance for r in rb):.5f}, smallest sampled at dt 0.1 "
        f"{min(s.min_clearance for s in sampled):.5f}; sampled hits {sum(s.hits for s in sampled)}; the continuous lower bound lies below the sampled minimum on "
        f"{len(below)} maps: " + ", ".join(f"map{i} {lo:.5f} < {sm:.5f}" for i, lo, sm in below))
    for i, r in zip(maps, rb):
        say(f"  map{i}: [{r.lower_clearance:.5f}, {r.upper_clearance:.5f}]")
    times = {name: [] for name, _ in routes}
    for _ in range(args.reps):
        for name, fn in routes:
            t0 = time.perf_counter()
            r = fn()
            times[name].append(time.perf_counter() - t0)
            del r
    med = {name: line(f"{name} K={K}", times[name], f"   {1e3 * statistics.median(times[name]) / K:.3f} ms per mission") for name, _ in routes}
    for host_route, dev_route, what in (("a", "b", "everything refined"), ("a", "c", "everything refined, agents to the host"), ("d", "e", "refine_below 0.5")):
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
