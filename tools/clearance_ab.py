"""A/B of a sweep's clearance to the obstacles: every downloaded plan through host.clearance on its downloaded grid against one
Session.clearance() on the resident plans and grids (profiles/clearance_ab.txt).  One process, host clock around calls that end
synchronised, a warm-up of every route, then alternating repetitions; medians with min / max.  The session is the hand-off sweep's: worlds,
searches and plans made on the device, then planned once.

  (a) Session.download() followed by host.clearance per mission: what a caller had to do before.  The host copies of the 50 grids are made
      BEFORE the clock starts (0.94 MB each: a caller without them pays that download on top), so (a) is the host route at its best
  (b) Session.clearance(): two kernels, K small records
  (c) Session.clearance(per_agent=True): the same with every agent's clearance into a host array, through the staging buffer

usage: python tools/clearance_ab.py [--reps 7] [--maps 1-50] [--out profiles/clearance_ab.txt]
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
    ap.add_argument("--mission", default="mission_64agents_15.json")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "clearance_ab.txt"))
    args = ap.parse_args()
    if planner.lib().rbp_device_count() < 1:
        raise SystemExit("tools/clearance_ab.py: no HIP device: nothing here is measured on a CPU")
    p, m = Param.test_sweep(), host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    K, N = len(maps), m.qn
    say(f"# tools/clearance_ab.py --reps {args.reps}: {K} maps x {N} agents, dt 0.1")
    search = planner.ecbs_search_batch(ws, list(range(K)), [m] * K, p)
    assert not any(search.status), "a search failed"
    sess = planner.Session.from_ecbs(search, p)
    search.close()
    sess.run()
    grids = [ws[k].download() for k in range(K)]   # (outside the clock: see the docstring)

    def route_a():
        st = sess.download()
        return st, [host.clearance(g, m, pl, 0.1, per_agent=True) for g, pl in zip(grids, sess.plans)]

    def route_b():
        return sess.clearance()

    def route_c():
        return sess.clearance(per_agent=True)

    (sta, ra), (rb, _), (rc, agents) = route_a(), route_b(), route_c()   # warm-up, and the comparison
    same = sta == [0] * K and [r.bits() for r in rb] == [r.bits() for r, _ in ra] == [r.bits() for r in rc]
    same = same and np.array_equal(agents.view(np.uint64), np.stack([a for _, a in ra]).view(np.uint64))
    say(f"K = {K}: segments {min(pl.M for pl in sess.plans)}..{max(pl.M for pl in sess.plans)}, samples {min(r.samples for r in rb)}..{max(r.samples for r in rb)}, "
        f"{sum(r.samples for r in rb) * N} lookups in grids of {grids[0].dist.nbytes / 1e6:.2f} MB; (b) and (c) equal host.clearance of the downloaded plans bit for bit: {same}; "
        f"smallest clearance {min(r.min_clearance for r in rb):.4f} m, hits {sum(r.hits for r in rb)}, outside {sum(r.outside for r in rb)} over all missions")
    ta, tb, tc = [], [], []
    for _ in range(args.reps):
        for ts, fn in ((ta, route_a), (tb, route_b), (tc, route_c)):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
            del r
    a, spa = line(f"a K={K}", ta, f"   {1e3 * statistics.median(ta) / K:.3f} ms per mission")
    b, spb = line(f"b K={K}", tb, f"   {1e6 * statistics.median(tb) / K:.2f} us per mission")
    c, spc = line(f"c K={K}", tc, f"   {1e6 * statistics.median(tc) / K:.2f} us per mission")
    say(f"K = {K}: (a) / (b) = {a / b:.1f}, (a) / (c) = {a / c:.1f};  (a) - (b) = {a - b:.3f} ms, (a) - (c) = {a - c:.3f} ms against the run-to-run "
        f"spreads (max - min) of the three routes, {spa:.3f} / {spb:.3f} / {spc:.3f} ms: the device call is faster by more than both spreads: {a - b > spa and a - b > spb}")
    sess.close()
    ws.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(OUT) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    raise SystemExit(main())
