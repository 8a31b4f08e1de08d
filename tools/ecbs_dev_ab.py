"""A/B of the ECBS front-end on resident worlds: the host search once per map against one device search for all maps
(profiles/ecbs_dev_ab.txt).  One process, host clock around calls that end synchronised, a warm-up of every route, then alternating
repetitions; medians with min / max.

  (a) for each of the 50 maps: planner.ecbs_plan (the mask from the resident grid, then the host search on this machine's CPU)
  (b) one planner.ecbs_plan_batch for the same 50 missions
  (c) the same call with K = 2000: 40 copies of the 50, bench.py's residency
  then one mission alone on either side, and a call with next to no search in it (the fixed cost of a call)

usage: python tools/ecbs_dev_ab.py [--reps 5] [--maps 1-50] [--copies 40]
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


def line(name, ts, extra=""):
    ms = [1e3 * t for t in ts]
    print(f"({name:<10}) median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   ({len(ms)} alternating repetitions){extra}", flush=True)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--copies", type=int, default=40)
    ap.add_argument("--mission", default="mission_64agents_15.json")
    args = ap.parse_args()
    p, m = Param.test_sweep(), host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    W = len(maps)
    budget = 128

    def route_a():
        return [planner.ecbs_plan(ws[n], m, p, budget) for n in range(W)]

    def route_b(copies=1):
        return planner.ecbs_plan_batch(ws, list(range(W)) * copies, [m] * (W * copies), p, max_nodes=budget, max_M=64)

    ref, got, big = route_a(), route_b(), route_b(args.copies)   # warm-up, and the comparison
    same = not got.status.any() and not big.status.any()
    for k in range(W * args.copies):
        r, g = ref[k % W], (got[k] if k < W else big[k])
        same = same and g is not None and np.array_equal(r.init_traj.view(np.uint32), g.init_traj.view(np.uint32)) and np.array_equal(r.T, g.T) \
            and r.ecbs_stats == g.ecbs_stats
    low = sum(r.ecbs_stats["low_level"] for r in ref)
    print(f"# tools/ecbs_dev_ab.py --reps {args.reps}: {W} maps x {m.qn} agents, {low} low-level expansions per {W} maps "
          f"({min(r.ecbs_stats['low_level'] for r in ref)}..{max(r.ecbs_stats['low_level'] for r in ref)} per map), "
          f"high-level expansions {min(r.ecbs_stats['high_level'] for r in ref)}..{max(r.ecbs_stats['high_level'] for r in ref)}")
    print(f"all routes bit-identical, counters included: {same}")
    ta, tb, tc = [], [], []
    for _ in range(args.reps):
        for ts, fn in ((ta, route_a), (tb, route_b), (tc, lambda: route_b(args.copies))):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    a = line("a", ta, f"   {1e3 * statistics.median(ta) / W:.1f} ms per map, {1e6 * statistics.median(ta) / low:.2f} us per low-level expansion")
    b = line("b", tb, f"   {1e6 * statistics.median(tb) / low:.2f} us per low-level expansion of the call")
    c = line(f"c K={W * args.copies}", tc, f"   {1e3 * statistics.median(tc) / (W * args.copies):.3f} ms per mission, "
             f"{1e6 * statistics.median(tc) / (low * args.copies):.3f} us per low-level expansion of the call")
    print(f"(a) / (b) = {a / b:.2f}")
    print(f"(a) x {args.copies} / (c) = {a * args.copies / c:.2f}")
    # one mission alone: the latency of a single wave, hence the kernel's time per expansion when nothing overlaps
    one = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        planner.ecbs_plan_batch(ws, [0], [m], p, max_nodes=budget, max_M=64)
        one.append(time.perf_counter() - t0)
    line("b K=1", one, f"   {1e6 * statistics.median(one) / ref[0].ecbs_stats['low_level']:.2f} us per low-level expansion of one wave "
         f"({ref[0].ecbs_stats['low_level']} expansions, map{maps[0]})")
    alone = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        planner.ecbs_plan(ws[0], m, p, budget)
        alone.append(time.perf_counter() - t0)
    line("a K=1", alone, f"   the host search of the same mission (map{maps[0]})")
    # the fixed cost of a call: one agent two cells from its goal on an empty mask -- the allocations, the clearing of one wave slot, the copies
    tiny = m.subset([0])
    tiny.goal[:] = tiny.start
    tiny.goal[0, 0] += 2 * p.grid_xy_res
    mask = np.zeros(host.ecbs_obstacles(ws[0].download(), tiny, p).shape, np.uint8)
    fixed = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        planner.ecbs_plan_masks([mask], [tiny], p, max_nodes=budget, max_M=64)
        fixed.append(time.perf_counter() - t0)
    line("fixed", fixed[1:], "   one call with next to no search in it")
    ws.close()
    return 0 if same else 1


if __name__ == "__main__":
    raise SystemExit(main())
