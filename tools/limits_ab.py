"""A/B of a sweep's certified velocity and acceleration limits in continuous time: every downloaded plan through host.limits against one
Session.limits() on the resident plans (profiles/limits_ab.txt).  One process, host clock around calls that end synchronised, a warm-up of
every route, then alternating repetitions; medians with min / max.  The session is the hand-off sweep's: worlds, searches and plans made on
the device, then planned once.

  (a) Session.download() followed by host.limits per mission, depth 4, everything refined: what a caller had to do before
  (b) Session.limits(depth=4, refine_above=-1): every item through the work list, 16 pieces of each of its six polynomials
  (c) as (b) with every agent's upper ratios into a host array, through the staging buffer
  (d) as (a) at the defaults (refine_above 0.5)
  (e) as (b) at the defaults: the coarse kernel over every item, the refine kernel over the listed ones

No speed is required of this call; the numbers are the record.  With them comes the finding the call exists to make: per map the width
upper - lower of both intervals at depths 0, 4 and 8 (everything refined), how many maps come out with uncertified == 0 under each
rbp_param.timescale_rule, and, where the two rules' factors differ (time_scale != time_scale_alt), whether lower_vel_ratio > 1 under the
literal rule 1.

usage: python tools/limits_ab.py [--reps 7] [--maps 1-50] [--out profiles/limits_ab.txt]
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


def planned(ws, K, m, p):
    search = planner.ecbs_search_batch(ws, list(range(K)), [m] * K, p)
    assert not any(search.status), "a search failed"
    sess = planner.Session.from_ecbs(search, p)
    search.close()
    sess.run()
    return sess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--mission", default="mission_64agents_15.json")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "limits_ab.txt"))
    args = ap.parse_args()
    if planner.lib().rbp_device_count() < 1:
        raise SystemExit("tools/limits_ab.py: no HIP device: nothing here is measured on a CPU")
    m = host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], Param.test_sweep())
    K, N, D = len(maps), m.qn, args.depth
    say(f"# tools/limits_ab.py --reps {args.reps}: {K} maps x {N} agents, depth {D}")
    sess = planned(ws, K, m, Param.test_sweep())

    def on_host(above):
        def route():
            st = sess.download()
            return st, [host.limits(m, pl, D, above, per_agent=True) for pl in sess.plans]
        return route

    routes = [("a", on_host(-1.0)), ("b", lambda: sess.limits(D, -1.0)), ("c", lambda: sess.limits(D, -1.0, per_agent=True)),
              ("d", on_host(0.5)), ("e", lambda: sess.limits(D, 0.5))]
    (sta, ra), (rb, _), (rc, agents), (std, rd), (re_, _) = [fn() for _, fn in routes]   # warm-up, and the comparison
    same = sta == std == [0] * K and [r.bits() for r in rb] == [r.bits() for r, _ in ra] == [r.bits() for r in rc]
    same = same and [r.bits() for r in re_] == [r.bits() for r, _ in rd]
    same = same and np.array_equal(agents.view(np.uint64), np.stack([a for _, a in ra]).view(np.uint64))
    items = sum(N * pl.M for pl in sess.plans)
    say(f"K = {K}: segments {min(pl.M for pl in sess.plans)}..{max(pl.M for pl in sess.plans)}, {items} (agent, segment) items, {sum(r.refined for r in re_)} of them "
        f"refined at refine_above 0.5 ({100.0 * sum(r.refined for r in re_) / items:.2f} %), {sum(r.refined for r in rb)} at -1; (b), (c), (e) equal "
        f"host.limits of the downloaded plans bit for bit: {same}")

    # ---- tightness and what is certified, rule 0 -----------------------------------------------------------------------------------
    by_depth = {d: sess.limits(d, -1.0)[0] for d in (0, 4, 8)}
    sampled = sess.dynamics(0.1)[0]
    say(f"K = {K}, timescale_rule 0: maps with uncertified == 0 at depth 0 / 4 / 8 (everything refined): "
        + " / ".join(str(sum(r.uncertified == 0 for r in by_depth[d])) for d in (0, 4, 8))
        + f"; at the defaults {sum(r.uncertified == 0 for r in re_)}; maps with violating > 0 at depth 8: {sum(r.violating > 0 for r in by_depth[8])}; "
        f"uncertified items at depth 8: {sum(r.uncertified for r in by_depth[8])} of {items}")
    say(f"K = {K}, timescale_rule 0: largest upper vel / acc ratio at depth 8 {max(r.upper_vel_ratio for r in by_depth[8])!r} / {max(r.upper_acc_ratio for r in by_depth[8])!r}; "
        f"largest sampled at dt 0.1 {max(s.peak_vel_ratio for s in sampled)!r} / {max(s.peak_acc_ratio for s in sampled)!r}")
    say("per map, upper - lower of the velocity interval at depth 0, 4, 8 | of the acceleration interval | [lower, upper] vel at depth 8 | acc at depth 8 | time scale")
    for k, i in enumerate(maps):
        wv = " ".join(f"{by_depth[d][k].upper_vel_ratio - by_depth[d][k].lower_vel_ratio:.3e}" for d in (0, 4, 8))
        wa = " ".join(f"{by_depth[d][k].upper_acc_ratio - by_depth[d][k].lower_acc_ratio:.3e}" for d in (0, 4, 8))
        r = by_depth[8][k]
        say(f"  map{i}: {wv} | {wa} | [{r.lower_vel_ratio:.6f}, {r.upper_vel_ratio:.6f}] | [{r.lower_acc_ratio:.6f}, {r.upper_acc_ratio:.6f}] | {sess.plans[k].time_scale:.6f}")

    # ---- the timings ---------------------------------------------------------------------------------------------------------------
    times = {name: [] for name, _ in routes}
    for _ in range(args.reps):
        for name, fn in routes:
            t0 = time.perf_counter()
            r = fn()
            times[name].append(time.perf_counter() - t0)
            del r
    med = {name: line(f"{name} K={K}", times[name], f"   {1e3 * statistics.median(times[name]) / K:.3f} ms per mission") for name, _ in routes}
    for host_route, dev_route, what in (("a", "b", "everything refined"), ("a", "c", "everything refined, agents to the host"), ("d", "e", "refine_above 0.5")):
        (a, spa), (b, spb) = med[host_route], med[dev_route]
        say(f"K = {K}, {what}: ({host_route}) / ({dev_route}) = {a / b:.1f};  ({host_route}) - ({dev_route}) = {a - b:.3f} ms against the run-to-run spreads "
            f"(max - min) {spa:.3f} / {spb:.3f} ms: the device call is faster by more than both spreads: {a - b > spa and a - b > spb}")
    sess.close()

    # ---- the literal rule ----------------------------------------------------------------------------------------------------------
    sess1 = planned(ws, K, m, Param.test_sweep(timescale_rule=1))
    r1 = sess1.limits(8, -1.0)[0]
    st1 = sess1.download()
    differ = [k for k, pl in enumerate(sess1.plans) if pl.time_scale != pl.time_scale_alt]
    say(f"K = {K}, timescale_rule 1: status all 0: {st1 == [0] * K}; maps with uncertified == 0 at depth 8: {sum(r.uncertified == 0 for r in r1)}; maps with violating > 0: "
        f"{sum(r.violating > 0 for r in r1)}; the two rules' factors differ on {len(differ)} maps")
    for k in differ:
        r, pl = r1[k], sess1.plans[k]
        say(f"  map{maps[k]}: time_scale {pl.time_scale:.6f} (rule 1) against {pl.time_scale_alt:.6f}; vel [{r.lower_vel_ratio:.6f}, {r.upper_vel_ratio:.6f}] "
            f"acc [{r.lower_acc_ratio:.6f}, {r.upper_acc_ratio:.6f}]; lower_vel_ratio > 1: {r.lower_vel_ratio > 1}; violating {r.violating}")
    sess1.close()
    ws.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(OUT) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    raise SystemExit(main())
