"""A/B of a sweep's sampled states, limit peaks and ratio curves: every downloaded plan through host.dynamics against one
Session.dynamics() on the resident plans (profiles/dynamics_ab.txt).  One process, host clock around calls that end synchronised, a warm-up
of every route, then alternating repetitions; medians with min / max.  The session is the hand-off sweep's: worlds, searches and plans made
on the device, then planned once.

  (a) Session.download() followed by host.dynamics with states and curves per mission: what a caller had to do before
  (b) Session.dynamics(states=True, curves=True, device_out=True): report (sizing), three kernels, K small records; the arrays stay in HBM
  (c) Session.dynamics(states=True, curves=True): the same into host arrays, through the bounded staging
  at K = 50 (64 agents x map1..50) and K = 50 x --copies (2000: bench.py's residency)

--only-dynamics: plan, then nothing but three device-output dynamics calls per K -- the run to put under `rocprofv3 --kernel-trace --stats`;
it prints the bytes the state kernel stores per call, for the bandwidth figure.

usage: python tools/dynamics_ab.py [--reps 5] [--reps-large 3] [--maps 1-50] [--copies 40] [--only-dynamics] [--out profiles/dynamics_ab.txt]
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
    ap.add_argument("--reps-large", type=int, default=3, help="repetitions at K = 50 x copies (route (a) takes seconds there)")
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--copies", type=int, default=40)
    ap.add_argument("--mission", default="mission_64agents_15.json")
    ap.add_argument("--only-dynamics", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dynamics_ab.txt"))
    args = ap.parse_args()
    if planner.lib().rbp_device_count() < 1:
        raise SystemExit("tools/dynamics_ab.py: no HIP device: nothing here is measured on a CPU")
    p, m = Param.test_sweep(), host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    trees = [host.load_octomap(f"map{i}.bt") for i in maps]
    ws = planner.DeviceWorlds([t[0] for t in trees], [t[1] for t in trees], p)
    W, N, ok = len(maps), m.qn, True
    say(f"# tools/dynamics_ab.py --reps {args.reps} --reps-large {args.reps_large} --copies {args.copies}: {W} maps x {N} agents, dt 0.1")
    for copies, reps in ((1, args.reps), (args.copies, args.reps_large)):
        K = W * copies
        sess = planned_session(ws, W, copies, m, p)

        def route_a():
            st = sess.download()
            S = max([1] + [host.report(m, p, pl).samples for pl in sess.plans])
            states, curves = np.zeros((K, N, 9, S)), np.zeros((K, S, 2))
            return st, [host.dynamics(m, p, pl, 0.1, states[k], curves[k]) for k, pl in enumerate(sess.plans)], states, curves

        def route_b():
            return sess.dynamics(states=True, curves=True, device_out=True)

        def route_c():
            return sess.dynamics(states=True, curves=True)

        if args.only_dynamics:
            for _ in range(3):
                rec, st, cu = route_b()
            say(f"K = {K}: the state kernel stores {8 * 9 * N * sum(r.samples for r in rec)} bytes per call, the curve kernel {16 * sum(r.samples for r in rec)}; "
                f"rows of {st.shape[3]} samples")
            sess.close()
            continue
        (sta, ra, sa_, ca_), (rb, sb_, cb_), (rc, sc_, cc_) = route_a(), route_b(), route_c()   # warm-up, and the comparison
        same = sta == [0] * K and [r.bits() for r in rb] == [r.bits() for r in ra] == [r.bits() for r in rc]
        same = same and np.array_equal(sc_.view(np.uint64), sa_.view(np.uint64)) and np.array_equal(cc_.view(np.uint64), ca_.view(np.uint64))
        n = min(K, 50)   # (the device arrays of the first 50 missions come down for the comparison; all of (c)'s were compared above)
        same = same and np.array_equal(sb_[:n].cpu().numpy().view(np.uint64), sa_[:n].view(np.uint64)) and np.array_equal(cb_[:n].cpu().numpy().view(np.uint64), ca_[:n].view(np.uint64))
        ok = ok and same
        say(f"K = {K}: segments {min(pl.M for pl in sess.plans)}..{max(pl.M for pl in sess.plans)}, samples {min(r.samples for r in rb)}..{max(r.samples for r in rb)}, "
            f"states {sa_.nbytes / 1e6:.1f} MB, curves {ca_.nbytes / 1e6:.2f} MB; (b) and (c) equal host.dynamics of the downloaded plans bit for bit: {same}; "
            f"peak velocity ratio {max(r.peak_vel_ratio for r in rb):.4f}, peak acceleration ratio {max(r.peak_acc_ratio for r in rb):.4f} over all missions")
        del sa_, ca_, sb_, cb_, sc_, cc_
        ta, tb, tc = [], [], []
        for _ in range(reps):
            for ts, fn in ((ta, route_a), (tb, route_b), (tc, route_c)):
                t0 = time.perf_counter()
                r = fn()
                ts.append(time.perf_counter() - t0)
                del r
        a, spa = line(f"a K={K}", ta, f"   {1e3 * statistics.median(ta) / K:.3f} ms per mission")
        b, spb = line(f"b K={K}", tb, f"   {1e6 * statistics.median(tb) / K:.2f} us per mission")
        c, spc = line(f"c K={K}", tc, f"   {1e6 * statistics.median(tc) / K:.2f} us per mission")
        say(f"K = {K}: (a) / (b) = {a / b:.1f}, (a) / (c) = {a / c:.1f};  (a) - (b) = {a - b:.3f} ms, (a) - (c) = {a - c:.3f} ms against the largest run-to-run "
            f"spread (max - min) of the three routes, {max(spa, spb, spc):.3f} ms")
        sess.close()
    ws.close()
    if not args.only_dynamics:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
