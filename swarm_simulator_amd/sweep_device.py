"""The map sweep of swarm_simulator_amd.test_all (swarm_traj_planner_rbp_test_all.cpp:49-103) on worlds that stay on the device.

With --device-worlds the distance grids of all maps are built on the GPU in one call and stay there (planner.DeviceWorlds): the ECBS
front-end gets its obstacle mask from the resident grid (planner.ecbs_plan) and both modes plan on it, with the report lines of test_all.
Without the flag this is test_all itself, argument for argument.
With --device-ecbs (only with --device-worlds) the searches of all maps run on the GPU too, in one call (planner.ecbs_plan_batch): the same
initial trajectories, and one report line for the whole front-end instead of one per map.
With --device-handoff (only with --device-ecbs and --mode batched) the searches' plans never come to the host: the session is built from
them where they lie (planner.ecbs_search_batch, planner.Session.from_ecbs).  The same report lines.

usage: python -m swarm_simulator_amd.sweep_device [--device-worlds [--device-ecbs [--device-handoff]]] [--mission mission_64agents_15.json] [--maps 1-50] [--mode batched]
       [--batch-size 4] [--iteration 1] [--joint] [--csv DIR]
"""
import argparse
import time

from . import host, planner, test_all
from .types import Param


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device-worlds", action="store_true", help="build all distance grids on the GPU in one call and keep them there")
    ap.add_argument("--device-ecbs", action="store_true", help="with --device-worlds: the ECBS searches of all maps in one call on the GPU, within the device search's capacities "
                    "(512 high-level expansions where the host search allows 200000, paths of at most 62 steps): a map beyond them ends the sweep "
                    "with an error where the host search would go on")
    ap.add_argument("--device-handoff", action="store_true", help="with --device-worlds --device-ecbs --mode batched: the session is built on the device from the "
                    "search's resident results, no initial trajectory passes through the host")
    ap.add_argument("--mission", default="mission_64agents_15.json")
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--mode", choices=["serial", "batched"], default="serial")
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--iteration", type=int, default=1)
    ap.add_argument("--joint", action="store_true")
    ap.add_argument("--csv", default=None, help="write coef<qi>.csv per map into DIR/map<i>/ (generateCoefCSV)")
    args, rest = ap.parse_known_args(argv)
    if args.device_ecbs and not args.device_worlds:
        ap.error("--device-ecbs needs --device-worlds")
    if args.device_handoff and not (args.device_ecbs and args.mode == "batched"):
        ap.error("--device-handoff needs --device-worlds --device-ecbs --mode batched")
    if not args.device_worlds:
        return test_all.main(argv)
    if rest:
        ap.error("unrecognized arguments: " + " ".join(rest))

    param = Param.test_sweep(batch_size=args.batch_size, iteration=args.iteration, sequential=not args.joint)
    mission = host.load_mission(args.mission)
    maps = test_all.parse_maps(args.maps)
    t0 = time.perf_counter()
    octrees = [host.load_octomap(f"map{i}.bt") for i in maps]
    worlds = planner.DeviceWorlds([o[0] for o in octrees], [o[1] for o in octrees], param)
    print(f"Euclidean Distmap runtime, {len(maps)} maps in one device build: {time.perf_counter() - t0:.6f}")
    try:
        plans, inits = [], None
        if args.device_handoff:
            return handoff_sweep(args, worlds, maps, mission, param)
        if args.device_ecbs:
            t0 = time.perf_counter()
            inits = planner.ecbs_plan_batch(worlds, list(range(len(maps))), [mission] * len(maps), param)
            print(f"Initial Trajectory Planner runtime, {len(maps)} maps in one device search: {time.perf_counter() - t0:.6f}")
            for i, st in zip(maps, inits.status):
                if st:  # (3: a capacity of the device search; the host search is the caller's choice, not a fallback)
                    print(f"[ERROR] map{i}: {host.ECBS_ERROR_TEXT.get(int(st), 'ECBSPlanner: device search capacity exceeded (status 3)')}")
                    return -1
        for n, i in enumerate(maps):
            print(f"Map: map{i}.bt")
            w = worlds[n]
            if inits is not None:
                pr = inits[n]
            else:
                t0 = time.perf_counter()
                try:
                    pr = planner.ecbs_plan(w, mission, param)
                except RuntimeError as e:
                    print(f"[ERROR] {e}")
                    return -1
                print(f"Initial Trajectory Planner runtime: {time.perf_counter() - t0:.6f}")
            if args.mode == "serial":
                t0 = time.perf_counter()
                cor = planner.Corridor(w, mission, param)
                if not cor.update(param.log, pr):
                    print(f"[ERROR] {cor.last_error}")
                    return -1
                print(f"BoxGenerator runtime: {time.perf_counter() - t0:.6f}")
                t0 = time.perf_counter()
                pl = planner.RBPPlanner(mission, param)
                if not pl.update(param.log, pr):
                    print(f"[ERROR] {pl.last_error}")
                    return -1
                print(f"SwarmPlanner runtime: {time.perf_counter() - t0:.6f}")
                test_all.report(i, mission, param, pr, args.csv)
            plans.append(pr)
        if args.mode == "batched":
            sess = planner.Session([worlds[n] for n in range(len(maps))], [mission] * len(plans), param, plans)
            t0 = time.perf_counter()
            sess.run()
            status = sess.download()
            dt = time.perf_counter() - t0
            print(f"BoxGenerator + SwarmPlanner runtime, {len(plans)} maps in one session: {dt:.6f} "
                  f"({len(plans) * mission.qn / dt:.1f} agent-trajectories/s incl. download)")
            sess.close()
            for i, p, st in zip(maps, plans, status):
                if st:
                    print(f"[ERROR] map{i}: status {st}")
                    return -1
                test_all.report(i, mission, param, p, args.csv)
        return 0
    finally:
        worlds.close()


def handoff_sweep(args, worlds, maps, mission, param):
    """--device-handoff: search, session and plan without an initial trajectory on the host; the report lines of the batched mode"""
    t0 = time.perf_counter()
    search = planner.ecbs_search_batch(worlds, list(range(len(maps))), [mission] * len(maps), param)
    print(f"Initial Trajectory Planner runtime, {len(maps)} maps in one device search: {time.perf_counter() - t0:.6f}")
    for i, st in zip(maps, search.status):
        if st:  # (3: a capacity of the device search; the host search is the caller's choice, not a fallback)
            print(f"[ERROR] map{i}: {host.ECBS_ERROR_TEXT.get(int(st), 'ECBSPlanner: device search capacity exceeded (status 3)')}")
            search.close()
            return -1
    for i in maps:
        print(f"Map: map{i}.bt")
    sess = planner.Session.from_ecbs(search, param)
    search.close()
    t0 = time.perf_counter()
    sess.run()
    status = sess.download()
    dt = time.perf_counter() - t0
    print(f"BoxGenerator + SwarmPlanner runtime, {sess.K} maps in one session: {dt:.6f} "
          f"({sess.K * mission.qn / dt:.1f} agent-trajectories/s incl. download)")
    sess.close()
    for i, p, st in zip(maps, sess.plans, status):
        if st:
            print(f"[ERROR] map{i}: status {st}")
            return -1
        test_all.report(i, mission, param, p, args.csv)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
