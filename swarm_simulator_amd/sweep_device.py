"""The map sweep of swarm_simulator_amd.test_all (swarm_traj_planner_rbp_test_all.cpp:49-103) on worlds that stay on the device.

With --device-worlds the distance grids of all maps are built on the GPU in one call and stay there (planner.DeviceWorlds): the ECBS
front-end gets its obstacle mask from the resident grid (planner.ecbs_plan) and both modes plan on it, with the report lines of test_all.
Without the flag this is test_all itself, argument for argument.
With --device-ecbs (only with --device-worlds) the searches of all maps run on the GPU too, in one call (planner.ecbs_plan_batch): the same
initial trajectories, and one report line for the whole front-end instead of one per map.
With --device-handoff (only with --device-ecbs and --mode batched) the searches' plans never come to the host: the session is built from
them where they lie (planner.ecbs_search_batch, planner.Session.from_ecbs).  The same report lines.
With --stream B (only with --device-handoff) the maps go through ONE reserved session in batches of B (planner.Session.reserved with room for
B missions, planner.Session.refill per batch): search, refill, run, report lines, batch after batch, as a planning service would, with no
session built or released in between.  The same per-map lines in map order for any B.
With --stream-plans B (only with --device-worlds --mode batched, not with --device-handoff) the same service for a caller whose plans are on
the HOST: per batch of B maps the initial trajectories come from the host search, or with --device-ecbs from that batch's downloaded device
search, and are loaded into ONE reserved session with planner.Session.refill_plans (packed staging, one copy and one kernel per round).
The same per-map lines in map order for any B.
With --device-report (only with --device-worlds --mode batched) the safety ratio and flight distance of every map's report line come from ONE
planner.Session.report() on the resident plans instead of host.validate per downloaded plan: the same line format, the numbers of the
rule the device and host.report share (csrc/common/report_rules.h; they differ from host.validate's by rounding).  Without --csv nothing
but K small records and two scalars per map is downloaded.
With --device-dynamics (only with --device-worlds --mode batched; off by default) ONE planner.Session.dynamics() on the resident plans adds a
line per map with the largest |velocity| / max_vel and |acceleration| / max_acc over all samples, agents and axes and where they lie
(csrc/common/state_rules.h): whether the plan respects its limits at the samples, the reference's third acceptance signal.
With --device-clearance (only with --device-worlds --mode batched; off by default) ONE planner.Session.clearance() on the resident plans and
grids adds a line per map with the smallest clearance to the obstacles, where it lies, and how many (sample, agent) items hit an obstacle
or left the grid (csrc/common/clearance_rules.h): whether the plan hits anything.
With --device-separation (only with --device-worlds --mode batched; off by default) ONE planner.Session.separation() on the resident plans
adds a line per map with a certified interval for the smallest safety ratio in CONTINUOUS time, where both ends lie, and how many (pair,
segment) items are uncertified, colliding and refined (csrc/common/separation_rules.h): whether the plan is separated between the samples.
With --device-swept-clearance (only with --device-worlds --mode batched; off by default) ONE planner.Session.swept_clearance() on the resident
plans and grids adds a line per map with a certified interval for the smallest clearance to the obstacles in CONTINUOUS time, where both
ends lie, and how many (agent, segment) items are uncertified, hitting, outside, over budget and refined (csrc/common/swept_rules.h):
whether the plan is clear of the obstacles between the samples.
With --device-limits (only with --device-worlds --mode batched; off by default) ONE planner.Session.limits() on the resident plans adds a
line per map with certified intervals for the largest velocity and acceleration, as fractions of the agents' limits, in CONTINUOUS time,
and how many (agent, segment) items are uncertified, violating and refined (csrc/common/limits_rules.h): whether the plan keeps max_vel and
max_acc between the samples.

usage: python -m swarm_simulator_amd.sweep_device [--device-worlds [--device-ecbs [--device-handoff [--stream B]]] [--stream-plans B] [--device-report] [--device-dynamics] [--device-clearance] [--device-separation] [--device-swept-clearance] [--device-limits]] [--mission mission_64agents_15.json] [--maps 1-50] [--mode batched]
       [--batch-size 4] [--iteration 1] [--joint] [--csv DIR]
"""
import argparse
import time
from types import SimpleNamespace

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
    ap.add_argument("--stream", type=int, default=0, metavar="B", help="with --device-handoff: the maps go through one reserved session in batches of B "
                    "(planner.Session.reserved, planner.Session.refill), nothing is allocated between the batches")
    ap.add_argument("--stream-plans", type=int, default=0, metavar="B", help="with --device-worlds --mode batched, without --device-handoff: the maps go "
                    "through one reserved session in batches of B whose host plans are loaded with planner.Session.refill_plans")
    ap.add_argument("--device-report", action="store_true", help="with --device-worlds --mode batched: safety ratio and flight distance of all maps from one "
                    "report call on the device (planner.Session.report); without --csv the coefficients are not downloaded")
    ap.add_argument("--device-dynamics", action="store_true", help="with --device-worlds --mode batched: one more line per map with both limit peak ratios and "
                    "where they lie, from one dynamics call on the device (planner.Session.dynamics)")
    ap.add_argument("--device-clearance", action="store_true", help="with --device-worlds --mode batched: one more line per map with the smallest clearance "
                    "to the obstacles, where it lies, hits and outsides, from one clearance call on the device (planner.Session.clearance)")
    ap.add_argument("--device-separation", action="store_true", help="with --device-worlds --mode batched: one more line per map with a certified interval "
                    "for the smallest safety ratio in continuous time, where it lies, uncertified / colliding / refined items, from one separation "
                    "call on the device (planner.Session.separation)")
    ap.add_argument("--device-swept-clearance", action="store_true", help="with --device-worlds --mode batched: one more line per map with a certified "
                    "interval for the smallest clearance to the obstacles in continuous time, where it lies, uncertified / hitting / outside / "
                    "over-budget / refined items, from one swept clearance call on the device (planner.Session.swept_clearance)")
    ap.add_argument("--device-limits", action="store_true", help="with --device-worlds --mode batched: one more line per map with certified intervals "
                    "for the largest velocity and acceleration ratios in continuous time, uncertified / violating / refined items, from one "
                    "limits call on the device (planner.Session.limits)")
    ap.add_argument("--mission", default="mission_64agents_15.json")
    ap.add_argument("--maps", default="1-50")
    ap.add_argument("--mode", choices=["serial", "batched"], default="serial")
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--iteration", type=int, default=1)
    ap.add_argument("--joint", action="store_true")
    ap.add_argument("--csv", default=None, help="write coef<qi>.csv per map into DIR/map<i>/ (generateCoefCSV)")
    args, rest = ap.parse_known_args(argv)
    if args.device_report and not (args.device_worlds and args.mode == "batched"):
        ap.error("--device-report needs --device-worlds --mode batched")
    if args.device_dynamics and not (args.device_worlds and args.mode == "batched"):
        ap.error("--device-dynamics needs --device-worlds --mode batched")
    if args.device_clearance and not (args.device_worlds and args.mode == "batched"):
        ap.error("--device-clearance needs --device-worlds --mode batched")
    if args.device_separation and not (args.device_worlds and args.mode == "batched"):
        ap.error("--device-separation needs --device-worlds --mode batched")
    if args.device_swept_clearance and not (args.device_worlds and args.mode == "batched"):
        ap.error("--device-swept-clearance needs --device-worlds --mode batched")
    if args.device_limits and not (args.device_worlds and args.mode == "batched"):
        ap.error("--device-limits needs --device-worlds --mode batched")
    if args.device_ecbs and not args.device_worlds:
        ap.error("--device-ecbs needs --device-worlds")
    if args.device_handoff and not (args.device_ecbs and args.mode == "batched"):
        ap.error("--device-handoff needs --device-worlds --device-ecbs --mode batched")
    if args.stream and not args.device_handoff:
        ap.error("--stream needs --device-worlds --device-ecbs --device-handoff --mode batched")
    if args.stream < 0:
        ap.error("--stream takes a positive batch size")
    if args.stream_plans < 0:
        ap.error("--stream-plans takes a positive batch size")
    if args.stream_plans and not (args.device_worlds and args.mode == "batched") or args.stream_plans and args.device_handoff:
        ap.error("--stream-plans needs --device-worlds --mode batched and excludes --device-handoff (whose plans never reach the host: --stream)")
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
        if args.stream_plans:
            return stream_plans_sweep(args, worlds, maps, mission, param)
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
            return run_and_report(args, sess, maps, plans, mission, param)
        return 0
    finally:
        worlds.close()


def handoff_sweep(args, worlds, maps, mission, param):
    """--device-handoff: search, session and plan without an initial trajectory on the host; the report lines of the batched mode"""
    if args.stream:
        return stream_sweep(args, worlds, maps, mission, param)
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
    return run_and_report(args, sess, maps, sess.plans, mission, param)


def stream_sweep(args, worlds, maps, mission, param):
    """--stream B: one reserved session with room for B missions; per batch of B maps a search, a refill, a run and the report lines"""
    B, sess = args.stream, None
    try:
        for b0 in range(0, len(maps), B):
            batch = maps[b0:b0 + B]
            t0 = time.perf_counter()
            search = planner.ecbs_search_batch(worlds, list(range(b0, b0 + len(batch))), [mission] * len(batch), param)
            try:
                print(f"Initial Trajectory Planner runtime, {len(batch)} maps in one device search: {time.perf_counter() - t0:.6f}")
                for i, st in zip(batch, search.status):
                    if st:  # (3: a capacity of the device search; the host search is the caller's choice, not a fallback)
                        print(f"[ERROR] map{i}: {host.ECBS_ERROR_TEXT.get(int(st), 'ECBSPlanner: device search capacity exceeded (status 3)')}")
                        return -1
                for i in batch:
                    print(f"Map: map{i}.bt")
                if sess is None:
                    sess = planner.Session.reserved(worlds, B, mission.qn, search.max_M, search.max_M, param)
                sess.refill(search)
                rc = run_and_report(args, sess, batch, sess.plans, mission, param, close=False)   # (ends synchronised: the search may go)
            finally:
                search.close()
            if rc:
                return rc
        return 0
    finally:
        if sess is not None:
            sess.close()


STREAM_PLANS_MAX_M = 64   # segments a slot of --stream-plans' session has room for: the device search's capacity (planner.ecbs_plan_batch)


def stream_plans_sweep(args, worlds, maps, mission, param):
    """--stream-plans B: one reserved session with room for B missions; per batch of B maps the host plans of a search, a refill_plans, a
    run and the report lines"""
    B = args.stream_plans
    sess = planner.Session.reserved(worlds, B, mission.qn, STREAM_PLANS_MAX_M, STREAM_PLANS_MAX_M, param)
    try:
        for b0 in range(0, len(maps), B):
            batch, idx = maps[b0:b0 + B], list(range(b0, min(b0 + B, len(maps))))
            if args.device_ecbs:
                t0 = time.perf_counter()
                plans = planner.ecbs_plan_batch(worlds, idx, [mission] * len(batch), param, max_M=STREAM_PLANS_MAX_M)
                print(f"Initial Trajectory Planner runtime, {len(batch)} maps in one device search: {time.perf_counter() - t0:.6f}")
                for i, st in zip(batch, plans.status):
                    if st:  # (3: a capacity of the device search; the host search is the caller's choice, not a fallback)
                        print(f"[ERROR] map{i}: {host.ECBS_ERROR_TEXT.get(int(st), 'ECBSPlanner: device search capacity exceeded (status 3)')}")
                        return -1
                plans = list(plans)
                for i in batch:
                    print(f"Map: map{i}.bt")
            else:
                plans = []
                for n, i in zip(idx, batch):
                    print(f"Map: map{i}.bt")
                    t0 = time.perf_counter()
                    try:
                        plans.append(planner.ecbs_plan(worlds[n], mission, param))
                    except RuntimeError as e:
                        print(f"[ERROR] {e}")
                        return -1
                    print(f"Initial Trajectory Planner runtime: {time.perf_counter() - t0:.6f}")
            try:
                sess.refill_plans([worlds[n] for n in idx], [mission] * len(batch), plans)
            except ValueError as e:   # (a plan beyond the session's strides)
                print(f"[ERROR] {e}")
                return -1
            rc = run_and_report(args, sess, batch, plans, mission, param, close=False)
            if rc:
                return rc
        return 0
    finally:
        sess.close()


def run_and_report(args, sess, maps, plans, mission, param, close=True):
    """the batched mode's run of a session and its report lines.  --device-report: the lines' two signals come from one Session.report(),
    and without --csv each line's cost, time scale and makespan from the session's scalars and that record instead of a download.
    close=False: the session is the caller's to refill."""
    download = not args.device_report or bool(args.csv)
    t0 = time.perf_counter()
    sess.run()
    status = sess.download() if download else None
    records = sess.report() if args.device_report else [None] * sess.K
    peaks = sess.dynamics()[0] if args.device_dynamics else [None] * sess.K
    clear = sess.clearance()[0] if args.device_clearance else [None] * sess.K
    separ = sess.separation()[0] if args.device_separation else [None] * sess.K
    swept = sess.swept_clearance()[0] if args.device_swept_clearance else [None] * sess.K
    limit = sess.limits()[0] if args.device_limits else [None] * sess.K
    dt = time.perf_counter() - t0
    print(f"BoxGenerator + SwarmPlanner runtime, {sess.K} maps in one session: {dt:.6f} "
          f"({sess.K * mission.qn / dt:.1f} agent-trajectories/s incl. {'download' if download else 'report'})")
    if not download:
        sc = sess.scalars(n=2)   # (kernels/rbp_dev.h: SC_TIME_SCALE, SC_TOTAL_COST -- read as rbp_session_download reads them)
        status = [r.status for r in records]
        plans = [SimpleNamespace(total_cost=float(c), time_scale=float(ts) if ts > 0 else 1.0, T=[r.end_time]) for (ts, c), r in zip(sc, records)]
    if close:
        sess.close()
    for i, p, st, rec, pk, cl, sp, sw, lm in zip(maps, plans, status, records, peaks, clear, separ, swept, limit):
        if st:
            print(f"[ERROR] map{i}: status {st}")
            return -1
        if rec is None:
            test_all.report(i, mission, param, p, args.csv)
        else:
            report_line(i, p, rec, args.csv)
        if pk is not None:
            dynamics_line(i, pk)
        if cl is not None:
            clearance_line(i, cl)
        if sp is not None:
            separation_line(i, sp)
        if sw is not None:
            swept_clearance_line(i, sw)
        if lm is not None:
            limits_line(i, lm)
    return 0


def limits_line(i, s):
    """--device-limits: the two intervals of a types.Limits, where their upper ends lie (agent, axis, segment, piece of depth), and the item
    counts; `none` for an end that no piece gave"""
    def where(ratio, agent, axis, segment, piece, depth):
        return f"{ratio:.5f} (agent {agent} axis {axis} segment {segment} piece {piece}/{1 << depth})" if segment >= 0 else "none"
    print(f"map{i}: continuous velocity ratio in [{s.lower_vel_ratio:.5f}, "
          f"{where(s.upper_vel_ratio, s.upper_vel_agent, s.upper_vel_axis, s.upper_vel_segment, s.upper_vel_piece, s.upper_vel_depth)}]  "
          f"acceleration ratio in [{s.lower_acc_ratio:.5f}, "
          f"{where(s.upper_acc_ratio, s.upper_acc_agent, s.upper_acc_axis, s.upper_acc_segment, s.upper_acc_piece, s.upper_acc_depth)}]  "
          f"uncertified {s.uncertified}  violating {s.violating}  refined {s.refined}")


def swept_clearance_line(i, s):
    """--device-swept-clearance: both ends of a types.SweptClearance's interval and where they lie (agent, segment, piece of depth), and the
    item counts; `none` for an end that no piece gave"""
    def where(clearance, agent, segment, piece, depth):
        return f"{clearance:.5f} (agent {agent} segment {segment} piece {piece}/{1 << depth})" if segment >= 0 else "none"
    print(f"map{i}: continuous clearance in [{where(s.lower_clearance, s.lower_agent, s.lower_segment, s.lower_piece, s.lower_depth)}, "
          f"{where(s.upper_clearance, s.upper_agent, s.upper_segment, s.upper_piece, s.upper_depth)}]  "
          f"uncertified {s.uncertified}  hitting {s.hitting}  outside {s.outside}  over budget {s.over_budget}  refined {s.refined}")


def separation_line(i, s):
    """--device-separation: both ends of a types.Separation's interval and where they lie (pair, segment, piece of depth), and the item
    counts; `none` for a plan without a pair"""
    def where(ratio, qi, qj, segment, piece, depth):
        return f"{ratio:.5f} (agents {qi} {qj} segment {segment} piece {piece}/{1 << depth})" if segment >= 0 else "none"
    print(f"map{i}: continuous safety ratio in [{where(s.lower_ratio, s.lower_qi, s.lower_qj, s.lower_segment, s.lower_piece, s.lower_depth)}, "
          f"{where(s.upper_ratio, s.upper_qi, s.upper_qj, s.upper_segment, s.upper_piece, s.upper_depth)}]  "
          f"uncertified {s.uncertified}  colliding {s.colliding}  refined {s.refined}")


def clearance_line(i, c):
    """--device-clearance: the smallest clearance of a types.Clearance and where it lies (agent, sample), hits and outsides; `none` for a plan without a sample"""
    where = f"{c.min_clearance:.4f} (agent {c.min_agent} sample {c.min_sample})" if c.min_sample >= 0 else "none"
    print(f"map{i}: minimum clearance {where}  hits {c.hits}  outside {c.outside}  samples {c.samples}")


def dynamics_line(i, d):
    """--device-dynamics: both limit peak ratios of a types.Dynamics and where they lie (agent, axis, sample); `none` for a plan without one"""
    def where(ratio, agent, axis, sample):
        return f"{ratio:.4f} (agent {agent} {'xyz'[axis]} sample {sample})" if sample >= 0 else "none"
    print(f"map{i}: peak velocity ratio {where(d.peak_vel_ratio, d.vel_agent, d.vel_axis, d.vel_sample)}  "
          f"peak acceleration ratio {where(d.peak_acc_ratio, d.acc_agent, d.acc_axis, d.acc_sample)}  samples {d.samples}")


def report_line(i, plan, record, csv_dir):
    """test_all.report's line, format and all, with the two signals of a types.Report computed on the device (planner.Session.report)
    where test_all.report calls host.validate; `plan` only has to carry total_cost, time_scale and T[-1] (and coef for a CSV)"""
    print(f"map{i}: QP total cost {plan.total_cost:.6f}  time_scale {plan.time_scale:.4f}  makespan {plan.T[-1]:.3f}  "
          f"safety margin ratio {record.min_safety_ratio:.4f}  total flight distance {record.total_flight_distance:.3f}")
    if csv_dir:
        import os
        host.write_coef_csv(os.path.join(csv_dir, f"map{i}"), plan)


if __name__ == "__main__":
    raise SystemExit(main())
