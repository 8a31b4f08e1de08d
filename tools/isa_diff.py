#!/usr/bin/env python3
"""Developer tool (no GPU needed): is the gfx950 device code of two source trees the same, function by function?

usage: tools/isa_diff.py <tree A> <tree B> [--jobs N] [--b-flags "-DLEVER=0"] > profiles/<tag>_isa.txt        (exit status 1 when anything differs)
--b-flags: extra compiler flags for tree B only -- a lever that B adds, switched off, must give A's device code.

Cross-compiles every kernels/*.hip of both trees to assembly (hipcc --cuda-device-only -S) under the flag sets of csrc/Makefile -- qp.hip
once per build of it, everything else with the plain flags --, cuts the output into functions (`.type NAME,@function` .. `.Lfunc_end`, plus
a kernel's `.amdhsa_kernel` descriptor: registers, LDS, scratch), strips comments and whitespace, renumbers the local labels in order of
appearance, and compares the TEXT per function name.  A refactor that must not touch the device code is checked before anything runs on a card.
"""
import argparse, concurrent.futures, glob, os, re, subprocess, sys

BASE = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S -o -".split()
W2, W4 = "-DQP_WAVES_PER_EU=2 -DQP_ROW_PF=4 -DQP_SUFFIX=_w2".split(), "-DQP_THREADS=256 -DQP_WAVES_PER_EU=2 -DQP_SUFFIX=_w4".split()
QP_VARIANTS = {"_w2": W2, "_w4": W4, "prof _w2": ["-DQP_PROFILE"] + W2, "prof _w4": ["-DQP_PROFILE"] + W4}
LOCAL = re.compile(r"\.(LBB|Ltmp|LJTI|Lfunc_begin|Lfunc_end)[0-9]+(_[0-9]+)?")


def functions(asm):
    """{name: normalised text} of one assembly file"""
    out, name, desc = {}, None, None
    for line in asm.splitlines():
        line = re.sub(r"\s+", " ", re.split(r";|//", line)[0]).strip()
        m = re.match(r"\.type (\S+),@function", line)
        if m:
            name, out[m.group(1)] = m.group(1), []
        m = re.match(r"\.amdhsa_kernel (\S+)", line)
        if m:
            desc = m.group(1)
        for fn in (name, desc):
            if fn and line:
                out.setdefault(fn, []).append(line)
        if line.startswith(".Lfunc_end"):
            name = None
        if line.startswith(".end_amdhsa_kernel"):
            desc = None
    ren = lambda text, seen: LOCAL.sub(lambda m: ".L%s#%d" % (m.group(1), seen.setdefault(m.group(0), len(seen))), text)
    return {fn: ren("\n".join(lines), {}) for fn, lines in out.items()}


def compile_tree(tree, pool, extra=()):
    """{variant: {function: (file, text)}}: the plain files alone, and together with each build of qp.hip"""
    src = os.path.join(tree, "swarm_simulator_amd", "csrc")
    inc = ["-I" + os.path.join(tree, "include"), "-I" + src, "-I" + os.path.join(src, "kernels"), "-I" + os.path.join(src, "abi")]
    run = lambda f, fl: pool.submit(lambda: functions(subprocess.run(["hipcc"] + BASE + inc + list(extra) + fl + [f], check=True, stdout=subprocess.PIPE,
                                                                     stderr=subprocess.DEVNULL, text=True).stdout))
    files = sorted(glob.glob(os.path.join(src, "kernels", "*.hip")))
    plain = {os.path.basename(f): run(f, []) for f in files if os.path.basename(f) != "qp.hip"}
    qp = {v: run(os.path.join(src, "kernels", "qp.hip"), fl) for v, fl in QP_VARIANTS.items()}
    res = {"plain": {fn: (f, t) for f, fut in plain.items() for fn, t in fut.result().items()}}
    for v, fut in qp.items():
        res[v] = dict(res["plain"], **{fn: ("qp.hip", t) for fn, t in fut.result().items()})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a"), ap.add_argument("b"), ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--b-flags", default="", help="extra compiler flags for tree B only")
    args = ap.parse_args()
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        A, B = compile_tree(args.a, pool), compile_tree(args.b, pool, args.b_flags.split())
    bad = 0
    if args.b_flags:
        print("# tree B compiled with", args.b_flags)
    print("# tools/isa_diff.py: device functions of B against A, text of the gfx950 assembly per function (labels renumbered, comments stripped)")
    for v in A:
        a, b = A[v], B[v]
        same = [fn for fn in a if fn in b and a[fn][1] == b[fn][1]]
        differ, missing, added = [fn for fn in a if fn in b and a[fn][1] != b[fn][1]], [fn for fn in a if fn not in b], [fn for fn in b if fn not in a]
        moved = [fn for fn in same if a[fn][0] != b[fn][0]]
        bad += len(differ) + len(missing)
        print(f"\n## {v}: {len(a)} functions in A, {len(b)} in B: {len(same)} identical, {len(differ)} differ, {len(missing)} missing in B, {len(added)} only in B")
        for tag, fns in (("differs", differ), ("missing in B", missing), ("only in B", added)):
            for fn in fns:
                print(f"  {tag}: {fn}")
        for fn in moved:
            print(f"  identical, moved {a[fn][0]} -> {b[fn][0]}: {fn}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
