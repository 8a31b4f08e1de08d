"""Where a knot's inverse factor lives in global memory (kernels/knot_factor_layout.h: QpWs::Lf, written by knot_inverse of
kernels/qp_wave_factor.inc, read by the staging threads of solve_staged in kernels/qp_wave_solve.inc).

The index functions are plain C, so their invariants are checked on the CPU by a stand-alone program (g++, with the address and
undefined-behaviour sanitizers where their runtimes are installed), for NK = 9, 18, 27, 36:
  * every (r, k >= kf_first(r)) and every 1 / d entry has an offset of its own inside the slot stride;
  * rows are contiguous and follow each other in order; for even NK every row and 1 / d start at an even offset, and every 16-byte pair
    of the run lies inside one row or inside 1 / d; the stride is a multiple of 16 doubles (a 128-byte line);
  * NK = 36: a slot on a 128-byte boundary touches exactly 45 lines, where the addressing this layout replaced -- restated here: row r
    at r * 36, columns k >= r, 1 / d at 36 * 36, slots 36 * 36 + 40 doubles apart -- touches at least 65 on every one of 35 consecutive slots;
  * the staging map of solve_staged, built from the header as the kernel builds it (unit e = thread + u * NST of the left chain's run
    followed by the right chain's), covers each stage-buffer destination side * SCH + r * KL_LD + k (k >= kf_first(r)) and
    side * SCH + SM + i exactly once and nothing else, for NST = 128 and 384 staging threads.

The second test cuts the sessions tests/test_gpu_packed_factor.py runs (N = 5 and 7 agents of the 8-agent golden) and finds an admissible
case for every M: no GPU is needed for that."""
import os
import subprocess
import tempfile

from tests import synth_qp as SQ

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(HERE, "..", "swarm_simulator_amd", "csrc", "kernels")

PROGRAM = r"""
#define KF_FN inline
#include "knot_factor_layout.h"
#include <cstdio>
#include <set>
#include <vector>
// of knot_lds.inc / qp_wave_solve.inc (KsLayout)
constexpr int KL_LD = 38, KL_I = 40;
static_assert(kf_tri(36) == 684 && kf_dinv(36) == 684 && kf_run(36) == 720 && kf_stride(36) == 720, "NK = 36: 684 + 36 doubles");
static_assert(kf_sq_stride(36) == 36 * 36 + KL_I, "the square image restates KL_I");

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAIL line %d (NK %d): %s\n", __LINE__, nk, #c);     \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    for (int nk : {9, 18, 27, 36}) {
        const int stride = kf_stride(nk), even = (nk & 1) == 0;
        // distinct offsets inside the stride; rows contiguous and in order
        std::vector<int> hit(stride, 0);
        int next = 0;
        for (int r = 0; r < nk; ++r) {
            const int f = kf_first(nk, r);
            CHECK(f <= r && r - f <= 1 && (even ? f == (r & ~1) : f == r));
            CHECK(kf_row(nk, r) == next && kf_elem(nk, r, f) == next && kf_len(nk, r) == nk - f);
            if (even) CHECK(kf_row(nk, r) % 2 == 0 && kf_len(nk, r) % 2 == 0);
            for (int k = f; k < nk; ++k) {
                const int o = kf_elem(nk, r, k);
                CHECK(o == next && o >= 0 && o < stride);
                hit[o]++, next++;
                CHECK(kf_row_of(nk, o) == r);
            }
        }
        CHECK(next == kf_tri(nk) && kf_dinv(nk) >= next && kf_dinv(nk) - next <= 1 && kf_dinv(nk) % 2 == 0);
        for (int i = 0; i < nk; ++i) {
            const int o = kf_dinv(nk) + i;
            CHECK(o < stride);
            hit[o]++;
        }
        for (int o = 0; o < stride; ++o) CHECK(hit[o] <= 1);
        CHECK(kf_run(nk) == kf_dinv(nk) + nk && stride >= kf_run(nk) && stride - kf_run(nk) < 16 && stride % 16 == 0);
        if (even) {  // every 16-byte pair of the run inside one row or inside 1 / d
            CHECK(kf_unit(nk) == 2 && kf_run(nk) % 2 == 0 && kf_units(nk) * 2 == kf_run(nk));
            for (int o = 0; o < kf_run(nk); o += 2) {
                if (o < kf_tri(nk))
                    CHECK(o + 1 < kf_tri(nk) && kf_row_of(nk, o) == kf_row_of(nk, o + 1));
                else
                    CHECK(o >= kf_dinv(nk) && o + 1 < kf_run(nk));
            }
        } else {
            CHECK(kf_unit(nk) == 1 && kf_units(nk) == kf_run(nk));
        }
        // the staging map of solve_staged
        const int SM = nk * KL_LD, SCH = SM + KL_I, STG = 2 * SCH, UN = kf_unit(nk), NU = kf_units(nk);
        for (int NST : {128, 384}) {
            const int MAXE = (2 * NU + NST - 1) / NST;
            std::vector<int> cover(STG, 0);
            for (int t = 0; t < NST; ++t)
                for (int u = 0; u < MAXE; ++u) {
                    const int e = t + u * NST;
                    if (e >= 2 * NU) continue;
                    // (kf_unit_side / kf_unit_off: what unit_src of solve_staged loads from; restated for the check)
                    const int side = kf_unit_side(nk, e), idx = kf_unit_off(nk, e) / UN;
                    CHECK(side == (e >= NU) && kf_unit_off(nk, e) == (e - side * NU) * UN && kf_unit_off(nk, e) + UN <= stride);
                    const int dd = kf_stage_dst(nk, kf_unit_off(nk, e), KL_LD, SM);
                    if (dd < 0) {  // only the gap between an odd triangle and 1 / d
                        CHECK(!even && idx * UN >= kf_tri(nk) && idx * UN < kf_dinv(nk));
                        continue;
                    }
                    if (UN == 2) CHECK((side * SCH + dd) % 2 == 0 && kf_stage_dst(nk, idx * UN + 1, KL_LD, SM) == dd + 1);
                    for (int q = 0; q < UN; ++q) {
                        CHECK(side * SCH + dd + q < STG);
                        cover[side * SCH + dd + q]++;
                    }
                }
            std::vector<int> want(STG, 0);
            for (int side = 0; side < 2; ++side) {
                for (int r = 0; r < nk; ++r)
                    for (int k = kf_first(nk, r); k < nk; ++k) want[side * SCH + r * KL_LD + k] = 1;
                for (int i = 0; i < nk; ++i) want[side * SCH + SM + i] = 1;
            }
            for (int o = 0; o < STG; ++o) CHECK(cover[o] == want[o]);
        }
        if (nk == 36) {  // 128-byte lines: 16 doubles
            std::set<int> lines;
            for (int o = 0; o < kf_run(nk); ++o) lines.insert(o / 16);
            CHECK((int)lines.size() == 45 && stride / 16 == 45);
            int lo = 1 << 30, hi = 0;
            for (int j = 0; j < 35; ++j) {  // the square image on a 128-byte boundary, slots 36 * 36 + 40 doubles apart
                std::set<long> sq;
                const long base = (long)j * (36 * 36 + 40);
                for (int r = 0; r < 36; ++r)
                    for (int k = r; k < 36; ++k) sq.insert((base + r * 36 + k) / 16);
                for (int i = 0; i < 36; ++i) sq.insert((base + 36 * 36 + i) / 16);
                CHECK((int)sq.size() >= 65);
                lo = (int)sq.size() < lo ? (int)sq.size() : lo, hi = (int)sq.size() > hi ? (int)sq.size() : hi;
            }
            printf("NK 36: packed 45 lines per slot; square image %d .. %d lines over 35 slots\n", lo, hi);
        }
        printf("NK %d: triangle %d, 1/d at %d, run %d, stride %d doubles ok\n", nk, kf_tri(nk), kf_dinv(nk), kf_run(nk), stride);
    }
    printf("PASS\n");
    return 0;
}
"""


def test_layout_invariants_and_staging_map():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write(PROGRAM)
        # the sanitizers where their runtimes are installed: a trivial program tells (the real one must then build with them)
        probe = os.path.join(d, "probe.cpp")
        with open(probe, "w") as f:
            f.write("int main() { return 0; }\n")
        SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        have = subprocess.run(["g++", "-o", os.path.join(d, "probe")] + SAN + [probe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
        print("build:", "address + undefined-behaviour sanitizers" if have else "no sanitizer runtimes on this machine: plain")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", KERNELS, "-o", exe, src] + (SAN if have else []))
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0 and out.strip().splitlines()[-1] == "PASS", out
    assert sum(1 for l in out.splitlines() if l.startswith("NK ") and l.endswith(" ok")) == 4, out


def test_cut_sessions_of_the_packed_factor_test_are_admissible():
    from tests.test_gpu_fwd_in_factor import cut_cases

    for N, tail in ((5, 1), (7, 3)):
        cfs = cut_cases(N)
        assert sorted(c.M for c, _ in cfs) == sorted(SQ.MS)
        assert all(c.N == N and c.param().batch_size == 4 and c.param().sequential and f is not None for c, f in cfs)
        assert N % 4 == tail  # the tail batch: order 9 * tail
