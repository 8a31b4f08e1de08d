"""Panel-blocked knot factorisation (kernels/knot_panel_layout.h, used by kernels/knot_lds.inc: kl_ldl_panels / kl_inverse_panels).

The index functions are plain C, so their invariants are checked on the CPU: the operand maps of v_mfma_f64_16x16x4_f64 are bijections
onto their tiles, the packed tile indices of the two triangles are permutations, panel images do not overlap and fit the C / U region
of KlArea, and a panel's rows are where the chain wave looks for them (register p % 4 of the tiles of tile row p / 4).

The second test is a host restatement of the device algorithm, lane by lane and in its operation order -- tiles in the C/D layout,
panel image, the 4 x 4 diagonal block factorised redundantly, rows eliminated against it, L written over the image, rank-4 tile updates,
panel-wise inverse from that image,
transposed store into the rows of MX -- against a plain scalar L D L' and triangular inverse, to the tolerances of tools/ubench/knot.hip
(|M err| < 1e-11 * scale, relative 1/d error < 1e-12), for NK = 9, 18, 27, 36, 20 seeded SPD matrices each at diagonal spreads 1, 1e4
and 1e8.  The third compiles the micro-benchmark for gfx950 (both paths) so that it cannot go stale against knot_lds.inc."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(HERE, "..", "swarm_simulator_amd", "csrc", "kernels")
UBENCH = os.path.join(HERE, "..", "tools", "ubench", "knot.hip")

PRELUDE = r"""
#define __host__
#define __device__
#include "knot_panel_layout.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>
// of knot_lds.inc (checked against it by the static_asserts there: kl_area_doubles)
constexpr int KL_LD = 38, KL_LDU = 50;
"""

LAYOUT = PRELUDE + r"""
int main() {
    // operand layouts: every (row, k) of A, (k, col) of B and (row, col) of C/D is served by exactly one (lane[, reg])
    int a[16][4] = {}, b[4][16] = {}, cd[16][16] = {};
    for (int lane = 0; lane < 64; ++lane) {
        a[kp_a_row(lane)][kp_a_k(lane)]++, b[kp_b_k(lane)][kp_b_col(lane)]++;
        for (int reg = 0; reg < 4; ++reg) cd[kp_cd_row(lane, reg)][kp_cd_col(lane)]++;
        // the documented 16x16x4 layout (kl_syrk): col = lane & 15, row = (lane >> 4) + 4 reg
        if (kp_cd_col(lane) != (lane & 15) || kp_cd_row(lane, 2) != (lane >> 4) + 8) return 1;
    }
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 4; ++k)
            if (a[i][k] != 1 || b[k][i] != 1) return 2;
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j)
            if (cd[i][j] != 1) return 3;
    for (int nk : {9, 18, 27, 36}) {
        const int nt = kp_nt(nk), np = kp_np(nk);
        if (16 * nt < nk || 16 * (nt - 1) >= nk || 4 * np < nk || 4 * (np - 1) >= nk || kp_rows(nk) != 16 * nt) return 4;
        // packed tile indices: permutations of 0 .. ntiles - 1
        std::vector<int> up(kp_ntiles(nt), 0), lo(kp_ntiles(nt), 0);
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = ti; tj < nt; ++tj) {
                const int u = kp_upper(ti, tj, nt), l = kp_lower(tj, ti);
                if (u < 0 || u >= kp_ntiles(nt) || l < 0 || l >= kp_ntiles(nt)) return 5;
                up[u]++, lo[l]++;
            }
        for (int t = 0; t < kp_ntiles(nt); ++t)
            if (up[t] != 1 || lo[t] != 1) return 6;
        // panel bookkeeping: row 4p + k of the padded block is register p % 4 of the lanes with lane >> 4 == k in tile row p / 4
        for (int p = 0; p < np; ++p) {
            const int tc = kp_panel_tile(p), q = kp_panel_reg(p);
            if (tc >= nt) return 7;
            for (int lane = 0; lane < 64; ++lane)
                if (16 * tc + kp_cd_row(lane, q) != 4 * p + (lane >> 4)) return 8;
            if (kp_first_live_tile(p) != (4 * (p + 1)) / 16) return 9;  // the tile row of the first row that is still live after panel p
        }
        // panel images: entries distinct inside an image, images disjoint, all inside the C / U region of KlArea ((NK + 1) * KL_LDU doubles)
        std::vector<int> hit(kp_img_total(nk), 0);
        for (int p = 0; p < np; ++p)
            for (int row = 0; row < kp_rows(nk); ++row)
                for (int k = 0; k < 4; ++k) {
                    const int o = kp_img_off(nk, p) + kp_img_entry(row, k);
                    if (o < 0 || o >= kp_img_total(nk)) return 10;
                    hit[o]++;
                }
        for (int h : hit)
            if (h != 1) return 11;
        if (kp_img_total(nk) > (nk + 1) * KL_LDU) return 12;
        if (kp_img_entry(1, 0) % 2 || kp_img_off(nk, 1) % 2) return 13;  // 16-byte aligned rows: ds_read_b128
    }
    std::printf("ok %d %d %d\n", kp_img_total(36), kp_ntiles(kp_nt(36)), kp_np(36));
    return 0;
}
"""

RESTATEMENT = PRELUDE + r"""
typedef std::vector<double> vec;
struct Wave {  // 64 lanes, up to 6 tiles of 4 registers
    double t[64][6][4];
};
// D = A B + C on one tile: operand a / b of every lane, C/D in reg[tile]; the four products of a sum in k order
static void mfma(Wave& w, int tile, const double (&a)[64], const double (&b)[64]) {
    for (int lane = 0; lane < 64; ++lane)
        for (int reg = 0; reg < 4; ++reg) {
            const int i = kp_cd_row(lane, reg), j = kp_cd_col(lane);
            double acc = w.t[lane][tile][reg];
            for (int k = 0; k < 4; ++k) acc = std::fma(a[i + 16 * k], b[j + 16 * k], acc);
            w.t[lane][tile][reg] = acc;
        }
}
struct Pivot {
    double i[4], w10, w20, w21, w30, w31, w32, l10, l20, l21, l30, l31, l32;
    bool ok;
};
static Pivot pivot(const double* img, int p) {  // kl_pivot_load + kl_pivot_factor
    auto D = [&](int a, int k) { return img[kp_img_entry(4 * p + a, k)]; };
    Pivot f;
    f.i[0] = 1.0 / D(0, 0);
    f.w10 = D(1, 0), f.l10 = f.w10 * f.i[0];
    f.w20 = D(2, 0), f.l20 = f.w20 * f.i[0];
    f.w30 = D(3, 0), f.l30 = f.w30 * f.i[0];
    const double d1 = std::fma(-f.l10, f.w10, D(1, 1));
    f.i[1] = 1.0 / d1;
    f.w21 = std::fma(-f.l20, f.w10, D(2, 1)), f.l21 = f.w21 * f.i[1];
    f.w31 = std::fma(-f.l30, f.w10, D(3, 1)), f.l31 = f.w31 * f.i[1];
    const double d2 = std::fma(-f.l21, f.w21, std::fma(-f.l20, f.w20, D(2, 2)));
    f.i[2] = 1.0 / d2;
    f.w32 = std::fma(-f.l31, f.w21, std::fma(-f.l30, f.w20, D(3, 2))), f.l32 = f.w32 * f.i[2];
    const double d3 = std::fma(-f.l32, f.w32, std::fma(-f.l31, f.w31, std::fma(-f.l30, f.w30, D(3, 3))));
    f.i[3] = 1.0 / d3;
    f.ok = D(0, 0) > 0 && d1 > 0 && d2 > 0 && d3 > 0;
    return f;
}
static void panel_row(const Pivot& f, const double* s, double (&L)[4], double (&W)[4]) {  // kl_panel_row
    W[0] = s[0], L[0] = W[0] * f.i[0];
    W[1] = std::fma(-L[0], f.w10, s[1]), L[1] = W[1] * f.i[1];
    W[2] = std::fma(-L[1], f.w21, std::fma(-L[0], f.w20, s[2])), L[2] = W[2] * f.i[2];
    W[3] = std::fma(-L[2], f.w32, std::fma(-L[1], f.w31, std::fma(-L[0], f.w30, s[3]))), L[3] = W[3] * f.i[3];
}

// the device algorithm on the lower triangle S (row-major, nk x nk): returns M = L^-T rows (row r contiguous, KL_LD stride) and 1 / d
static bool panels(int nk, const vec& S, vec& MX, vec& inv) {
    const int nt = kp_nt(nk), np = kp_np(nk);
    vec C(kp_img_total(nk), 0.0);
    static Wave s, n;
    // kl_tiles_load
    for (int lane = 0; lane < 64; ++lane)
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = ti; tj < nt; ++tj)
                for (int g = 0; g < 4; ++g) {
                    const int i = 16 * ti + kp_cd_row(lane, g), j = 16 * tj + kp_cd_col(lane), mx = i > j ? i : j, mn = i > j ? j : i;
                    s.t[lane][kp_upper(ti, tj, nt)][g] = mx >= nk ? (i == j ? 1.0 : 0.0) : S[mx * nk + mn];
                }
    auto panel_out = [&](int p) {
        for (int lane = 0; lane < 64; ++lane)
            for (int tj = kp_panel_tile(p); tj < nt; ++tj)
                C[kp_img_off(nk, p) + kp_img_entry(16 * tj + (lane & 15), lane >> 4)] = s.t[lane][kp_upper(kp_panel_tile(p), tj, nt)][kp_panel_reg(p)];
    };
    bool ok = true;
    panel_out(0);
    for (int p = 0; p < np; ++p) {  // kl_ldl_panels
        const double* img = C.data() + kp_img_off(nk, p);
        const Pivot f = pivot(img, p);
        ok = ok && f.ok;
        for (int a = 0; a < 4; ++a)
            if (4 * p + a < nk) inv[4 * p + a] = f.i[a];
        const int t0 = kp_first_live_tile(p);
        double a[3][64], b[3][64];
        for (int t = kp_panel_tile(p); t < nt; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                double L[4], W[4];
                panel_row(f, img + kp_img_entry(16 * t + (lane & 15), 0), L, W);
                b[t][lane] = W[lane >> 4], a[t][lane] = -(b[t][lane] * f.i[lane >> 4]);
            }
        for (int t = kp_panel_tile(p); t < nt; ++t)  // L replaces S in the image (after every lane has read its rows)
            for (int lane = 0; lane < 64; ++lane) C[kp_img_off(nk, p) + kp_img_entry(16 * t + (lane & 15), lane >> 4)] = -a[t][lane];
        if (p + 1 == np) break;
        for (int tj = t0; tj < nt; ++tj) mfma(s, kp_upper(t0, tj, nt), a[t0], b[tj]);
        panel_out(p + 1);
        for (int ti = t0 + 1; ti < nt; ++ti)
            for (int tj = ti; tj < nt; ++tj) mfma(s, kp_upper(ti, tj, nt), a[ti], b[tj]);
    }
    // kl_inverse_panels
    for (int lane = 0; lane < 64; ++lane)
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = 0; tj <= ti; ++tj)
                for (int g = 0; g < 4; ++g) n.t[lane][kp_lower(ti, tj)][g] = (ti == tj && kp_cd_row(lane, g) == kp_cd_col(lane)) ? 1.0 : 0.0;
    for (int p = 0; p < np; ++p) {
        const int tc = kp_panel_tile(p), q = kp_panel_reg(p);
        const double* img = C.data() + kp_img_off(nk, p);
        auto l = [&](int a, int k) { return img[kp_img_entry(4 * p + a, k)]; };  // the unit lower diagonal block of L
        const double k10 = -l(1, 0), k21 = -l(2, 1), k32 = -l(3, 2);
        const double k20 = std::fma(-l(2, 1), k10, -l(2, 0)), k31 = std::fma(-l(3, 2), k21, -l(3, 1));
        const double k30 = std::fma(-l(3, 2), k20, std::fma(-l(3, 1), k10, -l(3, 0)));
        double a[3][64], b[3][64];
        for (int t = tc; t < nt; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const double* L = img + kp_img_entry(16 * t + (lane & 15), 0);
                double G[4];
                G[3] = -L[3];
                G[2] = -std::fma(L[3], k32, L[2]);
                G[1] = -std::fma(L[3], k31, std::fma(L[2], k21, L[1]));
                G[0] = -std::fma(L[3], k30, std::fma(L[2], k20, std::fma(L[1], k10, L[0])));
                const int ar = 16 * t + (lane & 15) - 4 * p;
                if (ar < 4) {
                    G[0] = ar == 1 ? k10 : ar == 2 ? k20 : ar == 3 ? k30 : 0.0;
                    G[1] = ar == 2 ? k21 : ar == 3 ? k31 : 0.0;
                    G[2] = ar == 3 ? k32 : 0.0;
                    G[3] = 0.0;
                }
                a[t][lane] = G[lane >> 4];
            }
        for (int tj = 0; tj <= tc; ++tj)
            for (int lane = 0; lane < 64; ++lane) b[tj][lane] = n.t[lane][kp_lower(tc, tj)][q];
        for (int ti = tc; ti < nt; ++ti)
            for (int tj = 0; tj <= tc; ++tj) mfma(n, kp_lower(ti, tj), a[ti], b[tj]);
    }
    // kl_tiles_to_rows: M[row][col] = N[col][row]; padding -> row nk
    for (int lane = 0; lane < 64; ++lane)
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = 0; tj < nt; ++tj)
                for (int g = 0; g < 4; ++g) {
                    if (16 * ti + 4 * g >= nk) continue;
                    const int col = 16 * ti + kp_cd_row(lane, g), row = 16 * tj + kp_cd_col(lane);
                    const bool in = row < nk && col < nk;
                    const int o = in ? row * KL_LD + col : nk * KL_LD + (lane & 15);
                    if (o < 0 || o >= (nk + 1) * KL_LD) std::exit(20);  // inside the MX region of KlArea
                    MX[o] = tj <= ti ? n.t[lane][kp_lower(ti, tj)][g] : 0.0;
                }
    return ok;
}

int main() {
    double worst_m = 0, worst_d = 0;
    for (int nk : {9, 18, 27, 36})
        for (double spread : {1.0, 1e4, 1e8})
            for (int seed = 0; seed < 20; ++seed) {
                srand(1000 * nk + seed);
                auto rnd = [] { return rand() / (double)RAND_MAX - 0.5; };
                vec B(nk * nk), S(nk * nk);
                for (auto& v : B) v = rnd();
                for (int r = 0; r < nk; ++r)
                    for (int k = 0; k < nk; ++k) {
                        double s = 0;
                        for (int q = 0; q < nk; ++q) s += B[r * nk + q] * B[k * nk + q];
                        S[r * nk + k] = s + (r == k ? 30.0 + spread * (r % 5 == 0) : 0.0);
                    }
                // plain scalar L D L' and the inverse of L
                vec A = S, L(nk * nk, 0.0), d(nk), Li(nk * nk, 0.0);
                for (int c = 0; c < nk; ++c) {
                    d[c] = A[c * nk + c], L[c * nk + c] = 1;
                    for (int r = c + 1; r < nk; ++r) L[r * nk + c] = A[r * nk + c] / d[c];
                    for (int r = c + 1; r < nk; ++r)
                        for (int k = c + 1; k < nk; ++k) A[r * nk + k] -= L[r * nk + c] * d[c] * L[k * nk + c];
                }
                for (int c = 0; c < nk; ++c)
                    for (int r = 0; r < nk; ++r) {
                        double s = r == c ? 1.0 : 0.0;
                        for (int k = 0; k < r; ++k) s -= L[r * nk + k] * Li[k * nk + c];
                        Li[r * nk + c] = s;
                    }
                vec MX((nk + 1) * KL_LD, -7.0), inv(nk, 0.0);
                if (!panels(nk, S, MX, inv)) return 1;
                double em = 0, sm = 0, ed = 0;
                for (int r = 0; r < nk; ++r) {
                    for (int k = 0; k < nk; ++k) {
                        const double want = Li[k * nk + r];  // M[r][k] = (L^-1)[k][r]; the zeros below the diagonal are stored
                        if (k < r && MX[r * KL_LD + k] != 0.0) return 2;
                        em = std::fmax(em, std::fabs(MX[r * KL_LD + k] - want)), sm = std::fmax(sm, std::fabs(want));
                    }
                    ed = std::fmax(ed, std::fabs(inv[r] - 1.0 / d[r]) * std::fabs(d[r]));
                }
                if (!(em < 1e-11 * std::fmax(1.0, sm)) || !(ed < 1e-12)) {
                    std::printf("nk %d spread %g seed %d: M err %g (scale %g) 1/d err %g\n", nk, spread, seed, em, sm, ed);
                    return 3;
                }
                worst_m = std::fmax(worst_m, em / std::fmax(1.0, sm)), worst_d = std::fmax(worst_d, ed);
            }
    std::printf("ok %.3g %.3g\n", worst_m, worst_d);
    return 0;
}
"""


def _run(source):
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        open(src, "w").write(source)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", KERNELS, "-o", exe, src])
        return subprocess.check_output([exe]).decode().split()


def test_maps_of_the_panel_layout():
    # 9 panels of 48 rows x 4 columns, 6 tiles of a triangle of the padded 36 x 36 block
    assert _run(LAYOUT) == ["ok", "1728", "6", "9"]


def test_host_restatement_of_the_panel_algorithm_against_the_scalar_recursion():
    out = _run(RESTATEMENT)
    assert out[0] == "ok", out
    assert float(out[1]) < 1e-11 and float(out[2]) < 1e-12


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
@pytest.mark.parametrize("panel", [0, 1])
def test_the_knot_microbenchmark_compiles_for_gfx950(panel):
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", KERNELS, f"-DKL_PANEL={panel}",
                               "-c", "-o", os.path.join(d, "knot.o"), UBENCH])
