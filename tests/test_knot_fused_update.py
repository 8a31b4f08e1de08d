"""Rank-NK update of the next knot block formed in the MFMA tiles (kernels/knot_lds.inc: kl_fused_coef, kl_fused_update, kl_tiles_load
with OP 2; index maps kp_x_group / kp_x_first_kstep / kp_ksteps of kernels/knot_panel_layout.h).

A host restatement, lane by lane and MFMA step by MFMA step: the coefficients a lane picks for the rows it serves, the three rows of M
an operand element combines, A = -X and B = X / d, the k-steps that are left out because the B operand is all zeros, the padding rows
and columns, and T added to the tiles afterwards -- against the plain dense T - (Cpl M) D^-1 (Cpl M)'.

Cases: NK = 36 and, so that partial tiles, partial k-steps and padding rows are exercised, 9, 18, 27; dir = +1 and -1; the two-sided
accumulation of the middle block (the left chain's M with dir +1 and the right chain's with dir -1, each summed on its own, then added); random upper
triangular M (zeros below the diagonal stored, as kl_tiles_scatter leaves them), positive d spread over 1e4 and 1e8.
Bounds: 1e-11 * scale against the dense result (the bound of tools/ubench/knot.hip); bit equality between the restatement with and
without the skipped k-steps, which multiply exact zeros; bit equality with T - U as the path with stored X and U rounds it (the scaled
factor is the later row's, the middle block adds two separately rounded sums), so that the factorisation sees the numbers it saw before;
the tiles' padding is exactly the unit diagonal.

The second test compiles the micro-benchmark for gfx950 with -DKL_FUSED_UPDATE=0 and =1 so that neither side of the A/B goes stale."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(HERE, "..", "swarm_simulator_amd", "csrc", "kernels")
UBENCH = os.path.join(HERE, "..", "tools", "ubench", "knot.hip")

RESTATEMENT = r"""
#define __host__
#define __device__
#include "knot_panel_layout.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>
constexpr int KL_LD = 38;  // of knot_lds.inc
typedef std::vector<double> vec;
struct Wave {  // 64 lanes, up to 6 tiles of 4 registers
    double t[64][6][4];
};
static long n_mfma;
// D = A B + C on one tile: operand a / b of every lane, C/D in reg[tile]; the four products of a sum in k order
static void mfma(Wave& w, int tile, const double (&a)[64], const double (&b)[64]) {
    ++n_mfma;
    for (int lane = 0; lane < 64; ++lane)
        for (int reg = 0; reg < 4; ++reg) {
            const int i = kp_cd_row(lane, reg), j = kp_cd_col(lane);
            double acc = w.t[lane][tile][reg];
            for (int k = 0; k < 4; ++k) acc = std::fma(a[i + 16 * k], b[j + 16 * k], acc);
            w.t[lane][tile][reg] = acc;
        }
}
// coupling_coef of qp.hip: T_next,this[row][group + q] from the knot's 3 x 3 block E
static double coef(const double* E, int dir, int row, int q) { return dir > 0 ? E[3 * q + row % 3] : E[3 * (row % 3) + q]; }

// kl_fused_coef + kl_fused_update: s -= X D^-1 X', MX = rows of M (KL_LD stride, nk + 1 rows), I = 1 / d
static void fused_update(int nk, Wave& s, const vec& MX, const vec& I, const double* E, int dir, bool skip) {
    const int nt = kp_nt(nk), KS = kp_ksteps(nk);
    static double cf[64][3][3];
    static int grp[64][3];
    for (int lane = 0; lane < 64; ++lane)
        for (int t = 0; t < nt; ++t) {
            const int row = 16 * t + kp_a_row(lane);
            const bool in = row < nk;
            for (int q = 0; q < 3; ++q) cf[lane][t][q] = in ? coef(E, dir, row, q) : 0.0;
            grp[lane][t] = kp_x_group(in ? row : 0) * KL_LD + kp_a_k(lane);
        }
    for (int ks = 0; ks < KS; ++ks) {
        double a[3][64], b[3][64];
        for (int t = 0; t < nt; ++t) {
            if (skip && ks < kp_x_first_kstep(t)) continue;
            for (int lane = 0; lane < 64; ++lane) {
                const int kc = 4 * ks + kp_a_k(lane);
                const bool live = kc < nk;
                const int o = grp[lane][t] + 4 * ks;
                if (o + 2 * KL_LD >= (nk + 1) * KL_LD) std::exit(20);  // inside the MX region of KlArea
                const double x = cf[lane][t][0] * MX[o] + cf[lane][t][1] * MX[o + KL_LD] + cf[lane][t][2] * MX[o + 2 * KL_LD];
                const double dk = I[live ? kc : 0];
                a[t][lane] = live ? -x : 0.0;
                b[t][lane] = live ? x * dk : 0.0;
            }
        }
        for (int tj = 0; tj < nt; ++tj) {
            if (skip && ks < kp_x_first_kstep(tj)) continue;
            for (int ti = 0; ti <= tj; ++ti) mfma(s, kp_upper(ti, tj, nt), a[ti], b[tj]);
        }
    }
}
// kl_tiles_load, OP 2: T (lower triangle, row-major) added to the tiles, the padding set to the unit diagonal
static void add_t(int nk, Wave& s, const vec& T) {
    const int nt = kp_nt(nk);
    for (int lane = 0; lane < 64; ++lane)
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = ti; tj < nt; ++tj)
                for (int g = 0; g < 4; ++g) {
                    const int i = 16 * ti + kp_cd_row(lane, g), j = 16 * tj + kp_cd_col(lane), mx = i > j ? i : j, mn = i > j ? j : i;
                    double& v = s.t[lane][kp_upper(ti, tj, nt)][g];
                    v = mx >= nk ? (i == j ? 1.0 : 0.0) : v + T[mx * nk + mn];
                }
}

struct Side {
    vec MX, I, d;
    double E[9];
    int dir;
};
static double rnd() { return rand() / (double)RAND_MAX - 0.5; }
static Side make_side(int nk, double spread, int dir) {
    Side s;
    s.MX.assign((nk + 1) * KL_LD, -7.0), s.I.assign(40, -7.0), s.d.assign(nk, 0.0), s.dir = dir;  // (row nk and the columns >= nk: finite junk)
    for (int r = 0; r < nk; ++r)
        for (int k = 0; k < nk; ++k) s.MX[r * KL_LD + k] = k < r ? 0.0 : (k == r ? 1.0 : 2.0 * rnd());  // M = L^-T: unit upper triangular
    for (int k = 0; k < nk; ++k) s.d[k] = std::pow(spread, rand() / (double)RAND_MAX), s.I[k] = 1.0 / s.d[k];
    for (double& e : s.E) e = 3.0 * rnd();
    return s;
}
// the plain dense (Cpl M) D^-1 (Cpl M)' subtracted from S (full symmetric, row-major)
static void dense(int nk, vec& S, const Side& sd) {
    vec X(nk * nk, 0.0);
    for (int r = 0; r < nk; ++r)
        for (int k = 0; k < nk; ++k)
            for (int q = 0; q < 3; ++q) X[r * nk + k] += coef(sd.E, sd.dir, r, q) * sd.MX[(3 * (r / 3) + q) * KL_LD + k];
    for (int r = 0; r < nk; ++r)
        for (int c = 0; c < nk; ++c) {
            double u = 0;
            for (int k = 0; k < nk; ++k) u += X[r * nk + k] / sd.d[k] * X[c * nk + k];
            S[r * nk + c] -= u;
        }
}

// U (+)= X D^-1 X' as the path with stored X computes its LOWER tiles (kl_syrk: A = X[j] / d of the later row j, B = X[i], k-steps from the first
// live one of j's tile row, the products of a step in k order), X rounded as kl_coupling_rows stores it
static void stored_u(int nk, vec& U, const Side& sd, bool accumulate) {
    vec X(nk * nk);
    for (int r = 0; r < nk; ++r)
        for (int k = 0; k < nk; ++k) {
            const double* m0 = sd.MX.data() + kp_x_group(r) * KL_LD + k;
            X[r * nk + k] = coef(sd.E, sd.dir, r, 0) * m0[0] + coef(sd.E, sd.dir, r, 1) * m0[KL_LD] + coef(sd.E, sd.dir, r, 2) * m0[2 * KL_LD];
        }
    for (int j = 0; j < nk; ++j)
        for (int i = 0; i <= j; ++i) {
            double acc = 0;
            for (int k = 4 * kp_x_first_kstep(j / 16); k < nk; ++k) acc = std::fma(X[j * nk + k] * sd.I[k], X[i * nk + k], acc);
            U[j * nk + i] = accumulate ? U[j * nk + i] + acc : acc;
        }
}

int main() {
    // the k-step skip for the flagship size: tile rows 0, 1, 2 start at k-steps 0, 3, 7 -- 27 MFMAs instead of 54
    if (kp_ksteps(36) != 9 || kp_x_first_kstep(0) != 0 || kp_x_first_kstep(1) != 3 || kp_x_first_kstep(2) != 7) return 1;
    for (int r = 0; r < 48; ++r)
        if (kp_x_group(r) != r - r % 3 || 4 * kp_x_first_kstep(r / 16) > kp_x_group(r)) return 2;  // no skipped k-step holds a live column of any row of the tile row
    double worst = 0;
    for (int nk : {9, 18, 27, 36})
        for (double spread : {1e4, 1e8})
            for (int mode = 0; mode < 3; ++mode)  // 0: dir +1, 1: dir -1, 2: the middle block (both)
                for (int seed = 0; seed < 4; ++seed) {
                    srand(100000 * mode + 1000 * nk + seed + (spread > 1e5 ? 50 : 0));
                    vec T(nk * nk);
                    for (int r = 0; r < nk; ++r)
                        for (int k = 0; k <= r; ++k) T[r * nk + k] = T[k * nk + r] = 10.0 * rnd() + (r == k ? 30.0 + spread * (r % 5 == 0) : 0.0);
                    std::vector<Side> sides;
                    if (mode != 1) sides.push_back(make_side(nk, spread, +1));
                    if (mode != 0) sides.push_back(make_side(nk, spread, -1));
                    static Wave s[2];
                    long count[2];
                    for (int skip = 0; skip < 2; ++skip) {
                        std::memset(&s[skip], 0, sizeof(Wave));  // kl_tiles_zero
                        n_mfma = 0;
                        for (size_t k = 0; k < sides.size(); ++k) {  // wave_factor_mid: each side summed on its own, then the two sums added
                            static Wave s2;
                            Wave& dst = k == 0 ? s[skip] : s2;
                            if (k > 0) std::memset(&s2, 0, sizeof(Wave));
                            fused_update(nk, dst, sides[k].MX, sides[k].I, sides[k].E, sides[k].dir, skip != 0);
                            if (k > 0)
                                for (int lane = 0; lane < 64; ++lane)
                                    for (int t = 0; t < 6; ++t)
                                        for (int g = 0; g < 4; ++g) s[skip].t[lane][t][g] += s2.t[lane][t][g];
                        }
                        count[skip] = n_mfma;
                        add_t(nk, s[skip], T);
                    }
                    if (nk == 36 && (count[0] != 54 * (long)sides.size() || count[1] != 27 * (long)sides.size())) return 3;
                    // the bits of the path with stored X and U (kl_coupling_rows, kl_syrk, T - U): the factorisation must see the same numbers
                    vec U(nk * nk, 0.0);
                    for (size_t k = 0; k < sides.size(); ++k) stored_u(nk, U, sides[k], k > 0);
                    vec S = T;
                    for (const Side& sd : sides) dense(nk, S, sd);
                    double err = 0, scale = 0;
                    const int nt = kp_nt(nk);
                    for (int lane = 0; lane < 64; ++lane)
                        for (int ti = 0; ti < nt; ++ti)
                            for (int tj = ti; tj < nt; ++tj)
                                for (int g = 0; g < 4; ++g) {
                                    const int i = 16 * ti + kp_cd_row(lane, g), j = 16 * tj + kp_cd_col(lane), tile = kp_upper(ti, tj, nt);
                                    const double v = s[1].t[lane][tile][g];
                                    if (std::memcmp(&v, &s[0].t[lane][tile][g], 8) != 0 && !(v == 0.0 && s[0].t[lane][tile][g] == 0.0)) return 4;  // skip or not: the same bits
                                    if (i >= nk || j >= nk) {
                                        if (v != (i == j ? 1.0 : 0.0)) return 5;  // the padding: unit diagonal, exactly
                                        continue;
                                    }
                                    if (ti == tj && i > j) continue;  // (below the diagonal of a diagonal tile: not consumed)
                                    const double stored = T[j * nk + i] - U[j * nk + i];
                                    if (std::memcmp(&v, &stored, 8) != 0 && !(v == 0.0 && stored == 0.0)) return 7;  // the same bits as T - U of the stored path
                                    err = std::fmax(err, std::fabs(v - S[i * nk + j])), scale = std::fmax(scale, std::fabs(S[i * nk + j]));
                                }
                    if (!(err < 1e-11 * std::fmax(1.0, scale))) {
                        std::printf("nk %d spread %g mode %d seed %d: S err %g (scale %g)\n", nk, spread, mode, seed, err, scale);
                        return 6;
                    }
                    worst = std::fmax(worst, err / std::fmax(1.0, scale));
                }
    std::printf("ok %.3g\n", worst);
    return 0;
}
"""


def test_host_restatement_of_the_fused_update_against_the_dense_schur_complement():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        open(src, "w").write(RESTATEMENT)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", KERNELS, "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split()
    assert out[0] == "ok", out
    assert float(out[1]) < 1e-11


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
@pytest.mark.parametrize("fused", [0, 1])
def test_the_knot_microbenchmark_compiles_for_gfx950_with_and_without_the_fused_update(fused):
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", KERNELS, f"-DKL_FUSED_UPDATE={fused}",
                               "-c", "-o", os.path.join(d, "knot.o"), UBENCH])
