// Host restatement of the wave path's substitutions (kernels/knot_subst.h, as g++ builds it): a block-tridiagonal system of nj knots of
// order 36 with the product's coupling blocks (3x3-block diagonal), eliminated from both ends towards the middle block (twist_mid), with
// M_j = L_j^-T (rows of stride KL_LD, zeros left of the diagonal) and 1 / d_j as the kernel stores them.  It is solved twice with the
// header's step bodies, 64 threads standing in for the 64 lanes and a barrier for kl_sync:
//   FULL   as solve_staged does: forward steps, the middle block, backward steps, M_j in a stage buffer (1 / d behind it), the vectors
//          with KS_VPAD zeros either side;
//   SPLIT  as QP_FWD_IN_FACTOR does: the forward steps in elimination order out of a chain AREA (KfSlots: A and the partial sums at the
//          end of the panel images -- scribbled over between the steps, as the next factorisation does --, zeros / Z / V in the C region's
//          tail, 1 / d in I, NaNs behind the padding row of MX: the guarded product must not see them), z_j to a global vector; the middle
//          step; then backward only, out of stage buffers again, both V seeded with x_mid.
// The two must agree bit for bit; the distance of either to a long-double banded solve is printed for the record.
#include <pthread.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#define KS_FN inline
#define KP_FN inline
#include "kernels/knot_subst.h"

constexpr int NK = 36, LANES = 64;
static int twist_mid(int nj) { return nj / 2; }
static double rnd() { return rand() / (double)RAND_MAX - 0.5; }

struct System {
    int nj;
    std::vector<double> T;   // [nj][NK][NK] symmetric
    std::vector<double> Ek;  // [nj][9]: knot j couples j - 1 and j (entry 0 unused)
    std::vector<double> rhs;
    // factor, as QpWs::Lf holds it: M_j [NK][NK] row-major (upper triangle), then 1 / d_j
    std::vector<double> M, dinv;
};
// row rr of T_{j+dir,j} within its 3x3 block (coupling_coef of qp_wave_factor.inc)
static void coupling_coef(const System& S, int j, int dir, int rr, double& e0, double& e1, double& e2) {
    const double* E = S.Ek.data() + 9 * (dir > 0 ? j + 1 : j);
    e0 = dir > 0 ? E[rr % 3] : E[3 * (rr % 3)], e1 = dir > 0 ? E[3 + rr % 3] : E[3 * (rr % 3) + 1], e2 = dir > 0 ? E[6 + rr % 3] : E[3 * (rr % 3) + 2];
}
// T_{a,b}[r][c] for |a - b| = 1
static double coupling_entry(const System& S, int a, int b, int r, int c) {
    if (r / 3 != c / 3) return 0.0;
    double e[3];
    coupling_coef(S, b, a - b, r, e[0], e[1], e[2]);
    return e[c % 3];
}

static void factorise(System& S) {  // twisted elimination, plain double
    const int nj = S.nj, mid = twist_mid(nj);
    S.M.assign((size_t)nj * NK * NK, 0.0), S.dinv.assign((size_t)nj * NK, 0.0);
    auto knot = [&](int j, const std::vector<double>& Usum) {
        std::vector<double> A(NK * NK), L(NK * NK, 0.0), d(NK), Li(NK * NK, 0.0);
        for (int i = 0; i < NK * NK; ++i) A[i] = S.T[(size_t)j * NK * NK + i] - Usum[i];
        for (int c = 0; c < NK; ++c) {
            d[c] = A[c * NK + c], L[c * NK + c] = 1;
            if (!(d[c] > 0)) printf("pivot not positive\n"), exit(1);
            for (int r = c + 1; r < NK; ++r) L[r * NK + c] = A[r * NK + c] / d[c];
            for (int r = c + 1; r < NK; ++r)
                for (int k = c + 1; k < NK; ++k) A[r * NK + k] -= L[r * NK + c] * d[c] * L[k * NK + c];
        }
        for (int c = 0; c < NK; ++c)
            for (int r = 0; r < NK; ++r) {
                double s = r == c ? 1.0 : 0.0;
                for (int k = 0; k < r; ++k) s -= L[r * NK + k] * Li[k * NK + c];
                Li[r * NK + c] = s;
            }
        for (int r = 0; r < NK; ++r)
            for (int k = 0; k < NK; ++k) S.M[(size_t)j * NK * NK + r * NK + k] = k >= r ? Li[k * NK + r] : 0.0;
        for (int r = 0; r < NK; ++r) S.dinv[j * NK + r] = 1.0 / d[r];
    };
    auto update_towards = [&](int j, int jn, std::vector<double>& Uo) {  // Uo += X D_j^-1 X', X = T_{jn,j} M_j
        std::vector<double> X(NK * NK);
        for (int r = 0; r < NK; ++r)
            for (int k = 0; k < NK; ++k) {
                double s = 0;
                for (int q = 0; q < NK; ++q) s += coupling_entry(S, jn, j, r, q) * S.M[(size_t)j * NK * NK + q * NK + k];
                X[r * NK + k] = s;
            }
        for (int r = 0; r < NK; ++r)
            for (int k = 0; k < NK; ++k) {
                double s = 0;
                for (int c = 0; c < NK; ++c) s += X[r * NK + c] * S.dinv[j * NK + c] * X[k * NK + c];
                Uo[r * NK + k] += s;
            }
    };
    std::vector<double> Umid(NK * NK, 0.0), Uc(NK * NK, 0.0);
    for (int j = 0; j < mid; ++j) {
        knot(j, Uc);
        std::fill(Uc.begin(), Uc.end(), 0.0);
        update_towards(j, j + 1, j + 1 == mid ? Umid : Uc);
    }
    std::fill(Uc.begin(), Uc.end(), 0.0);
    for (int j = nj - 1; j > mid; --j) {
        knot(j, Uc);
        std::fill(Uc.begin(), Uc.end(), 0.0);
        update_towards(j, j - 1, j - 1 == mid ? Umid : Uc);
    }
    knot(mid, Umid);
}

static System make(int nj) {
    System S;
    S.nj = nj;
    srand(11 + nj);
    S.T.resize((size_t)nj * NK * NK), S.Ek.assign((size_t)nj * 9, 0.0), S.rhs.resize((size_t)nj * NK);
    for (int j = 0; j < nj; ++j) {
        std::vector<double> B(NK * NK);
        for (auto& v : B) v = rnd();
        for (int r = 0; r < NK; ++r)
            for (int k = 0; k < NK; ++k) {
                double s = 0;
                for (int q = 0; q < NK; ++q) s += B[r * NK + q] * B[k * NK + q];
                S.T[(size_t)j * NK * NK + r * NK + k] = s + (r == k ? 30.0 + 1e4 * (r % 5 == 0) : 0.0);  // some large diagonal entries, like interior-point weights
            }
        if (j > 0)
            for (int e = 0; e < 9; ++e) S.Ek[9 * j + e] = 3.0 * rnd();
        for (int r = 0; r < NK; ++r) S.rhs[j * NK + r] = 10.0 * rnd();
    }
    factorise(S);
    return S;
}

// ---- the 64 lanes ------------------------------------------------------------------------------------------------------------------
static pthread_barrier_t bar;
struct Sync {
    void operator()() const { pthread_barrier_wait(&bar); }
};
constexpr int SM = NK * KL_LD, LEAD = 16;
struct Shared {
    const System* S;
    // FULL / backward: one stage buffer per chain (LEAD zeros, M, 1 / d, zeros behind), the vectors A, Z, V per chain with padding, partial sums
    std::vector<double> stage[2], small, vec;
    // SPLIT forward: one area per chain (C region, MX with its padding row, I, NaNs behind), z / x_mid in a "global" vector
    std::vector<double> area[2], gl;
    std::vector<double> x_full, x_split;
};
constexpr int CSZ = KfSlots<NK>::CSZ, MXO = CSZ, IO = MXO + (NK + 1) * KL_LD, AREA = IO + KL_I, AREA_ALLOC = AREA + 10 * KL_LD;
static void load_stage(std::vector<double>& st, const System& S, int j) {  // what the staging waves do: the upper triangle and 1 / d
    for (int r = 0; r < NK; ++r)
        for (int k = r; k < NK; ++k) st[LEAD + r * KL_LD + k] = S.M[(size_t)j * NK * NK + r * NK + k];
    for (int r = 0; r < NK; ++r) st[LEAD + SM + r] = S.dinv[j * NK + r];
}
static void load_area(std::vector<double>& ar, const System& S, int j) {  // what the companion's scatter and the factorisation leave
    for (int r = 0; r < NK; ++r)
        for (int k = 0; k < NK; ++k) ar[MXO + r * KL_LD + k] = k >= r ? S.M[(size_t)j * NK * NK + r * NK + k] : 0.0;
    for (int r = 0; r < NK; ++r) ar[IO + r] = S.dinv[j * NK + r];
    for (int i = 0; i < KfSlots<NK>::PAD; ++i) ar[i] = 1e3 * (i % 7) - 2e3;  // the next block's panel images over A and the partial sums
}

struct LaneArg {
    Shared* sh;
    int lane;
};

static void* lane_main(void* arg) {
    Shared& sh = *((LaneArg*)arg)->sh;
    const System& S = *sh.S;
    const int r = ((LaneArg*)arg)->lane, nj = S.nj, mid = twist_mid(nj), nl = mid, nr = nj - 1 - mid, SF = nl > nr ? nl : nr;
    const bool act = r < NK;
    const int rr = act ? r : 0, g3 = 3 * (rr / 3), r3 = rr % 3, rs = act ? r : NK + 12;
    Sync sync;
    auto left_j = [&](int s) { return s < SF ? (s - (SF - nl) >= 0 ? s - (SF - nl) : -1) : (s == SF ? mid : (mid - 1 - (s - SF - 1) >= 0 ? mid - 1 - (s - SF - 1) : -1)); };
    auto right_j = [&](int s) { return s < SF ? (s - (SF - nr) >= 0 ? nj - 1 - (s - (SF - nr)) : -1) : (s == SF ? -1 : (mid + 1 + (s - SF - 1) <= nj - 1 ? mid + 1 + (s - SF - 1) : -1)); };
    auto whole = [&](int lane0, auto&& f) {  // one lane does the bookkeeping the other waves / the host do on the device, between two barriers
        sync();
        if (r == lane0) f();
        sync();
    };
    auto backward_coef = [&](int jb, int dir, double& q0, double& q1, double& q2) {  // step_coef of solve_staged, s > SF
        const double* E = S.Ek.data() + 9 * (dir > 0 ? jb + 1 : jb);
        q0 = dir > 0 ? E[3 * r3] : E[r3], q1 = dir > 0 ? E[3 * r3 + 1] : E[3 + r3], q2 = dir > 0 ? E[3 * r3 + 2] : E[6 + r3];
    };
    double* small = sh.small.data();
    auto chainvec = [&](int h, double*& A, double*& Z, double*& V, double*& ps) {
        A = small + KS_VPAD + (h == 0 ? 0 : 3 * KS_VLEN), Z = A + KS_VLEN, V = A + 2 * KS_VLEN, ps = small + 6 * KS_VLEN + (h == 0 ? 0 : 64);
    };
    auto middle_v = [&](double v, const double* V0, const double* V1) {  // the s == SF body of solve_staged up to its products
        if (mid > 0) {
            double e0, e1, e2;
            coupling_coef(S, mid - 1, +1, rr, e0, e1, e2);
            v -= e0 * V0[g3] + e1 * V0[g3 + 1] + e2 * V0[g3 + 2];
        }
        if (mid + 1 < nj) {
            double e0, e1, e2;
            coupling_coef(S, mid + 1, -1, rr, e0, e1, e2);
            v -= e0 * V1[g3] + e1 * V1[g3 + 1] + e2 * V1[g3 + 2];
        }
        return v;
    };
    auto backward_steps = [&](std::vector<double>& vec) {
        for (int s = SF + 1; s < 2 * SF + 1; ++s)
            for (int h = 0; h < 2; ++h) {
                const int jb = h == 0 ? left_j(s) : right_j(s), dir = h == 0 ? +1 : -1;
                if (jb < 0) continue;
                whole(0, [&] { load_stage(sh.stage[h], S, jb); });
                double *A, *Z, *V, *ps, e0, e1, e2;
                chainvec(h, A, Z, V, ps);
                backward_coef(jb, dir, e0, e1, e2);
                const double* Mst = sh.stage[h].data() + LEAD;
                const double x = ks_step_backward<NK>(Mst, Mst[SM + rr], vec.data() + jb * NK + rr, e0, e1, e2, A, Z, V, ps, r, g3, rs, sync);
                if (act) vec[jb * NK + r] = x;
            }
    };
    // ---- FULL
    whole(0, [&] { sh.vec = S.rhs, std::fill(sh.small.begin(), sh.small.end(), 0.0); });
    for (int s = 0; s < SF; ++s)
        for (int h = 0; h < 2; ++h) {
            const int jb = h == 0 ? left_j(s) : right_j(s), dir = h == 0 ? +1 : -1;
            if (jb < 0) continue;
            whole(0, [&] { load_stage(sh.stage[h], S, jb); });
            double *A, *Z, *V, *ps, e0 = 0, e1 = 0, e2 = 0;
            chainvec(h, A, Z, V, ps);
            const bool has_prev = h == 0 ? jb > 0 : jb + 1 < nj;
            if (has_prev) coupling_coef(S, jb - dir, dir, rr, e0, e1, e2);
            const double* Mst = sh.stage[h].data() + LEAD;
            ks_step_forward<NK>(Mst, Mst[SM + rr], sh.vec[jb * NK + rr], has_prev, e0, e1, e2, A, Z, V, ps, r, g3, rs, sync, [&](double z) {
                if (act) sh.vec[jb * NK + r] = z;
            });
        }
    {
        whole(0, [&] { load_stage(sh.stage[0], S, mid); });
        double *A0, *Z0, *V0, *ps, *A1, *Z1, *V1, *ps1;
        chainvec(0, A0, Z0, V0, ps), chainvec(1, A1, Z1, V1, ps1);
        const double* Mst = sh.stage[0].data() + LEAD;
        const double x = ks_step_middle<NK>(Mst, Mst + SM + rr, middle_v(sh.vec[mid * NK + rr], V0, V1), A0, Z0, ps, r, rs, sync);
        V0[rs] = x, V1[rs] = x;
        if (act) sh.vec[mid * NK + r] = x;
    }
    backward_steps(sh.vec);
    whole(0, [&] { sh.x_full = sh.vec; });
    // ---- SPLIT: forward out of the chains' areas, lanes without a row compute row 0's values and store them where lane 0 does
    using F = KfSlots<NK>;
    whole(0, [&] {
        sh.gl = S.rhs;
        for (int h = 0; h < 2; ++h) {
            std::fill(sh.area[h].begin(), sh.area[h].begin() + AREA, 0.0);
            std::fill(sh.area[h].begin() + AREA, sh.area[h].end(), std::numeric_limits<double>::quiet_NaN());
        }
    });
    for (int h = 0; h < 2; ++h) {
        const int count = h == 0 ? nl : nr, j0 = h == 0 ? 0 : nj - 1, dir = h == 0 ? +1 : -1;
        for (int i = 0, j = j0; i < count; ++i, j += dir) {
            whole(0, [&] { load_area(sh.area[h], S, j); });
            double e0, e1, e2;
            const bool first = i == 0;
            coupling_coef(S, first ? j : j - dir, dir, rr, e0, e1, e2);  // wave_forward_fetch
            e0 = first ? 0.0 : e0, e1 = first ? 0.0 : e1, e2 = first ? 0.0 : e2;
            double* C = sh.area[h].data();
            ks_step_forward<NK, true>((const double*)(C + MXO), C[IO + rr], sh.gl[j * NK + rr], true, e0, e1, e2, C + F::A, C + F::Z, C + F::V, C + F::PS, r, g3, rr, sync,
                                      [&](double z) { sh.gl[j * NK + rr] = z; });
        }
    }
    {
        whole(0, [&] { load_area(sh.area[0], S, mid); });
        double *Cl = sh.area[0].data(), *V0 = Cl + F::V, *V1 = sh.area[1].data() + F::V;
        const double x = ks_step_middle<NK, true>((const double*)(Cl + MXO), (const double*)(Cl + IO + rr), middle_v(sh.gl[mid * NK + rr], V0, V1), Cl + F::A, Cl + F::Z, Cl + F::PS, r, rr, sync);
        sync();
        sh.gl[mid * NK + rr] = x;
    }
    // backward only (solve_staged, rhs_mode 3)
    whole(0, [&] {
        sh.vec = sh.gl, std::fill(sh.small.begin(), sh.small.end(), 0.0);
        for (int t = 0; t < NK; ++t) small[KS_VPAD + 2 * KS_VLEN + t] = small[KS_VPAD + 5 * KS_VLEN + t] = sh.vec[mid * NK + t];
    });
    backward_steps(sh.vec);
    whole(0, [&] { sh.x_split = sh.vec; });
    return nullptr;
}

// reference: the whole system as a banded matrix, L D L' in long double
static std::vector<long double> reference(const System& S) {
    const int n = S.nj * NK, bw = 2 * NK;
    std::vector<long double> A((size_t)n * n, 0.0L), x(n);
    for (int j = 0; j < S.nj; ++j)
        for (int r = 0; r < NK; ++r) {
            for (int k = 0; k < NK; ++k) A[(size_t)(j * NK + r) * n + j * NK + k] = S.T[(size_t)j * NK * NK + r * NK + k];
            if (j > 0)
                for (int k = 0; k < NK; ++k) {
                    const double v = coupling_entry(S, j, j - 1, r, k);
                    A[(size_t)(j * NK + r) * n + (j - 1) * NK + k] = v, A[(size_t)((j - 1) * NK + k) * n + j * NK + r] = v;
                }
        }
    for (int i = 0; i < n; ++i) x[i] = S.rhs[i];
    for (int c = 0; c < n; ++c) {  // Gaussian elimination inside the band (symmetric positive definite: no pivoting)
        const int hi = c + bw < n ? c + bw : n;
        for (int r = c + 1; r < hi; ++r) {
            const long double l = A[(size_t)r * n + c] / A[(size_t)c * n + c];
            if (l == 0.0L) continue;
            for (int k = c; k < hi; ++k) A[(size_t)r * n + k] -= l * A[(size_t)c * n + k];
            x[r] -= l * x[c];
        }
    }
    for (int c = n - 1; c >= 0; --c) {
        const int hi = c + bw < n ? c + bw : n;
        long double s = x[c];
        for (int k = c + 1; k < hi; ++k) s -= A[(size_t)c * n + k] * x[k];
        x[c] = s / A[(size_t)c * n + c];
    }
    return x;
}

int main() {
    bool pass = true;
    for (int nj : {1, 2, 3, 4, 5, 8, 35}) {
        const System S = make(nj);
        Shared sh;
        sh.S = &S;
        for (int h = 0; h < 2; ++h) sh.stage[h].assign(LEAD + SM + KL_I + 10 * KL_LD, 0.0), sh.area[h].assign(AREA_ALLOC, 0.0);
        sh.small.assign(6 * KS_VLEN + 2 * 64, 0.0);
        pthread_barrier_init(&bar, nullptr, LANES);
        pthread_t th[LANES];
        LaneArg args[LANES];
        for (int l = 0; l < LANES; ++l) args[l] = LaneArg{&sh, l}, pthread_create(&th[l], nullptr, lane_main, &args[l]);
        for (int l = 0; l < LANES; ++l) pthread_join(th[l], nullptr);
        pthread_barrier_destroy(&bar);
        const std::vector<long double> ref = reference(S);
        const int n = nj * NK;
        int differ = 0;
        double e_full = 0, e_split = 0, scale = 0;
        for (int i = 0; i < n; ++i) {
            differ += std::memcmp(&sh.x_full[i], &sh.x_split[i], sizeof(double)) != 0;
            e_full = std::fmax(e_full, (double)fabsl(sh.x_full[i] - ref[i])), e_split = std::fmax(e_split, (double)fabsl(sh.x_split[i] - ref[i]));
            scale = std::fmax(scale, (double)fabsl(ref[i]));
        }
        // (the bound on the distance only keeps a restatement that is wrong in both routes from passing: diagonal >= 30, a few thousand unknowns,
        // condition below 1e4: 1e-9 relative is orders above what either route leaves, and a NaN fails it)
        const bool ok = differ == 0 && e_full <= 1e-9 * scale;
        printf("nj %2d: %d of %d entries differ between the full and the split substitution; max |x - long double| full %.3g split %.3g (scale %.3g)  %s\n", nj, differ, n,
               e_full, e_split, scale, ok ? "ok" : "MISMATCH");
        pass = pass && ok;
    }
    printf("%s\n", pass ? "knot subst ok" : "FAIL");
    return pass ? 0 : 1;
}
