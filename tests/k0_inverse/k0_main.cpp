// The per-mission table G = K0^-1 of the polish (csrc/common/ipm_rows.h: k0_inverse_column, k0g_symmetrise, k0g_at) as the host compiler
// builds it, against a dense inverse in long double.  K0 is assembled densely from D_j, E_j, which are restated here from the segment
// times the way kernels/qp.hip's mission_constants derives them.  The bound is relative to the route the table replaces: full
// forward / backward solves on unit vectors with the same factor.  See tests/test_k0_inverse.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common/ipm_rows.h"

using namespace ipm;
typedef long double ld;

static int failures = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x), failures++; \
    } while (0)

// D_j, E_j of knots j = 1 .. M - 1 (kernels/qp.hip: mission_constants), nj = M - 1 blocks
static void constants(const std::vector<double>& T, std::vector<double>& Dk, std::vector<double>& Ek) {
    const int M = (int)T.size() - 1;
    std::vector<double> Lk(9 * (M + 1), 0.0);
    Dk.assign(9 * (M + 1), 0.0), Ek.assign(9 * (M + 1), 0.0);
    for (int j = 1; j < M; ++j) {
        double* L = &Lk[9 * j];
        const double r = (T[j] - T[j - 1]) / (T[j + 1] - T[j]);
        L[0] = (1 + r) * (1 + r), L[1] = -2 * r * (1 + r), L[2] = r * r, L[3] = 1 + r, L[4] = -r, L[5] = 0, L[6] = 1, L[7] = 0, L[8] = 0;
    }
    for (int j = 1; j < M; ++j) {
        const double sl = pow(T[j] - T[j - 1], -5.0), sr = pow(T[j + 1] - T[j], -5.0);
        const double* L = &Lk[9 * j];
        double QL[9];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double s = 0;
                for (int c = 0; c < 3; ++c) s += Qbase[6 * (3 + a) + 3 + c] * sl * L[3 * c + b];
                QL[3 * a + b] = s;
            }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double s = 0;
                for (int c = 0; c < 3; ++c) s += L[3 * c + a] * QL[3 * c + b];
                Dk[9 * j + 3 * a + b] = 2 * (s + Qbase[6 * a + b] * sr);
            }
        if (j + 1 < M) {
            const double* Ln = &Lk[9 * (j + 1)];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    double s = 0;
                    for (int c = 0; c < 3; ++c) s += Qbase[6 * a + 3 + c] * sr * Ln[3 * c + b];
                    Ek[9 * j + 3 * a + b] = 2 * s;  // rows u_j, cols u_{j+1}
                }
        }
    }
}

// dense inverse in long double (Gauss-Jordan with partial pivoting)
static std::vector<ld> inverse(std::vector<ld> A, int n) {
    std::vector<ld> X(n * n, 0.0L);
    for (int i = 0; i < n; ++i) X[i * n + i] = 1;
    for (int k = 0; k < n; ++k) {
        int piv = k;
        for (int i = k + 1; i < n; ++i)
            if (fabsl(A[i * n + k]) > fabsl(A[piv * n + k])) piv = i;
        for (int c = 0; c < n; ++c) std::swap(A[k * n + c], A[piv * n + c]), std::swap(X[k * n + c], X[piv * n + c]);
        const ld ip = 1 / A[k * n + k];
        for (int c = 0; c < n; ++c) A[k * n + c] *= ip, X[k * n + c] *= ip;
        for (int i = 0; i < n; ++i) {
            if (i == k) continue;
            const ld m = A[i * n + k];
            if (m == 0) continue;
            for (int c = 0; c < n; ++c) A[i * n + c] -= m * A[k * n + c], X[i * n + c] -= m * X[k * n + c];
        }
    }
    return X;
}

static ld residual(const std::vector<ld>& K, const std::vector<ld>& X, int n) {  // max |K X - I|
    ld worst = 0;
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < n; ++c) {
            ld s = i == c ? -1.0L : 0.0L;
            for (int k = 0; k < n; ++k) s += K[i * n + k] * X[k * n + c];
            worst = fmaxl(worst, fabsl(s));
        }
    return worst;
}

static void one_case(const char* name, const std::vector<double>& T) {
    const int M = (int)T.size() - 1, nj = M - 1, n = 3 * nj;
    std::vector<double> Dk, Ek;
    constants(T, Dk, Ek);
    std::vector<ld> K(n * n, 0.0L);
    for (int jj = 0; jj < nj; ++jj) {
        const int j = jj + 1;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                K[(3 * jj + r) * n + 3 * jj + c] = Dk[9 * j + 3 * r + c];
                if (jj + 1 < nj) K[(3 * jj + r) * n + 3 * (jj + 1) + c] = K[(3 * (jj + 1) + c) * n + 3 * jj + r] = Ek[9 * j + 3 * r + c];
            }
    }
    const std::vector<ld> Kinv = inverse(K, n);
    // the factor, as k0_factor3 forms it
    std::vector<double> f(18 * nj);
    double Bp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int jj = 0; jj < nj; ++jj) {
        for (int e = 0; e < 9; ++e) f[18 * jj + e] = Dk[9 * (jj + 1) + e], f[18 * jj + 9 + e] = jj + 1 < nj ? Ek[9 * (jj + 1) + e] : 0.0;
        CHECK(k0_factor_step(&f[18 * jj], Bp, jj == 0));
    }
    // the route the table replaces: K0^-1 e_i by a full forward and backward pass
    std::vector<ld> Xsolve(n * n);
    for (int col = 0; col < n; ++col) {
        std::vector<double> y(n, 0.0);
        y[col] = 1.0;
        double p[3] = {0, 0, 0};
        for (int jj = 0; jj < nj; ++jj) {
            double v[3] = {y[3 * jj], y[3 * jj + 1], y[3 * jj + 2]};
            k0_forward_step((const double*)&f[18 * jj], jj > 0, v, p);
            for (int e = 0; e < 3; ++e) y[3 * jj + e] = p[e] = v[e];
        }
        for (int jj = nj - 1; jj >= 0; --jj) {
            double v[3] = {y[3 * jj], y[3 * jj + 1], y[3 * jj + 2]};
            k0_backward_step((const double*)&f[18 * jj], jj + 1 < nj, v, p);
            for (int e = 0; e < 3; ++e) y[3 * jj + e] = p[e] = v[e];
        }
        for (int i = 0; i < n; ++i) Xsolve[i * n + col] = y[i];
    }
    // the table
    std::vector<dd> fd(18 * nj);
    dd Bd[9];
    for (int jj = 0; jj < nj; ++jj) {
        for (int e = 0; e < 9; ++e) fd[18 * jj + e] = dd(Dk[9 * (jj + 1) + e]), fd[18 * jj + 9 + e] = dd(jj + 1 < nj ? Ek[9 * (jj + 1) + e] : 0.0);
        CHECK(k0_factor_step(&fd[18 * jj], Bd, jj == 0));
    }
    std::vector<double> G(k0g_doubles(nj), -7.0), lo(k0g_doubles(nj), -7.0);
    for (int col = 0; col < n; ++col) k0_inverse_column((const dd*)fd.data(), nj, col / 3, col % 3, G.data(), lo.data());
    for (int jj = 0; jj < nj; ++jj) k0g_symmetrise(&G[k0g_block(jj, jj)]);
    std::vector<ld> Xtab(n * n);
    ld amax = 0, err_tab = 0, err_solve = 0;
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < n; ++c) {
            const double g = k0g_at((const double*)G.data(), i / 3, i % 3, c / 3, c % 3);
            // exact symmetry of what the polish reads, and of the stored diagonal blocks
            CHECK(g == k0g_at((const double*)G.data(), c / 3, c % 3, i / 3, i % 3));
            Xtab[i * n + c] = g;
            amax = fmaxl(amax, fabsl(Kinv[i * n + c]));
            err_tab = fmaxl(err_tab, fabsl(g - Kinv[i * n + c]));
            err_solve = fmaxl(err_solve, fabsl(Xsolve[i * n + c] - Kinv[i * n + c]));
        }
    for (int jj = 0; jj < nj; ++jj) {
        const double* b = &G[k0g_block(jj, jj)];
        CHECK(b[1] == b[3] && b[2] == b[6] && b[5] == b[7]);
    }
    const ld res_tab = residual(K, Xtab, n), res_solve = residual(K, Xsolve, n), res_ref = residual(K, Kinv, n);
    printf("%-34s nj %2d  max|K0 G - I|: table %.3Le  unit-vector solves %.3Le  (long double inverse %.1Le)   max|G - K0^-1| / max|K0^-1|: table %.3Le  solves %.3Le\n",
           name, nj, res_tab, res_solve, res_ref, err_tab / amax, err_solve / amax);
    // a few ulps for the symmetrisation and the shortened forward pass, not orders of magnitude
    CHECK(res_tab <= 4 * res_solve);
    CHECK(err_tab <= 4 * err_solve);
}

int main() {
    const int njs[5] = {1, 2, 3, 7, 35};
    for (int q = 0; q < 5; ++q) {
        const int M = njs[q] + 1;
        char name[64];
        std::vector<double> T(M + 1);
        for (int m = 0; m <= M; ++m) T[m] = m;
        snprintf(name, sizeof name, "unit times");
        one_case(name, T);
        // knot ratios dl / dr above and below 1: segment lengths 0.6 .. 1.7, neither monotone nor periodic in the knot
        T[0] = 0.25;
        for (int m = 0; m < M; ++m) T[m + 1] = T[m] + 0.6 + 1.1 * ((m * 7 + 3) % 5) / 4.0;
        snprintf(name, sizeof name, "segments 0.6 .. 1.7, mixed ratios");
        one_case(name, T);
        for (int m = 0; m < M; ++m) T[m + 1] = T[m] + (m % 2 ? 2.0 : 0.5);  // ratios 4 and 1/4 alternating
        snprintf(name, sizeof name, "segments 0.5 / 2 alternating");
        one_case(name, T);
    }
    if (failures) return printf("%d checks failed\n", failures), 1;
    printf("k0 inverse ok\n");
    return 0;
}
