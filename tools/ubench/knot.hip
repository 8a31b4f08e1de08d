// Developer test + timing of kernels/knot_lds.inc in the arrangement the product runs (qp.hip, wave_factor_chain / knot_inverse): a chain
// wave and its companion wave on different SIMDs of ONE workgroup, synchronised by the progress words, over a chain of knot steps,
// against a host restatement.  NK = 9, 18, 27, 36; diagonal spreads 1e4 and 1e8 (the spread of an interior-point system).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I../../swarm_simulator_amd/csrc/kernels -DKL_PANEL=1 -o knot knot.hip && ./knot
// -DKL_PANEL=0: the column loop (kl_ldl / kl_follow_LinvT) for every NK; -DKL_PANEL=1: the panel path where kl_panel_path(NK) says so
// (-DKL_PANEL_MIN_NK=9: for every NK).  On the panel path the rank-NK update of the next block is formed in the MFMA tiles straight from M
// (kl_fused_update: no coupling rows, no stored X or U, M announced early); -DKL_FUSED_UPDATE=0 is the path with kl_coupling_rows / kl_syrk.
// Where X is not materialised the check is on the NEXT block's Schur complement T - X D^-1 X' instead (the tiles after the last step's
// update, with the first step's T standing in for the next block's).  -DUB_T_FIRST=1 (fused path, this tool only): T into the tiles first and
// the update on top, instead of the update from zero and T added afterwards (what the product does: its update runs before T's image is there).
// -DUB_FWD=1 (default; fused path): the chain also takes the forward substitution step of the block it has just factorised out of its own
// area, between the update of the next block and that block's T (kl_forward_step: qp.hip's QP_FWD_IN_FACTOR), chains of 1, 2, 3 and 17 knots
// as well; z_j and the last v are checked against a host restatement that uses the device's own M_j and 1 / d_j.  -DUB_FWD=0: without.
// One workgroup per launch; run it under a time limit of its own.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knot_lds.inc"

#ifndef UB_T_FIRST
#define UB_T_FIRST 0
#endif
#ifndef UB_FWD
#define UB_FWD 1
#endif
constexpr int STEPS = 6, MAXSTEPS = 17;  // STEPS: the chain every check runs; MAXSTEPS: the longest of the forward-step chains

// timers of the chain wave, cycles per knot step: [0] whole step, [1] syrk, [2] load + factorisation, [3] start of the factorisation ->
// "M rows are in MX" (what the chain waits for), [4] coupling rows; [5] of the companion wave: its whole step
// fused path: [1] the update in the tiles, [2] T into the tiles + factorisation, [3] as above, [4] what is left of the chain's wait for M
// once the factorisation is over (the gap between [2] and [3]); [0] is the sum of [1], [2], [4] and [6]; [6] the forward step (UB_FWD)
struct Timers {
    long long v[8];
};

// the diagonal block of one knot, as knot_ldl of qp.hip forms it: S = T_j (- U), factorised
template <int NK>
__device__ __forceinline__ bool ub_knot_ldl(const double* Tg, bool minus_u, kl_lds* base, int r, bool act, int rr, kl_ldsi* P, int pbase) {
    using A = KlArea<NK>;
    kl_lds *C = base + A::C, *I = base + A::I, *U = base + A::C;
    (void)U;
    if constexpr (kl_panel_path(NK)) {
        return kl_knot_panels<NK, false>([&](int mx, int mn) { return Tg[mn * NK + mx]; }, [] {}, minus_u, C, I, r, P, pbase);
    } else {
        double a[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) a[k] = Tg[k * NK + rr];
        if (minus_u) {
#pragma unroll
            for (int k = 0; k < NK; ++k) a[k] -= U[rr * KL_LDU + k];
            kl_sync();
        }
        return kl_ldl<NK>(a, C, I, r, act, P, pbase);
    }
}

// T: [STEPS][NK*NK] element (r,k) at k*NK + r (symmetric); E: [STEPS][9]; out M: [STEPS][NK*NK] row-major, X: element (r,k) at k*NK + r (last step),
// dinv [STEPS][NK].  256 threads: waves 0, 1 = chains, waves 2, 3 = their companions (only `pairs` of them work; pair 0 is checked)
template <int NK>
__global__ __launch_bounds__(256) void pair_kernel(const double* T, const double* E, double* Mo, double* Xo, double* Do, Timers* tm, int* okflag, int pairs, int steps, const double* rhs, double* Zo,
                                                   double* Vo) {
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    using A = KlArea<NK>;
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 63, h = wave & 1;
    const bool follower = wave >= 2;
    kl_ldsi* words = (kl_ldsi*)(lds_raw + 2 * A::SIZE);
    for (int i = threadIdx.x; i < 2 * A::SIZE + 8; i += 256) lds_raw[i] = 0.0;
    __syncthreads();
    if (h >= pairs) return;
    kl_lds* base = (kl_lds*)(lds_raw + h * A::SIZE);
    kl_lds *C = base + A::C, *MX = base + A::MX, *I = base + A::I, *U = base + A::C;
    kl_ldsi *P = words + 2 * h, *Mdone = P + 1;
    const bool act = r < NK;
    const int rr = act ? r : 0;
    long long t_all = 0, t_syrk = 0, t_fac = 0, t_m = 0, t_x = 0, t_fwd = 0;
    if constexpr (kl_fused_path(NK)) {
        if (!follower) {  // wave_factor_chain of qp.hip, fused path
            using KP = KlPanels<NK>;
            bool ok = true;
            int seen = 0;
            double cf[KP::NT][3];
            kl_d4 s[KP::TILES];
            const int li = r & 15, lk = r >> 4;
            // S_i = T_i - X D^-1 X' from block i - 1's M, in two halves around the point where the product waits for T_i's image
            auto update = [&](int i, bool prev) {
                const double* Tg = T + (size_t)i * NK * NK;
                if (UB_T_FIRST)
                    kl_tiles_load<NK, 0, false>(s, r, [&](int mx, int mn) { return Tg[mn * NK + mx]; });
                else
                    kl_tiles_zero<NK>(s);
                if (prev) kl_fused_update<NK>(s, MX, I, r, cf);
            };
            auto add_t = [&](int i) {
                const double* Tg = T + (size_t)i * NK * NK;
                if (!UB_T_FIRST) kl_tiles_load<NK, 2, false>(s, r, [&](int mx, int mn) { return Tg[mn * NK + mx]; });
            };
            long long c_fac0 = 0;
            [[maybe_unused]] double f_rhs = 0, f_e0 = 0, f_e1 = 0, f_e2 = 0;
            // the forward step of block i - 1 (wave_forward_step of qp.hip): z to Zo, v stays in the area
            auto forward = [&](int i) {
                const long long f0 = __builtin_readcyclecounter();
                if (UB_FWD) kl_forward_step<NK>(base, (__attribute__((address_space(1))) double*)(Zo + (size_t)(i - 1) * NK + rr), f_rhs, f_e0, f_e1, f_e2, r);
                const long long f1 = __builtin_readcyclecounter();
                t_fwd += f1 - f0, t_all += f1 - f0;
            };
            for (int i = 0; i <= steps; ++i) {
                const long long c0 = __builtin_readcyclecounter();
                if (i > 0) kl_await(Mdone, i, seen);
                const long long c1 = __builtin_readcyclecounter();
                if (i > 0) t_m += c1 - c_fac0, t_x += c1 - c0, t_all += c1 - c0;
                if (i == steps) {  // (the last block's M: without the forward steps the product leaves this wait to the workgroup barrier in front of the middle block)
                    forward(i);
                    break;
                }
                update(i, i > 0);
                if (i > 0) forward(i);
                const long long c2 = __builtin_readcyclecounter();
                const double* Ei = E + 9 * i;
                kl_fused_coef<NK>(cf, r, [&](int row, int q) { return Ei[3 * q + row % 3]; });  // T_{j+1,j}[r][3g+q] = E[q][r%3]
                add_t(i);
                if (!kl_ldl_panels<NK>(s, C, I, r, P, i * (NK + 1))) ok = false;
                const long long c3 = __builtin_readcyclecounter();
                if (UB_FWD) {  // wave_forward_fetch of qp.hip: what block i's step starts from, requested when the block is factorised
                    const double* Ep = E + 9 * (i > 0 ? i - 1 : 0);
                    f_rhs = rhs[(size_t)i * NK + rr];
                    f_e0 = i > 0 ? Ep[rr % 3] : 0.0, f_e1 = i > 0 ? Ep[3 + rr % 3] : 0.0, f_e2 = i > 0 ? Ep[6 + rr % 3] : 0.0;  // row rr of T_{i,i-1}
                }
                c_fac0 = c2;
                t_syrk += c2 - c1, t_fac += c3 - c2, t_all += c3 - c1;
            }
            if (UB_FWD && h == 0 && act) Vo[r] = (base + A::C + KfSlots<NK>::V)[r];  // the chain's last v
            // the check: the tiles the NEXT block would factorise, with the first step's T standing in for its T (upper triangle, row-major)
            update(0, true), add_t(0);
            if (h == 0) {
#pragma unroll
                for (int ti = 0; ti < KP::NT; ++ti)
#pragma unroll
                    for (int tj = ti; tj < KP::NT; ++tj)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int row = KP_T * ti + lk + 4 * g, col = KP_T * tj + li;
                            if (row < NK && col < NK && row <= col) Xo[(size_t)(steps - 1) * NK * NK + row * NK + col] = s[kp_upper(ti, tj, KP::NT)][g];
                        }
            }
            if (r == 0 && h == 0) tm->v[0] = t_all / steps, tm->v[1] = t_syrk / steps, tm->v[2] = t_fac / steps, tm->v[3] = t_m / steps, tm->v[4] = t_x / steps, tm->v[6] = t_fwd / steps;
            if (!ok && r == 0) *okflag = 1;
            return;
        }
    }
    if (!follower) {
        bool ok = true;
        int seen = 0;
        for (int i = 0; i < STEPS; ++i) {
            const long long c0 = __builtin_readcyclecounter();
            if (i > 0) kl_syrk<NK>(MX, I, U, r, false);
            const long long c1 = __builtin_readcyclecounter();
            const double* Ei = E + 9 * i;
            const double e0 = Ei[rr % 3], e1 = Ei[3 + rr % 3], e2 = Ei[6 + rr % 3];  // T_{j+1,j}[r][3g+q] = E[q][r%3]
            if (!ub_knot_ldl<NK>(T + (size_t)i * NK * NK, i > 0, base, r, act, rr, P, i * (NK + 1))) ok = false;
            const long long c2 = __builtin_readcyclecounter();
            kl_await(Mdone, i + 1, seen);
            const long long c3 = __builtin_readcyclecounter();
            double x[NK];
            kl_coupling_rows<NK>(x, MX, r, act, e0, e1, e2);
            if (act && h == 0 && i == STEPS - 1) {  // (the product does not store X: checked here on the last step only)
#pragma unroll
                for (int k = 0; k < NK; ++k) Xo[(size_t)i * NK * NK + k * NK + r] = x[k];
            }
            const long long c4 = __builtin_readcyclecounter();
            t_syrk += c1 - c0, t_fac += c2 - c1, t_m += c3 - c1, t_x += c4 - c3, t_all += c4 - c0;
        }
        if (r == 0 && h == 0) tm->v[0] = t_all / STEPS, tm->v[1] = t_syrk / STEPS, tm->v[2] = t_fac / STEPS, tm->v[3] = t_m / STEPS, tm->v[4] = t_x / STEPS;
        if (!ok && r == 0) *okflag = 1;
    } else {
        for (int i = 0; i < steps; ++i) {  // knot_inverse<NK, true> of qp.hip
            const long long c0 = __builtin_readcyclecounter();
            double m[NK];
            const double dinv = kl_inverse_rows<NK, true>(m, C, I, MX, r, act, P, i * (NK + 1), Mdone, i + 1);  // (announces M)
            if (act && h == 0) {  // row r of M = L^-T, entries k >= r: pairs, 16 bytes per lane and instruction
                double* Mr = Mo + (size_t)i * NK * NK + (size_t)r * NK;
                if ((NK & 1) == 0) {
#pragma unroll
                    for (int k = 0; k < NK; k += 2)
                        if (k + 1 >= r) *(kl_d2*)(Mr + k) = kl_d2{m[k], m[k + 1]};
                } else {
#pragma unroll
                    for (int k = 0; k < NK; ++k)
                        if (k >= r) Mr[k] = m[k];
                }
                Do[i * NK + r] = dinv;
            }
            t_all += __builtin_readcyclecounter() - c0;
        }
        if (r == 0 && h == 0) tm->v[5] = t_all / steps;
    }
}

static double rnd() { return rand() / (double)RAND_MAX - 0.5; }

template <int NK>
static bool run(double spread, bool timing) {
    std::vector<double> T(STEPS * NK * NK), E(STEPS * 9);
    srand(7 + NK);
    for (int i = 0; i < STEPS; ++i) {
        std::vector<double> B(NK * NK);
        for (auto& v : B) v = rnd();
        for (int r = 0; r < NK; ++r)
            for (int k = 0; k < NK; ++k) {
                double s = 0;
                for (int q = 0; q < NK; ++q) s += B[r * NK + q] * B[k * NK + q];
                T[(size_t)i * NK * NK + k * NK + r] = s + (r == k ? 30.0 + spread * (r % 5 == 0) : 0.0);  // SPD, some large diagonal entries like IPM weights
            }
        for (int e = 0; e < 9; ++e) E[9 * i + e] = 3.0 * rnd();
    }
    // host restatement
    std::vector<double> Mh(STEPS * NK * NK), Xh(STEPS * NK * NK), Dh(STEPS * NK), Ulast;
    {
        std::vector<double> U(NK * NK, 0.0);
        for (int i = 0; i < STEPS; ++i) {
            std::vector<double> A(NK * NK), L(NK * NK, 0.0), d(NK);
            for (int r = 0; r < NK; ++r)
                for (int k = 0; k < NK; ++k) A[r * NK + k] = T[(size_t)i * NK * NK + k * NK + r] - (i > 0 ? U[r * NK + k] : 0.0);
            for (int c = 0; c < NK; ++c) {
                d[c] = A[c * NK + c];
                L[c * NK + c] = 1;
                for (int r = c + 1; r < NK; ++r) L[r * NK + c] = A[r * NK + c] / d[c];
                for (int r = c + 1; r < NK; ++r)
                    for (int k = c + 1; k < NK; ++k) A[r * NK + k] -= L[r * NK + c] * d[c] * L[k * NK + c];
            }
            // M = L^-T: solve L' M = I  -> M[r][k]: row r of L^-T = column r of L^-1
            std::vector<double> Li(NK * NK, 0.0);
            for (int c = 0; c < NK; ++c) {  // column c of L^-1
                for (int r = 0; r < NK; ++r) {
                    double s = (r == c) ? 1.0 : 0.0;
                    for (int k = 0; k < r; ++k) s -= L[r * NK + k] * Li[k * NK + c];
                    Li[r * NK + c] = s;
                }
            }
            for (int r = 0; r < NK; ++r)
                for (int k = 0; k < NK; ++k) Mh[(size_t)i * NK * NK + r * NK + k] = Li[k * NK + r];  // M[r][k] = Li[k][r], row-major
            for (int r = 0; r < NK; ++r) Dh[i * NK + r] = 1.0 / d[r];
            std::vector<double> X(NK * NK);
            for (int r = 0; r < NK; ++r)
                for (int k = 0; k < NK; ++k) {
                    double s = 0;
                    for (int q = 0; q < 3; ++q) s += E[9 * i + 3 * q + r % 3] * Li[k * NK + 3 * (r / 3) + q];
                    X[r * NK + k] = s;
                    Xh[(size_t)i * NK * NK + k * NK + r] = s;
                }
            for (int r = 0; r < NK; ++r)
                for (int k = 0; k < NK; ++k) {
                    double s = 0;
                    for (int c = 0; c < NK; ++c) s += X[r * NK + c] / d[c] * X[k * NK + c];
                    U[r * NK + k] = s;
                }
        }
        Ulast = U;
    }
    double *dT, *dE, *dM, *dX, *dD, *dR, *dZ, *dV;  // (dR, dZ, dV: right-hand side, z and last v of the forward steps, checked by run_forward)
    Timers* dt;
    int* dok;
    bool hip_ok = true;
    auto ck = [&](hipError_t e) { if (e != hipSuccess) hip_ok = false; };
    ck(hipMalloc(&dT, T.size() * 8)), ck(hipMalloc(&dE, E.size() * 8)), ck(hipMalloc(&dM, Mh.size() * 8)), ck(hipMalloc(&dX, Xh.size() * 8)), ck(hipMalloc(&dD, Dh.size() * 8));
    ck(hipMalloc(&dt, sizeof(Timers))), ck(hipMalloc(&dok, 4));
    ck(hipMalloc(&dR, STEPS * NK * 8)), ck(hipMalloc(&dZ, STEPS * NK * 8)), ck(hipMalloc(&dV, NK * 8));
    if (hip_ok) ck(hipMemset(dR, 0, STEPS * NK * 8));
    if (!hip_ok) {
        printf("NK %d: allocation failed\nFAIL\n", NK);
        exit(2);  // nothing more is started on a device that failed
    }
    ck(hipMemcpy(dT, T.data(), T.size() * 8, hipMemcpyHostToDevice)), ck(hipMemcpy(dE, E.data(), E.size() * 8, hipMemcpyHostToDevice));
    ck(hipMemset(dok, 0, 4)), ck(hipMemset(dM, 0, Mh.size() * 8)), ck(hipMemset(dX, 0, Xh.size() * 8)), ck(hipMemset(dD, 0, Dh.size() * 8));
    const size_t lds = (2 * KlArea<NK>::SIZE + 8 + 10 * KL_LD) * sizeof(double);  // (+ what the second chain's guarded product reads behind its area: never cleared)
    ck(hipFuncSetAttribute((const void*)pair_kernel<NK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int pairs : {1, 2}) {
        if (!timing && pairs == 2) break;
        Timers h{};
        for (int rep = 0; rep < 2 && hip_ok; ++rep) {  // (the second launch is the one reported: warm instruction cache)
            hipLaunchKernelGGL(pair_kernel<NK>, dim3(1), dim3(256), lds, 0, dT, dE, dM, dX, dD, dt, dok, pairs, STEPS, dR, dZ, dV);
            ck(hipDeviceSynchronize());
        }
        if (!hip_ok) {
            printf("NK %d: launch failed\nFAIL\n", NK);
            exit(2);
        }
        ck(hipMemcpy(&h, dt, sizeof(h), hipMemcpyDeviceToHost));
        if (timing && kl_fused_path(NK))
            printf("NK %d panels, %d chain + companion pair%s: cycles per knot step %lld  (fused update %lld, T + factorisation %lld, factorisation start -> M announced %lld, "
                   "chain waits for M %lld; companion step %lld; forward step (UB_FWD=%d) %lld)\n",
                   NK, pairs, pairs > 1 ? "s" : "", h.v[0], h.v[1], h.v[2], h.v[3], h.v[4], h.v[5], UB_FWD, h.v[6]);
        else if (timing)
            printf("NK %d %s, %d chain + companion pair%s: cycles per knot step %lld  (syrk %lld, load + factorisation %lld, factorisation start -> M rows in MX %lld, "
                   "coupling rows %lld; companion step %lld)\n",
                   NK, kl_panel_path(NK) ? "panels" : "columns", pairs, pairs > 1 ? "s" : "", h.v[0], h.v[1], h.v[2], h.v[3], h.v[4], h.v[5]);
    }
    if (kl_fused_path(NK)) {  // X is not materialised: the last NK * NK slots hold the next block's Schur complement instead (upper triangle, row-major)
        const size_t o = (size_t)(STEPS - 1) * NK * NK;
        for (int r = 0; r < NK; ++r)
            for (int k = 0; k < NK; ++k) Xh[o + r * NK + k] = k >= r ? T[k * NK + r] - Ulast[r * NK + k] : 0.0;
    }
    std::vector<double> Mg(Mh.size()), Xg(Xh.size()), Dg(Dh.size());
    int okf = 1;
    ck(hipMemcpy(Mg.data(), dM, Mg.size() * 8, hipMemcpyDeviceToHost)), ck(hipMemcpy(Xg.data(), dX, Xg.size() * 8, hipMemcpyDeviceToHost));
    ck(hipMemcpy(Dg.data(), dD, Dg.size() * 8, hipMemcpyDeviceToHost)), ck(hipMemcpy(&okf, dok, 4, hipMemcpyDeviceToHost));
    hipFree(dT), hipFree(dE), hipFree(dM), hipFree(dX), hipFree(dD), hipFree(dt), hipFree(dok), hipFree(dR), hipFree(dZ), hipFree(dV);
    double em = 0, ex = 0, ed = 0, sm = 0, sx = 0;
    for (size_t i = 0; i < Mh.size(); ++i) {
        const int rr = (int)(i % (NK * NK)) / NK, kk = (int)(i % NK);
        if (((NK & 1) ? kk : (kk | 1)) >= rr) em = fmax(em, fabs(Mg[i] - Mh[i])), sm = fmax(sm, fabs(Mh[i]));  // only entries k >= r (pairs: k + 1 >= r) are stored
        if (i >= (size_t)(STEPS - 1) * NK * NK) ex = fmax(ex, fabs(Xg[i] - Xh[i])), sx = fmax(sx, fabs(Xh[i]));
    }
    for (size_t i = 0; i < Dh.size(); ++i) ed = fmax(ed, fabs(Dg[i] - Dh[i]) / fabs(Dh[i]));
    // (negated comparisons: a NaN fails)
    const bool pass = hip_ok && !okf && em < 1e-11 * fmax(1.0, sm) && ex < 1e-11 * fmax(1.0, sx) && ed < 1e-12;
    printf("NK %d spread %.0e: pivots positive: %s   max|M err| %.3g (scale %.3g)  max|%s err| %.3g (scale %.3g)  max rel 1/d err %.3g   %s\n", NK, spread,
           okf ? "NO" : "yes", em, sm, kl_fused_path(NK) ? "next S" : "X", ex, sx, ed, pass ? "ok" : "MISMATCH");
    return pass;
}

// The forward steps along a chain of `steps` knots (NK = 36, fused path): z_j and the chain's last v against a host restatement that uses the
// DEVICE's M_j and 1 / d_j -- what is checked is the step, in plain loops: r' = rhs_j - T_{j,j-1} v_{j-1}, z = D^-1 M' r', v = M z.  Both
// products sum at most 36 terms in another order than the device's pieces: 1e-12 of the scale is a hundred times their rounding.
// With UB_FWD=0 the chain runs all the same (a hang would show) and nothing is compared.
static bool run_forward(int steps) {
    constexpr int NK = 36;
    if (!kl_fused_path(NK)) return true;
    std::vector<double> T((size_t)steps * NK * NK), E(steps * 9), R(steps * NK);
    srand(100 + steps);
    for (int i = 0; i < steps; ++i) {
        std::vector<double> B(NK * NK);
        for (auto& v : B) v = rnd();
        for (int r = 0; r < NK; ++r)
            for (int k = 0; k < NK; ++k) {
                double s = 0;
                for (int q = 0; q < NK; ++q) s += B[r * NK + q] * B[k * NK + q];
                T[(size_t)i * NK * NK + k * NK + r] = s + (r == k ? 30.0 + 1e4 * (r % 5 == 0) : 0.0);
            }
        for (int e = 0; e < 9; ++e) E[9 * i + e] = 3.0 * rnd();
        for (int r = 0; r < NK; ++r) R[i * NK + r] = 10.0 * rnd();
    }
    double *dT, *dE, *dM, *dX, *dD, *dR, *dZ, *dV;
    Timers* dt;
    int* dok;
    bool hip_ok = true;
    auto ck = [&](hipError_t e) { if (e != hipSuccess) hip_ok = false; };
    const size_t nm = (size_t)steps * NK * NK * 8, nv = (size_t)steps * NK * 8;
    ck(hipMalloc(&dT, nm)), ck(hipMalloc(&dE, E.size() * 8)), ck(hipMalloc(&dM, nm)), ck(hipMalloc(&dX, nm)), ck(hipMalloc(&dD, nv)), ck(hipMalloc(&dR, nv)), ck(hipMalloc(&dZ, nv));
    ck(hipMalloc(&dV, NK * 8)), ck(hipMalloc(&dt, sizeof(Timers))), ck(hipMalloc(&dok, 4));
    if (!hip_ok) {
        printf("forward steps, chain of %d: allocation failed\nFAIL\n", steps);
        exit(2);
    }
    ck(hipMemcpy(dT, T.data(), nm, hipMemcpyHostToDevice)), ck(hipMemcpy(dE, E.data(), E.size() * 8, hipMemcpyHostToDevice)), ck(hipMemcpy(dR, R.data(), nv, hipMemcpyHostToDevice));
    ck(hipMemset(dok, 0, 4)), ck(hipMemset(dM, 0, nm)), ck(hipMemset(dX, 0, nm)), ck(hipMemset(dD, 0, nv)), ck(hipMemset(dZ, 0, nv)), ck(hipMemset(dV, 0, NK * 8)), ck(hipMemset(dt, 0, sizeof(Timers)));
    const size_t lds = (2 * KlArea<NK>::SIZE + 8 + 10 * KL_LD) * sizeof(double);  // (+ what the second chain's guarded product reads behind its area: never cleared)
    ck(hipFuncSetAttribute((const void*)pair_kernel<NK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (hip_ok) {
        hipLaunchKernelGGL(pair_kernel<NK>, dim3(1), dim3(256), lds, 0, dT, dE, dM, dX, dD, dt, dok, 1, steps, dR, dZ, dV);
        ck(hipDeviceSynchronize());
    }
    if (!hip_ok) {
        printf("forward steps, chain of %d: launch failed\nFAIL\n", steps);
        exit(2);  // nothing more is started on a device that failed
    }
    std::vector<double> M((size_t)steps * NK * NK), D(steps * NK), Z(steps * NK), V(NK);
    Timers h{};
    int okf = 1;
    ck(hipMemcpy(M.data(), dM, nm, hipMemcpyDeviceToHost)), ck(hipMemcpy(D.data(), dD, nv, hipMemcpyDeviceToHost)), ck(hipMemcpy(Z.data(), dZ, nv, hipMemcpyDeviceToHost));
    ck(hipMemcpy(V.data(), dV, NK * 8, hipMemcpyDeviceToHost)), ck(hipMemcpy(&h, dt, sizeof(h), hipMemcpyDeviceToHost)), ck(hipMemcpy(&okf, dok, 4, hipMemcpyDeviceToHost));
    hipFree(dT), hipFree(dE), hipFree(dM), hipFree(dX), hipFree(dD), hipFree(dR), hipFree(dZ), hipFree(dV), hipFree(dt), hipFree(dok);
    double ez = 0, ev = 0, sz = 0, sv = 0;
    std::vector<double> v(NK, 0.0);
    for (int i = 0; i < steps; ++i) {
        const double* Mi = M.data() + (size_t)i * NK * NK;  // row-major, entries k >= r
        std::vector<double> rp(NK), z(NK), vn(NK);
        for (int r = 0; r < NK; ++r) {
            double c = 0;
            if (i > 0)
                for (int q = 0; q < 3; ++q) c += E[9 * (i - 1) + 3 * q + r % 3] * v[3 * (r / 3) + q];
            rp[r] = R[i * NK + r] - c;
        }
        for (int c = 0; c < NK; ++c) {
            double s = 0;
            for (int k = 0; k <= c; ++k) s += Mi[k * NK + c] * rp[k];
            z[c] = D[i * NK + c] * s;
        }
        for (int r = 0; r < NK; ++r) {
            double s = 0;
            for (int k = r; k < NK; ++k) s += Mi[r * NK + k] * z[k];
            vn[r] = s;
        }
        v = vn;
        for (int r = 0; r < NK; ++r) ez = fmax(ez, fabs(Z[i * NK + r] - z[r])), sz = fmax(sz, fabs(z[r]));
    }
    for (int r = 0; r < NK; ++r) ev = fmax(ev, fabs(V[r] - v[r])), sv = fmax(sv, fabs(v[r]));
    const bool pass = hip_ok && !okf && (!UB_FWD || (ez < 1e-12 * fmax(1.0, sz) && ev < 1e-12 * fmax(1.0, sv)));
    if (UB_FWD)
        printf("forward steps, chain of %2d: max|z err| %.3g (scale %.3g)  max|last v err| %.3g (scale %.3g); cycles per knot step %lld, of which forward step %lld, chain waits for M %lld   %s\n",
               steps, ez, sz, ev, sv, h.v[0], h.v[6], h.v[4], pass ? "fwd ok" : "MISMATCH");
    else
        printf("forward steps off, chain of %2d: cycles per knot step %lld, chain waits for M %lld   %s\n", steps, h.v[0], h.v[4], pass ? "fwd off, chain ok" : "MISMATCH");
    return pass;
}

int main() {
    printf("KL_PANEL=%d KL_PANEL_MIN_NK=%d KL_FUSED_UPDATE=%d UB_T_FIRST=%d UB_FWD=%d; LDS per chain wave (NK 36): %d doubles = %.1f KB\n", KL_PANEL, KL_PANEL_MIN_NK, KL_FUSED_UPDATE, UB_T_FIRST, UB_FWD, KlArea<36>::SIZE, KlArea<36>::SIZE * 8 / 1024.0);
    bool pass = true;
    for (int steps : {1, 2, 3, MAXSTEPS}) pass = run_forward(steps) && pass;  // (first: a wrong announcement order would hang here, on the shortest chains)
    for (double spread : {1e4, 1e8}) {
        const bool timing = spread == 1e4;
        pass = run<9>(spread, timing) && pass;
        pass = run<18>(spread, timing) && pass;
        pass = run<27>(spread, timing) && pass;
        pass = run<36>(spread, timing) && pass;
    }
    printf("%s\n", pass ? "PASS" : "FAIL");
    return pass ? 0 : 1;
}
