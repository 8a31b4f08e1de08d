// Dual active-set solve of the polish (qp_polish.inc): products with the explicit inverse factor W = L^-1 of S_PP, one wavefront.
// Included by qp_polish.inc (and by tools/ubench/lhw.hip, which times and checks it alone); needs rl_dyn (qp_polish.inc), WSYNC
// (qp_polish_types.inc), fast_rsqrt (qp_rows.inc), kl_lds (knot_lds.inc).
//
// With L every step of Lawson-Hanson is a triangular solve: nP DEPENDENT steps of one wave, twice per appended row, and the Givens
// sweep of a deletion is another dependent chain with a wave barrier per column pair (measured: ~250 cycles per step of either).
// With W the same steps are products with a triangle, in which every lane owns a row or a column and runs its own multiply-add
// chain; the LDS loads do not depend on anything:
//   append row j:   l = W s_P (lane = row), d = s_jj - |l|^2, new row of W = (-W' l, 1) / sqrt(d)  (lane = column)
//   solve:          y = W' (W d_P) = W' w, with w kept up to date across appends
//   delete row k:   S_PP^-1 = W'W; without row/column k it is B'(I - c c'/|c|^2)B, B = W without column k, c = column k of W:
//                   plane rotations of the rows k..nP-1 of B, top down, turn c into |c| e_k; the rotated rows k+1.. are the new
//                   triangle (row i+1 -> row i) and row k is dropped.  The rotation angles depend on c alone (running norms), so they
//                   are known before the row loop, in which lane = column and nothing crosses lanes.
// The forward error of a solve is of the order cond(S_PP) eps either way; what decides acceptance is polish_qp's KKT check on the
// actual rows (with its refinement rounds), as before.
//
// STORAGE.  Rows in groups of eight; the rows of group g (8g .. 8g+7) are stored with 8(g+1) entries each -- the part right of the
// diagonal is kept ZERO -- at a stride of 8(g+1)+1 doubles (odd: the lanes of a "lane = row" access fall into different banks).  So
// a group of eight steps of either product needs ONE lane mask (lane < 8(g+1), resp. row >= 8g) instead of one per step, and its
// addresses are a base plus multiples of the stride.  Invariants: row r < nP has zeros at the columns r < c < 8(r/8+1); every entry of
// the storage is finite (lh_clear at the start of a solve), so a stale row >= nP times a zero multiplier is zero.
// The loops issue the loads of the NEXT group before the multiply-adds of the current one, with two register buffers used in turn (a
// copy "current = next" would make the wave wait for the loads it has just issued).
#define LH_H 3  // lane-distributed vectors: lane l holds entries l, l + 64, l + 128 (nP <= PL_PBIG = 192)
#include "lh_layout.h"
#define LHP_ZERO 1  // (row 0, column 1): a stored zero as soon as one row is active

__device__ __forceinline__ void lhv_load(const double* x, double (&r)[LH_H], int nP, int lane) {
#pragma unroll
    for (int h = 0; h < LH_H; ++h) r[h] = lane + 64 * h < nP ? x[lane + 64 * h] : 0.0;
}
__device__ __forceinline__ void lhv_store(double* x, const double (&r)[LH_H], int nP, int lane) {
#pragma unroll
    for (int h = 0; h < LH_H; ++h)
        if (lane + 64 * h < nP) x[lane + 64 * h] = r[h];
}
struct LhV {
    double v[LH_H];
};
__device__ __forceinline__ double lhv_pick(const LhV& x, int h) { return h == 0 ? x.v[0] : (h == 1 ? x.v[1] : x.v[2]); }  // h: wave-uniform

template <class PT>
__device__ __noinline__ void lh_clear(PT W, int rows_v) {
    const int rows = __builtin_amdgcn_readfirstlane(rows_v);  // (arguments of a function arrive in VGPRs: loop bounds into SGPRs)
    const int n = lhp_size(rows);
    for (int i = threadIdx.x & 63; i < n; i += 64) W[i] = 0.0;
    WSYNC();
}

// out_c = sum_{b >= c} W[b][c] x_b   (lane = column c; entries of x past nP are zero)
template <int NH, class PT>
__device__ __forceinline__ void w_cols_span(PT W, const LhV& x, double (&out)[LH_H], int g0, int g1, int lane) {
    double A[8][NH], B[8][NH];
    auto load = [&](int g, double (&buf)[8][NH]) {
        const int L = lhp_len(g), base = lhp_grp(g);
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const int c = lane + 64 * h;
            if (c < L) {
#pragma unroll
                for (int u = 0; u < 8; ++u) buf[u][h] = W[base + u * (L + 1) + c];
            }
        }
    };
    auto use = [&](int g, const double (&buf)[8][NH]) {
        const int L = lhp_len(g);
        const double xs = lhv_pick(x, g >> 3);
        double xb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xb[u] = rl_dyn(xs, (8 * g + u) & 63);
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            if (lane + 64 * h < L) {
#pragma unroll
                for (int u = 0; u < 8; ++u) out[h] += buf[u][h] * xb[u];
            }
        }
    };
    if (g0 >= g1) return;
    load(g0, A);
    for (int g = g0; g < g1; g += 2) {
        if (g + 1 < g1) load(g + 1, B);
        use(g, A);
        if (g + 1 < g1) {
            if (g + 2 < g1) load(g + 2, A);
            use(g + 1, B);
        }
    }
}
template <int HM, class PT>  // HM = 2: nP <= 128 (fewer registers to save around the call), 3: any
__device__ __noinline__ LhV w_cols_fn(PT W, LhV x, int nP_v) {
    const int nP = __builtin_amdgcn_readfirstlane(nP_v);
    const int lane = threadIdx.x & 63, ng = (nP + 7) >> 3;
    LhV o;
#pragma unroll
    for (int h = 0; h < LH_H; ++h) o.v[h] = 0.0;
    w_cols_span<1, PT>(W, x, o.v, 0, ng < 8 ? ng : 8, lane);       // rows 0..63: columns 0..63
    if (ng > 8) w_cols_span<2, PT>(W, x, o.v, 8, ng < 16 ? ng : 16, lane);
    if (HM > 2 && ng > 16) w_cols_span<(HM > 2 ? 3 : 2), PT>(W, x, o.v, 16, ng, lane);
    return o;
}

// nP <= 64: one register, a small function (a callee saves the registers it uses above the first 40: the three-register instance
// costs ~150 scratch stores and loads per call)
template <class PT>
__device__ __noinline__ double w_cols1_fn(PT W, double x0, int nP_v) {
    const int nP = __builtin_amdgcn_readfirstlane(nP_v);
    LhV x, o;
    x.v[0] = x0, x.v[1] = x.v[2] = 0.0;
    o.v[0] = o.v[1] = o.v[2] = 0.0;
    w_cols_span<1, PT>(W, x, o.v, 0, (nP + 7) >> 3, threadIdx.x & 63);
    return o.v[0];
}

// out_b = sum_{c <= b} W[b][c] x_c   (lane = row b; entries of x past nP are zero)
template <int H0, int HM, class PT>
__device__ __forceinline__ void w_rows_span(PT W, const LhV& x, double (&out)[LH_H], int g0, int g1, int nP, int lane) {
    // column groups g0..g1-1 (columns 8g..8g+7) concern the rows >= 8g: registers H0..HM-1
    constexpr int NH = HM - H0;
    int off[NH], row[NH];
#pragma unroll
    for (int q = 0; q < NH; ++q) {
        const int b = lane + 64 * (H0 + q);
        row[q] = b < nP ? b : -1;
        off[q] = lhp_row(b < nP ? b : 0);
    }
    double A[8][NH], B[8][NH];
    auto load = [&](int g, double (&buf)[8][NH]) {
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            if (row[q] >= 8 * g) {
#pragma unroll
                for (int u = 0; u < 8; ++u) buf[u][q] = W[off[q] + 8 * g + u];
            }
        }
    };
    auto use = [&](int g, const double (&buf)[8][NH]) {
        const double xs = lhv_pick(x, g >> 3);
        double xc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xc[u] = rl_dyn(xs, (8 * g + u) & 63);
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            if (row[q] >= 8 * g) {
#pragma unroll
                for (int u = 0; u < 8; ++u) out[H0 + q] += buf[u][q] * xc[u];
            }
        }
    };
    if (g0 >= g1) return;
    load(g0, A);
    for (int g = g0; g < g1; g += 2) {
        if (g + 1 < g1) load(g + 1, B);
        use(g, A);
        if (g + 1 < g1) {
            if (g + 2 < g1) load(g + 2, A);
            use(g + 1, B);
        }
    }
}
template <int HM, class PT>
__device__ __noinline__ LhV w_rows_fn(PT W, LhV x, int nP_v) {
    const int nP = __builtin_amdgcn_readfirstlane(nP_v);
    const int lane = threadIdx.x & 63, ng = (nP + 7) >> 3;
    LhV o;
#pragma unroll
    for (int h = 0; h < LH_H; ++h) o.v[h] = 0.0;
    w_rows_span<0, HM, PT>(W, x, o.v, 0, ng < 8 ? ng : 8, nP, lane);   // columns 0..63: all rows
    if (ng > 8) w_rows_span<1, HM, PT>(W, x, o.v, 8, ng < 16 ? ng : 16, nP, lane);
    if (HM > 2 && ng > 16) w_rows_span<(HM > 2 ? 2 : 1), HM, PT>(W, x, o.v, 16, ng, nP, lane);
    return o;
}
// nP <= 64: one register (the three-register instance above costs three times the loads' registers for nothing)
template <class PT>
__device__ __noinline__ double w_rows1_fn(PT W, double x0, int nP_v) {
    const int nP = __builtin_amdgcn_readfirstlane(nP_v);
    const int lane = threadIdx.x & 63, ng = (nP + 7) >> 3;
    const int row = lane < nP ? lane : -1, off = lhp_row(lane < nP ? lane : 0);
    double out = 0.0;
    double A[8], B[8];
    auto load = [&](int g, double (&buf)[8]) {
        if (row >= 8 * g) {
#pragma unroll
            for (int u = 0; u < 8; ++u) buf[u] = W[off + 8 * g + u];
        }
    };
    auto use = [&](int g, const double (&buf)[8]) {
        double xc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xc[u] = rl_dyn(x0, 8 * g + u);
        if (row >= 8 * g) {
#pragma unroll
            for (int u = 0; u < 8; ++u) out += buf[u] * xc[u];
        }
    };
    if (ng == 0) return 0.0;
    load(0, A);
    for (int g = 0; g < ng; g += 2) {
        if (g + 1 < ng) load(g + 1, B);
        use(g, A);
        if (g + 1 < ng) {
            if (g + 2 < ng) load(g + 2, A);
            use(g + 1, B);
        }
    }
    return out;
}

// remove active row k: see the note above.  scr: nP doubles of scratch (LDS).
template <int H, class PT>
__device__ __noinline__ void w_delete_fn(PT W, double* scr_g, int nP_v, int k_v) {
    const int nP = __builtin_amdgcn_readfirstlane(nP_v), k = __builtin_amdgcn_readfirstlane(k_v);
    const int lane = threadIdx.x & 63;
    kl_lds* scr = (kl_lds*)scr_g;
    // c = column k of W (rows k..nP-1), its squares to scratch, running norms by every lane for its own row
    double cr[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int b = lane + 64 * h;
        const bool on = b >= k && b < nP;
        const double v = W[on ? lhp_row(b) + k : LHP_ZERO];
        cr[h] = v;
        if (b < nP) scr[b] = v * v;
    }
    WSYNC();
    double cs[H], sn[H];  // rotation that brings row i (= lane + 64 h, i > k) in
    {
        double run[H], prev[H];
#pragma unroll
        for (int h = 0; h < H; ++h) run[h] = 0.0, prev[h] = 0.0;
        for (int r0 = k; r0 < nP; r0 += 8) {
            double q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = scr[r0 + u < nP ? r0 + u : k];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = r0 + u < nP ? r0 + u : 1 << 20;
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    run[h] += r <= lane + 64 * h ? q[u] : 0.0;   // rho_i^2, i = lane + 64 h
                    prev[h] += r < lane + 64 * h ? q[u] : 0.0;   // rho_{i-1}^2 (summed, not subtracted: c_i may dwarf it)
                }
            }
        }
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int i = lane + 64 * h;
            const bool on = i > k && i < nP;
            const double r2 = on ? run[h] : 1.0, p2 = on ? prev[h] : 1.0;  // both > 0: W[k][k] > 0
            const double inv = fast_rsqrt(r2);
            cs[h] = on ? p2 * fast_rsqrt(p2) * inv : 1.0;  // rho_{i-1} / rho_i
            sn[h] = on ? cr[h] * inv : 0.0;                // c_i / rho_i
        }
    }
    // acc = the row that collects c (starts as row k); lane = column
    constexpr int DU = 4;  // rows per group
    double acc[H], A[DU][H], B[DU][H];
    int cdst[H];
    auto fetch = [&](int i0, double (&g)[DU][H]) {
#pragma unroll
        for (int u = 0; u < DU; ++u) {
            const int i = i0 + u < nP ? i0 + u : nP - 1;
            const int off = lhp_row(i), len = lhp_len(i >> 3);
#pragma unroll
            for (int h = 0; h < H; ++h) g[u][h] = W[lane + 64 * h < len ? off + lane + 64 * h : LHP_ZERO];
        }
    };
    auto rotate = [&](int i0, const double (&g)[DU][H]) {
#pragma unroll
        for (int u = 0; u < DU; ++u) {
            const int i = i0 + u;
            if (i < nP) {  // (wave-uniform)
                const int li = i & 63, hi = i >> 6;
                double ci = rl_dyn(cs[0], li), si = rl_dyn(sn[0], li);
                if (H > 1 && hi == 1) ci = rl_dyn(cs[H > 1 ? 1 : 0], li), si = rl_dyn(sn[H > 1 ? 1 : 0], li);
                if (H > 2 && hi == 2) ci = rl_dyn(cs[H > 2 ? 2 : 0], li), si = rl_dyn(sn[H > 2 ? 2 : 0], li);
                const int tdst = lhp_row(i - 1), ldst = lhp_len((i - 1) >> 3);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const double a = acc[h], rv = g[u][h];
                    acc[h] = ci * a + si * rv;
                    const double nv = ci * rv - si * a;
                    if (cdst[h] < ldst) W[tdst + cdst[h]] = nv;  // (columns right of the new diagonal receive their zeros)
                }
            }
        }
    };
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int c = lane + 64 * h;
        acc[h] = W[c < lhp_len(k >> 3) ? lhp_row(k) + c : LHP_ZERO];
        cdst[h] = c < k ? c : (c > k ? c - 1 : 1 << 20);  // column k is not stored (it is zero)
    }
    // (row i+4.. of the input is fetched before row i-1.. of the output is stored: the compiler cannot move a load across a store
    // into the same array)
    fetch(k + 1, A);
    for (int i0 = k + 1; i0 < nP; i0 += 2 * DU) {
        if (i0 + DU < nP) fetch(i0 + DU, B);
        rotate(i0, A);
        if (i0 + DU < nP) {
            if (i0 + 2 * DU < nP) fetch(i0 + 2 * DU, A);
            rotate(i0 + DU, B);
        }
    }
    WSYNC();
}

// wrappers: Wl = the factor in LDS, or Wg = in global memory (the large-capacity second attempt); exactly one is non-null.  Every
// instance is a function of its own (__noinline__, vectors by value in VGPRs): inlined, they shared one register allocation with
// the whole dual solve and the scalar registers spilled into VGPR lanes around every step.
__device__ __forceinline__ void lh_rows(kl_lds* Wl, double* Wg, const double (&x)[LH_H], double (&out)[LH_H], int nP, int lane) {
    if (nP <= 64) {
        out[0] = Wg ? w_rows1_fn<double*>(Wg, x[0], nP) : w_rows1_fn<kl_lds*>(Wl, x[0], nP);
        out[1] = out[2] = 0.0;
        return;
    }
    LhV xi, o;
#pragma unroll
    for (int h = 0; h < LH_H; ++h) xi.v[h] = x[h];
    o = Wg ? w_rows_fn<3, double*>(Wg, xi, nP) : (nP <= 128 ? w_rows_fn<2, kl_lds*>(Wl, xi, nP) : w_rows_fn<3, kl_lds*>(Wl, xi, nP));
#pragma unroll
    for (int h = 0; h < LH_H; ++h) out[h] = o.v[h];
}
__device__ __forceinline__ void lh_cols(kl_lds* Wl, double* Wg, const double (&x)[LH_H], double (&out)[LH_H], int nP, int lane) {
    if (nP <= 64) {
        out[0] = Wg ? w_cols1_fn<double*>(Wg, x[0], nP) : w_cols1_fn<kl_lds*>(Wl, x[0], nP);
        out[1] = out[2] = 0.0;
        return;
    }
    LhV xi, o;
#pragma unroll
    for (int h = 0; h < LH_H; ++h) xi.v[h] = x[h];
    o = Wg ? w_cols_fn<3, double*>(Wg, xi, nP) : (nP <= 128 ? w_cols_fn<2, kl_lds*>(Wl, xi, nP) : w_cols_fn<3, kl_lds*>(Wl, xi, nP));
#pragma unroll
    for (int h = 0; h < LH_H; ++h) out[h] = o.v[h];
}
__device__ __forceinline__ void lh_delete(kl_lds* Wl, double* Wg, double* scr, int nP, int k, int lane) {
    if (Wg)
        w_delete_fn<3, double*>(Wg, scr, nP, k);
    else if (nP <= 64)
        w_delete_fn<1, kl_lds*>(Wl, scr, nP, k);
    else if (nP <= 128)
        w_delete_fn<2, kl_lds*>(Wl, scr, nP, k);
    else
        w_delete_fn<3, kl_lds*>(Wl, scr, nP, k);
}
__device__ __forceinline__ void lh_reset(kl_lds* Wl, double* Wg, int rows) {
    if (Wg)
        lh_clear<double*>(Wg, rows);
    else
        lh_clear<kl_lds*>(Wl, rows);
}
