// knot_lds.inc — one knot of the block-tridiagonal L D L' factorisation on ONE wavefront, cross-lane traffic through LDS broadcasts.
//
// Replaces (round 3) the v_readlane formulation of qp.hip's wave path.  Measured on MI355X (tools/ubench/lat.hip): a dependent
// v_fma_f64 costs 5 cycles, but every value that crosses lanes through v_readlane costs two VALU->SGPR->VALU hops (a dependent step
// "2 readlanes + multiply-add" is 29 cycles, and the 36-column right-looking update of a block, 70 readlanes per column, ran 17 k
// cycles per block).  An LDS broadcast -- every lane reads the SAME address, one ds_read_b128 delivers two matrix entries to all 64
// lanes -- costs one issue slot per two entries and ~65 cycles of latency that the next column's arithmetic hides.
//
// Data layout of one chain wave (row r of the knot block in lane r, NK <= 36 lanes active):
//   C  [NK][KL_LD]   column images of the factorisation: C[c][k] = Schur-updated A[k][c] (= L[k][c] * d_c), rows k >= c valid
//   I  [KL_I]        1 / d_c
//   MX [NK+1][KL_LD] rows of M = L^-T (row r = column r of L^-1), later overwritten by the rows of the coupling factor X = Cpl M
//   U  [NK][KL_LDU]  the rank-NK update X D^-1 X' of the next block, MFMA tiles written in the C/D layout; overlays C
// (Blocks on the fused path -- kl_fused_path(NK), the 36 x 36 blocks --: MX keeps M, X only ever exists as MFMA operands and U not at all, see
// kl_fused_update; the two lines above describe the column loop and -DKL_FUSED_UPDATE=0.)
// With M explicit, the coupling factor costs 3 multiply-adds per entry (the coupling block T_{j+1,j} is 3x3-block diagonal) and the
// substitutions become matrix-vector products instead of 36-step dependent chains.
//
// The column loop (kl_ldl, kl_follow_LinvT) pays one ds_read_b128 broadcast per two multiply-adds: 23 cycles per pair against 9 for the
// arithmetic, ~275 cycles per column, and the broadcasts queue in the LDS that a co-resident workgroup shares.  Blocks of
// NK >= KL_PANEL_MIN_NK columns (the 36 x 36 blocks of the flagship missions) take the PANEL path in the second half of this file
// instead: S and the running inverse live in the accumulators of v_mfma_f64_16x16x4_f64, a step eliminates 4 columns, C holds one
// small image per panel in place of the column images (knot_panel_layout.h), and I, MX, U and the progress words keep their meaning.
// tools/ubench/knot.hip times the paths (-DKL_PANEL=0/1, -DKL_FUSED_UPDATE=0/1) in the product's arrangement; profiles/knot_panel_ubench.txt and
// profiles/knot_fused_ubench.txt have the figures.
#pragma once
#include "knot_panel_layout.h"

#define KL_LD 38   // doubles per row: 16-byte aligned rows, and rows 0..15 of a ds_read_b128 land on distinct banks (38 * 2 = 76 = 12 mod 64)
#define KL_LDU 50
#define KL_I 40
#ifndef KL_XCH
#define KL_XCH 6
#endif
typedef __attribute__((address_space(3))) double kl_lds;
typedef __attribute__((address_space(3))) int kl_ldsi;
typedef double kl_d2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) kl_d2 kl_lds2;
typedef double kl_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int kl_area_doubles(int nk) {
    return ((nk + 1) * KL_LDU + (nk + 1) * KL_LD + KL_I + 1) & ~1;
}

template <int NK>
struct KlArea {  // doubles, one chain wave
    static constexpr int NT = (NK + 15) / 16;
    static constexpr int C = 0, CSZ = (NK + 1) * KL_LDU;  // C and U share this region (row NK of U: where the unused tile rows >= NK land)
    static constexpr int MX = CSZ, MXSZ = (NK + 1) * KL_LD;  // rows of M / X, and ONE padding row (row NK): the MFMA tiles' rows >= NK all read it (kl_syrk)
    static constexpr int I = MX + MXSZ;
    static constexpr int SIZE = (I + KL_I + 1) & ~1;
    static_assert(SIZE == kl_area_doubles(NK), "kl_area_doubles out of step with KlArea");
};

#ifndef KL_COLUMN_FENCE
#define KL_COLUMN_FENCE()
#endif

__device__ __forceinline__ void kl_sync() {  // orders this wave's LDS writes before its later LDS reads (LDS executes a wave's operations in order)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// progress words between a chain wave and the wave that follows it (LDS ints): relaxed atomics so that neither the repeated stores nor
// the polling loads are optimised away; ordering against the data comes from the LDS serving each wave's operations in order
__device__ __forceinline__ void kl_publish(kl_ldsi* P, int v) { __hip_atomic_store(P, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// wait until *P >= need; `seen` caches the last value read (wave-uniform: the loop is a scalar branch)
__device__ __forceinline__ void kl_await(kl_ldsi* P, int need, int& seen) {
    while (seen < need) {
        seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(P, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (seen < need) __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The same wait as ONE opaque instruction sequence: a C++ loop inside a fully unrolled column loop splits it into basic blocks, and the
// register allocator then spills the rows it holds (973 scratch instructions in the follower, measured); inline assembly keeps the
// column loop a single block.  s_waitcnt lgkmcnt(0) also drains the caller's prefetched LDS loads -- harmless.
__device__ __forceinline__ void kl_await_opaque(kl_ldsi* P, int need) {
    int tv, ts;
    const unsigned addr = (unsigned)(__SIZE_TYPE__)P;
    asm volatile(
        "1:\n\t"
        "ds_read_b32 %0, %2\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_readfirstlane_b32 %1, %0\n\t"
        "s_cmp_ge_i32 %1, %3\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_sleep 1\n\t"
        "s_branch 1b\n\t"
        "2:\n\t"
        : "=&v"(tv), "=&s"(ts)
        : "v"(addr), "s"(__builtin_amdgcn_readfirstlane(need))
        : "memory", "scc");
}

__device__ __forceinline__ double kl_rl(double v, int lane) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// The compiler issues an LDS load where the source has it and waits for it right before the first use; it does not move loads up across
// arithmetic to hide their latency (~65-130 cycles).  The column loops below are therefore written software-pipelined by hand: ONE
// register image v[] of a column's tail, each pair reloaded with the NEXT column's entries right after its last use, so that a load
// has a whole column of multiply-adds between issue and use.

// a[k] -= s * v[k] for k >= lo, and v <- entries of `next` that column lo - 1 + 1 ... needs (k >= lo_next); pairs at even k
template <int NK>
__device__ __forceinline__ void kl_axpy_roll(double (&a)[NK], double s, double (&v)[NK], int lo, const kl_lds* next, int lo_next, bool has_next) {
#pragma unroll
    for (int k = 0; k < NK; k += 2) {
        if (k + 1 < NK) {
            if (k >= lo) a[k] -= s * v[k];
            if (k + 1 >= lo) a[k + 1] -= s * v[k + 1];
            if (has_next && k + 1 >= lo_next) {
                const kl_d2 t = *(const kl_lds2*)(next + k);
                v[k] = t[0], v[k + 1] = t[1];
            }
        } else {
            if (k >= lo) a[k] -= s * v[k];
            if (has_next && k >= lo_next) v[k] = next[k];
        }
    }
}

template <int NK>
__device__ __forceinline__ void kl_load_tail(double (&v)[NK], const kl_lds* row, int lo) {
#pragma unroll
    for (int k = 0; k < NK; k += 2) {
        if (k + 1 < lo) continue;
        if (k + 1 < NK) {
            const kl_d2 t = *(const kl_lds2*)(row + k);
            v[k] = t[0], v[k + 1] = t[1];
        } else if (k >= lo) {
            v[k] = row[k];
        }
    }
}

// A = L D L' (L unit lower), right-looking, row r of A in a[] of lane r (entries k <= r are used).  On return C holds the column
// images, I the reciprocal pivots (a[] is consumed), and the return value says whether every pivot was positive.
// P / pbase: progress word for a second wave that follows the factorisation column by column (kl_follow_LinvT): *P = pbase + n once
// the images 0 .. n-1 and the reciprocal pivots 0 .. n-2 are in the LDS (n <= NK), pbase + NK + 1 once all NK pivots are.
template <int NK>
__device__ __forceinline__ bool kl_ldl(double (&a)[NK], kl_lds* C, kl_lds* I, int r, bool act, kl_ldsi* P, int pbase) {
    bool ok = true;
    // no control flow inside the unrolled column loop (every `if (act)` would split it into basic blocks, and the register allocator then
    // spills the whole row at each boundary): lanes >= NK store to the padding slot of the row image instead
    const int rs = act ? r : KL_LD - 1;
    C[rs] = a[0];
    kl_sync();
    kl_publish(P, pbase + 1);
    double first = NK > 1 ? C[1] : 0.0;  // col_0[1]
    double v[NK];
    kl_load_tail<NK>(v, C, 2);
#pragma unroll
    for (int c = 0; c < NK; ++c) {
        const double d = kl_rl(a[c], c);  // the pivot travels by v_readlane; reciprocal = rcp + one Newton step (2e-15)
        ok = ok && (d > 0);
        double inv = __builtin_amdgcn_rcp(d);
        inv = __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
        I[c] = inv;  // (every lane holds the same value: one store, no control flow)
        const double lc = a[c] * inv;
        if (c + 1 < NK) {
            // the next column's image leaves as soon as its entries exist; its first entry (the one the image after it waits for) is
            // requested at once, the rest of it pair by pair behind this column's updates
            a[c + 1] -= lc * first;
            kl_lds* nxt = C + (c + 1) * KL_LD;
            nxt[rs] = a[c + 1];
            kl_sync();
            kl_publish(P, pbase + c + 2);
            if (c + 2 < NK) first = nxt[c + 2];
            kl_axpy_roll<NK>(a, lc, v, c + 2, nxt, c + 3, c + 3 < NK);
        }
    }
    kl_sync();
    kl_publish(P, pbase + NK + 1);  // the last reciprocal pivot is in I as well
    return ok;
}

// m <- m L^-T for the row vector m of every lane (column images and reciprocal pivots of kl_ldl): with m = e_r on entry, m becomes row r
// of M = L^-T, i.e. column r of L^-1 (entries k >= r).  No dependent chain beyond one multiply-add per column.
template <int NK>
__device__ __forceinline__ void kl_row_times_LinvT(double (&m)[NK], const kl_lds* C, const kl_lds* I) {
    double v[NK];
    kl_load_tail<NK>(v, C, 1);
    double ic = I[0];
#pragma unroll
    for (int c = 0; c + 1 < NK; ++c) {
        const double s = m[c] * ic;
        if (c + 2 < NK) ic = I[c + 1];
        kl_axpy_roll<NK>(m, s, v, c + 1, C + (c + 1) * KL_LD, c + 2, c + 2 < NK);
    }
}

// the same in a SECOND wave, concurrently with the factorisation: column step c only needs image c + 1 (prefetched) and 1 / d_c, both
// published by kl_ldl during ITS column c -- the follower runs a column or two behind the chain, and the chain no longer pays for M
#ifndef KL_FOLLOW_STRIDE
#define KL_FOLLOW_STRIDE 2  // columns per look at the chain's progress word (a look costs an LDS round trip)
#endif
template <int NK>
__device__ __forceinline__ void kl_follow_LinvT(double (&m)[NK], const kl_lds* C, const kl_lds* I, kl_ldsi* P, int pbase) {
    double v[NK];
    kl_await_opaque(P, pbase + (KL_FOLLOW_STRIDE + 1 < NK ? KL_FOLLOW_STRIDE + 1 : NK));  // images 0 .. STRIDE, pivots 0 .. STRIDE - 1
    kl_load_tail<NK>(v, C, 1);
#pragma unroll
    for (int c = 0; c + 1 < NK; ++c) {
        // step c needs image c + 1 and 1 / d_c, i.e. *P >= pbase + c + 2
        if (c > 0 && c % KL_FOLLOW_STRIDE == 0) kl_await_opaque(P, pbase + (c + KL_FOLLOW_STRIDE + 1 < NK ? c + KL_FOLLOW_STRIDE + 1 : NK));
        const double s = m[c] * I[c];
        kl_axpy_roll<NK>(m, s, v, c + 1, C + (c + 1) * KL_LD, c + 2, c + 2 < NK);
    }
}

// rows of M (registers of lane r) -> MX
template <int NK>
__device__ __forceinline__ void kl_store_rows(const double (&m)[NK], kl_lds* MX, int r, bool act) {
    kl_lds* row = MX + (act ? r : NK) * KL_LD;  // lanes >= NK: a row of the tile padding (finite junk, see kl_syrk)
#pragma unroll
    for (int k = 0; k + 1 < NK; k += 2) *(kl_lds2*)(row + k) = kl_d2{m[k], m[k + 1]};
    if (NK & 1) row[NK - 1] = m[NK - 1];
    kl_sync();
}

// row r of X = Cpl M, Cpl 3x3-block diagonal: x[k] = e0 M[3g][k] + e1 M[3g+1][k] + e2 M[3g+2][k], g = r / 3 (M lower... rows of L^-T:
// M[q][k] = 0 for k < q, the zeros are stored).  Afterwards the rows of X replace the rows of M in MX (all lanes have read by then:
// the LDS serves a wave's operations in order).
template <int NK>
__device__ __forceinline__ void kl_coupling_rows(double (&x)[NK], kl_lds* MX, int r, bool act, double e0, double e1, double e2) {
    const int g3 = 3 * ((act ? r : 0) / 3);
    const kl_lds* m0 = MX + g3 * KL_LD;
    // the scheduler issues LDS loads where the source has them and waits at once: the loads of the next chunk are therefore written
    // ahead of the arithmetic of the current one (chunks of KL_XCH pairs of the three rows)
    constexpr int NP = NK / 2;
    kl_d2 t[2][3][KL_XCH];
#pragma unroll
    for (int p = 0; p < KL_XCH && p < NP; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) t[0][q][p] = *(const kl_lds2*)(m0 + q * KL_LD + 2 * p);
#pragma unroll
    for (int ch = 0; ch * KL_XCH < NP; ++ch) {
#pragma unroll
        for (int p = 0; p < KL_XCH; ++p)
            if ((ch + 1) * KL_XCH + p < NP)
#pragma unroll
                for (int q = 0; q < 3; ++q) t[(ch + 1) & 1][q][p] = *(const kl_lds2*)(m0 + q * KL_LD + 2 * ((ch + 1) * KL_XCH + p));
#pragma unroll
        for (int p = 0; p < KL_XCH; ++p) {
            const int k = 2 * (ch * KL_XCH + p);
            if (k + 1 < NK) {
                x[k] = e0 * t[ch & 1][0][p][0] + e1 * t[ch & 1][1][p][0] + e2 * t[ch & 1][2][p][0];
                x[k + 1] = e0 * t[ch & 1][0][p][1] + e1 * t[ch & 1][1][p][1] + e2 * t[ch & 1][2][p][1];
            }
        }
    }
    if (NK & 1) x[NK - 1] = e0 * m0[NK - 1] + e1 * m0[KL_LD + NK - 1] + e2 * m0[2 * KL_LD + NK - 1];
    kl_sync();
    kl_store_rows<NK>(x, MX, r, act);
}

// U (+)= X D^-1 X' (lower 16x16 tiles) with v_mfma_f64_16x16x4_f64: X rows in MX (rows >= NK hold finite junk that only reaches unused
// entries), 1/d in I, U rows < NK written in row-major order (C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg).
template <int NK>
__device__ __forceinline__ void kl_syrk(const kl_lds* MX, const kl_lds* I, kl_lds* U, int lane, bool accumulate) {
    constexpr int NT = (NK + 15) / 16, KS = (NK + 3) / 4;
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        kl_d4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = kl_d4{0, 0, 0, 0};
        // X = Cpl M with M = L^-T upper triangular and Cpl 3x3-block diagonal: X[r][k] = 0 for k < 3 (r / 3), so the tiles of tile row ti
        // only see columns k >= 3 ((16 ti) / 3): the earlier MFMA steps would multiply zeros (27 instead of 54 MFMAs for NK = 36)
        for (int ks = (3 * ((16 * ti) / 3)) / 4; ks < KS; ++ks) {
            const int kc = 4 * ks + lk;
            const double dk = kc < NK ? I[kc] : 0.0;
            // (tile rows >= NK read the padding row NK -- finite junk that only reaches unused entries of U --: the area holds NK + 1 rows, not
            // 16 NT; round 6: the 3.3 KB per chain this frees pay for the LDS images of the just-in-time block assembly, see twisted_factor)
            const double opi = (kc < NK ? MX[(16 * ti + li < NK ? 16 * ti + li : NK) * KL_LD + kc] : 0.0) * dk;
#pragma unroll
            for (int tj = 0; tj <= ti; ++tj) {
                const double opj = kc < NK ? MX[(16 * tj + li < NK ? 16 * tj + li : NK) * KL_LD + kc] : 0.0;
                acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(opi, opj, acc[tj], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = 16 * ti + lk + 4 * g;
                kl_lds* u = U + (row < NK ? row : NK) * KL_LDU + 16 * tj + li;
                *u = accumulate ? *u + acc[tj][g] : acc[tj][g];
            }
    }
    kl_sync();
}

// ---- panel-blocked formulation: 4 columns per step, trailing updates on v_mfma_f64_16x16x4_f64 (index maps: knot_panel_layout.h) -------
// The column loop above is bound by the LDS broadcasts of one wave (one ds_read_b128 per two multiply-adds, 23 cycles per pair against
// 9 for the arithmetic).  Here the Schur complement S lives in the accumulators of the MFMA instruction (upper 16 x 16 tiles of the
// block padded with a unit diagonal), and a step eliminates a PANEL of 4 columns:
//   (i)   the 4 panel rows of S go to an LDS image -- every lane owns exactly one entry per tile, one ds_write_b64 per tile;
//   (ii)  every lane reads the 4 x 4 diagonal block (broadcast) and factorises it redundantly in registers: 4 reciprocals per panel and
//         no cross-lane exchange inside a panel; the same L, D and 1 / d as the scalar recursion, in another order of roundings;
//   (iii) every lane eliminates the rows it serves as an MFMA operand (16 t + (lane & 15), t = the live tile rows) against that block
//         and keeps the entry of column lane >> 4: L is the A operand, L d the B operand of the rank-4 update of the live tiles, at
//         most 6 MFMAs per panel and 31 per block for NK = 36.  The tile row of the NEXT panel is updated first and that panel's
//         image leaves, its loads are issued, before the remaining tiles are updated.
//   (iv)  L of the panel replaces S in the image (the A operands just formed: one ds_write_b64 per tile), and the image is announced.
// The following wave computes N = L^-1 on the same panels: it reads the image of panel p (the rows of L it serves and the unit lower
// diagonal block L_pp), forms G = -L_p (L_pp)^-1 and applies N <- N + G N[panel rows] -- rank 4, the B operand being registers of
// its own lower tiles (see knot_panel_layout.h); it needs no reciprocal and no factorisation of its own.  M = L^-T is N transposed; it leaves the tiles for MX row by row.
// Every lane only ever writes inside the panel images, the (padded) rows of MX and I: there is no lane >= NK to keep out.
// Part of what is written there is UNDEFINED: in the panel's own tile row the lanes that serve rows above the panel (already eliminated)
// and the panel's own rows right of the diagonal run the row elimination on stale accumulator contents, and that junk -- possibly Inf or
// NaN after a failed pivot -- goes into the image as "L" and into the MFMA operands.  It only reaches finished rows and columns of the
// tiles (an entry of D depends on its own row of A and column of B), and the following wave never uses those image entries: it reads
// the strict lower part of the diagonal block, and masks the rows at and above the panel BITWISE (kl_pick; 0 * NaN would not do).
// Keep kl_pick a bit operation, and do not start reading those rows.
// Progress word: *P = pbase + p + 1 once the images 0 .. p hold L (p < NP <= NK), pbase + NK + 1 once every 1 / d is in I --
// every count is published whatever the pivots are.
#ifndef KL_PANEL
#define KL_PANEL 1
#endif
#ifndef KL_PANEL_MIN_NK
#define KL_PANEL_MIN_NK 36  // smaller blocks keep the column loop: NK = 9 loses on panels, 18 and 27 gain in tools/ubench/knot.hip but have not been through the product's A/B
#endif
__host__ __device__ constexpr bool kl_panel_path(int nk) { return KL_PANEL && nk >= KL_PANEL_MIN_NK; }

template <int NK>
struct KlPanels {
    static constexpr int NT = kp_nt(NK), NP = kp_np(NK), TILES = kp_ntiles(NT);
    static_assert(kp_img_total(NK) <= KlArea<NK>::CSZ, "the panel images must fit the C / U region");
};

__device__ __forceinline__ double kl_recip(double d) {  // rcp + one Newton step (2e-15), as in kl_ldl
    const double inv = __builtin_amdgcn_rcp(d);
    return __builtin_fma(__builtin_fma(-d, inv, 1.0), inv, inv);
}
// c ? a : b on the bits: a ?: on doubles that are computed nearby comes out as divergent branches (the compiler sinks the arithmetic into
// them), which split the unrolled panel loop into basic blocks -- measured at twice the time of a panel step
__device__ __forceinline__ double kl_pick(bool c, double a, double b) {
    const long long m = -(long long)c;
    return __longlong_as_double((__double_as_longlong(a) & m) | (__double_as_longlong(b) & ~m));
}
__device__ __forceinline__ double kl_sel4(const double (&v)[4], int k) {
    return kl_pick((k & 2) != 0, kl_pick((k & 1) != 0, v[3], v[2]), kl_pick((k & 1) != 0, v[1], v[0]));
}

// the 4 x 4 diagonal block of a panel: raw entries (lower triangle) as loaded, then its L D L'
struct KlPivot {
    double d0, d10, d11, d20, d21, d22, d30, d31, d32, d33;  // raw S[4p + a][4p + k], k <= a
    double i0, i1, i2, i3;                                    // 1 / d
    double w10, w20, w21, w30, w31, w32;                      // L d
    double l10, l20, l21, l30, l31, l32;                      // L
    bool ok;
};
__device__ __forceinline__ void kl_pivot_load(KlPivot& f, const kl_lds* img, int p) {  // wave-uniform addresses: broadcasts
    const kl_lds* b = img + kp_img_entry(KP_W * p, 0);
    f.d0 = b[0];
    const kl_d2 r1 = *(const kl_lds2*)(b + 4), r2 = *(const kl_lds2*)(b + 8), r3 = *(const kl_lds2*)(b + 12), r3b = *(const kl_lds2*)(b + 14);
    f.d22 = b[10];
    f.d10 = r1[0], f.d11 = r1[1], f.d20 = r2[0], f.d21 = r2[1], f.d30 = r3[0], f.d31 = r3[1], f.d32 = r3b[0], f.d33 = r3b[1];
}
__device__ __forceinline__ void kl_pivot_factor(KlPivot& f) {
    f.i0 = kl_recip(f.d0);
    f.w10 = f.d10, f.l10 = f.w10 * f.i0;
    f.w20 = f.d20, f.l20 = f.w20 * f.i0;
    f.w30 = f.d30, f.l30 = f.w30 * f.i0;
    const double d1 = __builtin_fma(-f.l10, f.w10, f.d11);
    f.i1 = kl_recip(d1);
    f.w21 = __builtin_fma(-f.l20, f.w10, f.d21), f.l21 = f.w21 * f.i1;
    f.w31 = __builtin_fma(-f.l30, f.w10, f.d31), f.l31 = f.w31 * f.i1;
    const double d2 = __builtin_fma(-f.l21, f.w21, __builtin_fma(-f.l20, f.w20, f.d22));
    f.i2 = kl_recip(d2);
    f.w32 = __builtin_fma(-f.l31, f.w21, __builtin_fma(-f.l30, f.w20, f.d32)), f.l32 = f.w32 * f.i2;
    const double d3 = __builtin_fma(-f.l32, f.w32, __builtin_fma(-f.l31, f.w31, __builtin_fma(-f.l30, f.w30, f.d33)));
    f.i3 = kl_recip(d3);
    f.ok = f.d0 > 0 && d1 > 0 && d2 > 0 && d3 > 0;
}
// one row of the panel against the factorised diagonal block: s (raw) -> W = L d and L
__device__ __forceinline__ void kl_panel_row(const KlPivot& f, const kl_d2 s01, const kl_d2 s23, double (&L)[4], double (&W)[4]) {
    W[0] = s01[0], L[0] = W[0] * f.i0;
    W[1] = __builtin_fma(-L[0], f.w10, s01[1]), L[1] = W[1] * f.i1;
    W[2] = __builtin_fma(-L[1], f.w21, __builtin_fma(-L[0], f.w20, s23[0])), L[2] = W[2] * f.i2;
    W[3] = __builtin_fma(-L[2], f.w32, __builtin_fma(-L[1], f.w31, __builtin_fma(-L[0], f.w30, s23[1]))), L[3] = W[3] * f.i3;
}

// S -> upper tiles: entry(mx, mn) returns the element (mx, mn), mx >= mn, of the symmetric NK x NK source (its lower triangle); rows and
// columns >= NK are the unit diagonal of the padding.  OP 1: subtract from the tiles instead; OP 2: add to them (the padding is SET all the
// same: whatever the tiles held there is replaced by the unit diagonal).  BOTH: the source holds both triangles
// of the diagonal tiles (the LDS images of T_j and U do) -- entry is then called with (column, row) of the tile entry as it stands,
// which is (mx, mn) above the diagonal and the mirrored, equal element below it: a lane's addresses are one base plus constants,
// instead of one register per diagonal-tile entry for the lane-dependent choice (the factorisation only consumes entries at and above
// the diagonal anyway).
template <int NK, int OP, bool BOTH, class F>
__device__ __forceinline__ void kl_tiles_load(kl_d4 (&s)[KlPanels<NK>::TILES], int lane, F&& entry) {
    constexpr int NT = KlPanels<NK>::NT;
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = ti; tj < NT; ++tj)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = KP_T * ti + lk + 4 * g, j = KP_T * tj + li;
                const int mx = BOTH ? j : i > j ? i : j, mn = BOTH ? i : i > j ? j : i;
                const bool full = KP_T * tj + KP_T <= NK;  // (compile time: tj >= ti)
                const bool pad = !full && (i >= NK || j >= NK);
                const double v = entry(full || mx < NK ? mx : NK - 1, full || mn < NK ? mn : NK - 1);
                const int tile = kp_upper(ti, tj, NT);
                if (OP == 1)
                    s[tile][g] -= pad ? 0.0 : v;
                else if (OP == 2)
                    s[tile][g] = pad ? (i == j ? 1.0 : 0.0) : s[tile][g] + v;
                else
                    s[tile][g] = pad ? (i == j ? 1.0 : 0.0) : v;
            }
}

// image of panel p: rows 4p .. 4p+3 of S (= its columns), one entry per lane and tile
template <int NK>
__device__ __forceinline__ void kl_panel_out(const kl_d4 (&s)[KlPanels<NK>::TILES], kl_lds* C, int p, int li, int lk) {
    constexpr int NT = KlPanels<NK>::NT;
    kl_lds* img = C + kp_img_off(NK, p);
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
        if (tj >= kp_panel_tile(p)) img[kp_img_entry(KP_T * tj + li, lk)] = s[kp_upper(kp_panel_tile(p), tj, NT)][kp_panel_reg(p)];
}

// the rows a lane serves (16 t + li, t >= t_first) of panel p from the LDS image
template <int NK>
__device__ __forceinline__ void kl_rows_load(kl_d2 (&raw)[KlPanels<NK>::NT][2], const kl_lds* img, int t_first, int li) {
#pragma unroll
    for (int t = 0; t < KlPanels<NK>::NT; ++t)
        if (t >= t_first) raw[t][0] = *(const kl_lds2*)(img + kp_img_entry(KP_T * t + li, 0)), raw[t][1] = *(const kl_lds2*)(img + kp_img_entry(KP_T * t + li, 2));
}

// S (upper tiles, consumed) = L D L': panel images into C, 1 / d into I, progress through P (see above); returns "every pivot positive"
template <int NK>
__device__ __forceinline__ bool kl_ldl_panels(kl_d4 (&s)[KlPanels<NK>::TILES], kl_lds* C, kl_lds* I, int lane, kl_ldsi* P, int pbase) {
    constexpr int NT = KlPanels<NK>::NT, NP = KlPanels<NK>::NP;
    const int li = lane & 15, lk = lane >> 4;
    bool ok = true;
    KlPivot f;
    kl_d2 raw[NT][2];
    kl_panel_out<NK>(s, C, 0, li, lk);
    kl_sync();
    kl_pivot_load(f, C, 0);
    kl_rows_load<NK>(raw, C, 0, li);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int tc = kp_panel_tile(p), t0 = kp_first_live_tile(p);
        kl_lds* img = C + kp_img_off(NK, p);
        kl_pivot_factor(f);
        ok = ok && f.ok;
        if (KP_W * p + 0 < NK) I[KP_W * p + 0] = f.i0;  // (every lane holds the same values: plain stores, no control flow)
        if (KP_W * p + 1 < NK) I[KP_W * p + 1] = f.i1;
        if (KP_W * p + 2 < NK) I[KP_W * p + 2] = f.i2;
        if (KP_W * p + 3 < NK) I[KP_W * p + 3] = f.i3;
        const double inv[4] = {f.i0, f.i1, f.i2, f.i3};
        const double isel = kl_sel4(inv, lk);
        double a[NT], b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t >= tc) {
                double L[4], W[4];
                kl_panel_row(f, raw[t][0], raw[t][1], L, W);
                b[t] = kl_sel4(W, lk);
                const double l = b[t] * isel;  // (= L[lk], the same product)
                a[t] = -l;
                img[kp_img_entry(KP_T * t + li, lk)] = l;  // L replaces S in the image: this wave's reads of the row are served first (in order)
            }
        // the tile row of the next panel first; its image and the loads of the next step leave before the other tiles are updated
        if (p + 1 < NP) {
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
                if (tj >= t0) s[kp_upper(t0, tj, NT)] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t0], b[tj], s[kp_upper(t0, tj, NT)], 0, 0, 0);
        }
        kl_sync();
        kl_publish(P, pbase + p + 1);
        if (p + 1 < NP) {
            kl_panel_out<NK>(s, C, p + 1, li, lk);
            kl_sync();
            kl_pivot_load(f, C + kp_img_off(NK, p + 1), p + 1);
            kl_rows_load<NK>(raw, C + kp_img_off(NK, p + 1), kp_panel_tile(p + 1), li);
            __builtin_amdgcn_sched_barrier(0);  // (the scheduler would put all MFMAs of the step in front of the image: 3 x 64 cycles of issue more on the chain)
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = ti; tj < NT; ++tj)
                    if (ti > t0) s[kp_upper(ti, tj, NT)] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], s[kp_upper(ti, tj, NT)], 0, 0, 0);
        }
    }
    kl_publish(P, pbase + NK + 1);  // every reciprocal pivot is in I
    return ok;
}

// One knot on the panel path, as the callers form it: S = T (- U) into the tiles, then its factorisation.  t_entry(mx, mn) returns
// T[mx][mn] of the assembled lower triangle (mx >= mn), t_loaded() runs once T's values have been requested (where the caller waits
// for them and releases their source); U is the rank-NK update that kl_syrk left in the C / U region.
// T_BOTH: T's source holds both triangles (see kl_tiles_load).
template <int NK, bool T_BOTH, class TF, class LF>
__device__ __forceinline__ bool kl_knot_panels(TF&& t_entry, LF&& t_loaded, bool minus_u, kl_lds* C, kl_lds* I, int lane, kl_ldsi* P, int pbase) {
    kl_d4 s[KlPanels<NK>::TILES];
    kl_tiles_load<NK, 0, T_BOTH>(s, lane, t_entry);
    t_loaded();
    if (minus_u) kl_tiles_load<NK, 1, true>(s, lane, [&](int mx, int mn) { return (double)C[mx * KL_LDU + mn]; });  // (kl_syrk writes whole diagonal tiles)
    kl_sync();  // (U is read: the panel images overlay it)
    return kl_ldl_panels<NK>(s, C, I, lane, P, pbase);
}

// ---- the rank-NK update formed in the tiles (KL_FUSED_UPDATE) --------------------------------------------------------------------------
// kl_coupling_rows + kl_syrk + the SUB pass above carry the same numbers through the LDS three times: M -> X (rows, over M), X -> U (tiles,
// stored), U -> S (read back element by element), each hop with its own kl_sync, all of it on the chain.  Here S_next = T - X D^-1 X' is
// accumulated where the factorisation consumes it: the tiles start at zero, every MFMA operand element X[16 t + li][4 ks + lk] is formed
// where it is needed from the three rows of M it combines (three ds_read_b64 a row apart: the 16 rows of a tile row fall into 6 groups
// whose 4 doubles lie on distinct banks -- 3 KL_LD doubles = 36 dwords mod 64 between groups --, the lanes of a group read one address)
// and the knot's nine coupling coefficients, A = -X and B = X / d go straight into v_mfma_f64_16x16x4_f64, and T is added when its
// image has arrived (kl_knot_panels_add).  Neither X nor U exists in the LDS, MX keeps M, and the chain wave writes nothing outside the
// panel images and I: the companion may announce M as soon as its tiles are scattered (kl_inverse_rows).
#ifndef KL_FUSED_UPDATE
#define KL_FUSED_UPDATE 1  // 0: the panel path with kl_coupling_rows / kl_syrk, the parent of the A/B in profiles/knot_fused_ubench.txt
#endif
__host__ __device__ constexpr bool kl_fused_path(int nk) { return KL_FUSED_UPDATE && kl_panel_path(nk); }

// the coefficients of the rows a lane forms: cf[t][q] multiplies row kp_x_group(16 t + li) + q of M; coef(row, q) returns T_next,this[row][group + q]
// (coupling_coef of qp_wave_factor.inc).  Rows of the padding get zeros: they contribute nothing, and the tiles' padding stays what kl_tiles_load sets.
template <int NK, class F>
__device__ __forceinline__ void kl_fused_coef(double (&cf)[KlPanels<NK>::NT][3], int lane, F&& coef) {
    const int li = lane & 15;
#pragma unroll
    for (int t = 0; t < KlPanels<NK>::NT; ++t) {
        const int row = KP_T * t + li;
        const bool in = KP_T * t + KP_T <= NK || row < NK;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double c = coef(in ? row : 0, q);
            cf[t][q] = in ? c : 0.0;
        }
    }
}

template <int NK>
__device__ __forceinline__ void kl_tiles_zero(kl_d4 (&s)[KlPanels<NK>::TILES]) {
#pragma unroll
    for (int t = 0; t < KlPanels<NK>::TILES; ++t) s[t] = kl_d4{0, 0, 0, 0};
}

// s -= X D^-1 X' (upper tiles), X = Cpl M: M rows in MX, 1 / d in I, Cpl in cf (kl_fused_coef).  SKIP: leave out the k-steps in which the
// B operand is all zeros (27 instead of 54 MFMAs for NK = 36); they multiply exact zeros, so the result has the same bits either way
template <int NK, bool SKIP = true>
__device__ __forceinline__ void kl_fused_update(kl_d4 (&s)[KlPanels<NK>::TILES], const kl_lds* MX, const kl_lds* I, int lane, const double (&cf)[KlPanels<NK>::NT][3]) {
    constexpr int NT = KlPanels<NK>::NT, KS = kp_ksteps(NK);
    const int li = lane & 15, lk = lane >> 4;
    const kl_lds* grp[NT];  // M[group of row 16 t + li][lk]: every address below is this plus a constant
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int row = KP_T * t + li;
        grp[t] = MX + kp_x_group(KP_T * t + KP_T <= NK || row < NK ? row : 0) * KL_LD + lk;
    }
    double raw[2][NT][3], dk[2];  // (the loads of a k-step are written one step ahead of their use: see kl_axpy_roll)
    auto request = [&](int ks) {
        const bool live = KP_W * ks + KP_W <= NK || KP_W * ks + lk < NK;  // (columns >= NK: the padding of the rows, finite)
        dk[ks & 1] = I[live ? KP_W * ks + lk : 0];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (!SKIP || ks >= kp_x_first_kstep(t))
#pragma unroll
                for (int q = 0; q < 3; ++q) raw[ks & 1][t][q] = grp[t][q * KL_LD + KP_W * ks];
    };
    request(0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks + 1 < KS) request(ks + 1);
        const bool live = KP_W * ks + KP_W <= NK || KP_W * ks + lk < NK;
        double a[NT], b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (!SKIP || ks >= kp_x_first_kstep(t)) {
                const double (&m)[3] = raw[ks & 1][t];
                const double x = cf[t][0] * m[0] + cf[t][1] * m[1] + cf[t][2] * m[2];  // (the expression of kl_coupling_rows)
                // entry (i, j) of an upper tile is -sum_k X[i][k] * fl(X[j][k] / d_k): the scaled factor is the one of the LATER row, as in the lower
                // tiles of kl_syrk that the parent path reads through their mirror image -- the products are exact inside the MFMA, so the tiles
                // get the bits of T - U
                a[t] = live ? -x : 0.0;
                b[t] = live ? x * dk[ks & 1] : 0.0;
            }
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
            if (!SKIP || ks >= kp_x_first_kstep(tj))
#pragma unroll
                for (int ti = 0; ti <= tj; ++ti)
                    s[kp_upper(ti, tj, NT)] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], s[kp_upper(ti, tj, NT)], 0, 0, 0);
    }
}

// One knot on the fused path: the tiles hold -X D^-1 X' (kl_tiles_zero, kl_fused_update: before the caller waits for T); T is added,
// then the factorisation.  t_entry, t_loaded, T_BOTH: see kl_knot_panels.  No kl_sync of its own: the update's reads of MX and I are served
// before the factorisation's writes to I (one wave, in order), and nothing lies under the panel images.
template <int NK, bool T_BOTH, class TF, class LF>
__device__ __forceinline__ bool kl_knot_panels_add(kl_d4 (&s)[KlPanels<NK>::TILES], TF&& t_entry, LF&& t_loaded, kl_lds* C, kl_lds* I, int lane, kl_ldsi* P, int pbase) {
    kl_tiles_load<NK, 2, T_BOTH>(s, lane, t_entry);
    t_loaded();
    return kl_ldl_panels<NK>(s, C, I, lane, P, pbase);
}

// N = L^-1 (lower tiles) from the panel images, panel by panel behind the chain (WAIT) or after it
template <int NK, bool WAIT>
__device__ __forceinline__ void kl_inverse_panels(kl_d4 (&n)[KlPanels<NK>::TILES], const kl_lds* C, int lane, kl_ldsi* P, int pbase) {
    constexpr int NT = KlPanels<NK>::NT, NP = KlPanels<NK>::NP;
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj)
#pragma unroll
            for (int g = 0; g < 4; ++g) n[kp_lower(ti, tj)][g] = (ti == tj && lk + 4 * g == li) ? 1.0 : 0.0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int tc = kp_panel_tile(p), q = kp_panel_reg(p);
        if (WAIT) kl_await_opaque(P, pbase + p + 1);
        const kl_lds* img = C + kp_img_off(NK, p);
        // the unit lower L_pp of the diagonal block (rows 4p + 1 .. 4p + 3 of the image, broadcasts), K = strict lower part of its inverse
        const kl_lds* bl = img + kp_img_entry(KP_W * p, 0);
        const double l10 = bl[4], l32 = bl[14];
        const kl_d2 r2 = *(const kl_lds2*)(bl + 8), r3 = *(const kl_lds2*)(bl + 12);
        kl_d2 raw[NT][2];
        kl_rows_load<NK>(raw, img, tc, li);
        const double l20 = r2[0], l21 = r2[1], l30 = r3[0], l31 = r3[1];
        const double k10 = -l10, k21 = -l21, k32 = -l32;
        const double k20 = __builtin_fma(-l21, k10, -l20), k31 = __builtin_fma(-l32, k21, -l31);
        const double k30 = __builtin_fma(-l32, k20, __builtin_fma(-l31, k10, -l30));
        double a[NT], b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t >= tc) {
                const double L[4] = {raw[t][0][0], raw[t][0][1], raw[t][1][0], raw[t][1][1]};
                double G[4];  // row of -L_p (L_pp)^-1
                G[3] = -L[3];
                G[2] = -__builtin_fma(L[3], k32, L[2]);
                G[1] = -__builtin_fma(L[3], k31, __builtin_fma(L[2], k21, L[1]));
                G[0] = -__builtin_fma(L[3], k30, __builtin_fma(L[2], k20, __builtin_fma(L[1], k10, L[0])));
                if (t == tc) {  // rows of the panel itself: K; rows above it: nothing
                    const int ar = KP_T * t + li - KP_W * p;
                    G[0] = kl_pick(ar >= 4, G[0], kl_pick(ar == 1, k10, kl_pick(ar == 2, k20, kl_pick(ar == 3, k30, 0.0))));
                    G[1] = kl_pick(ar >= 4, G[1], kl_pick(ar == 2, k21, kl_pick(ar == 3, k31, 0.0)));
                    G[2] = kl_pick(ar >= 4, G[2], kl_pick(ar == 3, k32, 0.0));
                    G[3] = kl_pick(ar >= 4, G[3], 0.0);
                }
                a[t] = kl_sel4(G, lk);
            }
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
            if (tj <= tc) b[tj] = n[kp_lower(tc, tj)][q];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj <= ti; ++tj)
                if (ti >= tc && tj <= tc) n[kp_lower(ti, tj)] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], n[kp_lower(ti, tj)], 0, 0, 0);
    }
}

// N (lower tiles) -> rows of M = N' in MX (zeros below the diagonal are stored; padding lands in row NK)
template <int NK>
__device__ __forceinline__ void kl_tiles_scatter(const kl_d4 (&n)[KlPanels<NK>::TILES], kl_lds* MX, int lane) {
    constexpr int NT = KlPanels<NK>::NT;
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (KP_T * ti + 4 * g >= NK) continue;  // columns of the padding only (compile time)
                const int col = KP_T * ti + lk + 4 * g, row = KP_T * tj + li;  // M[row][col] = N[col][row]
                const bool in = (KP_T * tj + KP_T <= NK || row < NK) && (KP_T * ti + 4 * g + 4 <= NK || col < NK);
                MX[in ? row * KL_LD + col : NK * KL_LD + li] = tj <= ti ? n[kp_lower(ti, tj)][g] : 0.0;
            }
    kl_sync();
}
// row r of MX back into m[] of lane r
template <int NK>
__device__ __forceinline__ void kl_row_load(double (&m)[NK], const kl_lds* MX, int r, bool act) {
    const kl_lds* row = MX + (act ? r : NK) * KL_LD;
#pragma unroll
    for (int k = 0; k + 1 < NK; k += 2) {
        const kl_d2 t = *(const kl_lds2*)(row + k);
        m[k] = t[0], m[k + 1] = t[1];
    }
    if (NK & 1) m[NK - 1] = row[NK - 1];
}

// M = L^-T of the block that kl_ldl / kl_ldl_panels factorise(d): row r into m[] of lane r and into MX; returns 1 / d_r.  FOLLOW:
// concurrently with the factorisation, in a second wave, which announces *Mdone = done_value once the chain may go on to its next block:
// MX holds M, and 1 / d has been read (the chain's next block overwrites I).
// Fused path: the announcement leaves right after the scatter, its kl_sync and the read of 1 / d; the read-back of the row, which only
// serves the caller's store to global memory, follows it.  That is safe because the chain no longer writes into MX: the next write to
// MX is THIS wave's scatter of the next block, in program order after the read-back, and the chain's update of the next block reads MX and I
// before its own factorisation writes I and the panel images that this wave's next scatter waits for.
// Otherwise the chain overwrites M with X as soon as it is told: the read-back comes first.
template <int NK, bool FOLLOW>
__device__ __forceinline__ double kl_inverse_rows(double (&m)[NK], const kl_lds* C, const kl_lds* I, kl_lds* MX, int r, bool act, kl_ldsi* P, int pbase,
                                                  kl_ldsi* Mdone = nullptr, int done_value = 0) {
    if constexpr (kl_panel_path(NK)) {
        kl_d4 n[KlPanels<NK>::TILES];
        kl_inverse_panels<NK, FOLLOW>(n, C, r, P, pbase);
        kl_tiles_scatter<NK>(n, MX, r);
        if (kl_fused_path(NK)) {
            if (FOLLOW) kl_await_opaque(P, pbase + NK + 1);
            const double dinv = I[act ? r : 0];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (keeps the compiler from moving the read below the store; the LDS serves a wave in order)
            if (FOLLOW) kl_publish(Mdone, done_value);
            kl_row_load<NK>(m, MX, r, act);
            return dinv;
        }
        kl_row_load<NK>(m, MX, r, act);
        kl_sync();
        if (FOLLOW) kl_await_opaque(P, pbase + NK + 1);
        const double dinv = I[act ? r : 0];
        if (FOLLOW) kl_publish(Mdone, done_value);
        return dinv;
    } else {
#pragma unroll
        for (int k = 0; k < NK; ++k) m[k] = (k == r) ? 1.0 : 0.0;
        if (FOLLOW)
            kl_follow_LinvT<NK>(m, C, I, P, pbase);
        else
            kl_row_times_LinvT<NK>(m, C, I);
        if (FOLLOW) kl_await_opaque(P, pbase + NK + 1);  // the LAST reciprocal pivot is written after the last image was announced
        const double dinv = I[act ? r : 0];  // (read before the chain is told to go on: its next block overwrites I)
        kl_store_rows<NK>(m, MX, r, act);
        if (FOLLOW) kl_publish(Mdone, done_value);
        return dinv;
    }
}

#include "knot_subst.h"
// ---- a substitution step out of the chain's own area (fused path; qp.hip: QP_FWD_IN_FACTOR, the predictor's forward pass) -----------------
// When the companion has announced M_jp (Mdone) the chain's own area holds all a forward step of knot jp needs: M_jp in MX -- rows of
// stride KL_LD, zeros left of the diagonal (kl_tiles_scatter): the layout of a stage buffer of solve_staged --, 1 / d_jp in I, and on the
// fused path neither is written again before the chain's factorisation of its NEXT block (I) and the companion's scatter behind it (MX).
// The step (knot_subst.h, the one solve_staged takes: same operations, same order, same M bits) runs behind the update of the next block,
// in front of the wait for that block's image, which it fills.  z_jp goes to global memory (z_out: this lane's entry).
// Where the step's small vectors live (KfSlots, doubles from KlArea::C):
//   * The panel images end at kp_img_total(NK); the C / U region is (NK + 1) KL_LDU doubles, and on the fused path nothing else is kept
//     in it (U does not exist, the scatter's padding lands in row NK of MX).  Its tail [PAD, CSZ) is written by nobody but these steps and
//     was cleared by the caller at the start of the factorisation (twisted_factor): the zeros behind A and in front of Z (the products read A[NK .. 3 CH - 1] and Z[NK - 3 CH .. -1]; one
//     run of 10 serves both), then Z and V -- V is what travels from step to step and on to the middle block --, then zeros up to CSZ,
//     which is where the product by rows reads the up to 9 doubles in front of MX.  (Columns 36, 37 of MX's rows are never written: zeros.)
//   * A (r') and the 64 partial sums overlay the END OF THE LAST PANEL IMAGE.  That is idle in the window: the companion has read every
//     image of block jp before its scatter, hence before it announced Mdone (kl_inverse_rows: kl_inverse_panels, kl_tiles_scatter, publish;
//     behind the announcement it only reads MX), and the next writer of the images is this wave's factorisation of the next block, in
//     program order behind the step.  Nothing outlives the step there.
//   * The product by columns would read rows NK + 1 .. 3 CH - 1 behind MX: I (finite), then the next area, the progress words, the
//     assembly images -- not this wave's to vouch for: ks_matvec_cols<NK, GUARD = true> drops those terms.
// No branch inside the step: lanes >= NK compute row 0's values (rr = 0 throughout) and store them where lane 0 does.
template <int NK>
__device__ __forceinline__ void kl_forward_step(kl_lds* base, __attribute__((address_space(1))) double* z_out, double rhs_r, double e0, double e1, double e2, int r) {
    using A = KlArea<NK>;
    using F = KfSlots<NK>;
    static_assert(F::CSZ == A::CSZ, "knot_subst.h out of step with KlArea");
    kl_lds *C = base + A::C, *MX = base + A::MX, *I = base + A::I;
    const int rr = r < NK ? r : 0, g3 = 3 * (rr / 3);
    ks_step_forward<NK, true>((const kl_lds*)MX, I[rr], rhs_r, true, e0, e1, e2, C + F::A, C + F::Z, C + F::V, C + F::PS, r, g3, rr, [] { kl_sync(); },
                              [&](double z) { *z_out = z; });
}
// the middle block's step out of the area `base` that holds M_mid and 1 / d_mid: v = rhs_mid[rr] less both chains' coupling terms (their last
// v: the V slots of their areas); returns x_mid[rr].  A, Z and the partial sums: base's slots (the middle block's images have been read)
template <int NK>
__device__ __forceinline__ double kl_middle_step(kl_lds* base, double v, int r) {
    using A = KlArea<NK>;
    using F = KfSlots<NK>;
    kl_lds* C = base + A::C;
    const int rr = r < NK ? r : 0;
    return ks_step_middle<NK, true>((const kl_lds*)(base + A::MX), (const kl_lds*)(base + A::I + rr), v, C + F::A, C + F::Z, C + F::PS, r, rr, [] { kl_sync(); });
}
