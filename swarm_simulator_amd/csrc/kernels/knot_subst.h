// One knot step of the substitutions T du = rhs with the explicit M_j = L_j^-T of the twisted factorisation, stated once: for
// solve_staged (qp_wave_solve.inc, M_j in a stage buffer), for the forward steps the chain waves take along the factorisation
// (qp_wave_factor.inc, QP_FWD_IN_FACTOR: M_j in the chain's own area) and for the host (tests/knot_subst/subst_main.cpp, g++: one thread
// per lane, `sync` a barrier).  Plain C++ templates over the pointer types (LDS pointers on the device, double* on the host).
//   forward   r'  = rhs_j - T_{j,jp} v_jp          (3x3-block sparse)         y = M_j' r'      z_j = D_j^-1 y      v_j = M_j z_j
//   middle    forward with both neighbours' v, then x_mid = M z
//   backward  w   = T_{jn,j}' x_jn                 x_j = M_j (z_j - D_j^-1 M_j' w)
// A step is written for ONE lane of the 64 that take it together; sync() orders the lanes' stores before their later loads.
//
// The two products of a chain step use M_j's triangle with ALL 64 lanes: a lane owns a PIECE -- KsPieces::CH consecutive terms of one row
// (or column) -- instead of a whole row, of which only NK <= 36 exist and whose lower half is zeros: 15 loads and multiply-adds per
// lane instead of 36, then the up to three pieces of a row meet through 64 doubles of LDS.  Chunk t of the product by rows covers the
// columns NK - CH (t + 1) .. NK - 1 - CH t (anchored at the right edge: row r needs the chunks with NK - 1 - CH t >= r), chunk t of the
// product by columns the rows CH t .. CH t + CH - 1 (anchored at the top: column c needs the chunks with CH t <= c).  Terms that fall
// left of / below the diagonal multiply the matrix's zeros, terms outside the block multiply the zero padding of the VECTOR (KS_VPAD
// slots either side; whatever finite number sits at the matrix address): no masks, no branches.
// GUARD (product by columns): the rows behind the padding row NK of the matrix -- up to row CH * 3 - 1 -- are not the caller's to keep
// finite (a chain's area is followed by the next area, the progress words, images that may never have been written): their terms are
// replaced by zeros, so that a NaN there cannot meet the vector's zero padding.  The sums of the rows < NK do not change.
#pragma once
#include "knot_panel_layout.h"
#ifndef KS_FN
#define KS_FN __host__ __device__ __forceinline__
#endif
#ifndef KL_LD
#define KL_LD 38  // knot_lds.inc
#endif
#ifndef KL_I
#define KL_I 40   // knot_lds.inc
#endif
#ifndef KL_LDU
#define KL_LDU 50  // knot_lds.inc
#endif
#define KS_VPAD 16                          // zero slots either side of a chain vector
#define KS_VLEN (KS_VPAD + KL_I + KS_VPAD)  // doubles per vector (the slot NK + 12 takes the writes of the lanes without a row)
template <int NK>
struct KsPieces {
    static constexpr int CH = (NK * 15 + 35) / 36;  // 36 -> 15, 27 -> 12, 18 -> 8, 9 -> 4
    static constexpr int N0 = NK, N1 = NK - CH > 0 ? NK - CH : 0, N2 = NK - 2 * CH > 0 ? NK - 2 * CH : 0;
    static_assert(NK - 3 * CH <= 0 && N0 + N1 + N2 <= 64, "three chunks, one wavefront");
    static_assert(3 * CH - NK <= KS_VPAD && 3 * CH - 1 - (NK - 1) <= KS_VPAD, "vector padding");
    static KS_FN void of_lane(int lane, int& idx, int& t) {
        t = lane < N0 ? 0 : (lane < N0 + N1 ? 1 : 2);
        idx = lane < N0 ? lane : (lane < N0 + N1 ? lane - N0 : (lane < N0 + N1 + N2 ? lane - N0 - N1 : 0));
    }
};
// sum_k Mst[k][c] * b[k] for column c = rr (lanes rr < NK; b: vector base, i.e. entry 0); psum: 64 doubles of scratch
template <int NK, bool GUARD = false, class MP, class VP, class PP, class SY>
KS_FN double ks_matvec_cols(MP Mst, VP b, PP psum, int lane, SY&& sync) {
    using P = KsPieces<NK>;
    int idx, t;
    P::of_lane(lane, idx, t);
    const int k0 = P::CH * t, c = k0 + idx;
    const auto mp = Mst + k0 * KL_LD + c;
    const auto bp = b + k0;
    double mv[P::CH], bv[P::CH];
#pragma unroll
    for (int j = 0; j < P::CH; ++j) {
        mv[j] = mp[j * KL_LD], bv[j] = bp[j];
        if (GUARD && 2 * P::CH + j > NK) mv[j] = k0 + j > NK ? 0.0 : mv[j];
    }
    double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < P::CH; ++j) {
        if (j % 3 == 0) s0 += mv[j] * bv[j];
        if (j % 3 == 1) s1 += mv[j] * bv[j];
        if (j % 3 == 2) s2 += mv[j] * bv[j];
    }
    psum[lane] = (s0 + s1) + s2;
    sync();
    const int cc = lane < NK ? lane : 0;
    double r = psum[cc];
    if (P::N1 > 0) r += cc >= P::CH ? psum[P::N0 + cc - P::CH] : 0.0;
    if (P::N2 > 0) r += cc >= 2 * P::CH ? psum[P::N0 + P::N1 + cc - 2 * P::CH] : 0.0;
    return r;
}
// sum_k Mst[r][k] * b[k] for row r = rr
template <int NK, class MP, class VP, class PP, class SY>
KS_FN double ks_matvec_rows(MP Mst, VP b, PP psum, int lane, SY&& sync) {
    using P = KsPieces<NK>;
    int idx, t;
    P::of_lane(lane, idx, t);
    const int k0 = NK - P::CH * (t + 1);  // may be negative: the vector is padded, the matrix address holds some finite number
    const auto mp = Mst + idx * KL_LD + k0;
    const auto bp = b + k0;
    double mv[P::CH], bv[P::CH];
#pragma unroll
    for (int j = 0; j < P::CH; ++j) mv[j] = mp[j], bv[j] = bp[j];
    double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < P::CH; ++j) {
        if (j % 3 == 0) s0 += mv[j] * bv[j];
        if (j % 3 == 1) s1 += mv[j] * bv[j];
        if (j % 3 == 2) s2 += mv[j] * bv[j];
    }
    psum[lane] = (s0 + s1) + s2;
    sync();
    const int rr = lane < NK ? lane : 0;
    double r = psum[rr];
    if (P::N1 > 0) r += rr < P::N1 ? psum[P::N0 + rr] : 0.0;
    if (P::N2 > 0) r += rr < P::N2 ? psum[P::N0 + P::N1 + rr] : 0.0;
    return r;
}

// The step bodies.  Mst: M_j, row stride KL_LD, zeros left of the diagonal; A, Z, V: the chain's vectors (entry 0; A and Z with zero
// padding either side, see above), ps: 64 doubles; lane: 0 .. 63; g3 = 3 * (row / 3) of the lane's row; rs: the slot the lane writes (its
// row, or for a lane without one a slot nobody's products see -- or row 0, whose values such a lane computes).
// forward: rhs_r = rhs_j[row], e0..e2 = row `row` of T_{j,jp} (has_prev), v_jp in V; put_z(z) takes z_j[row]; v_j replaces v_jp in V.
template <int NK, bool GUARD = false, class MP, class VP, class PP, class SY, class ZF>
KS_FN void ks_step_forward(MP Mst, double dinv, double rhs_r, bool has_prev, double e0, double e1, double e2, VP A, VP Z, VP V, PP ps, int lane, int g3, int rs,
                           SY&& sync, ZF&& put_z) {
    double v = rhs_r;
    if (has_prev) v -= e0 * V[g3] + e1 * V[g3 + 1] + e2 * V[g3 + 2];  // r' = rhs_j - T_{j,jp} v_jp
    sync();
    A[rs] = v;
    sync();
    const double z = dinv * ks_matvec_cols<NK, GUARD>(Mst, A, ps, lane, sync);
    Z[rs] = z;
    put_z(z);
    sync();
    const double vj = ks_matvec_rows<NK>(Mst, Z, ps, lane, sync);
    sync();
    V[rs] = vj;
}
// middle: v = rhs_mid[row] less both neighbours' coupling terms (ks_couple); dinv_p[0] = 1 / d_mid[row]; returns x_mid[row]
KS_FN double ks_couple(double e0, double e1, double e2, double v0, double v1, double v2) { return e0 * v0 + e1 * v1 + e2 * v2; }
template <int NK, bool GUARD = false, class MP, class DP, class VP, class PP, class SY>
KS_FN double ks_step_middle(MP Mst, DP dinv_p, double v, VP A0, VP Z0, PP ps, int lane, int rs, SY&& sync) {
    A0[rs] = v;
    sync();
    const double z = dinv_p[0] * ks_matvec_cols<NK, GUARD>(Mst, A0, ps, lane, sync);
    Z0[rs] = z;
    sync();
    const double x = ks_matvec_rows<NK>(Mst, Z0, ps, lane, sync);
    sync();
    return x;
}
// backward: e0..e2 = column `row` of T_{jn,j} within its 3x3 block, x_jn in V, z_p[0] = z_j[row]; x_j replaces x_jn in V and is returned
template <int NK, bool GUARD = false, class MP, class ZP, class VP, class PP, class SY>
KS_FN double ks_step_backward(MP Mst, double dinv, ZP z_p, double e0, double e1, double e2, VP A, VP Z, VP V, PP ps, int lane, int g3, int rs, SY&& sync) {
    // w = T_{jn,j}' x_jn: column rr of the 3x3 block of its (agent, dim) group, rows g3 .. g3+2 (x_jn sits in V)
    const double wv = e0 * V[g3] + e1 * V[g3 + 1] + e2 * V[g3 + 2];
    sync();
    A[rs] = wv;
    sync();
    const double u = z_p[0] - dinv * ks_matvec_cols<NK, GUARD>(Mst, A, ps, lane, sync);
    Z[rs] = u;
    sync();
    const double x = ks_matvec_rows<NK>(Mst, Z, ps, lane, sync);
    sync();
    V[rs] = x;
    return x;
}

// Where the vectors of a forward step live that a chain wave takes out of its own area (doubles from KlArea::C; wave_forward_step in
// qp_wave_factor.inc has the argument): A and the partial sums at the end of the last panel image, then -- in the tail of the C / U region
// that the fused path keeps nothing in -- 10 zeros (behind A, in front of Z), Z, V, and zeros up to the region's end, in front of MX.
template <int NK>
struct KfSlots {
    static constexpr int CSZ = (NK + 1) * KL_LDU;  // KlArea<NK>::CSZ
    static constexpr int PAD = kp_img_total(NK), Z = PAD + 10, V = Z + NK, END = V + NK, A = PAD - NK, PS = A - 64;
    static_assert(KsPieces<NK>::CH * 3 - NK <= 10, "the run of zeros between A and Z");
    static_assert(END + 9 <= CSZ && PS >= kp_img_off(NK, kp_np(NK) - 1), "forward-step vectors: tail of the C region, end of the last panel image");
};
