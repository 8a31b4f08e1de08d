// Where a knot's inverse factor lives in global memory (QpWs::Lf), stated once: for the companion wave that writes it (knot_inverse,
// qp_wave_factor.inc), for the staging threads that read it (solve_staged, qp_wave_solve.inc) and, being plain C, for the CPU
// (tests/test_knot_factor_layout.py).
//
// What a knot j leaves for the substitutions is M_j = L_j^-T, upper triangular of order NK <= 36, and the NK reciprocal pivots 1 / d_j.
// A slot holds them as ONE CONTIGUOUS RUN of doubles:
//   row r of M_j from column kf_first(NK, r) to NK - 1, rows 0, 1, .. NK - 1 one behind the other;
//   even NK: kf_first = r & ~1 -- the companion stores 16 bytes (two columns) per lane and instruction, so an odd row starts with the zero
//            left of its diagonal, every row starts at an even offset and no 16-byte pair of the run straddles two rows;
//   odd NK:  kf_first = r, 8-byte elements;
//   1 / d_j at the next even offset behind the triangle; the slot stride is the run rounded up to 16 doubles (a 128-byte line).
// NK = 36: 684 + 36 = 720 doubles = 45 lines exactly.  (The square [NK][NK] image this replaces spread the same 702 useful doubles over
// 65 .. 69 lines, and HBM moves whole lines: kf_sq_* keeps its addressing for the A/B lever QP_LF_PACKED = 0.)
// QpWs::Lf starts on a 128-byte boundary (carve, qp_base.inc).
#pragma once
#ifndef KF_FN
#define KF_FN __host__ __device__ inline
#endif

KF_FN constexpr int kf_first(int nk, int r) { return (nk & 1) ? r : (r & ~1); }  // first stored column of row r
KF_FN constexpr int kf_len(int nk, int r) { return nk - kf_first(nk, r); }
// offset of row r's first stored entry = sum of kf_len over the rows before it (r = nk: doubles of the whole triangle)
KF_FN constexpr int kf_row(int nk, int r) {
    return (nk & 1) ? r * nk - r * (r - 1) / 2 : 2 * (r / 2) * nk - 2 * (r / 2) * (r / 2 - 1) + (r & 1) * (nk - (r & ~1));
}
KF_FN constexpr int kf_elem(int nk, int r, int k) { return kf_row(nk, r) + k - kf_first(nk, r); }  // M_j[r][k], k >= kf_first(nk, r)
KF_FN constexpr int kf_tri(int nk) { return kf_row(nk, nk); }
KF_FN constexpr int kf_dinv(int nk) { return (kf_tri(nk) + 1) & ~1; }   // 1 / d_j [nk]
KF_FN constexpr int kf_run(int nk) { return kf_dinv(nk) + nk; }         // doubles of the run
KF_FN constexpr int kf_stride(int nk) { return (kf_run(nk) + 15) & ~15; }  // doubles per knot

// the square image (QP_LF_PACKED = 0): M_j [nk][nk] row-major, then 1 / d_j; 40 = KL_I of knot_lds.inc
KF_FN constexpr int kf_sq_elem(int nk, int r, int k) { return r * nk + k; }
KF_FN constexpr int kf_sq_dinv(int nk) { return nk * nk; }
KF_FN constexpr int kf_sq_stride(int nk) { return nk * nk + 40; }

// ---- staging: the run in UNITS, what one staging thread loads with one instruction -- a 16-byte pair for even NK, a double for odd NK
KF_FN constexpr int kf_unit(int nk) { return (nk & 1) ? 1 : 2;  }
KF_FN constexpr int kf_units(int nk) { return (kf_run(nk) + kf_unit(nk) - 1) / kf_unit(nk); }
// A step stages two knots, the left chain's and the right chain's: unit e < 2 kf_units(nk) of the two runs, one behind the other, belongs to
// chain kf_unit_side and starts at offset kf_unit_off of that knot's slot.  Staging thread t of NST has the units t, t + NST, ...
KF_FN constexpr int kf_unit_side(int nk, int e) { return e >= kf_units(nk) ? 1 : 0; }
KF_FN constexpr int kf_unit_off(int nk, int e) { return (e - kf_unit_side(nk, e) * kf_units(nk)) * kf_unit(nk); }
// the row that holds offset o < kf_tri(nk): a float estimate of the root of kf_row(r) = o, made exact in integers
KF_FN int kf_row_of(int nk, int o) {
    int r;
    if (nk & 1) {  // r nk - r (r - 1) / 2 <= o
        const float b = (float)(2 * nk + 1);
        r = (int)((b - __builtin_sqrtf(b * b - 8.0f * (float)o)) * 0.5f);
    } else {  // pairs of rows p = r / 2: 2 p (nk + 1) - 2 p^2 <= o
        const float b = (float)(nk + 1);
        r = 2 * (int)((b - __builtin_sqrtf(b * b - 2.0f * (float)o)) * 0.5f);
    }
    r = r < 0 ? 0 : (r > nk - 1 ? nk - 1 : r);
    while (r > 0 && kf_row(nk, r) > o) --r;
    while (r + 1 < nk && kf_row(nk, r + 1) <= o) ++r;
    return r;
}
// where the double at offset o of the run goes in a chain's half of a stage buffer (M_j with rows ld apart, 1 / d_j at sm), or -1 for
// the gap between an odd triangle and 1 / d_j.  The unit at o covers o .. o + kf_unit - 1, consecutive there as here.
KF_FN int kf_stage_dst(int nk, int o, int ld, int sm) {
    if (o >= kf_dinv(nk)) return o < kf_run(nk) ? sm + (o - kf_dinv(nk)) : -1;
    if (o >= kf_tri(nk)) return -1;
    const int r = kf_row_of(nk, o);
    return r * ld + kf_first(nk, r) + (o - kf_row(nk, r));
}
