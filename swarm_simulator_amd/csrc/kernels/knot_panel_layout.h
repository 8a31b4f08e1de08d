// Index maps of the panel-blocked knot factorisation (knot_lds.inc, kl_ldl_panels / kl_inverse_panels): plain C, so that their
// invariants are checked on the CPU (tests/test_knot_panel_layout.py).
//
// A knot block (NK x NK, NK <= 36) is padded with a unit diagonal to 16 NT rows and cut into 16 x 16 tiles that live in the
// accumulators of v_mfma_f64_16x16x4_f64; a panel is 4 columns, the k of that instruction.  Operand layouts of the instruction
// (D = A B + C; A 16 x 4, B 4 x 16, C / D 16 x 16), one double per lane for A and B, four for C / D:
//   A    row = lane & 15, k   = lane >> 4
//   B    k   = lane >> 4, col = lane & 15
//   C/D  col = lane & 15, row = (lane >> 4) + 4 reg
// The chain wave keeps the UPPER tiles of the symmetric Schur complement S (ti <= tj): row 4p + k of panel p is then register p % 4 of
// lane (col & 15, k) of the tiles (p / 4, tj) -- every lane owns one entry of the panel per tile.  The following wave keeps the LOWER
// tiles of the running inverse N = L^-1 (ti >= tj): the 4 panel rows of N, the B operand of its rank-4 update, are the same registers.
#pragma once
#ifndef KP_FN
#define KP_FN __host__ __device__ inline
#endif

#define KP_W 4     // columns of a panel
#define KP_T 16    // rows / columns of a tile

KP_FN constexpr int kp_nt(int nk) { return (nk + KP_T - 1) / KP_T; }   // tiles per side
KP_FN constexpr int kp_np(int nk) { return (nk + KP_W - 1) / KP_W; }   // panels (the last one may reach into the padding)
KP_FN constexpr int kp_rows(int nk) { return KP_T * kp_nt(nk); }       // padded size

// operand layouts
KP_FN constexpr int kp_a_row(int lane) { return lane & 15; }
KP_FN constexpr int kp_a_k(int lane) { return lane >> 4; }
KP_FN constexpr int kp_b_col(int lane) { return lane & 15; }
KP_FN constexpr int kp_b_k(int lane) { return lane >> 4; }
KP_FN constexpr int kp_cd_col(int lane) { return lane & 15; }
KP_FN constexpr int kp_cd_row(int lane, int reg) { return (lane >> 4) + 4 * reg; }

// packed index of a triangle's tile: upper (ti <= tj) for S, lower (ti >= tj) for N; both count 0 .. nt (nt + 1) / 2 - 1
KP_FN constexpr int kp_ntiles(int nt) { return nt * (nt + 1) / 2; }
KP_FN constexpr int kp_upper(int ti, int tj, int nt) { return ti * nt - ti * (ti - 1) / 2 + (tj - ti); }
KP_FN constexpr int kp_lower(int ti, int tj) { return ti * (ti + 1) / 2 + tj; }

// panel bookkeeping: panel p lies in tile row / column p / 4 and is register p % 4 of the C/D layout there
KP_FN constexpr int kp_panel_tile(int p) { return p / (KP_T / KP_W); }
KP_FN constexpr int kp_panel_reg(int p) { return p % (KP_T / KP_W); }
// first tile row of S that still changes when panel p is eliminated (the panel's own tile row is finished with its last panel)
KP_FN constexpr int kp_first_live_tile(int p) { return kp_panel_tile(p + 1); }

// Rank-NK update of the next block formed in the tiles (kl_fused_update): S -= X D^-1 X' with X = Cpl M, Cpl 3x3-block diagonal and
// M = L^-T upper triangular.  Row r of X combines the three rows kp_x_group(r) .. + 2 of M, so X[r][k] = 0 for k < kp_x_group(r): the rows
// of tile row t only see the k-steps (4 columns each) from kp_x_first_kstep(t) on, and the upper tile (ti, tj) those of its LATER tile row tj.
KP_FN constexpr int kp_x_group(int row) { return 3 * (row / 3); }
KP_FN constexpr int kp_x_first_kstep(int t) { return kp_x_group(KP_T * t) / KP_W; }
KP_FN constexpr int kp_ksteps(int nk) { return (nk + KP_W - 1) / KP_W; }

// LDS image of the panels (doubles, relative to KlArea::C): panel p holds the padded rows j of S's columns 4p .. 4p+3 as they are when
// the panels before p have been eliminated, entry (j, k) = S[j][4p + k] -- 32 bytes per row, one ds_read_b128 pair
KP_FN constexpr int kp_img_doubles(int nk) { return kp_rows(nk) * KP_W; }
KP_FN constexpr int kp_img_off(int nk, int p) { return p * kp_img_doubles(nk); }
KP_FN constexpr int kp_img_entry(int row, int k) { return row * KP_W + k; }
KP_FN constexpr int kp_img_total(int nk) { return kp_np(nk) * kp_img_doubles(nk); }
