// qp_tiled.inc — the tiled path (nk > 36): the block-tridiagonal factorisation and the substitutions on 16x16 MFMA tiles (ld4T .. solve_tiled),
// and the identity padding its block layout needs (init_block_pads).  Included by qp.hip after the wave-register path; needs QP_THREADS of qp.hip,
// QpDims, QpWs (qp_base.inc) and d4 (qp_wave_factor.inc).

// ------------------------------------------------------------------------------------------------------------
// tiled path (nk > 36: batches of 5..64 agents, e.g. plan/batch_size = 8 or the joint QP of a whole mission).
// Knot blocks live in global memory (L2-resident), row-major with the leading dimension ld = nk rounded up to 16
// (padding rows/columns are identity), cut into 16x16 tiles for v_mfma_f64_16x16x4_f64:
//   factor, per knot j, LEFT-looking over tile columns p of the stacked panel [A_j ; C_j]  (A_j = T_jj - B B',
//   B = L_{j,j-1}, C_j = T_{j+1,j}):
//     (1) tile (ti,p) -= B(ti,:) B(p,:)' + A(ti,:16p) A(p,:16p)'      (8 waves, one MFMA tile each, K = ld + 16p)
//         C(ti,p)    -= C(ti,:16p) A(p,:16p)'
//     (2) every wave factors the 16x16 diagonal tile in registers (lane = row, v_readlane broadcasts) and
//     (3) solves its share of the rows below (one row per lane):  X <- X L_pp^{-T}
//   two workgroup barriers per tile column.  L_jj overwrites the lower triangle of Td[j], L_{j+1,j} overwrites To[j].
//   substitutions: block matvecs by the whole workgroup, the triangular solves by wave 0 tile by tile.
// ------------------------------------------------------------------------------------------------------------
// memory helpers of the tiled path: LDS = true turns the generic pointer into an LDS one (ds_read/ds_write instead of flat)
#define AS_LDS __attribute__((address_space(3)))
template <bool LDS>
__device__ __forceinline__ d4 ld4T(const double* p) {
    if (LDS) return *(const AS_LDS d4*)(p);
    return *reinterpret_cast<const d4*>(p);
}
template <bool LDS>
__device__ __forceinline__ double ldT(const double* p) {
    if (LDS) return *(const AS_LDS double*)(p);
    return *p;
}
template <bool LDS>
__device__ __forceinline__ void stT(double* p, double v) {
    if (LDS)
        *(AS_LDS double*)(p) = v;
    else
        *p = v;
}
template <bool LDS>
__device__ __forceinline__ void st4T(double* p, d4 v) {
    if (LDS)
        *(AS_LDS d4*)(p) = v;
    else
        *reinterpret_cast<d4*>(p) = v;
}

// acc += X(16 x K) Y(16 x K)'   (X, Y row-major, K a multiple of 16).  Lane (i = l&15, g = l>>4) loads X[i][k0+4g .. +3]:
// the four MFMA steps of a 16-chunk use k = 4g + s on both operands, a permutation of the summation index.
template <bool LDS>
__device__ __forceinline__ void tile_nt(d4& acc, const double* X, int ldx, const double* Y, int ldy, int K, int lane) {
    const int i = lane & 15, g = lane >> 4;
    const double* xp = X + (size_t)i * ldx + 4 * g;
    const double* yp = Y + (size_t)i * ldy + 4 * g;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const d4 xa = ld4T<LDS>(xp + k0), yb = ld4T<LDS>(yp + k0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[0], yb[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[1], yb[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[2], yb[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[3], yb[3], acc, 0, 0, 0);
    }
}

// C(16x16) -= acc   (C/D layout: row = (l>>4) + 4*reg, col = l&15)
template <bool LDS>
__device__ __forceinline__ void tile_sub(double* C, int ldc, const d4& acc, int lane) {
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double* cp = C + (size_t)(g + 4 * r) * ldc + i;
        stT<LDS>(cp, ldT<LDS>(cp) - acc[r]);
    }
}

// global (ld x ld, dense) -> LDS (leading dimension ldl): all loads of a thread are issued before its LDS stores, so the
// copy costs one memory round trip, not one per element
__device__ __forceinline__ void stage_block(double* dst, int ldl, const double* src, int ld) {
    const int total = ld * ld;
    for (int base = threadIdx.x; base < total; base += 8 * QP_THREADS) {
        double tmp[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int it = base + u * QP_THREADS;
            tmp[u] = it < total ? src[it] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int it = base + u * QP_THREADS;
            if (it < total) *(AS_LDS double*)(dst + (it / ld) * ldl + it % ld) = tmp[u];
        }
    }
}

// one knot of the tiled factorisation: A (ld x ld, lower) <- chol(A - B B'), C <- C A^{-T}.  A, B, C may live in global
// memory or in LDS (generic pointers; leading dimension ld doubles, order 16*NT)
template <bool LDS>
__device__ __forceinline__ bool factor_knot_tiled(double* A, const double* B, double* C, int ld, int NT, int* flag) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int NW = QP_THREADS / 64;
    const int n = 16 * NT;
    for (int p = 0; p < NT; ++p) {
        const int nA = NT - p, nC = (C && p > 0) ? NT : 0;
        if (B || p > 0) {
            for (int t = wave; t < nA + nC; t += NW) {
                d4 acc = d4{0, 0, 0, 0};
                const double* Ap = A + (size_t)p * 16 * ld;
                if (t < nA) {
                    const int ti = p + t;
                    if (B) tile_nt<LDS>(acc, B + (size_t)ti * 16 * ld, ld, B + (size_t)p * 16 * ld, ld, n, lane);
                    if (p > 0) tile_nt<LDS>(acc, A + (size_t)ti * 16 * ld, ld, Ap, ld, 16 * p, lane);
                    tile_sub<LDS>(A + (size_t)ti * 16 * ld + 16 * p, ld, acc, lane);
                } else {
                    const int ti = t - nA;
                    tile_nt<LDS>(acc, C + (size_t)ti * 16 * ld, ld, Ap, ld, 16 * p, lane);
                    tile_sub<LDS>(C + (size_t)ti * 16 * ld + 16 * p, ld, acc, lane);
                }
            }
            __threadfence_block();
            __syncthreads();
        }
        // diagonal tile: every wave factors its own register copy (lane&15 = row)
        double a[16];
        {
            const double* dp = A + (size_t)(16 * p + (lane & 15)) * ld + 16 * p;
            const d4 v0 = ld4T<LDS>(dp), v1 = ld4T<LDS>(dp + 4), v2 = ld4T<LDS>(dp + 8), v3 = ld4T<LDS>(dp + 12);
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = v0[k], a[4 + k] = v1[k], a[8 + k] = v2[k], a[12 + k] = v3[k];
        }
        double inv;  // reciprocal of this lane's diagonal entry: the row solves below multiply instead of dividing
        const bool ok = chol_rows<16>(a, inv);
        if (!ok && tid == 0) *flag = 1;
        // rows below in A, all rows of C:  x <- x L_pp^{-T}
        const int nbelow = n - 16 * (p + 1), total = nbelow + (C ? n : 0);
        for (int base = 0; base < total; base += QP_THREADS) {
            const int idx = base + tid;
            const bool act = idx < total;
            double* rp = !act ? A : (idx < nbelow ? A + (size_t)(16 * (p + 1) + idx) * ld + 16 * p : C + (size_t)(idx - nbelow) * ld + 16 * p);
            double x[16];
            const d4 v0 = ld4T<LDS>(rp), v1 = ld4T<LDS>(rp + 4), v2 = ld4T<LDS>(rp + 8), v3 = ld4T<LDS>(rp + 12);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = v0[k], x[4 + k] = v1[k], x[8 + k] = v2[k], x[12 + k] = v3[k];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                double sv = x[c];
#pragma unroll
                for (int k = 0; k < c; ++k) sv -= x[k] * rl(a[k], c);
                x[c] = sv * rl(inv, c);
            }
            if (act) {
                st4T<LDS>(rp, d4{x[0], x[1], x[2], x[3]});
                st4T<LDS>(rp + 4, d4{x[4], x[5], x[6], x[7]});
                st4T<LDS>(rp + 8, d4{x[8], x[9], x[10], x[11]});
                st4T<LDS>(rp + 12, d4{x[12], x[13], x[14], x[15]});
            }
        }
        __threadfence_block();
        __syncthreads();
        if (*flag) return false;
        if (wave == 0 && lane < 16) {  // nobody reads the diagonal tile again during the factorisation
            double* dp = A + (size_t)(16 * p + lane) * ld + 16 * p;
#pragma unroll
            for (int k = 0; k < 16; ++k) stT<LDS>(dp + k, k <= lane ? a[k] : 0.0);
        }
    }
    return true;
}

__device__ bool factor_tiled(const QpDims& d, const QpWs& w, int* flag, double* lds, int lds_avail) {
    const int ld = d.ldb, NT = ld / 16, tid = threadIdx.x;
    if (tid == 0) *flag = 0;
    __syncthreads();
    const int ldl = ld + 2;  // LDS leading dimension: rows 16 apart fall into different banks
    if (3 * ld * ldl <= lds_avail) {
        // LDS-resident variant (nk <= 72): the three blocks of a knot stay in LDS, every dependent step of the panel
        // loop is an LDS round trip instead of an L2 one.  T_{j+1,j} is generated in place from Ek (it is 3x3-block
        // diagonal), L_{j,j-1} is the previous knot's C buffer.
        double* bufA = lds;
        double* bufB = lds + (size_t)ld * ldl;
        double* bufC = lds + 2 * (size_t)ld * ldl;
        for (int j = 0; j < d.nj; ++j) {
            const double* Ag = w.Td + (size_t)j * ld * ld;
            stage_block(bufA, ldl, Ag, ld);
            const bool hasC = j + 1 < d.nj;
            if (hasC) {
                const double* E = w.Ek + 9 * (j + 1);
                for (int it = tid; it < ld * ld; it += QP_THREADS) {
                    const int rr = it / ld, cc = it % ld;
                    bufC[rr * ldl + cc] = (rr / 3 == cc / 3 && rr < d.nk && cc < d.nk) ? E[3 * (cc % 3) + (rr % 3)] : 0.0;
                }
            }
            __syncthreads();
            if (!factor_knot_tiled<true>(bufA, j > 0 ? bufB : nullptr, hasC ? bufC : nullptr, ldl, NT, flag)) return false;
            __syncthreads();  // the diagonal tiles are written late by wave 0
            double* Aw = w.Td + (size_t)j * ld * ld;
            for (int it = tid; it < ld * ld; it += QP_THREADS) Aw[it] = bufA[(it / ld) * ldl + it % ld];
            if (hasC) {
                double* Cw = w.To + (size_t)j * ld * ld;
                for (int it = tid; it < ld * ld; it += QP_THREADS) Cw[it] = bufC[(it / ld) * ldl + it % ld];
            }
            double* t = bufB;
            bufB = bufC, bufC = t;
            __syncthreads();
        }
    } else {
        for (int j = 0; j < d.nj; ++j) {
            double* A = w.Td + (size_t)j * ld * ld;
            const double* B = j > 0 ? w.To + (size_t)(j - 1) * ld * ld : nullptr;
            double* C = j + 1 < d.nj ? w.To + (size_t)j * ld * ld : nullptr;
            if (!factor_knot_tiled<false>(A, B, C, ld, NT, flag)) return false;
        }
    }
    __threadfence_block();
    __syncthreads();
    return true;
}

// v <- L^{-1} v for one knot block (wave 0; v in LDS, ld entries)
template <bool LDS>
__device__ __forceinline__ void trisolve_fwd(const double* L, int ld, int n, double* v, int lane) {
    const int NT = n / 16, i = lane & 15;
    for (int p = 0; p < NT; ++p) {
        double a[16];
        const double* dp = L + (size_t)(16 * p + i) * ld + 16 * p;
        const d4 v0 = ld4T<LDS>(dp), v1 = ld4T<LDS>(dp + 4), v2 = ld4T<LDS>(dp + 8), v3 = ld4T<LDS>(dp + 12);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = v0[k], a[4 + k] = v1[k], a[8 + k] = v2[k], a[12 + k] = v3[k];
        double x = v[16 * p + i], dgl = 1.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) dgl = (i == k) ? a[k] : dgl;
        const double inv = 1.0 / dgl;  // one division per tile instead of one per dependent step
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const double xc = rl(x, c) * rl(inv, c);
            x = (i == c) ? xc : (i > c ? x - a[c] * xc : x);
        }
        if (lane < 16) v[16 * p + i] = x;
        for (int r0 = 16 * (p + 1); r0 < n; r0 += 64) {
            const int r = r0 + lane;
            const bool act = r < n;
            const double* rp = L + (size_t)(act ? r : 0) * ld + 16 * p;
            const d4 u0 = ld4T<LDS>(rp), u1 = ld4T<LDS>(rp + 4), u2 = ld4T<LDS>(rp + 8), u3 = ld4T<LDS>(rp + 12);
            double sv = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                sv += u0[k] * rl(x, k) + u1[k] * rl(x, 4 + k) + u2[k] * rl(x, 8 + k) + u3[k] * rl(x, 12 + k);
            if (act) v[r] -= sv;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// v <- L^{-T} v
template <bool LDS>
__device__ __forceinline__ void trisolve_bwd(const double* L, int ld, int n, double* v, int lane) {
    const int NT = n / 16, i = lane & 15;
    for (int p = NT - 1; p >= 0; --p) {
        double at[16];  // column i of the diagonal tile
#pragma unroll
        for (int k = 0; k < 16; ++k) at[k] = ldT<LDS>(L + (size_t)(16 * p + k) * ld + 16 * p + i);
        double x = v[16 * p + i], dgl = 1.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) dgl = (i == k) ? at[k] : dgl;
        const double inv = 1.0 / dgl;
#pragma unroll
        for (int c = 15; c >= 0; --c) {
            const double xc = rl(x, c) * rl(inv, c);
            x = (i == c) ? xc : (i < c ? x - at[c] * xc : x);
        }
        if (lane < 16) v[16 * p + i] = x;
        for (int k0 = 0; k0 < 16 * p; k0 += 64) {
            const int k = k0 + lane;
            const bool act = k < 16 * p;
            const double* cp = L + (size_t)(16 * p) * ld + (act ? k : 0);
            double sv = 0;
#pragma unroll
            for (int c = 0; c < 16; ++c) sv += ldT<LDS>(cp + (size_t)c * ld) * rl(x, c);
            if (act) v[k] -= sv;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// solve T du = rhs in place (rhs in global, nk per knot).  lds: 2*ld vector buffers + QP_THREADS partial sums.
__device__ void solve_tiled(const QpDims& d, const QpWs& w, double* rhs, double* lds, int lds_avail) {
    const int nk = d.nk, ld = d.ldb, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double* cur = lds;
    double* oth = lds + ld;
    double* part = lds + 2 * ld;
    // small blocks: the diagonal factor of the knot is staged in LDS (coalesced copy by all threads) so that the tile-by-
    // tile triangular solve of wave 0 is a chain of LDS round trips, not L2 ones
    const int ldl = ld + 2;
    double* Lst = part + QP_THREADS;
    const bool staged = 2 * ld + QP_THREADS + ld * ldl <= lds_avail;
    for (int j = 0; j < d.nj; ++j) {  // forward: v_j <- L_jj^{-1} (v_j - L_{j,j-1} v_{j-1})
        for (int r = tid; r < ld; r += QP_THREADS) cur[r] = r < nk ? rhs[(size_t)j * nk + r] : 0.0;
        __syncthreads();
        if (j > 0) {
            const double* Lo = w.To + (size_t)(j - 1) * ld * ld;
            const int i = tid & 15;
            for (int r0 = 0; r0 < nk; r0 += QP_THREADS / 16) {  // 16 lanes per row
                const int r = r0 + (tid >> 4);
                double sv = 0;
                if (r < nk)
                    for (int c = i; c < ld; c += 16) sv += Lo[(size_t)r * ld + c] * oth[c];
                sv += __shfl_xor(sv, 8), sv += __shfl_xor(sv, 4), sv += __shfl_xor(sv, 2), sv += __shfl_xor(sv, 1);
                if (r < nk && i == 0) cur[r] -= sv;
            }
            __syncthreads();
        }
        if (staged) {
            stage_block(Lst, ldl, w.Td + (size_t)j * ld * ld, ld);
            __syncthreads();
        }
        if (wave == 0) {
            if (staged)
                trisolve_fwd<true>(Lst, ldl, ld, cur, lane);
            else
                trisolve_fwd<false>(w.Td + (size_t)j * ld * ld, ld, ld, cur, lane);
        }
        __syncthreads();
        for (int r = tid; r < nk; r += QP_THREADS) rhs[(size_t)j * nk + r] = cur[r];
        double* t = cur;
        cur = oth, oth = t;
    }
    __threadfence_block();
    for (int j = d.nj - 1; j >= 0; --j) {  // backward: v_j <- L_jj^{-T} (v_j - L_{j+1,j}' v_{j+1})
        __syncthreads();
        for (int r = tid; r < ld; r += QP_THREADS) cur[r] = r < nk ? rhs[(size_t)j * nk + r] : 0.0;
        __syncthreads();
        if (j + 1 < d.nj) {
            const double* Lo = w.To + (size_t)j * ld * ld;
            if (ld <= QP_THREADS) {
                const int ng = QP_THREADS / ld, c = tid % ld, g = tid / ld;
                if (g < ng) {
                    double sv = 0;
                    for (int r = g; r < ld; r += ng) sv += Lo[(size_t)r * ld + c] * oth[r];
                    part[tid] = sv;
                }
                __syncthreads();
                if (tid < nk) {
                    double sv = 0;
                    for (int q = 0; q < ng; ++q) sv += part[q * ld + tid];
                    cur[tid] -= sv;
                }
            } else {
                for (int c = tid; c < nk; c += QP_THREADS) {
                    double sv = 0;
                    for (int r = 0; r < ld; ++r) sv += Lo[(size_t)r * ld + c] * oth[r];
                    cur[c] -= sv;
                }
            }
            __syncthreads();
        }
        if (staged) {
            stage_block(Lst, ldl, w.Td + (size_t)j * ld * ld, ld);
            __syncthreads();
        }
        if (wave == 0) {
            if (staged)
                trisolve_bwd<true>(Lst, ldl, ld, cur, lane);
            else
                trisolve_bwd<false>(w.Td + (size_t)j * ld * ld, ld, ld, cur, lane);
        }
        __syncthreads();
        for (int r = tid; r < nk; r += QP_THREADS) rhs[(size_t)j * nk + r] = cur[r];
        double* t = cur;
        cur = oth, oth = t;
    }
    __threadfence_block();
    __syncthreads();
}

// identity padding of the diagonal blocks (once per launch: the factorisation maps it onto itself)
__device__ void init_block_pads(const QpDims& d, const QpWs& w) {
    const int nk = d.nk, ld = d.ldb;
    if (ld == nk) return;
    const int npad = ld - nk;
    for (int it = threadIdx.x; it < d.nj * npad * ld; it += QP_THREADS) {
        const int j = it / (npad * ld), q = it % (npad * ld), r = nk + q / ld, c = q % ld;
        double* A = w.Td + (size_t)j * ld * ld;
        A[(size_t)r * ld + c] = r == c ? 1.0 : 0.0;
        A[(size_t)c * ld + r] = r == c ? 1.0 : 0.0;
    }
}
