// jqp_tile.inc -- the BLOCKED SYMMETRIC SWEEP of the joint solver (see the head of jqp.hip): 64 x 64 tiles on v_mfma_f64_16x16x4_f64.
// Included once by jqp.hip, inside its anonymous namespace, behind Chain / chain_step.  Three schedules share ONE copy of every tile operation:
//
//   look-ahead          jq_pivot0(0), then per step [jq_panel] jq_update          (the workgroup of tile (k+1, k+1) inverts the next pivot)
//   bulk                per step jq_pivot0(k) jq_panel jq_update_bulk             (no LDS in the update, three workgroups per CU)
//   bulk, double step   per pass jq_pivot2 jq_panel2 jq_update2_bulk              (two pivot tiles per pass over the matrix)
//
//   sweep_open          what every sweep kernel starts with: the mission's workspace and SweepCtx (order and buffers of this step)
//   inv64_lds           the pivot tile's inverse in LDS; pivot_thresholds: the polish's deletion thresholds for it
//   panel_rows<LD>      Y_T = B_Tk P for one block row: to memory (jq_panel) or to LDS (jq_update with JArgs::fuse_panel) -- the same bits
//   tri_tile, sym_tile  which tile a workgroup takes, where block B_T,kc of the symmetric matrix is stored
//   quad_load / quad_mac / quad_store   a wave's 32 x 32 quadrant of B_IJ - Y_I B_Jk' (the double step calls quad_mac twice)
//   edge_copy           pivot row and column of the bulk updates (jq_update stages its copy in LDS)

// ping-pong buffers of the sweep: X[0] = the knot's slot in `inv`, X[1] = the chain's scratch; pass t reads X[(t + p0) & 1] and writes
// the other; p0 = (number of passes) & 1 makes the last pass land in X[0]
__device__ __forceinline__ int sweep_parity0(const JArgs& A, int nblk) { return (A.sweep2 ? (nblk + 1) / 2 : nblk) & 1; }
__device__ __forceinline__ double* sweep_buf(const Ws& w, const JDims& d, const JLayout& L, int chain, int jj, int which) {
    return which == 0 ? w.inv + (size_t)jj * L.nkpS * L.nkpS : w.scr + (size_t)chain * L.nkpS * L.nkpS;
}

// what a sweep kernel works on: kind 0 = the Schur complement of a knot (step s of a chain / the middle knot), kind 1 = the polish's
// S_AA (jqp_polish.inc; order and buffers from the mission's polish record)
struct SweepCtx {
    bool active;
    int nblk;
    const double* src;  // X[(k + p0) & 1]
    double* dst;        // X[(k + p0 + 1) & 1]
    double* Pk;         // pivot inverse of step k
    double* Pn;         // ... of step k + 1 (look-ahead)
    double* P2;         // double step (k, k + 1): the three tiles P00, P10, P11 of the pivot block's inverse
    double* Y;          // panel (double step: two tiles per block row)
    double* bad;        // counter of non-positive pivots
    const double* G;    // polish (kind 1): the matrix before the sweep (tile-major): its diagonal scales the deletion threshold; else nullptr
};
__device__ __forceinline__ SweepCtx sweep_ctx(const JArgs& A, const Ws& w, const JDims& d, int kind, int s, int mid, int k, int chain) {
    SweepCtx c;
    c.bad = w.st + ST_BADPIV;
    c.G = nullptr;
    if (kind == 0) {
        const Chain ch = chain_step(d, chain, s, mid != 0);
        c.active = ch.active && w.st[ST_STATE] == 0.0 && w.st[ST_RETRY] == 0.0 && w.st[ST_GO] == 0.0;
        c.nblk = d.nblk;
        // pass t of np: a double step takes the pivots (2 t, 2 t + 1), an odd order ends with a single step
        const int t = A.sweep2 ? (k >> 1) : k, p0 = sweep_parity0(A, d.nblk);
        c.src = sweep_buf(w, d, A.L, chain, ch.jj, (t + p0) & 1);
        c.dst = sweep_buf(w, d, A.L, chain, ch.jj, (t + p0 + 1) & 1);
        c.Pk = w.P + ((size_t)chain * 2 + (k & 1)) * JTT, c.Pn = w.P + ((size_t)chain * 2 + ((k + 1) & 1)) * JTT;
        c.P2 = w.P + (size_t)(4 + 3 * chain) * JTT;
        c.Y = w.Y + (size_t)chain * 2 * A.L.nblkS * JTT;
    } else {
        const Pol p = pol_carve(A, blockIdx.z);
        c.nblk = p.cnt[PC_NBLK];
        c.active = chain == 0 && w.st[ST_STATE] == 0.0 && w.st[ST_GO] != 0.0 && w.st[ST_PSTATE] == (double)PS_SOLVE && !p.cnt[PC_BPPDONE] && k < c.nblk;
        const int p0 = c.nblk & 1;
        c.src = ((k + p0) & 1) ? p.W1 : p.W0;
        c.dst = ((k + p0 + 1) & 1) ? p.W1 : p.W0;
        c.Pk = p.P + (size_t)(k & 1) * JTT, c.Pn = p.P + (size_t)((k + 1) & 1) * JTT;
        c.Y = p.Y;
        c.P2 = nullptr;
        c.G = p.G;
    }
    return c;
}
// what every sweep kernel starts with (grid.z = mission; `chain` is blockIdx.y + A.chain0 except in jq_update, which interleaves the chains)
struct SweepOpen {
    Ws w;
    SweepCtx c;  // (carries the order in tiles, c.nblk: no sweep kernel needs more of the mission's JDims)
};
__device__ __forceinline__ SweepOpen sweep_open(const JArgs& A, int kind, int s, int mid, int k, int chain) {
    SweepOpen o;
    o.w = carve(A, blockIdx.z);
    o.c = sweep_ctx(A, o.w, jdims(A.S.N, A.S.Mk[blockIdx.z]), kind, s, mid, k, chain);
    return o;
}

// ---- 64 x 64 SPD inverse in LDS (256 threads): the same blocked sweep one level down, 16 x 16 sub-tiles on the MFMA, the diagonal
// sub-tile by Gauss-Jordan with the rows in lanes (v_readlane broadcasts).  In: Am = the SPD tile, leading dimension LDA.
// Out: Am = -(tile)^-1.  *bad is set when a pivot is not positive.
constexpr int LDA = 66;  // (ds_read_b64 of lane (i, g) at row i, column 4 kk + g: conflict free with 66)
constexpr size_t JQ_UPDATE_LDS_EXTRA = 64 * sizeof(double) + 16;  // thr[JT] + the bad-pivot flag behind Am and the scratch
struct InvScratch {
    double Pi[4][16 * 18];  // per wave: its copy of the diagonal sub-tile, inverted in place
    double Yb[4][16 * 18];
    // (Z of wave w lives in Pi[w]: a wave is done with its copy of the pivot sub-tile when it stores Z, only wave kk's copy is needed
    // afterwards and wave kk stores no Z -- 9 KB less, which lets a third workgroup of jq_update onto a CU)
};
#define JQ_WSYNC()                                             \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
    } while (0)
// 16 x 16 Gauss-Jordan inverse in LDS by ONE wave, in place (leading dimension 18): lane (r = l & 15, g = l >> 4) owns the entries
// D[r][4g .. 4g+3] in registers and publishes them after every column step; what a step needs from other lanes -- the pivot, the
// pivot row's segment, the row's entry in the pivot column -- are same-address LDS reads (broadcasts: ~7 cycles per 8 bytes, no
// v_readlane chains).  LDS serves a wave's operations in order, so a step's reads see the previous step's writes.
// thr (or nullptr): per column, the pivot size at or below which the row is DELETED from the solve instead of eliminated: row and column
// become zero, i.e. the result is the inverse of the matrix without that row, with a zero row and column in its place.  The polish uses it
// for active rows that are linear combinations of the rows before them (five control points around a knot are functions of three
// variables: a trajectory that runs along a box face makes four or five bound rows of one agent and axis active at once); everything
// downstream of a zero column of the pivot inverse -- panel, update, the other sub-tiles -- stays zero by the sweep's own algebra.
__device__ __forceinline__ bool gj16_lds(double* D, int lane, const double* thr = nullptr) {
    const int r = lane & 15, g = lane >> 4;
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = D[r * 18 + 4 * g + q];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const double p = D[c * 18 + c], f = D[r * 18 + c];
        double pr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pr[q] = D[c * 18 + 4 * g + q];
        if (thr && p <= thr[c]) {  // (wave-uniform)
            if (r == c) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = 0.0;
            }
            if (g == c / 4) v[c % 4] = 0.0;
        } else {
            ok = ok && (p > 0.0);
            const double ip = fast_rcp(p), fi = f * ip;
            if (r == c) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = pr[q] * ip;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] -= fi * pr[q];
            }
            if (g == c / 4) v[c % 4] = r == c ? ip : -fi;
        }
        JQ_WSYNC();
#pragma unroll
        for (int q = 0; q < 4; ++q) D[r * 18 + 4 * g + q] = v[q];
        JQ_WSYNC();
    }
    return ok;
}
__device__ __forceinline__ void inv64_lds_inl(double* Am, InvScratch* sc, int* bad, const double* thr = nullptr) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    for (int kk = 0; kk < 4; ++kk) {
        // every wave inverts its own copy of the diagonal sub-tile (no barrier between the inversion and the wave's panel product)
        double* Pi = sc->Pi[wave];
#pragma unroll
        for (int q = 0; q < 4; ++q) Pi[li * 18 + 4 * lg + q] = Am[(16 * kk + li) * LDA + 16 * kk + 4 * lg + q];
        JQ_WSYNC();
        const bool okp = gj16_lds(Pi, lane, thr ? thr + 16 * kk : nullptr);
        if (!okp && tid == 0) *bad = 1;
        // panel: row block i = wave: Z = A[i][kk] (old), Y = Z Pi'
        if (wave != kk) {
            d4 acc = d4{0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double av = Am[(16 * wave + li) * LDA + 16 * kk + 4 * q + lg];
                const double bv = Pi[li * 18 + 4 * q + lg];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc->Yb[wave][(lg + 4 * r) * 18 + li] = acc[r];
                sc->Pi[wave][(lg + 4 * r) * 18 + li] = Am[(16 * wave + lg + 4 * r) * LDA + 16 * kk + li];
            }
        }
        __syncthreads();
        // update: row block i = wave, all four column blocks
        for (int jb = 0; jb < 4; ++jb) {
            double* At = Am + (16 * wave) * LDA + 16 * jb;
            if (wave == kk && jb == kk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) At[(lg + 4 * r) * LDA + li] = -Pi[(lg + 4 * r) * 18 + li];
            } else if (jb == kk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) At[(lg + 4 * r) * LDA + li] = sc->Yb[wave][(lg + 4 * r) * 18 + li];
            } else if (wave == kk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) At[(lg + 4 * r) * LDA + li] = sc->Yb[jb][li * 18 + lg + 4 * r];
            } else {
                d4 acc = d4{0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double av = sc->Yb[wave][li * 18 + 4 * q + lg];
                    const double bv = sc->Pi[jb][li * 18 + 4 * q + lg];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) At[(lg + 4 * r) * LDA + li] -= acc[r];
            }
        }
        __syncthreads();
    }
}

// (out of line for the pivot kernels, which have a CU to themselves; jq_update inlines it so that ITS register budget applies)
__device__ void inv64_lds(double* Am, InvScratch* sc, int* bad, const double* thr = nullptr) { inv64_lds_inl(Am, sc, bad, thr); }

// Pbuf[chain][parity] <- symmetrised inverse of the SPD tile held (as its NEGATED inverse after inv64_lds) in Am
__device__ __forceinline__ void store_pivot_inverse(const double* Am, double* Pg) {
    for (int i = threadIdx.x; i < JTT; i += 256) {
        const int r = i >> 6, c = i & 63;
        Pg[i] = -0.5 * (Am[r * LDA + c] + Am[c * LDA + r]);
    }
}

// deletion thresholds of pivot tile (k, k) for inv64_lds -- the polish only (c.G: pol_tau x the diagonal of the matrix before the sweep), nullptr
// for a knot.  Written by the first JT threads: the caller's barrier publishes them.
__device__ __forceinline__ const double* pivot_thresholds(const JArgs& A, const Ws& w, const SweepCtx& c, int k, double* thr) {
    if (!c.G) return nullptr;
    if (threadIdx.x < JT) thr[threadIdx.x] = A.pol_tau * w.st[ST_PTAU] * c.G[((size_t)k * c.nblk + k) * JTT + (size_t)threadIdx.x * (JT + 1)];
    return thr;
}

// pivot tile of step k.  k = 0: first pivot of a knot; k > 0: only in the bulk schedule (many workgroups per launch), where the update
// kernel has no look-ahead (jq_update_bulk)
__global__ __launch_bounds__(256) void jq_pivot0(JArgs A, int kind, int s, int mid, int k) {
    const SweepOpen o = sweep_open(A, kind, s, mid, k, blockIdx.y + A.chain0);
    const SweepCtx& c = o.c;
    if (!c.active || k >= c.nblk) return;
    __shared__ double Am[JT * LDA];
    __shared__ InvScratch sc;
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    const double* tkk = c.src + ((size_t)k * c.nblk + k) * JTT;  // pivot tile (k, k) as the steps before k left it
    for (int i = threadIdx.x; i < JTT; i += 256) Am[(i >> 6) * LDA + (i & 63)] = tkk[i];
    __shared__ double thr[JT];
    const double* th = pivot_thresholds(A, o.w, c, k, thr);
    __syncthreads();
    inv64_lds(Am, &sc, &bad, th);
    store_pivot_inverse(Am, c.Pk);
    // a non-positive pivot (the matrix is SPD in exact arithmetic) is counted, not fatal: the sweep needs no square roots, and with
    // Newton weights of 1e9 the last interior-point iterations work at the edge of double precision
    if (bad && threadIdx.x == 0) *c.bad = 1.0;  // (a flag: the two chains' workgroups may both set it, never a read-modify-write)
}

// operand fragments of a 16-row block for v_mfma_f64_16x16x4_f64 over K = 64: lane (i, g) holds rows[i][16 ch + 4 g + q], ch, q = 0..3
// (the four MFMA steps of a 16-chunk use k = 4 g + q on both operands: a permutation of the summation index, see tile_nt in qp_tiled.inc).
// TR: the operand is the TRANSPOSE of the stored tile (rows of the operand are columns of the tile).
__device__ __forceinline__ void load_frag(const double* tile, int row0, bool tr, int li, int lg, d4 (&f)[4]) {
    if (!tr) {
        const double* p = tile + (size_t)(row0 + li) * JT + 4 * lg;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) f[ch] = *reinterpret_cast<const d4*>(p + 16 * ch);
    } else {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int q = 0; q < 4; ++q) f[ch][q] = tile[(size_t)(16 * ch + 4 * lg + q) * JT + row0 + li];
    }
}

// block B_T,kc of the symmetric matrix X, of which the sweep keeps the lower triangle: tile (T, kc) below the diagonal, tile (kc, T)' -- to be
// read TRANSPOSED -- for T < kc
__device__ __forceinline__ const double* sym_tile(const double* X, int nblk, int T, int kc) {
    return X + (T < kc ? (size_t)kc * nblk + T : (size_t)T * nblk + kc) * JTT;
}

// panel rows of step k: Y_T = B_Tk P for block row T != k, leading dimension LD: JT = a tile in memory (jq_panel), LDA = Am of jq_update.
// When JArgs::fuse_panel is set every workgroup of jq_update forms the panel rows it needs itself and the panel launch -- a dependent
// kernel boundary per 64 columns -- disappears from the look-ahead schedule (one extra 64^3 product per tile, P and B_Tk come from the L2).
// Decided per launch (JArgs::fuse_panel): it pays while a launch is a round or so of workgroups (64 agents 0.267 -> 0.245 s; one chain of a
// 256-agent mission, 666 tiles, 3.84 -> 3.75 s) and costs 5 % when both chains of that mission share the launches (1332 tiles).
template <int LD>
__device__ __forceinline__ void panel_rows(const double* X, const double* P, int nblk, int k, int T, double* Y, int wave, int li, int lg) {
    d4 zf[4];
    load_frag(sym_tile(X, nblk, T, k), 16 * wave, T < k, li, lg, zf);  // rows 16 wave .. of B_Tk
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        d4 pf[4];
        load_frag(P, 16 * tj, false, li, lg, pf);  // P symmetric: Z P = Z P'
        d4 acc = d4{0, 0, 0, 0};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(zf[ch][q], pf[ch][q], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Y[(16 * wave + lg + 4 * r) * LD + 16 * tj + li] = acc[r];
    }
}

// panel of step k: Y_J = B_Jk P for every J != k
__global__ __launch_bounds__(256) void jq_panel(JArgs A, int kind, int s, int mid, int k) {
    const int J = blockIdx.x;
    const SweepOpen o = sweep_open(A, kind, s, mid, k, blockIdx.y + A.chain0);
    const SweepCtx& c = o.c;
    if (!c.active || J >= c.nblk || J == k) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    panel_rows<JT>(c.src, c.Pk, c.nblk, k, J, c.Y + (size_t)J * JTT, wave, lane & 15, lane >> 4);
}

// tile b = I (I + 1) / 2 + J of the lower triangle, I >= J
__device__ __forceinline__ void tri_tile(int b, int& I, int& J) {
    I = (int)((sqrtf(8.0f * b + 1.0f) - 1.0f) * 0.5f);
    if (I * (I + 1) / 2 > b) I--;
    if ((I + 1) * (I + 2) / 2 <= b) I++;
    J = b - I * (I + 1) / 2;
}

// ---- rank-64 update of a tile, C - Y Z', by four waves: wave (wr, wc) owns a 32 x 32 quadrant as 2 x 2 MFMA blocks of 16 x 16, lane
// (li, lg) holds rows lg + 4 r, column li of each block
struct Quad {  // (handed on BY VALUE: by reference the three update kernels came out 15 to 40 registers wider, jq_update2_bulk past its fourth wave per SIMD)
    int wr, wc, li, lg;
};
__device__ __forceinline__ Quad quad_of(int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    return Quad{wave >> 1, wave & 1, lane & 15, lane >> 4};
}
__device__ __forceinline__ void quad_load(const double* Ct, const Quad q, double (&cv)[2][2][4]) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) cv[ti][tj][r] = Ct[(size_t)(32 * q.wr + 16 * ti + q.lg + 4 * r) * JT + 32 * q.wc + 16 * tj + q.li];
}
// acc += Y Z' over K = 64.  Y: a tile in memory, or (ylds) Ylds: the panel rows in LDS with leading dimension LDA; trZ: Z is the transpose of the
// stored tile Zt.  Operands of ONE 16-column chunk at a time: the register budget of three workgroups per CU.  (ylds is tested per operand
// load on purpose: with two instances of the MFMA block jq_update came out 168 registers wide, the ceiling of its launch bounds, with scratch.)
__device__ __forceinline__ void quad_mac(const double* Y, const double* Ylds, bool ylds, const double* Zt, bool trZ, const Quad q, d4 (&acc)[2][2]) {
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        d4 yf[2], zf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (ylds) {
#pragma unroll
                for (int e = 0; e < 4; ++e) yf[t][e] = Ylds[(32 * q.wr + 16 * t + q.li) * LDA + 16 * ch + 4 * q.lg + e];
            } else {
                yf[t] = *reinterpret_cast<const d4*>(Y + (size_t)(32 * q.wr + 16 * t + q.li) * JT + 16 * ch + 4 * q.lg);
            }
            if (!trZ) {
                zf[t] = *reinterpret_cast<const d4*>(Zt + (size_t)(32 * q.wc + 16 * t + q.li) * JT + 16 * ch + 4 * q.lg);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) zf[t][e] = Zt[(size_t)(16 * ch + 4 * q.lg + e) * JT + 32 * q.wc + 16 * t + q.li];
            }
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[ti][e], zf[tj][e], acc[ti][tj], 0, 0, 0);
    }
}
// out <- sgn (C - acc), leading dimension LD (JT: a tile in memory, LDA: Am); mirror: outT <- the transpose as well
template <int LD>
__device__ __forceinline__ void quad_store(const double (&cv)[2][2][4], const d4 (&acc)[2][2], double sgn, const Quad q, double* out, double* outT,
                                           bool mirror) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = sgn * (cv[ti][tj][r] - acc[ti][tj][r]);
                const int rr = 32 * q.wr + 16 * ti + q.lg + 4 * r, cc = 32 * q.wc + 16 * tj + q.li;
                out[(size_t)rr * LD + cc] = v;
                if (mirror) outT[(size_t)cc * LD + rr] = v;
            }
}
// pivot row and column of a bulk update: out <- f src (tr: f src'), mirror: outT <- the transpose as well
__device__ __forceinline__ void edge_copy(const double* src, bool tr, double f, double* out, double* outT, bool mirror) {
    for (int i = threadIdx.x; i < JTT; i += 256) {
        const int r = i >> 6, cc = i & 63;
        const double v = f * (tr ? src[(size_t)cc * JT + r] : src[i]);
        out[i] = v;
        if (mirror) outT[(size_t)cc * JT + r] = v;
    }
}

// update of step k: every tile (I, J), I >= J, of the lower triangle
//   (k, k) <- -P        (I, k) <- Y_I        (k, J) <- Y_J'        else  B_IJ - Y_I B_Jk'
// The last step writes -(...) = the inverse itself, with both triangles.  Look-ahead: the workgroup of tile (k+1, k+1) inverts it.
__global__ __launch_bounds__(256, 3) void jq_update(JArgs A, int kind, int s, int mid, int k) {
    // Which tile this workgroup takes.  Workgroups start in the order x, then y: the chains of a launch are interleaved (so that both
    // chains' first tiles start in the first round), and the tile that carries the look-ahead inversion -- 20 us of dependent work
    // on top of its update, the longest job of the launch -- is taken by the FIRST workgroup of its chain instead of one in the middle of
    // the triangle (with hundreds of tiles per chain, a 256-agent mission, it used to start in the second or third round and the
    // launch ended with that inversion alone on the chip).  The arithmetic of a tile does not depend on who computes it.
    const int lin = (int)(blockIdx.y * gridDim.x + blockIdx.x), nchl = (int)gridDim.y;
    int b = lin / nchl;
    const SweepOpen o = sweep_open(A, kind, s, mid, k, lin % nchl + A.chain0);
    const SweepCtx& c = o.c;
    const int nblk = c.nblk;
    if (!c.active || b >= nblk * (nblk + 1) / 2) return;
    if (k + 1 < nblk) {
        const int lookb = (k + 1) * (k + 2) / 2 + (k + 1);
        b = b == 0 ? lookb : (b == lookb ? 0 : b);
    }
    int I, J;
    tri_tile(b, I, J);
    const double* X = c.src;
    const double* P = c.Pk;
    const bool last = k == nblk - 1, look = !last && I == k + 1 && J == k + 1, fuse = A.fuse_panel != 0;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    // LDS is DYNAMIC here (JQ_UPDATE_LDS bytes per launch): with a static size the compiler derives the occupancy from a 64 KB LDS and then
    // spends 248 registers; the CU has 160 KB, three workgroups of 52.7 KB fit, and the register budget has to follow (launch bounds)
    extern __shared__ double jq_update_lds[];
    double* Am = jq_update_lds;                                        // [JT * LDA]
    InvScratch& sc = *reinterpret_cast<InvScratch*>(Am + JT * LDA);
    double* thr = reinterpret_cast<double*>(&sc + 1);                  // [JT]
    int& bad = *reinterpret_cast<int*>(thr + JT);
    double* out = c.dst + ((size_t)I * nblk + J) * JTT;
    double* outT = c.dst + ((size_t)J * nblk + I) * JTT;
    const double sgn = last ? -1.0 : 1.0;
    if (I == k || J == k) {  // copies (through LDS for the transposed ones)
        const double* src = (I == k && J == k) ? P : (J == k ? c.Y + (size_t)I * JTT : c.Y + (size_t)J * JTT);
        const bool tr = (I == k && J != k);
        const double f = (I == k && J == k) ? -sgn : sgn;
        if (fuse && !(I == k && J == k))
            panel_rows<LDA>(X, P, nblk, k, J == k ? I : J, Am, wave, li, lg);
        else
            for (int i = tid; i < JTT; i += 256) Am[(i >> 6) * LDA + (i & 63)] = src[i];
        __syncthreads();
        for (int i = tid; i < JTT; i += 256) {
            const int r = i >> 6, cc = i & 63;
            const double v = f * (tr ? Am[cc * LDA + r] : Am[r * LDA + cc]);
            out[i] = v;
            if (last && I != J) outT[(size_t)cc * JT + r] = v;
        }
        return;
    }
    const Quad q = quad_of(tid);
    double cv[2][2][4];
    quad_load(X + ((size_t)I * nblk + J) * JTT, q, cv);
    if (fuse) {
        panel_rows<LDA>(X, P, nblk, k, I, Am, wave, li, lg);
        __syncthreads();
    }
    d4 acc[2][2] = {};
    quad_mac(c.Y + (size_t)I * JTT, Am, fuse, sym_tile(X, nblk, J, k), J < k, q, acc);
    if (!(last && I != J) && !look) {
        quad_store<JT>(cv, acc, sgn, q, out, nullptr, false);
        return;
    }
    // through LDS: mirrored store of the last step / look-ahead inversion of the next pivot
    if (fuse) __syncthreads();  // (Y_I is still being read from Am by the other waves)
    quad_store<LDA>(cv, acc, sgn, q, Am, nullptr, false);
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int i = tid; i < JTT; i += 256) {
        const int r = i >> 6, cc = i & 63;
        out[i] = Am[r * LDA + cc];
        if (last) outT[i] = Am[cc * LDA + r];
    }
    if (look) {
        const double* th = pivot_thresholds(A, o.w, c, k + 1, thr);
        __syncthreads();
        inv64_lds_inl(Am, &sc, &bad, th);
        store_pivot_inverse(Am, c.Pn);
        if (bad && tid == 0) *c.bad = 1.0;
    }
}

// The same update for launches with thousands of tiles (many resident missions, or one 256-agent mission): no look-ahead -- the next pivot
// is inverted by jq_pivot0(k + 1) in a launch of its own --, hence no LDS (the look-ahead scratch costs every workgroup of jq_update 61 KB)
// and a register budget for three workgroups per CU.
__global__ __launch_bounds__(256, 3) void jq_update_bulk(JArgs A, int kind, int s, int mid, int k) {
    const int b = blockIdx.x;
    const SweepOpen o = sweep_open(A, kind, s, mid, k, blockIdx.y + A.chain0);
    const SweepCtx& c = o.c;
    const int nblk = c.nblk;
    if (!c.active || b >= nblk * (nblk + 1) / 2) return;
    int I, J;
    tri_tile(b, I, J);
    const bool last = k == nblk - 1, mirror = last && I != J;
    double* out = c.dst + ((size_t)I * nblk + J) * JTT;
    double* outT = c.dst + ((size_t)J * nblk + I) * JTT;
    const double sgn = last ? -1.0 : 1.0;
    if (I == k || J == k) {
        const double* src = (I == k && J == k) ? c.Pk : (J == k ? c.Y + (size_t)I * JTT : c.Y + (size_t)J * JTT);
        edge_copy(src, I == k && J != k, (I == k && J == k) ? -sgn : sgn, out, outT, mirror);
        return;
    }
    const Quad q = quad_of(threadIdx.x);
    double cv[2][2][4];
    quad_load(c.src + ((size_t)I * nblk + J) * JTT, q, cv);
    d4 acc[2][2] = {};
    quad_mac(c.Y + (size_t)I * JTT, nullptr, false, sym_tile(c.src, nblk, J, k), J < k, q, acc);
    quad_store<JT>(cv, acc, sgn, q, out, outT, mirror);
}

// ------------------------------------------------------------------------------------------------------------------------
// Double steps of the bulk schedule: the pivots (k, k + 1) in ONE pass over the matrix.  jq_update_bulk is bound by HBM, not by the MFMA
// (profiles/r05_joint_pmc.txt: 1.6 GB of reads and writes per 286 us launch = 5.6 TB/s at 200 resident missions): every pass reads and
// writes the knot's whole lower triangle for a rank-64 update.  Sweeping on the 128 x 128 pivot block [B_kk B_k+1,k'; B_k+1,k B_k+1,k+1]
// is the same two sweep steps composed -- P2 = block^-1, Y2_J = [B_Jk B_J,k+1] P2, (I, J) <- B_IJ - Y2_I [B_Jk B_J,k+1]' -- with half the
// passes over the matrix per unit of arithmetic.
// ------------------------------------------------------------------------------------------------------------------------
// P2 by block elimination in one workgroup: Pa = B_kk^-1, W = B_k+1,k Pa, Ps = (B_k+1,k+1 - W B_k+1,k')^-1,
// P11 = Ps, P10 = -Ps W, P00 = Pa + W' Ps W.  The four 64^3 products run on plain FMAs out of LDS (a few microseconds per knot and pass).
__global__ __launch_bounds__(256) void jq_pivot2(JArgs A, int s, int mid, int k) {
    const int tid = threadIdx.x;
    const SweepOpen o = sweep_open(A, 0, s, mid, k, blockIdx.y + A.chain0);
    const SweepCtx& c = o.c;
    if (!c.active || k + 1 >= c.nblk) return;
    extern __shared__ double lds2[];  // Am, Bm, Wm: 3 x JT x LDA doubles
    __shared__ InvScratch sc;
    __shared__ int bad;
    double *Am = lds2, *Bm = lds2 + JT * LDA, *Wm = lds2 + 2 * JT * LDA;
    const int nblk = c.nblk;
    const double* t00 = c.src + ((size_t)k * nblk + k) * JTT;
    const double* t10 = c.src + ((size_t)(k + 1) * nblk + k) * JTT;
    const double* t11 = c.src + ((size_t)(k + 1) * nblk + k + 1) * JTT;
    double *P00 = c.P2, *P10 = c.P2 + JTT, *P11 = c.P2 + 2 * JTT;
    // Am holds -(inverse) after inv64_lds: p <- the symmetrised inverse, 16 entries per thread, and back into Am (and to Pg)
    auto symmetrise = [&](double (&p)[16], double* Pg) {
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const int i = tid + 256 * n, r = i >> 6, cc = i & 63;
            p[n] = -0.5 * (Am[r * LDA + cc] + Am[cc * LDA + r]);
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const int i = tid + 256 * n;
            Am[(i >> 6) * LDA + (i & 63)] = p[n];
            if (Pg) Pg[i] = p[n];
        }
        __syncthreads();
    };
    if (tid == 0) bad = 0;
    for (int i = tid; i < JTT; i += 256) Am[(i >> 6) * LDA + (i & 63)] = t00[i], Bm[(i >> 6) * LDA + (i & 63)] = t10[i];
    __syncthreads();
    inv64_lds(Am, &sc, &bad);  // Am = -Pa
    double pa[16];
    symmetrise(pa, nullptr);
    const int r0 = 4 * (tid >> 4), c0 = 4 * (tid & 15);
    double acc[4][4];  // this thread's 4 x 4 block (r0.., c0..) of a 64^3 product
    auto each_acc = [&](auto&& put) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) put(r0 + x, c0 + y, acc[x][y]);
    };
    // MODE 0: X[r][m] Yv[m][c]   1: X[r][m] Yv[c][m]   2: X[m][r] Yv[m][c]
#define JQ_MM(MODE, X, Yv)                                                                            \
    do {                                                                                              \
        _Pragma("unroll") for (int x = 0; x < 4; ++x) _Pragma("unroll") for (int y = 0; y < 4; ++y) acc[x][y] = 0.0; \
        for (int m = 0; m < JT; ++m) {                                                                \
            double a[4], b[4];                                                                        \
            _Pragma("unroll") for (int x = 0; x < 4; ++x) a[x] = (MODE) == 2 ? (X)[m * LDA + r0 + x] : (X)[(r0 + x) * LDA + m]; \
            _Pragma("unroll") for (int y = 0; y < 4; ++y) b[y] = (MODE) == 1 ? (Yv)[(c0 + y) * LDA + m] : (Yv)[m * LDA + c0 + y]; \
            _Pragma("unroll") for (int x = 0; x < 4; ++x) _Pragma("unroll") for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], b[y], acc[x][y]); \
        }                                                                                             \
    } while (0)
    JQ_MM(0, Bm, Am);  // W = B10 Pa
    each_acc([&](int r, int cc, double v) { Wm[r * LDA + cc] = v; });
    __syncthreads();
    JQ_MM(1, Wm, Bm);  // W B10'
    each_acc([&](int r, int cc, double v) { Am[r * LDA + cc] = t11[(size_t)r * JT + cc] - v; });
    __syncthreads();
    inv64_lds(Am, &sc, &bad);  // Am = -Ps
    double ps[16];
    symmetrise(ps, P11);
    JQ_MM(0, Am, Wm);  // V = Ps W
    each_acc([&](int r, int cc, double v) { Bm[r * LDA + cc] = v, P10[(size_t)r * JT + cc] = -v; });
    __syncthreads();
    JQ_MM(2, Wm, Bm);  // W' V
    each_acc([&](int r, int cc, double v) { Am[r * LDA + cc] = v; });
    __syncthreads();
#undef JQ_MM
#pragma unroll
    for (int n = 0; n < 16; ++n) {
        const int i = tid + 256 * n, r = i >> 6, cc = i & 63;
        P00[i] = pa[n] + 0.5 * (Am[r * LDA + cc] + Am[cc * LDA + r]);
    }
    if (bad && tid == 0) *c.bad = 1.0;
}

// panel of the double step: Y2_J = [B_Jk B_J,k+1] P2 for every block row J outside the pivot block (two tiles per J)
__global__ __launch_bounds__(256) void jq_panel2(JArgs A, int s, int mid, int k) {
    const int J = blockIdx.x;
    const SweepOpen o = sweep_open(A, 0, s, mid, k, blockIdx.y + A.chain0);
    const SweepCtx& c = o.c;
    const int nblk = c.nblk;
    if (!c.active || J >= nblk || J == k || J == k + 1 || k + 1 >= nblk) return;
    const bool tr = J < k;
    const double *Z0 = sym_tile(c.src, nblk, J, k), *Z1 = sym_tile(c.src, nblk, J, k + 1);
    const double *P00 = c.P2, *P10 = c.P2 + JTT, *P11 = c.P2 + 2 * JTT;
    double* Y0 = c.Y + (size_t)J * 2 * JTT;
    double* Y1 = Y0 + JTT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    d4 z0[4], z1[4];
    load_frag(Z0, 16 * wave, tr, li, lg, z0);
    load_frag(Z1, 16 * wave, tr, li, lg, z1);
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        d4 pf[4];
        d4 a0 = d4{0, 0, 0, 0}, a1 = d4{0, 0, 0, 0};
        load_frag(P00, 16 * tj, false, li, lg, pf);  // Z0 P00 (symmetric)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int q = 0; q < 4; ++q) a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(z0[ch][q], pf[ch][q], a0, 0, 0, 0);
        load_frag(P10, 16 * tj, true, li, lg, pf);  // Z1 P10: the operand's rows are P10's columns
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int q = 0; q < 4; ++q) a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(z1[ch][q], pf[ch][q], a0, 0, 0, 0);
        load_frag(P10, 16 * tj, false, li, lg, pf);  // Z0 P01 = Z0 P10'
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int q = 0; q < 4; ++q) a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(z0[ch][q], pf[ch][q], a1, 0, 0, 0);
        load_frag(P11, 16 * tj, false, li, lg, pf);  // Z1 P11 (symmetric)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int q = 0; q < 4; ++q) a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(z1[ch][q], pf[ch][q], a1, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Y0[(size_t)(16 * wave + lg + 4 * r) * JT + 16 * tj + li] = a0[r];
            Y1[(size_t)(16 * wave + lg + 4 * r) * JT + 16 * tj + li] = a1[r];
        }
    }
}

// update of the double step: every tile (I, J), I >= J, of the lower triangle
//   pivot block <- -P2      (I, k + h) <- Y2_I[h]      (k + h, J) <- Y2_J[h]'      else  B_IJ - Y2_I[0] B_Jk' - Y2_I[1] B_J,k+1'
// (the last pass writes -(...) = the inverse itself, with both triangles)
__global__ __launch_bounds__(256, 3) void jq_update2_bulk(JArgs A, int s, int mid, int k) {
    const int b = blockIdx.x;
    const SweepOpen o = sweep_open(A, 0, s, mid, k, blockIdx.y + A.chain0);
    const SweepCtx& c = o.c;
    const int nblk = c.nblk;
    if (!c.active || k + 1 >= nblk || b >= nblk * (nblk + 1) / 2) return;
    int I, J;
    tri_tile(b, I, J);
    const bool last = k + 1 == nblk - 1, mirror = last && I != J;
    double* out = c.dst + ((size_t)I * nblk + J) * JTT;
    double* outT = c.dst + ((size_t)J * nblk + I) * JTT;
    const double sgn = last ? -1.0 : 1.0;
    const bool Ik = I == k || I == k + 1, Jk = J == k || J == k + 1;
    if (Ik || Jk) {
        const double* src;
        bool tr = false;
        double f = sgn;
        if (Ik && Jk)
            src = c.P2 + (size_t)(I == k ? 0 : (J == k ? 1 : 2)) * JTT, f = -sgn;
        else if (Jk)
            src = c.Y + ((size_t)I * 2 + (J - k)) * JTT;
        else
            src = c.Y + ((size_t)J * 2 + (I - k)) * JTT, tr = true;
        edge_copy(src, tr, f, out, outT, mirror);
        return;
    }
    const Quad q = quad_of(threadIdx.x);
    double cv[2][2][4];
    quad_load(c.src + ((size_t)I * nblk + J) * JTT, q, cv);
    d4 acc[2][2] = {};
    quad_mac(c.Y + (size_t)I * 2 * JTT, nullptr, false, sym_tile(c.src, nblk, J, k), J < k, q, acc);
    quad_mac(c.Y + ((size_t)I * 2 + 1) * JTT, nullptr, false, sym_tile(c.src, nblk, J, k + 1), J < k, q, acc);
    quad_store<JT>(cv, acc, sgn, q, out, outT, mirror);
}
