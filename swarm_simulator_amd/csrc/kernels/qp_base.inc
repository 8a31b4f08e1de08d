// qp_base.inc — what every layer of the batch QP stands on: the phase timers (PROF*), the dimensions and the workspace of one batch QP
// (QpDims, QpWs, carve), the wave- and block-wide reductions, the helpers that move wave-uniform arguments into scalar registers
// (BlkArgs, uni, blk_unpack, uni_words) and the per-mission constants.  Included by qp.hip, first; needs SC_* (rbp_dev.h), Qbase of ipm::
// (the row header of common/, which only qp.hip itself includes) and qp.hip's levers and polish sizes (QP_THREADS, polish_ws_doubles).

#ifdef QP_PROFILE
#define PROF_DECL long long prof_t0 = wall_clock64(), prof_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PROF(i)                                \
    do {                                       \
        __syncthreads();                       \
        long long t_ = wall_clock64();         \
        prof_acc[i] += t_ - prof_t0;           \
        prof_t0 = t_;                          \
    } while (0)
#define PROF_FLUSH(scal)                                                         \
    do {                                                                         \
        if (threadIdx.x == 0)                                                    \
            for (int i_ = 0; i_ < 12; ++i_) scal[SC_PROF0 + i_] += (double)prof_acc[i_]; \
    } while (0)
#else
#define PROF_DECL
#define PROF(i)
#define PROF_FLUSH(scal)
#endif

// ------------------------------------------------------------------------------------------------------------
// dimensions of one batch QP
// ------------------------------------------------------------------------------------------------------------
struct QpDims {
    int N, M, oq;       // agents, segments, 6M
    int nb, NF, npb;    // batch agents, frozen agents, in-batch pairs
    int nk, nj, ld;     // block order 9*nb, knots M-1, padded leading dimension
    int ldb;            // leading dimension of the knot blocks in global memory: nk (wave path) or nk rounded up to 16 (tiled path)
    int first;          // first agent of the batch (batches are contiguous: qi / batch_size == l)
    int ncol0;          // rows every control point of a batch agent has: 6 bound rows + (nb - 1) in-batch pair rows
    int ntile;          // 64-lane tiles of control points: ceil(nb * oq / 64)
    size_t nslot_max;   // capacity of the row arrays: ntile * 64 * (ncol0 + NF)
};

__host__ __device__ inline QpDims make_dims(int N, int M, int first, int nb) {
    QpDims d;
    d.N = N, d.M = M, d.oq = 6 * M, d.nb = nb, d.NF = N - nb, d.npb = nb * (nb - 1) / 2;
    d.nk = 9 * nb, d.nj = M - 1, d.ld = d.nk + 1, d.first = first;
    d.ldb = d.nk <= 36 ? d.nk : ((d.nk + 15) & ~15);
    d.ncol0 = 6 + nb - 1, d.ntile = (nb * d.oq + 63) / 64;
    d.nslot_max = (size_t)d.ntile * 64 * (d.ncol0 + d.NF);
    return d;
}

// ROW STORAGE ("sliced ELLPACK", slice = one wavefront).  A sweep hands one control point (agent a, segment, i) of a batch agent
// to a thread; that thread owns ALL rows that touch its control point:
//     6 bound rows  |  nb - 1 in-batch pair rows  |  cnt(a, segment) frozen-neighbour rows that survived the presolve
// Control points are numbered wi = 6 * rank(a, segment) + i with the (a, segment) groups ranked by falling row count, 64
// consecutive wi form a tile (= the lanes of one wavefront), and row `idx` of control point wi lives in slot
//     tile_base[wi / 64] + idx * 64 + (wi % 64)
// so every load/store of a sweep is ONE coalesced 512-byte access per wavefront and array, and consecutive rows of a thread
// are consecutive 512-byte lines: a pure stream.  (The previous layout kept the rows of a group contiguous: a wavefront then
// touched eleven 48-byte pieces of different cache lines per array and step, and HBM-side traffic was ~2.5x the bytes used.)
// A pair row is shared by two control points (one of each agent) and is STORED TWICE, once in each one's column: both copies
// are updated by the same arithmetic on the same inputs, hence stay bit-identical; reductions count the copy of the lower
// agent only.  Only (s, z) are stored per row -- the corrector term and the step (ds, dz) are recomputed where they are needed
// (they are functions of s, z and the two direction vectors), which halves the bytes of a sweep; the step sweep writes the
// new (s, z) into a second pair of arrays (ping-pong) so that a rejected step can be repeated from the old state.
struct QpWs {
    double *s, *z, *s2, *z2;        // row state [nslot]: current / next
    double *rh;                     // [nslot] frozen-neighbour rows: the constant of slack = rh - n . x_a
    double *cc, *ds;                // [nslot] polish only: candidate marks / slack at the trial point
    double *cpacc;                  // [12][nb*oq]: S(6) yv(3) gz(3) per control point, ALL its rows (bounds, pairs, frozen); component-major, so
                                    // that the passes that read three or six of the twelve (rbase, rhs, assembly) fetch only those
    double *pwgt;                   // [npb*oq] Newton weight of every in-batch pair row (off-diagonal blocks of the knot matrices)
    double *dx, *dxa, *cvec;        // [nb*3*oq]
    double *rbase, *rhs;            // [(M-1)*nk]  (blocks of order 36: rhs is LIVE from rbase_from_acc, which leaves the predictor's right-hand side
                                    // there, until the factorisation chains have consumed it; a refused polish, which uses it for its primal
                                    // steps in that window, is followed by rhs_from_acc -- any other use of it there needs the same)
    double *Td, *To;                // [(M-1)][nk*nk], [(M-2)][nk*nk]
    double *Lf;                     // wave path: [(M-1)] slots of M_j = L_j^-T (its triangle) and 1 / d_j, laid out by knot_factor_layout.h; on a
                                    // 128-byte boundary inside a region of 2 (M-1) nk^2 doubles (nk <= 36), of which it uses a fraction
    double *boxlo, *boxhi;          // [nb][M][3]
    double *Lk, *Dk, *Ek;           // [M+1][9]
    double *segsc;                  // [M] dt^-5 (build_Q_p :349-351)
    int *flist, *fcnt, *fbase;      // non-redundant frozen neighbours per (batch agent, segment): [nb][M][NF], [nb][M], [nb][M]
    int *fnear;                     // (round 5) [nb][M] how many of a group's neighbours are NEAR (they come first in its rows; the far ones sit at
                                    // the back of its flist): the interior-point sweeps only walk the near rows (see QP_FAR_SLACK)
    int *fperm, *frank;             // [nb][M]: groups ordered by falling row count (fperm[rank] = group, frank[group] = rank)
    int *tile_base;                 // [ntile + 1] first slot of each tile
    int *wi_of;                     // [nb*oq] column (wi) of control point (a, j6)
    float* nrm;                     // [sum cnt][3] signed normal of frozen row (group, idx): the six rows of a group share it
    double* polish;                 // PolishWs storage
    double* prof;                   // QP_PROFILE builds: this mission's diagnostic scalars (chain-side timers), else nullptr
};

__host__ __device__ inline size_t ws_int_count(int N, int M, int nbmax) {
    QpDims d = make_dims(N, M, 0, nbmax);
    return (size_t)nbmax * M * N /*flist*/ + 5 * (size_t)nbmax * M /*fcnt fbase fperm frank fnear*/ + d.ntile + 1 + (size_t)nbmax * d.oq /*wi_of*/ +
           3 * (size_t)nbmax * M * N /*nrm (floats)*/ + 8;
}

__host__ __device__ inline size_t ws_doubles(int N, int M, int nbmax) {
    QpDims d = make_dims(N, M, 0, nbmax);
    size_t n = 7 * d.nslot_max + 12 * (size_t)nbmax * d.oq + (size_t)(d.npb ? d.npb : 1) * d.oq + 3 * (size_t)nbmax * 3 * d.oq +
               2 * (size_t)d.nj * d.nk + (size_t)d.nj * d.ldb * d.ldb + 2 * (size_t)d.nj * (d.nk < 36 ? d.nk : 36) * (d.nk < 36 ? d.nk : 36) +
               (size_t)(d.nj > 1 ? d.nj - 1 : 1) * d.ldb * d.ldb + 4 +
               2 * (size_t)nbmax * M * 3 + 3 * (size_t)(M + 1) * 9 + M + 64 + (ws_int_count(N, M, nbmax) + 1) / 2 + 2 +
               /* polish: cand, V, S, counters, big factor */ polish_ws_doubles(d.nj, d.nk);
    return n;
}

__device__ inline QpWs carve(double* base, const QpDims& d, int nbmax) {
    QpDims dm = make_dims(d.N, d.M, 0, nbmax);
    QpWs w;
    double* p = base;
    w.s = p, p += dm.nslot_max;
    w.z = p, p += dm.nslot_max;
    w.s2 = p, p += dm.nslot_max;
    w.z2 = p, p += dm.nslot_max;
    w.rh = p, p += dm.nslot_max;
    w.cc = p, p += dm.nslot_max;
    w.ds = p, p += dm.nslot_max;
    w.cpacc = p, p += 12 * (size_t)nbmax * d.oq;
    w.pwgt = p, p += (size_t)(dm.npb ? dm.npb : 1) * d.oq;
    w.dx = p, p += (size_t)nbmax * 3 * d.oq;
    w.dxa = p, p += (size_t)nbmax * 3 * d.oq;
    w.cvec = p, p += (size_t)nbmax * 3 * d.oq;
    w.rbase = p, p += (size_t)dm.nj * dm.nk;
    w.rhs = p, p += (size_t)dm.nj * dm.nk;
    p += (4 - ((p - base) & 3)) & 3;  // 32-byte alignment of the blocks (vector loads of the tiled path)
    w.Td = p, p += (size_t)dm.nj * dm.ldb * dm.ldb;
    w.To = p, p += (size_t)(dm.nj > 1 ? dm.nj - 1 : 1) * dm.ldb * dm.ldb;
    // wave path only (a short last batch).  The slots start on a 128-byte line (the mission's base is one: abi/session.hip): the region is
    // more than twice what they need -- kf_stride(nk) <= nk^2 -- so the up to 15 doubles in front of them come out of it
    w.Lf = p + ((16 - ((p - base) & 15)) & 15), p += 2 * (size_t)dm.nj * (dm.nk < 36 ? dm.nk : 36) * (dm.nk < 36 ? dm.nk : 36);
    w.boxlo = p, p += (size_t)nbmax * d.M * 3;
    w.boxhi = p, p += (size_t)nbmax * d.M * 3;
    w.Lk = p, p += (size_t)(d.M + 1) * 9;
    w.Dk = p, p += (size_t)(d.M + 1) * 9;
    w.Ek = p, p += (size_t)(d.M + 1) * 9;
    w.segsc = p, p += d.M;
    int* ip = (int*)p;
    w.flist = ip, ip += (size_t)nbmax * d.M * d.N;
    w.fnear = ip, ip += (size_t)nbmax * d.M;
    w.fcnt = ip, ip += (size_t)nbmax * d.M;
    w.fbase = ip, ip += (size_t)nbmax * d.M;
    w.fperm = ip, ip += (size_t)nbmax * d.M;
    w.frank = ip, ip += (size_t)nbmax * d.M;
    w.tile_base = ip, ip += dm.ntile + 1;
    w.wi_of = ip, ip += (size_t)nbmax * d.oq;
    w.nrm = (float*)ip;
    w.polish = p + (ws_int_count(d.N, d.M, nbmax) + 1) / 2 + 2;
    w.prof = nullptr;
    return w;
}

// ---- reductions ------------------------------------------------------------------------------------------------
// Wave-wide (result in every lane): inside a row of 16 lanes by DPP (quad permutes, half-row and row mirrors: VALU latency), across the
// four rows through readlane: ~300 cycles, where six butterfly steps of ds_bpermute pairs took ~1000 of dependent LDS round trips -- an
// interior-point iteration has ten of these reductions, and every Lawson-Hanson step of the polish two or three on its dependent path.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double red_op(double a, double b, int op) { return op == 0 ? a + b : (op == 1 ? fmax(a, b) : fmin(a, b)); }
__device__ __forceinline__ double rl(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double wave_red(double v, int op /*0 sum,1 max,2 min*/) {
    using namespace red_order;  // (common/reduce_order.h: the order of operations, shared with its host restatement)
    v = red_op(v, dpp_f64<DPP_CTRL[0]>(v), op);  // quad_perm [1,0,3,2]
    v = red_op(v, dpp_f64<DPP_CTRL[1]>(v), op);  // quad_perm [2,3,0,1]
    v = red_op(v, dpp_f64<DPP_CTRL[2]>(v), op);  // row_half_mirror
    v = red_op(v, dpp_f64<DPP_CTRL[3]>(v), op);  // row_mirror: every lane of a row holds the row's result
    return red_op(red_op(rl(v, 0), rl(v, 16), op), red_op(rl(v, 32), rl(v, 48), op), op);
}
// Block-wide: the wave reduction, then across the waves through `red`.  Two barriers: the one in front of the write would only protect
// the previous reduction's readers, which the barrier at ITS end has already let go.
__device__ inline double block_reduce(double v, int op /*0 sum,1 max,2 min*/, double* red) {
    v = wave_red(v, op);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double r = red[0];
    for (int i = 1; i < QP_THREADS / 64; ++i) r = red_op(r, red[i], op);
    __syncthreads();
    return r;
}
// K reductions that happen together: every value keeps its own operation and its own order of operations -- the wave steps of wave_red and
// the left-to-right walk over the wavefronts' results, so each result is block_reduce's bit for bit --, but the K DPP chains are
// interleaved step by step (independent instructions fill each other's latency) and ONE pair of barriers serves a chunk of values
// (common/reduce_order.h: four values on the 256-thread build, two on the 512-thread build; a K above that takes a pair of barriers more).
template <int K>
__device__ __forceinline__ void block_reduce_n(double (&v)[K], const int (&op)[K], double* red) {
    using namespace red_order;
    constexpr int NW = QP_THREADS / 64, CH = chunk(NW);
    static_assert(CH >= 1, "a value's partial results fit the reduction scratch");
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = red_op(v[q], dpp_f64<DPP_CTRL[0]>(v[q]), op[q]);
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = red_op(v[q], dpp_f64<DPP_CTRL[1]>(v[q]), op[q]);
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = red_op(v[q], dpp_f64<DPP_CTRL[2]>(v[q]), op[q]);
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = red_op(v[q], dpp_f64<DPP_CTRL[3]>(v[q]), op[q]);
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = red_op(red_op(rl(v[q], 0), rl(v[q], 16), op[q]), red_op(rl(v[q], 32), rl(v[q], 48), op[q]), op[q]);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q0 = 0; q0 < K; q0 += CH) {
        if (lane == 0) {
#pragma unroll
            for (int q = q0; q < K && q < q0 + CH; ++q) red[slot(q - q0, wave, NW)] = v[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = q0; q < K && q < q0 + CH; ++q) {
            double r = red[slot(q - q0, 0, NW)];
            for (int i = 1; i < NW; ++i) r = red_op(r, red[slot(q - q0, i, NW)], op[q]);
            v[q] = r;
        }
        __syncthreads();
    }
}

// ---- wave-uniform arguments ------------------------------------------------------------------------------------
// What the stand-alone factor / solve functions (factor_entry_*, solve_entry_*) take by value:
struct BlkArgs {
    int nk, nj, ldb, lds_avail;
    double *Td, *To, *Lf;
    double* Ek;
    double* prof;
#if QP_FWD36
    double* rhs;  // QP_FWD_IN_FACTOR: the chains read the predictor's right-hand side and leave z_j / x_mid there (QpWs::rhs)
#endif
};
// Arguments of a non-kernel function arrive in VECTOR registers, and the compiler treats them as divergent: every pointer, dimension and
// address derived from them would live in VGPRs for the whole function -- that is what spills inside the knot
// loops, and a spill reload on a dependent chain costs a memory round trip.  They are wave-uniform by construction, so they are moved to
// scalar registers explicitly (v_readfirstlane); everything computed from them then stays scalar.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <class T>
__device__ __forceinline__ T* uni(T* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (T*)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void blk_unpack(const BlkArgs& b, QpDims& d, QpWs& w) {
    d = QpDims{};
    w = QpWs{};
    d.nk = uni(b.nk), d.nj = uni(b.nj), d.ldb = uni(b.ldb), d.ld = d.nk + 1;
    w.Td = uni(b.Td), w.To = uni(b.To), w.Lf = uni(b.Lf), w.Ek = uni(b.Ek), w.prof = uni(b.prof);
#if QP_FWD36
    w.rhs = uni(b.rhs);  // (every other pointer of QpWs stays null in the stand-alone functions)
#endif
}
// the same for a whole struct passed by value (polish_entry): every 32-bit word of it through v_readfirstlane
template <class T>
__device__ __forceinline__ T uni_words(const T& v) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    union U {
        T t;
        unsigned wd[sizeof(T) / 4];
        __device__ U() {}
    } in, out;
    in.t = v;
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) out.wd[i] = __builtin_amdgcn_readfirstlane(in.wd[i]);
    return out.t;
}

// ------------------------------------------------------------------------------------------------------------
// per-mission constants: L_j (continuity map), D_j = L_j'(2Q22)L_j + 2Q11, E_j = 2 Q12 L_{j+1}
// Aeq_base rows at knot j (rbp_planner.hpp:390-399):  dl^-i nn_i A_T.row(i) c_{j-1} = dr^-i nn_i A_0.row(i) c_j
// ------------------------------------------------------------------------------------------------------------
__device__ void mission_constants(const QpDims& d, const double* T, QpWs& w) {
    const int M = d.M;
    for (int m = threadIdx.x; m < M; m += QP_THREADS) w.segsc[m] = pow(T[m + 1] - T[m], -5.0);
    for (int j = threadIdx.x; j <= M; j += QP_THREADS) {
        double* L = w.Lk + 9 * j;
        for (int e = 0; e < 9; ++e) L[e] = 0;
        if (j >= 1 && j < M) {
            const double r = (T[j] - T[j - 1]) / (T[j + 1] - T[j]);  // dl / dr
            // c5 = u0 ; c4 = c5 - r (u1 - u0) ; c3 = 2 c4 - c5 + r^2 (u0 - 2 u1 + u2)   (rows: c3, c4, c5)
            L[0] = (1 + r) * (1 + r), L[1] = -2 * r * (1 + r), L[2] = r * r;
            L[3] = 1 + r, L[4] = -r, L[5] = 0;
            L[6] = 1, L[7] = 0, L[8] = 0;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j <= M; j += QP_THREADS) {
        double* D = w.Dk + 9 * j;
        double* E = w.Ek + 9 * j;
        for (int e = 0; e < 9; ++e) D[e] = 0, E[e] = 0;
        if (j >= 1 && j < M) {
            const double sl = pow(T[j] - T[j - 1], -5.0), sr = pow(T[j + 1] - T[j], -5.0);  // build_Q_p :349-351
            const double* L = w.Lk + 9 * j;
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
                    D[3 * a + b] = 2 * (s + Qbase[6 * a + b] * sr);
                }
            if (j + 1 < M) {
                const double* Ln = w.Lk + 9 * (j + 1);
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) {
                        double s = 0;
                        for (int c = 0; c < 3; ++c) s += Qbase[6 * a + 3 + c] * sr * Ln[3 * c + b];
                        E[3 * a + b] = 2 * s;  // rows u_j, cols u_{j+1}
                    }
            }
        }
    }
    __syncthreads();
}
