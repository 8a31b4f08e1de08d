// qp_batch.inc — the batch driver: the set-up of one batch QP (qp_setup_batch), its interior-point loop and polish (qp_batch_body), the
// per-mission tables (mission_tables) and the out-of-line rest of a mission's schedule (restore_dummy, qp_batch_body_outofline,
// qp_finish_schedule); the trace build's checksums (TRC, trc_sum).  Included by qp.hip last, after qp_polish.inc: it calls into every layer
// above it.  The kernels that run it (qp_batch_kernel) and the launch stay in qp.hip.

#ifdef QP_TRACE
#ifndef QP_TRACE_BATCH
#define QP_TRACE_BATCH 0
#endif
// developer build: per-iteration checksums of the first batch QP of a mission, written into the mission's coef slot
#define TRC(slot, expr)                                                         \
    do {                                                                        \
        if (batch == QP_TRACE_BATCH && pass_index == 0 && iter < 100) {                       \
            const double v_ = (expr);                                           \
            if (tid == 0) trc[iter * 16 + (slot)] = v_;                         \
        }                                                                       \
    } while (0)
__device__ double trc_sum(const double* p, size_t n, double* red) {
    double a = 0;
    for (size_t i = threadIdx.x; i < n; i += QP_THREADS) a += fabs(p[i]);
    return block_reduce(a, 0, red);
}
#else
#define TRC(slot, expr)
#endif

// ------------------------------------------------------------------------------------------------------------
// set-up of one batch QP (all threads of the workgroup): mission constants, the SFC box of every (batch agent, segment), the pinned end
// control points, the presolve lists and the row constants.  false: the mission was abandoned (S.status set).
// ------------------------------------------------------------------------------------------------------------
// far_R: QP_FAR_SLACK of this attempt (1e300: every row near); nfar: how many (group, neighbour) entries were classified far.
__device__ __forceinline__ bool qp_setup_batch(const DevSession& S, RowCtx& c, double* ctrl, const double* T, int mission, int first, int nb,
                                               int* flag, double* lds, int& frozen_free_rows, double far_R, int& nfar) {
    const int tid = threadIdx.x, N = S.N;
    const QpDims& d = c.d;
    const QpWs& w = c.w;
    const int M = d.M;
    // (segsc, Lk, Dk, Ek and the polish's K0 tables are the mission's: mission_tables, once per launch)
    init_block_pads(d, w);

    // SFC box of every (batch agent, segment): first box with end time >= T[m+1]  (rbp_planner.hpp:447-453)
    // (the box end times go through LDS: the scan below is a chain of dependent reads -- four threads, ~40 steps each --, and from
    // global memory every step was a trip of its own; the boxes themselves are then copied by all threads at once)
    {
        const int need = nb * S.max_boxes + (M + 2) + (nb * M + 1) / 2 + 1;
        const bool stage = need <= c.lds_avail;          // (wide batches of the tiled path: straight from global memory)
        double* bt_l = lds;                              // [nb][max_boxes]
        double* T_l = lds + nb * S.max_boxes;            // [M + 1]
        int* sel_l = stage ? (int*)(T_l + M + 2) : w.fcnt;  // [nb][M]  (fcnt is filled by the presolve below)
        if (stage) {
            for (int it = tid; it < nb * S.max_boxes; it += QP_THREADS)
                bt_l[it] = S.sfc_time[((size_t)mission * N + first + it / S.max_boxes) * S.max_boxes + it % S.max_boxes];
            for (int it = tid; it <= M; it += QP_THREADS) T_l[it] = T[it];
            __syncthreads();
        }
        for (int a = tid; a < nb; a += QP_THREADS) {
            const int qa = first + a;
            int nbx = S.sfc_count[(size_t)mission * N + qa];
            if (nbx <= 0) {  // no SFC boxes: the planner stage was run on a plan whose corridor was never computed (caller error)
                atomicCAS(&S.status[mission], 0, (int)RBP_ERR_BAD_ARGUMENT);
                nbx = 1;  // keeps the reads below inside the agent's slot; the mission is abandoned after the barrier
            }
            const double* bt = stage ? bt_l + a * S.max_boxes : S.sfc_time + ((size_t)mission * N + qa) * S.max_boxes;
            const double* Tt = stage ? T_l : T;
            int bi = 0;
            for (int m = 0; m < M; ++m) {
                while (bi < nbx && bt[bi] < Tt[m + 1]) bi++;
                sel_l[a * M + m] = bi < nbx ? bi : nbx - 1;
            }
        }
        __threadfence_block();
        __syncthreads();
        for (int it = tid; it < nb * M * 3; it += QP_THREADS) {
            const int am = it / 3, k = it % 3, a = am / M;
            const double* bx = S.sfc_box + ((size_t)mission * N + first + a) * S.max_boxes * 6 + 6 * sel_l[am];
            w.boxlo[(size_t)am * 3 + k] = bx[k];
            w.boxhi[(size_t)am * 3 + k] = bx[3 + k];
        }
        __threadfence_block();
        __syncthreads();
    }
    // pin the six end control points of the batch agents to the start/goal state (rows 0-5 of Aeq_base, :380-387)
    for (int it = tid; it < nb * 3; it += QP_THREADS) {
        const int a = it / 3, k = it % 3, qa = first + a;
        const double* st = S.start + ((size_t)mission * N + qa) * 9;
        const double* gl = S.goal + ((size_t)mission * N + qa) * 9;
        const double h0 = T[1] - T[0], hT = T[M] - T[M - 1];
        double* x = ctrl + ((size_t)qa * 3 + k) * d.oq;
        x[0] = st[k], x[1] = x[0] + h0 * st[k + 3] / 5, x[2] = 2 * x[1] - x[0] + h0 * h0 * st[k + 6] / 20;
        double* xe = x + 6 * (M - 1);
        xe[5] = gl[k], xe[4] = xe[5] - hT * gl[k + 3] / 5, xe[3] = 2 * xe[4] - xe[5] + hT * hT * gl[k + 6] / 20;
    }
    __threadfence();
    __syncthreads();
    if (__hip_atomic_load(&S.status[mission], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return false;  // set above: an agent without boxes

    // ---- presolve: a frozen-neighbour row  sg*n.(d_f - x_a) >= r_a + r_f  is implied by the SFC bounds of (a, segment) when
    // its slack is positive for EVERY x_a in the box; such rows cannot be active and are dropped (exact: the feasible
    // set is unchanged).  Per (agent, segment) the surviving neighbours are listed; ~72 % of the rows go away on the
    // 64-agent missions.
    // (the work area is free here: the box stage's last reader is behind the barriers above; wide batches of the tiled path: global memory)
    const bool cnt_lds = (3 * nb * M + 1) / 2 <= c.lds_avail;
    int* fc_l = cnt_lds ? (int*)lds : w.fcnt;            // [nb][M]  fcnt
    int* fn_l = cnt_lds ? (int*)lds + nb * M : w.fnear;  // [nb][M]  fnear
    int* fp_l = cnt_lds ? (int*)lds + 2 * nb * M : w.fperm;  // [nb * M]  fperm
    for (int it = tid; it < nb * M; it += QP_THREADS) {
        const int a = it / M, seg = it % M, qa = first + a;
        const double ra = c.radius[qa];
        const double* lo = w.boxlo + ((size_t)a * M + seg) * 3;
        const double* hi = w.boxhi + ((size_t)a * M + seg) * 3;
        int cnt = 0, nfar_g = 0;
        int* fl = w.flist + (size_t)it * N;
        double xa6[6][3];  // this group's own control points at the starting point (the near / far classification, see QP_FAR_SLACK)
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int e = 0; e < 3; ++e) xa6[i][e] = ctrl[((size_t)qa * 3 + e) * d.oq + 6 * seg + i];
        // (four neighbours per round, all their loads ahead of the list stores: the compiler does not move a load across a store, and a
        // neighbour per round meant 60 trips to memory in a row, ~1 us each under load)
        for (int f0 = 0; f0 < N && N > 1; f0 += 4) {
            bool keep4[4], far4[4];
            float nvq[4][3];
            double cf[4][6][3];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = f0 + q < N ? f0 + q : N - 1;
                const bool a_first = qa < f;
                const int lo_ = a_first ? qa : f, hi_ = a_first ? f : qa;
                const float* nv = c.normals + (pair_index(N, lo_ == hi_ ? 0 : lo_, lo_ == hi_ ? 1 : hi_) * M + seg) * 3;
#pragma unroll
                for (int e = 0; e < 3; ++e) nvq[q][e] = nv[e];
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int e = 0; e < 3; ++e) cf[q][i][e] = ctrl[((size_t)f * 3 + e) * d.oq + 6 * seg + i];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = f0 + q;
                const bool a_first = qa < f;
                const double sg = a_first ? 1.0 : -1.0;
                const double n0 = sg * (double)nvq[q][0], n1 = sg * (double)nvq[q][1], n2 = sg * (double)nvq[q][2];
                const double mx = fmax(n0 * lo[0], n0 * hi[0]) + fmax(n1 * lo[1], n1 * hi[1]) + fmax(n2 * lo[2], n2 * hi[2]);
                const double rr = ra + c.radius[f < N ? f : 0];
                bool keep = false;
                double smin = 1e300;  // smallest slack of the group's six rows at the starting point
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double nd = n0 * cf[q][i][0] + n1 * cf[q][i][1] + n2 * cf[q][i][2];
                    if (!(nd - rr - mx > 1e-6)) keep = true;
                    smin = fmin(smin, nd - rr - (n0 * xa6[i][0] + n1 * xa6[i][1] + n2 * xa6[i][2]));
                }
                keep4[q] = keep && f < N && !(f >= first && f < first + nb);
                far4[q] = smin > far_R;
            }
            // the near neighbours fill the group's list from the front, the far ones from the back (entry idx >= near count of the group's
            // rows is fl[N - 1 - (idx - near count)]): the rows of the interior-point phase come first in every column
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (keep4[q]) {
                    if (far4[q])
                        fl[N - 1 - nfar_g++] = f0 + q;
                    else
                        fl[cnt++] = f0 + q;
                }
        }
        w.fnear[it] = cnt;
        w.fcnt[it] = cnt + nfar_g;
        if (cnt_lds) fc_l[it] = cnt + nfar_g, fn_l[it] = cnt;
    }
    // The groups' counts go on through LDS (fc_l, fn_l: written above next to the global arrays; fp_l: the rank sort's permutation): the two
    // prefix sums and the rank sort below read every group's count -- 144 loads per thread, which from global memory were trips --, and with
    // the counts there the first prefix sum and the rank sort have no global dependency between them: one phase, two barriers fewer.
    if (tid == 0) flag[0] = 0, flag[1] = 0;
    __threadfence_block();
    __syncthreads();
    // offsets of the groups' normal lists (exclusive prefix sum of the counts) and the number of non-constant frozen rows: every group
    // sums its predecessors itself.  Sweep work order: the threads of a wavefront walk the row lists of their control points in lockstep, so
    // a wave costs as much as its longest list.  Handing out the (agent, segment) groups by falling row count puts lists of
    // similar length into the same wave (and the long ones into the first round).  Rank sort, one thread per group.
    for (int it = tid; it < nb * M; it += QP_THREADS) {
        const int ci = fc_l[it], cn = fn_l[it];
        int acc = 0, rank = 0;
        for (int o = 0; o < nb * M; ++o) {
            const int co = fc_l[o];
            acc += o < it ? co : 0;
            rank += (co > ci || (co == ci && o < it)) ? 1 : 0;
        }
        w.fbase[it] = acc;
        const int seg = it % M;
        atomicAdd(flag, cn * ((seg == 0 || seg == M - 1) ? (M == 1 ? 0 : 3) : 6));  // (rows of the interior-point phase: the near ones)
        atomicAdd(flag + 1, ci - cn);
        w.fperm[rank] = it;
        if (cnt_lds) fp_l[rank] = it;
        w.frank[it] = rank;
    }
    __threadfence_block();
    __syncthreads();
    frozen_free_rows = *flag;
    nfar = flag[1];
    // row storage (see the note above QpWs): tile t holds the control points wi = 64 t .. 64 t + 63; its columns are as long as
    // its first (= longest) one
    for (int t = tid; t <= d.ntile; t += QP_THREADS) {  // (every tile sums its predecessors)
        int base = 0;
        for (int o = 0; o < t; ++o) base += 64 * (d.ncol0 + fc_l[fp_l[(64 * o) / 6]]);
        w.tile_base[t] = base;
    }
    for (int wi = tid; wi < nb * d.oq; wi += QP_THREADS) {
        const int grp = fp_l[wi / 6], a = grp / M, seg = grp - a * M;
        w.wi_of[a * d.oq + 6 * seg + wi % 6] = wi;
    }
    __threadfence_block();
    __syncthreads();
    // tabulate the constants of the surviving frozen rows: the signed normal per (group, neighbour) and, per row,
    // rh = n . d_f - (r_a + r_f)
    for (int it = tid; it < nb * M * 6; it += QP_THREADS) {
        const int as = it / 6, i = it % 6, a = as / M, seg = as % M, qa = first + a, j6 = 6 * seg + i;
        const int cnt = w.fcnt[as], cn = w.fnear[as];
        const int* fl = w.flist + (size_t)as * N;
        const int wi = 6 * w.frank[as] + i;
        const size_t r0 = (size_t)w.tile_base[wi >> 6] + (wi & 63) + (size_t)d.ncol0 * 64;
        float* nr = w.nrm + (size_t)w.fbase[as] * 3;
        const double ra = c.radius[qa];
        for (int i0 = 0; i0 < cnt; i0 += 4) {  // (four rows per round, loads first: see the presolve loop)
            int fq[4];
            float nvq[4][3];
            double cfq[4][3];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = i0 + q < cnt ? i0 + q : cnt - 1;
                fq[q] = fl[e < cn ? e : N - 1 - (e - cn)];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = fq[q];
                const bool a_first = qa < f;
                const float* nv = c.normals + (pair_index(N, a_first ? qa : f, a_first ? f : qa) * M + seg) * 3;
#pragma unroll
                for (int e = 0; e < 3; ++e) nvq[q][e] = nv[e], cfq[q][e] = ctrl[((size_t)f * 3 + e) * d.oq + j6];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = i0 + q, f = fq[q];
                if (idx < cnt) {
                    const float sgf = qa < f ? 1.0f : -1.0f;
                    const double n0 = (double)(sgf * nvq[q][0]), n1 = (double)(sgf * nvq[q][1]), n2 = (double)(sgf * nvq[q][2]);
                    if (i == 0) nr[3 * idx] = sgf * nvq[q][0], nr[3 * idx + 1] = sgf * nvq[q][1], nr[3 * idx + 2] = sgf * nvq[q][2];
                    w.rh[r0 + (size_t)idx * 64] = n0 * cfq[q][0] + n1 * cfq[q][1] + n2 * cfq[q][2] - (ra + c.radius[f]);
                }
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    return true;
}

// ------------------------------------------------------------------------------------------------------------
// one batch QP of one mission (all threads of the workgroup)
// ------------------------------------------------------------------------------------------------------------
// far_R: see QP_FAR_SLACK.  Returns 1 when the batch QP has to be solved again with every row near (the caller puts the batch agents'
// control points back to the starting point first), else 0.
__device__ __forceinline__ int qp_batch_body(const DevSession& S, double* ws_base, size_t ws_stride, int mission, int batch, int nbmax,
                                             int reset_cost, int lds_doubles, int pass_index, double far_R) {
    const int tid = threadIdx.x;
    if (S.status[mission] != 0) return 0;
    // M of this mission: made wave-uniform explicitly (an SGPR like every other dimension; as a per-lane value it was spilled
    // and reloaded under divergent control flow with some lanes reading garbage)
    const int N = S.N, M = __builtin_amdgcn_readfirstlane(S.Mk[mission]), MS = S.M;  // MS: slot stride of the per-mission arrays
    const int first = batch * nbmax;
    const int nb = min(nbmax, N - first);
    if (nb <= 0) return 0;
    RowCtx c;
    c.meta = nullptr;
    c.scal = S.scalars + (size_t)mission * SC_N, c.mission = mission, c.lds_avail = lds_doubles - 32;
    c.d = make_dims(N, M, first, nb);
    c.w = carve(ws_base + (size_t)mission * ws_stride, c.d, nbmax);
    double* ctrl = S.ctrl + (size_t)mission * N * 3 * 6 * MS;
    c.ctrl = ctrl;
    c.normals = S.rsfc_normal + (size_t)mission * S.npair * MS * 3;
    c.radius = S.radius + (size_t)mission * N;
    const QpDims& d = c.d;
    const QpWs& w = c.w;
    const double* T = S.T + (size_t)mission * (MS + 1);
    double* scal = S.scalars + (size_t)mission * SC_N;

    // dynamic LDS: [0,32) reduction scratch + flags (always live), then a work area shared in turn by the block
    // factorisation (3 blocks), the staged substitutions (4 padded blocks + rhs) and the polish
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    double* red = lds_raw;  // 16
    int* flag = (int*)(lds_raw + 16);
    double* lds = lds_raw + 32;
#ifdef QP_PROFILE
#if QP_FWD36
    const BlkArgs ba{d.nk, d.nj, d.ldb, c.lds_avail, w.Td, w.To, w.Lf, w.Ek, scal, w.rhs};
#else
    const BlkArgs ba{d.nk, d.nj, d.ldb, c.lds_avail, w.Td, w.To, w.Lf, w.Ek, scal};
#endif
#else
#if QP_FWD36
    const BlkArgs ba{d.nk, d.nj, d.ldb, c.lds_avail, w.Td, w.To, w.Lf, w.Ek, nullptr, w.rhs};
#else
    const BlkArgs ba{d.nk, d.nj, d.ldb, c.lds_avail, w.Td, w.To, w.Lf, w.Ek, nullptr};
#endif
#endif

    PROF_DECL;
    int frozen_free_rows = 0, nfar = 0;
    if (!qp_setup_batch(S, c, ctrl, T, mission, first, nb, flag, lds, frozen_free_rows, far_R, nfar)) return 0;
    PROF(8);  // batch setup: constants, SFC boxes, presolve lists, row constants
    PassIO io;
    __shared__ RowCtx c_lds;  // the sweeps' view of the row context (see sweep<>)
#if QP_ROW_BLK > 0
    __shared__ SweepMeta meta_lds;
    const bool meta_ok = nb * d.M <= QP_META_G && d.ntile + 1 <= 16 && d.N <= 256 && (size_t)nb * d.M * d.N < 65536;
    __syncthreads();
    if (meta_ok) {
        for (int rk = tid; rk < nb * d.M; rk += QP_THREADS) {
            const int g = w.fperm[rk];
            meta_lds.grp[rk] = (unsigned char)g, meta_lds.near[rk] = (unsigned char)w.fnear[g], meta_lds.all[rk] = (unsigned char)w.fcnt[g];
            meta_lds.fbase[rk] = (unsigned short)w.fbase[g];
        }
        for (int t = tid; t <= d.ntile; t += QP_THREADS) meta_lds.tile_base[t] = w.tile_base[t];
    }
    c.meta = meta_ok ? &meta_lds : nullptr;
#endif
    __syncthreads();
    if (tid == 0) c_lds = c;
    __syncthreads();
    io.mu0 = QP_MU0, io.s_floor = QP_SFLOOR, io.dreg = 1e-9, io.sigma_mu = 0, io.alpha = 0;
    // presolve: constant rows (pinned control points) must hold within 1e-6 (CPLEX default feasibility tolerance)
    io.vmax = 0;
    row_pass<PASS_PRESOLVE>(c, io);
    const double pin_viol = block_reduce(io.vmax, 1, red);
    if (pin_viol > 1e-6) {
        if (tid == 0) {
            atomicCAS(&S.status[mission], 0, (int)RBP_ERR_QP_FAILED);
#ifndef QP_PROFILE
            scal[SC_PROF0 + 1] = 1000.0 * batch + 1, scal[SC_PROF0 + 2] = pin_viol;  // why: a constant (pinned) row is violated
#endif
        }
        return 0;
    }
    const double nrows_free = (double)((size_t)(d.oq - 6) * (6 * d.nb + d.npb)) + (double)frozen_free_rows;  // every pair row once
    bool ok = false;
    int it_count = 0, polished = 0, early_tries = 0, fail_reason = 3;
    double gap_next = 0, pres_next = 0, kkt_ipm = 0;
    double flops = 0, rows_swept = 0, row_bytes = 0, sweep_bytes = 0;
    // ALGORITHMIC HBM bytes of one interior-point iteration (DESIGN.md 3.3; the numerator of the HBM roofline): per row the three
    // sweeps read (s, z) three times and write them once (64 B), frozen rows also read their constant three times (+24 B); per free
    // control point the accumulators are written twice and read four times (288 B); the knot blocks: on the tiled path 8 block
    // transfers of ldb^2 doubles per knot (T_j written and read, two factor blocks written once and read by both substitutions); on the
    // wave path the knot's factor is ONE triangle, M_j = L_j^-T, written once and staged four times (forward and backward pass of the two
    // substitutions), plus the reciprocal pivots: 5 triangles + 5 nk.  (Until round 6 the model also counted T_j written and read as a
    // triangle -- 7 triangles -- which both builds have stopped doing: the blocks are assembled just in time into LDS images and never
    // reach global memory, so those bytes are no longer part of what the algorithm has to move.)
    // (QP_FWD_IN_FACTOR, blocks of order 36: the predictor's forward pass reads M_j where the factorisation left it in LDS and its middle block
    // is not staged either: 4.5 triangles + 4.5 nk on average -- bookkeeping of what is moved, not a gain of its own)
#if QP_FWD36
    const double blk_doubles = d.nk == 36 ? 4.5 * (d.nk * (d.nk + 1) / 2) + 4.5 * d.nk : (d.nk < 36 ? 5.0 * (d.nk * (d.nk + 1) / 2) + 5.0 * d.nk : 8.0 * d.ldb * d.ldb);
#else
    const double blk_doubles = d.nk <= 36 ? 5.0 * (d.nk * (d.nk + 1) / 2) + 5.0 * d.nk : 8.0 * d.ldb * d.ldb;
#endif
    const double bytes_sweeps = 88.0 * frozen_free_rows + 64.0 * (double)(d.oq - 6) * (6.0 * d.nb + 2.0 * d.npb) + 288.0 * (double)d.nb * (d.oq - 6);
    const double bytes_iter = bytes_sweeps + 8.0 * (double)d.nj * blk_doubles;
    const PolishWs pw = polish_carve(w.polish, d.nj);
    row_pass<PASS_INIT>(c, io);
    __threadfence_block();
    __syncthreads();
#ifdef QP_TRACE
    double* trc = S.coef + (size_t)mission * N * 3 * 6 * MS;
#endif
    for (int iter = 0; iter < QP_MAX_ITERS; ++iter) {
        it_count = iter;
        // ---- sweep 1: weights, accumulators, residual norms (from the second iteration on it is fused into the previous
        // iteration's update sweep)
        PROF(0);
        if (iter == 0) {
            io.sum0 = 0, io.vmax = 0;
            SWEEP(PASS_BUILD);
        }
        PROF(1);
        if (iter == 0) {
            double rv[2] = {io.sum0, io.vmax};
            block_reduce_n<2>(rv, {0, 1}, red);
            gap_next = rv[0], pres_next = rv[1];
        }
        const double gap = gap_next, pres = pres_next;
        __threadfence_block();
        __syncthreads();
        double dmax, gmax;
        // rbase = -F'(2Qx + G'z); on the QP_FWD36 path also the predictor's rhs = rbase + F'G'v, which the chains consume block by block while
        // they factorise (an iteration that ends below in a termination test or an accepted polish leaves it unused)
        constexpr bool rhs_early = QP_FWD36;
        rbase_from_acc(c, dmax, gmax, rhs_early && d.nk == 36);
        double dg[2] = {dmax, gmax};
        block_reduce_n<2>(dg, {1, 1}, red);
        const double dres = dg[0] / (1.0 + dg[1]);
        const double mu = gap / nrows_free;
        rows_swept += nrows_free;
        kkt_ipm = fmax(pres, fmax(dres, mu));
        TRC(0, gap); TRC(1, pres); TRC(2, dres); TRC(3, trc_sum(w.rbase, (size_t)d.nj * d.nk, red)); TRC(4, trc_sum(w.cpacc, (size_t)12 * d.nb * d.oq, red));
        if (pres < 1e-9 && dres < 1e-9 && mu < 1e-10) {
            ok = true;
            break;
        }
        // rows inconsistent at rounding level (no interior and infeasible by ~1e-9): the regularised iteration settles
        // on the least-violation point with pres stuck; accept below CPLEX's default feasibility tolerance 1e-6.
        if (pres < 1e-6 && dres < 1e-9 && mu < 1e-13) {
            ok = true;
            break;
        }
        // complementarity has collapsed (mu < 1e-14) with the primal residual at rounding level while the dual residual sits on
        // its noise floor (Newton weights of 1e9+ on degenerate active sets: ~5e-9 relative): more iterations change nothing.
        // The active-set polish below turns this point into the certified optimum; if it is refused, kkt_max reports the floor.
        if (pres < 1e-9 && dres < 1e-7 && mu < 1e-14) {
            ok = true;
            break;
        }
        PROF(2);
        // EARLY CROSSOVER: the polish returns the exact optimum (KKT-verified on every row) as soon as the interior-point
        // iterate identifies the active set, which happens several iterations before the 1e-10 termination test: try it
        // when the residuals and mu fall below QP_EARLY_TOL = 1e-6 and once more at mu < 1e-8 (tuned on the 50-map sweep);
        // a refused attempt leaves the iterate untouched and the loop goes on to the 1e-10 test and the final polish.
        // POLISH FIRST (Gauss-Seidel passes >= 2, e.g. plan/iteration = 50 of BASELINE config C5): the current point is the
        // previous pass's optimum of this batch, only the frozen neighbours have moved a little, so the active set is
        // mostly unchanged.  Before the first interior-point iteration the active-set step is tried directly with the rows
        // near their bounds as candidates; it is accepted only under the same full KKT check as always (so it IS the
        // optimum of this pass's QP), otherwise the interior-point method runs as in the first pass.
        const bool polish_first = pass_index > 0 && iter == 0;
        const bool early = early_tries < QP_EARLY_TRIES && pres < QP_EARLY_TOL && dres < QP_EARLY_TOL &&
                           mu < (early_tries == 0 ? QP_EARLY_TOL : 1e-2 * QP_EARLY_TOL);
        if (S.p.polish && (polish_first || early)) {
            if (!polish_first) early_tries++;
            const int acc = polish_entry(c, pw, lds, red, flag, polish_first ? 1 : 0);
            __syncthreads();
            PROF(0);
#ifdef QP_POLSTATS
            if (tid == 0 && !polish_first) scal[25] += (early_tries == 1), scal[26] += (early_tries == 1 && acc == 0), scal[27] += (early_tries == 2), scal[29] += (early_tries == 2 && acc == 0);  // (tools/experiments/r05_polstats.py)
#endif
            if (acc == 0) {
                ok = true, polished = 1;
                break;
            }
            // (a refused attempt has used QpWs::rhs for its primal steps: the predictor's right-hand side once more, from rbase and the accumulators)
            if (rhs_early && d.nk == 36) rhs_from_acc(c, false, 0.0);
        }
        // ---- Newton matrix and factorisation
        // wave path, 512 threads: assembled behind the factorisation chains by waves 4.. (twisted_factor); the 256-thread build has no
        // waves to spare (two chains, two companions) and assembles up front with all of them
        if (d.nk > 36)
            assemble_blocks(c, lds);
        else if (ASM_HELPERS == 0 && !QP_FOLLOW_ASM)
            assemble_blocks_lds(asm_args(c), d.nj, lds);  // (256-thread build, round 6: the chains' companion waves assemble just in time instead)
        // QP_FWD_IN_FACTOR: the predictor's right-hand side is known now -- rbase + F'G'v of the build sweep's accumulators, the arithmetic the
        // rhs_mode 1 prologue of solve_staged repeats -- and the chains consume it block by block while they factorise
        // (rbase_from_acc has left it already)
        PROF(3);
        __threadfence_block();
        __syncthreads();
        TRC(5, trc_sum(w.Td, (size_t)d.nj * d.ldb * d.ldb, red));
        if (!factor_entry(ba, asm_args(c), lds, flag)) {
            fail_reason = 2;  // Newton matrix not positive definite
            break;
        }
        // logged flops of the factorisation: tiled path Cholesky + coupling solve + rank-k update = 7/3 nk^3 per knot; wave path L D L'
        // (1/3), the triangular inverse M = L^-T (1/3), the coupling rows (3 multiply-adds per entry) and the rank-nk update on the
        // columns where X is structurally non-zero (1/2): 7/6 nk^3 + 6 nk^2
        flops += d.nk <= 36 ? (double)d.nj * ((7.0 / 6.0) * d.nk * (double)d.nk * d.nk + 6.0 * d.nk * (double)d.nk)
                            : (double)d.nj * (7.0 / 3.0) * d.nk * (double)d.nk * d.nk;
        PROF(4);
        // (wave path: the knots' slots, as far as they go -- what a slot does not use stays as the workspace was cleared)
        TRC(6, trc_sum(d.nk <= 36 ? w.Lf : w.Td, d.nk <= 36 ? (size_t)d.nj * (QP_LF_PACKED ? kf_stride(d.nk) : kf_sq_stride(d.nk)) : (size_t)d.nj * d.ldb * d.ldb, red));
        // ---- predictor
#ifndef QP_TRACE
        if (d.nk <= 36) {
            PROF(5);
            // (fused: starts with rhs_from_acc into the LDS vector; ends with apply_F from it, fence and barrier -- see SolveOut)
            #if QP_FWD36
            solve_entry(ba, w.rhs, lds, SolveOut{w.dxa, w.Lk, d.oq, d.nk == 36 ? 3 : 1, w.cpacc, w.rbase, 0.0});  // (3: z_j and x_mid are in w.rhs, backward steps only)
#else
            solve_entry(ba, w.rhs, lds, SolveOut{w.dxa, w.Lk, d.oq, 1, w.cpacc, w.rbase, 0.0});
#endif
            PROF(6);
        } else
#endif
        {
            rhs_from_acc(c, false, 0.0);  // rhs = rbase + F'G'v (v from the build sweep)
            __threadfence_block();
            __syncthreads();
            PROF(5);
            TRC(7, trc_sum(w.rhs, (size_t)d.nj * d.nk, red));
            solve_entry(ba, w.rhs, lds);
            PROF(6);
            TRC(8, trc_sum(w.rhs, (size_t)d.nj * d.nk, red));
            apply_F(d, w, w.rhs, w.dxa);
            __threadfence_block();
            __syncthreads();
        }
        io.sum0 = io.sum1 = io.sum2 = 0, io.vmax = 1.0;  // vmax = max(1, max -d/x): a_aff = min(1, min -x/d)
        PROF(5);
        SWEEP(PASS_AFF);
        PROF(7);
        double av[4] = {io.vmax, io.sum0, io.sum1, io.sum2};
        block_reduce_n<4>(av, {1, 0, 0, 0}, red);
        const double a_aff = 1.0 / av[0];
        const double q0 = av[1], q1 = av[2], q2 = av[3];
        const double mu_aff = (q0 + a_aff * q1 + a_aff * a_aff * q2) / nrows_free;
        TRC(9, a_aff); TRC(10, mu_aff);
        double sigma = mu_aff / mu;
        sigma = QP_SIGMA_POW == 2 ? sigma * sigma : (QP_SIGMA_POW == 4 ? sigma * sigma * sigma * sigma : sigma * sigma * sigma);
        io.sigma_mu = sigma * mu;
        // ---- corrector (its right-hand side was accumulated by the AFF sweep in two parts)
        __threadfence_block();
        __syncthreads();
        PROF(8);
#ifndef QP_TRACE
        if (d.nk <= 36) {
            PROF(5);
            solve_entry(ba, w.rhs, lds, SolveOut{w.dx, w.Lk, d.oq, 2, w.cpacc, w.rbase, io.sigma_mu});
            PROF(6);
        } else
#endif
        {
            rhs_from_acc(c, true, io.sigma_mu);
            __threadfence_block();
            __syncthreads();
            PROF(5);
            TRC(11, trc_sum(w.rhs, (size_t)d.nj * d.nk, red));
            solve_entry(ba, w.rhs, lds);
            PROF(6);
            TRC(12, trc_sum(w.rhs, (size_t)d.nj * d.nk, red));
            apply_F(d, w, w.rhs, w.dx);
            __threadfence_block();
            __syncthreads();
        }
        flops += 2.0 * d.nj * 4.0 * d.nk * (double)d.nk;
        io.vmax = QP_STEP_FRAC;  // alpha = min(1, frac * min -x/d) = frac / max(frac, max -d/x)
        PROF(5);
        SWEEP(PASS_STEP);
        PROF(9);
        double alpha = QP_STEP_FRAC / block_reduce(io.vmax, 1, red);
        TRC(13, alpha);
        __threadfence_block();
        __syncthreads();
        // ---- step, wide neighbourhood (no product below 1e-3 * mu(alpha)) and the next iteration's first sweep in ONE pass:
        // x += alpha dx is applied speculatively, the sweep reads the OLD row state, recomputes the step, writes the NEW state
        // into the second pair of arrays, evaluates the neighbourhood test on it and builds the next iteration's weights and
        // residuals.  In the rare case the test fails the sweep is repeated from the (untouched) old state with 0.8 alpha.
        double applied = 0;
        for (int bt = 0; bt < 40; ++bt) {
            const double delta = alpha - applied;
            {  // (the batch agents' control points are contiguous: [first .. first + nb) x 3 x oq; XU entries per thread and round, loads first:
               // 3072 entries per round, so the 2592 of a batch of four at M = 36 are ONE trip to memory where rounds of four were three)
                double* xb = ctrl + (size_t)first * 3 * d.oq;
                const int nx = d.nb * 3 * d.oq;
                constexpr int XU = 3072 / QP_THREADS;
                for (int i0 = tid; i0 < nx; i0 += XU * QP_THREADS) {
                    double xv[XU], dv4[XU];
#pragma unroll
                    for (int q = 0; q < XU; ++q) {
                        const int i = i0 + q * QP_THREADS;
                        xv[q] = i < nx ? xb[i] : 0.0, dv4[q] = i < nx ? w.dx[i] : 0.0;
                    }
#pragma unroll
                    for (int q = 0; q < XU; ++q) {
                        const int i = i0 + q * QP_THREADS;
                        if (i < nx) xb[i] = xv[q] + delta * dv4[q];
                    }
                }
            }
            __threadfence_block();
            __syncthreads();
            io.alpha = alpha, io.sum0 = 0, io.vmax = 0, io.vmin = 1e300;
            SWEEP(PASS_UPBUILD);
            applied = alpha;
            double uv[3] = {io.sum0, io.vmax, io.vmin};
            block_reduce_n<3>(uv, {0, 1, 2}, red);
            gap_next = uv[0], pres_next = uv[1];
            const double pmin = uv[2];
            rows_swept += nrows_free;
            __threadfence_block();
            __syncthreads();
            if (pmin >= QP_NBHD_GAMMA * gap_next / nrows_free) break;
            alpha *= QP_NBHD_BACKOFF;
        }
        // the new state becomes the current one
        {
            double* t0 = c.w.s;
            c.w.s = c.w.s2, c.w.s2 = t0;
            t0 = c.w.z, c.w.z = c.w.z2, c.w.z2 = t0;
            if (tid == 0) c_lds.w.s = c.w.s, c_lds.w.s2 = c.w.s2, c_lds.w.z = c.w.z, c_lds.w.z2 = c.w.z2;
            __syncthreads();
        }
        rows_swept += 2 * nrows_free;
        row_bytes += bytes_iter, sweep_bytes += bytes_sweeps;
        PROF(10);  // the fused step / neighbourhood / build sweeps
        PROF(11);  // (slot of the separate update sweep they replaced: tools/qp_phase_profile.py still lists it, ~0)
    }
    if (!ok && nfar > 0) {  // the interior-point method failed on the reduced row set: once more with every row
        if (tid == 0) scal[SC_IPM_ITERS] += it_count, scal[SC_FLOPS] += flops, scal[SC_ROWS] += rows_swept;
        return 1;
    }
    if (!ok) {
        if (tid == 0) {
            atomicCAS(&S.status[mission], 0, (int)RBP_ERR_QP_FAILED);
#ifndef QP_PROFILE
            scal[SC_PROF0 + 1] = 1000.0 * batch + fail_reason, scal[SC_PROF0 + 2] = it_count;  // why: 2 factor, 3 iteration cap
#endif
        }
        return 0;
    }
    // ---- active-set polish
    if (S.p.polish && !polished) {
        int acc = polish_entry(c, pw, lds, red, flag, 0);
        if (acc == 3) {  // the dual active-set solve ran out of capacity: once more with the big factor in global memory
            __syncthreads();
            acc = polish_entry(c, pw, lds, red, flag, 2);
        }
        polished = acc == 0 ? 1 : 0;
#ifdef QP_POLSTATS
        if (tid == 0) scal[30] += 1, scal[31] += polished;
#endif
        PROF(0);
#ifndef QP_PROFILE
        if (acc != 0 && tid == 0) scal[SC_PROF0] += 1000.0 * batch + acc;  // diagnostic: which batch was not polished, and why
#endif
        __syncthreads();
    }
    __syncthreads();
    if (S.p.polish && !polished && nfar > 0) {  // refused, and rows the interior-point phase never saw exist: this point is not an answer
        if (tid == 0) scal[SC_IPM_ITERS] += it_count, scal[SC_FLOPS] += flops, scal[SC_ROWS] += rows_swept;
        return 1;
    }
    const double kkt = polished ? red[12] : kkt_ipm;
    // objective of this batch: sum x' Q_p x  (cplex.getObjValue, :164)
    double obj = 0;
    for (int it = tid; it < d.nb * 3 * M; it += QP_THREADS) {
        const int a = it / (3 * M), k = (it / M) % 3, m = it % M;
        const double sc = w.segsc[m];
        const double* xs = ctrl + ((size_t)(first + a) * 3 + k) * d.oq + 6 * m;
        double q = 0;
        for (int i = 0; i < 6; ++i)
            for (int jj = 0; jj < 6; ++jj) q += Qbase[6 * i + jj] * xs[i] * xs[jj];
        obj += q * sc;
    }
    obj = block_reduce(obj, 0, red);
    if (tid == 0) {
        if (reset_cost) scal[SC_TOTAL_COST] = 0;
        scal[SC_TOTAL_COST] += obj;
        scal[SC_IPM_ITERS] += it_count;
        scal[SC_QP_SOLVED] += 1;
        scal[SC_POLISHED] += polished;
        scal[SC_KKT_MAX] = fmax(scal[SC_KKT_MAX], kkt);
        scal[SC_FLOPS] += flops;
        scal[SC_ROWS] += rows_swept;
#ifndef QP_LHSTATS
        scal[SC_ROW_BYTES] += row_bytes;
        scal[SC_SWEEP_BYTES] += sweep_bytes;
#endif
    }
    PROF_FLUSH(scal);
    return 0;
}

// the batch agents' control points back at the starting point of the first pass: build_dummy (dummy_ctrl_point) for agents [first, first + nbmax)
__device__ void restore_dummy(const DevSession& s, int mission, int first, int nbmax) {
    const int N = s.N, MS = s.M, PS = MS + 1, M = s.Mk[mission], P = M + 1, oq = 6 * M;
    const int nb = min(nbmax, N - first);
    double* ctrl = s.ctrl + (size_t)mission * N * 3 * 6 * MS;
    for (int it = threadIdx.x; it < nb * 3 * oq; it += QP_THREADS) {
        const int j6 = it % oq, k = (it / oq) % 3, qi = first + it / (3 * oq);
        const int m = j6 / 6, j = j6 % 6;
        const float* tr = s.init_traj + (size_t)mission * N * PS * 3 + (size_t)qi * P * 3;
        ctrl[((size_t)qi * 3 + k) * oq + j6] = dummy_ctrl_point(tr, m, j, k);
    }
}

// What depends on the mission's segment times alone, once per launch and ahead of its first batch QP: segsc, Lk, Dk, Ek (mission_constants)
// and the polish's tables of K0 (qp_polish.inc).  carve() places them by nbmax, so every batch of the mission -- a narrower last one, a
// second attempt from qp_finish_schedule -- finds them where they were written.  Out of line: nothing of it is live in the batch loop.
__device__ __noinline__ void mission_tables(const DevSession* Sg, double* ws_base, size_t ws_stride, int mission, int nbmax) {
    const DevSession& S = *Sg;
    ws_base = uni(ws_base), mission = uni(mission), nbmax = uni(nbmax);
    if (S.status[mission] != 0) return;
    const int N = S.N, M = __builtin_amdgcn_readfirstlane(S.Mk[mission]);
    const QpDims d = make_dims(N, M, 0, min(nbmax, N));
    QpWs w = carve(ws_base + (size_t)mission * ws_stride, d, nbmax);
    mission_constants(d, S.T + (size_t)mission * (S.M + 1), w);
    __threadfence_block();
    __syncthreads();
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    k0_mission_tables(d.nj, w, polish_carve(w.polish, d.nj), lds_raw + 32);
    __threadfence_block();
    __syncthreads();
}

// The REST of a mission's schedule from batch (it0, l0) on, whose first attempt on the reduced row set failed (see qp_batch_kernel): that batch
// again with every row, then the remaining batches and passes.  Sg: the kernel's copy of the session struct in LDS (the body was written for a
// struct that lives in registers: it gets a private copy).
// ONE batch QP out of line.  (round 6) The rest-of-schedule function below used to inline the body inside its loops; with the body's calls
// compiled under interprocedural register allocation, a value the compiler had hoisted out of those loops into a vector register came back
// from a FAILED factorisation (the early way out of the interior-point loop) with the callee's leftovers in some lanes, and the next
// attempt computed addresses from it (memory fault in rbase_from_acc, found with rocgdb; -mllvm -enable-ipra=0 made it disappear at -6 % of
// the bench).  A call per batch QP gives every attempt a fresh frame: nothing of one attempt's register state reaches the next.  This path
// runs for ~1 batch QP in 800; its speed does not matter.
__device__ __noinline__ int qp_batch_body_outofline(const DevSession* Sg, double* ws_base, size_t ws_stride, int mission, int batch, int nbmax,
                                                    int reset_cost, int lds_doubles, int pass_index, double far_R) {
    const DevSession S = *Sg;
    return qp_batch_body(S, uni(ws_base), ws_stride, uni(mission), uni(batch), uni(nbmax), uni(reset_cost), uni(lds_doubles), uni(pass_index), far_R);
}
__device__ __noinline__ void qp_finish_schedule(const DevSession* Sg, double* ws_base, size_t ws_stride, int mission, int passes, int biter, int nbmax,
                                               int lds_doubles, int it0, int l0) {
    const DevSession S = *Sg;
    ws_base = uni(ws_base), mission = uni(mission), passes = uni(passes), biter = uni(biter), nbmax = uni(nbmax), lds_doubles = uni(lds_doubles);
    it0 = uni(it0), l0 = uni(l0);
    for (int it = it0; it < passes; ++it)
        for (int l = (it == it0 ? l0 : 0); l < biter; ++l) {
            const bool failed = it == it0 && l == l0;
            for (int attempt = failed ? 1 : 0; attempt < 2; ++attempt) {
                if (attempt == 1) {
#ifndef QP_PROFILE
                    if (threadIdx.x == 0) S.scalars[(size_t)mission * SC_N + SC_PROF0 + 3] += 1;
#endif
                    restore_dummy(S, mission, l * nbmax, nbmax);
                    __threadfence_block();
                    __syncthreads();
                }
                const double far_R = (attempt == 0 && it == 0 && S.p.polish && S.p.far_slack > 0.0) ? S.p.far_slack : 1e300;
                const int again = uni(qp_batch_body_outofline(Sg, ws_base, ws_stride, mission, l, nbmax, (int)(l == 0), lds_doubles, it, far_R));
                __threadfence_block();
                __syncthreads();
                if (!again) break;
            }
        }
}
