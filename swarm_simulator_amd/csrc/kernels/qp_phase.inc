// qp_phase.inc — the PHASE-SPLIT schedule of the batch QPs (round 5); included by qp.hip inside its anonymous namespace, 256-thread build.
//
// qp_batch_kernel runs a mission's whole Gauss-Seidel schedule on ONE workgroup: its three row sweeps per interior-point iteration
// (a stream over the row state, HBM bound) share a kernel -- registers, LDS, occupancy of two waves per SIMD -- with the dependent chains
// of the knot factorisation, the substitutions and the polish (latency bound).  Here the interior-point iteration is cut at its sweeps:
//
//   ph_advance   one workgroup per mission: everything between two chip-wide sweeps that is a dependent chain or glue -- the
//                wide-neighbourhood test of the step just swept, convergence tests, early / final active-set polish, the end of a batch QP
//                and the set-up of the next one (presolve, row constants, first build sweep), knot assembly, the twisted factorisation,
//                the predictor solve.  A mission runs on until it needs the affine sweep;
//   ph_sweep<P>  the AFFINE, STEP and UPDATE+BUILD sweeps as kernels of their own over ALL missions: a workgroup takes four 64-lane tiles
//                of a batch QP's control points (the sliced-ELLPACK columns of QpWs), no chain code and no LDS work area in the kernel,
//                so it runs at the occupancy its own registers allow; its block reductions go to a small per-mission array of partials,
//                summed in a fixed order by the consumer (bit-reproducible, no floating-point atomics);
//   ph_corr      one workgroup per mission: centring parameter from the affine sweep's partials, corrector right-hand side and solve;
//   ph_ctrl      step length from the step sweep's partials and x += alpha dx (mode 0); the wide-neighbourhood test of an update sweep,
//                with the 0.8-alpha repeat of a refused step (mode 1).
//
// One ROUND = ph_advance, sweep AFF, ph_corr, sweep STEP, ph_ctrl(0), sweep UP, [ph_ctrl(1), sweep UP] x 2.  Every mission carries its own
// state record (phase, batch, pass, iteration, scalars): missions are NOT in lock step across batch boundaries -- a mission whose batch QP
// has converged sets up its next one in the same ph_advance call -- only across the sweeps of a round; kernels skip missions whose
// phase is not theirs.  The host enqueues a fixed budget of rounds (no synchronisation: rbp_session_run stays asynchronous); a mission
// that is finished costs an early exit per launch, one that is not finished when the budget ends fails with RBP_ERR_QP_FAILED (the
// counterpart of QP_MAX_ITERS).  The missions of a session are split over a few streams (groups) whose rounds overlap: while one
// group's chains run, another group's sweeps stream.
//
// Same mathematics, same device functions as qp_batch_kernel (qp.hip); only the reductions over a sweep are summed in a different order.

enum { PH_SETUP = 0, PH_HEAD, PH_AFF, PH_STEP, PH_UP, PH_DONE, PH_FAILED };

struct PhState {
    int phase, batch, pass, iter, early_tries, par /* which (s, z) pair is current */, bt /* repeats of the update sweep */, rounds;
    int frozen_free_rows, pad0, pad1, pad2;
    double gap, pres, mu, sigma_mu, alpha, applied, nrows_free, kkt_ipm;
    double flops, rows_swept, row_bytes, sweep_bytes, bytes_iter, bytes_sweeps;
};
static_assert(sizeof(PhState) <= PH_STATE_DOUBLES * sizeof(double), "PH_STATE_DOUBLES");

__device__ __forceinline__ PhState* ph_state(double* ws_base, size_t ws_stride, size_t st_off, int mission) {
    return (PhState*)(ws_base + (size_t)mission * ws_stride + st_off);
}
__device__ __forceinline__ double* ph_partials(PhState* st) { return (double*)st + PH_STATE_DOUBLES; }  // [workgroup][8]: sum0 sum1 sum2 vmax vmin

// the row context of (mission, batch) -- pointer arithmetic only, recomputed by every kernel instead of being kept in memory
__device__ __forceinline__ void ph_context(const DevSession& S, double* ws_base, size_t ws_stride, int mission, int batch, int nbmax, int lds_doubles,
                                           int par, RowCtx& c, double*& ctrl, const double*& T) {
    const int N = S.N, M = __builtin_amdgcn_readfirstlane(S.Mk[mission]), MS = S.M;
    const int first = batch * nbmax, nb = min(nbmax, N - first);
    c.pw = nullptr;
    c.meta = nullptr;
    c.scal = S.scalars + (size_t)mission * SC_N, c.mission = mission, c.lds_avail = lds_doubles - 32;
    c.d = make_dims(N, M, first, nb);
    c.w = carve(ws_base + (size_t)mission * ws_stride, c.d, nbmax);
    if (par) {
        double* t = c.w.s;
        c.w.s = c.w.s2, c.w.s2 = t;
        t = c.w.z, c.w.z = c.w.z2, c.w.z2 = t;
    }
    ctrl = S.ctrl + (size_t)mission * N * 3 * 6 * MS;
    c.ctrl = ctrl;
    c.normals = S.rsfc_normal + (size_t)mission * S.npair * MS * 3;
    c.radius = S.radius + (size_t)mission * N;
    T = S.T + (size_t)mission * (MS + 1);
}

// x += delta dx over the batch agents' control points (contiguous: [first .. first + nb) x 3 x oq)
__device__ __forceinline__ void ph_move_x(const RowCtx& c, double* ctrl, double delta) {
    double* xb = ctrl + (size_t)c.d.first * 3 * c.d.oq;
    const int nx = c.d.nb * 3 * c.d.oq;
    for (int i0 = threadIdx.x; i0 < nx; i0 += 4 * QP_THREADS) {
        double xv[4], dv4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * QP_THREADS;
            xv[q] = i < nx ? xb[i] : 0.0, dv4[q] = i < nx ? c.w.dx[i] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * QP_THREADS;
            if (i < nx) xb[i] = xv[q] + delta * dv4[q];
        }
    }
}

// wide-neighbourhood test of the update sweep that has just run for this mission (partials of its workgroups).  true: the step stands
// (the new row state becomes the current one, the next iteration's build data are in place); false: x has been moved back to 0.8 alpha
// and the update sweep must run again.
__device__ __forceinline__ bool ph_nbhd_test(PhState& st, const RowCtx& c, double* ctrl, const double* part) {
    const int nwg = ph_nwg(c.d.nb, c.d.M);
    double g = 0, pmax = 0, pmin = 1e300;
    for (int i = 0; i < nwg; ++i) g += part[8 * i], pmax = fmax(pmax, part[8 * i + 3]), pmin = fmin(pmin, part[8 * i + 4]);
    st.rows_swept += st.nrows_free;
    if (pmin >= QP_NBHD_GAMMA * g / st.nrows_free || st.bt >= 39) {
        st.gap = g, st.pres = pmax;
        st.par ^= 1, st.iter += 1, st.bt = 0;
        st.rows_swept += 2 * st.nrows_free;
        st.row_bytes += st.bytes_iter, st.sweep_bytes += st.bytes_sweeps;
        st.phase = PH_HEAD;
        return true;
    }
    const double a_new = 0.8 * st.alpha;
    ph_move_x(c, ctrl, a_new - st.applied);
    st.alpha = a_new, st.applied = a_new, st.bt += 1;
    return false;
}

__global__ __launch_bounds__(256) void ph_init(DevSession S, double* ws_base, size_t ws_stride, size_t st_off) {
    const int mission = blockIdx.x * blockDim.x + threadIdx.x;
    if (mission >= S.K) return;
    PhState* sg = ph_state(ws_base, ws_stride, st_off, mission);
    PhState z = {};
    z.phase = S.status[mission] != 0 ? PH_FAILED : PH_SETUP;
    *sg = z;
}

// missions the round budget did not finish: the counterpart of the interior-point iteration cap
__global__ __launch_bounds__(256) void ph_finish(DevSession S, double* ws_base, size_t ws_stride, size_t st_off) {
    const int mission = blockIdx.x * blockDim.x + threadIdx.x;
    if (mission >= S.K) return;
    PhState* sg = ph_state(ws_base, ws_stride, st_off, mission);
    if (sg->phase < PH_DONE && S.status[mission] == 0) {
        S.status[mission] = (int)RBP_ERR_QP_FAILED;
        double* scal = S.scalars + (size_t)mission * SC_N;
#ifndef QP_PROFILE
        scal[SC_PROF0 + 1] = 1000.0 * sg->batch + 4, scal[SC_PROF0 + 2] = sg->iter;  // why: 4 = the round budget of the phase-split schedule ran out
#endif
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// ph_advance: one workgroup per mission, everything between two chip-wide sweeps
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QP_THREADS, QP_WAVES_PER_EU) void ph_advance(DevSession S, double* ws_base, size_t ws_stride, size_t st_off, int m0, int passes,
                                                                         int biter, int nbmax, int lds_doubles) {
    const int mission = m0 + (int)blockIdx.x, tid = threadIdx.x;
    PhState* sg = ph_state(ws_base, ws_stride, st_off, mission);
    PhState st = *sg;
    st.phase = __builtin_amdgcn_readfirstlane(st.phase);
    if (st.phase >= PH_DONE || st.phase == PH_AFF || st.phase == PH_STEP) return;
    if (S.status[mission] != 0) {  // (failed in an earlier stage or kernel)
        if (tid == 0) sg->phase = PH_FAILED;
        return;
    }
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    double* red = lds_raw;  // 16
    int* flag = (int*)(lds_raw + 16);
    double* lds = lds_raw + 32;
    __shared__ RowCtx c_lds;
    double* scal = S.scalars + (size_t)mission * SC_N;
    st.rounds += 1;
    for (;;) {
        st.batch = __builtin_amdgcn_readfirstlane(st.batch), st.par = __builtin_amdgcn_readfirstlane(st.par);
        RowCtx c;
        c.meta = nullptr;
        double* ctrl;
        const double* T;
        ph_context(S, ws_base, ws_stride, mission, st.batch, nbmax, lds_doubles, st.par, c, ctrl, T);
        const QpDims& d = c.d;
        const QpWs& w = c.w;
        const int M = d.M, first = d.first;
        PassIO io;
        io.mu0 = QP_MU0, io.s_floor = QP_SFLOOR, io.dreg = 1e-9, io.sigma_mu = 0, io.alpha = 0;
        PolishWs pw;
        pw.cand = (Cand*)w.polish;
        pw.V = w.polish + PL_NC * 14;
        pw.Sg = pw.V + (size_t)(PL_NC + 1) * d.nj * d.nk;
        pw.ncand = (int*)(pw.Sg + PL_NC * PL_NC);
        pw.Lbig = pw.Sg + PL_NC * PL_NC + 8;
        bool finished = false, polished = false;
        int fail_reason = 0;
        if (st.phase == PH_SETUP) {
            // ---- a new batch QP: set-up, presolve check, starting point, first build sweep (all on this workgroup: once per batch QP)
            if (d.nb <= 0) {
                st.phase = PH_DONE;
                break;
            }
            int frozen_free_rows = 0, nfar = 0;  // (every row near: the phase split has no second attempt, see QP_FAR_SLACK)
            if (!qp_setup_batch(S, c, ctrl, T, mission, first, d.nb, flag, lds, frozen_free_rows, 1e300, nfar)) {
                st.phase = PH_FAILED;
                break;
            }
            __syncthreads();
            if (tid == 0) c_lds = c;
            __syncthreads();
            io.vmax = 0;
            row_pass<PASS_PRESOLVE>(c, io);
            const double pin_viol = block_reduce(io.vmax, 1, red);
            if (pin_viol > 1e-6) {
                if (tid == 0) {
                    atomicCAS(&S.status[mission], 0, (int)RBP_ERR_QP_FAILED);
#ifndef QP_PROFILE
                    scal[SC_PROF0 + 1] = 1000.0 * st.batch + 1, scal[SC_PROF0 + 2] = pin_viol;  // why: a constant (pinned) row is violated
#endif
                }
                st.phase = PH_FAILED;
                break;
            }
            st.frozen_free_rows = frozen_free_rows;
            st.nrows_free = (double)((size_t)(d.oq - 6) * (6 * d.nb + d.npb)) + (double)frozen_free_rows;  // every pair row once
            const double blk_doubles = d.nk <= 36 ? 7.0 * (d.nk * (d.nk + 1) / 2) + 5.0 * d.nk : 8.0 * d.ldb * d.ldb;  // (see qp_batch_body)
            st.bytes_sweeps = 88.0 * frozen_free_rows + 64.0 * (double)(d.oq - 6) * (6.0 * d.nb + 2.0 * d.npb) + 288.0 * (double)d.nb * (d.oq - 6);
            st.bytes_iter = st.bytes_sweeps + 8.0 * (double)d.nj * blk_doubles;
            st.iter = 0, st.early_tries = 0, st.bt = 0, st.kkt_ipm = 0;
            st.flops = st.rows_swept = st.row_bytes = st.sweep_bytes = 0;
            row_pass<PASS_INIT>(c, io);
            __threadfence_block();
            __syncthreads();
            io.sum0 = 0, io.vmax = 0;
            io = sweep<PASS_BUILD>(&c_lds, io);
            st.gap = block_reduce(io.sum0, 0, red);
            st.pres = block_reduce(io.vmax, 1, red);
            st.phase = PH_HEAD;
        } else if (st.phase == PH_UP) {
            // ---- the update sweep of the last round: does the step stand?
            if (!ph_nbhd_test(st, c, ctrl, ph_partials(sg))) break;  // (x moved back: the next update sweep repeats it)
            continue;                                               // (the row arrays have changed places: new context)
        }
        // ---- PH_HEAD: residuals, termination, polish, or the next Newton system
        if (st.iter >= QP_MAX_ITERS) {
            fail_reason = 3;
        } else {
            __threadfence_block();
            __syncthreads();
            double dmax, gmax;
            rbase_from_acc(c, dmax, gmax);  // rbase = -F'(2Qx + G'z)
            const double dres = block_reduce(dmax, 1, red) / (1.0 + block_reduce(gmax, 1, red));
            const double mu = st.gap / st.nrows_free, pres = st.pres;
            st.mu = mu;
            st.rows_swept += st.nrows_free;
            st.kkt_ipm = fmax(pres, fmax(dres, mu));
            if ((pres < 1e-9 && dres < 1e-9 && mu < 1e-10) || (pres < 1e-6 && dres < 1e-9 && mu < 1e-13) || (pres < 1e-9 && dres < 1e-7 && mu < 1e-14)) {
                finished = true;  // (the three exits of qp_batch_body)
            } else {
                const bool polish_first = st.pass > 0 && st.iter == 0;
                const bool early = st.early_tries < QP_EARLY_TRIES && pres < QP_EARLY_TOL && dres < QP_EARLY_TOL &&
                                   mu < (st.early_tries == 0 ? QP_EARLY_TOL : 1e-2 * QP_EARLY_TOL);
                if (S.p.polish && (polish_first || early)) {
                    if (!polish_first) st.early_tries++;
                    const int acc = polish_entry(c, pw, lds, red, flag, polish_first ? 1 : 0);
                    __syncthreads();
                    if (acc == 0) finished = true, polished = true;
                }
            }
            if (!finished) {
                // ---- Newton matrix, factorisation, predictor
                if (d.nk > 36)
                    assemble_blocks(c, lds);
                else
                    if (!QP_FOLLOW_ASM) assemble_blocks_lds(asm_args(c), d.nj, lds);
                __threadfence_block();
                __syncthreads();
                const BlkArgs ba{d.nk, d.nj, d.ldb, c.lds_avail, w.Td, w.To, w.Lf, w.Ek, nullptr};
                if (!factor_entry(ba, asm_args(c), lds, flag)) {
                    fail_reason = 2;  // Newton matrix not positive definite
                } else {
                    st.flops += d.nk <= 36 ? (double)d.nj * ((7.0 / 6.0) * d.nk * (double)d.nk * d.nk + 6.0 * d.nk * (double)d.nk)
                                           : (double)d.nj * (7.0 / 3.0) * d.nk * (double)d.nk * d.nk;
                    rhs_from_acc(c, false, 0.0);  // rhs = rbase + F'G'v (v from the build sweep)
                    __threadfence_block();
                    __syncthreads();
                    solve_entry(ba, w.rhs, lds);
                    apply_F(d, w, w.rhs, w.dxa);
                    st.phase = PH_AFF;
                    break;
                }
            }
        }
        if (fail_reason) {
            if (tid == 0) {
                atomicCAS(&S.status[mission], 0, (int)RBP_ERR_QP_FAILED);
#ifndef QP_PROFILE
                scal[SC_PROF0 + 1] = 1000.0 * st.batch + fail_reason, scal[SC_PROF0 + 2] = st.iter;  // why: 2 factor, 3 iteration cap
#endif
            }
            st.phase = PH_FAILED;
            break;
        }
        // ---- the batch QP has converged: final polish, objective, diagnostics; then the next batch of the schedule
        if (S.p.polish && !polished) {
            int acc = polish_entry(c, pw, lds, red, flag, 0);
            if (acc == 3) {  // the dual active-set solve ran out of capacity: once more with the big factor in global memory
                __syncthreads();
                acc = polish_entry(c, pw, lds, red, flag, 2);
            }
            polished = acc == 0;
#ifndef QP_PROFILE
            if (acc != 0 && tid == 0) scal[SC_PROF0] += 1000.0 * st.batch + acc;  // diagnostic: which batch was not polished, and why
#endif
            __syncthreads();
        }
        __syncthreads();
        const double kkt = polished ? red[12] : st.kkt_ipm;
        double obj = 0;  // objective of this batch: sum x' Q_p x  (cplex.getObjValue, :164)
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
            if (st.batch == 0) scal[SC_TOTAL_COST] = 0;
            scal[SC_TOTAL_COST] += obj;
            scal[SC_IPM_ITERS] += st.iter;
            scal[SC_QP_SOLVED] += 1;
            scal[SC_POLISHED] += polished ? 1 : 0;
            scal[SC_KKT_MAX] = fmax(scal[SC_KKT_MAX], kkt);
            scal[SC_FLOPS] += st.flops;
            scal[SC_ROWS] += st.rows_swept;
#ifndef QP_LHSTATS
            scal[SC_ROW_BYTES] += st.row_bytes;
            scal[SC_SWEEP_BYTES] += st.sweep_bytes;
#endif
        }
        st.batch += 1, st.par = 0;
        if (st.batch >= biter) st.batch = 0, st.pass += 1;
        st.phase = st.pass >= passes ? PH_DONE : PH_SETUP;
        __threadfence_block();
        __syncthreads();
        if (st.phase == PH_DONE) break;
    }
    __syncthreads();
    if (tid == 0) *sg = st;
}

// ------------------------------------------------------------------------------------------------------------------------
// chip-wide row sweeps: grid (workgroups of a batch QP, missions of the group)
// ------------------------------------------------------------------------------------------------------------------------
#ifndef PH_SWEEP_WAVES
#define PH_SWEEP_WAVES 4  // minimum waves per SIMD the sweep kernels are compiled for
#endif
template <int PASS>
__global__ __launch_bounds__(256, PH_SWEEP_WAVES) void ph_sweep(DevSession S, double* ws_base, size_t ws_stride, size_t st_off, int m0, int nbmax) {
    const int mission = m0 + (int)blockIdx.y;
    PhState* sg = ph_state(ws_base, ws_stride, st_off, mission);
    constexpr int want = PASS == PASS_AFF ? PH_AFF : (PASS == PASS_STEP ? PH_STEP : PH_UP);
    if (__builtin_amdgcn_readfirstlane(sg->phase) != want) return;
    __shared__ RowCtx c_lds;
    __shared__ double red[16];
    RowCtx c;
    c.meta = nullptr;
    double* ctrl;
    const double* T;
    ph_context(S, ws_base, ws_stride, mission, __builtin_amdgcn_readfirstlane(sg->batch), nbmax, 64, __builtin_amdgcn_readfirstlane(sg->par), c, ctrl, T);
    const int wi_begin = (int)blockIdx.x * 256;
    if (wi_begin >= c.d.nb * c.d.oq) return;  // (a short last batch, or a mission with fewer segments than the session's largest)
    if (threadIdx.x == 0) c_lds = c;
    __syncthreads();
    PassIO io;
    io.mu0 = QP_MU0, io.s_floor = QP_SFLOOR, io.dreg = 1e-9, io.sigma_mu = sg->sigma_mu, io.alpha = sg->alpha;
    io.sum0 = io.sum1 = io.sum2 = 0;
    io.vmax = PASS == PASS_AFF ? 1.0 : (PASS == PASS_STEP ? QP_STEP_FRAC : 0.0), io.vmin = 1e300;
    row_pass<PASS>(c_lds, io, wi_begin + (int)threadIdx.x, wi_begin + 256, 256);
    const double s0 = block_reduce(io.sum0, 0, red);
    const double s1 = PASS == PASS_AFF ? block_reduce(io.sum1, 0, red) : 0.0, s2 = PASS == PASS_AFF ? block_reduce(io.sum2, 0, red) : 0.0;
    const double vx = block_reduce(io.vmax, 1, red);
    const double vn = PASS == PASS_UPBUILD ? block_reduce(io.vmin, 2, red) : 1e300;
    if (threadIdx.x == 0) {
        double* p = ph_partials(sg) + 8 * blockIdx.x;
        p[0] = s0, p[1] = s1, p[2] = s2, p[3] = vx, p[4] = vn;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// ph_corr: centring parameter, corrector right-hand side (accumulated by the affine sweep in two parts) and solve
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QP_THREADS, QP_WAVES_PER_EU) void ph_corr(DevSession S, double* ws_base, size_t ws_stride, size_t st_off, int m0, int nbmax,
                                                                      int lds_doubles) {
    const int mission = m0 + (int)blockIdx.x, tid = threadIdx.x;
    PhState* sg = ph_state(ws_base, ws_stride, st_off, mission);
    if (__builtin_amdgcn_readfirstlane(sg->phase) != PH_AFF) return;
    PhState st = *sg;
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    double* lds = lds_raw + 32;
    RowCtx c;
    c.meta = nullptr;
    double* ctrl;
    const double* T;
    ph_context(S, ws_base, ws_stride, mission, __builtin_amdgcn_readfirstlane(st.batch), nbmax, lds_doubles, __builtin_amdgcn_readfirstlane(st.par), c, ctrl, T);
    const QpDims& d = c.d;
    const QpWs& w = c.w;
    const int nwg = ph_nwg(d.nb, d.M);
    const double* part = ph_partials(sg);
    double vmax = 1.0, q0 = 0, q1 = 0, q2 = 0;
    for (int i = 0; i < nwg; ++i) q0 += part[8 * i], q1 += part[8 * i + 1], q2 += part[8 * i + 2], vmax = fmax(vmax, part[8 * i + 3]);
    const double a_aff = 1.0 / vmax;
    const double mu_aff = (q0 + a_aff * q1 + a_aff * a_aff * q2) / st.nrows_free;
    double sigma = mu_aff / st.mu;
    sigma = QP_SIGMA_POW == 2 ? sigma * sigma : (QP_SIGMA_POW == 4 ? sigma * sigma * sigma * sigma : sigma * sigma * sigma);
    st.sigma_mu = sigma * st.mu;
    rhs_from_acc(c, true, st.sigma_mu);
    __threadfence_block();
    __syncthreads();
    const BlkArgs ba{d.nk, d.nj, d.ldb, c.lds_avail, w.Td, w.To, w.Lf, w.Ek, nullptr};
    solve_entry(ba, w.rhs, lds);
    apply_F(d, w, w.rhs, w.dx);
    st.flops += 2.0 * d.nj * 4.0 * d.nk * (double)d.nk;
    st.phase = PH_STEP;
    __syncthreads();
    if (tid == 0) *sg = st;
}

// ------------------------------------------------------------------------------------------------------------------------
// ph_ctrl: mode 0 = step length and x += alpha dx after the step sweep; mode 1 = wide-neighbourhood test after an update sweep
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QP_THREADS) void ph_ctrl(DevSession S, double* ws_base, size_t ws_stride, size_t st_off, int m0, int nbmax, int mode) {
    const int mission = m0 + (int)blockIdx.x, tid = threadIdx.x;
    PhState* sg = ph_state(ws_base, ws_stride, st_off, mission);
    const int phase = __builtin_amdgcn_readfirstlane(sg->phase);
    if (phase != (mode == 0 ? PH_STEP : PH_UP)) return;
    PhState st = *sg;
    RowCtx c;
    c.meta = nullptr;
    double* ctrl;
    const double* T;
    ph_context(S, ws_base, ws_stride, mission, __builtin_amdgcn_readfirstlane(st.batch), nbmax, 64, __builtin_amdgcn_readfirstlane(st.par), c, ctrl, T);
    if (mode == 0) {
        const int nwg = ph_nwg(c.d.nb, c.d.M);
        const double* part = ph_partials(sg);
        double vmax = QP_STEP_FRAC;  // alpha = min(1, frac * min -x/d) = frac / max(frac, max -d/x)
        for (int i = 0; i < nwg; ++i) vmax = fmax(vmax, part[8 * i + 3]);
        st.alpha = QP_STEP_FRAC / vmax;
        ph_move_x(c, ctrl, st.alpha);
        st.applied = st.alpha, st.bt = 0;
        st.phase = PH_UP;
    } else {
        (void)ph_nbhd_test(st, c, ctrl, ph_partials(sg));
    }
    __syncthreads();
    if (tid == 0) *sg = st;
}
