// qp.hip — the batched RBP QP on gfx950: assembly, interior-point solve, active-set polish.
//
// Replaces the QP of RBPPlanner::update (reference: swarm_planner/include/rbp_planner.hpp:33-84): buildConstMtx :100-109,
// populatebyrow :551-688, cplex.solve() :158.  build_dummy in front of it and the Bernstein->monomial loop and timeScale behind it are
// kernels/traj.hip.
//
// Formulation (DESIGN.md "QP"): the equality rows of Aeq_base (:353-405) are C2 continuity at the knots plus the
// pinned end states, so per (agent, dim) and interior knot j the three control points right of the knot are free
// (u_j) and the three left of it are L_j u_j.  In these coordinates the batch QP has NO equality rows, every
// inequality row (SFC bound :626-635, RSFC :638-684) touches exactly one knot, and the Newton matrix of a
// primal-dual interior-point method, F'(2Q)F + J' W J, is block tridiagonal over the M-1 knots with dense
// blocks of order nk = 9 * (batch agents).  One workgroup runs one mission's whole batch schedule in one launch:
//   * three row sweeps per interior-point iteration stream the row state -- (s, z) only, in sliced-ELLPACK order: one coalesced
//     512-byte access per wavefront and array, see QpWs -- from HBM (affine sweep incl. both parts of the corrector rhs; step
//     sweep; step into the ping-pong arrays + neighbourhood test + next iteration's weights);
//   * per-control-point 3x3 accumulators are expanded into the knot blocks (no atomics) by the six waves that would otherwise
//     idle behind the factorisation chains, block by block just ahead of them (twisted_factor);
//   * the block-tridiagonal factorisation: nk <= 36 twisted two-wave chains, L D L' with column images broadcast through LDS (36 x 36
//     blocks: 4-column panels on the FP64 MFMA, knot_lds.inc), the explicit inverse factor M = L^-T by a companion wave, MFMA rank-k updates; wider batches an MFMA-tiled path
//     (LDS-resident for nk <= 72); substitutions as matrix-vector products with the staged M;
//   * an active-set polish (qp_polish.inc) turns the interior-point answer into the exact optimum, verified by a full
//     KKT check; from the second Gauss-Seidel pass on it is tried before any interior-point iteration.
// Batches of a mission are solved strictly in the reference's order (Gauss-Seidel, :140-148); parallelism comes
// from the 3*nb coupled blocks inside a batch and from the K missions of a session.  The file is compiled twice
// (512 / 256 threads per workgroup, see the note above planner_workspace_bytes).  Workspace, reductions and
// the wave-uniform arguments are qp_base.inc, the row sweeps qp_rows.inc, right-hand sides and knot-block assembly qp_newton.inc, the
// wave-register path qp_wave_factor.inc / qp_wave_solve.inc, the tiled path qp_tiled.inc, the factor / solve entries qp_entries.inc, the
// polish qp_polish_types.inc (its records) / qp_polish.inc, the batch driver qp_batch.inc: each included once, in dependency order.  This
// file keeps the levers, the kernels and the launch.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "rbp_dev.h"

// The QP is tolerance-judged floating point: allow FMA contraction here (the Makefile disables it globally because
// corridor.hip must round exactly like the reference's float32 code).
#pragma clang fp contract(fast)

#include "knot_lds.inc"  // (below the pragma: its multiply-adds must contract)
#include "common/ipm_rows.h"  // the arithmetic of a row, shared with jqp.hip
#include "common/reduce_order.h"  // the order of operations of a workgroup-wide reduction, shared with its host restatement

#ifndef QP_THREADS
#define QP_THREADS 512
#endif
// QP_MAX_NB (rbp_dev.h): nk <= 36: wave-register path; wider: MFMA-tiled path (blocks in LDS up to nk = 72, else global)
#define QP_MAX_ITERS 80
#ifndef QP_WARM_TAU
#define QP_WARM_TAU 1e-3  // polish-first (Gauss-Seidel passes >= 2): rows closer than this to their bound are candidates
#endif
#ifndef QP_MU0
#define QP_MU0 3e-1     // interior-point start: z = mu0 / s with s = max(slack, s_floor)  (tuned on the 50-map sweep)
#endif
#ifndef QP_ROW_UNROLL  // frozen-row stream of a sweep: rows unrolled per thread.  A/B on one box (r03, 2000 missions resident): 1: 82.8 k,
#define QP_ROW_UNROLL 2  // 2: 86.0 k, 4: 78.8 k agent-trajectories/s
#endif
#ifndef QP_ROW_PF
#define QP_ROW_PF 0  // prefetch distance (rows) of the frozen-row stream; 0 = plain loop unrolled QP_ROW_UNROLL times
#endif
#ifndef QP_ROW_BLK
#define QP_ROW_BLK (QP_THREADS >= 512 ? 0 : 4)  // (round 6) frozen-row stream in BLOCKS of this many rows whose loads are issued a block ahead (see row_pass); 0 = off.
                                             // The 256-thread build (missions that share the memory system with 511 others); A/B 3 / 4 / 5 / 6: 4
#endif
// a generic pointer into the workspace as the GLOBAL pointer it is: loads / stores through it are global_* instructions (one memory counter,
// counted in order) instead of flat_* (both counters, and the compiler waits for every outstanding access at the first use of any)
#define QG(p) ((__attribute__((address_space(1))) double*)(p))
#define QGC(p) ((__attribute__((address_space(1))) const double*)(p))
#define QGF(p) ((__attribute__((address_space(1))) const float*)(p))
#ifndef QP_FAR_SLACK
// REDUCED ROW SET of the interior-point phase (round 5).  A frozen-neighbour row whose slack at the batch QP's starting point exceeds this
// many metres for all six control points of its (agent, segment) group is FAR: the interior-point sweeps do not walk it (no (s, z), no
// weight, no ratio test).  Correctness does not depend on the choice: the active-set polish verifies EVERY row of the full QP at the point it
// proposes (far rows that come out violated join the candidates and the dual is solved again), and a batch QP whose polish is refused -- or
// whose interior-point method fails -- while far rows exist is solved again from its starting point with every row near.  Applies to the
// first Gauss-Seidel pass of the sequential schedule with the polish on.  The value travels in rbp_solver_opts.qp_far_slack (DevParam::far_slack);
// this is its default (abi/session.hip rbp_solver_opts_defaults).
#define QP_FAR_SLACK 0.7  // (A/B on one box, 2000 missions resident: off 100.1 k, 1.0 m 123.2 k, 0.7 m 127.7 k, 0.5 m 127.2 k agent-trajectories/s;
                          // batch QPs solved twice on the 50-map sweep: 0 / 1 / 8 of 800; 0.25 m costs iterations: profiles/r05_ab_reduced_rows.txt)
#endif
#ifndef QP_SIGMA_POW
#define QP_SIGMA_POW 3  // Mehrotra's centring exponent
#endif
#ifndef QP_NBHD_GAMMA
#define QP_NBHD_GAMMA 1e-3  // wide neighbourhood: no complementarity product below gamma * mu
#endif
#ifndef QP_NBHD_BACKOFF
#define QP_NBHD_BACKOFF 0.8  // a step the wide-neighbourhood test refuses is repeated with this fraction of its length
#endif
#ifndef QP_STEP_FRAC
#define QP_STEP_FRAC 0.997  // fraction of the step to the boundary (A/B on one box: 0.98 +5 %, 0.99 +1.4 %, 0.997 and 0.999 best, 0.9999 +20 % time)
#endif
#ifndef QP_SFLOOR
#define QP_SFLOOR 1e-1
#endif
#ifndef QP_WAVES_PER_EU
#define QP_WAVES_PER_EU 2  // 256 VGPRs per lane in both builds (one 512-thread or two 256-thread workgroups per CU)
#endif
#ifndef QP_CHAIN_PRIO
#define QP_CHAIN_PRIO 3  // s_setprio level of the waves that run a dependent chain (factor, substitutions, dual active-set solve)
#endif
#ifndef QP_STAGE_BUFS
#define QP_STAGE_BUFS (QP_THREADS >= 512 ? 3 : 2)  // (the 256-thread build shares a CU's LDS between two workgroups)
#endif
#ifndef QP_STAGE_REGS
#define QP_STAGE_REGS (QP_THREADS >= 512 ? 0 : 2)  // register sets of a staging thread whose loads stay in flight across step barriers (solve_staged; 0 = load and store within one step): the 256-thread build, whose missions share the memory system with 511 others
#endif
#ifndef QP_MID_FOLLOW
#define QP_MID_FOLLOW (QP_THREADS >= 512)  // see wave_factor_mid
#endif
// The knots' inverse factors M_j in global memory as contiguous triangles (knot_factor_layout.h), fetched by the staging threads of the
// substitutions as runs of 16-byte pairs; 0 = the square image [NK][NK] fetched 8 bytes at a time, the parent of the A/B in
// profiles/packed_m_ab.txt (one tree builds both sides).
// The 256-thread build, whose missions share the memory system with 511 others: planner stage at 2000 missions 607.9 -> 585.3 ms in every one
// of three passes, 200 GB fewer bytes fetched per launch.  One mission alone on the 512-thread build has no such pressure and measured 0.6 ms
// (0.8 %) SLOWER with the packed layout in every pass: that build keeps the square.  (A factor is written and read inside one launch of one
// build, so the two need not agree.)
#ifndef QP_LF_PACKED
#define QP_LF_PACKED (QP_THREADS >= 512 ? 0 : 1)
#endif
// (A second lever, QP_STAGE_EARLY -- the loads of a substitution's first stage(s) issued at the entry of solve_staged, ahead of the
// right-hand side's, instead of behind the zero-fill barrier -- was built and measured with this one: no gain alone, 1.1 .. 1.7 ms slower on
// top of the packed layout in every one of three passes (profiles/packed_m_ab.txt).  Its code is not kept.)
// The predictor's forward substitution carried along the factorisation (blocks on the fused path, i.e. of order 36): a chain wave takes the
// forward step of the block it has just factorised out of its own LDS area -- M_jp in MX, 1 / d_jp in I -- between the update of the next
// block and the wait for that block's image, the middle block's step follows its factorisation, and the predictor's solve_staged runs the
// backward steps only (SolveOut::rhs_mode 3): 18 of its 35 step barriers and one of the four stagings of every M_j go.  kl_forward_step
// (knot_lds.inc) has the details.  A/B against the parent on one box, builds alternating (profiles/fwd_in_factor_ab.txt): planner stage at
// 2000 missions 615.7 -> 608.4 ms in every one of three passes, one mission alone 77.07 -> 75.26 ms, the 50-mission sweep 103.1 -> 102.0 ms,
// control points bit for bit the same.  The chain timers say the step does NOT hide in the wait for the image (3.4 us per step under load,
// mostly waiting for its own four global loads): the gain is what the solve loses.  The trace build compares the right-hand sides of the
// full substitution: off there.
#ifndef QP_FWD_IN_FACTOR
#ifdef QP_TRACE
#define QP_FWD_IN_FACTOR 0
#else
#define QP_FWD_IN_FACTOR 1  // both builds: profiles/fwd_in_factor_ab.txt
#endif
#endif
#if QP_FWD_IN_FACTOR && KL_FUSED_UPDATE && KL_PANEL && KL_PANEL_MIN_NK <= 36  // (kl_fused_path(36) for the preprocessor: the lever's lines of the kernel body)
#define QP_FWD36 1
#else
#define QP_FWD36 0
#endif
#ifndef QP_EARLY_TRIES
#define QP_EARLY_TRIES 2
#endif
#ifndef QP_EARLY_TOL
#define QP_EARLY_TOL 1e-6
#endif
// LDS doubles used by polish_qp: 2 blocks + packed factor + vectors + int arrays (see qp_polish.inc)
#include "lh_layout.h"
#include "knot_factor_layout.h"  // QpWs::Lf: a knot's M_j and 1 / d_j as one contiguous run
#define PL_NC 256   // polish: candidate rows
#define PL_PMAX 160  // polish: rows simultaneously active in the dual solve (wide batches; 112 on the wave path, whose
                     // workgroups are meant to share a CU's LDS in pairs)
#define PL_PBIG 192  // second attempt of a polish whose dual solve ran out of capacity: factor in global memory (rare: ~1 batch QP in 800)
__host__ __device__ inline int polish_pmax(int nk) { return nk <= 36 ? 112 : PL_PMAX; }
// polish workspace.  Per mission (mission_tables): the factor of K0 (18 nj, then its failure flag) and the table of K0^-1; per batch QP:
// cand, S, counters, big factor, the primal step's table of active rows (an entry per row, agent and axis: four doubles), and last the
// gradient column v0 with the gradient and the primal step's right-hand side behind it, the only part that depends on the batch's nk.  (S also lends its storage to mission_tables: low halves of the table.)
__host__ __device__ inline size_t polish_s_doubles(int nj) { return std::max((size_t)PL_NC * PL_NC, ipm::k0g_doubles(nj)); }
__host__ __device__ inline size_t polish_ws_doubles(int nj, int nk) {
    return 18 * (size_t)nj + 2 + ipm::k0g_doubles(nj) + PL_NC * 14 + polish_s_doubles(nj) + 8 + lhp_size(PL_PBIG) + 4 * 6 * PL_PBIG + 3 * (size_t)nj * nk;
}
__host__ __device__ inline int polish_lds_doubles(int nk) {
    const int pm = polish_pmax(nk);
    return lhp_size(pm) + 3 * PL_NC + 3 * pm + (pm + 2 * PL_NC + 8) / 2 + 8;
}

namespace {
using namespace ipm;

#include "qp_base.inc"          // timers, QpDims / QpWs, reductions, wave-uniform arguments, mission constants
#include "qp_polish_types.inc"  // the polish's records, as far as the sweeps emit them
#include "qp_rows.inc"          // the row sweeps: passes, row context, row_op, row_pass with its three frozen-row streams, sweep<PASS>
#include "qp_newton.inc"        // control-space <-> reduced-space maps, right-hand sides, knot-block assembly
#include "qp_wave_factor.inc"   // nk <= 36: twisted factorisation in wave registers
#include "qp_wave_solve.inc"    // nk <= 36: staged substitutions
#include "qp_tiled.inc"         // nk > 36: factorisation and substitutions on MFMA tiles, the blocks' identity padding
#include "qp_entries.inc"       // factor_entry / solve_entry: the stand-alone functions per role of a wave
#include "qp_polish.inc"        // the active-set polish: the algorithms (its records: qp_polish_types.inc, ahead of the sweeps)
#include "qp_batch.inc"         // the batch driver: set-up, interior-point loop, mission tables, the out-of-line rest of a schedule

// One workgroup per mission runs the WHOLE Gauss-Seidel schedule of solveQP (rbp_planner.hpp:140-203: `passes` sweeps
// over `biter` batches) in one launch: missions are independent, so nothing forces them to wait for each other at batch
// boundaries (a launch per batch costs the sum over batches of the slowest mission's interior-point iteration count),
// and with more missions than CUs the hardware dispatcher balances them.
__global__ __launch_bounds__(QP_THREADS, QP_WAVES_PER_EU) void qp_batch_kernel(DevSession S, double* ws_base, size_t ws_stride, int passes,
                                                               int biter, int nbmax, int lds_doubles) {
    // longest missions of the previous run first (DevSession::qp_order): with more missions than resident workgroups the step ends when
    // the last mission does, and a long one started late leaves most of the chip idle behind it
    const int mission = S.qp_order ? __builtin_amdgcn_readfirstlane(S.qp_order[blockIdx.x]) : (int)blockIdx.x;
    const long long t_start = wall_clock64();
    // First Gauss-Seidel pass, polish on: the interior-point phase works on the reduced row set (QP_FAR_SLACK).  A batch QP that does not end
    // polished that way is solved again from its starting point -- the reference's dummy control points -- with every row: rare (1 of the 800
    // batch QPs of the 50-map sweep at 0.7 m).  The batch loop itself holds NO call: when a first attempt fails the loop stops, and the rest
    // of the mission's schedule -- that batch again with every row, then the remaining batches and passes -- runs out of line in
    // qp_finish_schedule, a stand-alone copy of the body, after the loops.  Measured, 2000 missions resident (profiles/r05_ab_reduced_rows.txt):
    // this 133.8 k agent-trajectories/s; a second attempt called from INSIDE the loop 127.7 .. 129.6 k (state kept across the call site,
    // whichever way the session struct travels), a loop of two attempts around the inlined body ~123 k, a "redo" trip through the batch loop 87 k.
    __shared__ DevSession S_lds;  // (for mission_tables and qp_finish_schedule)
    if (threadIdx.x == 0) S_lds = S;
    __syncthreads();
    mission_tables(&S_lds, ws_base, ws_stride, mission, nbmax);
    int stop_it = -1, stop_l = 0;
    for (int it = 0; it < passes && stop_it < 0; ++it)
        for (int l = 0; l < biter; ++l) {
            const double far_R = (it == 0 && S.p.polish && S.p.far_slack > 0.0) ? S.p.far_slack : 1e300;
            const int again = qp_batch_body(S, ws_base, ws_stride, mission, l, nbmax, (int)(l == 0), lds_doubles, it, far_R);
            __threadfence_block();
            __syncthreads();
            if (again) {
                stop_it = it, stop_l = l;
                break;
            }
        }
    if (stop_it >= 0) qp_finish_schedule(&S_lds, ws_base, ws_stride, mission, passes, biter, nbmax, lds_doubles, stop_it, stop_l);
    if (S.qp_cost && threadIdx.x == 0) S.qp_cost[mission] = (unsigned long long)(wall_clock64() - t_start) + 1;
}

// rank of every mission by the previous run's cost, longest first (ties by index); identity while any mission has no cost yet
__global__ __launch_bounds__(256) void qp_order_kernel(DevSession S) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= S.K) return;
    const unsigned long long c = S.qp_cost[k];
    int rank = 0;
    bool valid = c != 0;
    for (int o = 0; o < S.K; ++o) {
        const unsigned long long co = S.qp_cost[o];
        valid = valid && co != 0;
        rank += (co > c || (co == c && o < k)) ? 1 : 0;
    }
    // (valid is the same for every thread: each of them has looked at all costs)
    if (valid)
        S.qp_order[rank] = k;
    else
        S.qp_order[k] = k;
}

}  // namespace

// This file is compiled twice (csrc/Makefile), both with 256 VGPRs per lane: QP_THREADS=512 (one workgroup per CU: the fastest single
// mission, its sweeps prefetch four rows ahead) and QP_THREADS=256 (two workgroups per CU: the throughput build, used when there are
// more missions than CUs).  QP_SUFFIX names the entry points; abi/session.hip picks one per launch.
#ifndef QP_SUFFIX
#define QP_SUFFIX _w2
#endif
#define QP_CAT2(a, b) a##b
#define QP_CAT(a, b) QP_CAT2(a, b)
size_t QP_CAT(planner_workspace_bytes, QP_SUFFIX)(int N, int M, int batch_size_eff) {
    return (ws_doubles(N, M, batch_size_eff) * sizeof(double) + 255) & ~size_t(255);
}

// dynamic LDS of the QP kernels: the largest of the tiled path's vectors, the polish (dual factor + 3x3 chain factor) and the wave
// path's staged substitutions (a short last batch may take the wave path even when bs > 4)
static size_t qp_lds_bytes(int bs, int M) {
    const int nk = 9 * bs;
    const int nkw = std::min(nk, 36);
    size_t lds = sizeof(double) * (2 * (size_t)((nk + 15) & ~15) + QP_THREADS + 32) + 16;
    lds = std::max(lds, sizeof(double) * (size_t)(std::max(polish_lds_doubles(nk), polish_lds_doubles(nkw)) + 18 * (M - 1) + 32) + 16);
    lds = std::max(lds, sizeof(double) * (size_t)(54 * (M - 1) + 32) + 16);  // k0_mission_tables: the factor in double and in dd
    lds = std::max(lds, sizeof(double) * (16 + (size_t)QP_STAGE_BUFS * 2 * (nkw * KL_LD + KL_I) + (size_t)(M - 1) * nkw + 2 + 6 * KS_VLEN + 2 * 64 + 64));  // solve_staged
    // chain areas + assembly progress counters (+ the assembling waves' LDS scratch in the 512-thread build)
    // (256-thread build: the two companion waves' images of the just-in-time assembly)
    lds = std::max(lds, sizeof(double) * (size_t)(2 * kl_area_doubles(nkw) + 128 + (QP_FOLLOW_ASM ? 2 : ASM_HELPERS) * ASML_DOUBLES(nkw, nkw / 9) + 32) + 16);
    if (nk > 36 && nk <= 72) {  // LDS-resident tiled path: three blocks of a knot (leading dimension + 2)
        const size_t lb = (size_t)((nk + 15) & ~15);
        lds = std::max(lds, sizeof(double) * (3 * lb * (lb + 2) + 34) + 16);
    }
    return lds;
}

void QP_CAT(launch_planner, QP_SUFFIX)(const DevSession& s, void* qp_ws, size_t ws_bytes_per_mission, hipStream_t st) {
    const int M = s.M;  // the slot stride (largest M of the session)
    const BatchSchedule sched = batch_schedule(s.p.sequential, s.p.batch_size, s.p.batch_iter, s.N);
    const int bs = sched.bs, biter = sched.biter;
    launch_planner_prologue(s, st);
    if (biter > 0) {
        if (bs > QP_MAX_NB) {
            // a batch wider than QP_MAX_NB agents (nk > 576: the joint QP of a mission with more than 64 agents) is refused by
            // rbp_session_run before any launch (abi/session.hip); reaching this line is an internal error
            (void)rbp_set_error(RBP_ERR_BAD_ARGUMENT, "launch_planner: batch wider than the QP kernel supports");
            return;
        }
        const size_t lds = qp_lds_bytes(bs, M);
        (void)hipFuncSetAttribute((const void*)qp_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (s.p.iteration > 0 && s.qp_order) hipLaunchKernelGGL(qp_order_kernel, dim3((s.K + 255) / 256), dim3(256), 0, st, s);
        if (s.p.iteration > 0)
            hipLaunchKernelGGL(qp_batch_kernel, dim3(s.K), dim3(QP_THREADS), lds, st, s, (double*)qp_ws,
                               ws_bytes_per_mission / sizeof(double), s.p.iteration, biter, bs, (int)(lds / sizeof(double)) - 2);
    }
#ifdef QP_TRACE
    return;  // the coef slot holds the trace
#endif
    launch_planner_epilogue(s, st);
}
