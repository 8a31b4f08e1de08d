// qp_wave_factor.inc — the wave-register path (nk <= 36), factorisation: the twisted block-tridiagonal L D L' of two chain waves, their
// companions (M = L^-T) and the waves that assemble the knot blocks just in time (twisted_factor).  Included by qp.hip behind
// qp_newton.inc, whose knot-block assembly it needs (AsmArgs, ASML_DOUBLES, assemble_knots_lds, fasm_fetch / fasm_tiles); from qp.hip the
// levers (QP_THREADS, QP_MID_FOLLOW, QP_CHAIN_PRIO) and QG / QGC; fast_rsqrt (qp_rows.inc); QpDims, QpWs, rl (qp_base.inc); kl_*, KL_*,
// KlPanels (knot_lds.inc).

// ------------------------------------------------------------------------------------------------------------
// wave-register path (nk <= 36, i.e. batches of up to 4 agents): the whole block-tridiagonal Cholesky and the
// substitutions run in ONE wavefront with matrix rows held in VGPRs (lane r = row r, NK doubles per block) and
// v_readlane broadcasts instead of LDS traffic: every step of the dependent chains costs a few issue cycles
// instead of an LDS round trip, and no workgroup barrier is needed inside a knot.
// (Round 3: the cross-lane traffic of the factorisation goes through LDS broadcasts instead, see knot_lds.inc; v_readlane is
// left for the pivots.)  The substitutions stage the knots' M_j through LDS (prefetched by the otherwise idle waves).
// ------------------------------------------------------------------------------------------------------------
// TWISTED ("burn at both ends") factorisation: wave 0 eliminates blocks 0 .. mid-1 upwards, wave 1 eliminates blocks
// nj-1 .. mid+1 downwards, concurrently on two SIMDs; the middle block collects both Schur complements.  It halves the
// length of the dependent chain (factor and substitutions alike) at no extra arithmetic.
//   Lf[j] = M_j = L_j^-T (the rows' triangle as one contiguous run), then 1 / d_j   (knot_factor_layout.h; KF_SLOT doubles per knot)
__device__ __forceinline__ int twist_mid(int nj) { return nj / 2; }

// Progress counters of the just-in-time block assembly (LDS ints behind the two chain areas): cnt[i] counts the helper waves that
// have finished the blocks of chain step i; a chain may load its i-th block when all QP_THREADS/64 - 2 of them have.
// Wave roles of the wave path's factorisation: 0, 1 = the two chains; 2, 3 = their companions (M = L^-T behind the chain, see
// wave_factor_follow); the 512-thread build has four more waves, which assemble the knot blocks behind the chains (one wave per block,
// through the LDS: assemble_knots_lds); the 256-thread build assembles all blocks up front (assemble_blocks_lds).
#define ASM_WAVE0 4                                                        // first assembling wave
#define ASM_HELPERS (QP_THREADS / 64 > ASM_WAVE0 ? QP_THREADS / 64 - ASM_WAVE0 : 0)   // assembling waves
// (round 6) 256-thread build: no waves to spare for the assembly -- but the two COMPANION waves (M = L^-T behind the chains) idle between
// the end of one block's factorisation and the start of the next (while the chain forms the coupling rows and the rank-36 update): each
// assembles its chain's NEXT block into an LDS image in that gap, just in time, and the chain reads it from there (the Timg path of the
// 512-thread build).  The up-front assembly phase -- 11 % of a mission's time under load, most of it spent waiting for its own loads and
// stores: profiles/r06_ab_qp_levers.txt -- and the round trip of every T_j through global memory disappear.
#ifndef QP_FOLLOW_ASM
#define QP_FOLLOW_ASM (ASM_HELPERS == 0)
#endif
#define ASMF_READY(cnt, h) ((kl_ldsi*)((cnt) + 76 + (h)))  // images the companion of chain h has finished (monotone over a factorisation)
__device__ __forceinline__ void wait_blocks(int* cnt, int i) {
    while (__hip_atomic_load(cnt + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < ASM_HELPERS) __builtin_amdgcn_s_sleep(2);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

typedef double d4 __attribute__((ext_vector_type(4)));

template <int NK>
__device__ __forceinline__ bool chol_rows(double (&a)[NK], double& dinv) {  // right-looking; a[c] = L[r][c] for lanes r >= c
    bool ok = true;                                                           // dinv: 1 / L[r][r] of this lane's row (tiled path)
    const int r = threadIdx.x & 63;
    dinv = 1.0;
#pragma unroll
    for (int c = 0; c < NK; ++c) {
        const double dcc = rl(a[c], c);
        if (!(dcc > 0)) ok = false;
        const double inv = fast_rsqrt(dcc);
        dinv = (r == c) ? inv : dinv;
        a[c] *= inv;
#pragma unroll
        for (int k = c + 1; k < NK; ++k) a[k] -= a[c] * rl(a[c], k);
    }
    return ok;
}

// ---- one chain of the twisted factorisation (round 3: knot_lds.inc, cross-lane traffic through LDS broadcasts) --------------------
// Per knot j of the chain (the chain's previous knot jp = j - dir):
//   S_j = T_j - X_j D_jp^-1 X_j'          X_j = T_{j,jp} L_jp^-T  (rows of block j), the rank-NK update on v_mfma_f64_16x16x4_f64
//   S_j = L_j D_j L_j'                    kl_ldl: column images in LDS; NK = 36: kl_ldl_panels, 4 columns per step on the FP64 MFMA, panel images in LDS
//   M_j = L_j^-T                          explicit (kl_inverse_rows): the substitutions are matrix-vector products with M_j, and
//   X_jn = Cpl M_j                        the coupling factor towards the next knot costs three multiply-adds per entry
// What a knot leaves in global memory for the substitutions is M_j (row r contiguous, entries k < r are zeros) and 1 / d_j: 5.5 KB of
// triangle + diagonal instead of the two full blocks (L_j, X_j: 20.7 KB) of the round-2 formulation; X never leaves the LDS.
// The 36 x 36 blocks (kl_fused_path(NK)) do not store X at all: the chain forms S_j in the MFMA tiles straight from M_jp (kl_fused_update), each
// operand element of X_j from three rows of M_jp and the knot's nine coupling coefficients, and the companion announces M_j before its read-back.
// A knot's slot in QpWs::Lf (knot_factor_layout.h): the rows of M_j from the diagonal on (even NK: from the even column at or left of it, the
// companion's 16-byte stores) one behind the other, then 1 / d_j -- 45 lines of 128 bytes for a 36 x 36 knot, which the staging threads of the
// substitutions fetch as one run of 16-byte pairs, where the square image [NK][NK] spread the same triangle over 65 .. 69 lines (HBM moves
// whole lines) and was fetched 8 bytes at a time.  QP_LF_PACKED = 0 keeps the square for the A/B (profiles/packed_m_ab.txt).
#if QP_LF_PACKED
#define KF_SLOT(NK) kf_stride(NK)           // doubles per knot
#define KF_ELEM(NK, r, k) kf_elem(NK, r, k)  // M_j[r][k]
#define KF_DINV(NK) kf_dinv(NK)             // 1 / d_j
#else
static_assert(KL_I == 40, "kf_sq_stride (knot_factor_layout.h) restates KL_I");
#define KF_SLOT(NK) kf_sq_stride(NK)
#define KF_ELEM(NK, r, k) kf_sq_elem(NK, r, k)
#define KF_DINV(NK) kf_sq_dinv(NK)
#endif
static_assert(KF_SLOT(9) + 15 <= 2 * 81 && KF_SLOT(18) + 15 <= 2 * 324 && KF_SLOT(27) + 15 <= 2 * 729 && KF_SLOT(36) + 15 <= 2 * 1296,
              "a knot's slot and the doubles in front of the first one fit the region carve() gives QpWs::Lf");

// coefficients of row rr of the coupling block between knot j and the next knot of the chain: T_{j+dir,j}[rr][3g + q], g = rr / 3
// (T_{j+1,j} = blockdiag(E_{knot j+1}'), T_{j-1,j} = T_{j,j-1}'; see assemble_blocks)
__device__ __forceinline__ void coupling_coef(const QpWs& w, int j, int dir, int rr, double& e0, double& e1, double& e2) {
    // (a GLOBAL load, not a flat one: a flat load also counts on the LDS counter, and the chain's next wait for its own LDS traffic would
    // wait for this trip to memory as well -- the very latency the early issue is meant to hide)
    const __attribute__((address_space(1))) double* E = QGC(w.Ek) + 9 * (dir > 0 ? j + 1 : j);
    e0 = dir > 0 ? E[rr % 3] : E[3 * (rr % 3)], e1 = dir > 0 ? E[3 + rr % 3] : E[3 * (rr % 3) + 1],
    e2 = dir > 0 ? E[6 + rr % 3] : E[3 * (rr % 3) + 2];
}

// the diagonal block of one knot: S = T_j (- U) into registers, factorised (1 / d in I; in C the column images of kl_ldl or, for the blocks
// on the panel path -- kl_panel_path(NK), the 36 x 36 blocks --, the panel images of kl_ldl_panels); P / pbase: see kl_ldl / kl_ldl_panels.
// Timg != nullptr (512-thread build): T_j is read from the assembling wave's LDS image instead of global memory -- the block never leaves
// the CU, and the chain does not start every knot with a trip to memory --; when the values have arrived *consumed = consumed_value
// tells the assembling wave that it may overwrite the image.
template <int NK>
__device__ __forceinline__ bool knot_ldl(const QpWs& w, int j, bool minus_u, kl_lds* base, int r, bool act, int rr, kl_ldsi* P, int pbase,
                                         const kl_lds* Timg = nullptr, kl_ldsi* consumed = nullptr, int consumed_value = 0) {
    using A = KlArea<NK>;
    kl_lds *C = base + A::C, *I = base + A::I, *U = base + A::C;
    if constexpr (kl_panel_path(NK)) {  // S straight into the MFMA tiles of the panel-blocked factorisation (knot_lds.inc, kl_knot_panels)
        if (Timg)
            return kl_knot_panels<NK, true>([&](int mx, int mn) { return (double)Timg[mn * KL_LD + mx]; },  // (the images hold both triangles)
                                      [&] {
                                          kl_sync();
                                          if (consumed) kl_publish(consumed, consumed_value);
                                      },
                                      minus_u, C, I, r, P, pbase);
        const double* Tg = w.Td + (size_t)j * NK * NK;
        return kl_knot_panels<NK, false>([&](int mx, int mn) { return Tg[mn * NK + mx]; }, [] {}, minus_u, C, I, r, P, pbase);
    }
    double a[NK];
    if (Timg) {
#pragma unroll
        for (int k = 0; k < NK; ++k) a[k] = Timg[k * KL_LD + rr];
        kl_sync();
        if (consumed) kl_publish(consumed, consumed_value);
    } else {
        const double* Tg = w.Td + (size_t)j * NK * NK;
        // T is symmetric: column access = row access; only k <= r was assembled and is used, but whole rows are fetched
#pragma unroll
        for (int k = 0; k < NK; ++k) a[k] = Tg[k * NK + rr];
    }
    if (minus_u) {
#pragma unroll
        for (int k = 0; k < NK; ++k) a[k] -= U[rr * KL_LDU + k];
        kl_sync();
    }
    return kl_ldl<NK>(a, C, I, r, act, P, pbase);
}

// The fused path (kl_fused_path(NK), knot_lds.inc): the caller has accumulated -X_j D_jp^-1 X_j' in the tiles s (kl_fused_update, straight from
// M_jp in MX: neither X nor U is stored); T_j is added to them and the block factorised.  Timg, consumed: as above.
template <int NK>
__device__ __forceinline__ bool knot_ldl_add(const QpWs& w, int j, kl_d4 (&s)[KlPanels<NK>::TILES], kl_lds* base, int r, kl_ldsi* P, int pbase,
                                             const kl_lds* Timg = nullptr, kl_ldsi* consumed = nullptr, int consumed_value = 0) {
    using A = KlArea<NK>;
    kl_lds *C = base + A::C, *I = base + A::I;
    if (Timg)
        return kl_knot_panels_add<NK, true>(s, [&](int mx, int mn) { return (double)Timg[mn * KL_LD + mx]; },  // (the images hold both triangles)
                                            [&] {
                                                kl_sync();
                                                if (consumed) kl_publish(consumed, consumed_value);
                                            },
                                            C, I, r, P, pbase);
    const double* Tg = w.Td + (size_t)j * NK * NK;
    return kl_knot_panels_add<NK, false>(s, [&](int mx, int mn) { return Tg[mn * NK + mx]; }, [] {}, C, I, r, P, pbase);
}
// the coupling coefficients of the rows a lane forms in kl_fused_update, towards the knot after j: coupling_coef for the rows 16 t + (lane & 15)
template <int NK>
__device__ __forceinline__ void fused_coupling_coef(const QpWs& w, int j, int dir, int lane, double (&cf)[KlPanels<NK>::NT][3]) {
    const __attribute__((address_space(1))) double* E = QGC(w.Ek) + 9 * (dir > 0 ? j + 1 : j);  // (global loads, see coupling_coef)
    kl_fused_coef<NK>(cf, lane, [&](int row, int q) { return dir > 0 ? E[3 * q + row % 3] : E[3 * (row % 3) + q]; });
}

// M = L^-T of the block just factorised: rows into MX (for the coupling factor) and, with 1 / d, into global memory (for the
// substitutions).  FOLLOW: run by the chain's companion wave concurrently with knot_ldl of the chain wave (kl_inverse_rows: kl_follow_LinvT a
// column or two behind the chain, or kl_inverse_panels one panel behind it).
template <int NK, bool FOLLOW>
__device__ __forceinline__ void knot_inverse(const QpWs& w, int j, kl_lds* base, int r, bool act, kl_ldsi* P, int pbase, int& seen, kl_ldsi* Mdone,
                                             int done_value) {
    using A = KlArea<NK>;
    kl_lds *C = base + A::C, *MX = base + A::MX, *I = base + A::I;
    double m[NK];
    // (kl_inverse_rows announces *Mdone = done_value as soon as the chain may go on: after the read of 1 / d -- its next block overwrites I --, and on
    // the fused path BEFORE the read-back of the row that the stores below need)
    const double dinv = kl_inverse_rows<NK, FOLLOW>(m, C, I, MX, r, act, P, pbase, Mdone, done_value);
    __attribute__((address_space(1))) double* Mg = QG(w.Lf + (size_t)j * KF_SLOT(NK));
    // (256-thread build: the next block's inputs, sent for a block ago by global_load_lds, are counted on this wave's memory counter; they have
    // long landed -- drain the counter HERE, so that the tiles' wait for them does not have to wait for the row stores below as well)
    if (FOLLOW && QP_FOLLOW_ASM) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (act) {  // row r of M_j and 1 / d_j -> QpWs::Lf (16 bytes per lane and store instruction: the store path of a CU is issue bound)
        __attribute__((address_space(1))) double* row = Mg + KF_ELEM(NK, r, 0);  // (where column 0 would be: only k >= kf_first(NK, r) is stored)
        if ((NK & 1) == 0) {
#pragma unroll
            for (int k = 0; k < NK; k += 2)
                if (k + 1 >= r) *(__attribute__((address_space(1))) kl_d2*)(row + k) = kl_d2{m[k], m[k + 1]};  // (M_j is upper triangular; the staging does not fetch the rest)
        } else {
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (k >= r) row[k] = m[k];
        }
        Mg[KF_DINV(NK) + r] = dinv;
    }
}

// chain-side timers of the left chain (-DQP_PROFILE; 100 MHz clock, like the phase timers): SC 25 = the rank-NK update, 26 = waiting for the block
// assembly, 27 = the knot itself (T into the tiles, factorisation, waiting for M; without the fused update also the coupling rows),
// 29 = the forward substitution steps taken along the way (QP_FWD_IN_FACTOR; slot 28 is SC_SWEEP_BYTES).
// They must not change what they measure: the time stamp is wave-uniform and stays in scalar registers, a step adds its difference to a
// 64-bit LDS word behind the progress words (cleared with them at the start of a factorisation; every lane adds, all but lane 0 of the left
// chain add zero: no branch inside the step), and the three sums go to global memory once per factorisation (CHAIN_FLUSH).
#if defined(QP_PROFILE) && !defined(QP_LHSTATS) && !defined(QP_SOLVE_TIMERS)
#define CHAIN_TW(cnt, slot) ((__attribute__((address_space(3))) unsigned long long*)((cnt) + 96) + ((slot) - 25))
#define CHAIN_T0 long long ct_ = wall_clock64()
#define CHAIN_T(slot)                                                                                                                              \
    do {                                                                                                                                           \
        const long long t_ = wall_clock64();                                                                                                       \
        __hip_atomic_fetch_add(CHAIN_TW(cnt, slot), (dir > 0 && r == 0) ? (unsigned long long)(t_ - ct_) : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
        ct_ = t_;                                                                                                                                  \
    } while (0)
#define CHAIN_FLUSH()                                                                                   \
    do {                                                                                                \
        kl_sync();                                                                                      \
        if (w.prof && dir > 0 && r == 0)                                                                \
            for (int k_ = 25; k_ < 28; ++k_) w.prof[k_] += (double)(long long)*CHAIN_TW(cnt, k_);       \
        if (QP_FWD_IN_FACTOR && w.prof && dir > 0 && r == 0) w.prof[29] += (double)(long long)*CHAIN_TW(cnt, 29); \
    } while (0)
#else
#define CHAIN_T0
#define CHAIN_T(slot)
#define CHAIN_FLUSH()
#endif
// progress words of chain h (LDS ints behind the assembly counters): [2h] = images / pivots published by the chain wave (monotone over
// the whole factorisation: block i publishes i * (NK + 1) + 1 ...), [2h + 1] = blocks whose M rows the companion wave has put into MX
#define CHAIN_SYNC(cnt, h) ((kl_ldsi*)((cnt) + 64 + 2 * (h)))
// 512-thread build: [h] = number of blocks chain h has read out of the assembling waves' LDS images (a wave may overwrite its image of
// step i - 2 when this says i - 1)
#define ASM_CONSUMED(cnt, h) ((kl_ldsi*)((cnt) + 72 + (h)))

// ---- the predictor's forward substitution along the factorisation (QP_FWD_IN_FACTOR; blocks on the fused path): kl_forward_step and
// kl_middle_step of knot_lds.inc, which has the argument for where the step's vectors live.  z_jp goes to QpWs::rhs, where solve_staged's
// backward-only mode (SolveOut::rhs_mode 3) finds it.
static_assert((QP_FWD36 != 0) == (QP_FWD_IN_FACTOR && kl_fused_path(36)), "QP_FWD36 (qp.hip) out of step with kl_fused_path");
// rhs_r, e0 .. e2: rhs_jp[rr] and row rr of T_{jp,jpp} (zeros for a chain's first block), loaded by the caller a block ahead
template <int NK>
__device__ __forceinline__ void wave_forward_step(const QpWs& w, kl_lds* base, int jp, double rhs_r, double e0, double e1, double e2, int r) {
    kl_forward_step<NK>(base, QG(w.rhs) + (size_t)jp * NK + (r < NK ? r : 0), rhs_r, e0, e1, e2, r);
}
// what the caller loads for the step of block j, right after it has factorised it (global loads, see coupling_coef)
template <int NK>
__device__ __forceinline__ void wave_forward_fetch(const QpWs& w, int j, int dir, bool first, int r, double& rhs_r, double& e0, double& e1, double& e2) {
    const int rr = r < NK ? r : 0;
    rhs_r = QGC(w.rhs)[(size_t)j * NK + rr];
    coupling_coef(w, first ? j : j - dir, dir, rr, e0, e1, e2);  // (first block: a valid address, T_{j+dir,j}; its coefficients become zeros)
    e0 = first ? 0.0 : e0, e1 = first ? 0.0 : e1, e2 = first ? 0.0 : e2;
}

// one chain: blocks j0, j0+dir, ... (count of them).  The chain wave factorises; its companion wave (wave_factor_follow) computes
// M_j = L_j^-T a column or two (panel path: one panel of 4 columns) behind and stores it.  On return the chain's LDS area holds the coupling factor X towards the middle
// block (MX; on the fused path M of the chain's last block instead, once the companion is done) and the reciprocal pivots of its last block (I): wave_factor_mid
// reads both chains' areas.
template <int NK>
__device__ __forceinline__ bool wave_factor_chain(const QpDims& d, const QpWs& w, int j0, int count, int dir, double* ldsW, int* cnt, int h) {
    using A = KlArea<NK>;
    kl_lds* base = (kl_lds*)ldsW;
    kl_lds *MX = base + A::MX, *I = base + A::I, *U = base + A::C;
    kl_ldsi *P = CHAIN_SYNC(cnt, h), *Mdone = P + 1;
    const int r = threadIdx.x & 63;
    const bool act = r < NK;
    const int rr = act ? r : 0;
    bool ok = true;
    int seen = 0, seen_img = 0;
    if constexpr (kl_fused_path(NK)) {
        // S_j is formed in the tiles: -X_j D_jp^-1 X_j' from M_jp (MX: the companion's rows, which this wave no longer overwrites) as soon as the
        // companion has announced them, still in front of the wait for T_j's image; then T_j, then the factorisation.  No coupling rows.
        double cf[KlPanels<NK>::NT][3];
        [[maybe_unused]] double f_rhs = 0, f_e0 = 0, f_e1 = 0, f_e2 = 0;  // QP_FWD_IN_FACTOR: what the forward step of the block just factorised starts from
        for (int i = 0, j = j0; i < count; ++i, j += dir) {
            CHAIN_T0;
            kl_d4 s[KlPanels<NK>::TILES];
            kl_tiles_zero<NK>(s);
            if (i > 0) {
                kl_await(Mdone, i, seen);
                CHAIN_T(27);
                kl_fused_update<NK>(s, MX, I, r, cf);
            }
            CHAIN_T(25);
            if (QP_FWD_IN_FACTOR) {
                // the forward step of block i - 1, out of MX / I, into the wait for block i's image (wave_forward_step).  Its store of z is a
                // block's factorisation ahead of the next wait on the memory counter (the update's coefficients, one iteration on)
                if (i > 0) wave_forward_step<NK>(w, base, j - dir, f_rhs, f_e0, f_e1, f_e2, r);
                CHAIN_T(29);
            }
            if (QP_FOLLOW_ASM)
                kl_await(ASMF_READY(cnt, h), i + 1, seen_img);
            else
                wait_blocks(cnt, i);
            CHAIN_T(26);
            fused_coupling_coef<NK>(w, j, dir, r, cf);  // (issued here: nine loads from the L2, needed by the NEXT block's update)
            const kl_lds* Timg = ASM_HELPERS > 0 ? (const kl_lds*)(ldsW - (size_t)h * A::SIZE + 2 * A::SIZE + 128 + (size_t)(h + 2 * (i & 1)) * ASML_DOUBLES(NK, (NK / 9)))
                                 : QP_FOLLOW_ASM ? (const kl_lds*)(ldsW - (size_t)h * A::SIZE + 2 * A::SIZE + 128 + (size_t)h * ASML_DOUBLES(NK, (NK / 9)))
                                                 : nullptr;
            if (!knot_ldl_add<NK>(w, j, s, base, r, P, i * (NK + 1), Timg, ASM_CONSUMED(cnt, h), i + 1)) ok = false;
            // (the step's four loads leave here, not earlier: they are not live across the panel loop, and have the companion's last panel
            // and the next block's update to land)
            if (QP_FWD_IN_FACTOR) wave_forward_fetch<NK>(w, j, dir, i == 0, r, f_rhs, f_e0, f_e1, f_e2);
            CHAIN_T(27);
        }
        if (QP_FWD_IN_FACTOR) {  // the chain's last block: its M has to be waited for here (count > 0: see the callers)
            CHAIN_T0;
            kl_await(Mdone, count, seen);
            CHAIN_T(27);
            wave_forward_step<NK>(w, base, j0 + (count - 1) * dir, f_rhs, f_e0, f_e1, f_e2, r);
            CHAIN_T(29);
        }
        CHAIN_FLUSH();
        return ok;  // (lever off: the last block's M is waited for by the workgroup barrier in front of wave_factor_mid)
    }
    for (int i = 0, j = j0; i < count; ++i, j += dir) {
        CHAIN_T0;
        if (i > 0) kl_syrk<NK>(MX, I, U, r, false);
        CHAIN_T(25);
        if (QP_FOLLOW_ASM)
            kl_await(ASMF_READY(cnt, h), i + 1, seen_img);  // the companion wave's image of this block
        else
            wait_blocks(cnt, i);
        CHAIN_T(26);
        double e0, e1, e2, x[NK];
        coupling_coef(w, j, dir, rr, e0, e1, e2);  // (issued here: three loads from the L2, ~1 us under load, needed after the factorisation)
        // (512-thread build: T_j from the LDS image of the assembling wave (side h, parity of the step), see twisted_factor)
        // (256-thread build: from the ONE image of the chain's companion wave, see twisted_factor ROLE 2)
        const kl_lds* Timg = ASM_HELPERS > 0 ? (const kl_lds*)(ldsW - (size_t)h * A::SIZE + 2 * A::SIZE + 128 + (size_t)(h + 2 * (i & 1)) * ASML_DOUBLES(NK, (NK / 9)))
                             : QP_FOLLOW_ASM ? (const kl_lds*)(ldsW - (size_t)h * A::SIZE + 2 * A::SIZE + 128 + (size_t)h * ASML_DOUBLES(NK, (NK / 9)))
                                             : nullptr;
        if (!knot_ldl<NK>(w, j, i > 0, base, r, act, rr, P, i * (NK + 1), Timg, ASM_CONSUMED(cnt, h), i + 1)) ok = false;
        kl_await(Mdone, i + 1, seen);
        kl_coupling_rows<NK>(x, MX, r, act, e0, e1, e2);
        CHAIN_T(27);
    }
    CHAIN_FLUSH();
    return ok;
}

// the middle block collects both Schur complements (the chains' areas: ldsL = left chain = this wave's own area, ldsR = right chain)
template <int NK>
__device__ __forceinline__ bool wave_factor_mid(const QpDims& d, const QpWs& w, double* ldsL, double* ldsR, int* cnt, int cnt_idx) {
    using A = KlArea<NK>;
    kl_lds *bl = (kl_lds*)ldsL, *br = (kl_lds*)ldsR;
    const int r = threadIdx.x & 63, mid = twist_mid(d.nj);
    const bool act = r < NK;
    const int rr = act ? r : 0;
    int nsy = 0;
    [[maybe_unused]] kl_d4 s[kl_fused_path(NK) ? KlPanels<NK>::TILES : 1];
    if constexpr (kl_fused_path(NK)) {  // both chains' updates into the one set of tiles: the left chain's M with the coefficients towards mid from below, the right chain's from above
        double cl[KlPanels<NK>::NT][3], cr[KlPanels<NK>::NT][3];
        if (mid > 0) fused_coupling_coef<NK>(w, mid - 1, +1, r, cl);
        if (mid + 1 < d.nj) fused_coupling_coef<NK>(w, mid + 1, -1, r, cr);
        kl_tiles_zero<NK>(s);
        if (mid > 0) kl_fused_update<NK>(s, bl + A::MX, bl + A::I, r, cl);
        if (mid + 1 < d.nj) {
            if (mid > 0) {  // each side summed on its own, then the two sums added: the roundings of U_left + U_right (once per factorisation)
                kl_d4 s2[KlPanels<NK>::TILES];
                kl_tiles_zero<NK>(s2);
                kl_fused_update<NK>(s2, br + A::MX, br + A::I, r, cr);
#pragma unroll
                for (int t = 0; t < KlPanels<NK>::TILES; ++t) s[t] += s2[t];
            } else {
                kl_fused_update<NK>(s, br + A::MX, br + A::I, r, cr);
            }
        }
    } else {
        if (mid > 0) kl_syrk<NK>(bl + A::MX, bl + A::I, bl + A::C, r, false), nsy++;
        if (mid + 1 < d.nj) kl_syrk<NK>(br + A::MX, br + A::I, bl + A::C, r, nsy > 0), nsy++;
    }
    if (QP_FOLLOW_ASM) {
        int seen_img = 0;
        kl_await(ASMF_READY(cnt, 0), mid + 1, seen_img);  // the left chain's companion makes the middle block after the chain's mid blocks
    } else {
        wait_blocks(cnt, cnt_idx);
    }
    // progress words of the middle block.  512-thread build: its M is computed by the left chain's companion wave, like every other
    // block's (twisted_factor, ROLE 2) -- on the chain wave it is ~10 k cycles more at the end of every factorisation: one mission
    // 122.4 -> 121.1 ms.  With two workgroups per CU the polling companion costs the neighbour more than it saves (-1.3 % at 2000
    // resident, A/B on one box): the 256-thread build keeps M on the chain wave.
    kl_ldsi* scratch = CHAIN_SYNC(cnt, 2);
    const kl_lds* Timg = ASM_HELPERS > 0 ? (const kl_lds*)(ldsL + 2 * A::SIZE + 128 + (size_t)(2 * (cnt_idx & 1)) * ASML_DOUBLES(NK, (NK / 9)))
                         : QP_FOLLOW_ASM ? (const kl_lds*)(ldsL + 2 * A::SIZE + 128) : nullptr;
    bool ok;
    if constexpr (kl_fused_path(NK))
        ok = knot_ldl_add<NK>(w, mid, s, bl, r, scratch, 0, Timg);
    else
        ok = knot_ldl<NK>(w, mid, nsy > 0, bl, r, act, rr, scratch, 0, Timg);
    if (!QP_MID_FOLLOW) {
        int seen = 0;
        knot_inverse<NK, false>(w, mid, bl, r, act, scratch, 0, seen, scratch, 0);
    }
    if constexpr (QP_FWD_IN_FACTOR && kl_fused_path(NK)) {
        // The middle step of the predictor's substitution (the s == SF body of solve_staged): forward with both chains' last v -- each in
        // the V slot of its chain's area (KfSlots; the right chain's made visible by the workgroup barrier in front of this function; zeros
        // where there is no chain) --, then backward, out of M_mid in the left area's MX and 1 / d_mid in its I.  x_mid goes to QpWs::rhs.
        // A, Z and the partial sums: the left area's slots -- the middle block's images have been read (above, or by the companion before its
        // announcement), and the left chain's own last step is over.
        using F = KfSlots<NK>;
        if (QP_MID_FOLLOW) {  // M_mid comes from the left chain's companion (twisted_factor)
            int seen = 0;
            kl_await(scratch + 1, 1, seen);
        }
        const kl_lds *V0 = bl + A::C + F::V, *V1 = br + A::C + F::V;
        const int g3 = 3 * (rr / 3);
        double v = QGC(w.rhs)[(size_t)mid * NK + rr];
        if (mid > 0) {
            double e0, e1, e2;
            coupling_coef(w, mid - 1, +1, rr, e0, e1, e2);
            v -= e0 * V0[g3] + e1 * V0[g3 + 1] + e2 * V0[g3 + 2];
        }
        if (mid + 1 < d.nj) {
            double e0, e1, e2;
            coupling_coef(w, mid + 1, -1, rr, e0, e1, e2);
            v -= e0 * V1[g3] + e1 * V1[g3 + 1] + e2 * V1[g3 + 2];
        }
        const double x = kl_middle_step<NK>(bl, v, r);
        QG(w.rhs)[(size_t)mid * NK + rr] = x;
    }
    return ok;
}

// whole twisted factorisation; every thread of the workgroup calls it.  flag: LDS int.
// The knot blocks T_j are ASSEMBLED HERE, by waves that do not run a chain, in the order the chains consume them (step i: blocks i
// and nj-1-i; last the middle one), each step announced through an LDS counter (wait_blocks): the assembly -- 8-10 % of an
// interior-point iteration when it was a phase of its own -- disappears behind the dependent chains.
// ROLE: 0 = compiled for the two chain waves, 2 = for their companions (waves 2, 3), 1 = for the assembling waves (4..) of the
// 512-thread build: three __noinline__ functions with the same workgroup barriers, see solve_staged.
template <int NK, int ROLE>
__device__ __forceinline__ bool twisted_factor(const QpDims& d, const QpWs& w, int* flag, double* lds, const AsmArgs* asmb) {
    const int wave = (ROLE == 0 || ROLE == 2) ? (threadIdx.x >> 6) & 1 : 4, mid = twist_mid(d.nj);  // roles 0 / 2: which chain
    const int nl = mid, nr = d.nj - 1 - mid, SF = nl > nr ? nl : nr;
    constexpr int AREA = KlArea<NK>::SIZE;    // one chain wave's LDS area (knot_lds.inc)
    int* cnt = (int*)(lds + 2 * AREA);  // [SF + 1] assembly counters, then (at +64) the chains' progress words
    static_assert((QP_MAX_M - 1) / 2 + 1 <= 64, "cnt[0..SF] must end below CHAIN_SYNC (cnt + 64): sessions with M > QP_MAX_M are refused");
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    bool ok = true;
    // rows >= NK of the X images are never written by a row's own lane: clear them once (they only feed unused tile entries)
    for (int i = threadIdx.x; i < 2 * AREA + 64; i += QP_THREADS) lds[i] = 0.0;
    __syncthreads();
    // The chain waves issue dependent instructions; whenever the SIMD's arbiter makes one of them queue behind the ready instructions
    // of other waves (the helpers, the co-resident workgroup's sweeps) the chain stretches, while giving it the first slot costs the
    // others next to nothing: raise the priority for the chain (+2.5 % at 2000 missions).
    if (ROLE == 0) {
        __builtin_amdgcn_s_setprio(QP_CHAIN_PRIO);
        if (wave == 0 && mid > 0) ok = wave_factor_chain<NK>(d, w, 0, mid, +1, lds, cnt, 0);
        if (wave == 1 && nr > 0) ok = wave_factor_chain<NK>(d, w, d.nj - 1, nr, -1, lds + AREA, cnt, 1);
        if (wave == 1) __builtin_amdgcn_s_setprio(0);
    }
    if (ROLE == 1) {
        // assembling waves (512-thread build): through the LDS like the 256-thread build's up-front assembly (assemble_knots_lds), one
        // wave per block.  Waves 4, 5 take the left / right chain's block of the even steps, waves 6, 7 those of the odd steps (two
        // chain steps of time per block); a wave announces its block by adding ASM_HELPERS / 2 to the step's counter, so that
        // wait_blocks sees ASM_HELPERS when both blocks of a step are out.  The middle block (step SF) is wave 4's / 6's.
        const AsmArgs A = *asmb;
        const int hw = (threadIdx.x >> 6) - ASM_WAVE0, side = hw & 1, par = hw >> 1;  // par: parity of the steps this wave serves
        double* scratch = lds + 2 * AREA + 128 + (size_t)hw * ASML_DOUBLES(NK, (NK / 9));
        int i = par - 2;
        kl_ldsi* consumed = ASM_CONSUMED(cnt, side);
        int seen_c = 0;
        assemble_knots_lds<false>(
            A, scratch,
            [&] {
                for (i += 2; i <= SF; i += 2) {
                    const bool work = i < SF ? (side ? i < nr : i < nl) : side == 0;
                    if (work) {
                        if (i >= 2) kl_await(consumed, i - 1, seen_c);  // the chain has read this wave's image of step i - 2
                        return i < SF ? (side ? d.nj - 1 - i : i) : mid;
                    }
                    // nothing to assemble for this wave at step i: announce it all the same
                    if ((threadIdx.x & 63) == 0)
                        __hip_atomic_fetch_add(cnt + i, i < SF ? ASM_HELPERS / 2 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                return -1;
            },
            [&](int) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if ((threadIdx.x & 63) == 0)
                    __hip_atomic_fetch_add(cnt + i, i < SF ? ASM_HELPERS / 2 : ASM_HELPERS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            });
    }
    if (ROLE == 2) {
        // companion of chain `wave`: M_j behind the chain's factorisation of block j
        const int count = wave == 0 ? nl : nr, j0 = wave == 0 ? 0 : d.nj - 1, dir = wave == 0 ? +1 : -1;
        kl_lds* base = (kl_lds*)(lds + wave * AREA);
        kl_ldsi *P = CHAIN_SYNC(cnt, wave), *Mdone = P + 1;
        const int r = threadIdx.x & 63;
        int seen = 0;
        if (QP_FOLLOW_ASM) {
            // ... and the chain's blocks, assembled just in time: block n + 1 right after the companion work of block n, while the chain
            // forms the coupling rows and the rank-NK update; the left chain's companion makes the MIDDLE block last.  One image per chain:
            // the chain read block n out of it at the start of its factorisation (ASM_CONSUMED), long before block n + 1 is written.
            const AsmArgs A = *asmb;
            double* scratch = lds + 2 * AREA + 128 + (size_t)wave * ASML_DOUBLES(NK, (NK / 9));
            kl_ldsi *ready = ASMF_READY(cnt, wave), *consumed = ASM_CONSUMED(cnt, wave);
            const int total = count + (wave == 0 ? 1 : 0);
            int seen_c = 0;
            auto blk = [&](int n) { return n < count ? j0 + n * dir : mid; };
            auto make = [&](int n) {  // block n's inputs are in the scratch (fetched a block ago): its tiles, then the fetch of block n + 1
                if (n > 0) kl_await(consumed, n, seen_c);
                fasm_tiles(A, scratch, blk(n));
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                kl_publish(ready, n + 1);
                if (n + 1 < total) fasm_fetch(A, scratch, blk(n + 1));
            };
            if (total > 0) {
                fasm_fetch(A, scratch, blk(0));
                make(0);
            }
            for (int i = 0; i < count; ++i) {
                knot_inverse<NK, true>(w, j0 + i * dir, base, r, r < NK, P, i * (NK + 1), seen, Mdone, i + 1);
                if (i + 1 < total) make(i + 1);
            }
        } else {
            for (int i = 0; i < count; ++i) knot_inverse<NK, true>(w, j0 + i * dir, base, r, r < NK, P, i * (NK + 1), seen, Mdone, i + 1);
        }
    }
    if (!ok && (threadIdx.x & 63) == 0) atomicExch(flag, 1);
    __threadfence_block();
    __syncthreads();
    if (*flag) return false;
    if (ROLE == 0 && wave == 0) {
        if (!wave_factor_mid<NK>(d, w, lds, lds + AREA, cnt, SF) && threadIdx.x == 0) *flag = 1;
        __builtin_amdgcn_s_setprio(0);
    }
    if (QP_MID_FOLLOW && ROLE == 2 && wave == 0) {  // M of the middle block, behind wave_factor_mid's factorisation
        const int r = threadIdx.x & 63;
        int seen = 0;
        kl_ldsi* P = CHAIN_SYNC(cnt, 2);
        knot_inverse<NK, true>(w, mid, (kl_lds*)lds, r, r < NK, P, 0, seen, P + 1, 1);
    }
    __threadfence_block();
    __syncthreads();
    return *flag == 0;
}
