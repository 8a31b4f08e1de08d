// qp_polish_types.inc — what the row sweeps need of the active-set polish (qp_polish.inc: the algorithms): the candidate record and the
// polish workspace (Cand, PolishWs, polish_carve), emit_cand, and the wave helpers of the dual solve (WSYNC, wave_argmax).
// Included by qp.hip after qp_base.inc, ahead of qp_rows.inc; needs QpDims, QpWs, wave_red (qp_base.inc) and the PL_* sizes of qp.hip.

// PL_NC (candidate rows) and PL_PMAX (rows simultaneously active in the dual solve) are defined in qp.hip

struct Cand {
    double n[3], t[3];  // row = sum_k n_k * (t . u_{a,k}) - [b >= 0] sum_k n_k * (t . u_{b,k})  at knot `knot`
    double slack, snap_val;
    double strength;  // z/s of the interior-point iterate (0 < . for candidates): warm start order of the dual solve
    int row, knot, a, b, snap_idx, pad;
};

struct PolishWs {
    Cand* cand;    // [PL_NC]
    double* v0;    // [3][nred]  the gradient column K0^-1 F'(2Qx); then the gradient F'(2Qx) itself and the primal step's g + J_P' z
    double* Sg;    // [PL_NC][PL_NC]
    int* ncand;    // [4] counter, accepted flag, ...
    double* Lbig;  // [PL_PBIG (PL_PBIG + 1) / 2] packed factor of the second, large-capacity attempt (global memory)
    double* ptab;  // [6 PL_PBIG][4] primal step: the active rows listed per (agent, dim) -- knot and position in P, sgn n_k t[0..2]
    // the mission's (k0_mission_tables): K0 depends on the segment times alone
    double* k0f;   // [nj][18] factor of K0 in double (k0_factor_step), then two ints: the double / the dd factor met a pivot that is not positive
    double* G;     // lower block triangle of K0^-1 (ipm::k0g_block)
};
// (the order follows polish_ws_doubles: what moves with the batch's nk comes last)
__device__ __forceinline__ PolishWs polish_carve(double* p, int nj) {
    PolishWs pw;
    pw.k0f = p, p += 18 * (size_t)nj + 2;
    pw.G = p, p += k0g_doubles(nj);
    pw.cand = (Cand*)p, p += PL_NC * 14;
    pw.Sg = p, p += polish_s_doubles(nj);
    pw.ncand = (int*)p, p += 8;
    pw.Lbig = p, p += lhp_size(PL_PBIG);
    pw.ptab = p, p += 4 * 6 * PL_PBIG;
    pw.v0 = p;
    return pw;
}

#define WSYNC()                                             \
    do {                                                    \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                    \
    } while (0)

// (wave_red, the wave-wide reduction of a double, is qp_base.inc's; the same steps for an int)
__device__ __forceinline__ int wave_min_int(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// the largest `best` of the wave and, among the lanes that hold it, the smallest index (-1: no lane has a candidate)
__device__ __forceinline__ void wave_argmax(double& best, int& bidx) {
    const double top = wave_red(bidx >= 0 ? best : -1e300, 1);
    const int idx = wave_min_int(bidx >= 0 && best == top ? bidx : 0x7fffffff);
    best = top, bidx = idx == 0x7fffffff ? -1 : idx;
}

__device__ __forceinline__ void knot_of(const QpDims& d, const QpWs& w, int j6, int& knot, double t[3]) {
    const int m = j6 / 6, i = j6 % 6;
    if (i < 3) {
        knot = m;
        t[0] = t[1] = t[2] = 0;
        t[i] = 1;
    } else {
        knot = m + 1;
        const double* L = w.Lk + 9 * (m + 1) + 3 * (i - 3);
        t[0] = L[0], t[1] = L[1], t[2] = L[2];
    }
}

__device__ __forceinline__ void emit_cand(const QpDims& d, const QpWs& w, const PolishWs& pw, size_t r, int j6, int a, int b, double n0,
                                          double n1, double n2, double slack, int snap_idx, double snap_val, double strength) {
    const int idx = atomicAdd(pw.ncand, 1);
    if (idx >= PL_NC) return;
    Cand& c = pw.cand[idx];
    c.n[0] = n0, c.n[1] = n1, c.n[2] = n2;
    knot_of(d, w, j6, c.knot, c.t);
    c.slack = slack, c.snap_val = snap_val, c.strength = strength;
    c.row = (int)r, c.a = a, c.b = b, c.snap_idx = snap_idx, c.pad = 0;
}
