// qp_entries.inc — the entries of the block factorisation and the substitutions: the choice between the wave-register and the tiled path
// (factor_dispatch, solve_dispatch) and the stand-alone functions the batch driver calls, one per role of a wave (factor_entry_*,
// solve_entry_*; factor_entry, solve_entry).  Included by qp.hip after qp_wave_factor.inc, qp_wave_solve.inc and qp_tiled.inc, whose
// twisted_factor, solve_staged / SolveOut, factor_tiled and solve_tiled it needs; AsmArgs (qp_newton.inc); BlkArgs, blk_unpack, uni (qp_base.inc).

template <int ROLE>
__device__ __forceinline__ bool factor_dispatch(const QpDims& d, const QpWs& w, double* lA, int* flag, int lds_avail, const AsmArgs* asmb) {
    if (d.nk <= 36) {
        switch (d.nk) {
            case 9: return twisted_factor<9, ROLE>(d, w, flag, lA, asmb);
            case 18: return twisted_factor<18, ROLE>(d, w, flag, lA, asmb);
            case 27: return twisted_factor<27, ROLE>(d, w, flag, lA, asmb);
            default: return twisted_factor<36, ROLE>(d, w, flag, lA, asmb);
        }
    }
    if (ROLE != 0) return true;  // (the companion / assembling roles only exist on the wave path)
    return factor_tiled(d, w, flag, lA, lds_avail);
}

template <int ROLE>
__device__ __forceinline__ void solve_dispatch(const QpDims& d, const QpWs& w, double* rhs, double* lA, int lds_avail, SolveOut so = SolveOut{nullptr, nullptr, 0}) {
    if (d.nk <= 36) {
        switch (d.nk) {  // lA = start of the dynamic LDS region (the three block buffers are free between factorisations)
            case 9: solve_staged<9, ROLE>(d, w, rhs, lA, so); break;
            case 18: solve_staged<18, ROLE>(d, w, rhs, lA, so); break;
            case 27: solve_staged<27, ROLE>(d, w, rhs, lA, so); break;
            default: solve_staged<36, ROLE>(d, w, rhs, lA, so); break;
        }
        return;
    }
    if (ROLE != 1) solve_tiled(d, w, rhs, lA, lds_avail);  // (the staging role only exists on the wave path)
}

// The block factorisation / substitutions are compiled as stand-alone functions with by-value arguments: their register
// allocation (the wave-register path wants every VGPR) then neither depends on nor disturbs the row sweeps around them,
// and no kernel-level struct has its address taken.
// (inlining these two was measured: 1100 VGPR spills, 31k instead of 51k agent-trajectories/s)
__device__ __noinline__ bool factor_entry_chain(BlkArgs b, AsmArgs A, double* lds, int* flag) {
    QpDims d;
    QpWs w;
    blk_unpack(b, d, w);
    const AsmArgs Au = uni(A);
    return factor_dispatch<0>(d, w, uni(lds), uni(flag), uni(b.lds_avail), &Au);
}
__device__ __noinline__ bool factor_entry_assemble(BlkArgs b, AsmArgs A, double* lds, int* flag) {
    QpDims d;
    QpWs w;
    blk_unpack(b, d, w);
    const AsmArgs Au = uni(A);
    return factor_dispatch<1>(d, w, uni(lds), uni(flag), uni(b.lds_avail), &Au);
}
__device__ __noinline__ bool factor_entry_follow(BlkArgs b, AsmArgs A, double* lds, int* flag) {
    QpDims d;
    QpWs w;
    blk_unpack(b, d, w);
    const AsmArgs Au = uni(A);
    return factor_dispatch<2>(d, w, uni(lds), uni(flag), uni(b.lds_avail), &Au);
}
__device__ __forceinline__ bool factor_entry(const BlkArgs& b, const AsmArgs& A, double* lds, int* flag) {
    const int wave = threadIdx.x >> 6;
    if (b.nk <= 36 && wave >= 4) return factor_entry_assemble(b, A, lds, flag);
    if (b.nk <= 36 && wave >= 2) return factor_entry_follow(b, A, lds, flag);
    return factor_entry_chain(b, A, lds, flag);
}
__device__ __noinline__ void solve_entry_chain(BlkArgs b, double* rhs, double* lds, SolveOut so) {
    QpDims d;
    QpWs w;
    blk_unpack(b, d, w);
    solve_dispatch<0>(d, w, uni(rhs), uni(lds), uni(b.lds_avail), SolveOut{uni(so.dx_out), uni(so.Lk), uni(so.oq), uni(so.rhs_mode), uni(so.cpacc), uni(so.rbase), so.sigma_mu});
}
__device__ __noinline__ void solve_entry_stage(BlkArgs b, double* rhs, double* lds, SolveOut so) {
    QpDims d;
    QpWs w;
    blk_unpack(b, d, w);
    solve_dispatch<1>(d, w, uni(rhs), uni(lds), uni(b.lds_avail), SolveOut{uni(so.dx_out), uni(so.Lk), uni(so.oq), uni(so.rhs_mode), uni(so.cpacc), uni(so.rbase), so.sigma_mu});
}
// (every wave passes the same workgroup barriers in either function)
__device__ __forceinline__ void solve_entry(const BlkArgs& b, double* rhs, double* lds, SolveOut so = SolveOut{nullptr, nullptr, 0}) {
    if (b.nk <= 36 && (threadIdx.x >> 6) >= 2)
        solve_entry_stage(b, rhs, lds, so);
    else
        solve_entry_chain(b, rhs, lds, so);
}
