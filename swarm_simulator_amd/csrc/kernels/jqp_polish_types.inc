// jqp_polish_types.inc — what the joint solver's sweeps and layout need of its active-set polish (jqp_polish.inc: the kernels): the polish
// counters and states (PC_*, PS_*), pol_ncmax, the polish record of a mission and its place in the workspace (Pol, PolLayout, pol_layout,
// pol_carve) and pol_emit.  Included by jqp.hip ahead of its sweeps; needs JArgs (jqp.h) and JDims / jdims, JT / JTT of jqp.hip.

enum { PC_NRAW = 0, PC_NCAND, PC_NA, PC_NBLK, PC_NINF, PC_BEST, PC_PLEFT, PC_BPPDONE, PC_FIRSTNEW, PC_ROUND, PC_OUTER, PC_REFINE, PC_REASON,
       PC_BPPIT, PC_NNEW, PC_MODE /* 0: block principal pivoting, 1: block Lawson-Hanson from the best pivoting iterate */, PC_LHIT, PC_N = 32 };
// polish state of a mission (ST_PSTATE)
enum { PS_IDLE = 0, PS_SOLVE /* (new) candidates: S, dual solve */, PS_PRIMAL /* primal step + verification */, PS_ACCEPTED, PS_FAILED };

// candidate rows a polish attempt can hold.  Measured: 10..13 candidates per agent at the iterates the attempts start from (622..778 rows at
// 64 agents, active sets of 610..840); 20 N + 512 leaves a factor 1.7..2.3 of room.  (32 N + 512 until round 5: the four candidate-squared
// matrices S, W0, W1, G were 210 of a 64-agent mission's 349 MB of workspace; now 103 of 242.)
__host__ __device__ inline int pol_ncmax(int N) {
    int n = 20 * N + 512;
    if (n > 16384) n = 16384;
    return (n + JT - 1) / JT * JT;
}

struct Pol {
    int* cnt;
    double *R, *c0, *v0, *jz, *du;
    int *r_row, *r_a, *r_b, *r_j6, *r_snap;
    double *r_n, *r_slack, *r_str, *r_snapv;
    int *c_row, *c_a, *c_b, *c_knot, *c_snap;
    double *c_n, *c_t, *c_slack, *c_str, *c_snapv;
    double *dv, *z, *g, *e, *y, *bestz;
    int *inA, *Aidx, *flip, *mark, *bestA, *pos, *twin;
    double *S, *W0, *W1, *G, *P, *Y, *rA, *scal;
    int ncmax, nr;
};

struct PolLayout {  // offsets in doubles: the records from o_pol, the candidate-squared matrices (S .. Y) from o_inv
    size_t cnt, R, c0, v0, jz, du, r_int, r_dbl, c_int, c_dbl, vec, ia, pos, total;
    size_t S, W0, W1, G, P, Y, big_total;
};
__host__ __device__ inline PolLayout pol_layout(int N, int MS) {
    const JDims d = jdims(N, MS);
    const size_t nc = pol_ncmax(N), nr = 3 * (size_t)d.nj, nv = (size_t)d.nj * d.nkp;
    const size_t nrows = 6 * (size_t)d.ncp + (size_t)d.npair * d.oq;
    PolLayout L;
    size_t o = 0;
    auto take = [&](size_t n) {
        const size_t r = o;
        o += (n + 31) & ~size_t(31);
        return r;
    };
    L.cnt = take(PC_N / 2 + 1), L.R = take(nr * nr), L.c0 = take(nv), L.v0 = take(nv), L.jz = take(nv), L.du = take(nv);
    L.r_int = take(5 * nc / 2 + 4), L.r_dbl = take(6 * nc), L.c_int = take(5 * nc / 2 + 4), L.c_dbl = take(9 * nc);
    L.vec = take(7 * nc + 8), L.ia = take(3 * nc + 4), L.pos = take(nrows / 2 + 4);
    L.total = o;
    // The four candidate-squared matrices, the pivot tiles and the panel of the polish's sweep share their memory with the explicit
    // inverses of the interior-point iteration (Ws::inv): a polish call never applies those, and every interior-point round factorises
    // before it solves (launch_planner_joint), so neither outlives the other's turn.
    o = 0;
    L.S = take(nc * nc), L.W0 = take(nc * nc), L.W1 = take(nc * nc), L.G = take(nc * nc), L.P = take(2 * JTT), L.Y = take(nc * JT);
    L.big_total = o;
    return L;
}
__device__ __forceinline__ Pol pol_carve(const JArgs& A, int mission) {
    double* b = A.ws + (size_t)mission * A.L.stride + A.L.o_pol;
    const PolLayout L = pol_layout(A.L.N, A.L.MS);
    const size_t nc = pol_ncmax(A.L.N);
    Pol p;
    p.ncmax = (int)nc, p.nr = 3 * A.L.njS;
    p.cnt = (int*)(b + L.cnt), p.R = b + L.R, p.c0 = b + L.c0, p.v0 = b + L.v0, p.jz = b + L.jz, p.du = b + L.du;
    int* ri = (int*)(b + L.r_int);
    p.r_row = ri, p.r_a = ri + nc, p.r_b = ri + 2 * nc, p.r_j6 = ri + 3 * nc, p.r_snap = ri + 4 * nc;
    double* rd = b + L.r_dbl;
    p.r_n = rd, p.r_slack = rd + 3 * nc, p.r_str = rd + 4 * nc, p.r_snapv = rd + 5 * nc;
    int* ci = (int*)(b + L.c_int);
    p.c_row = ci, p.c_a = ci + nc, p.c_b = ci + 2 * nc, p.c_knot = ci + 3 * nc, p.c_snap = ci + 4 * nc;
    double* cd = b + L.c_dbl;
    p.c_n = cd, p.c_t = cd + 3 * nc, p.c_slack = cd + 6 * nc, p.c_str = cd + 7 * nc, p.c_snapv = cd + 8 * nc;
    double* v = b + L.vec;
    p.dv = v, p.z = v + nc, p.g = v + 2 * nc, p.e = v + 3 * nc, p.rA = v + 4 * nc, p.y = v + 5 * nc, p.bestz = v + 6 * nc, p.scal = v + 7 * nc;
    int* ia = (int*)(b + L.ia);
    p.inA = ia, p.Aidx = ia + nc, p.flip = ia + 2 * nc, p.mark = ia + 3 * nc, p.bestA = ia + 4 * nc, p.twin = ia + 5 * nc;
    p.pos = (int*)(b + L.pos);
    double* bb = A.ws + (size_t)mission * A.L.stride + A.L.o_inv;
    p.S = bb + L.S, p.W0 = bb + L.W0, p.W1 = bb + L.W1, p.G = bb + L.G, p.P = bb + L.P, p.Y = bb + L.Y;
    return p;
}

// a row joins the raw candidate list (unordered: jp_sort puts the new ones into ascending row order)
__device__ __forceinline__ void pol_emit(const Pol& p, int row, int a, int b, int j6, double n0, double n1, double n2, double slack, int snap,
                                         double snapv, double strength) {
    const int idx = atomicAdd(&p.cnt[PC_NRAW], 1);
    if (idx >= p.ncmax) return;
    p.r_row[idx] = row, p.r_a[idx] = a, p.r_b[idx] = b, p.r_j6[idx] = j6, p.r_snap[idx] = snap;
    p.r_n[3 * idx] = n0, p.r_n[3 * idx + 1] = n1, p.r_n[3 * idx + 2] = n2;
    p.r_slack[idx] = slack, p.r_str[idx] = strength, p.r_snapv[idx] = snapv;
}
