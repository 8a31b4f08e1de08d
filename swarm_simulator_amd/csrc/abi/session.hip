// session.hip — the C ABI of include/rbp.h on top of the HIP kernels.
//
// rbp_corridor_update / rbp_planner_update are the drop-in calls for Corridor::update (rbp_corridor.hpp:21-26)
// and RBPPlanner::update (rbp_planner.hpp:33-84); they are thin wrappers over the device-resident, batched
// session API that bench.py times.  There is NO CPU fallback: without a HIP device every call fails with
// RBP_ERR_NO_DEVICE.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../common/plan_stage.h"
#include "../kernels/jqp.h"
#include "../kernels/rbp_dev.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? RBP_ERR_NO_DEVICE : RBP_ERR_HIP, \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                              \
    } while (0)

struct Arena {
    char* base = nullptr;
    size_t size = 0, off = 0;
    template <class T>
    T* take(size_t n) {
        off = (off + 255) & ~size_t(255);
        T* p = reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return p;
    }
};

// host [N][mbk][w] <-> device slot [N][MB][w]
template <class T>
void repack_boxes(T* dst, int dst_mb, const T* src, int src_mb, int N, int w) {
    const int nb = std::min(dst_mb, src_mb);
    for (int a = 0; a < N; ++a) memcpy(dst + (size_t)a * dst_mb * w, src + (size_t)a * src_mb * w, sizeof(T) * (size_t)nb * w);
}

}  // namespace

int rbp_set_error(int code, const char* msg) { return fail(code, msg); }  // for the other translation units (kernels/edt.hip)

// A context owns one device arena that successive sessions (and the synchronous one-shot calls) reuse: the drop-in calls
// rbp_corridor_update / rbp_planner_update would otherwise hipMalloc + hipFree ~10 MB per plan.
static rbp_solver_opts default_solver_opts() {
    rbp_solver_opts o;
    rbp_solver_opts_defaults(&o);
    return o;
}

struct rbp_ctx {
    int device = 0;
    char* base = nullptr;
    size_t cap = 0;
    bool busy = false;  // a live session is using the arena
    rbp_solver_opts opts = default_solver_opts();
    char* ws_base = nullptr;  // QP workspace of the context's sessions: reserved by the first PLANNER run that needs it, kept, grown on demand
    size_t ws_cap = 0;
};

struct rbp_session {
    int device = 0;
    int n_cu = 256;
    DevSession d{};
    rbp_param param{};
    Arena arena;
    rbp_ctx* ctx = nullptr;  // non-null: the arena belongs to this context
    rbp_solver_opts opts = default_solver_opts();
    // QP workspace: reserved by the first PLANNER run for the options then in force (not by create: a corridor-only session needs none, and
    // the grid-wide joint solver's is large); a session's own allocation, or its context's
    void* qp_ws = nullptr;
    size_t qp_ws_per_mission = 0;
    char* ws_own = nullptr;
    bool ws_joint = false;    // what the workspace was laid out for
    int bs = 1, biter = 0;    // batch schedule of the plan (batch_schedule, kernels/rbp_dev.h)
    std::vector<int> Mk, MBk;         // per-mission segments / box capacity (host copy of DevSession::Mk, MBk)
    std::vector<DevWorld> worlds_h;
    // planner-stage inputs as uploaded, in device layout (so that a run which overwrote them can be reset)
    std::vector<int> sfc_count0;
    std::vector<double> sfc_box0, sfc_time0, rsfc_time0;
    std::vector<float> rsfc_normal0;
    bool have_corridor_inputs = false;
    bool joint_wide = false;  // the joint QP (plan/sequential = false) runs on the grid-wide solver (kernels/jqp.hip): decided per PLANNER run
    JointStats joint_stats{};
    int last_stages = 0;      // stages of the last rbp_session_run (time_scale only concerns a run that included the planner)
    // rbp_session_run_async of a grid-wide joint session: the solver's host loop (one synchronisation per interior-point round) runs on a
    // thread and a stream of the session's own; every later call on the session joins it first (join_worker)
    std::thread worker;
    int worker_rc = RBP_OK;
    hipStream_t jstream = nullptr;
    hipEvent_t jev_in = nullptr;
    // rbp_session_shard_joint: this session is one rank of a pair that shares a joint solve's factorisation (kernels/jqp.h JointShard);
    // the exchange buffers are the session's own
    JointShard shard{};
    char* shard_buf = nullptr;
    char* report_buf = nullptr;  // rbp_session_report: K reports and the pair kernel's partial minima (report_workspace_bytes), reserved by the first call
    char* dynamics_buf = nullptr;  // rbp_session_dynamics: K structs and the state kernel's partial peaks (dynamics_workspace_bytes), reserved by the first call
    char* separation_buf = nullptr;  // rbp_session_separation: K structs, one chunk's work list and partial tallies (separation_workspace_bytes), reserved by the first call
    char* clearance_buf = nullptr;  // rbp_session_clearance: K structs and the agent kernel's records (clearance_workspace_bytes), reserved by the first call
    char* swept_buf = nullptr;  // rbp_session_swept_clearance: K structs, one chunk's work list, item clearances and partial tallies (swept_workspace_bytes), reserved by the first call
    char* limits_buf = nullptr;  // rbp_session_limits: K structs, one chunk's work list, item ratios and partial tallies (limits_workspace_bytes), reserved by the first call
    // rbp_session_refill_from_ecbs: the capacity the arena was laid out for (session_describe; after a refill d.K <= cap.K, and d.M, d.max_boxes
    // stay cap's: the strides), the set of worlds the grids belong to (known for sessions that were created reserved or from a search, found
    // by the first refill of any other), and the staging block of the refills (RefillStage of kernels/rbp_dev.h: pinned, its device twin, and
    // the event behind the last copy out of it).  The QP workspace and the reports' buffers are sized for cap.K.
    rbp_session_capacity cap{};
    const rbp_dev_worlds* ws = nullptr;
    bool empty = false;  // created reserved and not refilled yet: the session holds no mission
    int lds_max = 0;     // the device's LDS per workgroup, as session_describe read it
    char *stage_h = nullptr, *stage_d = nullptr;
    hipEvent_t stage_ev = nullptr;
    bool stage_busy = false;  // stage_ev has been recorded
    // rbp_session_refill_from_plans: the staging block of a caller's plans (common/plan_stage.h: pinned, pstage_bytes of room for one round),
    // its device twin and the event behind the last copy out of it (rbp_session_reserve_plan_stage)
    char *pstage_h = nullptr, *pstage_d = nullptr;
    size_t pstage_bytes = 0;
    hipEvent_t pstage_ev = nullptr;
    bool pstage_busy = false;  // pstage_ev has been recorded
};

// what run, download and the reports answer for a reserved session that has not been refilled
static int no_mission(const rbp_session* s, const char* who) {
    return s->empty ? fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + ": the session holds no mission (created reserved and not refilled yet: rbp_session_refill_from_ecbs)") : RBP_OK;
}

// waits for the session's asynchronous joint run, if one is in flight; reports its error once
static int join_worker(rbp_session* s) {
    if (!s->worker.joinable()) return RBP_OK;
    s->worker.join();
    const int rc = s->worker_rc;
    s->worker_rc = RBP_OK;
    return rc ? fail(rc, "joint QP (asynchronous run): HIP error") : RBP_OK;
}

extern "C" {

const char* rbp_version(void) { return "rbp-mi355x 0.3 (gfx950)"; }
int rbp_abi_version(void) { return RBP_ABI_VERSION; }
size_t rbp_sizeof(int which) {
    switch (which) {
        case RBP_SIZEOF_WORLD: return sizeof(rbp_world);
        case RBP_SIZEOF_MISSION: return sizeof(rbp_mission);
        case RBP_SIZEOF_PARAM: return sizeof(rbp_param);
        case RBP_SIZEOF_PLAN: return sizeof(rbp_plan);
        case RBP_SIZEOF_COUNTERS: return sizeof(rbp_counters);
        case RBP_SIZEOF_DEVICE_ARRAYS: return sizeof(rbp_device_arrays);
        case RBP_SIZEOF_SOLVER_OPTS: return sizeof(rbp_solver_opts);
        case RBP_SIZEOF_ECBS_OUT: return sizeof(rbp_ecbs_out);
        case RBP_SIZEOF_REPORT: return sizeof(rbp_report);
        case RBP_SIZEOF_DYNAMICS: return sizeof(rbp_dynamics);
        case RBP_SIZEOF_CLEARANCE: return sizeof(rbp_clearance);
        case RBP_SIZEOF_SEPARATION: return sizeof(rbp_separation);
        case RBP_SIZEOF_SWEPT_CLEARANCE: return sizeof(rbp_swept_clearance);
        case RBP_SIZEOF_LIMITS: return sizeof(rbp_limits);
        case RBP_SIZEOF_SESSION_CAPACITY: return sizeof(rbp_session_capacity);
        default: return 0;
    }
}
const char* rbp_last_error(void) { return g_err.c_str(); }

int rbp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void rbp_param_defaults(rbp_param* p) {  // param.hpp:44-70
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->world_min[0] = -5, p->world_min[1] = -5, p->world_min[2] = 0;
    p->world_max[0] = 5, p->world_max[1] = 5, p->world_max[2] = 2.5;
    p->grid_xy_res = 0.3, p->grid_z_res = 0.6, p->grid_margin = 0.2, p->ecbs_w = 1.3;
    p->box_xy_res = 0.1, p->box_z_res = 0.1;
    p->time_scale = 1, p->time_step = 1, p->downwash = 2.0;
    p->n = 5, p->phi = 3, p->sequential = 0, p->batch_size = 4, p->batch_iter = 0, p->iteration = 1;
    p->log = 0;
    p->timescale_rule = RBP_TIMESCALE_ALL_REAL_ROOTS;
}

void rbp_solver_opts_defaults(rbp_solver_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->size = (int32_t)sizeof(*o);
    o->polish = 1, o->joint_wide_min_agents = 16, o->joint_corrector = 1, o->joint_schedule = 0;
    o->qp_schedule = 0, o->qp_variant = 0, o->qp_block_order = 1, o->qp_groups = 0, o->qp_rounds = 0;
    o->qp_far_slack = 0.7;
}

static int check_solver_opts(const rbp_solver_opts* o) {
    if (!o) return fail(RBP_ERR_BAD_ARGUMENT, "null solver options");
    if (o->size != (int32_t)sizeof(rbp_solver_opts)) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_solver_opts.size does not match this library (fill it with rbp_solver_opts_defaults)");
    if (o->joint_wide_min_agents < 0 || o->joint_schedule < 0 || o->joint_schedule > 3 || o->qp_schedule < 0 || o->qp_schedule > 2 ||
        !(o->qp_variant == 0 || o->qp_variant == 2 || o->qp_variant == 4) || o->qp_groups < 0 || o->qp_rounds < 0 || !(o->qp_far_slack == o->qp_far_slack))
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_solver_opts: field out of range");
    return RBP_OK;
}

static size_t al(size_t n) { return ((n + 255) & ~size_t(255)) + 256; }

// ---- what rbp_session_create and rbp_session_create_from_ecbs share: one set of parameter checks, one arena layout ----------------------
static int check_session_param(const rbp_param* param) {
    if (param->n != 5 || param->phi != 3) return fail(RBP_ERR_UNSUPPORTED_DEGREE, "RBPPlanner: n should be 5, phi 3");
    if (param->timescale_rule != RBP_TIMESCALE_ALL_REAL_ROOTS && param->timescale_rule != RBP_TIMESCALE_FIRST_EIGENVALUES)
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_param.timescale_rule must be RBP_TIMESCALE_ALL_REAL_ROOTS (0) or RBP_TIMESCALE_FIRST_EIGENVALUES (1)");
    // the SFC kernel caches at most SFC_MAXS sample keys per axis (isObstacleInBox walks the box on the box_res lattice,
    // rbp_corridor.hpp:47-63): reject worlds / resolutions that would be truncated instead of growing boxes through obstacles
    if (!(param->box_xy_res > 0) || !(param->box_z_res > 0)) return fail(RBP_ERR_BAD_ARGUMENT, "box/xy_res and box/z_res must be positive");
    for (int a = 0; a < 3; ++a) {
        const double res = a < 2 ? param->box_xy_res : param->box_z_res;
        const double ext = param->world_max[a] - param->world_min[a];
        if (!(ext >= 0) || std::ceil(ext / res) + 3 > SFC_MAXS)
            return fail(RBP_ERR_BAD_ARGUMENT, "world extent / box resolution exceeds the SFC sample cache (" + std::to_string(SFC_MAXS - 3) + " steps per axis)");
    }
    return RBP_OK;
}

// bytes of a session's arena: the grids it uploads (none for grids referenced in place) and every array session_carve takes
static size_t session_arena_bytes(size_t grid_bytes, int K, int N, int M, int MB) {
    const int P = M + 1, npair = N * (N - 1) / 2, oq = 6 * M;
    return grid_bytes + al(sizeof(DevWorld) * K) + 2 * al(sizeof(int) * K) + al(sizeof(float) * (size_t)K * N * P * 3) +
                         al(sizeof(double) * K * P) + 2 * al(sizeof(double) * (size_t)K * N * 9) + al(sizeof(double) * K * N) +
                         2 * al(sizeof(double) * (size_t)K * N * 3) + al(sizeof(int) * K * N) + al(sizeof(unsigned) * (size_t)K * SFC_MASK_WORDS) +
                         al(sizeof(double) * (size_t)K * N * MB * 6) + al(sizeof(double) * (size_t)K * N * MB) +
                         al(sizeof(float) * (size_t)K * npair * M * 3 + 16) + al(sizeof(double) * K * M) +
                         2 * al(sizeof(double) * (size_t)K * N * 3 * oq) + al(sizeof(int) * K) + al(sizeof(double) * K * SC_N) +
                         al(sizeof(unsigned long long) * K * CT_N) + al(sizeof(int) * K) + al(sizeof(unsigned long long) * K) + 4096;
}

// the arena of `total` bytes, the session's own or its context's, cleared before anything is written into it
static int session_reserve_arena(rbp_session* s, rbp_ctx* ctx, int device, size_t total) {
    if (ctx) {
        if (ctx->busy) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_ctx: the context's arena is in use by another session");
        if (ctx->device != device) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_ctx: context belongs to another device");
        if (ctx->cap < total) {  // grow (with headroom, so that a sequence of slightly different plans does not reallocate)
            if (ctx->base) (void)hipFree(ctx->base);
            ctx->base = nullptr, ctx->cap = 0;
            const size_t want = total + total / 4;
            hipError_t e = hipMalloc((void**)&ctx->base, want);
            if (e != hipSuccess) return fail(RBP_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
            ctx->cap = want;
        }
        s->ctx = ctx, ctx->busy = true;
        s->arena.base = ctx->base;
    } else {
        hipError_t e = hipMalloc((void**)&s->arena.base, total);
        if (e != hipSuccess) return fail(RBP_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    s->arena.size = total;
    // synchronous on purpose: small pageable host-to-device copies may be carried out by the CPU ahead of work queued on the
    // stream, so an asynchronous clear could wipe what the uploads below have just written
    HIP_TRY(hipMemset(s->arena.base, 0, total));
    HIP_TRY(hipDeviceSynchronize());
    return RBP_OK;
}

// words of LDS sfc_kernel reserves for the occupancy mask: the largest grid of the K worlds that fits
static int session_mask_words(const rbp_world* worlds, int K) {
    int mask_words = 0;
    for (int k = 0; k < K; ++k) {
        const size_t nc = (size_t)worlds[k].dim[0] * worlds[k].dim[1] * worlds[k].dim[2];
        const size_t words = ((((nc + 63) >> 6) * 2 + 2) + 3) & ~size_t(3);
        if (words <= SFC_MASK_WORDS) mask_words = std::max(mask_words, (int)words);
    }
    return mask_words;
}

// the shapes and parameters of DevSession (everything but its pointers) for K missions on `worlds`, strides M and MB; the session's capacity
static int session_describe(rbp_session* s, int device, const rbp_param* param, const rbp_world* worlds, int K, int N, int M, int MB) {
    const int npair = N * (N - 1) / 2;
    DevSession& d = s->d;
    d.K = K, d.N = N, d.M = M, d.max_boxes = MB, d.npair = npair;
    d.agent_begin = 0, d.agent_end = N;
    for (int a = 0; a < 3; ++a) {
        const double bres = a < 2 ? param->box_xy_res : param->box_z_res;
        d.sfc_cap[a] = std::min(SFC_MAXS, (int)std::ceil((param->world_max[a] - param->world_min[a]) / bres) + 4);
    }
    s->cap.K = K, s->cap.N = N, s->cap.M = M, s->cap.max_boxes = MB;
    d.sfc_mask_words = session_mask_words(worlds, K);
    {   // sfc_kernel keeps box_log [max_boxes][M + 1] per agent of a workgroup in LDS, beside the mask and the key lists: refuse here, with the
        // numbers, what the launch would refuse with a generic HIP error (the QP kernels take M <= QP_MAX_M = 128; the corridor's
        // bound depends on max_boxes, which defaults to M)
        int lds_max = 160 * 1024;
        (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
        s->lds_max = lds_max;
        const size_t need = corridor_lds_bytes(d);
        if (need > (size_t)std::max(lds_max, 64 * 1024))
            return fail(RBP_ERR_BAD_ARGUMENT, "Corridor: " + std::to_string(need) + " bytes of LDS per workgroup for max_boxes = " + std::to_string(MB) +
                                                  ", M = " + std::to_string(M) + " (box_log is [max_boxes][M + 1] per agent) exceed the device's " +
                                                  std::to_string(lds_max) + "; pass a smaller plan.max_boxes (the reference's corridors hold ~6-10 boxes per agent)");
    }
    for (int a = 0; a < 3; ++a) d.p.world_min[a] = param->world_min[a], d.p.world_max[a] = param->world_max[a];
    d.p.box_xy_res = param->box_xy_res, d.p.box_z_res = param->box_z_res, d.p.downwash = param->downwash;
    d.p.sequential = param->sequential, d.p.batch_size = param->batch_size, d.p.batch_iter = param->batch_iter;
    d.p.iteration = param->iteration, d.p.time_scale = param->time_scale;
    d.p.timescale_rule = param->timescale_rule;
    d.p.polish = 1, d.p.far_slack = 0.7;  // (rbp_solver_opts.polish / qp_far_slack of the run)
    return RBP_OK;
}

// The arrays of a session in its arena, after the grids it uploaded: the one layout of both constructors.  The arrays a constructor has to
// fill come back in `in`; DevSession gets every pointer.
struct SessionInputs {
    DevWorld* worlds;
    int *Mk, *MBk;
    float* init_traj;
    double *T, *start, *goal, *radius, *max_vel, *max_acc;
};
static int session_carve(rbp_session* s, SessionInputs& in) {
    Arena& A = s->arena;
    DevSession& d = s->d;
    const int K = d.K, N = d.N, M = d.M, MB = d.max_boxes, npair = d.npair, P = M + 1, oq = 6 * M;
    in.worlds = A.take<DevWorld>(K);
    in.Mk = A.take<int>(K);
    in.MBk = A.take<int>(K);
    in.init_traj = A.take<float>((size_t)K * N * P * 3);
    in.T = A.take<double>((size_t)K * P);
    in.start = A.take<double>((size_t)K * N * 9);
    in.goal = A.take<double>((size_t)K * N * 9);
    in.radius = A.take<double>((size_t)K * N);
    in.max_vel = A.take<double>((size_t)K * N * 3);
    in.max_acc = A.take<double>((size_t)K * N * 3);
    d.sfc_mask = A.take<unsigned>((size_t)K * SFC_MASK_WORDS);
    d.sfc_count = A.take<int>((size_t)K * N);
    d.sfc_box = A.take<double>((size_t)K * N * MB * 6);
    d.sfc_time = A.take<double>((size_t)K * N * MB);
    d.rsfc_normal = A.take<float>((size_t)K * npair * M * 3 + 4);
    d.rsfc_time = A.take<double>((size_t)K * M);
    d.ctrl = A.take<double>((size_t)K * N * 3 * oq);
    d.coef = A.take<double>((size_t)K * N * 3 * oq);
    d.status = A.take<int>(K);
    d.scalars = A.take<double>((size_t)K * SC_N);
    d.counters = A.take<unsigned long long>((size_t)K * CT_N);
    d.qp_order = A.take<int>(K);
    d.qp_cost = A.take<unsigned long long>(K);
    if (A.off > A.size) return fail(RBP_ERR_HIP, "arena overflow (internal sizing error)");
    d.worlds = in.worlds, d.Mk = in.Mk, d.MBk = in.MBk;
    d.init_traj = in.init_traj, d.T = in.T, d.start = in.start, d.goal = in.goal, d.radius = in.radius, d.max_vel = in.max_vel, d.max_acc = in.max_acc;
    return RBP_OK;
}

static int session_create_impl(rbp_session** out, int device, int K, const rbp_world* worlds, const rbp_mission* missions,
                               const rbp_param* param, const rbp_plan* plans, rbp_ctx* ctx) {
    if (!out || K <= 0 || !worlds || !missions || !param || !plans) return fail(RBP_ERR_BAD_ARGUMENT, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(RBP_ERR_NO_DEVICE, "no HIP device: the RBP path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(RBP_ERR_NO_DEVICE, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    // every mission keeps its own M = makespan + 2 (ecbs_planner.hpp:41-43) and box capacity; only N is common
    const int N = plans[0].N;
    int M = 0, MB = 0;  // session maxima = slot strides
    for (int k = 0; k < K; ++k) {
        if (plans[k].N != N || missions[k].N != N) return fail(RBP_ERR_BAD_ARGUMENT, "all missions of a session must share N");
        if (plans[k].N <= 0 || plans[k].M < 2 || plans[k].max_boxes <= 0)
            return fail(RBP_ERR_BAD_ARGUMENT, "need N >= 1, M >= 2, max_boxes >= 1");
        if (!plans[k].T || !plans[k].init_traj || !worlds[k].dist)
            return fail(RBP_ERR_BAD_ARGUMENT, "plan.T / plan.init_traj / world.dist must be set");
        M = std::max(M, (int)plans[k].M), MB = std::max(MB, (int)plans[k].max_boxes);
    }
    if (int rc = check_session_param(param)) return rc;
    const BatchSchedule sched = batch_schedule(param->sequential, param->batch_size, param->batch_iter, N);
    const int bs = sched.bs, biter = sched.biter;

    struct Guard {  // every error path below releases the session (and with it the arena)
        rbp_session* s;
        ~Guard() {
            if (s) rbp_session_destroy(s);
        }
    } guard{new rbp_session()};
    rbp_session* s = guard.s;
    s->device = device;
    s->param = *param;
    s->Mk.resize(K), s->MBk.resize(K);
    for (int k = 0; k < K; ++k) s->Mk[k] = plans[k].M, s->MBk[k] = plans[k].max_boxes;
    const int P = M + 1, npair = N * (N - 1) / 2;
    s->bs = bs, s->biter = biter;
    if (ctx) s->opts = ctx->opts;
    {
        hipDeviceProp_t prop;
        s->n_cu = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
    }

    // a grid may already lie in HBM (rbp_dev_worlds, a caller's tensor): such a grid is used where it is.  A pointer the runtime does not
    // know is reported as an error or as unregistered memory, depending on the runtime: both mean host
    std::vector<char> on_device(K, 0);
    for (int k = 0; k < K; ++k) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, worlds[k].dist) != hipSuccess) {
            (void)hipGetLastError();  // (the error is sticky)
            continue;
        }
        if (at.type != hipMemoryTypeDevice) continue;
        if (at.device != device) return fail(RBP_ERR_BAD_ARGUMENT, "world.dist of mission " + std::to_string(k) + " lies on device " + std::to_string(at.device) +
                                                                       ", the session on device " + std::to_string(device));
        on_device[k] = 1;
    }
    // missions that share a map (same grid pointer and shape, e.g. several passes of a map sweep) share one device copy
    auto same_grid = [&](int a, int b) {
        return worlds[a].dist == worlds[b].dist && worlds[a].dim[0] == worlds[b].dim[0] && worlds[a].dim[1] == worlds[b].dim[1] &&
               worlds[a].dim[2] == worlds[b].dim[2];
    };
    std::vector<int> grid_of(K);
    for (int k = 0; k < K; ++k) {
        grid_of[k] = k;
        for (int j = 0; j < k; ++j)
            if (grid_of[j] == j && same_grid(j, k)) {
                grid_of[k] = j;
                break;
            }
    }
    size_t grid_bytes = 0;
    for (int k = 0; k < K; ++k)
        if (grid_of[k] == k && !on_device[k]) grid_bytes += al(sizeof(float) * (size_t)worlds[k].dim[0] * worlds[k].dim[1] * worlds[k].dim[2]);
    const size_t total = session_arena_bytes(grid_bytes, K, N, M, MB);
    if (int rc = session_reserve_arena(s, ctx, device, total)) return rc;
    if (int rc = session_describe(s, device, param, worlds, K, N, M, MB)) return rc;
    Arena& A = s->arena;
    s->worlds_h.resize(K);
#define UP(dst, src, bytes) HIP_TRY(hipMemcpy((void*)(dst), (src), (bytes), hipMemcpyHostToDevice))
    for (int k = 0; k < K; ++k) {
        size_t n = (size_t)worlds[k].dim[0] * worlds[k].dim[1] * worlds[k].dim[2];
        float* g;
        if (on_device[k]) {
            g = const_cast<float*>(worlds[k].dist);  // referenced in place: the caller keeps it alive (include/rbp.h)
        } else if (grid_of[k] == k) {
            g = A.take<float>(n);
            UP(g, worlds[k].dist, sizeof(float) * n);
        } else {
            g = const_cast<float*>(s->worlds_h[grid_of[k]].dist);
        }
        DevWorld& w = s->worlds_h[k];
        for (int a = 0; a < 3; ++a) w.dim[a] = worlds[k].dim[a], w.key_min[a] = worlds[k].key_min[a];
        w.res = worlds[k].res;
        w.dist = g;
    }
    SessionInputs in;
    if (int rc = session_carve(s, in)) return rc;
    UP(in.worlds, s->worlds_h.data(), sizeof(DevWorld) * K);
    UP(in.Mk, s->Mk.data(), sizeof(int) * K);
    UP(in.MBk, s->MBk.data(), sizeof(int) * K);
    float* traj = in.init_traj;
    double *T = in.T, *start = in.start, *goal = in.goal, *radius = in.radius, *mv = in.max_vel, *ma = in.max_acc;
    bool have_corr = true;
    for (int k = 0; k < K; ++k)
        have_corr = have_corr && plans[k].sfc_count && plans[k].sfc_box && plans[k].sfc_time && plans[k].rsfc_normal && plans[k].rsfc_time;
    // corridor outputs handed in as planner inputs only count if some agent actually has boxes
    if (have_corr) {
        bool any = false;
        for (int k = 0; k < K && !any; ++k)
            for (int a = 0; a < N && !any; ++a) any = plans[k].sfc_count[a] > 0;
        have_corr = any;
    }
    s->have_corridor_inputs = have_corr;
    if (have_corr) {
        s->sfc_count0.assign((size_t)K * N, 0), s->sfc_box0.assign((size_t)K * N * MB * 6, 0.0), s->sfc_time0.assign((size_t)K * N * MB, 0.0);
        s->rsfc_normal0.assign((size_t)K * npair * M * 3, 0.0f), s->rsfc_time0.assign((size_t)K * M, 0.0);
    }
    for (int k = 0; k < K; ++k) {
        const int Mq = plans[k].M, Pq = Mq + 1, MBq = plans[k].max_boxes;
        UP(traj + (size_t)k * N * P * 3, plans[k].init_traj, sizeof(float) * (size_t)N * Pq * 3);
        UP(T + (size_t)k * P, plans[k].T, sizeof(double) * Pq);
        UP(start + (size_t)k * N * 9, missions[k].start, sizeof(double) * N * 9);
        UP(goal + (size_t)k * N * 9, missions[k].goal, sizeof(double) * N * 9);
        UP(radius + (size_t)k * N, missions[k].radius, sizeof(double) * N);
        UP(mv + (size_t)k * N * 3, missions[k].max_vel, sizeof(double) * N * 3);
        UP(ma + (size_t)k * N * 3, missions[k].max_acc, sizeof(double) * N * 3);
        if (have_corr) {
            memcpy(&s->sfc_count0[(size_t)k * N], plans[k].sfc_count, sizeof(int) * N);
            repack_boxes(&s->sfc_box0[(size_t)k * N * MB * 6], MB, plans[k].sfc_box, MBq, N, 6);
            repack_boxes(&s->sfc_time0[(size_t)k * N * MB], MB, plans[k].sfc_time, MBq, N, 1);
            memcpy(&s->rsfc_normal0[(size_t)k * npair * M * 3], plans[k].rsfc_normal, sizeof(float) * (size_t)npair * Mq * 3);
            memcpy(&s->rsfc_time0[(size_t)k * M], plans[k].rsfc_time, sizeof(double) * Mq);
        }
    }
#undef UP
    int rc = rbp_session_reset(s, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    guard.s = nullptr;
    *out = s;
    return RBP_OK;
}

int rbp_session_create(rbp_session** out, int device, int K, const rbp_world* worlds, const rbp_mission* missions,
                       const rbp_param* param, const rbp_plan* plans) {
    return session_create_impl(out, device, K, worlds, missions, param, plans, nullptr);
}

int rbp_session_create_in(rbp_ctx* ctx, rbp_session** out, int K, const rbp_world* worlds, const rbp_mission* missions,
                          const rbp_param* param, const rbp_plan* plans) {
    if (!ctx) return fail(RBP_ERR_BAD_ARGUMENT, "null context");
    return session_create_impl(out, ctx->device, K, worlds, missions, param, plans, ctx);
}

// A session of the missions a device search solved (rbp_dev_ecbs, kernels/ecbs.hip), built where its results lie: the worlds are the
// resident grids of the search's set, referenced in place like any device grid above; T, init_traj and the mission arrays are written
// into the arena by the two kernels of kernels/handoff.hip.  Checks, arena and layout are session_create_impl's.
int rbp_session_create_from_ecbs(rbp_session** out, const rbp_dev_ecbs* e, const rbp_param* param, int32_t max_boxes, int32_t* slot_of) {
    const char* who = "rbp_session_create_from_ecbs: ";
    if (out) *out = nullptr;
    if (!out || !e || !param) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "need out, the search's handle and param");
    if (!e->have_limits) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "the search's missions came without max_vel / max_acc");
    const int N = e->N, device = e->device;
    std::vector<int> src;  // the missions the session holds
    for (int k = 0; k < e->K; ++k) {
        if (slot_of) slot_of[k] = e->status_h[k] == 0 ? (int)src.size() : -1;
        if (e->status_h[k] == 0) src.push_back(k);
    }
    const int K = (int)src.size();
    if (K == 0) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "no mission of the search has status 0");
    int M = 0, MB = 0;  // session maxima = slot strides
    std::vector<rbp_world> worlds(K);
    std::vector<int> Mk(K), MBk(K);
    for (int j = 0; j < K; ++j) {
        Mk[j] = e->M_h[src[j]], MBk[j] = max_boxes > 0 ? max_boxes : Mk[j];
        M = std::max(M, Mk[j]), MB = std::max(MB, MBk[j]);
        if (int rc = rbp_dev_worlds_get(e->ws, e->world_index[src[j]], &worlds[j])) return rc;
    }
    if (int rc = check_session_param(param)) return rc;
    HIP_TRY(hipSetDevice(device));
    const BatchSchedule sched = batch_schedule(param->sequential, param->batch_size, param->batch_iter, N);

    struct Guard {  // every error path below releases the session (and with it the arena)
        rbp_session* s;
        ~Guard() {
            if (s) rbp_session_destroy(s);
        }
    } guard{new rbp_session()};
    rbp_session* s = guard.s;
    s->device = device;
    s->param = *param;
    s->Mk = Mk, s->MBk = MBk;
    s->bs = sched.bs, s->biter = sched.biter;
    {
        hipDeviceProp_t prop;
        s->n_cu = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    if (int rc = session_reserve_arena(s, nullptr, device, session_arena_bytes(0, K, N, M, MB))) return rc;  // (cleared, and the clear complete)
    if (int rc = session_describe(s, device, param, worlds.data(), K, N, M, MB)) return rc;
    s->worlds_h.resize(K);
    for (int j = 0; j < K; ++j) {
        DevWorld& w = s->worlds_h[j];
        for (int a = 0; a < 3; ++a) w.dim[a] = worlds[j].dim[a], w.key_min[a] = worlds[j].key_min[a];
        w.res = worlds[j].res;
        w.dist = worlds[j].dist;  // referenced in place: the set of worlds outlives the session (include/rbp.h)
    }
    SessionInputs in;
    if (int rc = session_carve(s, in)) return rc;
    HIP_TRY(hipMemcpy(in.worlds, s->worlds_h.data(), sizeof(DevWorld) * K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.Mk, s->Mk.data(), sizeof(int) * K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in.MBk, s->MBk.data(), sizeof(int) * K, hipMemcpyHostToDevice));
    DeviceBuffers b;  // the source list, freed when the kernels below have completed
    const int* d_src = b.upload(src);
    HIP_TRY(b.err);
    if (int rc = launch_ecbs_plan_write(*e, K, d_src, in.Mk, M + 1, true, in.T, in.init_traj, nullptr)) return rc;
    if (int rc = launch_ecbs_mission_gather(*e, K, d_src, in.start, in.goal, in.radius, in.max_vel, in.max_acc, nullptr)) return rc;
    s->have_corridor_inputs = false;
    s->ws = e->ws;
    if (int rc = rbp_session_reset(s, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    guard.s = nullptr;
    *out = s;
    return RBP_OK;
}

// The staging block of the refills and its device twin, sized for the capacity, and the event a refill waits on before it reuses the block.
static int session_reserve_stage(rbp_session* s) {
    if (s->stage_h) return RBP_OK;
    const size_t bytes = RefillStage(s->cap.K).bytes();
    HIP_TRY(hipHostMalloc((void**)&s->stage_h, bytes, hipHostMallocDefault));
    HIP_TRY(hipMalloc((void**)&s->stage_d, bytes));
    HIP_TRY(hipEventCreateWithFlags(&s->stage_ev, hipEventDisableTiming));
    return RBP_OK;
}

// An empty session of a stated capacity on the device of a set of worlds: the arena, laid out and cleared as both constructors above do it,
// and the refills' staging block.  rbp_session_refill_from_ecbs gives it its missions.
int rbp_session_create_reserved(rbp_session** out, const rbp_dev_worlds* ws, const rbp_session_capacity* cap, const rbp_param* param) {
    const char* who = "rbp_session_create_reserved: ";
    if (out) *out = nullptr;
    if (!out || !ws || !cap || !param) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "need out, the set of worlds, the capacity and param");
    if (cap->K < 1 || cap->N < 1 || cap->M < 2 || cap->max_boxes < 1) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "need K >= 1, N >= 1, M >= 2, max_boxes >= 1");
    if (int rc = check_session_param(param)) return rc;
    const int K = cap->K, N = cap->N, M = cap->M, MB = cap->max_boxes, W = rbp_dev_worlds_count(ws);
    if (W < 1) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "the set of worlds is empty");
    const int device = dev_worlds_device(ws);
    // the shapes session_describe looks at (the occupancy mask's words, the LDS of sfc_kernel) for the set's grids; a refill states them again
    // for the worlds of its missions
    std::vector<rbp_world> worlds(K);
    for (int k = 0; k < K; ++k)
        if (int rc = rbp_dev_worlds_get(ws, k % W, &worlds[k])) return rc;
    HIP_TRY(hipSetDevice(device));
    const BatchSchedule sched = batch_schedule(param->sequential, param->batch_size, param->batch_iter, N);

    struct Guard {  // every error path below releases the session (and with it the arena)
        rbp_session* s;
        ~Guard() {
            if (s) rbp_session_destroy(s);
        }
    } guard{new rbp_session()};
    rbp_session* s = guard.s;
    s->device = device;
    s->param = *param;
    s->bs = sched.bs, s->biter = sched.biter;
    {
        hipDeviceProp_t prop;
        s->n_cu = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    if (int rc = session_reserve_arena(s, nullptr, device, session_arena_bytes(0, K, N, M, MB))) return rc;  // (cleared, and the clear complete)
    if (int rc = session_describe(s, device, param, worlds.data(), K, N, M, MB)) return rc;
    SessionInputs in;
    if (int rc = session_carve(s, in)) return rc;
    if (int rc = session_reserve_stage(s)) return rc;
    s->d.K = 0, s->empty = true;  // no mission yet
    s->ws = ws;
    s->have_corridor_inputs = false;
    guard.s = nullptr;
    *out = s;
    return RBP_OK;
}

int rbp_session_capacity_of(const rbp_session* s, rbp_session_capacity* out) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_capacity_of: null argument");
    *out = s->cap;
    return RBP_OK;
}

// The missions of a search into the slots 0 .. K'-1 of a session that exists.  Every check comes before anything of the session changes;
// then the host's copy of the per-mission state follows, the staging block goes up in one asynchronous copy, and one kernel does the rest.
int rbp_session_refill_from_ecbs(rbp_session* s, const rbp_dev_ecbs* e, int32_t max_boxes, int32_t* slot_of, void* stream) {
    const char* who = "rbp_session_refill_from_ecbs: ";
    if (!s || !e) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "need the session and the search's handle");
    if (int jrc = join_worker(s)) return jrc;  // (a failed asynchronous solve: its error, and the session stays as it is)
    if (!e->have_limits) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "the search's missions came without max_vel / max_acc");
    if (s->shard.nranks == 2) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "a session sharded over two ranks (rbp_session_shard_joint) is not refilled");
    if (e->device != s->device)
        return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "the search lies on device " + std::to_string(e->device) + ", the session on device " + std::to_string(s->device));
    const rbp_session_capacity& cap = s->cap;
    if (e->N != cap.N) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "the search's missions have " + std::to_string(e->N) + " agents, the session's " + std::to_string(cap.N));
    if (s->ws && e->ws != s->ws) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "the search ran on another set of worlds than the session's");
    if (!s->ws) {  // a session of rbp_session_create / _create_in: refillable when every grid it plans on is a grid of the search's set
        const int W = rbp_dev_worlds_count(e->ws);
        for (const DevWorld& w : s->worlds_h) {
            bool found = false;
            for (int i = 0; i < W && !found; ++i) {
                rbp_world g;
                found = rbp_dev_worlds_get(e->ws, i, &g) == RBP_OK && g.dist == w.dist;
            }
            if (!found) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "the session's grids are not those of the search's set of worlds (rbp_dev_worlds)");
        }
    }
    std::vector<int> src, slots(e->K);
    for (int k = 0; k < e->K; ++k) {
        slots[k] = e->status_h[k] == 0 ? (int)src.size() : -1;
        if (e->status_h[k] == 0) src.push_back(k);
    }
    if (slot_of) std::copy(slots.begin(), slots.end(), slot_of);
    const int K = (int)src.size();
    if (K == 0) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "no mission of the search has status 0");
    if (K > cap.K) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + std::to_string(K) + " missions with status 0, the session's capacity is " + std::to_string(cap.K));
    std::vector<rbp_world> worlds(K);
    std::vector<int> Mk(K), MBk(K);
    for (int j = 0; j < K; ++j) {
        Mk[j] = e->M_h[src[j]], MBk[j] = max_boxes > 0 ? max_boxes : Mk[j];
        if (Mk[j] > cap.M || MBk[j] > cap.max_boxes)
            return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "mission " + std::to_string(src[j]) + ": M = " + std::to_string(Mk[j]) + ", max_boxes = " + std::to_string(MBk[j]) +
                                                  " exceed the session's strides M = " + std::to_string(cap.M) + ", max_boxes = " + std::to_string(cap.max_boxes));
        if (int rc = rbp_dev_worlds_get(e->ws, e->world_index[src[j]], &worlds[j])) return rc;
    }
    DevSession nd = s->d;  // the occupancy mask's words are those of the new missions' worlds, as in a fresh session of them
    nd.K = K, nd.sfc_mask_words = session_mask_words(worlds.data(), K);
    if (corridor_lds_bytes(nd) > (size_t)std::max(s->lds_max, 64 * 1024))
        return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "Corridor: " + std::to_string(corridor_lds_bytes(nd)) + " bytes of LDS per workgroup for the new missions' grids exceed the device's " +
                                              std::to_string(s->lds_max));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = session_reserve_stage(s)) return rc;  // (a session that was not created reserved: its first refill)
    if (s->stage_busy) HIP_TRY(hipEventSynchronize(s->stage_ev));  // the previous refill's copy has left the staging block
    const RefillStage L(cap.K);
    DevWorld* wd = reinterpret_cast<DevWorld*>(s->stage_h + L.worlds());
    for (int j = 0; j < K; ++j) {
        DevWorld& w = wd[j];
        for (int a = 0; a < 3; ++a) w.dim[a] = worlds[j].dim[a], w.key_min[a] = worlds[j].key_min[a];
        w.res = worlds[j].res;
        w.dist = worlds[j].dist;  // referenced in place: the set of worlds outlives the session (include/rbp.h)
    }
    memcpy(s->stage_h + L.src(), src.data(), sizeof(int) * K);
    memcpy(s->stage_h + L.Mk(), Mk.data(), sizeof(int) * K);
    memcpy(s->stage_h + L.MBk(), MBk.data(), sizeof(int) * K);
    HIP_TRY(hipMemcpyAsync(s->stage_d, s->stage_h, L.bytes(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->stage_ev, st));
    s->stage_busy = true;
    if (int rc = launch_session_refill(*e, nd, K, s->stage_d, cap.K, 8 * s->n_cu, st)) return rc;
    // The batch QP kernels leave parts of a mission's workspace as the reservation cleared them (kernels/qp_batch.inc), and which parts
    // depends on the mission: the blocks of the refilled slots are cleared again, on the stream, as a fresh session's would be
    if (s->qp_ws) HIP_TRY(hipMemsetAsync(s->qp_ws, 0, s->qp_ws_per_mission * (size_t)K, st));
    s->d = nd;
    s->Mk = Mk, s->MBk = MBk;
    s->worlds_h.assign(wd, wd + K);
    s->ws = e->ws;
    s->have_corridor_inputs = false;
    s->last_stages = 0;
    s->empty = false;
    return RBP_OK;
}

// ---- the other source of a refill: a caller's own plans, staged (common/plan_stage.h) ------------------------------------------------
static int check_capacity(const char* who, const rbp_session_capacity* cap) {
    if (!cap) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "null capacity");
    if (cap->K < 1 || cap->N < 1 || cap->M < 2 || cap->max_boxes < 1) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "need K >= 1, N >= 1, M >= 2, max_boxes >= 1");
    return RBP_OK;
}

int rbp_plan_stage_bytes(const rbp_session_capacity* cap, int32_t K, size_t* bytes) {
    const char* who = "rbp_plan_stage_bytes: ";
    if (bytes) *bytes = 0;
    if (int rc = check_capacity(who, cap)) return rc;
    if (K < 1 || !bytes) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "need K >= 1 and bytes");
    *bytes = plan_stage::mission_bytes(cap->N, cap->M) * (size_t)K;
    return RBP_OK;
}

// the block a session reserves for `bytes` = 0: its capacity's missions in one round, up to RBP_REFILL_STAGE_BYTES (one mission at the least)
static size_t default_plan_stage_bytes(const rbp_session* s) {
    const size_t one = plan_stage::mission_bytes(s->cap.N, s->cap.M);
    return std::max(one, std::min(one * (size_t)s->cap.K, (size_t)RBP_REFILL_STAGE_BYTES));
}

int rbp_session_reserve_plan_stage(rbp_session* s, size_t bytes) {
    const char* who = "rbp_session_reserve_plan_stage: ";
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "null session");
    const size_t one = plan_stage::mission_bytes(s->cap.N, s->cap.M), want = bytes ? bytes : default_plan_stage_bytes(s);
    if (want < one)
        return fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + std::to_string(want) + " bytes are less than one mission of the session's capacity takes (" + std::to_string(one) + ")");
    if (s->pstage_h)
        return want == s->pstage_bytes ? RBP_OK
                                       : fail(RBP_ERR_BAD_ARGUMENT, std::string(who) + "the block has been reserved with " + std::to_string(s->pstage_bytes) + " bytes, not " + std::to_string(want));
    HIP_TRY(hipSetDevice(s->device));
    char *h = nullptr, *d = nullptr;
    hipEvent_t ev = nullptr;
    hipError_t e = hipHostMalloc((void**)&h, want, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&d, want);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) {  // all of the block or nothing
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        return fail(RBP_ERR_HIP, std::string(who) + std::to_string(want) + " bytes of pinned and device memory: " + hipGetErrorString(e));
    }
    s->pstage_h = h, s->pstage_d = d, s->pstage_ev = ev, s->pstage_bytes = want, s->pstage_busy = false;
    return RBP_OK;
}

// K of a caller's missions into the slots 0 .. K-1 of a session that exists.  Every check comes before anything of the session changes;
// then the missions go up in rounds of the staging block: pack, one asynchronous copy, one launch of session_refill_plans_kernel.
int rbp_session_refill_from_plans(rbp_session* s, int32_t K, const rbp_world* worlds, const rbp_mission* missions, const rbp_plan* plans, void* stream) {
    const std::string who = "rbp_session_refill_from_plans: ";
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, who + "null session");
    if (K < 1) return fail(RBP_ERR_BAD_ARGUMENT, who + "need K >= 1");
    if (!worlds || !missions || !plans) return fail(RBP_ERR_BAD_ARGUMENT, who + "need worlds, missions and plans");
    if (int jrc = join_worker(s)) return jrc;  // (a failed asynchronous solve: its error, and the session stays as it is)
    if (s->shard.nranks == 2) return fail(RBP_ERR_BAD_ARGUMENT, who + "a session sharded over two ranks (rbp_session_shard_joint) is not refilled");
    const rbp_session_capacity& cap = s->cap;
    if (K > cap.K) return fail(RBP_ERR_BAD_ARGUMENT, who + std::to_string(K) + " missions, the session's capacity is " + std::to_string(cap.K));
    auto refuse = [&](int k, const std::string& what) { return fail(RBP_ERR_BAD_ARGUMENT, who + "mission " + std::to_string(k) + ": " + what); };
    for (int k = 0; k < K; ++k) {
        const rbp_plan& p = plans[k];
        const rbp_mission& m = missions[k];
        if (p.N != cap.N) return refuse(k, "plan.N = " + std::to_string(p.N) + ", the session's missions have " + std::to_string(cap.N) + " agents");
        if (m.N != cap.N) return refuse(k, "mission.N = " + std::to_string(m.N) + ", the session's missions have " + std::to_string(cap.N) + " agents");
        if (p.M < 2 || p.M > cap.M) return refuse(k, "plan.M = " + std::to_string(p.M) + " outside [2, the session's stride " + std::to_string(cap.M) + "]");
        if (p.max_boxes < 1 || p.max_boxes > cap.max_boxes)
            return refuse(k, "plan.max_boxes = " + std::to_string(p.max_boxes) + " outside [1, the session's stride " + std::to_string(cap.max_boxes) + "]");
        if (!p.T) return refuse(k, "plan.T is null");
        if (!p.init_traj) return refuse(k, "plan.init_traj is null");
        if (!m.start) return refuse(k, "mission.start is null");
        if (!m.goal) return refuse(k, "mission.goal is null");
        if (!m.radius) return refuse(k, "mission.radius is null");
        if (!m.max_vel) return refuse(k, "mission.max_vel is null");
        if (!m.max_acc) return refuse(k, "mission.max_acc is null");
        if (!worlds[k].dist) return refuse(k, "world.dist is null");
    }
    HIP_TRY(hipSetDevice(s->device));
    for (int k = 0; k < K; ++k) {  // a refill uploads no grid: every grid lies on the session's device already
        if (k > 0 && worlds[k].dist == worlds[k - 1].dist) continue;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, worlds[k].dist) != hipSuccess) {  // a pointer the runtime does not know: host (the error is sticky)
            (void)hipGetLastError();
            return refuse(k, "world.dist is a host pointer; a refill takes grids that lie on the device (rbp_dev_worlds)");
        }
        if (at.type != hipMemoryTypeDevice) return refuse(k, "world.dist is a host pointer; a refill takes grids that lie on the device (rbp_dev_worlds)");
        if (at.device != s->device) return refuse(k, "world.dist lies on device " + std::to_string(at.device) + ", the session on device " + std::to_string(s->device));
    }
    DevSession nd = s->d;  // the occupancy mask's words are those of the new missions' worlds, as in a fresh session of them
    nd.K = K, nd.sfc_mask_words = session_mask_words(worlds, K);
    if (corridor_lds_bytes(nd) > (size_t)std::max(s->lds_max, 64 * 1024))
        return fail(RBP_ERR_BAD_ARGUMENT, who + "Corridor: " + std::to_string(corridor_lds_bytes(nd)) + " bytes of LDS per workgroup for the new missions' grids exceed the device's " +
                                              std::to_string(s->lds_max));
    if (!s->pstage_h)
        if (int rc = rbp_session_reserve_plan_stage(s, 0)) return rc;  // (not reserved up front: the first refill from plans)
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> Mk(K), MBk(K);
    std::vector<DevWorld> wd(K);
    for (int k = 0; k < K; ++k) {
        Mk[k] = plans[k].M, MBk[k] = plans[k].max_boxes;
        DevWorld& w = wd[k];
        for (int a = 0; a < 3; ++a) w.dim[a] = worlds[k].dim[a], w.key_min[a] = worlds[k].key_min[a];
        w.res = worlds[k].res;
        w.dist = worlds[k].dist;  // referenced in place: the caller keeps it alive until the next refill (include/rbp.h)
    }
    std::vector<plan_stage::Source> src;
    for (int j0 = 0; j0 < K;) {
        const int j1 = plan_stage::round_end(Mk.data(), K, cap.N, j0, s->pstage_bytes);  // (> j0: the block holds a mission of the capacity's shape)
        if (j1 <= j0) return fail(RBP_ERR_HIP, who + "a mission does not fit the staging block (internal sizing error)");
        src.resize(j1 - j0);
        for (int j = j0; j < j1; ++j)
            src[j - j0] = plan_stage::Source{Mk[j], MBk[j], &wd[j], plans[j].T, plans[j].init_traj, missions[j].start, missions[j].goal, missions[j].radius,
                                             missions[j].max_vel, missions[j].max_acc};
        if (s->pstage_busy) HIP_TRY(hipEventSynchronize(s->pstage_ev));  // the previous copy has left the block; stream order protects its twin
        const size_t bytes = plan_stage::pack_round(s->pstage_h, src.data(), j1 - j0, cap.N);
        HIP_TRY(hipMemcpyAsync(s->pstage_d, s->pstage_h, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(s->pstage_ev, st));
        s->pstage_busy = true;
        if (int rc = launch_session_refill_plans(nd, j0, j1 - j0, s->pstage_d, 8 * s->n_cu, st)) return rc;
        j0 = j1;
    }
    // (the QP workspace blocks of the refilled slots: as rbp_session_refill_from_ecbs clears them)
    if (s->qp_ws) HIP_TRY(hipMemsetAsync(s->qp_ws, 0, s->qp_ws_per_mission * (size_t)K, st));
    s->d = nd;
    s->Mk = Mk, s->MBk = MBk;
    s->worlds_h = wd;
    s->have_corridor_inputs = false;
    s->last_stages = 0;
    s->empty = false;
    return RBP_OK;
}

// T, the SFC end times and the RSFC times are never rescaled on the device (timescale_kernel only records the factor and
// rescales the coefficients; rbp_session_download applies it to its host copies), so a session can be re-run as it is:
// reset clears the per-run status / diagnostics and puts back corridor inputs the caller uploaded, in case a CORRIDOR
// stage overwrote them.
int rbp_session_reset(rbp_session* s, void* stream) {
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, "null session");
    if (int jrc = join_worker(s)) return jrc;
    hipStream_t st = (hipStream_t)stream;
    const DevSession& d = s->d;
    const int K = d.K, N = d.N, M = d.M, MB = d.max_boxes;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(d.status, 0, sizeof(int) * K, st));
    HIP_TRY(hipMemsetAsync(d.scalars, 0, sizeof(double) * K * SC_N, st));
    HIP_TRY(hipMemsetAsync(d.counters, 0, sizeof(unsigned long long) * K * CT_N, st));
    if (s->have_corridor_inputs) {
        HIP_TRY(hipMemcpyAsync(d.sfc_count, s->sfc_count0.data(), sizeof(int) * (size_t)K * N, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d.sfc_box, s->sfc_box0.data(), sizeof(double) * (size_t)K * N * MB * 6, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d.sfc_time, s->sfc_time0.data(), sizeof(double) * (size_t)K * N * MB, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d.rsfc_normal, s->rsfc_normal0.data(), sizeof(float) * (size_t)K * d.npair * M * 3, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d.rsfc_time, s->rsfc_time0.data(), sizeof(double) * (size_t)K * M, hipMemcpyHostToDevice, st));
    }
    return RBP_OK;
}

int rbp_session_set_agent_range(rbp_session* s, int32_t agent_begin, int32_t agent_end) {
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, "null session");
    if (int jrc = join_worker(s)) return jrc;
    if (agent_begin < 0 || agent_end < agent_begin || agent_end > s->d.N) return fail(RBP_ERR_BAD_ARGUMENT, "agent range outside [0, N]");
    s->d.agent_begin = agent_begin, s->d.agent_end = agent_end;
    return RBP_OK;
}

// The QP workspace of a PLANNER run.  Which solver runs -- and with it the workspace layout -- depends on the plan and on the session's
// solver options; the workspace is reserved here, by the first run that needs it (a corridor-only session reserves nothing), in the
// session's own allocation or its context's (kept across the context's sessions, grown on demand), and cleared once.
static int ensure_planner_workspace(rbp_session* s, hipStream_t st) {
    const DevSession& d = s->d;
    const int N = d.N, M = d.M, K = s->cap.K;  // (reserved for the capacity: a refill may bring up to cap.K missions)
    const rbp_solver_opts& o = s->opts;
    // The joint QP of a mission (plan/sequential = false: one batch of all N agents) is spread over the whole chip by kernels/jqp.hip when it
    // is wide enough to pay for a launch per phase (default: 16 agents or more, i.e. knot blocks of order >= 144).  Measured
    // (tools/gpu_joint_sweep.py, one mission / 250 / 1000 resident): 16 agents 0.067 s against 0.283 s, 9.2 k against 8.0 k, 11.2 k against
    // 7.4 k agent-trajectories/s; 32 agents 0.105 s against 1.6 s, and the one-workgroup polish (<= 256 candidate rows) accepts none of the 50
    // maps there; 8 agents: 0.038 s against 0.062 s alone but 10.6 k against 18.1 k at 250 resident -- below 16 agents a workgroup per mission
    // stays.  The grid-wide solver has no limit on N.
    const bool joint_wide = !s->param.sequential && s->biter > 0 && N >= 2 && o.joint_wide_min_agents > 0 && N >= o.joint_wide_min_agents;
    if (!joint_wide) {
        // a batch wider than the one-workgroup kernel factorises (the joint QP of a mission with more than planner_max_batch() agents), or a
        // mission with more than QP_MAX_M segments (the factor chains' LDS progress words sit behind 64 per-step assembly counters)
        if (M > QP_MAX_M) return fail(RBP_ERR_BAD_ARGUMENT, "more than " + std::to_string(QP_MAX_M) + " segments per mission are not supported by the QP kernel");
        if (s->biter > 0 && s->bs > planner_max_batch())
            return fail(RBP_ERR_BAD_ARGUMENT, "batch wider than " + std::to_string(planner_max_batch()) +
                                                  " agents (joint QP of a large mission) is not supported by the one-workgroup QP kernel "
                                                  "(rbp_solver_opts.joint_wide_min_agents selects the grid-wide solver)");
    }
    // Every mission's workspace of the batch QP kernels starts on a 128-byte line: the knots' factors (QpWs::Lf, kernels/knot_factor_layout.h) are
    // carved in whole lines from there.  planner_workspace_bytes_* round to 256 bytes already; the stride is rounded here all the same, and the
    // base below, inside the 256 spare bytes of the allocation.
    const size_t per = joint_wide ? joint_workspace_bytes(N, M)
                                  : (std::max(planner_workspace_bytes_w2(N, M, s->bs), planner_workspace_bytes_w4(N, M, s->bs)) + 127) & ~size_t(127);
    s->joint_wide = joint_wide;
    if (s->qp_ws && s->ws_joint == joint_wide && s->qp_ws_per_mission == per) return RBP_OK;
    const size_t total = per * (size_t)K + 256;
    auto too_large = [&](hipError_t e) {
        return fail(RBP_ERR_HIP, "QP workspace: " + std::to_string(total) + " bytes (" + std::to_string(K) + " missions x " + std::to_string(per) +
                                     " bytes for " + (joint_wide ? "the grid-wide joint solver" : "the batch QP kernels") + ") could not be reserved: " +
                                     hipGetErrorString(e));
    };
    char* base = nullptr;
    if (s->ctx) {
        rbp_ctx* c = s->ctx;
        if (c->ws_cap < total) {
            HIP_TRY(hipStreamSynchronize(st));
            if (c->ws_base) (void)hipFree(c->ws_base);
            c->ws_base = nullptr, c->ws_cap = 0;
            const size_t want = total + total / 4;
            hipError_t e = hipMalloc((void**)&c->ws_base, want);
            if (e != hipSuccess) return too_large(e);
            c->ws_cap = want;
        }
        base = c->ws_base;
    } else {
        if (s->ws_own) {
            HIP_TRY(hipStreamSynchronize(st));
            (void)hipFree(s->ws_own);
            s->ws_own = nullptr;
        }
        hipError_t e = hipMalloc((void**)&s->ws_own, total);
        if (e != hipSuccess) return too_large(e);
        base = s->ws_own;
    }
    HIP_TRY(hipMemsetAsync(base, 0, total, st));
    s->qp_ws = base + (128 - (size_t)base % 128) % 128, s->qp_ws_per_mission = per, s->ws_joint = joint_wide;  // (hipMalloc returns 256-byte multiples: + 0)
    return RBP_OK;
}

size_t rbp_session_workspace_bytes(rbp_session* s) { return s && s->qp_ws ? s->qp_ws_per_mission : 0; }

int rbp_session_reserve_workspace(rbp_session* s, void* stream) {
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, "null session");
    if (int jrc = join_worker(s)) return jrc;
    HIP_TRY(hipSetDevice(s->device));
    return ensure_planner_workspace(s, (hipStream_t)stream);
}

int rbp_session_set_solver_opts(rbp_session* s, const rbp_solver_opts* o) {
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, "null session");
    if (int jrc = join_worker(s)) return jrc;
    int rc = check_solver_opts(o);
    if (rc) return rc;
    s->opts = *o;
    return RBP_OK;
}

// `async`: a grid-wide joint PLANNER stage is handed to the session's worker thread (everything else only enqueues anyway)
static int run_impl(rbp_session* s, int stages, void* stream, bool async) {
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, "null session");
    if (int jrc = join_worker(s)) return jrc;
    if (int rc = no_mission(s, "rbp_session_run")) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    const rbp_solver_opts& o = s->opts;
    if (stages & RBP_STAGE_PLANNER) {
        int rc = ensure_planner_workspace(s, st);
        if (rc) return rc;
        // refusals of a sharded session BEFORE anything is enqueued or any state of the session changes (joint_wide is known now)
        if (s->shard.nranks == 2 && !s->joint_wide)
            return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_shard_joint: this plan does not run on the grid-wide joint solver (rbp_solver_opts.joint_wide_min_agents), there is no factorisation to share");
        if (s->shard.nranks == 2 && async)
            return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_run_async: a session sharded over two ranks (rbp_session_shard_joint) calls the exchange hook on the caller's thread: use rbp_session_run");
    }
    s->last_stages = stages;
    s->d.p.polish = o.polish ? 1 : 0;
    s->d.p.far_slack = o.qp_far_slack;
    if (stages & RBP_STAGE_CORRIDOR) {
        int rc = launch_corridor(s->d, st);
        if (rc) return rc;
    }
    if ((stages & RBP_STAGE_PLANNER) && s->joint_wide) {
        // grid-wide joint QP: a launch per phase; the host learns once per interior-point iteration whether any mission is still
        // running, so this call SYNCHRONISES the stream (unlike the batch path, which only enqueues)
        launch_planner_prologue(s->d, st);
        int rc = RBP_OK;
        JointOpts jo;
        jo.corrector = o.joint_corrector ? 1 : 0, jo.schedule = o.joint_schedule;
        if (s->shard.nranks == 2) jo.shard = &s->shard;
        if (async) {
            // rbp_session_run_async: the host loop moves to a thread and a stream of the session's own, ordered after what the caller's
            // stream holds so far (inputs, the CORRIDOR stage, the prologue) by an event
            if (!s->jstream) {
                HIP_TRY(hipStreamCreateWithFlags(&s->jstream, hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&s->jev_in, hipEventDisableTiming));
            }
            HIP_TRY(hipEventRecord(s->jev_in, st));
            HIP_TRY(hipGetLastError());
            s->worker_rc = RBP_OK;
            s->worker = std::thread([s, jo]() {
                int wrc = RBP_OK;
                hipStream_t js = s->jstream;
                if (hipSetDevice(s->device) != hipSuccess || hipStreamWaitEvent(js, s->jev_in, 0) != hipSuccess) wrc = RBP_ERR_HIP;
                if (!wrc && s->d.p.iteration > 0) wrc = launch_planner_joint(s->d, s->qp_ws, js, &s->joint_stats, jo);
                if (!wrc) {
                    launch_planner_epilogue(s->d, js);
                    if (hipStreamSynchronize(js) != hipSuccess || hipGetLastError() != hipSuccess) wrc = RBP_ERR_HIP;
                }
                s->worker_rc = wrc;
            });
            return RBP_OK;
        }
        if (s->d.p.iteration > 0) rc = launch_planner_joint(s->d, s->qp_ws, st, &s->joint_stats, jo);
        if (rc == RBP_ERR_EXCHANGE) return rc;  // (kernels/jqp.hip has recorded which exchange failed and why)
        if (rc) return fail(rc, "joint QP: HIP error");
        launch_planner_epilogue(s->d, st);
    } else if ((stages & RBP_STAGE_PLANNER) && o.qp_schedule == 2) {
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_solver_opts.qp_schedule = 2: the phase-split schedule was retired because it lost every comparison with one workgroup "
                                          "per mission (docs/HISTORY.md, r05)");
    } else if (stages & RBP_STAGE_PLANNER) {
        // one workgroup per mission (qp_batch_kernel; docs/HISTORY.md r05 has the A/B against the retired phase split).  Two workgroups
        // per CU (the 256-thread build) pay off as soon as there are more missions than CUs: the 512-thread build would need a second round
        // (measured at 300/400/500 missions: +17-21 %)
        const bool w4 = o.qp_variant ? o.qp_variant == 4 : s->d.K > s->n_cu;
        DevSession d = s->d;
        if (!o.qp_block_order) d.qp_order = nullptr, d.qp_cost = nullptr;
        if (w4)
            launch_planner_w4(d, s->qp_ws, s->qp_ws_per_mission, st);
        else
            launch_planner_w2(d, s->qp_ws, s->qp_ws_per_mission, st);
    }
    HIP_TRY(hipGetLastError());
    return RBP_OK;
}

int rbp_session_run(rbp_session* s, int stages, void* stream) { return run_impl(s, stages, stream, false); }
int rbp_session_run_async(rbp_session* s, int stages, void* stream) { return run_impl(s, stages, stream, true); }
int rbp_session_wait(rbp_session* s) {
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, "null session");
    return join_worker(s);
}

static int shard_joint_impl(rbp_session* s, int32_t rank, int32_t nranks, rbp_exchange_fn exchange, rbp_exchange_stream_fn exchange_stream,
                            rbp_exchange_abort_fn abort_peer, void* user, double timeout_s) {
    if (!s) return fail(RBP_ERR_BAD_ARGUMENT, "null session");
    if (int jrc = join_worker(s)) return jrc;
    if (nranks == 1) {  // undo: this session runs both chains again (the buffers stay until destroy)
        s->shard.nranks = 1, s->shard.rank = 0, s->shard.exchange = nullptr, s->shard.exchange_stream = nullptr, s->shard.abort_peer = nullptr, s->shard.user = nullptr;
        return RBP_OK;
    }
    if (nranks != 2 || rank < 0 || rank > 1 || (!exchange && !exchange_stream))
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_shard_joint: the twisted elimination has two chains -- nranks must be 2 (or 1 to undo), rank 0 or 1, and an exchange hook is needed");
    if (s->param.sequential || s->d.N < 2)
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_shard_joint: only a joint QP (plan/sequential = false) has a factorisation to share; the sequential schedule shards by mission");
    const size_t cap = joint_exchange_bytes(s->d.N, s->d.M, s->d.K);
    if (!s->shard_buf) {
        HIP_TRY(hipSetDevice(s->device));
        const hipError_t e = hipMalloc((void**)&s->shard_buf, 2 * cap + 64);  // (+ the error word of the stream-ordered exchange)
        if (e != hipSuccess)
            return fail(RBP_ERR_HIP, "rbp_session_shard_joint: exchange buffers (2 x " + std::to_string(cap) + " bytes) could not be reserved: " + hipGetErrorString(e));
    }
    s->shard.rank = rank, s->shard.nranks = 2, s->shard.send = (double*)s->shard_buf, s->shard.recv = (double*)(s->shard_buf + cap), s->shard.cap = cap;
    s->shard.xerr = (double*)(s->shard_buf + 2 * cap);
    s->shard.exchange = exchange, s->shard.exchange_stream = exchange_stream, s->shard.abort_peer = abort_peer, s->shard.user = user, s->shard.timeout_s = timeout_s;
    return RBP_OK;
}
int rbp_session_shard_joint(rbp_session* s, int32_t rank, int32_t nranks, rbp_exchange_fn exchange, void* user) {
    return shard_joint_impl(s, rank, nranks, exchange, nullptr, nullptr, user, 0.0);
}
int rbp_session_shard_joint_stream(rbp_session* s, int32_t rank, int32_t nranks, rbp_exchange_stream_fn exchange, rbp_exchange_abort_fn abort_peer, void* user,
                                   double timeout_s) {
    return shard_joint_impl(s, rank, nranks, nullptr, exchange, abort_peer, user, timeout_s);
}

int rbp_session_download(rbp_session* s, rbp_plan* plans, int32_t* status, void* stream) {
    if (!s || !plans) return fail(RBP_ERR_BAD_ARGUMENT, "null argument");
    if (int jrc = join_worker(s)) return jrc;
    if (int rc = no_mission(s, "rbp_session_download")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const DevSession& d = s->d;
    const int K = d.K, N = d.N, M = d.M, MB = d.max_boxes, P = M + 1, oq = 6 * M;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int> stat(K);
    std::vector<double> sc((size_t)K * SC_N);
    std::vector<double> boxbuf, timebuf;
#define DN(dst, src, bytes) HIP_TRY(hipMemcpy((dst), (const void*)(src), (bytes), hipMemcpyDeviceToHost))
    DN(stat.data(), d.status, sizeof(int) * K);
    DN(sc.data(), d.scalars, sizeof(double) * K * SC_N);
    int first = 0;
    const BatchSchedule sched = batch_schedule(s->param.sequential, s->param.batch_size, s->param.batch_iter, N);
    const int bs = sched.bs, biter = sched.biter;
    for (int k = 0; k < K; ++k) {
        rbp_plan& p = plans[k];
        const int Mq = s->Mk[k], Pq = Mq + 1, oqq = 6 * Mq, MBq = s->MBk[k];
        if (p.N != N || p.M != Mq || p.max_boxes != MBq) return fail(RBP_ERR_BAD_ARGUMENT, "plan shape differs from the session");
        const double* q = &sc[(size_t)k * SC_N];
        // timeScale (rbp_planner.hpp:250-264) multiplies T, the SFC end times and the RSFC times by time_scale: done here, on
        // the host copies (the same IEEE products), because the device arrays stay unscaled (see rbp_session_reset)
        // ... and only when the last run included the planner: after a CORRIDOR-only run the scalar still holds the factor of
        // an earlier planner run, which has nothing to do with the corridor times just written
        const double ts = ((s->last_stages & RBP_STAGE_PLANNER) && q[SC_TIME_SCALE] > 0) ? q[SC_TIME_SCALE] : 1.0;
        DN(p.T, d.T + (size_t)k * P, sizeof(double) * Pq);
        if (ts != 1.0)
            for (int m = 0; m < Pq; ++m) p.T[m] *= ts;
        if (p.sfc_count) DN(p.sfc_count, d.sfc_count + (size_t)k * N, sizeof(int) * N);
        if (p.sfc_box) {
            if (MBq == MB) {
                DN(p.sfc_box, d.sfc_box + (size_t)k * N * MB * 6, sizeof(double) * (size_t)N * MB * 6);
            } else {
                boxbuf.resize((size_t)N * MB * 6);
                DN(boxbuf.data(), d.sfc_box + (size_t)k * N * MB * 6, sizeof(double) * (size_t)N * MB * 6);
                repack_boxes(p.sfc_box, MBq, boxbuf.data(), MB, N, 6);
            }
        }
        if (p.sfc_time) {
            timebuf.resize((size_t)N * MB);
            DN(timebuf.data(), d.sfc_time + (size_t)k * N * MB, sizeof(double) * (size_t)N * MB);
            std::vector<int> cnt(N);
            DN(cnt.data(), d.sfc_count + (size_t)k * N, sizeof(int) * N);
            if (ts != 1.0)
                for (int a = 0; a < N; ++a)
                    for (int b = 0; b < cnt[a] && b < MB; ++b) timebuf[(size_t)a * MB + b] *= ts;
            repack_boxes(p.sfc_time, MBq, timebuf.data(), MB, N, 1);
        }
        if (p.rsfc_normal) DN(p.rsfc_normal, d.rsfc_normal + (size_t)k * d.npair * M * 3, sizeof(float) * (size_t)d.npair * Mq * 3);
        if (p.rsfc_time) {
            DN(p.rsfc_time, d.rsfc_time + (size_t)k * M, sizeof(double) * Mq);
            if (ts != 1.0)
                for (int m = 0; m < Mq; ++m) p.rsfc_time[m] *= ts;
        }
        // the planner's outputs belong to a run that included the planner: after a CORRIDOR-only run the device still holds the control
        // points / coefficients of an earlier planner run (coef even rescaled by THAT run's time_scale), which do not go with the corridor
        // just written -- they are not handed out, and the solver outcome reads "no QP solved"
        const bool planned = (s->last_stages & RBP_STAGE_PLANNER) != 0;
        if (planned && p.coef) DN(p.coef, d.coef + (size_t)k * N * 3 * oq, sizeof(double) * (size_t)N * 3 * oqq);
        if (planned && p.ctrl) DN(p.ctrl, d.ctrl + (size_t)k * N * 3 * oq, sizeof(double) * (size_t)N * 3 * oqq);
        p.time_scale = ts;
        p.time_scale_alt = ((s->last_stages & RBP_STAGE_PLANNER) && q[SC_TIME_SCALE_ALT] > 0) ? q[SC_TIME_SCALE_ALT] : 1.0;
        p.total_cost = planned ? q[SC_TOTAL_COST] : 0.0;
        p.qp_iterations = planned ? (int)q[SC_IPM_ITERS] : 0;
        p.qp_solves = planned ? (int)q[SC_QP_SOLVED] : 0;
        p.qp_unpolished = planned ? (int)(q[SC_QP_SOLVED] - q[SC_POLISHED]) : 0;
        p.kkt_max = planned ? q[SC_KKT_MAX] : 0.0;
        if (biter > 0) {
            int last = biter - 1, nb = std::min(bs, N - last * bs);
            p.x_size = 3 * nb * oqq;
            p.eq_size = 3 * nb * 3 * (Mq + 1);
            int nf = N - nb;
            p.ineq_size = 2 * p.x_size + (nb * (nb - 1) / 2 + nb * nf) * oqq;
        }
        if (status) status[k] = stat[k];
        if (!first && stat[k]) first = stat[k];
    }
#undef DN
    if (first) g_err = "mission failed with status " + std::to_string(first);
    return first;
}

// The missions' safety ratios and flight distances from where the plans lie (kernels/report.hip): coef, T, the time scale among the
// scalars, radius and status are read in place, K structs come back in one copy, and nothing of the session is written.
int rbp_session_report(rbp_session* s, double dt, rbp_report* out, void* stream) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_report: null argument");
    if (!(dt > 0)) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_report: dt must be positive");
    if (int jrc = join_worker(s)) return jrc;
    if (int rc = no_mission(s, "rbp_session_report")) return rc;
    if (!(s->last_stages & RBP_STAGE_PLANNER))
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_report: the session's last run did not include the PLANNER stage: there are no coefficients to report on");
    const DevSession& d = s->d;
    if (report_tile(d.N) <= 0)
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_report: " + std::to_string(d.N) + " agents: the positions of one sample do not fit the report kernel's LDS budget");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    if (!s->report_buf) {
        const hipError_t e = hipMalloc((void**)&s->report_buf, report_workspace_bytes(s->cap.K));
        if (e != hipSuccess) {
            s->report_buf = nullptr;
            return fail(RBP_ERR_HIP, std::string("rbp_session_report: workspace: ") + hipGetErrorString(e));
        }
    }
    ReportInputs in{};
    in.K = d.K, in.N = d.N, in.M_stride = d.M, in.Mk = d.Mk, in.T = d.T, in.coef = d.coef, in.radius = d.radius;
    in.ts = d.scalars + SC_TIME_SCALE, in.ts_stride = SC_N, in.status = d.status;
    in.downwash = d.p.downwash, in.dt = dt;
    if (int rc = launch_report(in, s->report_buf, st)) return rc;
    HIP_TRY(hipMemcpyAsync(out, s->report_buf, sizeof(rbp_report) * (size_t)d.K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RBP_OK;
}

// The missions' sampled states, limit peaks and ratio curves from where the plans lie (kernels/dynamics.hip): the report's inputs and the
// agents' limits are read in place, K structs come back in one copy (per chunk of missions where a destination is on the host), states and
// curves go where the caller wants them, and nothing of the session is written.
int rbp_session_dynamics(rbp_session* s, double dt, rbp_dynamics* out, double* states, double* curves, int32_t S_stride, void* stream) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_dynamics: null argument");
    if (!(dt > 0)) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_dynamics: dt must be positive");
    if ((states || curves) && S_stride < 1) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_dynamics: S_stride must be at least 1 where states or curves are given");
    if (int jrc = join_worker(s)) return jrc;
    if (int rc = no_mission(s, "rbp_session_dynamics")) return rc;
    if (!(s->last_stages & RBP_STAGE_PLANNER))
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_dynamics: the session's last run did not include the PLANNER stage: there are no coefficients to sample");
    const DevSession& d = s->d;
    if (dynamics_tile(d.N) <= 0)
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_dynamics: " + std::to_string(d.N) + " agents: the positions of one sample do not fit the curve kernel's LDS budget");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->dynamics_buf) {
        const hipError_t e = hipMalloc((void**)&s->dynamics_buf, dynamics_workspace_bytes(s->cap.K));
        if (e != hipSuccess) {
            s->dynamics_buf = nullptr;
            return fail(RBP_ERR_HIP, std::string("rbp_session_dynamics: workspace: ") + hipGetErrorString(e));
        }
    }
    DynamicsInputs in{};
    in.r.K = d.K, in.r.N = d.N, in.r.M_stride = d.M, in.r.Mk = d.Mk, in.r.T = d.T, in.r.coef = d.coef, in.r.radius = d.radius;
    in.r.ts = d.scalars + SC_TIME_SCALE, in.r.ts_stride = SC_N, in.r.status = d.status;
    in.r.downwash = d.p.downwash, in.r.dt = dt;
    in.max_vel = d.max_vel, in.max_acc = d.max_acc;
    return dynamics_run("rbp_session_dynamics", s->device, in, out, states, curves, S_stride, s->dynamics_buf, (hipStream_t)stream);
}

// The missions' clearance to the obstacles from where the plans and the grids lie (kernels/clearance.hip): the report's inputs and the
// session's worlds are read in place, K structs come back in one copy, the agents' clearances go where the caller wants them, and nothing
// of the session is written.
int rbp_session_clearance(rbp_session* s, double dt, rbp_clearance* out, double* agent_clearance, void* stream) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_clearance: null argument");
    if (!(dt > 0)) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_clearance: dt must be positive");
    if (int jrc = join_worker(s)) return jrc;
    if (int rc = no_mission(s, "rbp_session_clearance")) return rc;
    if (!(s->last_stages & RBP_STAGE_PLANNER))
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_clearance: the session's last run did not include the PLANNER stage: there are no coefficients to look up");
    const DevSession& d = s->d;
    HIP_TRY(hipSetDevice(s->device));
    if (!s->clearance_buf) {
        const hipError_t e = hipMalloc((void**)&s->clearance_buf, clearance_workspace_bytes(s->cap.K, d.N));
        if (e != hipSuccess) {
            s->clearance_buf = nullptr;
            return fail(RBP_ERR_HIP, std::string("rbp_session_clearance: workspace: ") + hipGetErrorString(e));
        }
    }
    ClearanceInputs in{};
    in.r.K = d.K, in.r.N = d.N, in.r.M_stride = d.M, in.r.Mk = d.Mk, in.r.T = d.T, in.r.coef = d.coef, in.r.radius = d.radius;
    in.r.ts = d.scalars + SC_TIME_SCALE, in.r.ts_stride = SC_N, in.r.status = d.status;
    in.r.downwash = d.p.downwash, in.r.dt = dt;
    in.worlds = d.worlds;
    return clearance_run("rbp_session_clearance", s->device, in, out, agent_clearance, s->clearance_buf, (hipStream_t)stream);
}

// A certified interval for the missions' smallest safety ratio in continuous time from where the plans lie (kernels/separation.hip):
// the report's inputs are read in place, K structs come back in one copy, the pairs' lower ratios go where the caller wants them, and
// nothing of the session is written.
int rbp_session_separation(rbp_session* s, int32_t depth, double refine_below, rbp_separation* out, double* pair_lower, void* stream) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_separation: null argument");
    if (int rc = separation_check_arguments("rbp_session_separation", depth, refine_below)) return rc;
    if (int jrc = join_worker(s)) return jrc;
    if (int rc = no_mission(s, "rbp_session_separation")) return rc;
    if (!(s->last_stages & RBP_STAGE_PLANNER))
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_separation: the session's last run did not include the PLANNER stage: there are no coefficients to bound");
    const DevSession& d = s->d;
    HIP_TRY(hipSetDevice(s->device));
    if (!s->separation_buf) {
        const hipError_t e = hipMalloc((void**)&s->separation_buf, separation_workspace_bytes(s->cap.K, d.N, d.M));
        if (e != hipSuccess) {
            s->separation_buf = nullptr;
            return fail(RBP_ERR_HIP, std::string("rbp_session_separation: workspace: ") + hipGetErrorString(e));
        }
    }
    SeparationInputs in{};
    in.r.K = d.K, in.r.N = d.N, in.r.M_stride = d.M, in.r.Mk = d.Mk, in.r.T = d.T, in.r.coef = d.coef, in.r.radius = d.radius;
    in.r.ts = d.scalars + SC_TIME_SCALE, in.r.ts_stride = SC_N, in.r.status = d.status;
    in.r.downwash = d.p.downwash, in.r.dt = 0.0;
    in.depth = depth, in.refine_below = refine_below;
    return separation_run("rbp_session_separation", s->device, in, out, pair_lower, s->separation_buf, (hipStream_t)stream);
}

// A certified interval for the missions' smallest clearance to the obstacles in continuous time from where the plans and the grids lie
// (kernels/swept.hip): the report's inputs and the session's worlds are read in place, K structs come back in one copy, the agents' lower
// clearances go where the caller wants them, and nothing of the session is written.
int rbp_session_swept_clearance(rbp_session* s, int32_t depth, double refine_below, rbp_swept_clearance* out, double* agent_lower, void* stream) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_swept_clearance: null argument");
    if (int rc = swept_check_arguments("rbp_session_swept_clearance", depth, refine_below)) return rc;
    if (int jrc = join_worker(s)) return jrc;
    if (int rc = no_mission(s, "rbp_session_swept_clearance")) return rc;
    if (!(s->last_stages & RBP_STAGE_PLANNER))
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_swept_clearance: the session's last run did not include the PLANNER stage: there are no coefficients to bound");
    const DevSession& d = s->d;
    HIP_TRY(hipSetDevice(s->device));
    if (!s->swept_buf) {
        const hipError_t e = hipMalloc((void**)&s->swept_buf, swept_workspace_bytes(s->cap.K, d.N, d.M));
        if (e != hipSuccess) {
            s->swept_buf = nullptr;
            return fail(RBP_ERR_HIP, std::string("rbp_session_swept_clearance: workspace: ") + hipGetErrorString(e));
        }
    }
    SweptInputs in{};
    in.r.K = d.K, in.r.N = d.N, in.r.M_stride = d.M, in.r.Mk = d.Mk, in.r.T = d.T, in.r.coef = d.coef, in.r.radius = d.radius;
    in.r.ts = d.scalars + SC_TIME_SCALE, in.r.ts_stride = SC_N, in.r.status = d.status;
    in.r.downwash = d.p.downwash, in.r.dt = 0.0;
    in.worlds = d.worlds;
    in.depth = depth, in.refine_below = refine_below;
    return swept_run("rbp_session_swept_clearance", s->device, in, out, agent_lower, s->swept_buf, (hipStream_t)stream);
}

// Certified intervals for the missions' largest velocity and acceleration ratios in continuous time from where the plans lie
// (kernels/limits.hip): the report's inputs and the session's limits are read in place, K structs come back in one copy, the agents' upper
// ratios go where the caller wants them, and nothing of the session is written.
int rbp_session_limits(rbp_session* s, int32_t depth, double refine_above, rbp_limits* out, double* agent_upper, void* stream) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_limits: null argument");
    if (int rc = limits_check_arguments("rbp_session_limits", depth, refine_above)) return rc;
    if (int jrc = join_worker(s)) return jrc;
    if (int rc = no_mission(s, "rbp_session_limits")) return rc;
    if (!(s->last_stages & RBP_STAGE_PLANNER))
        return fail(RBP_ERR_BAD_ARGUMENT, "rbp_session_limits: the session's last run did not include the PLANNER stage: there are no coefficients to bound");
    const DevSession& d = s->d;
    HIP_TRY(hipSetDevice(s->device));
    if (!s->limits_buf) {
        const hipError_t e = hipMalloc((void**)&s->limits_buf, limits_workspace_bytes(s->cap.K, d.N, d.M));
        if (e != hipSuccess) {
            s->limits_buf = nullptr;
            return fail(RBP_ERR_HIP, std::string("rbp_session_limits: workspace: ") + hipGetErrorString(e));
        }
    }
    LimitsInputs in{};
    in.r.K = d.K, in.r.N = d.N, in.r.M_stride = d.M, in.r.Mk = d.Mk, in.r.T = d.T, in.r.coef = d.coef, in.r.radius = d.radius;
    in.r.ts = d.scalars + SC_TIME_SCALE, in.r.ts_stride = SC_N, in.r.status = d.status;
    in.r.downwash = d.p.downwash, in.r.dt = 0.0;
    in.max_vel = d.max_vel, in.max_acc = d.max_acc;
    in.depth = depth, in.refine_above = refine_above;
    return limits_run("rbp_session_limits", s->device, in, out, agent_upper, s->limits_buf, (hipStream_t)stream);
}

int rbp_session_device_arrays(rbp_session* s, int32_t mission, rbp_device_arrays* out) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "null argument");
    const DevSession& d = s->d;
    if (mission < 0 || mission >= d.K) return fail(RBP_ERR_BAD_ARGUMENT, "mission index outside the session");
    const size_t k = (size_t)mission;
    out->sfc_count = d.sfc_count + k * d.N;
    out->sfc_box = d.sfc_box + k * d.N * d.max_boxes * 6;
    out->sfc_time = d.sfc_time + k * d.N * d.max_boxes;
    out->rsfc_normal = d.rsfc_normal + k * d.npair * d.M * 3;
    out->rsfc_time = d.rsfc_time + k * d.M;
    out->status = d.status + k;
    out->N = d.N, out->M = d.M, out->max_boxes = d.max_boxes, out->npair = d.npair, out->device = s->device;
    return RBP_OK;
}

int rbp_session_counters(rbp_session* s, rbp_counters* out, void* stream) {
    if (!s || !out) return fail(RBP_ERR_BAD_ARGUMENT, "null argument");
    if (int jrc = join_worker(s)) return jrc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const int K = s->d.K;
    std::vector<unsigned long long> ct((size_t)K * CT_N);
    std::vector<double> sc((size_t)K * SC_N);
    HIP_TRY(hipMemcpy(ct.data(), s->d.counters, sizeof(unsigned long long) * ct.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sc.data(), s->d.scalars, sizeof(double) * sc.size(), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    for (int k = 0; k < K; ++k) {
        out->sfc_samples += (double)ct[(size_t)k * CT_N + CT_SFC_SAMPLES];
        out->qp_flops += sc[(size_t)k * SC_N + SC_FLOPS];
        out->qp_ipm_iters += sc[(size_t)k * SC_N + SC_IPM_ITERS];
        out->qp_solves += sc[(size_t)k * SC_N + SC_QP_SOLVED];
        out->qp_constraint_rows += sc[(size_t)k * SC_N + SC_ROWS];
        out->qp_polished += sc[(size_t)k * SC_N + SC_POLISHED];
        out->qp_row_bytes += sc[(size_t)k * SC_N + SC_ROW_BYTES];
        out->kkt_max = std::max(out->kkt_max, sc[(size_t)k * SC_N + SC_KKT_MAX]);
    }
    return RBP_OK;
}

int rbp_session_scalars(rbp_session* s, double* out, int n, void* stream) {
    if (!s || !out || n <= 0 || n > SC_N) return fail(RBP_ERR_BAD_ARGUMENT, "bad argument");
    if (int jrc = join_worker(s)) return jrc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    std::vector<double> sc((size_t)s->d.K * SC_N);
    HIP_TRY(hipMemcpy(sc.data(), s->d.scalars, sizeof(double) * sc.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < s->d.K; ++k) memcpy(out + (size_t)k * n, &sc[(size_t)k * SC_N], sizeof(double) * n);
    return RBP_OK;
}

void rbp_session_destroy(rbp_session* s) {
    if (!s) return;
    (void)join_worker(s);
    if (s->jstream) {
        (void)hipSetDevice(s->device);
        (void)hipStreamDestroy(s->jstream);
        (void)hipEventDestroy(s->jev_in);
    }
    if (s->ws_own) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->ws_own);
    }
    if (s->shard_buf) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->shard_buf);
    }
    if (s->report_buf) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->report_buf);
    }
    if (s->dynamics_buf) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->dynamics_buf);
    }
    if (s->clearance_buf) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->clearance_buf);
    }
    if (s->separation_buf) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->separation_buf);
    }
    if (s->swept_buf) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->swept_buf);
    }
    if (s->limits_buf) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->limits_buf);
    }
    if (s->stage_h || s->stage_d || s->stage_ev) {
        (void)hipSetDevice(s->device);
        if (s->stage_ev) (void)hipEventDestroy(s->stage_ev);
        if (s->stage_h) (void)hipHostFree(s->stage_h);
        if (s->stage_d) (void)hipFree(s->stage_d);
    }
    if (s->pstage_h || s->pstage_d || s->pstage_ev) {
        (void)hipSetDevice(s->device);
        if (s->pstage_ev) (void)hipEventDestroy(s->pstage_ev);
        if (s->pstage_h) (void)hipHostFree(s->pstage_h);
        if (s->pstage_d) (void)hipFree(s->pstage_d);
    }
    if (s->ctx) {
        s->ctx->busy = false;  // the arena (and the QP workspace) stay with the context
    } else if (s->arena.base) {
        (void)hipSetDevice(s->device);
        (void)hipFree(s->arena.base);
    }
    delete s;
}

// ---- contexts ---------------------------------------------------------------------------------------------------------
int rbp_ctx_create(rbp_ctx** out, int device) {
    if (!out) return fail(RBP_ERR_BAD_ARGUMENT, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(RBP_ERR_NO_DEVICE, "no HIP device: the RBP path has no CPU fallback");
    if (device < 0) (void)hipGetDevice(&device);  // the calling thread's current device
    if (device < 0 || device >= ndev) return fail(RBP_ERR_NO_DEVICE, "device index out of range");
    auto* c = new rbp_ctx();
    c->device = device;
    *out = c;
    return RBP_OK;
}

void rbp_ctx_destroy(rbp_ctx* c) {
    if (!c) return;
    if (c->base || c->ws_base) {
        (void)hipSetDevice(c->device);
        if (c->base) (void)hipFree(c->base);
        if (c->ws_base) (void)hipFree(c->ws_base);
    }
    delete c;
}

// The per-thread default context of the drop-in calls.  A worker thread that exits gives its arena back (hipFree); at process
// exit the HIP runtime may already be gone when thread_local destructors run, so from the first atexit handler on nothing is
// freed any more (the runtime releases device memory itself).  rbp_release_thread_context() frees it on request.
namespace {
bool g_process_exiting = false;
struct Tls {
    rbp_ctx* c = nullptr;
    ~Tls() {
        if (c && !g_process_exiting) rbp_ctx_destroy(c);
        c = nullptr;
    }
};
Tls& tls_ctx() {
    static const int registered = (atexit([] { g_process_exiting = true; }), 0);
    (void)registered;
    thread_local Tls tls;
    return tls;
}
}  // namespace

void rbp_release_thread_context(void) {
    Tls& tls = tls_ctx();
    if (tls.c) rbp_ctx_destroy(tls.c);
    tls.c = nullptr;
}

static int one_shot(rbp_ctx* ctx, const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan,
                    int stages, int agent_begin = 0, int agent_end = -1) {
    if (!mission || !param || !plan) return fail(RBP_ERR_BAD_ARGUMENT, "null argument");
    if (stages == RBP_STAGE_PLANNER) {
        if (!(plan->sfc_count && plan->sfc_box && plan->sfc_time && plan->rsfc_normal && plan->rsfc_time))
            return fail(RBP_ERR_BAD_ARGUMENT, "RBPPlanner::update needs the corridor (plan.sfc_* and plan.rsfc_*) as input");
        for (int a = 0; a < plan->N; ++a)
            if (plan->sfc_count[a] <= 0 || plan->sfc_count[a] > plan->max_boxes)
                return fail(RBP_ERR_BAD_ARGUMENT, "RBPPlanner::update: plan.sfc_count must be in [1, max_boxes] for every agent (run Corridor::update first)");
    }
    rbp_world dummy_world;
    float zero = 0.0f;
    if (!world) {  // planner stage does not read the map
        dummy_world.dim[0] = dummy_world.dim[1] = dummy_world.dim[2] = 1;
        dummy_world.key_min[0] = dummy_world.key_min[1] = dummy_world.key_min[2] = 0;
        dummy_world.res = 1.0, dummy_world.dist = &zero;
        world = &dummy_world;
    }
    // without an explicit context the calling thread's own one is used (created on first use on its current device), so the
    // drop-in calls do not allocate device memory per plan either
    Tls& tls = tls_ctx();
    if (!ctx) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        rbp_solver_opts keep = tls.c ? tls.c->opts : default_solver_opts();
        if (tls.c && tls.c->device != dev) {
            rbp_ctx_destroy(tls.c);
            tls.c = nullptr;
        }
        if (!tls.c) {
            int rc = rbp_ctx_create(&tls.c, dev);
            if (rc) return rc;
            tls.c->opts = keep;
        }
        ctx = tls.c;
    }
    rbp_session* s = nullptr;
    int rc = session_create_impl(&s, ctx->device, 1, world, mission, param, plan, ctx);
    if (rc) return rc;
    if (agent_end >= 0) rc = rbp_session_set_agent_range(s, agent_begin, agent_end);
    if (!rc) rc = rbp_session_run(s, stages, nullptr);
    if (!rc) {
        int32_t st = 0;
        rc = rbp_session_download(s, plan, &st, nullptr);
    }
    rbp_session_destroy(s);
    return rc;
}

int rbp_ctx_set_solver_opts(rbp_ctx* ctx, const rbp_solver_opts* o) {
    int rc = check_solver_opts(o);
    if (rc) return rc;
    if (!ctx) {  // the calling thread's default context
        Tls& tls = tls_ctx();
        if (!tls.c) {
            int ndev = 0, dev = 0;
            if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RBP_ERR_NO_DEVICE, "no HIP device: the RBP path has no CPU fallback");
            (void)hipGetDevice(&dev);
            rc = rbp_ctx_create(&tls.c, dev);
            if (rc) return rc;
        }
        ctx = tls.c;
    }
    ctx->opts = *o;
    return RBP_OK;
}

int rbp_corridor_update(const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan) {
    if (!world) return fail(RBP_ERR_BAD_ARGUMENT, "null world");
    return one_shot(nullptr, world, mission, param, plan, RBP_STAGE_CORRIDOR);
}

int rbp_corridor_update_range(const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan,
                              int32_t agent_begin, int32_t agent_end) {
    if (!world) return fail(RBP_ERR_BAD_ARGUMENT, "null world");
    if (agent_end < 0) return fail(RBP_ERR_BAD_ARGUMENT, "agent range outside [0, N]");
    return one_shot(nullptr, world, mission, param, plan, RBP_STAGE_CORRIDOR, agent_begin, agent_end);
}

int rbp_planner_update(const rbp_mission* mission, const rbp_param* param, rbp_plan* plan) {
    return one_shot(nullptr, nullptr, mission, param, plan, RBP_STAGE_PLANNER);
}

int rbp_ctx_corridor_update(rbp_ctx* ctx, const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan) {
    if (!ctx || !world) return fail(RBP_ERR_BAD_ARGUMENT, "null context / world");
    return one_shot(ctx, world, mission, param, plan, RBP_STAGE_CORRIDOR);
}

int rbp_ctx_planner_update(rbp_ctx* ctx, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan) {
    if (!ctx) return fail(RBP_ERR_BAD_ARGUMENT, "null context");
    return one_shot(ctx, nullptr, mission, param, plan, RBP_STAGE_PLANNER);
}

int rbp_ctx_plan_update(rbp_ctx* ctx, const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan) {
    if (!ctx || !world) return fail(RBP_ERR_BAD_ARGUMENT, "null context / world");
    return one_shot(ctx, world, mission, param, plan, RBP_STAGE_ALL);
}

}  // extern "C"
