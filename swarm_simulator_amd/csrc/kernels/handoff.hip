// handoff.hip — from the device search's packed paths to what a session plans from, without a host trip (gfx950).
//
// ecbs_kernel (kernels/ecbs.hip) leaves every mission's paths as packed cells in HBM; a rbp_dev_ecbs keeps them there beside the missions'
// states and limits.  The two kernels here turn them into the arrays of a consumer, where the consumer wants them:
//   ecbs_plan_write_kernel      T [n][stride] and init_traj [n][N][stride][3] of the chosen missions -- the download buffer of
//                               rbp_dev_ecbs_download (stride max_M + 1, all K missions) or a session's arena (rbp_session_create_from_ecbs:
//                               stride = the largest M + 1 of the missions it holds, and inside its slot every mission is laid out with
//                               its own M + 1, as kernels/rbp_dev.h says of a session);
//   ecbs_mission_gather_kernel  start / goal / radius / max_vel / max_acc of the chosen missions into the session's [n][N][...] arrays.
//   session_refill_kernel       both of the above for the slots 0 .. n-1 of a session that already exists (rbp_session_refill_from_ecbs), with the
//                               slots' descriptors and the clears a fresh arena would have provided, in one launch.
//   session_refill_plans_kernel the same for the slots [j0, j0 + n) from a caller's own plans (rbp_session_refill_from_plans), which the host
//                               packed into a staging block: layout and element rules are common/plan_stage.h.
// All are one element per lane, consecutive lanes on consecutive elements of a row: plain vector loads and stores, no LDS, no atomics.  The
// element bodies (plan_time_element, plan_traj_element, mission_gather_element) are stated once and called by the kernels that need them.
// Every value of the first is a rule of common/ecbs_rules.h (plan_time, plan_waypoint) -- the text the host's write_plan loops over -- and
// that header's `#pragma clang fp contract(off)` holds for this whole file, so the device rounds each operation as the host does.
#include "rbp_dev.h"

#include <string>

#include "common/ecbs_rules.h"
#include "common/plan_stage.h"

namespace {

constexpr int HANDOFF_THREADS = 128;

struct PlanWrite {
    int n, N, stride, path_stride;  // destination slots, agents, waypoints a slot has room for per agent, cells per path slot
    int compact;                    // 1: a session's layout, the agents' rows of slot j are Mj[j] + 1 waypoints long (kernels/rbp_dev.h); 0: `stride` long
    int chunks, t_chunks;           // blocks per slot of init_traj: ceil(3 N stride / HANDOFF_THREADS), and per row of T
    double gmin[3], gres[3], time_step;
    const int* src;                 // [n] the mission of the search that slot j takes
    const int* Mj;                  // [n] its segment count, < 0: no plan
    const int* out_len;             // [K][N]
    const unsigned* out_path;       // [K][N][path_stride]
    const double *start, *goal;     // [K][N][9]
    double* T;                      // [n][stride]
    float* init_traj;               // [n][N * stride * 3]
};

// element i of row j of T: what lies beyond a mission's own M is zero
__device__ __forceinline__ void plan_time_element(const PlanWrite& w, int j, int i) {
    w.T[(size_t)j * w.stride + i] = i <= w.Mj[j] ? ecbs_rules::plan_time(i, w.time_step) : 0.0;
}

// float f (< 3 N stride) of slot j of init_traj: what lies beyond a mission's own M is zero
__device__ __forceinline__ void plan_traj_element(const PlanWrite& w, int j, int f) {
    const int slot = 3 * w.N * w.stride;
    const int M = w.Mj[j], row = 3 * (w.compact && M >= 0 ? M + 1 : w.stride);
    const int a = f / row, e = f - a * row, wp = e / 3, axis = e - 3 * wp;
    float v = 0.0f;
    if (a < w.N && wp <= M) {
        const size_t ka = (size_t)w.src[j] * w.N + a;
        const unsigned* path = w.out_path + ka * w.path_stride;
        v = ecbs_rules::plan_waypoint(wp, axis, w.out_len[ka], [&](int p) { return PackedCell{path[p]}; }, w.start + 9 * ka, w.goal + 9 * ka, w.gmin, w.gres);
    }
    w.init_traj[(size_t)j * slot + f] = v;
}

// The first n * chunks blocks write the slots of init_traj, one float per lane and a slot `chunks` blocks wide; the last n * t_chunks
// blocks write the rows of T.  Every element of the destination is written: what lies beyond a mission's own M is zero.
__global__ __launch_bounds__(HANDOFF_THREADS) void ecbs_plan_write_kernel(PlanWrite w) {
    const int traj_blocks = w.n * w.chunks;
    if ((int)blockIdx.x >= traj_blocks) {
        const int tb = (int)blockIdx.x - traj_blocks, j = tb / w.t_chunks;
        const int i = (tb - j * w.t_chunks) * HANDOFF_THREADS + (int)threadIdx.x;
        if (i < w.stride) plan_time_element(w, j, i);
        return;
    }
    const int j = (int)blockIdx.x / w.chunks;
    const int f = ((int)blockIdx.x - j * w.chunks) * HANDOFF_THREADS + (int)threadIdx.x;   // float of slot j
    if (f >= 3 * w.N * w.stride) return;
    plan_traj_element(w, j, f);
}

struct MissionGather {
    int n, N;
    const int* src;                                            // [n]
    const double *start, *goal, *radius, *max_vel, *max_acc;   // [K][N][9 9 1 3 3]
    double *d_start, *d_goal, *d_radius, *d_max_vel, *d_max_acc;  // [n][N][9 9 1 3 3]
};

// double r (< 25 N) of mission j: its [N][9] start, [N][9] goal, [N] radius, [N][3] max_vel, [N][3] max_acc
__device__ __forceinline__ void mission_gather_element(const MissionGather& g, int j, int r) {
    const size_t s = (size_t)g.src[j] * g.N, d = (size_t)j * g.N;
    if (r < 9 * g.N) {
        g.d_start[d * 9 + r] = g.start[s * 9 + r];
        return;
    }
    r -= 9 * g.N;
    if (r < 9 * g.N) {
        g.d_goal[d * 9 + r] = g.goal[s * 9 + r];
        return;
    }
    r -= 9 * g.N;
    if (r < g.N) {
        g.d_radius[d + r] = g.radius[s + r];
        return;
    }
    r -= g.N;
    if (r < 3 * g.N) {
        g.d_max_vel[d * 3 + r] = g.max_vel[s * 3 + r];
        return;
    }
    r -= 3 * g.N;
    g.d_max_acc[d * 3 + r] = g.max_acc[s * 3 + r];
}

// 25 N doubles per mission, one double per lane
__global__ __launch_bounds__(HANDOFF_THREADS) void ecbs_mission_gather_kernel(MissionGather g) {
    const long long t = (long long)blockIdx.x * HANDOFF_THREADS + threadIdx.x;
    const int per = 25 * g.N;
    if (t >= (long long)g.n * per) return;
    const int j = (int)(t / per);
    mission_gather_element(g, j, (int)(t - (long long)j * per));
}

// ---- the refill of a session that exists ------------------------------------------------------------------------------------------------
constexpr int REFILL_THREADS = 256;
constexpr int REFILL_Z64 = 8;  // ranges of 8-byte words cleared from their base: scalars, counters, qp_cost, sfc_box, sfc_time, rsfc_time, ctrl, coef

// the clears a fresh arena would hold as zeros, for a run of consecutive slots: every array's range starts at its first slot
struct SlotClears {
    int* sfc_count;
    float* rsfc_normal;
    unsigned long long* z64[REFILL_Z64];
    long long n64[REFILL_Z64];
    long long n_count, n_normal;
};

struct SessionRefill {
    PlanWrite w;      // n slots, compact, stride = the session's M + 1; src and Mj are the STAGED lists
    MissionGather g;  // (src: the staged list)
    const unsigned long long* st_worlds;  // staged descriptors, WORLD_WORDS words each
    const int* st_MBk;
    unsigned long long* worlds;
    int *Mk, *MBk, *status, *qp_order;
    SlotClears c;
    long long n_traj, n_T, n_gather, n_desc, total;
};
constexpr int WORLD_WORDS = (int)(sizeof(DevWorld) / sizeof(unsigned long long));
static_assert(sizeof(DevWorld) % sizeof(unsigned long long) == 0, "a descriptor is copied in 8-byte words");

// element i (< clear_elements) of the clears: sfc_count, the floats of rsfc_normal, then the 8-byte ranges
__device__ __forceinline__ void slot_clear_element(const SlotClears& c, long long i) {
    if (i < c.n_count) {
        c.sfc_count[i] = 0;
        return;
    }
    i -= c.n_count;
    if (i < c.n_normal) {
        c.rsfc_normal[i] = 0.0f;
        return;
    }
    i -= c.n_normal;
#pragma unroll
    for (int z = 0; z < REFILL_Z64; ++z) {
        if (i >= 0 && i < c.n64[z]) c.z64[z][i] = 0ull;
        i -= c.n64[z];
    }
}

// the clears of the slots [j0, j0 + n) of a session with the pointers and strides of `d`; returns their element count
long long slot_clears(SlotClears& c, const DevSession& d, int j0, int n) {
    const long long N = d.N, M = d.M, MB = d.max_boxes, oq = 6LL * M;
    c.sfc_count = d.sfc_count + N * j0, c.n_count = N * n;
    c.rsfc_normal = d.rsfc_normal + 3LL * d.npair * M * j0, c.n_normal = 3LL * d.npair * M * n;
    long long total = c.n_count + c.n_normal;
    auto z64 = [&](int z, void* p, long long per_slot) {
        c.z64[z] = static_cast<unsigned long long*>(p) + per_slot * j0, c.n64[z] = per_slot * n, total += c.n64[z];
    };
    z64(0, d.scalars, SC_N), z64(1, d.counters, CT_N), z64(2, d.qp_cost, 1), z64(3, d.sfc_box, 6 * N * MB), z64(4, d.sfc_time, N * MB);
    z64(5, d.rsfc_time, M), z64(6, d.ctrl, 3 * N * oq), z64(7, d.coef, 3 * N * oq);
    return total;
}

// One flat index space, walked by a grid-stride loop, one element per lane and step: the floats of init_traj, the doubles of T, the
// gathered doubles, the descriptors' words with each slot's Mk / MBk / status / qp_order, sfc_count, the floats of rsfc_normal, and the
// 8-byte ranges.  Slots 0 .. n-1 of every array are contiguous from its base, so every clear is a range from the base.
__global__ __launch_bounds__(REFILL_THREADS) void session_refill_kernel(SessionRefill r) {
    const long long step = (long long)gridDim.x * REFILL_THREADS;
    for (long long t = (long long)blockIdx.x * REFILL_THREADS + threadIdx.x; t < r.total; t += step) {
        long long i = t;
        if (i < r.n_traj) {
            const int slot = 3 * r.w.N * r.w.stride, j = (int)(i / slot);
            plan_traj_element(r.w, j, (int)(i - (long long)j * slot));
            continue;
        }
        i -= r.n_traj;
        if (i < r.n_T) {
            const int j = (int)(i / r.w.stride);
            plan_time_element(r.w, j, (int)(i - (long long)j * r.w.stride));
            continue;
        }
        i -= r.n_T;
        if (i < r.n_gather) {
            const int per = 25 * r.g.N, j = (int)(i / per);
            mission_gather_element(r.g, j, (int)(i - (long long)j * per));
            continue;
        }
        i -= r.n_gather;
        if (i < r.n_desc) {
            r.worlds[i] = r.st_worlds[i];
            const int j = (int)(i / WORLD_WORDS);
            if (i == (long long)j * WORLD_WORDS) r.Mk[j] = r.w.Mj[j], r.MBk[j] = r.st_MBk[j], r.status[j] = 0, r.qp_order[j] = 0;
            continue;
        }
        i -= r.n_desc;
        slot_clear_element(r.c, i);
    }
}

// ---- the same from a caller's plans, staged (common/plan_stage.h) ------------------------------------------------------------------------
static_assert(plan_stage::WORLD_WORDS == WORLD_WORDS, "common/plan_stage.h stages a DevWorld word by word");

struct SessionRefillPlans {
    const char* block;     // the device twin of the staging block, holding one round
    plan_stage::Round R;   // the slots [j0, j0 + n) and the session's N and stride M + 1
    MissionGather g;       // n missions from the round's tables (src: its list 0 .. n-1) into the slots from j0
    float* init_traj;      // the session's arrays, from slot 0 (the element rules give indices from there)
    double* T;
    unsigned long long* worlds;  // ... and from slot j0
    int *Mk, *MBk, *status, *qp_order;
    SlotClears c;          // of the slots [j0, j0 + n)
    long long n_traj, n_T, n_gather, n_desc, total;
};

// session_refill_kernel's index space and walk.  init_traj and T are the two element rules of common/plan_stage.h, the 25 N doubles go
// through mission_gather_element, the descriptors' words come out of the round's entries, the clears are slot_clear_element.  Every
// index derives from the round's tables, which the host packed from checked shapes.
__global__ __launch_bounds__(REFILL_THREADS) void session_refill_plans_kernel(SessionRefillPlans r) {
    const long long step = (long long)gridDim.x * REFILL_THREADS;
    for (long long t = (long long)blockIdx.x * REFILL_THREADS + threadIdx.x; t < r.total; t += step) {
        long long i = t, dst;
        if (i < r.n_traj) {
            const float v = plan_stage::traj_element(r.block, r.R, i, &dst);
            r.init_traj[dst] = v;
            continue;
        }
        i -= r.n_traj;
        if (i < r.n_T) {
            const double v = plan_stage::time_element(r.block, r.R, i, &dst);
            r.T[dst] = v;
            continue;
        }
        i -= r.n_T;
        if (i < r.n_gather) {
            const int per = 25 * r.g.N, j = (int)(i / per);
            mission_gather_element(r.g, j, (int)(i - (long long)j * per));
            continue;
        }
        i -= r.n_gather;
        if (i < r.n_desc) {
            const int j = (int)(i / WORLD_WORDS), w = (int)(i - (long long)j * WORLD_WORDS);
            const plan_stage::Entry& e = plan_stage::entry(r.block, j);
            r.worlds[i] = e.world[w];
            if (w == 0) r.Mk[j] = e.Mk, r.MBk[j] = e.MBk, r.status[j] = 0, r.qp_order[j] = 0;
            continue;
        }
        i -= r.n_desc;
        slot_clear_element(r.c, i);
    }
}

int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": launch: " + hipGetErrorString(e)).c_str());
}

}  // namespace

int launch_ecbs_plan_write(const rbp_dev_ecbs& e, int n, const int* src, const int* Mj, int stride, bool compact, double* T, float* init_traj,
                           hipStream_t st) {
    PlanWrite w{};
    w.n = n, w.N = e.N, w.stride = stride, w.path_stride = e.path_stride, w.compact = compact;
    const long long slot = 3LL * e.N * stride;
    w.chunks = (int)((slot + HANDOFF_THREADS - 1) / HANDOFF_THREADS), w.t_chunks = (stride + HANDOFF_THREADS - 1) / HANDOFF_THREADS;
    for (int a = 0; a < 3; ++a) w.gmin[a] = e.gmin[a], w.gres[a] = e.gres[a];
    w.time_step = e.time_step;
    w.src = src, w.Mj = Mj, w.out_len = e.out_len, w.out_path = e.out_path, w.start = e.start, w.goal = e.goal;
    w.T = T, w.init_traj = init_traj;
    const long long blocks = (long long)n * (w.chunks + w.t_chunks);
    if (n <= 0 || stride <= 0 || slot > 0x7fffffffLL || blocks > 0x7fffffffLL)
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "ecbs_plan_write_kernel: nothing to write, or more than 2^31 blocks or floats per mission");
    hipLaunchKernelGGL(ecbs_plan_write_kernel, dim3((unsigned)blocks), dim3(HANDOFF_THREADS), 0, st, w);
    return launched("ecbs_plan_write_kernel");
}

int launch_ecbs_mission_gather(const rbp_dev_ecbs& e, int n, const int* src, double* start, double* goal, double* radius, double* max_vel,
                               double* max_acc, hipStream_t st) {
    MissionGather g{};
    g.n = n, g.N = e.N, g.src = src;
    g.start = e.start, g.goal = e.goal, g.radius = e.radius, g.max_vel = e.max_vel, g.max_acc = e.max_acc;
    g.d_start = start, g.d_goal = goal, g.d_radius = radius, g.d_max_vel = max_vel, g.d_max_acc = max_acc;
    const long long blocks = ((long long)n * 25 * e.N + HANDOFF_THREADS - 1) / HANDOFF_THREADS;
    if (n <= 0 || blocks > 0x7fffffffLL) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "ecbs_mission_gather_kernel: nothing to gather, or more than 2^31 blocks");
    hipLaunchKernelGGL(ecbs_mission_gather_kernel, dim3((unsigned)blocks), dim3(HANDOFF_THREADS), 0, st, g);
    return launched("ecbs_mission_gather_kernel");
}

int launch_session_refill(const rbp_dev_ecbs& e, const DevSession& d, int n, const char* staged, int capacity_K, int max_blocks, hipStream_t st) {
    const RefillStage L(capacity_K);
    const int N = d.N, PS = d.M + 1;
    const long long slot = 3LL * N * PS;
    if (n <= 0 || n > capacity_K || slot > 0x7fffffffLL)
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "session_refill_kernel: nothing to refill, more missions than the capacity, or more than 2^31 floats per mission");
    SessionRefill r{};
    const int* src = reinterpret_cast<const int*>(staged + L.src());
    const int* Mj = reinterpret_cast<const int*>(staged + L.Mk());
    PlanWrite& w = r.w;
    w.n = n, w.N = N, w.stride = PS, w.path_stride = e.path_stride, w.compact = 1;
    for (int a = 0; a < 3; ++a) w.gmin[a] = e.gmin[a], w.gres[a] = e.gres[a];
    w.time_step = e.time_step;
    w.src = src, w.Mj = Mj, w.out_len = e.out_len, w.out_path = e.out_path, w.start = e.start, w.goal = e.goal;
    w.T = d.T, w.init_traj = const_cast<float*>(d.init_traj);
    MissionGather& g = r.g;
    g.n = n, g.N = N, g.src = src;
    g.start = e.start, g.goal = e.goal, g.radius = e.radius, g.max_vel = e.max_vel, g.max_acc = e.max_acc;
    g.d_start = const_cast<double*>(d.start), g.d_goal = const_cast<double*>(d.goal), g.d_radius = const_cast<double*>(d.radius);
    g.d_max_vel = const_cast<double*>(d.max_vel), g.d_max_acc = const_cast<double*>(d.max_acc);
    r.st_worlds = reinterpret_cast<const unsigned long long*>(staged + L.worlds());
    r.st_MBk = reinterpret_cast<const int*>(staged + L.MBk());
    r.worlds = reinterpret_cast<unsigned long long*>(const_cast<DevWorld*>(d.worlds));
    r.Mk = const_cast<int*>(d.Mk), r.MBk = const_cast<int*>(d.MBk), r.status = d.status, r.qp_order = d.qp_order;
    r.n_traj = slot * n, r.n_T = (long long)PS * n, r.n_gather = 25LL * N * n, r.n_desc = (long long)WORLD_WORDS * n;
    r.total = r.n_traj + r.n_T + r.n_gather + r.n_desc + slot_clears(r.c, d, 0, n);
    const long long blocks = std::min<long long>((r.total + REFILL_THREADS - 1) / REFILL_THREADS, std::max(max_blocks, 1));
    hipLaunchKernelGGL(session_refill_kernel, dim3((unsigned)blocks), dim3(REFILL_THREADS), 0, st, r);
    return launched("session_refill_kernel");
}

int launch_session_refill_plans(const DevSession& d, int j0, int n, const char* staged, int max_blocks, hipStream_t st) {
    namespace ps = plan_stage;
    const int N = d.N, PS = d.M + 1;
    const long long slot = 3LL * N * PS;
    if (j0 < 0 || n <= 0 || slot > 0x7fffffffLL)
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "session_refill_plans_kernel: nothing to refill, or more than 2^31 floats per mission");
    SessionRefillPlans r{};
    r.block = staged;
    r.R = ps::Round{j0, n, N, PS};
    auto doubles = [&](size_t off) { return reinterpret_cast<const double*>(staged + off); };
    MissionGather& g = r.g;
    g.n = n, g.N = N, g.src = reinterpret_cast<const int*>(staged + ps::off_src(n));
    g.start = doubles(ps::off_start(n)), g.goal = doubles(ps::off_goal(n, N)), g.radius = doubles(ps::off_radius(n, N));
    g.max_vel = doubles(ps::off_max_vel(n, N)), g.max_acc = doubles(ps::off_max_acc(n, N));
    const size_t a0 = (size_t)j0 * N;  // the first agent of slot j0
    g.d_start = const_cast<double*>(d.start) + a0 * 9, g.d_goal = const_cast<double*>(d.goal) + a0 * 9, g.d_radius = const_cast<double*>(d.radius) + a0;
    g.d_max_vel = const_cast<double*>(d.max_vel) + a0 * 3, g.d_max_acc = const_cast<double*>(d.max_acc) + a0 * 3;
    r.init_traj = const_cast<float*>(d.init_traj), r.T = d.T;
    r.worlds = reinterpret_cast<unsigned long long*>(const_cast<DevWorld*>(d.worlds) + j0);
    r.Mk = const_cast<int*>(d.Mk) + j0, r.MBk = const_cast<int*>(d.MBk) + j0, r.status = d.status + j0, r.qp_order = d.qp_order + j0;
    r.n_traj = ps::traj_elements(r.R), r.n_T = ps::time_elements(r.R), r.n_gather = 25LL * N * n, r.n_desc = (long long)WORLD_WORDS * n;
    r.total = r.n_traj + r.n_T + r.n_gather + r.n_desc + slot_clears(r.c, d, j0, n);
    const long long blocks = std::min<long long>((r.total + REFILL_THREADS - 1) / REFILL_THREADS, std::max(max_blocks, 1));
    hipLaunchKernelGGL(session_refill_plans_kernel, dim3((unsigned)blocks), dim3(REFILL_THREADS), 0, st, r);
    return launched("session_refill_plans_kernel");
}
