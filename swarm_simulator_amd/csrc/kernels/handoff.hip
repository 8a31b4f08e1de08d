// handoff.hip — from the device search's packed paths to what a session plans from, without a host trip (gfx950).
//
// ecbs_kernel (kernels/ecbs.hip) leaves every mission's paths as packed cells in HBM; a rbp_dev_ecbs keeps them there beside the missions'
// states and limits.  The two kernels here turn them into the arrays of a consumer, where the consumer wants them:
//   ecbs_plan_write_kernel      T [n][stride] and init_traj [n][N][stride][3] of the chosen missions -- the download buffer of
//                               rbp_dev_ecbs_download (stride max_M + 1, all K missions) or a session's arena (rbp_session_create_from_ecbs:
//                               stride = the largest M + 1 of the missions it holds, and inside its slot every mission is laid out with
//                               its own M + 1, as kernels/rbp_dev.h says of a session);
//   ecbs_mission_gather_kernel  start / goal / radius / max_vel / max_acc of the chosen missions into the session's [n][N][...] arrays.
// Both are one element per lane, consecutive lanes on consecutive elements of a row: plain vector loads and stores, no LDS, no atomics.
// Every value of the first is a rule of common/ecbs_rules.h (plan_time, plan_waypoint) -- the text the host's write_plan loops over -- and
// that header's `#pragma clang fp contract(off)` holds for this whole file, so the device rounds each operation as the host does.
#include "rbp_dev.h"

#include <string>

#include "common/ecbs_rules.h"

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

// The first n * chunks blocks write the slots of init_traj, one float per lane and a slot `chunks` blocks wide; the last n * t_chunks
// blocks write the rows of T.  Every element of the destination is written: what lies beyond a mission's own M is zero.
__global__ __launch_bounds__(HANDOFF_THREADS) void ecbs_plan_write_kernel(PlanWrite w) {
    const int traj_blocks = w.n * w.chunks;
    if ((int)blockIdx.x >= traj_blocks) {
        const int tb = (int)blockIdx.x - traj_blocks, j = tb / w.t_chunks;
        const int i = (tb - j * w.t_chunks) * HANDOFF_THREADS + (int)threadIdx.x;
        if (i < w.stride) w.T[(size_t)j * w.stride + i] = i <= w.Mj[j] ? ecbs_rules::plan_time(i, w.time_step) : 0.0;
        return;
    }
    const int j = (int)blockIdx.x / w.chunks;
    const int f = ((int)blockIdx.x - j * w.chunks) * HANDOFF_THREADS + (int)threadIdx.x;   // float of slot j
    const int slot = 3 * w.N * w.stride;
    if (f >= slot) return;
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

struct MissionGather {
    int n, N;
    const int* src;                                            // [n]
    const double *start, *goal, *radius, *max_vel, *max_acc;   // [K][N][9 9 1 3 3]
    double *d_start, *d_goal, *d_radius, *d_max_vel, *d_max_acc;  // [n][N][9 9 1 3 3]
};

// 25 N doubles per mission: its [N][9] start, [N][9] goal, [N] radius, [N][3] max_vel, [N][3] max_acc, one double per lane
__global__ __launch_bounds__(HANDOFF_THREADS) void ecbs_mission_gather_kernel(MissionGather g) {
    const long long t = (long long)blockIdx.x * HANDOFF_THREADS + threadIdx.x;
    const int per = 25 * g.N;
    if (t >= (long long)g.n * per) return;
    const int j = (int)(t / per);
    int r = (int)(t - (long long)j * per);
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
