// rbp_dev.h — device-side layout of one session (K missions with common N, per-mission M) and kernel entry points.
//
// Every mission has its own segment count M_k = makespan + 2 (ecbs_planner.hpp:41-43, rbp_planner.hpp:35).  A mission's
// slot in every array is sized for the session's largest M (DevSession::M, the STRIDE), but inside its slot the data is
// laid out compactly with the mission's own M_k = Mk[mission] -- exactly the layout a one-mission session would have.
//
// HBM layout (all arrays mission-major, SoA inside a mission; sizes for the headline N=64, M=36):
//   dist      [K] float grids, x-major / z-fastest (0.94 MB each)        — read by the SFC kernel
//   init_traj [K][N][M+1][3] f32 (28 KB)  T [K][M+1] f64
//   start/goal[K][N][9] f64   radius [K][N]   max_vel/max_acc [K][N][3]
//   sfc_count [K][N] i32  sfc_box [K][N][MB][6] f64  sfc_time [K][N][MB] f64
//   rsfc_normal [K][N(N-1)/2][M][3] f32 (871 KB)   rsfc_time [K][M] f64
//   ctrl / coef [K][N][3][6M] f64 (332 KB each)
//   QP workspace per mission (see QpWs in qp_base.inc)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rbp.h"

#define SP_EPSILON 1e-9        /* reference: swarm_planner/include/sp_const.hpp:3 */
#define SP_EPSILON_FLOAT 1e-6  /* sp_const.hpp:4 */
#define QP_MAX_NB 64           /* widest batch (agents) one workgroup factorises: nk = 9 * 64 = 576 */
#define QP_MAX_M 128           /* most segments per mission the QP kernel takes: 64 LDS step counters for (M - 1) / 2 chain steps, see twisted_factor */
inline int planner_max_batch() { return QP_MAX_NB; }
#define SFC_MAXS 512           /* sfc_kernel: max samples per axis (world extent / box resolution + 3); checked at session create */
#define SFC_MASK_WORDS 8192    /* occupancy bitmask of a grid: 262144 cells = 32 KB; larger grids are read as floats */

struct DevWorld {
    int dim[3];
    int key_min[3];
    double res;
    const float* dist;  // device
};

struct DevParam {
    double world_min[3], world_max[3];
    double box_xy_res, box_z_res, downwash;
    int sequential, batch_size, batch_iter, iteration, time_scale;
    int timescale_rule;  // rbp_param.timescale_rule (RBP_TIMESCALE_*)
    int polish;  // 1: active-set polish after the interior-point solve (default)
    double far_slack;  // rbp_solver_opts.qp_far_slack (kernels/qp.hip QP_FAR_SLACK); <= 0: every row near
};

// per-session pointers handed to kernels by value
struct DevSession {
    int K, N, M, max_boxes, npair;  // M, max_boxes: session maxima = slot strides; per-mission values in Mk / MBk
    const int* Mk;            // [K] segments of mission k (<= M)
    const int* MBk;           // [K] box capacity of mission k (<= max_boxes): plan.max_boxes of the caller
    int sfc_cap[3];           // sfc_kernel: capacity of the per-axis key lists = world extent / box resolution + 4 (<= SFC_MAXS)
    int sfc_mask_words;       // sfc_kernel: words of LDS reserved for the occupancy mask (largest grid of the session that fits, multiple of 4)
    int agent_begin, agent_end;  // corridor stage only: agents (and pair rows i) of this shard, [0, N) when not sharded
    DevParam p;
    const DevWorld* worlds;   // [K]
    const float* init_traj;   // [K][N][M+1][3]
    double* T;                // [K][M+1]
    const double* start;      // [K][N][9]
    const double* goal;       // [K][N][9]
    const double* radius;     // [K][N]
    const double* max_vel;    // [K][N][3]
    const double* max_acc;    // [K][N][3]
    unsigned* sfc_mask;       // [K][SFC_MASK_WORDS] bit = dist < radius(agent 0) - 1e-6, written by mask_kernel, read by sfc_kernel
    int* sfc_count;           // [K][N]
    double* sfc_box;          // [K][N][MB][6]
    double* sfc_time;         // [K][N][MB]
    float* rsfc_normal;       // [K][npair][M][3]
    double* rsfc_time;        // [K][M]
    double* ctrl;             // [K][N][3][6M]
    double* coef;             // [K][N][3][6M]
    int* status;              // [K] first error per mission (0 ok)
    double* scalars;          // [K][8]: time_scale, total_cost, ipm_iters, qp_solved, polished, ...
    unsigned long long* counters;  // [K][4]: sfc samples, ...
    // block -> mission order of the QP kernel (r03): a session that is run again starts its LONGEST missions first (wall-clock cycles
    // of each mission's workgroup in the previous run, kept across rbp_session_reset); identity on the first run.  Results do not
    // depend on the order (every mission is a workgroup of its own); nullptr disables it (RBP_QP_ORDER=0).
    int* qp_order;                 // [K]
    unsigned long long* qp_cost;   // [K]
};

enum { SC_TIME_SCALE = 0, SC_TOTAL_COST = 1, SC_IPM_ITERS = 2, SC_QP_SOLVED = 3, SC_POLISHED = 4, SC_FLOPS = 5, SC_ROWS = 6,
       SC_KKT_MAX = 7,    // max over the batch QPs of the KKT residual of the accepted answer (see rbp_plan::kkt_max)
       SC_PROF0 = 8,      // SC_PROF0..SC_PROF0+15: per-phase cycle counters (QP_PROFILE builds); slot 8 otherwise: which batch was not polished
       SC_ROW_BYTES = 24, // algorithmic HBM bytes of the QP kernel (row state, row constants, knot blocks)
       SC_SWEEP_BYTES = 28, // ... the part of SC_ROW_BYTES the three row sweeps of an interior-point iteration stream (bench.py: sweep_phase_gbs)
       SC_TIME_SCALE_ALT = 32, // the factor the other rule of rbp_param.timescale_rule gives (rbp_plan::time_scale_alt)
       SC_N = 36 };
enum { CT_SFC_SAMPLES = 0, CT_N = 4 };

// effective batch size and number of batches solved per pass (setBatch, rbp_planner.hpp:849-872; the loop of :142)
struct BatchSchedule {
    int bs, biter;
};
inline BatchSchedule batch_schedule(int sequential, int batch_size, int batch_iter, int N) {
    int bs = sequential ? batch_size : N;
    if (bs <= 0) bs = 1;
    if (bs > N) bs = N;
    const int bmax = (N + bs - 1) / bs;
    int biter = sequential ? batch_iter : 1;
    if (sequential && (biter < 0 || biter > bmax)) biter = bmax;
    return {bs, biter};
}

// build_dummy (rbp_planner.hpp:513-549): control point j of segment m of the waypoint-constant trajectory, dimension k, from one agent's
// waypoints tr[M + 1][3] -- the first three of a segment sit on its first waypoint, the last three on its second.
// (idx runs with m, one waypoint pair per segment; the `idx >= size-1` branch is unreachable for M+1 waypoints)
__device__ __forceinline__ double dummy_ctrl_point(const float* tr, int m, int j, int k) {
#pragma clang fp contract(fast)  // as in its callers' files (the Makefile's -ffp-contract=off is for corridor.hip): one fused multiply-add
    const int a = (j < 3) ? 0 : 1;
    return (1 - a) * (double)tr[3 * m + k] + a * (double)tr[3 * (m + 1) + k];
}

int rbp_set_error(int code, const char* msg);  // abi/session.hip: records the message rbp_last_error() returns, returns code

struct DeviceScope {  // the calling thread's current device is put back when the call returns
    int prev = -1;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) (void)hipSetDevice(device);
        else prev = -1;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

struct DeviceBuffers {  // device allocations of one call, freed when it returns; the first error sticks
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    template <class T>
    T* get(size_t count, bool zero = false) {
        void* p = nullptr;
        if (err == hipSuccess) err = hipMalloc(&p, std::max<size_t>(sizeof(T) * count, 16));
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(p);
        if (zero) err = hipMemsetAsync(p, 0, sizeof(T) * count, 0);
        return static_cast<T*>(p);
    }
    template <class T>
    T* upload(const std::vector<T>& v) {
        T* p = get<T>(v.size());
        if (p && !v.empty()) err = hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
        return p;
    }
    ~DeviceBuffers() {
        for (void* p : ptrs) (void)hipFree(p);
    }
};

// kernels/ecbs.hip: the ECBS search on the device (the rules it shares with csrc/host/ecbs.cpp, the planning lattice among them, are in
// common/ecbs_rules.h).  ecbs_check_arguments: the argument checks both entry points share (no device work; dim_in
// may be null, dim receives the planning lattice of param).  ecbs_plan_on_device: the search on K masks that are already on the CURRENT
// device ([K][dim0 * dim1 * dim2] bytes; d_outside [K] or null: missions whose lattice left the world's grid), results into `out`.
int ecbs_check_arguments(const char* who, int32_t K, const int32_t* dim_in, const rbp_mission* missions, const rbp_param* param,
                         int64_t max_high_level_nodes, const rbp_ecbs_out* out, int32_t dim[3]);
int ecbs_plan_on_device(const char* who, int32_t K, const int32_t dim[3], const unsigned char* d_masks, const unsigned* d_outside,
                        const rbp_mission* missions, const rbp_param* param, int64_t max_high_level_nodes, rbp_ecbs_out* out);
// what ecbs_check_arguments checks of a search apart from its rbp_ecbs_out: for the search that fills none (rbp_dev_worlds_ecbs_search)
int ecbs_check_search(const char* who, int32_t K, const int32_t* dim_in, const rbp_mission* missions, const rbp_param* param,
                      int64_t max_high_level_nodes, int32_t max_M, int32_t dim[3]);

struct PackedCell {  // a lattice cell of the device search, x | y << 10 | z << 20, as the conflict rules and the plan writer of common/ecbs_rules.h read one
    unsigned c;
    __host__ __device__ int x() const { return (int)(c & 1023u); }
    __host__ __device__ int y() const { return (int)((c >> 10) & 1023u); }
    __host__ __device__ int z() const { return (int)(c >> 20); }
    __host__ __device__ bool operator==(const PackedCell& o) const { return c == o.c; }
};

// rbp_dev_ecbs (include/rbp.h): a search whose results stay where ecbs_kernel left them.  The device arrays belong to `results`; the
// host keeps the few words the search reports per mission and what a plan's shape is computed from.
struct rbp_dev_ecbs {
    const rbp_dev_worlds* ws = nullptr;  // the set the missions were searched on (the caller keeps it alive)
    int device = 0;
    int K = 0, N = 0, max_M = 0, path_stride = 0;
    double gmin[3] = {}, gres[3] = {}, time_step = 0;  // the planning lattice and plan/time_step of the search's param
    bool have_limits = false;                        // every mission came with max_vel and max_acc (a session needs them)
    DeviceBuffers results;
    const int* status = nullptr;          // [K]
    const int* out_len = nullptr;         // [K][N] cells of each path
    const unsigned* out_path = nullptr;   // [K][N][path_stride] packed cells
    const long long* out_count = nullptr; // [K][2]
    const double *start = nullptr, *goal = nullptr, *radius = nullptr, *max_vel = nullptr, *max_acc = nullptr;  // [K][N][9 9 1 3 3]
    std::vector<int> world_index, status_h, len_h, M_h, makespan_h, sum_cost_h;  // [K] ([K][N]: len_h)
    std::vector<long long> count_h;                                               // [K][2]
};
// kernels/ecbs.hip: ecbs_plan_on_device up to and without the download of the paths -- fills `e` (but for ws / world_index) on the current device
int ecbs_search_on_device(const char* who, int32_t K, const int32_t dim[3], const unsigned char* d_masks, const unsigned* d_outside,
                          const rbp_mission* missions, const rbp_param* param, int64_t max_high_level_nodes, int32_t max_M, rbp_dev_ecbs* e);

// kernels/handoff.hip: T / init_traj from the resident paths of `e`, written where a consumer wants them.  Destination slot j takes
// mission src[j] of the search; Mj[j] is its segment count (< 0: no plan, the slot is written as zeros); both are device arrays [n].
// T [n][stride], init_traj [n][N][stride][3], stride > every Mj; compact: inside its slot mission j is [N][Mj[j] + 1][3], a session's
// layout (above).  Everything beyond a mission's own M is written as zero.
int launch_ecbs_plan_write(const rbp_dev_ecbs& e, int n, const int* src, const int* Mj, int stride, bool compact, double* T, float* init_traj,
                           hipStream_t st);
// the five mission arrays [n][N][9 9 1 3 3] gathered from the packed copies of `e` by the same source list
int launch_ecbs_mission_gather(const rbp_dev_ecbs& e, int n, const int* src, double* start, double* goal, double* radius, double* max_vel,
                               double* max_acc, hipStream_t st);

// kernels/handoff.hip: a session's slots 0 .. n-1 refilled from the resident results of `e` in ONE launch (rbp_session_refill_from_ecbs).
// `staged` is the device twin of the session's staging block, laid out by RefillStage for the session's capacity K: the world
// descriptors, then the source list, Mk and MBk of the n missions.  session_refill_kernel copies descriptors, Mk and MBk into the
// session's arrays, writes T / init_traj (the element bodies of ecbs_plan_write_kernel, compact, stride d.M + 1) and the five mission
// arrays (the element body of ecbs_mission_gather_kernel), and clears, for those slots, what a run reads before it writes or a download
// hands out beyond what a run writes: status, scalars, counters, qp_order, qp_cost, sfc_count, sfc_box, sfc_time, rsfc_normal, rsfc_time,
// ctrl and coef.  `d` holds the session's pointers and STRIDES (d.K is not read).  No allocation, no synchronisation.
struct RefillStage {
    int K;  // capacity
    explicit RefillStage(int capacity) : K(capacity) {}
    size_t worlds() const { return 0; }
    size_t src() const { return sizeof(DevWorld) * (size_t)K; }
    size_t Mk() const { return src() + sizeof(int) * (size_t)K; }
    size_t MBk() const { return Mk() + sizeof(int) * (size_t)K; }
    size_t bytes() const { return MBk() + sizeof(int) * (size_t)K; }
};
int launch_session_refill(const rbp_dev_ecbs& e, const DevSession& d, int n, const char* staged, int capacity_K, int max_blocks, hipStream_t st);
// kernels/handoff.hip: a session's slots [j0, j0 + n) refilled from ONE ROUND of a caller's plans (rbp_session_refill_from_plans) in one
// launch.  `staged` is the device twin of the plans' staging block holding that round as common/plan_stage.h lays it out (pack_round);
// session_refill_plans_kernel writes init_traj and T by that header's element rules, the mission arrays, the descriptors with Mk / MBk and
// the clears of session_refill_kernel, for those slots only.  `d` holds the session's pointers and STRIDES.
int launch_session_refill_plans(const DevSession& d, int j0, int n, const char* staged, int max_blocks, hipStream_t st);
// kernels/edt.hip: the device a set of worlds lies on
int dev_worlds_device(const rbp_dev_worlds* ws);

// kernels/report.hip: the safety ratio and flight distance of K missions (rbp_report of include/rbp.h) from device arrays in a session's
// layout.  launch_report enqueues its two kernels on `st`; the K reports are then at the front of `workspace` (report_workspace_bytes(K)
// bytes of device memory, nothing to initialise).  report_tile(N) == 0: more agents than one sample's positions fit the LDS budget for,
// which launch_report refuses with RBP_ERR_BAD_ARGUMENT before it launches anything.
struct ReportInputs {
    int K, N, M_stride;
    const int* Mk;         // [K] segments of mission k (<= M_stride)
    const double* T;       // [K][M_stride + 1], not scaled
    const double* coef;    // [K] slots of N * 3 * 6 * M_stride, mission k's own [N][3][6 Mk[k]] at the front of its slot
    const double* radius;  // [K][N]
    const double* ts;      // mission k's time scale is ts[k * ts_stride] (<= 0 reads as 1); null: 1
    int ts_stride;
    const int* status;     // [K] or null: a mission whose status is not 0 is reported as such and not evaluated
    double downwash, dt;
};
int report_tile(int N);
size_t report_workspace_bytes(int K);
int launch_report(const ReportInputs& in, void* workspace, hipStream_t st);

// kernels/dynamics.hip: the sampled states, limit peaks and ratio curves of K missions (rbp_dynamics of include/rbp.h) from device arrays in
// a session's layout.  launch_dynamics enqueues its kernels on `st` and allocates nothing; states [K][N][9][S_stride] and curves
// [K][S_stride][2] are device pointers or null; the K structs are then at the front of `workspace` (dynamics_workspace_bytes(K) bytes of
// device memory, nothing to initialise).  dynamics_tile(N) == 0: more agents than the curve kernel's LDS budget holds one sample of, which
// launch_dynamics refuses.  dynamics_run: the same with `states` / `curves` wherever the caller has them -- on `device` (the current one),
// written in place, or on the host, through bounded staging -- and the structs copied to `out` on the host; it returns when all has arrived.
struct DynamicsInputs {
    ReportInputs r;
    const double* max_vel;  // [K][N][3]
    const double* max_acc;  // [K][N][3]
};
int dynamics_tile(int N);
size_t dynamics_workspace_bytes(int K);
int launch_dynamics(const DynamicsInputs& in, double* states, double* curves, int S_stride, void* workspace, hipStream_t st);
int dynamics_run(const char* who, int device, const DynamicsInputs& in, rbp_dynamics* out, double* states, double* curves, int S_stride,
                 void* workspace, hipStream_t st);

// kernels/clearance.hip: the clearance of K missions to the obstacles of their worlds (rbp_clearance of include/rbp.h) from device arrays
// in a session's layout and a device array of K worlds whose grids lie on the device.  launch_clearance enqueues its two kernels on `st` and
// allocates nothing; agent_clearance [K][N] is a device pointer or null; the K structs are then at the front of `workspace`
// (clearance_workspace_bytes(K, N) bytes of device memory, nothing to initialise).  clearance_run: the same with `agent_clearance` wherever
// the caller has it -- on `device` (the current one), written in place, or on the host, through one staging buffer -- and the structs
// copied to `out` on the host; it returns when all has arrived.  (r.downwash is not read.)
struct ClearanceInputs {
    ReportInputs r;
    const DevWorld* worlds;  // [K] on the device
};
size_t clearance_workspace_bytes(int K, int N);
int launch_clearance(const ClearanceInputs& in, double* agent_clearance, void* workspace, hipStream_t st);
int clearance_run(const char* who, int device, const ClearanceInputs& in, rbp_clearance* out, double* agent_clearance, void* workspace, hipStream_t st);

// kernels/separation.hip: a certified interval for the smallest safety ratio of K missions in continuous time (rbp_separation of
// include/rbp.h) from device arrays in a session's layout.  launch_separation enqueues its kernels on `st` and allocates nothing;
// pair_lower [K][N (N-1) / 2] is a device pointer or null; the K structs are then at the front of `workspace`
// (separation_workspace_bytes(K, N, M_stride) bytes of device memory, nothing to initialise: the structs, and one chunk's work-list counters,
// work list and partial tallies, sized by the shapes alone).  separation_run: the same with `pair_lower` wherever the caller has it -- on
// `device` (the current one), written in place, or on the host, through one staging buffer -- and the structs copied to `out` on the host;
// it returns when all has arrived.  separation_check_arguments: depth and refine_below, no device work.  (r.dt is not read.)
struct SeparationInputs {
    ReportInputs r;
    int depth;
    double refine_below;
};
int separation_check_arguments(const char* who, int32_t depth, double refine_below);
size_t separation_workspace_bytes(int K, int N, int M_stride);
int launch_separation(const SeparationInputs& in, double* pair_lower, void* workspace, hipStream_t st);
int separation_run(const char* who, int device, const SeparationInputs& in, rbp_separation* out, double* pair_lower, void* workspace, hipStream_t st);

// kernels/swept.hip: a certified interval for the smallest clearance of K missions to the obstacles in continuous time
// (rbp_swept_clearance of include/rbp.h) from device arrays in a session's layout and a device array of K worlds whose grids lie on the
// device.  launch_swept enqueues its kernels on `st` and allocates nothing; agent_lower [K][N] is a device pointer or null; the K structs
// are then at the front of `workspace` (swept_workspace_bytes(K, N, M_stride) bytes of device memory, nothing to initialise: the structs,
// and one chunk's work-list counters, work list, item clearances and partial tallies, sized by the shapes alone).  swept_run: the same
// with `agent_lower` wherever the caller has it -- on `device` (the current one), written in place, or on the host, through one staging
// buffer -- and the structs copied to `out` on the host; it returns when all has arrived.  swept_check_arguments: depth and refine_below,
// no device work.  (r.dt and r.downwash are not read.)
struct SweptInputs {
    ReportInputs r;
    const DevWorld* worlds;  // [K] on the device
    int depth;
    double refine_below;
};
int swept_check_arguments(const char* who, int32_t depth, double refine_below);
size_t swept_workspace_bytes(int K, int N, int M_stride);
int launch_swept(const SweptInputs& in, double* agent_lower, void* workspace, hipStream_t st);
int swept_run(const char* who, int device, const SweptInputs& in, rbp_swept_clearance* out, double* agent_lower, void* workspace, hipStream_t st);

// kernels/limits.hip: certified intervals for the largest velocity and acceleration ratios of K missions in continuous time (rbp_limits of
// include/rbp.h) from device arrays in a session's layout.  launch_limits enqueues its kernels on `st` and allocates nothing; agent_upper
// [K][N][2] is a device pointer or null; the K structs are then at the front of `workspace` (limits_workspace_bytes(K, N, M_stride) bytes
// of device memory, nothing to initialise: the structs, and one chunk's work-list counters, work list, item ratios and partial tallies,
// sized by the shapes alone).  limits_run: the same with `agent_upper` wherever the caller has it -- on `device` (the current one), written
// in place, or on the host, through one staging buffer -- and the structs copied to `out` on the host; it returns when all has arrived.
// limits_check_arguments: depth and refine_above, no device work.  (r.radius, r.dt and r.downwash are not read.)
struct LimitsInputs {
    ReportInputs r;
    const double* max_vel;  // [K][N][3]
    const double* max_acc;  // [K][N][3]
    int depth;
    double refine_above;
};
int limits_check_arguments(const char* who, int32_t depth, double refine_above);
size_t limits_workspace_bytes(int K, int N, int M_stride);
int launch_limits(const LimitsInputs& in, double* agent_upper, void* workspace, hipStream_t st);
int limits_run(const char* who, int device, const LimitsInputs& in, rbp_limits* out, double* agent_upper, void* workspace, hipStream_t st);

// launchers (defined in the .hip files)
int launch_corridor(const DevSession& s, hipStream_t st);
size_t corridor_lds_bytes(const DevSession& s);  // dynamic LDS of sfc_kernel for this session's shapes
// kernels/traj.hip: build_dummy in front of a QP solve of either kind (batch: kernels/qp.hip, joint: kernels/jqp.hip), Bernstein -> monomial
// + timeScale behind it
void launch_planner_prologue(const DevSession& s, hipStream_t st);
void launch_planner_epilogue(const DevSession& s, hipStream_t st);
// kernels/qp.hip is built twice, both with 256 VGPRs: _w2 = 512 threads, one workgroup per CU; _w4 = 256 threads, two workgroups per CU
void launch_planner_w2(const DevSession& s, void* qp_ws, size_t qp_ws_bytes_per_mission, hipStream_t st);
void launch_planner_w4(const DevSession& s, void* qp_ws, size_t qp_ws_bytes_per_mission, hipStream_t st);
size_t planner_workspace_bytes_w2(int N, int M, int batch_size_eff);
size_t planner_workspace_bytes_w4(int N, int M, int batch_size_eff);
