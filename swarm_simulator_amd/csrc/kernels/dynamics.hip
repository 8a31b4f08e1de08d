// dynamics.hip — the sampled states of resident plans, their limit peaks and their ratio curves, where the coefficients are: in HBM (gfx950).
//
// What the reference's publisher samples of a plan besides the two numbers of report.hip (rbp_publisher.hpp:670-683, 697-767, 769-798) for K
// missions in two or three launches, from a session's own arrays (rbp_session_dynamics, abi/session.hip) or a caller's (rbp_dev_dynamics):
//   dynamics_state_kernel   DYN_BLOCKS workgroups per mission.  The (agent, sample) items of a mission are cut into chunks of 64 consecutive
//                           samples of one agent, numbered sample block first, agent second; every wavefront takes every
//                           (DYN_BLOCKS * 4)-th chunk, so its lanes sit on consecutive samples of one agent: the agent's coefficients are
//                           read once per wavefront and segment, a row of the output [agent][row][sample] is stored as 512 contiguous
//                           bytes, and -- because a wavefront's chunks ascend in time -- each lane's segment count runs along its samples
//                           (segments_before with `from`).  A lane evaluates the nine values, stores them where a states buffer was given and
//                           the samples fit its rows, and folds its six limit ratios into its two running peaks; the workgroup reduces the
//                           peaks through LDS and writes one pair per (workgroup, mission).  The number of samples depends on the time scale,
//                           which only the device knows: the wavefronts loop, the grid does not grow.
//   dynamics_curve_kernel   only when curves are asked for; report.hip's tile scheme: the positions of a tile of samples go into LDS (same
//                           32 KB budget, same tile), then each wavefront takes every 4th sample of the tile, its lanes the pairs; minimum
//                           and maximum are reduced across the wavefront by shuffles and lane 0 stores curve[sample][0..1].  Every sample
//                           belongs to exactly one wavefront: nothing is merged across workgroups.  (The tile loader is a copy of
//                           report.hip's loop, local to this file: report.hip is not touched.)
//   dynamics_finish_kernel  one wavefront per mission: merges the partial peaks and writes the rbp_dynamics.
// Every number is a rule of common/state_rules.h -- the text rbp_dynamics_host (host/validate.cpp) loops over -- and the headers'
// `#pragma clang fp contract(off)` holds for this whole file.  Peaks are kept under an order (state_rules::take) and curves by value, so
// nothing depends on which lane or workgroup met a candidate first: no floating-point atomics.  Plain C++, vector stores only.
#include "rbp_dev.h"

#include <string>
#include <type_traits>

#include "common/state_rules.h"

namespace {

constexpr int DYN_THREADS = 256;
constexpr int DYN_WAVES = DYN_THREADS / 64;
constexpr int DYN_BLOCKS = 16;             // workgroups per mission of the state and the curve kernel
constexpr int DYN_CHUNK = 64;              // samples of a chunk: one per lane
constexpr int CURVE_TILE_MAX = 64;         // most samples of a curve tile
constexpr int CURVE_POS_BYTES = 32 * 1024; // LDS budget of a tile's positions, 24 bytes per agent and sample
constexpr size_t DYN_STAGE_BYTES = (size_t)64 << 20;  // RBP_DYNAMICS_STAGE_BYTES of include/rbp.h

using state_rules::Curve;
using state_rules::Peak;
typedef __attribute__((address_space(1))) double gdouble;

static_assert(sizeof(Peak) == 40, "three doubles, three indices and a pad");
static_assert(sizeof(rbp_dynamics) == 96, "seven doubles and ten words");

// dynamic LDS of dynamics_curve_kernel: the tile's segment counts, the tile's positions [sample][agent][3]
constexpr int CURVE_LDS_BEFORE = 0;
constexpr int CURVE_LDS_POS = CURVE_LDS_BEFORE + CURVE_TILE_MAX * (int)sizeof(int);
static_assert(CURVE_LDS_POS % 16 == 0, "every carve offset a multiple of 16");

struct DynArgs {
    DynamicsInputs in;
    int tile;           // samples per curve tile: dynamics_tile(N)
    int S_stride;       // samples a row of states / curves holds
    double* states;     // [K][N][9][S_stride] on the device, or null
    double* curves;     // [K][S_stride][2] on the device, or null
    Peak* partial;      // [K][DYN_BLOCKS][2]: velocity, acceleration
    rbp_dynamics* out;  // [K]
};

struct MissionView {
    int M, samples;
    double ts, end_time;
    const double *T, *coef, *radius;
    bool computed;  // false: a mission with a status, or with more samples than are evaluated
};

__device__ __forceinline__ MissionView mission_view(const ReportInputs& in, int k) {
    MissionView v;
    v.M = in.Mk[k];
    const double q = in.ts ? in.ts[(size_t)k * in.ts_stride] : 1.0;
    v.ts = q > 0 ? q : 1.0;  // (rbp_session_download: a scalar that was never written is no scale)
    v.T = in.T + (size_t)k * (in.M_stride + 1);
    v.coef = in.coef + (size_t)k * in.N * 3 * 6 * in.M_stride;
    v.radius = in.radius + (size_t)k * in.N;
    v.end_time = report_rules::scaled_time(v.T[v.M], v.ts);
    v.samples = report_rules::sample_count(v.end_time, in.dt);
    v.computed = !(in.status && in.status[k] != 0) && v.samples >= 0;
    return v;
}

// pair e of the N (N - 1) / 2 of a mission (report.hip's decoding: each unordered pair once, one division; which e names which pair does
// not matter, a curve keeps values only)
__device__ __forceinline__ void pair_of(int e, int N, int* qi, int* qj) {
    const int h = (N - 1) / 2;
    int d, a;
    if (e < N * h) {
        d = e / N;
        a = e - d * N;
        d += 1;
    } else {
        d = N / 2;
        a = e - N * h;
    }
    int b = a + d;
    if (b >= N) b -= N;
    *qi = a < b ? a : b;
    *qj = a < b ? b : a;
}

// the workgroup's peak under the rule's order, in red[0] when it returns
__device__ __forceinline__ void reduce_peaks(Peak* red, int tid, const Peak& mine) {
    red[tid] = mine;
    __syncthreads();
    for (int off = DYN_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) state_rules::take(&red[tid], red[tid + off]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(DYN_THREADS, 8) void dynamics_state_kernel(DynArgs g) {
    extern __shared__ __attribute__((aligned(16))) char dynamics_lds[];
    Peak* red = reinterpret_cast<Peak*>(dynamics_lds);  // [DYN_THREADS] (an LDS address to the compiler: ds_ instructions, see profiles/dynamics_isa.txt)
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, N = g.in.r.N;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (the same in every lane: chunk, agent and limits are scalars)
    const MissionView v = mission_view(g.in.r, k);
    Peak vel = state_rules::no_peak(), acc = state_rules::no_peak();
    if (v.computed) {
        const bool store = g.states && v.samples <= g.S_stride;
        const double* lim_v = g.in.max_vel + (size_t)k * N * 3;
        const double* lim_a = g.in.max_acc + (size_t)k * N * 3;
        gdouble* dst = (gdouble*)g.states + (size_t)k * N * 9 * g.S_stride;
        const int chunks = ((v.samples + DYN_CHUNK - 1) / DYN_CHUNK) * N;  // (at most 2^14 sample blocks of at most 1365 agents)
        int before = 0;
        for (int c = (int)blockIdx.x * DYN_WAVES + wave; c < chunks; c += DYN_BLOCKS * DYN_WAVES) {
            const int sb = c / N, a = c - sb * N, j = sb * DYN_CHUNK + lane;
            if (j < v.samples) {
                const double t = report_rules::sample_time(j, g.in.r.dt);
                before = report_rules::segments_before(v.T, v.M, v.ts, t, before);  // (this lane's samples ascend)
                const int m = report_rules::segment_index(before);
                const double tseg = report_rules::segment_time(v.T, v.ts, t, before);
                gdouble* row = dst + (size_t)a * 9 * g.S_stride + j;  // (stored only where j < samples <= S_stride)
#pragma unroll 1
                for (int ax = 0; ax < 3; ++ax) {  // state_rules::agent_state and take_state, an axis at a time
                    double p, vv, aa;
                    state_rules::axis_state(report_rules::coef_of(v.coef, v.M, a, ax, m), tseg, &p, &vv, &aa);
                    if (store) row[(size_t)ax * g.S_stride] = p, row[(size_t)(3 + ax) * g.S_stride] = vv, row[(size_t)(6 + ax) * g.S_stride] = aa;
                    state_rules::take_axis(&vel, &acc, vv, aa, lim_v[3 * a + ax], lim_a[3 * a + ax], j, a, ax);
                }
            }
        }
    }
    Peak* out = g.partial + ((size_t)k * DYN_BLOCKS + blockIdx.x) * 2;
    reduce_peaks(red, tid, vel);
    if (tid == 0) out[0] = red[0];
    __syncthreads();  // (the second reduction overwrites red[0])
    reduce_peaks(red, tid, acc);
    if (tid == 0) out[1] = red[0];
}

__global__ __launch_bounds__(DYN_THREADS) void dynamics_curve_kernel(DynArgs g) {
    extern __shared__ __attribute__((aligned(16))) char dynamics_lds[];
    int* before = reinterpret_cast<int*>(dynamics_lds + CURVE_LDS_BEFORE);
    double* pos = reinterpret_cast<double*>(dynamics_lds + CURVE_LDS_POS);
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, N = g.in.r.N, npair = N * (N - 1) / 2;
    const MissionView v = mission_view(g.in.r, k);
    if (!v.computed || v.samples > g.S_stride) return;  // (the same in every lane of the workgroup: no barrier is left waiting)
    gdouble* dst = (gdouble*)g.curves + (size_t)k * 2 * g.S_stride;
    for (int first = (int)blockIdx.x * g.tile; first < v.samples; first += DYN_BLOCKS * g.tile) {
        const int len = min(g.tile, v.samples - first);
        if (tid < len) before[tid] = report_rules::segments_before(v.T, v.M, v.ts, report_rules::sample_time(first + tid, g.in.r.dt), 0);
        __syncthreads();
        for (int i = tid; i < len * N; i += DYN_THREADS) {
            const int a = i / len, s = i - a * len;
            report_rules::agent_position(v.coef, v.M, v.T, v.ts, a, report_rules::sample_time(first + s, g.in.r.dt), before[s], pos + 3 * (s * N + a));
        }
        __syncthreads();
        for (int s = wave; s < len; s += DYN_WAVES) {
            Curve c = state_rules::no_curve();
            for (int e = lane; e < npair; e += 64) {
                int qi, qj;
                pair_of(e, N, &qi, &qj);
                state_rules::curve_take(&c, report_rules::safety_ratio(pos + 3 * (s * N + qi), pos + 3 * (s * N + qj), g.in.r.downwash, v.radius[qi] + v.radius[qj]));
            }
            for (int off = 32; off > 0; off >>= 1) state_rules::curve_merge(&c, Curve{__shfl_xor(c.min_ratio, off), __shfl_xor(c.max_ratio, off)});
            if (lane == 0) dst[2 * (size_t)(first + s)] = c.min_ratio, dst[2 * (size_t)(first + s) + 1] = c.max_ratio;  // first + s < samples <= S_stride
        }
        __syncthreads();  // (the next tile overwrites the positions)
    }
}

__global__ __launch_bounds__(64) void dynamics_finish_kernel(DynArgs g) {
    const int k = (int)blockIdx.x;
    if (threadIdx.x != 0) return;
    const MissionView v = mission_view(g.in.r, k);
    rbp_dynamics r;
    r.status = g.in.r.status ? g.in.r.status[k] : 0;
    Peak vel = state_rules::no_peak(), acc = state_rules::no_peak();
    if (r.status != 0) {  // nothing is computed of a mission that has failed
        r.end_time = 0.0, r.samples = 0, r.stored = 0;
    } else {
        if (v.computed)
            for (int b = 0; b < DYN_BLOCKS; ++b) {
                state_rules::take(&vel, g.partial[((size_t)k * DYN_BLOCKS + b) * 2]);
                state_rules::take(&acc, g.partial[((size_t)k * DYN_BLOCKS + b) * 2 + 1]);
            }
        r.end_time = v.end_time, r.samples = v.samples;
        r.stored = state_rules::stores(v.samples, g.states || g.curves, g.S_stride) ? 1 : 0;
    }
    r.peak_vel_ratio = vel.ratio, r.peak_vel = vel.value, r.peak_vel_limit = vel.limit;
    r.peak_acc_ratio = acc.ratio, r.peak_acc = acc.value, r.peak_acc_limit = acc.limit;
    r.vel_sample = vel.sample, r.vel_agent = vel.agent, r.vel_axis = vel.axis;
    r.acc_sample = acc.sample, r.acc_agent = acc.agent, r.acc_axis = acc.axis;
    g.out[k] = r;
}

size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

// missions k0 .. k0 + n of `g` as a launch of their own (the kernels index by mission through the pointers)
DynArgs slice(const DynArgs& g, int k0, int n) {
    DynArgs s = g;
    ReportInputs& r = s.in.r;
    const size_t N = (size_t)r.N;
    r.K = n, r.Mk += k0, r.T += (size_t)k0 * (r.M_stride + 1), r.coef += (size_t)k0 * N * 3 * 6 * r.M_stride, r.radius += (size_t)k0 * N;
    if (r.ts) r.ts += (size_t)k0 * r.ts_stride;
    if (r.status) r.status += k0;
    s.in.max_vel += (size_t)k0 * N * 3, s.in.max_acc += (size_t)k0 * N * 3;
    if (s.states) s.states += (size_t)k0 * N * 9 * s.S_stride;
    if (s.curves) s.curves += (size_t)k0 * 2 * s.S_stride;
    s.out += k0, s.partial += (size_t)k0 * DYN_BLOCKS * 2;
    return s;
}

// where a destination lies, as rbp_session_create classifies rbp_world.dist: a pointer the runtime does not know is reported as an error or
// as unregistered memory, depending on the runtime: both mean host.  1: on `device`; 0: host; -1: on another device
int on_device(const void* p, int device) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // (the error is sticky)
        return 0;
    }
    if (at.type != hipMemoryTypeDevice) return 0;
    return at.device == device ? 1 : -1;
}

}  // namespace

// samples per tile of dynamics_curve_kernel for N agents: report_tile's number; 0: not even one
int dynamics_tile(int N) {
    if (N <= 0) return 0;
    return std::min(CURVE_TILE_MAX, CURVE_POS_BYTES / (24 * N));
}

size_t dynamics_workspace_bytes(int K) { return al256(sizeof(rbp_dynamics) * (size_t)K) + sizeof(Peak) * (size_t)K * DYN_BLOCKS * 2; }

int launch_dynamics(const DynamicsInputs& in, double* states, double* curves, int S_stride, void* workspace, hipStream_t st) {
    DynArgs g{};
    g.in = in, g.tile = dynamics_tile(in.r.N), g.S_stride = S_stride, g.states = states, g.curves = curves;
    const int K = in.r.K;
    if (K <= 0 || K > 65535 * 16 || g.tile <= 0 || ((states || curves) && S_stride < 1))
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, ("dynamics: no mission, no room for a sample, or " + std::to_string(in.r.N) + " agents: the positions of one sample (24 bytes per agent) must fit " +
                                                    std::to_string(CURVE_POS_BYTES) + " bytes of LDS").c_str());
    g.out = static_cast<rbp_dynamics*>(workspace);
    g.partial = reinterpret_cast<Peak*>(static_cast<char*>(workspace) + al256(sizeof(rbp_dynamics) * (size_t)K));
    const size_t state_lds = sizeof(Peak) * DYN_THREADS, curve_lds = (size_t)CURVE_LDS_POS + (size_t)24 * in.r.N * g.tile;
    // gridDim.y holds at most 65535 missions: more go in slices
    for (int k0 = 0; k0 < K; k0 += 65535) {
        const int n = std::min(65535, K - k0);
        const DynArgs s = slice(g, k0, n);
        hipLaunchKernelGGL(dynamics_state_kernel, dim3(DYN_BLOCKS, (unsigned)n), dim3(DYN_THREADS), state_lds, st, s);
        if (curves) hipLaunchKernelGGL(dynamics_curve_kernel, dim3(DYN_BLOCKS, (unsigned)n), dim3(DYN_THREADS), curve_lds, st, s);
        hipLaunchKernelGGL(dynamics_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string("dynamics kernels: launch: ") + hipGetErrorString(e)).c_str());
}

// The kernels on device inputs, results to wherever the caller wants them (the current device is `device`).  A destination on the device
// is written in place by the kernels; a host destination goes through a staging allocation of at most DYN_STAGE_BYTES (one mission's rows
// where those are larger), chunk of missions by chunk: the structs of a chunk come back first and say which missions were stored and how
// many samples each has, then only those entries are copied, so that everything else of the host buffer stays as it was.
int dynamics_run(const char* who, int device, const DynamicsInputs& in, rbp_dynamics* out, double* states, double* curves, int S_stride,
                 void* workspace, hipStream_t st) {
    auto fail = [&](hipError_t err) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(err)).c_str()); };
    const int sd = states ? on_device(states, device) : 1, cd = curves ? on_device(curves, device) : 1;
    if (sd < 0 || cd < 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": states / curves lie on another device than the plans (device " + std::to_string(device) + ")").c_str());
    const int K = in.r.K;
    const size_t N = (size_t)in.r.N, srow = N * 9 * (size_t)S_stride, crow = 2 * (size_t)S_stride;
    auto structs = [&](int k0, int n) { return hipMemcpyAsync(out + k0, static_cast<rbp_dynamics*>(workspace) + k0, sizeof(rbp_dynamics) * (size_t)n, hipMemcpyDeviceToHost, st); };
    if (sd && cd) {
        if (int rc = launch_dynamics(in, states, curves, S_stride, workspace, st)) return rc;
        hipError_t e = structs(0, K);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e == hipSuccess ? RBP_OK : fail(e);
    }
    const size_t per = sizeof(double) * ((sd ? 0 : srow) + (cd ? 0 : crow));
    const int chunk = (int)std::min<size_t>((size_t)std::min(K, 65535), std::max<size_t>(1, DYN_STAGE_BYTES / per));
    DeviceBuffers b;
    double* stage_s = sd ? nullptr : b.get<double>(srow * chunk);
    double* stage_c = cd ? nullptr : b.get<double>(crow * chunk);
    if (b.err != hipSuccess) return fail(b.err);
    DynArgs whole{};  // (only to slice the inputs and the workspace by the one rule)
    whole.in = in, whole.S_stride = S_stride, whole.states = sd ? states : nullptr, whole.curves = cd ? curves : nullptr;
    whole.out = static_cast<rbp_dynamics*>(workspace);
    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int n = std::min(chunk, K - k0);
        const DynArgs s = slice(whole, k0, n);
        if (int rc = launch_dynamics(s.in, sd ? s.states : stage_s, cd ? s.curves : stage_c, S_stride, s.out, st)) return rc;
        // (a chunk's structs are at the front of ITS workspace, which is the whole workspace from mission k0 on; the partial peaks behind
        //  them lie inside the whole workspace too: al256(n structs) + n partials <= the same of K - k0 missions)
        hipError_t e = structs(k0, n);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        for (int i = 0; i < n && e == hipSuccess; ++i) {
            const rbp_dynamics& r = out[k0 + i];
            if (!r.stored || r.samples <= 0) continue;
            if (!sd)
                e = hipMemcpy2DAsync(states + (size_t)(k0 + i) * srow, sizeof(double) * S_stride, stage_s + (size_t)i * srow, sizeof(double) * S_stride,
                                     sizeof(double) * r.samples, N * 9, hipMemcpyDeviceToHost, st);
            if (!cd && e == hipSuccess)
                e = hipMemcpyAsync(curves + (size_t)(k0 + i) * crow, stage_c + (size_t)i * crow, sizeof(double) * 2 * r.samples, hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the next chunk overwrites the staging)
        if (e != hipSuccess) return fail(e);
    }
    return RBP_OK;
}

extern "C" int rbp_dev_dynamics(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T, const double* time_scale,
                                const double* coef, const double* radius, const double* max_vel, const double* max_acc, double downwash,
                                double dt, rbp_dynamics* out, double* states, double* curves, int32_t S_stride) {
    auto bad = [&](const std::string& what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, ("rbp_dev_dynamics: " + what).c_str()); };
    if (!M || !T || !coef || !radius || !max_vel || !max_acc || !out) return bad("M, T, coef, radius, max_vel, max_acc and out must be given");
    if (K <= 0 || N <= 0 || M_stride <= 0 || !(dt > 0) || !(downwash > 0)) return bad("K, N, M_stride, dt and downwash must be positive");
    if ((states || curves) && S_stride < 1) return bad("S_stride must be at least 1 where states or curves are given");
    for (int k = 0; k < K; ++k) {
        if (M[k] <= 0 || M[k] > M_stride) return bad("mission " + std::to_string(k) + ": M outside 1..M_stride");
        if (time_scale && !(time_scale[k] > 0)) return bad("mission " + std::to_string(k) + ": the time scale must be positive");
    }
    if (dynamics_tile(N) <= 0 || K > 65535 * 16)
        return bad(std::to_string(N) + " agents: the positions of one sample (24 bytes per agent) must fit " + std::to_string(CURVE_POS_BYTES) + " bytes of LDS");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rbp_set_error(RBP_ERR_NO_DEVICE, "no HIP device: the dynamics kernels have no CPU fallback (rbp_dynamics_host is the host's)");
    if (device < 0) (void)hipGetDevice(&device);
    if (device < 0 || device >= ndev) return rbp_set_error(RBP_ERR_NO_DEVICE, "device index out of range");
    DeviceScope scope(device);
    DeviceBuffers b;
    auto up = [&](const auto* src, size_t n) {
        using E = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
        E* p = b.get<E>(n);
        if (p) b.err = hipMemcpy(p, src, sizeof(E) * n, hipMemcpyHostToDevice);
        return p;
    };
    DynamicsInputs in{};
    ReportInputs& r = in.r;
    r.K = K, r.N = N, r.M_stride = M_stride, r.downwash = downwash, r.dt = dt;
    r.Mk = up(M, (size_t)K);
    r.T = up(T, (size_t)K * (M_stride + 1));
    r.coef = up(coef, (size_t)K * N * 3 * 6 * M_stride);
    r.radius = up(radius, (size_t)K * N);
    r.ts = time_scale ? up(time_scale, (size_t)K) : nullptr, r.ts_stride = 1;
    r.status = nullptr;
    in.max_vel = up(max_vel, (size_t)K * N * 3);
    in.max_acc = up(max_acc, (size_t)K * N * 3);
    char* ws = b.get<char>(dynamics_workspace_bytes(K));
    if (b.err != hipSuccess) return rbp_set_error(RBP_ERR_HIP, (std::string("rbp_dev_dynamics: ") + hipGetErrorString(b.err)).c_str());
    return dynamics_run("rbp_dev_dynamics", device, in, out, states, curves, S_stride, ws, 0);
}
