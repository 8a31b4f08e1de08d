// report.hip — a mission's safety ratio and flight distance where its coefficients are: in HBM (gfx950).
//
// The two acceptance signals of the reference (rbp_publisher.hpp:685-695, 769-798) for K missions in two launches, from a session's own
// arrays (rbp_session_report, abi/session.hip) or from a caller's, uploaded once (rbp_dev_report, below):
//   report_pair_kernel    REPORT_BLOCKS workgroups per mission.  A workgroup takes every REPORT_BLOCKS-th TILE of samples: it writes the
//                         positions of all N agents at the tile's samples into LDS (one lane per (agent, sample), consecutive lanes on
//                         consecutive samples of one agent, so a wavefront reads one agent's coefficients), then its lanes take the
//                         (pair, sample) items of the tile, each keeping the minimum it has seen and where; one minimum per workgroup
//                         goes to HBM.  The number of samples depends on the time scale, which only the device knows: the workgroups
//                         loop, the grid does not grow.
//   report_finish_kernel  one wavefront per mission: one lane per agent (strided beyond 64) walks that agent's samples in ascending order
//                         and sums its steps; lane 0 then merges the mission's partial minima, sums the agents' lengths in ascending
//                         order and writes the rbp_report.
// Every number is a rule of common/report_rules.h -- the text rbp_report_host (host/validate.cpp) loops over -- and that header's
// `#pragma clang fp contract(off)` holds for this whole file, so the device rounds each operation as the host does; the minimum is kept
// under an order (report_rules::take) that does not depend on which lane or workgroup met a candidate first.  Plain C++, vector stores only.
#include "rbp_dev.h"

#include <string>
#include <type_traits>

#include "common/report_rules.h"

namespace {

constexpr int REPORT_THREADS = 256;
constexpr int REPORT_BLOCKS = 16;            // workgroups per mission of report_pair_kernel
constexpr int REPORT_TILE_MAX = 64;          // most samples of a tile
constexpr int REPORT_POS_BYTES = 32 * 1024;  // LDS budget of a tile's positions, 24 bytes per agent and sample

using report_rules::Minimum;

// dynamic LDS of report_pair_kernel: the workgroup's minima, the tile's segment counts, the tile's positions [sample][agent][3]
constexpr int PAIR_LDS_MIN = 0;
constexpr int PAIR_LDS_BEFORE = PAIR_LDS_MIN + REPORT_THREADS * (int)sizeof(Minimum);
constexpr int PAIR_LDS_POS = PAIR_LDS_BEFORE + REPORT_TILE_MAX * (int)sizeof(int);
static_assert(sizeof(Minimum) == 24 && PAIR_LDS_BEFORE % 16 == 0 && PAIR_LDS_POS % 16 == 0, "every carve offset a multiple of 16");

struct ReportArgs {
    ReportInputs in;
    int tile;          // samples per tile: report_tile(N)
    Minimum* partial;  // [K][REPORT_BLOCKS]
    rbp_report* out;   // [K]
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

// pair e of the N (N - 1) / 2 of a mission, as (qi, qi + d mod N): d = 1 .. (N - 1) / 2 for every qi, and for an even N the distance N / 2
// for the first N / 2 agents -- each unordered pair once, decoded with one division.  Which e names which pair does not matter: the
// minimum is kept under the order of the rule.
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

__global__ __launch_bounds__(REPORT_THREADS) void report_pair_kernel(ReportArgs g) {
    extern __shared__ __attribute__((aligned(16))) char report_lds[];
    Minimum* red = reinterpret_cast<Minimum*>(report_lds + PAIR_LDS_MIN);
    int* before = reinterpret_cast<int*>(report_lds + PAIR_LDS_BEFORE);
    double* pos = reinterpret_cast<double*>(report_lds + PAIR_LDS_POS);
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, N = g.in.N, npair = N * (N - 1) / 2;
    const MissionView v = mission_view(g.in, k);
    Minimum best = report_rules::no_minimum();
    if (v.computed && npair > 0) {
        for (int first = (int)blockIdx.x * g.tile; first < v.samples; first += REPORT_BLOCKS * g.tile) {
            const int len = min(g.tile, v.samples - first);
            if (tid < len) before[tid] = report_rules::segments_before(v.T, v.M, v.ts, report_rules::sample_time(first + tid, g.in.dt), 0);
            __syncthreads();
            for (int i = tid; i < len * N; i += REPORT_THREADS) {
                const int a = i / len, s = i - a * len;
                report_rules::agent_position(v.coef, v.M, v.T, v.ts, a, report_rules::sample_time(first + s, g.in.dt), before[s],
                                             pos + 3 * (s * N + a));
            }
            __syncthreads();
            for (int i = tid; i < len * npair; i += REPORT_THREADS) {
                const int s = i / npair;
                int qi, qj;
                pair_of(i - s * npair, N, &qi, &qj);
                const double r = report_rules::safety_ratio(pos + 3 * (s * N + qi), pos + 3 * (s * N + qj), g.in.downwash, v.radius[qi] + v.radius[qj]);
                report_rules::take(&best, Minimum{r, first + s, qi, qj});
            }
            __syncthreads();  // (the next tile overwrites the positions)
        }
    }
    red[tid] = best;
    __syncthreads();
    for (int off = REPORT_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) report_rules::take(&red[tid], red[tid + off]);
        __syncthreads();
    }
    if (tid == 0) g.partial[(size_t)k * REPORT_BLOCKS + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void report_finish_kernel(ReportArgs g) {
    extern __shared__ __attribute__((aligned(16))) char report_lds[];
    double* len = reinterpret_cast<double*>(report_lds);  // [N] the agents' path lengths
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x, N = g.in.N;
    const MissionView v = mission_view(g.in, k);
    if (v.computed) {
        for (int a = lane; a < N; a += 64) {
            double sum = 0.0, prev[3] = {0.0, 0.0, 0.0}, cur[3];
            int before = 0;
            for (int j = 0; j < v.samples; ++j) {
                const double t = report_rules::sample_time(j, g.in.dt);
                before = report_rules::segments_before(v.T, v.M, v.ts, t, before);
                report_rules::agent_position(v.coef, v.M, v.T, v.ts, a, t, before, cur);
                if (j > 0) sum = sum + report_rules::step_length(prev, cur);
                prev[0] = cur[0], prev[1] = cur[1], prev[2] = cur[2];
            }
            len[a] = sum;
        }
    }
    __syncthreads();
    if (lane != 0) return;
    rbp_report r;
    r.status = g.in.status ? g.in.status[k] : 0, r.reserved = 0;
    if (r.status != 0) {  // nothing is computed of a mission that has failed
        r.min_safety_ratio = 0.0, r.total_flight_distance = 0.0, r.end_time = 0.0;
        r.samples = 0, r.min_sample = -1, r.min_qi = -1, r.min_qj = -1;
    } else {
        Minimum best = report_rules::no_minimum();
        double total = 0.0;
        if (v.computed) {
            for (int b = 0; b < REPORT_BLOCKS; ++b) report_rules::take(&best, g.partial[(size_t)k * REPORT_BLOCKS + b]);
            for (int a = 0; a < N; ++a) total = total + len[a];
        }
        r.min_safety_ratio = best.ratio, r.total_flight_distance = total, r.end_time = v.end_time;
        r.samples = v.samples, r.min_sample = best.sample, r.min_qi = best.qi, r.min_qj = best.qj;
    }
    g.out[k] = r;
}

size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

// samples per tile of report_pair_kernel for N agents: as many as REPORT_POS_BYTES hold, at most REPORT_TILE_MAX; 0: not even one
int report_tile(int N) {
    if (N <= 0) return 0;
    return std::min(REPORT_TILE_MAX, REPORT_POS_BYTES / (24 * N));
}

size_t report_workspace_bytes(int K) { return al256(sizeof(rbp_report) * (size_t)K) + sizeof(Minimum) * (size_t)K * REPORT_BLOCKS; }

int launch_report(const ReportInputs& in, void* workspace, hipStream_t st) {
    ReportArgs g{};
    g.in = in, g.tile = report_tile(in.N);
    if (in.K <= 0 || in.K > 65535 * 16 || g.tile <= 0)
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, ("report: no mission, or " + std::to_string(in.N) + " agents: the positions of one sample (24 bytes per agent) must fit " +
                                                    std::to_string(REPORT_POS_BYTES) + " bytes of LDS").c_str());
    g.out = static_cast<rbp_report*>(workspace);
    g.partial = reinterpret_cast<Minimum*>(static_cast<char*>(workspace) + al256(sizeof(rbp_report) * (size_t)in.K));
    const size_t pair_lds = (size_t)PAIR_LDS_POS + (size_t)24 * in.N * g.tile, finish_lds = ((size_t)8 * in.N + 15) & ~size_t(15);
    // gridDim.y holds at most 65535 missions: more go in slices (the kernels index by mission through the pointers)
    for (int k0 = 0; k0 < in.K; k0 += 65535) {
        ReportArgs s = g;
        const int n = std::min(65535, in.K - k0);
        s.in.K = n, s.in.Mk += k0, s.in.T += (size_t)k0 * (in.M_stride + 1), s.in.coef += (size_t)k0 * in.N * 3 * 6 * in.M_stride, s.in.radius += (size_t)k0 * in.N;
        if (s.in.ts) s.in.ts += (size_t)k0 * in.ts_stride;
        if (s.in.status) s.in.status += k0;
        s.out += k0, s.partial += (size_t)k0 * REPORT_BLOCKS;
        hipLaunchKernelGGL(report_pair_kernel, dim3(REPORT_BLOCKS, (unsigned)n), dim3(REPORT_THREADS), pair_lds, st, s);
        hipLaunchKernelGGL(report_finish_kernel, dim3((unsigned)n), dim3(64), finish_lds, st, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string("report kernels: launch: ") + hipGetErrorString(e)).c_str());
}

extern "C" int rbp_dev_report(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T, const double* time_scale,
                              const double* coef, const double* radius, double downwash, double dt, rbp_report* out) {
    auto bad = [&](const std::string& what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, ("rbp_dev_report: " + what).c_str()); };
    if (!M || !T || !coef || !radius || !out) return bad("M, T, coef, radius and out must be given");
    if (K <= 0 || N <= 0 || M_stride <= 0 || !(dt > 0) || !(downwash > 0)) return bad("K, N, M_stride, dt and downwash must be positive");
    for (int k = 0; k < K; ++k) {
        if (M[k] <= 0 || M[k] > M_stride) return bad("mission " + std::to_string(k) + ": M outside 1..M_stride");
        if (time_scale && !(time_scale[k] > 0)) return bad("mission " + std::to_string(k) + ": the time scale must be positive");
    }
    if (report_tile(N) <= 0 || K > 65535 * 16)
        return bad(std::to_string(N) + " agents: the positions of one sample (24 bytes per agent) must fit " + std::to_string(REPORT_POS_BYTES) + " bytes of LDS");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rbp_set_error(RBP_ERR_NO_DEVICE, "no HIP device: the report kernels have no CPU fallback (rbp_report_host is the host's)");
    if (device < 0) (void)hipGetDevice(&device);
    if (device < 0 || device >= ndev) return rbp_set_error(RBP_ERR_NO_DEVICE, "device index out of range");
    DeviceScope scope(device);
    auto fail = [&](hipError_t err) { return rbp_set_error(RBP_ERR_HIP, (std::string("rbp_dev_report: ") + hipGetErrorString(err)).c_str()); };
    DeviceBuffers b;
    auto up = [&](const auto* src, size_t n) {
        using E = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
        E* p = b.get<E>(n);
        if (p) b.err = hipMemcpy(p, src, sizeof(E) * n, hipMemcpyHostToDevice);
        return p;
    };
    ReportInputs in{};
    in.K = K, in.N = N, in.M_stride = M_stride, in.downwash = downwash, in.dt = dt;
    in.Mk = up(M, (size_t)K);
    in.T = up(T, (size_t)K * (M_stride + 1));
    in.coef = up(coef, (size_t)K * N * 3 * 6 * M_stride);
    in.radius = up(radius, (size_t)K * N);
    in.ts = time_scale ? up(time_scale, (size_t)K) : nullptr, in.ts_stride = 1;
    in.status = nullptr;
    char* ws = b.get<char>(report_workspace_bytes(K));
    if (b.err != hipSuccess) return fail(b.err);
    if (int rc = launch_report(in, ws, 0)) return rc;
    const hipError_t err = hipMemcpy(out, ws, sizeof(rbp_report) * (size_t)K, hipMemcpyDeviceToHost);  // (synchronises with the kernels)
    return err == hipSuccess ? RBP_OK : fail(err);
}
