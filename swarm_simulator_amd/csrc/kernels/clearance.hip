// clearance.hip — how close resident plans come to the obstacles, where the coefficients and the distance grids are: in HBM (gfx950).
//
// The grid's value under every agent at every sample t = j * dt less the agent's radius, for K missions in two launches, from a session's
// own arrays and worlds (rbp_session_clearance, abi/session.hip) or a caller's (rbp_dev_clearance):
//   clearance_agent_kernel   one wavefront per (mission, agent), four agents per workgroup, the mission in gridDim.y.  The wavefront strides
//                            over its agent's samples in chunks of 64, a lane per sample; a lane's samples ascend, so its segment count runs
//                            along them (segments_before with `from`).  A lane evaluates the three Horner positions, forms the cell by the
//                            rule and issues ONE float load from the grid: consecutive samples of one agent are neighbours in space, so the
//                            64 loads of a chunk fall into a few cache lines of a grid that fits the L2.  Each lane keeps its minimum under
//                            the rule's order; hits and outsides are counted per chunk from the ballot into wave-uniform counters.  After the
//                            loop the minimum is reduced across the wavefront by a shuffle butterfly and lane 0 stores one record per agent
//                            (and the agent's clearance where the caller's destination is on the device).  No LDS, no barrier, no atomics.
//   clearance_finish_kernel  one wavefront per mission: lanes take agents lane, lane + 64, ..., merge under the rule's order (sample first,
//                            then agent) and sum the counters; after a wave reduction lane 0 writes the rbp_clearance.  A mission with a
//                            status, or with more samples than are evaluated, is written here and skipped by the first kernel.
// Every number is a rule of common/clearance_rules.h -- the text rbp_clearance_host (host/validate.cpp) loops over -- and the headers'
// `#pragma clang fp contract(off)` holds for this whole file.  The minimum is kept under an order (clearance_rules::take), so nothing
// depends on which lane or agent met a candidate first.  Plain C++, vector stores only.
#include "rbp_dev.h"

#include <string>
#include <type_traits>

#include "common/clearance_rules.h"

namespace {

constexpr int CLR_THREADS = 256;
constexpr int CLR_AGENTS = CLR_THREADS / 64;  // agents of a workgroup: one per wavefront
constexpr int CLR_CHUNK = 64;                 // samples of a chunk: one per lane

using clearance_rules::Minimum;
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) const float gcfloat;

// what the first kernel leaves of one agent
struct AgentRecord {
    double clearance, dist;  // the agent's smallest clearance (1e9: no sample) and the grid's value there
    int32_t sample, pad;     // where (-1: none)
    long long hits, outside;
};
typedef __attribute__((address_space(1))) AgentRecord gAgentRecord;
typedef __attribute__((address_space(1))) rbp_clearance gclearance;

static_assert(sizeof(AgentRecord) == 40, "two doubles, two words, two counters");
static_assert(sizeof(rbp_clearance) == 56, "three doubles, two counters, four words");

struct ClrArgs {
    ClearanceInputs in;
    AgentRecord* agents;      // [K][N]
    double* agent_clearance;  // [K][N] on the device, or null
    rbp_clearance* out;       // [K]
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

// the wavefront's minimum under the rule's order, in every lane
__device__ __forceinline__ Minimum wave_minimum(Minimum m) {
    for (int off = 32; off > 0; off >>= 1)
        clearance_rules::take(&m, Minimum{__shfl_xor(m.clearance, off), __shfl_xor(m.dist, off), __shfl_xor(m.sample, off), __shfl_xor(m.agent, off)});
    return m;
}

__global__ __launch_bounds__(CLR_THREADS) void clearance_agent_kernel(ClrArgs g) {
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, N = g.in.r.N;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (the same in every lane: agent, radius and world are scalars)
    const int a = (int)blockIdx.x * CLR_AGENTS + wave;
    if (a >= N) return;  // (no barrier in this kernel: a wavefront may leave on its own)
    const MissionView v = mission_view(g.in.r, k);
    if (!v.computed) return;  // (clearance_finish_kernel writes the mission)
    const DevWorld w = g.in.worlds[k];
    gcfloat* dist = (gcfloat*)w.dist;
    const double rf = clearance_rules::resolution_factor(w.res), radius = v.radius[a];
    Minimum best = clearance_rules::no_minimum();
    long long hits = 0, outside = 0;  // wave-uniform
    int before = 0;
    for (int base = 0; base < v.samples; base += CLR_CHUNK) {
        const int j = base + lane;
        bool hit = false, out = false;
        if (j < v.samples) {
            const double t = report_rules::sample_time(j, g.in.r.dt);
            before = report_rules::segments_before(v.T, v.M, v.ts, t, before);  // (this lane's samples ascend)
            double p[3];
            report_rules::agent_position(v.coef, v.M, v.T, v.ts, a, t, before, p);
            const long long cell = clearance_rules::cell_of(w.dim, w.key_min, rf, p);  // (inside: 0 <= cell < dim0 * dim1 * dim2, by the rule's test)
            const double d = clearance_rules::distance_of(cell, cell >= 0 ? dist[cell] : 0.0f);
            clearance_rules::take(&best, Minimum{clearance_rules::clearance(d, radius), d, j, a});
            hit = clearance_rules::is_hit(d, radius), out = cell < 0;
        }
        hits += __popcll(__ballot(hit));
        outside += __popcll(__ballot(out));
    }
    best = wave_minimum(best);
    if (lane == 0) {
        gAgentRecord* rec = (gAgentRecord*)g.agents + ((size_t)k * N + a);
        rec->clearance = best.clearance, rec->dist = best.dist, rec->sample = best.sample, rec->pad = 0;
        rec->hits = hits, rec->outside = outside;
        if (g.agent_clearance) ((gdouble*)g.agent_clearance)[(size_t)k * N + a] = best.clearance;
    }
}

__global__ __launch_bounds__(64) void clearance_finish_kernel(ClrArgs g) {
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x, N = g.in.r.N;
    const MissionView v = mission_view(g.in.r, k);
    const int status = g.in.r.status ? g.in.r.status[k] : 0;
    Minimum best = clearance_rules::no_minimum();
    long long hits = 0, outside = 0;
    if (v.computed) {
        const gAgentRecord* rec = (const gAgentRecord*)g.agents + (size_t)k * N;
        for (int a = lane; a < N; a += 64) {  // (an agent without a minimum carries 1e9 and sample -1, which `take` never takes)
            clearance_rules::take(&best, Minimum{rec[a].clearance, rec[a].dist, rec[a].sample, a});
            hits += rec[a].hits, outside += rec[a].outside;
        }
        best = wave_minimum(best);
        for (int off = 32; off > 0; off >>= 1) hits += __shfl_xor(hits, off), outside += __shfl_xor(outside, off);
    }
    if (lane != 0) return;
    gclearance* r = (gclearance*)g.out + k;
    if (status != 0) {  // nothing is computed of a mission that has failed
        r->min_clearance = 0.0, r->min_dist = 0.0, r->end_time = 0.0, r->hits = 0, r->outside = 0;
        r->samples = 0, r->min_sample = -1, r->min_agent = -1, r->status = status;
        return;
    }
    r->min_clearance = best.clearance, r->min_dist = best.dist, r->end_time = v.end_time, r->hits = hits, r->outside = outside;
    r->samples = v.samples, r->min_sample = best.sample, r->min_agent = best.agent, r->status = 0;
}

size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

// missions k0 .. k0 + n of `g` as a launch of their own (the kernels index by mission through the pointers)
ClrArgs slice(const ClrArgs& g, int k0, int n) {
    ClrArgs s = g;
    ReportInputs& r = s.in.r;
    const size_t N = (size_t)r.N;
    r.K = n, r.Mk += k0, r.T += (size_t)k0 * (r.M_stride + 1), r.coef += (size_t)k0 * N * 3 * 6 * r.M_stride, r.radius += (size_t)k0 * N;
    if (r.ts) r.ts += (size_t)k0 * r.ts_stride;
    if (r.status) r.status += k0;
    s.in.worlds += k0, s.agents += (size_t)k0 * N, s.out += k0;
    if (s.agent_clearance) s.agent_clearance += (size_t)k0 * N;
    return s;
}

// where a pointer lies, as rbp_session_create classifies rbp_world.dist: a pointer the runtime does not know is reported as an error or
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

size_t clearance_workspace_bytes(int K, int N) { return al256(sizeof(rbp_clearance) * (size_t)K) + sizeof(AgentRecord) * (size_t)K * N; }

int launch_clearance(const ClearanceInputs& in, double* agent_clearance, void* workspace, hipStream_t st) {
    const int K = in.r.K, N = in.r.N;
    if (K <= 0 || N <= 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "clearance: no mission or no agent");
    ClrArgs g{};
    g.in = in, g.agent_clearance = agent_clearance;
    g.out = static_cast<rbp_clearance*>(workspace);
    g.agents = reinterpret_cast<AgentRecord*>(static_cast<char*>(workspace) + al256(sizeof(rbp_clearance) * (size_t)K));
    // gridDim.y holds at most 65535 missions: more go in slices
    for (int k0 = 0; k0 < K; k0 += 65535) {
        const int n = std::min(65535, K - k0);
        const ClrArgs s = slice(g, k0, n);
        hipLaunchKernelGGL(clearance_agent_kernel, dim3((unsigned)((N + CLR_AGENTS - 1) / CLR_AGENTS), (unsigned)n), dim3(CLR_THREADS), 0, st, s);
        hipLaunchKernelGGL(clearance_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string("clearance kernels: launch: ") + hipGetErrorString(e)).c_str());
}

// The kernels on device inputs, the K records copied to `out` on the host in one copy, the agents' clearances to wherever the caller wants
// them (the current device is `device`): a destination on the device is written in place by the first kernel; a host destination goes
// through one staging buffer and one copy, of which only the rows of the missions that were computed reach the caller's array.
int clearance_run(const char* who, int device, const ClearanceInputs& in, rbp_clearance* out, double* agent_clearance, void* workspace, hipStream_t st) {
    auto fail = [&](hipError_t err) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(err)).c_str()); };
    const int ad = agent_clearance ? on_device(agent_clearance, device) : 1;
    if (ad < 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": agent_clearance lies on another device than the plans (device " + std::to_string(device) + ")").c_str());
    const size_t K = (size_t)in.r.K, N = (size_t)in.r.N;
    DeviceBuffers b;
    double* stage = ad ? nullptr : b.get<double>(K * N);
    if (b.err != hipSuccess) return fail(b.err);
    if (int rc = launch_clearance(in, ad ? agent_clearance : stage, workspace, st)) return rc;
    hipError_t e = hipMemcpyAsync(out, workspace, sizeof(rbp_clearance) * K, hipMemcpyDeviceToHost, st);
    std::vector<double> rows;
    if (!ad && e == hipSuccess) {
        rows.resize(K * N);
        e = hipMemcpyAsync(rows.data(), stage, sizeof(double) * K * N, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    if (!ad)
        for (size_t k = 0; k < K; ++k)
            if (out[k].status == 0 && out[k].samples >= 0) std::copy(rows.begin() + k * N, rows.begin() + (k + 1) * N, agent_clearance + k * N);
    return RBP_OK;
}

extern "C" int rbp_dev_clearance(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T, const double* time_scale,
                                 const double* coef, const double* radius, const rbp_world* worlds, double dt, rbp_clearance* out,
                                 double* agent_clearance) {
    auto bad = [&](const std::string& what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, ("rbp_dev_clearance: " + what).c_str()); };
    if (!M || !T || !coef || !radius || !worlds || !out) return bad("M, T, coef, radius, worlds and out must be given");
    if (K <= 0 || N <= 0 || M_stride <= 0 || !(dt > 0)) return bad("K, N, M_stride and dt must be positive");
    for (int k = 0; k < K; ++k) {
        if (M[k] <= 0 || M[k] > M_stride) return bad("mission " + std::to_string(k) + ": M outside 1..M_stride");
        if (time_scale && !(time_scale[k] > 0)) return bad("mission " + std::to_string(k) + ": the time scale must be positive");
        if (!worlds[k].dist || !(worlds[k].res > 0) || worlds[k].dim[0] <= 0 || worlds[k].dim[1] <= 0 || worlds[k].dim[2] <= 0)
            return bad("mission " + std::to_string(k) + ": the world needs a grid, a positive res and positive dim");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rbp_set_error(RBP_ERR_NO_DEVICE, "no HIP device: the clearance kernels have no CPU fallback (rbp_clearance_host is the host's)");
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
    // the grids: a device grid is referenced in place, a host grid uploaded once per distinct (pointer, shape)
    std::vector<DevWorld> wh((size_t)K);
    auto same_grid = [&](int i, int j) {
        return worlds[i].dist == worlds[j].dist && worlds[i].dim[0] == worlds[j].dim[0] && worlds[i].dim[1] == worlds[j].dim[1] && worlds[i].dim[2] == worlds[j].dim[2];
    };
    for (int k = 0; k < K; ++k) {
        DevWorld& w = wh[(size_t)k];
        for (int a = 0; a < 3; ++a) w.dim[a] = worlds[k].dim[a], w.key_min[a] = worlds[k].key_min[a];
        w.res = worlds[k].res, w.dist = nullptr;
        const int where = on_device(worlds[k].dist, device);
        if (where < 0) return bad("world.dist of mission " + std::to_string(k) + " lies on another device than device " + std::to_string(device));
        if (where > 0) {
            w.dist = worlds[k].dist;  // referenced in place
            continue;
        }
        for (int j = 0; j < k && !w.dist; ++j)
            if (same_grid(j, k)) w.dist = wh[(size_t)j].dist;
        if (!w.dist) w.dist = up(worlds[k].dist, (size_t)w.dim[0] * w.dim[1] * w.dim[2]);
        if (b.err != hipSuccess) break;
    }
    ClearanceInputs in{};
    ReportInputs& r = in.r;
    r.K = K, r.N = N, r.M_stride = M_stride, r.downwash = 1.0, r.dt = dt;
    r.Mk = up(M, (size_t)K);
    r.T = up(T, (size_t)K * (M_stride + 1));
    r.coef = up(coef, (size_t)K * N * 3 * 6 * M_stride);
    r.radius = up(radius, (size_t)K * N);
    r.ts = time_scale ? up(time_scale, (size_t)K) : nullptr, r.ts_stride = 1;
    r.status = nullptr;
    in.worlds = b.upload(wh);
    char* ws = b.get<char>(clearance_workspace_bytes(K, N));
    if (b.err != hipSuccess) return rbp_set_error(RBP_ERR_HIP, (std::string("rbp_dev_clearance: ") + hipGetErrorString(b.err)).c_str());
    return clearance_run("rbp_dev_clearance", device, in, out, agent_clearance, ws, 0);
}
