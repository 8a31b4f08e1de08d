// swept.hip — a certified interval for the smallest clearance of resident plans to the obstacles in continuous time, where the
// coefficients and the distance grids are: in HBM (gfx950).
//
// For K missions, from a session's own arrays and worlds (rbp_session_swept_clearance, abi/session.hip) or a caller's
// (rbp_dev_swept_clearance).  An item is an agent a and a segment m; a mission's items are numbered e = a * M_stride + m, the segment
// fastest, so that the 64 items of a wavefront read the coefficient rows of few agents and consecutive lanes look at neighbouring parts of
// the grid.  Four launches per chunk of missions, the mission in gridDim.y:
//   swept_init_kernel    clears the mission's work-list counter.
//   swept_coarse_kernel  one lane per item, one wavefront per 64 consecutive items.  A lane forms the item's control points and sizes
//                        (swept_rules::item_of), the box of its depth-0 piece, and scans the box serially, z fastest (about ten cells on
//                        planned trajectories, at most RBP_SWEPT_MAX_CELLS).  An item that stays at depth 0 is folded into the lane's tally and
//                        its lower clearance stored in the mission's [N][M_stride] array; the others are appended to the mission's work
//                        list, one uint32 each: ballot, popcount, ONE integer atomic add per wavefront, the lane's place from the ballot's
//                        lower bits.  The list's order depends on the schedule; nothing that is reported does.
//   swept_refine_kernel  L = min(2^depth, 64) neighbouring lanes per listed item, lane l taking pieces l, l + L, ...: the pieces of an item
//                        sit in neighbouring lanes and their boxes in neighbouring cache lines.  A piece is D halvings from the segment's
//                        control points (swept_rules::piece_readings).  The item's state (lower clearance, flags) is reduced over its L
//                        lanes by a segmented shuffle butterfly and its first lane counts the item and stores its lower clearance.  A
//                        mission has a fixed number of wavefronts (SWEPT_REFINE_FACTOR per wavefront of the coarse kernel) that stride over
//                        the list, so the partial tallies are sized by the shapes alone; wavefronts beyond the list's length leave at once.
//   swept_finish_kernel  one wavefront per mission merges the partials of both kernels (swept_rules::merge), reduces the items' lower
//                        clearances to the agents' (where the caller wants them) and writes the rbp_swept_clearance.  A mission with a
//                        status is written here and skipped by the others.
// Lower clearances can be negative, so they are not kept by an atomic minimum on their bit patterns: every item has one writer.  No
// floating-point atomics, no LDS, no barrier; the grid is read through pointers in the global address space.
// Every number is a rule of common/swept_rules.h -- the text rbp_swept_clearance_host (host/validate.cpp) loops over -- and the headers'
// `#pragma clang fp contract(off)` holds for this whole file.  Plain C++, vector stores only.
#include "rbp_dev.h"

#include <string>
#include <type_traits>

#include "common/swept_rules.h"

namespace {

constexpr int SWEPT_THREADS = 256;
constexpr int SWEPT_WAVES = SWEPT_THREADS / 64;  // wavefronts of a workgroup
constexpr unsigned SWEPT_REFINE_FACTOR = 4;      // the refine kernel's wavefronts of a mission per wavefront of the coarse kernel
// the most items of one mission: an item's number is a uint32, and so is the number the last wavefront's last lane forms beyond them
constexpr unsigned long long SWEPT_MAX_ITEMS = (1ull << 32) - 64;

using swept_rules::ItemState;
using swept_rules::Minimum;
using swept_rules::Tally;
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) unsigned guint;
typedef __attribute__((address_space(1))) const float gcfloat;
typedef __attribute__((address_space(1))) rbp_swept_clearance gswept;
typedef __attribute__((address_space(1))) Tally gTally;

static_assert(sizeof(Tally) == 104, "two minima of two doubles and four words, five counters");
static_assert(sizeof(rbp_swept_clearance) == 120, "five doubles, five counters, ten words");

struct SweptArgs {
    SweptInputs in;
    unsigned stride;           // items of a mission's slot: N * M_stride
    unsigned waves;            // the coarse kernel's wavefronts of a mission: ceil(stride / 64)
    unsigned rwaves;           // the refine kernel's: SWEPT_REFINE_FACTOR * waves
    unsigned* count;           // [n] work-list lengths
    unsigned* list;            // [n][stride]
    double* item_lower;        // [n][stride]: every item's lower clearance, written by the kernel that settles the item
    Tally* partial;            // [n][waves + rwaves]: the coarse kernel's, then the refine kernel's
    double* agent_lower;       // [n][N] on the device, or null
    rbp_swept_clearance* out;  // [n]
};

struct MissionView {
    int M;
    double ts;
    const double *T, *coef, *radius;
    bool computed;  // false: a mission with a status
};

__device__ __forceinline__ MissionView mission_view(const ReportInputs& in, int k) {
    MissionView v;
    v.M = in.Mk[k];
    const double q = in.ts ? in.ts[(size_t)k * in.ts_stride] : 1.0;
    v.ts = q > 0 ? q : 1.0;  // (rbp_session_download: a scalar that was never written is no scale)
    v.T = in.T + (size_t)k * (in.M_stride + 1);
    v.coef = in.coef + (size_t)k * in.N * 3 * 6 * in.M_stride;
    v.radius = in.radius + (size_t)k * in.N;
    v.computed = !(in.status && in.status[k] != 0);
    return v;
}

__device__ __forceinline__ Minimum shuffled(const Minimum& m, int off) {
    return Minimum{__shfl_xor(m.clearance, off), __shfl_xor(m.dist, off), __shfl_xor(m.segment, off), __shfl_xor(m.piece, off), __shfl_xor(m.agent, off), __shfl_xor(m.depth, off)};
}
// the wavefront's tally under the rule's order, in every lane
__device__ __forceinline__ Tally wave_tally(Tally t) {
    for (int off = 32; off > 0; off >>= 1) {
        Tally o;
        o.lower = shuffled(t.lower, off), o.upper = shuffled(t.upper, off);
        o.uncertified = __shfl_xor(t.uncertified, off), o.hitting = __shfl_xor(t.hitting, off), o.outside = __shfl_xor(t.outside, off);
        o.over_budget = __shfl_xor(t.over_budget, off), o.refined = __shfl_xor(t.refined, off);
        swept_rules::merge(&t, o);
    }
    return t;
}
__device__ __forceinline__ void store_minimum(gTally* p, bool upper, const Minimum& m) {
    if (upper)
        p->upper.clearance = m.clearance, p->upper.dist = m.dist, p->upper.segment = m.segment, p->upper.piece = m.piece, p->upper.agent = m.agent, p->upper.depth = m.depth;
    else
        p->lower.clearance = m.clearance, p->lower.dist = m.dist, p->lower.segment = m.segment, p->lower.piece = m.piece, p->lower.agent = m.agent, p->lower.depth = m.depth;
}
__device__ __forceinline__ void store_tally(gTally* p, const Tally& t) {
    store_minimum(p, false, t.lower), store_minimum(p, true, t.upper);
    p->uncertified = t.uncertified, p->hitting = t.hitting, p->outside = t.outside, p->over_budget = t.over_budget, p->refined = t.refined;
}
__device__ __forceinline__ Tally load_tally(const gTally* p) {
    Tally t;
    t.lower = Minimum{p->lower.clearance, p->lower.dist, p->lower.segment, p->lower.piece, p->lower.agent, p->lower.depth};
    t.upper = Minimum{p->upper.clearance, p->upper.dist, p->upper.segment, p->upper.piece, p->upper.agent, p->upper.depth};
    t.uncertified = p->uncertified, t.hitting = p->hitting, t.outside = p->outside, t.over_budget = p->over_budget, t.refined = p->refined;
    return t;
}

__global__ __launch_bounds__(64) void swept_init_kernel(SweptArgs g) {
    const int k = (int)(blockIdx.x * 64u + threadIdx.x);
    if (k < g.in.r.K) ((guint*)g.count)[k] = 0u;
}

__global__ __launch_bounds__(SWEPT_THREADS) void swept_coarse_kernel(SweptArgs g) {
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63;
    const unsigned w = blockIdx.x * SWEPT_WAVES + (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    if (w >= g.waves) return;  // (no barrier in this kernel: a wavefront may leave on its own)
    const MissionView v = mission_view(g.in.r, k);
    if (!v.computed) return;  // (swept_finish_kernel writes the mission)
    const DevWorld world = g.in.worlds[k];
    gcfloat* dist = (gcfloat*)world.dist;
    const double rf = clearance_rules::resolution_factor(world.res);
    const unsigned e = w * 64u + (unsigned)lane;
    const int a = (int)(e / (unsigned)g.in.r.M_stride), m = (int)(e % (unsigned)g.in.r.M_stride);
    const bool active = e < g.stride && m < v.M;
    Tally t = swept_rules::empty_tally();
    bool refine = false;
    if (active) {
        const double radius = v.radius[a];
        const swept_rules::Item it = swept_rules::item_of(v.coef, v.M, v.T, v.ts, a, m);
        // (a box that is scanned lies inside the grid by the rule's test on the doubles and holds at most RBP_SWEPT_MAX_CELLS cells)
        const swept_rules::Readings r0 = swept_rules::piece_readings(it, 0, 0, world.dim, world.key_min, rf, dist);
        refine = swept_rules::is_refined(r0, radius, g.in.refine_below);
        if (!refine) {  // (it stays at depth 0, whose readings are at hand)
            ItemState s = swept_rules::empty_item();
            swept_rules::take_piece(&t, &s, r0, radius, 0, 0, m, a);
            swept_rules::count_item(&t, s, false);
            ((gdouble*)g.item_lower)[(size_t)k * g.stride + e] = s.lower;
        }
    }
    const unsigned long long listed = __ballot(refine);
    if (listed) {  // (wave-uniform)
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(g.count + k, (unsigned)__popcll(listed));
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        // every item is appended at most once, so base + place < stride
        if (refine) ((guint*)g.list)[(size_t)k * g.stride + base + (unsigned)__popcll(listed & ((1ull << lane) - 1ull))] = e;
    }
    t = wave_tally(t);
    if (lane == 0) store_tally((gTally*)g.partial + ((size_t)k * (g.waves + g.rwaves) + w), t);
}

__global__ __launch_bounds__(SWEPT_THREADS) void swept_refine_kernel(SweptArgs g) {
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, depth = g.in.depth;
    const unsigned w = blockIdx.x * SWEPT_WAVES + (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    if (w >= g.rwaves) return;
    const unsigned count = ((const guint*)g.count)[k];  // (<= stride; 0 for a mission that is not computed)
    const int pieces = 1 << depth;
    const int L = pieces < 64 ? pieces : 64;             // lanes of an item
    const unsigned per_wave = 64u / (unsigned)L;         // items of a wavefront's round
    const unsigned rounds = (count + per_wave - 1u) / per_wave;
    if (w >= rounds) return;  // (swept_finish_kernel reads min(rounds, rwaves) partials)
    const MissionView v = mission_view(g.in.r, k);
    const DevWorld world = g.in.worlds[k];
    gcfloat* dist = (gcfloat*)world.dist;
    const double rf = clearance_rules::resolution_factor(world.res);
    const int l = lane & (L - 1);
    Tally t = swept_rules::empty_tally();
    for (unsigned round = w; round < rounds; round += g.rwaves) {  // (wave-uniform)
        const unsigned at = round * per_wave + (unsigned)(lane / L);
        ItemState s = swept_rules::empty_item();
        unsigned e = 0;
        int a = 0, m = 0;
        if (at < count) {
            e = ((const guint*)g.list)[(size_t)k * g.stride + at];  // (an item of the coarse kernel: e < stride, m < M)
            a = (int)(e / (unsigned)g.in.r.M_stride), m = (int)(e % (unsigned)g.in.r.M_stride);
            const double radius = v.radius[a];
            const swept_rules::Item it = swept_rules::item_of(v.coef, v.M, v.T, v.ts, a, m);
            for (int p = l; p < pieces; p += L)
                swept_rules::take_piece(&t, &s, swept_rules::piece_readings(it, depth, p, world.dim, world.key_min, rf, dist), radius, depth, p, m, a);
        }
        for (int off = L >> 1; off > 0; off >>= 1) {  // (over the item's own lanes: an aligned group of L)
            ItemState o;
            o.lower = __shfl_xor(s.lower, off), o.flags = __shfl_xor(s.flags, off);
            swept_rules::merge_item(&s, o);
        }
        if (at < count && l == 0) {
            swept_rules::count_item(&t, s, true);
            ((gdouble*)g.item_lower)[(size_t)k * g.stride + e] = s.lower;
        }
    }
    t = wave_tally(t);
    if (lane == 0) store_tally((gTally*)g.partial + ((size_t)k * (g.waves + g.rwaves) + g.waves + w), t);
}

__global__ __launch_bounds__(64) void swept_finish_kernel(SweptArgs g) {
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x, N = g.in.r.N;
    const MissionView v = mission_view(g.in.r, k);
    const int status = g.in.r.status ? g.in.r.status[k] : 0;
    Tally t = swept_rules::empty_tally();
    if (v.computed) {
        const gTally* part = (const gTally*)g.partial + (size_t)k * (g.waves + g.rwaves);
        const unsigned count = ((const guint*)g.count)[k];
        const int pieces = 1 << g.in.depth;
        const unsigned per_wave = 64u / (unsigned)(pieces < 64 ? pieces : 64);
        const unsigned rounds = (count + per_wave - 1u) / per_wave;
        const unsigned refine_partials = rounds < g.rwaves ? rounds : g.rwaves;  // (the refine kernel's wavefronts that stored a partial)
        for (unsigned i = (unsigned)lane; i < g.waves; i += 64u) swept_rules::merge(&t, load_tally(part + i));
        for (unsigned i = (unsigned)lane; i < refine_partials; i += 64u) swept_rules::merge(&t, load_tally(part + g.waves + i));
        t = wave_tally(t);
        if (g.agent_lower) {
            const gdouble* items = (const gdouble*)g.item_lower + (size_t)k * g.stride;
            for (int a = lane; a < N; a += 64) {
                double al = RBP_CLEARANCE_NONE;
                for (int m = 0; m < v.M; ++m) {
                    const double lo = items[(size_t)a * g.in.r.M_stride + m];
                    if (lo < al) al = lo;
                }
                ((gdouble*)g.agent_lower)[(size_t)k * N + a] = al;
            }
        }
    }
    if (lane != 0) return;
    gswept* r = (gswept*)g.out + k;
    if (status != 0) {  // nothing is computed of a mission that has failed
        r->lower_clearance = 0.0, r->upper_clearance = 0.0, r->lower_dist = 0.0, r->upper_dist = 0.0, r->end_time = 0.0;
        r->uncertified = 0, r->hitting = 0, r->outside = 0, r->over_budget = 0, r->refined = 0;
        r->lower_segment = -1, r->lower_piece = -1, r->lower_agent = -1, r->lower_depth = -1;
        r->upper_segment = -1, r->upper_piece = -1, r->upper_agent = -1, r->upper_depth = -1;
        r->status = status, r->reserved = 0;
        return;
    }
    r->lower_clearance = t.lower.clearance, r->upper_clearance = t.upper.clearance, r->lower_dist = t.lower.dist, r->upper_dist = t.upper.dist;
    r->end_time = report_rules::scaled_time(v.T[v.M], v.ts);
    r->uncertified = t.uncertified, r->hitting = t.hitting, r->outside = t.outside, r->over_budget = t.over_budget, r->refined = t.refined;
    r->lower_segment = t.lower.segment, r->lower_piece = t.lower.piece, r->lower_agent = t.lower.agent, r->lower_depth = t.lower.depth;
    r->upper_segment = t.upper.segment, r->upper_piece = t.upper.piece, r->upper_agent = t.upper.agent, r->upper_depth = t.upper.depth;
    r->status = 0, r->reserved = 0;
}

size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

// how a call's missions are cut: a mission's items, its wavefronts, and the missions of a chunk under the work list's budget
struct Shape {
    unsigned long long stride;
    unsigned waves, rwaves;
    int chunk;
};
Shape shape_of(int K, int N, int M_stride) {
    Shape s;
    s.stride = (unsigned long long)N * (unsigned long long)M_stride;
    s.waves = (unsigned)((s.stride + 63) / 64);
    s.rwaves = SWEPT_REFINE_FACTOR * s.waves;
    const unsigned long long budget = RBP_SWEPT_LIST_BYTES / sizeof(unsigned);
    unsigned long long c = s.stride ? budget / s.stride : (unsigned long long)K;
    c = c < 1 ? 1 : c;
    c = c > 65535 ? 65535 : c;  // (gridDim.y)
    s.chunk = (int)(c > (unsigned long long)K ? (unsigned long long)K : c);
    return s;
}

// missions k0 .. k0 + n of `g` as a launch of their own (the kernels index by mission through the pointers; the list, the counters, the
// items' clearances and the partials are the chunk's and are used again by the next one, which the stream orders)
SweptArgs slice(const SweptArgs& g, int k0, int n) {
    SweptArgs s = g;
    ReportInputs& r = s.in.r;
    const size_t N = (size_t)r.N;
    r.K = n, r.Mk += k0, r.T += (size_t)k0 * (r.M_stride + 1), r.coef += (size_t)k0 * N * 3 * 6 * r.M_stride, r.radius += (size_t)k0 * N;
    if (r.ts) r.ts += (size_t)k0 * r.ts_stride;
    if (r.status) r.status += k0;
    s.in.worlds += k0, s.out += k0;
    if (s.agent_lower) s.agent_lower += (size_t)k0 * N;
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

int swept_check_arguments(const char* who, int32_t depth, double refine_below) {
    if (depth < 0 || depth > RBP_SWEPT_MAX_DEPTH)
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": depth must lie in 0 .. " + std::to_string(RBP_SWEPT_MAX_DEPTH)).c_str());
    if (refine_below != refine_below) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": refine_below must be a number").c_str());
    return RBP_OK;
}

size_t swept_workspace_bytes(int K, int N, int M_stride) {
    const Shape s = shape_of(K, N, M_stride);
    return al256(sizeof(rbp_swept_clearance) * (size_t)K) + al256(sizeof(unsigned) * (size_t)s.chunk) +
           al256(sizeof(unsigned) * (size_t)s.chunk * (size_t)s.stride) + al256(sizeof(double) * (size_t)s.chunk * (size_t)s.stride) +
           sizeof(Tally) * (size_t)s.chunk * ((size_t)s.waves + s.rwaves);
}

int launch_swept(const SweptInputs& in, double* agent_lower, void* workspace, hipStream_t st) {
    const int K = in.r.K, N = in.r.N;
    if (K <= 0 || N <= 0 || in.r.M_stride <= 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "swept clearance: no mission, no agent or no segment");
    if (int rc = swept_check_arguments("swept clearance", in.depth, in.refine_below)) return rc;
    const Shape sh = shape_of(K, N, in.r.M_stride);
    if (sh.stride > SWEPT_MAX_ITEMS) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "swept clearance: a mission of more than 2^32 - 64 (agent, segment) items");
    SweptArgs g{};
    g.in = in, g.stride = (unsigned)sh.stride, g.waves = sh.waves, g.rwaves = sh.rwaves;
    g.agent_lower = agent_lower;
    char* p = static_cast<char*>(workspace);
    g.out = reinterpret_cast<rbp_swept_clearance*>(p), p += al256(sizeof(rbp_swept_clearance) * (size_t)K);
    g.count = reinterpret_cast<unsigned*>(p), p += al256(sizeof(unsigned) * (size_t)sh.chunk);
    g.list = reinterpret_cast<unsigned*>(p), p += al256(sizeof(unsigned) * (size_t)sh.chunk * (size_t)sh.stride);
    g.item_lower = reinterpret_cast<double*>(p), p += al256(sizeof(double) * (size_t)sh.chunk * (size_t)sh.stride);
    g.partial = reinterpret_cast<Tally*>(p);
    const unsigned blocks = (sh.waves + SWEPT_WAVES - 1) / SWEPT_WAVES, rblocks = (sh.rwaves + SWEPT_WAVES - 1) / SWEPT_WAVES;
    for (int k0 = 0; k0 < K; k0 += sh.chunk) {
        const int n = std::min(sh.chunk, K - k0);
        const SweptArgs s = slice(g, k0, n);
        hipLaunchKernelGGL(swept_init_kernel, dim3((unsigned)(n + 63) / 64u), dim3(64), 0, st, s);
        hipLaunchKernelGGL(swept_coarse_kernel, dim3(blocks, (unsigned)n), dim3(SWEPT_THREADS), 0, st, s);
        hipLaunchKernelGGL(swept_refine_kernel, dim3(rblocks, (unsigned)n), dim3(SWEPT_THREADS), 0, st, s);
        hipLaunchKernelGGL(swept_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string("swept clearance kernels: launch: ") + hipGetErrorString(e)).c_str());
}

// The kernels on device inputs, the K records copied to `out` on the host in one copy, the agents' lower clearances to wherever the caller
// wants them (the current device is `device`): a destination on the device is written in place by the finish kernel; a host destination
// goes through one staging buffer and one copy, of which only the rows of the missions that were computed reach the caller's array.
int swept_run(const char* who, int device, const SweptInputs& in, rbp_swept_clearance* out, double* agent_lower, void* workspace, hipStream_t st) {
    auto fail = [&](hipError_t err) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(err)).c_str()); };
    const int ad = agent_lower ? on_device(agent_lower, device) : 1;
    if (ad < 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": agent_lower lies on another device than the plans (device " + std::to_string(device) + ")").c_str());
    const size_t K = (size_t)in.r.K, N = (size_t)in.r.N;
    DeviceBuffers b;
    double* stage = ad ? nullptr : b.get<double>(K * N);
    if (b.err != hipSuccess) return fail(b.err);
    if (int rc = launch_swept(in, ad ? agent_lower : stage, workspace, st)) return rc;
    hipError_t e = hipMemcpyAsync(out, workspace, sizeof(rbp_swept_clearance) * K, hipMemcpyDeviceToHost, st);
    std::vector<double> rows;
    if (!ad && e == hipSuccess) {
        rows.resize(K * N);
        e = hipMemcpyAsync(rows.data(), stage, sizeof(double) * K * N, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    if (!ad)
        for (size_t k = 0; k < K; ++k)
            if (out[k].status == 0) std::copy(rows.begin() + k * N, rows.begin() + (k + 1) * N, agent_lower + k * N);
    return RBP_OK;
}

extern "C" int rbp_dev_swept_clearance(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T, const double* time_scale,
                                       const double* coef, const double* radius, const rbp_world* worlds, int32_t depth, double refine_below,
                                       rbp_swept_clearance* out, double* agent_lower) {
    auto bad = [&](const std::string& what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, ("rbp_dev_swept_clearance: " + what).c_str()); };
    if (!M || !T || !coef || !radius || !worlds || !out) return bad("M, T, coef, radius, worlds and out must be given");
    if (K <= 0 || N <= 0 || M_stride <= 0) return bad("K, N and M_stride must be positive");
    if (int rc = swept_check_arguments("rbp_dev_swept_clearance", depth, refine_below)) return rc;
    for (int k = 0; k < K; ++k) {
        if (M[k] <= 0 || M[k] > M_stride) return bad("mission " + std::to_string(k) + ": M outside 1..M_stride");
        if (time_scale && !(time_scale[k] > 0)) return bad("mission " + std::to_string(k) + ": the time scale must be positive");
        if (!worlds[k].dist || !(worlds[k].res > 0) || worlds[k].dim[0] <= 0 || worlds[k].dim[1] <= 0 || worlds[k].dim[2] <= 0)
            return bad("mission " + std::to_string(k) + ": the world needs a grid, a positive res and positive dim");
    }
    if ((unsigned long long)N * (unsigned long long)M_stride > SWEPT_MAX_ITEMS) return bad("a mission of more than 2^32 - 64 (agent, segment) items");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rbp_set_error(RBP_ERR_NO_DEVICE, "no HIP device: the swept clearance kernels have no CPU fallback (rbp_swept_clearance_host is the host's)");
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
    SweptInputs in{};
    ReportInputs& r = in.r;
    r.K = K, r.N = N, r.M_stride = M_stride, r.downwash = 1.0, r.dt = 0.0;
    r.Mk = up(M, (size_t)K);
    r.T = up(T, (size_t)K * (M_stride + 1));
    r.coef = up(coef, (size_t)K * N * 3 * 6 * M_stride);
    r.radius = up(radius, (size_t)K * N);
    r.ts = time_scale ? up(time_scale, (size_t)K) : nullptr, r.ts_stride = 1;
    r.status = nullptr;
    in.worlds = b.upload(wh);
    in.depth = depth, in.refine_below = refine_below;
    char* ws = b.get<char>(swept_workspace_bytes(K, N, M_stride));
    if (b.err != hipSuccess) return rbp_set_error(RBP_ERR_HIP, (std::string("rbp_dev_swept_clearance: ") + hipGetErrorString(b.err)).c_str());
    return swept_run("rbp_dev_swept_clearance", device, in, out, agent_lower, ws, 0);
}
