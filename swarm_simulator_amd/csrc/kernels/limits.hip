// limits.hip — certified intervals for the largest velocity and acceleration of resident plans, as fractions of the agents' limits, in
// continuous time, where the coefficients are: in HBM (gfx950).
//
// For K missions, from a session's own arrays (rbp_session_limits, abi/session.hip) or a caller's (rbp_dev_limits).  An item is an agent a
// and a segment m; a mission's items are numbered e = a * M_stride + m, the segment fastest (the item space of swept.hip), so that the 64
// items of a wavefront read the coefficient rows of few agents.  Four launches per chunk of missions, the mission in gridDim.y:
//   limits_init_kernel    clears the mission's work-list counter.
//   limits_coarse_kernel  one lane per item, one wavefront per 64 consecutive items.  A lane evaluates the item's six polynomials (three
//                         axes, velocity and acceleration) on the whole segment, one after the other (limits_rules::take_pieces at depth
//                         0).  An item that stays at depth 0 is folded into the lane's tally and its two upper ratios stored in the
//                         mission's [N][M_stride][2] array; the others are appended to the mission's work list, one uint32 each: ballot,
//                         popcount, ONE integer atomic add per wavefront, the lane's place from the ballot's lower bits.  The list's order
//                         depends on the schedule; nothing that is reported does.
//   limits_refine_kernel  L = min(2^depth, 64) neighbouring lanes per listed item, lane l taking pieces l, l + L, ... of every polynomial.
//                         The item's state (upper ratios, flags) is reduced over its L lanes by a segmented shuffle butterfly and its first
//                         lane counts the item and stores its upper ratios.  A mission has a fixed number of wavefronts
//                         (LIMITS_REFINE_FACTOR per wavefront of the coarse kernel) that stride over the list, so the partial tallies are
//                         sized by the shapes alone; wavefronts beyond the list's length leave at once.
//   limits_finish_kernel  one wavefront per mission merges the partials of both kernels (limits_rules::merge), reduces the items' upper
//                         ratios to the agents' (where the caller wants them) and writes the rbp_limits.  A mission with a status is
//                         written here and skipped by the others.
// Every item has one writer.  No floating-point atomics, no LDS, no barrier; results go through pointers in the global address space.
// Every number is a rule of common/limits_rules.h -- the text rbp_limits_host (host/limits.cpp) loops over -- and the headers'
// `#pragma clang fp contract(off)` holds for this whole file.  Plain C++, vector stores only.
#include "rbp_dev.h"

#include <string>
#include <type_traits>

#include "common/limits_rules.h"

namespace {

constexpr int LIMITS_THREADS = 256;
constexpr int LIMITS_WAVES = LIMITS_THREADS / 64;  // wavefronts of a workgroup
constexpr unsigned LIMITS_REFINE_FACTOR = 4;       // the refine kernel's wavefronts of a mission per wavefront of the coarse kernel
// the most items of one mission: an item's number is a uint32, and so is the number the last wavefront's last lane forms beyond them
constexpr unsigned long long LIMITS_MAX_ITEMS = (1ull << 32) - 64;

using limits_rules::ItemState;
using limits_rules::Peak;
using limits_rules::Tally;
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) unsigned guint;
typedef __attribute__((address_space(1))) rbp_limits glimits;
typedef __attribute__((address_space(1))) Tally gTally;
typedef __attribute__((address_space(1))) Peak gPeak;

static_assert(sizeof(Peak) == 32, "a double and six words");
static_assert(sizeof(Tally) == 152, "four peaks, three counters");
static_assert(sizeof(rbp_limits) == 152, "five doubles, three counters, twenty-two words");

struct LimitsArgs {
    LimitsInputs in;
    unsigned stride;      // items of a mission's slot: N * M_stride
    unsigned waves;       // the coarse kernel's wavefronts of a mission: ceil(stride / 64)
    unsigned rwaves;      // the refine kernel's: LIMITS_REFINE_FACTOR * waves
    unsigned* count;      // [n] work-list lengths
    unsigned* list;       // [n][stride]
    double* item_upper;   // [n][stride][2]: every item's upper velocity and acceleration ratio, written by the kernel that settles the item
    Tally* partial;       // [n][waves + rwaves]: the coarse kernel's, then the refine kernel's
    double* agent_upper;  // [n][N][2] on the device, or null
    rbp_limits* out;      // [n]
};

struct MissionView {
    int M;
    double ts;
    const double *T, *coef, *max_vel, *max_acc;
    bool computed;  // false: a mission with a status
};

__device__ __forceinline__ MissionView mission_view(const LimitsInputs& li, int k) {
    const ReportInputs& in = li.r;
    MissionView v;
    v.M = in.Mk[k];
    const double q = in.ts ? in.ts[(size_t)k * in.ts_stride] : 1.0;
    v.ts = q > 0 ? q : 1.0;  // (rbp_session_download: a scalar that was never written is no scale)
    v.T = in.T + (size_t)k * (in.M_stride + 1);
    v.coef = in.coef + (size_t)k * in.N * 3 * 6 * in.M_stride;
    v.max_vel = li.max_vel + (size_t)k * in.N * 3;
    v.max_acc = li.max_acc + (size_t)k * in.N * 3;
    v.computed = !(in.status && in.status[k] != 0);
    return v;
}

__device__ __forceinline__ Peak shuffled(const Peak& m, int off) {
    return Peak{__shfl_xor(m.ratio, off), __shfl_xor(m.segment, off), __shfl_xor(m.piece, off), __shfl_xor(m.agent, off), __shfl_xor(m.axis, off), __shfl_xor(m.depth, off), 0};
}
// the wavefront's tally under the rule's order, in every lane
__device__ __forceinline__ Tally wave_tally(Tally t) {
    for (int off = 32; off > 0; off >>= 1) {
        Tally o;
        o.lower_vel = shuffled(t.lower_vel, off), o.upper_vel = shuffled(t.upper_vel, off);
        o.lower_acc = shuffled(t.lower_acc, off), o.upper_acc = shuffled(t.upper_acc, off);
        o.uncertified = __shfl_xor(t.uncertified, off), o.violating = __shfl_xor(t.violating, off), o.refined = __shfl_xor(t.refined, off);
        limits_rules::merge(&t, o);
    }
    return t;
}
__device__ __forceinline__ void store_peak(gPeak* p, const Peak& m) {
    p->ratio = m.ratio, p->segment = m.segment, p->piece = m.piece, p->agent = m.agent, p->axis = m.axis, p->depth = m.depth, p->pad = 0;
}
__device__ __forceinline__ Peak load_peak(const gPeak* p) { return Peak{p->ratio, p->segment, p->piece, p->agent, p->axis, p->depth, 0}; }
__device__ __forceinline__ void store_tally(gTally* p, const Tally& t) {
    store_peak(&p->lower_vel, t.lower_vel), store_peak(&p->upper_vel, t.upper_vel);
    store_peak(&p->lower_acc, t.lower_acc), store_peak(&p->upper_acc, t.upper_acc);
    p->uncertified = t.uncertified, p->violating = t.violating, p->refined = t.refined;
}
__device__ __forceinline__ Tally load_tally(const gTally* p) {
    Tally t;
    t.lower_vel = load_peak(&p->lower_vel), t.upper_vel = load_peak(&p->upper_vel);
    t.lower_acc = load_peak(&p->lower_acc), t.upper_acc = load_peak(&p->upper_acc);
    t.uncertified = p->uncertified, t.violating = p->violating, t.refined = p->refined;
    return t;
}

__global__ __launch_bounds__(64) void limits_init_kernel(LimitsArgs g) {
    const int k = (int)(blockIdx.x * 64u + threadIdx.x);
    if (k < g.in.r.K) ((guint*)g.count)[k] = 0u;
}

__global__ __launch_bounds__(LIMITS_THREADS) void limits_coarse_kernel(LimitsArgs g) {
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63;
    const unsigned w = blockIdx.x * LIMITS_WAVES + (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    if (w >= g.waves) return;  // (no barrier in this kernel: a wavefront may leave on its own)
    const MissionView v = mission_view(g.in, k);
    if (!v.computed) return;  // (limits_finish_kernel writes the mission)
    const unsigned e = w * 64u + (unsigned)lane;
    const int a = (int)(e / (unsigned)g.in.r.M_stride), m = (int)(e % (unsigned)g.in.r.M_stride);
    const bool active = e < g.stride && m < v.M;  // (e < stride: a < N)
    Tally t = limits_rules::empty_tally();
    bool refine = false;
    if (active) {
        ItemState s = limits_rules::empty_item();
        limits_rules::take_pieces(&t, &s, v.coef, v.M, v.T, v.ts, a, m, v.max_vel + 3 * (size_t)a, v.max_acc + 3 * (size_t)a, 0, 0, 1, 1);
        refine = limits_rules::is_refined(s, g.in.refine_above);
        if (!refine) {  // (it stays at depth 0, whose bounds are at hand)
            limits_rules::count_item(&t, s, false);
            gdouble* up = (gdouble*)g.item_upper + ((size_t)k * g.stride + e) * 2;
            up[0] = s.upper_vel, up[1] = s.upper_acc;
        }
    }
    if (refine) t = limits_rules::empty_tally();  // (the depth-0 bounds of a refined item are dropped)
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

__global__ __launch_bounds__(LIMITS_THREADS) void limits_refine_kernel(LimitsArgs g) {
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, depth = g.in.depth;
    const unsigned w = blockIdx.x * LIMITS_WAVES + (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    if (w >= g.rwaves) return;
    const unsigned count = ((const guint*)g.count)[k];  // (<= stride; 0 for a mission that is not computed)
    const int pieces = 1 << depth;
    const int L = pieces < 64 ? pieces : 64;             // lanes of an item
    const unsigned per_wave = 64u / (unsigned)L;         // items of a wavefront's round
    const unsigned rounds = (count + per_wave - 1u) / per_wave;
    if (w >= rounds) return;  // (limits_finish_kernel reads min(rounds, rwaves) partials)
    const MissionView v = mission_view(g.in, k);
    const int l = lane & (L - 1);
    Tally t = limits_rules::empty_tally();
    for (unsigned round = w; round < rounds; round += g.rwaves) {  // (wave-uniform)
        const unsigned at = round * per_wave + (unsigned)(lane / L);
        ItemState s = limits_rules::empty_item();
        unsigned e = 0;
        if (at < count) {
            e = ((const guint*)g.list)[(size_t)k * g.stride + at];  // (an item of the coarse kernel: e < stride, m < M)
            const int a = (int)(e / (unsigned)g.in.r.M_stride), m = (int)(e % (unsigned)g.in.r.M_stride);
            limits_rules::take_pieces(&t, &s, v.coef, v.M, v.T, v.ts, a, m, v.max_vel + 3 * (size_t)a, v.max_acc + 3 * (size_t)a, depth, l, pieces, L);
        }
        for (int off = L >> 1; off > 0; off >>= 1) {  // (over the item's own lanes: an aligned group of L)
            ItemState o;
            o.upper_vel = __shfl_xor(s.upper_vel, off), o.upper_acc = __shfl_xor(s.upper_acc, off), o.flags = __shfl_xor(s.flags, off);
            limits_rules::merge_item(&s, o);
        }
        if (at < count && l == 0) {
            limits_rules::count_item(&t, s, true);
            gdouble* up = (gdouble*)g.item_upper + ((size_t)k * g.stride + e) * 2;
            up[0] = s.upper_vel, up[1] = s.upper_acc;
        }
    }
    t = wave_tally(t);
    if (lane == 0) store_tally((gTally*)g.partial + ((size_t)k * (g.waves + g.rwaves) + g.waves + w), t);
}

__global__ __launch_bounds__(64) void limits_finish_kernel(LimitsArgs g) {
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x, N = g.in.r.N;
    const MissionView v = mission_view(g.in, k);
    const int status = g.in.r.status ? g.in.r.status[k] : 0;
    Tally t = limits_rules::empty_tally();
    if (v.computed) {
        const gTally* part = (const gTally*)g.partial + (size_t)k * (g.waves + g.rwaves);
        const unsigned count = ((const guint*)g.count)[k];
        const int pieces = 1 << g.in.depth;
        const unsigned per_wave = 64u / (unsigned)(pieces < 64 ? pieces : 64);
        const unsigned rounds = (count + per_wave - 1u) / per_wave;
        const unsigned refine_partials = rounds < g.rwaves ? rounds : g.rwaves;  // (the refine kernel's wavefronts that stored a partial)
        for (unsigned i = (unsigned)lane; i < g.waves; i += 64u) limits_rules::merge(&t, load_tally(part + i));
        for (unsigned i = (unsigned)lane; i < refine_partials; i += 64u) limits_rules::merge(&t, load_tally(part + g.waves + i));
        t = wave_tally(t);
        if (g.agent_upper) {
            const gdouble* items = (const gdouble*)g.item_upper + (size_t)k * g.stride * 2;
            for (int a = lane; a < N; a += 64) {
                ItemState au = limits_rules::empty_item();
                for (int m = 0; m < v.M; ++m) {
                    const gdouble* up = items + ((size_t)a * g.in.r.M_stride + m) * 2;
                    limits_rules::merge_item(&au, ItemState{up[0], up[1], 0});
                }
                gdouble* dst = (gdouble*)g.agent_upper + ((size_t)k * N + a) * 2;
                dst[0] = au.upper_vel, dst[1] = au.upper_acc;
            }
        }
    }
    if (lane != 0) return;
    glimits* r = (glimits*)g.out + k;
    if (status != 0) {  // nothing is computed of a mission that has failed
        t = limits_rules::empty_tally();
        r->end_time = 0.0;
    } else {
        r->end_time = report_rules::scaled_time(v.T[v.M], v.ts);
    }
    r->lower_vel_ratio = t.lower_vel.ratio, r->upper_vel_ratio = t.upper_vel.ratio;
    r->lower_acc_ratio = t.lower_acc.ratio, r->upper_acc_ratio = t.upper_acc.ratio;
    r->uncertified = t.uncertified, r->violating = t.violating, r->refined = t.refined;
    r->lower_vel_segment = t.lower_vel.segment, r->lower_vel_piece = t.lower_vel.piece, r->lower_vel_agent = t.lower_vel.agent;
    r->lower_vel_axis = t.lower_vel.axis, r->lower_vel_depth = t.lower_vel.depth;
    r->upper_vel_segment = t.upper_vel.segment, r->upper_vel_piece = t.upper_vel.piece, r->upper_vel_agent = t.upper_vel.agent;
    r->upper_vel_axis = t.upper_vel.axis, r->upper_vel_depth = t.upper_vel.depth;
    r->lower_acc_segment = t.lower_acc.segment, r->lower_acc_piece = t.lower_acc.piece, r->lower_acc_agent = t.lower_acc.agent;
    r->lower_acc_axis = t.lower_acc.axis, r->lower_acc_depth = t.lower_acc.depth;
    r->upper_acc_segment = t.upper_acc.segment, r->upper_acc_piece = t.upper_acc.piece, r->upper_acc_agent = t.upper_acc.agent;
    r->upper_acc_axis = t.upper_acc.axis, r->upper_acc_depth = t.upper_acc.depth;
    r->status = status, r->reserved = 0;
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
    s.rwaves = LIMITS_REFINE_FACTOR * s.waves;
    const unsigned long long budget = RBP_LIMITS_LIST_BYTES / sizeof(unsigned);
    unsigned long long c = s.stride ? budget / s.stride : (unsigned long long)K;
    c = c < 1 ? 1 : c;
    c = c > 65535 ? 65535 : c;  // (gridDim.y)
    s.chunk = (int)(c > (unsigned long long)K ? (unsigned long long)K : c);
    return s;
}

// missions k0 .. k0 + n of `g` as a launch of their own (the kernels index by mission through the pointers; the list, the counters, the
// items' ratios and the partials are the chunk's and are used again by the next one, which the stream orders)
LimitsArgs slice(const LimitsArgs& g, int k0, int n) {
    LimitsArgs s = g;
    ReportInputs& r = s.in.r;
    const size_t N = (size_t)r.N;
    r.K = n, r.Mk += k0, r.T += (size_t)k0 * (r.M_stride + 1), r.coef += (size_t)k0 * N * 3 * 6 * r.M_stride;
    if (r.radius) r.radius += (size_t)k0 * N;
    if (r.ts) r.ts += (size_t)k0 * r.ts_stride;
    if (r.status) r.status += k0;
    s.in.max_vel += (size_t)k0 * N * 3, s.in.max_acc += (size_t)k0 * N * 3, s.out += k0;
    if (s.agent_upper) s.agent_upper += (size_t)k0 * N * 2;
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

int limits_check_arguments(const char* who, int32_t depth, double refine_above) {
    if (depth < 0 || depth > RBP_LIMITS_MAX_DEPTH)
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": depth must lie in 0 .. " + std::to_string(RBP_LIMITS_MAX_DEPTH)).c_str());
    if (refine_above != refine_above) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": refine_above must be a number").c_str());
    return RBP_OK;
}

size_t limits_workspace_bytes(int K, int N, int M_stride) {
    const Shape s = shape_of(K, N, M_stride);
    return al256(sizeof(rbp_limits) * (size_t)K) + al256(sizeof(unsigned) * (size_t)s.chunk) +
           al256(sizeof(unsigned) * (size_t)s.chunk * (size_t)s.stride) + al256(sizeof(double) * 2 * (size_t)s.chunk * (size_t)s.stride) +
           sizeof(Tally) * (size_t)s.chunk * ((size_t)s.waves + s.rwaves);
}

int launch_limits(const LimitsInputs& in, double* agent_upper, void* workspace, hipStream_t st) {
    const int K = in.r.K, N = in.r.N;
    if (K <= 0 || N <= 0 || in.r.M_stride <= 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "limits: no mission, no agent or no segment");
    if (int rc = limits_check_arguments("limits", in.depth, in.refine_above)) return rc;
    const Shape sh = shape_of(K, N, in.r.M_stride);
    if (sh.stride > LIMITS_MAX_ITEMS) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "limits: a mission of more than 2^32 - 64 (agent, segment) items");
    LimitsArgs g{};
    g.in = in, g.stride = (unsigned)sh.stride, g.waves = sh.waves, g.rwaves = sh.rwaves;
    g.agent_upper = agent_upper;
    char* p = static_cast<char*>(workspace);
    g.out = reinterpret_cast<rbp_limits*>(p), p += al256(sizeof(rbp_limits) * (size_t)K);
    g.count = reinterpret_cast<unsigned*>(p), p += al256(sizeof(unsigned) * (size_t)sh.chunk);
    g.list = reinterpret_cast<unsigned*>(p), p += al256(sizeof(unsigned) * (size_t)sh.chunk * (size_t)sh.stride);
    g.item_upper = reinterpret_cast<double*>(p), p += al256(sizeof(double) * 2 * (size_t)sh.chunk * (size_t)sh.stride);
    g.partial = reinterpret_cast<Tally*>(p);
    const unsigned blocks = (sh.waves + LIMITS_WAVES - 1) / LIMITS_WAVES, rblocks = (sh.rwaves + LIMITS_WAVES - 1) / LIMITS_WAVES;
    for (int k0 = 0; k0 < K; k0 += sh.chunk) {
        const int n = std::min(sh.chunk, K - k0);
        const LimitsArgs s = slice(g, k0, n);
        hipLaunchKernelGGL(limits_init_kernel, dim3((unsigned)(n + 63) / 64u), dim3(64), 0, st, s);
        hipLaunchKernelGGL(limits_coarse_kernel, dim3(blocks, (unsigned)n), dim3(LIMITS_THREADS), 0, st, s);
        hipLaunchKernelGGL(limits_refine_kernel, dim3(rblocks, (unsigned)n), dim3(LIMITS_THREADS), 0, st, s);
        hipLaunchKernelGGL(limits_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string("limits kernels: launch: ") + hipGetErrorString(e)).c_str());
}

// The kernels on device inputs, the K records copied to `out` on the host in one copy, the agents' upper ratios to wherever the caller
// wants them (the current device is `device`): a destination on the device is written in place by the finish kernel; a host destination
// goes through one staging buffer and one copy, of which only the rows of the missions that were computed reach the caller's array.
int limits_run(const char* who, int device, const LimitsInputs& in, rbp_limits* out, double* agent_upper, void* workspace, hipStream_t st) {
    auto fail = [&](hipError_t err) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(err)).c_str()); };
    const int ad = agent_upper ? on_device(agent_upper, device) : 1;
    if (ad < 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": agent_upper lies on another device than the plans (device " + std::to_string(device) + ")").c_str());
    const size_t K = (size_t)in.r.K, row = (size_t)in.r.N * 2;
    DeviceBuffers b;
    double* stage = ad ? nullptr : b.get<double>(K * row);
    if (b.err != hipSuccess) return fail(b.err);
    if (int rc = launch_limits(in, ad ? agent_upper : stage, workspace, st)) return rc;
    hipError_t e = hipMemcpyAsync(out, workspace, sizeof(rbp_limits) * K, hipMemcpyDeviceToHost, st);
    std::vector<double> rows;
    if (!ad && e == hipSuccess) {
        rows.resize(K * row);
        e = hipMemcpyAsync(rows.data(), stage, sizeof(double) * K * row, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    if (!ad)
        for (size_t k = 0; k < K; ++k)
            if (out[k].status == 0) std::copy(rows.begin() + k * row, rows.begin() + (k + 1) * row, agent_upper + k * row);
    return RBP_OK;
}

extern "C" int rbp_dev_limits(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T, const double* time_scale,
                              const double* coef, const double* max_vel, const double* max_acc, int32_t depth, double refine_above,
                              rbp_limits* out, double* agent_upper) {
    auto bad = [&](const std::string& what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, ("rbp_dev_limits: " + what).c_str()); };
    if (!M || !T || !coef || !max_vel || !max_acc || !out) return bad("M, T, coef, max_vel, max_acc and out must be given");
    if (K <= 0 || N <= 0 || M_stride <= 0) return bad("K, N and M_stride must be positive");
    if (int rc = limits_check_arguments("rbp_dev_limits", depth, refine_above)) return rc;
    for (int k = 0; k < K; ++k) {
        if (M[k] <= 0 || M[k] > M_stride) return bad("mission " + std::to_string(k) + ": M outside 1..M_stride");
        if (time_scale && !(time_scale[k] > 0)) return bad("mission " + std::to_string(k) + ": the time scale must be positive");
        for (size_t i = (size_t)k * N * 3; i < (size_t)(k + 1) * N * 3; ++i)
            if (!(max_vel[i] > 0) || !(max_acc[i] > 0)) return bad("mission " + std::to_string(k) + ": every limit must be a positive number");
    }
    if ((unsigned long long)N * (unsigned long long)M_stride > LIMITS_MAX_ITEMS) return bad("a mission of more than 2^32 - 64 (agent, segment) items");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rbp_set_error(RBP_ERR_NO_DEVICE, "no HIP device: the limits kernels have no CPU fallback (rbp_limits_host is the host's)");
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
    LimitsInputs in{};
    ReportInputs& r = in.r;
    r.K = K, r.N = N, r.M_stride = M_stride, r.downwash = 1.0, r.dt = 0.0;
    r.Mk = up(M, (size_t)K);
    r.T = up(T, (size_t)K * (M_stride + 1));
    r.coef = up(coef, (size_t)K * N * 3 * 6 * M_stride);
    r.radius = nullptr;
    r.ts = time_scale ? up(time_scale, (size_t)K) : nullptr, r.ts_stride = 1;
    r.status = nullptr;
    in.max_vel = up(max_vel, (size_t)K * N * 3);
    in.max_acc = up(max_acc, (size_t)K * N * 3);
    in.depth = depth, in.refine_above = refine_above;
    char* ws = b.get<char>(limits_workspace_bytes(K, N, M_stride));
    if (b.err != hipSuccess) return rbp_set_error(RBP_ERR_HIP, (std::string("rbp_dev_limits: ") + hipGetErrorString(b.err)).c_str());
    return limits_run("rbp_dev_limits", device, in, out, agent_upper, ws, 0);
}
