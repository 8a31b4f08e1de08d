// separation.hip — a certified interval for the smallest safety ratio of resident plans in continuous time, where the coefficients
// are: in HBM (gfx950).
//
// For K missions, from a session's own arrays (rbp_session_separation, abi/session.hip) or a caller's (rbp_dev_separation).  An item is a
// pair qi < qj and a segment m; a mission's items are numbered e = pair * M_stride + m, the segment fastest, so that the 64 items of a
// wavefront read the coefficient rows of few agents.  Four launches per chunk of missions, the mission in gridDim.y:
//   separation_init_kernel    clears the mission's work-list counter and, where the caller wants the pairs' lower ratios on the device,
//                             sets the row of a mission that is computed to 1e9.
//   separation_coarse_kernel  one lane per item, one wavefront per 64 consecutive items.  A lane forms the item's control points and S
//                             (separation_rules::item_of) and its depth-0 bounds.  Items that stay at depth 0 are folded into the lane's
//                             tally; the others are appended to the mission's work list, one uint32 each: ballot, popcount, ONE atomic
//                             add per wavefront, the lane's place from the ballot's lower bits.  The list's order depends on the
//                             schedule; nothing that is reported does.  The tallies are reduced over the wavefront by a shuffle
//                             butterfly under the rule's order and lane 0 stores one partial per wavefront.
//   separation_refine_kernel  one lane per listed item, walking its 2^depth pieces; a piece is D halvings from the segment's control
//                             points (separation_rules::item_piece), so a lane holds the 18 doubles of the segment, 18 of the piece and
//                             11 of q in registers: no LDS, no scratch.  (The alternative, a lane per (item, piece), was not built.)
//                             Wavefronts beyond the list's length leave at once; the others store one partial each.
//   separation_finish_kernel  one wavefront per mission merges the partials of both kernels (separation_rules::merge) and writes the
//                             rbp_separation.  A mission with a status is written here and skipped by the others.
// The pairs' lower ratios are kept with a 64-bit integer atomic minimum on the doubles' bit patterns: the ratios are non-negative, so they
// order like their bits and the result does not depend on the order of arrival.
// Every number is a rule of common/separation_rules.h -- the text rbp_separation_host (host/validate.cpp) loops over -- and the headers'
// `#pragma clang fp contract(off)` holds for this whole file.  Plain C++, vector stores only.
#include "rbp_dev.h"

#include <string>
#include <type_traits>

#include "common/separation_rules.h"

namespace {

constexpr int SEP_THREADS = 256;
constexpr int SEP_WAVES = SEP_THREADS / 64;  // wavefronts of a workgroup: 64 items each
// the most items of one mission: an item's number is a uint32, and so is the number the last wavefront's last lane forms beyond them
constexpr unsigned long long SEP_MAX_ITEMS = (1ull << 32) - 64;

using separation_rules::Minimum;
using separation_rules::Tally;
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) unsigned guint;
typedef __attribute__((address_space(1))) rbp_separation gseparation;

static_assert(sizeof(Tally) == 88, "two minima of a double and five words (padded to 32 bytes), three counters");
static_assert(sizeof(rbp_separation) == 96, "three doubles, three counters, twelve words");
typedef __attribute__((address_space(1))) Tally gTally;

struct SepArgs {
    ReportInputs in;      // (dt is not read)
    int depth;
    double refine_below;
    long long pairs;      // N (N - 1) / 2
    unsigned stride;      // items of a mission's slot: pairs * M_stride
    unsigned waves;       // wavefronts of a mission: ceil(stride / 64)
    unsigned* count;      // [n] work-list lengths
    unsigned* list;       // [n][stride]
    Tally* partial;       // [n][2 * waves]: the coarse kernel's, then the refine kernel's
    double* pair_lower;   // [n][pairs] on the device, or null
    rbp_separation* out;  // [n]
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

// the row start of agent qi in the pair order, and the pair (qi, qj) of an index below N (N - 1) / 2
__device__ __forceinline__ long long row_start(int N, int qi) { return separation_rules::pair_index(N, qi, qi + 1); }
__device__ __forceinline__ void pair_of(int N, long long pair, int* qi, int* qj) {
    const double b = 2.0 * N - 1.0;
    int i = (int)((b - sqrt(b * b - 8.0 * (double)pair)) / 2.0);  // an estimate, put right by the two loops
    i = i < 0 ? 0 : (i > N - 2 ? N - 2 : i);
    while (i > 0 && row_start(N, i) > pair) --i;
    while (i < N - 2 && row_start(N, i + 1) <= pair) ++i;
    *qi = i, *qj = i + 1 + (int)(pair - row_start(N, i));
}

__device__ __forceinline__ Minimum shuffled(const Minimum& m, int off) {
    return Minimum{__shfl_xor(m.ratio, off), __shfl_xor(m.segment, off), __shfl_xor(m.piece, off), __shfl_xor(m.qi, off), __shfl_xor(m.qj, off), __shfl_xor(m.depth, off)};
}
// the wavefront's tally under the rule's order, in every lane
__device__ __forceinline__ Tally wave_tally(Tally t) {
    for (int off = 32; off > 0; off >>= 1) {
        Tally o;
        o.lower = shuffled(t.lower, off), o.upper = shuffled(t.upper, off);
        o.uncertified = __shfl_xor(t.uncertified, off), o.colliding = __shfl_xor(t.colliding, off), o.refined = __shfl_xor(t.refined, off);
        separation_rules::merge(&t, o);
    }
    return t;
}
__device__ __forceinline__ void store_tally(gTally* p, const Tally& t) {
    p->lower.ratio = t.lower.ratio, p->lower.segment = t.lower.segment, p->lower.piece = t.lower.piece, p->lower.qi = t.lower.qi;
    p->lower.qj = t.lower.qj, p->lower.depth = t.lower.depth;
    p->upper.ratio = t.upper.ratio, p->upper.segment = t.upper.segment, p->upper.piece = t.upper.piece, p->upper.qi = t.upper.qi;
    p->upper.qj = t.upper.qj, p->upper.depth = t.upper.depth;
    p->uncertified = t.uncertified, p->colliding = t.colliding, p->refined = t.refined;
}
__device__ __forceinline__ Tally load_tally(const gTally* p) {
    Tally t;
    t.lower = Minimum{p->lower.ratio, p->lower.segment, p->lower.piece, p->lower.qi, p->lower.qj, p->lower.depth};
    t.upper = Minimum{p->upper.ratio, p->upper.segment, p->upper.piece, p->upper.qi, p->upper.qj, p->upper.depth};
    t.uncertified = p->uncertified, t.colliding = p->colliding, t.refined = p->refined;
    return t;
}

// a pair's lower ratio into the caller's array: non-negative doubles order like their bits (a NaN, or 1e9 and more, is not taken)
__device__ __forceinline__ void pair_minimum(double* pair_lower, long long index, double lower) {
    if (!(lower < RBP_REPORT_NO_RATIO)) return;
    unsigned long long bits;
    __builtin_memcpy(&bits, &lower, 8);
    atomicMin(reinterpret_cast<unsigned long long*>(pair_lower) + index, bits);
}

__global__ __launch_bounds__(SEP_THREADS) void separation_init_kernel(SepArgs g) {
    const int k = (int)blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) ((guint*)g.count)[k] = 0u;
    if (!g.pair_lower) return;
    if (g.in.status && g.in.status[k] != 0) return;  // (the row of a mission that is not computed stays as it is)
    gdouble* row = (gdouble*)g.pair_lower + (size_t)k * (size_t)g.pairs;
    for (long long p = (long long)blockIdx.x * SEP_THREADS + threadIdx.x; p < g.pairs; p += (long long)gridDim.x * SEP_THREADS)
        row[p] = RBP_REPORT_NO_RATIO;
}

__global__ __launch_bounds__(SEP_THREADS) void separation_coarse_kernel(SepArgs g) {
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, N = g.in.N;
    const unsigned w = blockIdx.x * SEP_WAVES + (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    if (w >= g.waves) return;  // (no barrier in this kernel: a wavefront may leave on its own)
    const MissionView v = mission_view(g.in, k);
    if (!v.computed) return;  // (separation_finish_kernel writes the mission)
    const unsigned e = w * 64u + (unsigned)lane;
    const long long pair = (long long)(e / (unsigned)g.in.M_stride);
    const int m = (int)(e % (unsigned)g.in.M_stride);
    const bool active = e < g.stride && m < v.M;
    Tally t = separation_rules::empty_tally();
    bool refine = false;
    if (active) {
        int qi, qj;
        pair_of(N, pair, &qi, &qj);
        const double radius_sum = v.radius[qi] + v.radius[qj];
        const separation_rules::Item it = separation_rules::item_of(v.coef, v.M, v.T, v.ts, qi, qj, m, g.in.downwash);
        const separation_rules::Bounds b0 = separation_rules::item_piece(it, 0, 0, radius_sum);
        refine = separation_rules::is_refined(b0.lower, g.refine_below);
        if (!refine) {  // (it stays at depth 0, whose bounds are at hand)
            double item_lower = RBP_REPORT_NO_RATIO, item_upper = RBP_REPORT_NO_RATIO;
            separation_rules::take_piece(&t, &item_lower, &item_upper, b0, 0, 0, m, qi, qj);
            separation_rules::count_item(&t, item_lower, item_upper, false);
            if (g.pair_lower) pair_minimum(g.pair_lower, (long long)k * g.pairs + pair, item_lower);
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
    if (lane == 0) store_tally((gTally*)g.partial + ((size_t)k * 2u * g.waves + w), t);
}

__global__ __launch_bounds__(SEP_THREADS) void separation_refine_kernel(SepArgs g) {
    const int k = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, N = g.in.N;
    const unsigned w = blockIdx.x * SEP_WAVES + (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    if (w >= g.waves) return;
    const unsigned count = ((const guint*)g.count)[k];  // (<= stride; 0 for a mission that is not computed)
    if ((unsigned long long)w * 64u >= count) return;
    const MissionView v = mission_view(g.in, k);
    const unsigned at = w * 64u + (unsigned)lane;
    Tally t = separation_rules::empty_tally();
    if (at < count) {
        const unsigned e = ((const guint*)g.list)[(size_t)k * g.stride + at];  // (an item of the coarse kernel: e < stride, m < M)
        const long long pair = (long long)(e / (unsigned)g.in.M_stride);
        const int m = (int)(e % (unsigned)g.in.M_stride);
        int qi, qj;
        pair_of(N, pair, &qi, &qj);
        const double radius_sum = v.radius[qi] + v.radius[qj];
        const separation_rules::Item it = separation_rules::item_of(v.coef, v.M, v.T, v.ts, qi, qj, m, g.in.downwash);
        double item_lower = RBP_REPORT_NO_RATIO, item_upper = RBP_REPORT_NO_RATIO;
        separation_rules::take_pieces(&t, &item_lower, &item_upper, it, g.depth, 0, 1 << g.depth, radius_sum, m, qi, qj);
        separation_rules::count_item(&t, item_lower, item_upper, true);
        if (g.pair_lower) pair_minimum(g.pair_lower, (long long)k * g.pairs + pair, item_lower);
    }
    t = wave_tally(t);
    if (lane == 0) store_tally((gTally*)g.partial + ((size_t)k * 2u * g.waves + g.waves + w), t);
}

__global__ __launch_bounds__(64) void separation_finish_kernel(SepArgs g) {
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
    const MissionView v = mission_view(g.in, k);
    const int status = g.in.status ? g.in.status[k] : 0;
    Tally t = separation_rules::empty_tally();
    if (v.computed) {
        const gTally* part = (const gTally*)g.partial + (size_t)k * 2u * g.waves;
        const unsigned count = ((const guint*)g.count)[k];
        const unsigned refined_waves = (count + 63u) / 64u;  // (the refine kernel's wavefronts that stored a partial)
        for (unsigned i = (unsigned)lane; i < g.waves; i += 64u) separation_rules::merge(&t, load_tally(part + i));
        for (unsigned i = (unsigned)lane; i < refined_waves; i += 64u) separation_rules::merge(&t, load_tally(part + g.waves + i));
        t = wave_tally(t);
    }
    if (lane != 0) return;
    gseparation* r = (gseparation*)g.out + k;
    if (status != 0) {  // nothing is computed of a mission that has failed
        r->lower_ratio = 0.0, r->upper_ratio = 0.0, r->end_time = 0.0, r->uncertified = 0, r->colliding = 0, r->refined = 0;
        r->lower_segment = -1, r->lower_piece = -1, r->lower_qi = -1, r->lower_qj = -1;
        r->upper_segment = -1, r->upper_piece = -1, r->upper_qi = -1, r->upper_qj = -1;
        r->lower_depth = -1, r->upper_depth = -1, r->status = status, r->reserved = 0;
        return;
    }
    r->lower_ratio = t.lower.ratio, r->upper_ratio = t.upper.ratio, r->end_time = report_rules::scaled_time(v.T[v.M], v.ts);
    r->uncertified = t.uncertified, r->colliding = t.colliding, r->refined = t.refined;
    r->lower_segment = t.lower.segment, r->lower_piece = t.lower.piece, r->lower_qi = t.lower.qi, r->lower_qj = t.lower.qj;
    r->upper_segment = t.upper.segment, r->upper_piece = t.upper.piece, r->upper_qi = t.upper.qi, r->upper_qj = t.upper.qj;
    r->lower_depth = t.lower.depth, r->upper_depth = t.upper.depth, r->status = 0, r->reserved = 0;
}

size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

// how a call's missions are cut: a mission's items, its wavefronts, and the missions of a chunk under the work list's budget
struct Shape {
    unsigned long long pairs, stride;
    unsigned waves;
    int chunk;
};
Shape shape_of(int K, int N, int M_stride) {
    Shape s;
    s.pairs = (unsigned long long)N * (unsigned long long)(N - 1) / 2;
    s.stride = s.pairs * (unsigned long long)M_stride;
    s.waves = (unsigned)((s.stride + 63) / 64);
    const unsigned long long budget = RBP_SEPARATION_LIST_BYTES / sizeof(unsigned);
    unsigned long long c = s.stride ? budget / s.stride : (unsigned long long)K;
    c = c < 1 ? 1 : c;
    c = c > 65535 ? 65535 : c;  // (gridDim.y)
    s.chunk = (int)(c > (unsigned long long)K ? (unsigned long long)K : c);
    return s;
}

// missions k0 .. k0 + n of `g` as a launch of their own (the kernels index by mission through the pointers; the list, the counters and
// the partials are the chunk's and are used again by the next one, which the stream orders)
SepArgs slice(const SepArgs& g, int k0, int n) {
    SepArgs s = g;
    ReportInputs& r = s.in;
    const size_t N = (size_t)r.N;
    r.K = n, r.Mk += k0, r.T += (size_t)k0 * (r.M_stride + 1), r.coef += (size_t)k0 * N * 3 * 6 * r.M_stride, r.radius += (size_t)k0 * N;
    if (r.ts) r.ts += (size_t)k0 * r.ts_stride;
    if (r.status) r.status += k0;
    s.out += k0;
    if (s.pair_lower) s.pair_lower += (size_t)k0 * (size_t)g.pairs;
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

int separation_check_arguments(const char* who, int32_t depth, double refine_below) {
    if (depth < 0 || depth > RBP_SEPARATION_MAX_DEPTH)
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": depth must lie in 0 .. " + std::to_string(RBP_SEPARATION_MAX_DEPTH)).c_str());
    if (!(refine_below > 0)) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": refine_below must be a number above 0").c_str());
    return RBP_OK;
}

size_t separation_workspace_bytes(int K, int N, int M_stride) {
    const Shape s = shape_of(K, N, M_stride);
    return al256(sizeof(rbp_separation) * (size_t)K) + al256(sizeof(unsigned) * (size_t)s.chunk) +
           al256(sizeof(unsigned) * (size_t)s.chunk * (size_t)s.stride) + sizeof(Tally) * (size_t)s.chunk * 2 * (size_t)s.waves;
}

int launch_separation(const SeparationInputs& in, double* pair_lower, void* workspace, hipStream_t st) {
    const int K = in.r.K, N = in.r.N;
    if (K <= 0 || N <= 0 || in.r.M_stride <= 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "separation: no mission, no agent or no segment");
    if (int rc = separation_check_arguments("separation", in.depth, in.refine_below)) return rc;
    const Shape sh = shape_of(K, N, in.r.M_stride);
    if (sh.stride > SEP_MAX_ITEMS) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "separation: a mission of more than 2^32 - 64 (pair, segment) items");
    SepArgs g{};
    g.in = in.r, g.depth = in.depth, g.refine_below = in.refine_below;
    g.pairs = (long long)sh.pairs, g.stride = (unsigned)sh.stride, g.waves = sh.waves;
    g.pair_lower = pair_lower;
    char* p = static_cast<char*>(workspace);
    g.out = reinterpret_cast<rbp_separation*>(p), p += al256(sizeof(rbp_separation) * (size_t)K);
    g.count = reinterpret_cast<unsigned*>(p), p += al256(sizeof(unsigned) * (size_t)sh.chunk);
    g.list = reinterpret_cast<unsigned*>(p), p += al256(sizeof(unsigned) * (size_t)sh.chunk * (size_t)sh.stride);
    g.partial = reinterpret_cast<Tally*>(p);
    const unsigned init_blocks = (unsigned)std::min<unsigned long long>(std::max<unsigned long long>(1, (sh.pairs + SEP_THREADS - 1) / SEP_THREADS), 1024);
    const unsigned blocks = (sh.waves + SEP_WAVES - 1) / SEP_WAVES;
    for (int k0 = 0; k0 < K; k0 += sh.chunk) {
        const int n = std::min(sh.chunk, K - k0);
        const SepArgs s = slice(g, k0, n);
        hipLaunchKernelGGL(separation_init_kernel, dim3(init_blocks, (unsigned)n), dim3(SEP_THREADS), 0, st, s);
        if (blocks) {  // (a mission of one agent has no item)
            hipLaunchKernelGGL(separation_coarse_kernel, dim3(blocks, (unsigned)n), dim3(SEP_THREADS), 0, st, s);
            hipLaunchKernelGGL(separation_refine_kernel, dim3(blocks, (unsigned)n), dim3(SEP_THREADS), 0, st, s);
        }
        hipLaunchKernelGGL(separation_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string("separation kernels: launch: ") + hipGetErrorString(e)).c_str());
}

// The kernels on device inputs, the K records copied to `out` on the host in one copy, the pairs' lower ratios to wherever the caller
// wants them (the current device is `device`): a destination on the device is written in place; a host destination goes through one
// staging buffer and one copy, of which only the rows of the missions that were computed reach the caller's array.
int separation_run(const char* who, int device, const SeparationInputs& in, rbp_separation* out, double* pair_lower, void* workspace, hipStream_t st) {
    auto fail = [&](hipError_t err) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(err)).c_str()); };
    const int pd = pair_lower ? on_device(pair_lower, device) : 1;
    if (pd < 0) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": pair_lower lies on another device than the plans (device " + std::to_string(device) + ")").c_str());
    const size_t K = (size_t)in.r.K, P = (size_t)in.r.N * (size_t)(in.r.N - 1) / 2;
    DeviceBuffers b;
    double* stage = pd ? nullptr : b.get<double>(K * P);
    if (b.err != hipSuccess) return fail(b.err);
    if (int rc = launch_separation(in, pd ? pair_lower : stage, workspace, st)) return rc;
    hipError_t e = hipMemcpyAsync(out, workspace, sizeof(rbp_separation) * K, hipMemcpyDeviceToHost, st);
    std::vector<double> rows;
    if (!pd && P && e == hipSuccess) {
        rows.resize(K * P);
        e = hipMemcpyAsync(rows.data(), stage, sizeof(double) * K * P, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    if (!pd && P)
        for (size_t k = 0; k < K; ++k)
            if (out[k].status == 0) std::copy(rows.begin() + k * P, rows.begin() + (k + 1) * P, pair_lower + k * P);
    return RBP_OK;
}

extern "C" int rbp_dev_separation(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T, const double* time_scale,
                                  const double* coef, const double* radius, double downwash, int32_t depth, double refine_below,
                                  rbp_separation* out, double* pair_lower) {
    auto bad = [&](const std::string& what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, ("rbp_dev_separation: " + what).c_str()); };
    if (!M || !T || !coef || !radius || !out) return bad("M, T, coef, radius and out must be given");
    if (K <= 0 || N <= 0 || M_stride <= 0 || !(downwash > 0)) return bad("K, N, M_stride and downwash must be positive");
    if (int rc = separation_check_arguments("rbp_dev_separation", depth, refine_below)) return rc;
    for (int k = 0; k < K; ++k) {
        if (M[k] <= 0 || M[k] > M_stride) return bad("mission " + std::to_string(k) + ": M outside 1..M_stride");
        if (time_scale && !(time_scale[k] > 0)) return bad("mission " + std::to_string(k) + ": the time scale must be positive");
    }
    if ((unsigned long long)N * (unsigned long long)(N - 1) / 2 * (unsigned long long)M_stride > SEP_MAX_ITEMS)
        return bad("a mission of more than 2^32 - 64 (pair, segment) items");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rbp_set_error(RBP_ERR_NO_DEVICE, "no HIP device: the separation kernels have no CPU fallback (rbp_separation_host is the host's)");
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
    SeparationInputs in{};
    ReportInputs& r = in.r;
    r.K = K, r.N = N, r.M_stride = M_stride, r.downwash = downwash, r.dt = 0.0;
    r.Mk = up(M, (size_t)K);
    r.T = up(T, (size_t)K * (M_stride + 1));
    r.coef = up(coef, (size_t)K * N * 3 * 6 * M_stride);
    r.radius = up(radius, (size_t)K * N);
    r.ts = time_scale ? up(time_scale, (size_t)K) : nullptr, r.ts_stride = 1;
    r.status = nullptr;
    in.depth = depth, in.refine_below = refine_below;
    char* ws = b.get<char>(separation_workspace_bytes(K, N, M_stride));
    if (b.err != hipSuccess) return rbp_set_error(RBP_ERR_HIP, (std::string("rbp_dev_separation: ") + hipGetErrorString(b.err)).c_str());
    return separation_run("rbp_dev_separation", device, in, out, pair_lower, ws, 0);
}
