// plan_stage.h — the staging block of rbp_session_refill_from_plans, stated once for the host packer (abi/session.hip), the kernel that
// empties it (kernels/handoff.hip session_refill_plans_kernel) and the stand-alone check of both (tests/plan_stage/stage_main.cpp).
//
// A caller's K missions go to the device in ROUNDS: as many consecutive missions as fit the block are packed tightly into it, the block
// goes up in one copy, one kernel launch writes the slots [j0, j0 + n) of the session from it.  A round of n missions of N agents is
//   Entry   [n]            per mission Mk, MBk, its world descriptor and the offsets of its T and init_traj in the block
//   src     [n] int32      0 .. n-1: the source list mission_gather_element (kernels/handoff.hip) reads, in 8 n bytes
//   start   [n][N][9]  goal [n][N][9]  radius [n][N]  max_vel [n][N][3]  max_acc [n][N][3]   doubles, that element body's layout
//   per mission, in order: T [Mk + 1] doubles, init_traj [N][Mk + 1][3] floats (the compact rows a session slot holds,
//                          kernels/rbp_dev.h), padded to 8 bytes
// so a mission costs mission_bytes(N, Mk) wherever it stands and a round is the sum over its missions.  Every offset is in bytes from
// the start of the block and a multiple of 8 (init_traj: of 4).
//
// The element rules say what the kernel stores for a flat index of a round; the packer's check walks the same functions on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PS_FN __host__ __device__ inline
#else
#define PS_FN inline
#endif

namespace plan_stage {

constexpr int WORLD_WORDS = 5;  // a world descriptor (DevWorld of kernels/rbp_dev.h) in 8-byte words: dim[3], key_min[3], res, dist

struct Entry {
    int32_t Mk, MBk;
    unsigned long long world[WORLD_WORDS];
    unsigned long long off_T, off_traj;
};
static_assert(sizeof(Entry) == 64, "an entry is eight 8-byte words");

// what the kernel needs beside the block: the slots the round fills and the session's shape (stride = waypoints a slot has room for per agent)
struct Round {
    int j0, n, N, stride;
};

PS_FN size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }
PS_FN size_t mission_bytes(int N, int M) {
    return sizeof(Entry) + 8 + 200 * (size_t)N + 8 * ((size_t)M + 1) + align8(12 * (size_t)N * ((size_t)M + 1));
}

// offsets of a round's tables
PS_FN size_t off_entries() { return 0; }
PS_FN size_t off_src(int n) { return sizeof(Entry) * (size_t)n; }
PS_FN size_t off_start(int n) { return off_src(n) + 8 * (size_t)n; }
PS_FN size_t off_goal(int n, int N) { return off_start(n) + 72 * (size_t)N * n; }
PS_FN size_t off_radius(int n, int N) { return off_goal(n, N) + 72 * (size_t)N * n; }
PS_FN size_t off_max_vel(int n, int N) { return off_radius(n, N) + 8 * (size_t)N * n; }
PS_FN size_t off_max_acc(int n, int N) { return off_max_vel(n, N) + 24 * (size_t)N * n; }
PS_FN size_t off_payload(int n, int N) { return off_max_acc(n, N) + 24 * (size_t)N * n; }

// the greedy partition: the round that starts at mission j0 ends before the returned mission -- as many consecutive missions as fit
// `block_bytes`.  Returns j0 when not even mission j0 fits.
inline int round_end(const int* Mk, int K, int N, int j0, size_t block_bytes) {
    size_t used = 0;
    int j = j0;
    while (j < K && mission_bytes(N, Mk[j]) <= block_bytes - used) used += mission_bytes(N, Mk[j]), ++j;
    return j;
}

// the bytes of the round [j0, j1)
inline size_t round_bytes(const int* Mk, int N, int j0, int j1) {
    size_t b = 0;
    for (int j = j0; j < j1; ++j) b += mission_bytes(N, Mk[j]);
    return b;
}

// One mission as the packer takes it: host arrays of the shapes include/rbp.h gives rbp_plan and rbp_mission.
struct Source {
    int M, MB;
    const void* world;  // WORLD_WORDS 8-byte words
    const double* T;
    const float* init_traj;
    const double *start, *goal, *radius, *max_vel, *max_acc;
};

// packs the round of the n missions src[0 .. n-1] into `block`; returns its bytes (= the sum of their mission_bytes)
inline size_t pack_round(char* block, const Source* src, int n, int N) {
    Entry* entries = reinterpret_cast<Entry*>(block + off_entries());
    int32_t* ids = reinterpret_cast<int32_t*>(block + off_src(n));
    size_t off = off_payload(n, N);
    for (int r = 0; r < n; ++r) {
        const Source& s = src[r];
        const size_t P = (size_t)s.M + 1;
        Entry& e = entries[r];
        e.Mk = s.M, e.MBk = s.MB;
        memcpy(e.world, s.world, sizeof(e.world));
        ids[2 * r] = 0, ids[2 * r + 1] = 0;  // (the list is the first n of these 2 n words; written below)
        memcpy(block + off_start(n) + 72 * (size_t)N * r, s.start, 72 * (size_t)N);
        memcpy(block + off_goal(n, N) + 72 * (size_t)N * r, s.goal, 72 * (size_t)N);
        memcpy(block + off_radius(n, N) + 8 * (size_t)N * r, s.radius, 8 * (size_t)N);
        memcpy(block + off_max_vel(n, N) + 24 * (size_t)N * r, s.max_vel, 24 * (size_t)N);
        memcpy(block + off_max_acc(n, N) + 24 * (size_t)N * r, s.max_acc, 24 * (size_t)N);
        e.off_T = off;
        memcpy(block + off, s.T, 8 * P);
        off += 8 * P;
        e.off_traj = off;
        const size_t tb = 12 * (size_t)N * P;
        memcpy(block + off, s.init_traj, tb);
        memset(block + off + tb, 0, align8(tb) - tb);
        off += align8(tb);
    }
    for (int r = 0; r < n; ++r) ids[r] = r;
    return off;
}

// ---- the element rules: what a flat index of a round stores, and where ---------------------------------------------------------------
PS_FN const Entry& entry(const char* block, int r) { return reinterpret_cast<const Entry*>(block + off_entries())[r]; }
PS_FN long long traj_elements(const Round& R) { return 3LL * R.N * R.stride * R.n; }
PS_FN long long time_elements(const Round& R) { return (long long)R.stride * R.n; }

// float i (< traj_elements) of the round: float f of slot j of init_traj is the staged float when f < 3 N (Mj + 1), else 0.0f.
// *dst is its index in the session's init_traj [K][3 N stride].
PS_FN float traj_element(const char* block, const Round& R, long long i, long long* dst) {
    const long long slot = 3LL * R.N * R.stride;
    const int r = (int)(i / slot);
    const long long f = i - (long long)r * slot;
    const Entry& e = entry(block, r);
    *dst = (long long)(R.j0 + r) * slot + f;
    return f < 3LL * R.N * (e.Mk + 1) ? reinterpret_cast<const float*>(block + e.off_traj)[f] : 0.0f;
}

// double i (< time_elements) of the round: element t of row j of T is staged when t <= Mj, else 0.0.  *dst is its index in T [K][stride].
PS_FN double time_element(const char* block, const Round& R, long long i, long long* dst) {
    const int r = (int)(i / R.stride), t = (int)(i - (long long)r * R.stride);
    const Entry& e = entry(block, r);
    *dst = (long long)(R.j0 + r) * R.stride + t;
    return t <= e.Mk ? reinterpret_cast<const double*>(block + e.off_T)[t] : 0.0;
}

}  // namespace plan_stage
