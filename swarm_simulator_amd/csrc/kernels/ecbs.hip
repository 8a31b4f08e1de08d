// ecbs.hip — the ECBS front-end search on gfx950, one wavefront per mission.
//
// The search of csrc/host/ecbs.cpp (rbp_ecbs_plan_obstacles: root solutions in agent order, the high-level focal search, the low-level
// A*-epsilon over (t, x, y, z), the final statistics), run where the missions already are.  The host library is the reference, and the
// device search returns ITS bits: every queue of ecbs.cpp has a total order that ends in a node id, so the minimum std::set::begin()
// returns is the minimum a lane-strided scan with a wave reduction finds over an unordered array; everything is integer arithmetic apart
// from the two conflict predicates; those, the planning lattice, position -> cell and the writer of T / init_traj are read from common/ecbs_rules.h.
//
// One workgroup is one wavefront; it takes missions from an atomic counter until none is left, so the grid is sized to the device and the
// workspace belongs to the wave SLOT: a low-level node pool with its open array, a "seen" bitmap over (t, cell), a high-level node pool.
//   low level   open entries are (f, -g | focal + in-focal bit | id) in three arrays; a pop is one coalesced pass that finds min f and the
//               focal minimum by (focal, f, -g, id) at once, a widening (min f went up) is a second pass that flags old w < f <= new w.
//               `best` and `closed` of the host are one bit per (t, cell): a state is skipped if it is in either, and the first discovery
//               is never replaced.  Only the time layers a search touched are cleared.
//               The validity of the 7 neighbours (mask, seen bit, the agent's constraints from LDS) is tested by 7 x 9 lanes at once;
//               the two focal terms of a valid neighbour are ballots over the other agents (chunks of 64).
//   high level  a node keeps the one path it replanned, its constraint and its parent; a popped node's solution is put together in LDS
//               from its ancestor chain (global memory when N * (L + 1) cells do not fit), and so are an agent's constraints.
//               count_conflicts / first_conflict: per time step and agent i, lanes are the agents j > i.
// In-focal membership is explicit state, set by the host's two rules only (at creation, at a widening): at the high level the bound can
// go DOWN, and the host's focal set then keeps nodes the current bound would exclude.
// Every loop is bounded (node pools, the high-level budget, t_limit), nothing waits for another wave.  A mission that exceeds a device
// capacity ends with status 3 (RBP_ECBS_CAPACITY) and the wave takes the next one.
#include "rbp_dev.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "common/ecbs_rules.h"

namespace {

constexpr int ECBS_MAX_AGENTS = 256;
constexpr int ECBS_MAX_DIM = 1024;        // a cell is packed as x | y << 10 | z << 20
constexpr int ECBS_MAX_SEGMENTS = 4096;   // rbp_ecbs_out.max_M
constexpr int ECBS_MAX_HL_BUDGET = RBP_ECBS_MAX_HIGH_LEVEL_NODES;   // max_high_level_nodes: B budgeted expansions need 2 B + 1 node slots
constexpr int ECBS_LL_NODES = 32768;      // low-level node pool of a wave slot
constexpr size_t ECBS_MAX_SEEN_BYTES = size_t(16) << 20;  // seen bitmap of a wave slot
constexpr size_t ECBS_LDS_BYTES = 64 << 10;               // the current node's paths stay in LDS while the workgroup's whole LDS fits this (without them: <= 43 KB)
constexpr int ECBS_WAVES_PER_CU = 4;
constexpr unsigned NOT_FOCAL = 0x80000000u;
constexpr int HL_WORDS = 8;  // per high-level node: total, conflicts, agent, parent, constraint (t << 1 | edge), from cell, to cell, path length
enum { HL_TOTAL = 0, HL_CONFLICTS = 1, HL_AGENT = 2, HL_PARENT = 3, HL_CONS_TK = 4, HL_CONS_A = 5, HL_CONS_B = 6, HL_LEN = 7 };

struct EcbsDev {
    int K, N, dim[3], ncell;
    int seen_words, layers;   // words of a time layer of the seen bitmap, layers of a slot
    int lcap, stride;         // longest path cost a node may hold (max_M - 2); cells per path slot (odd: LDS banks)
    int hl_budget, hl_nodes;
    int sol_in_lds;
    float w;
    double grid;
    const unsigned char* masks;  // [K][ncell]
    const unsigned* outside;     // [K] or nullptr: a lattice sample lay outside the world's grid
    const int* start;            // [K][N][3] cells (may lie outside the lattice)
    const int* goal;
    const double* radius;        // [K][N]
    unsigned* counter;
    // workspace, one slice per wave slot
    uint4* ll_nodes;     // [ECBS_LL_NODES] cell, t << 16 | f, focal, parent
    unsigned* ll_open;   // [3][ECBS_LL_NODES] f << 16 | 65535 - g; focal | NOT_FOCAL; id
    unsigned* seen;      // [layers][seen_words]
    int* hl_meta;        // [hl_nodes][HL_WORDS]
    unsigned* hl_path;   // [hl_nodes][stride]
    unsigned* hl_open;   // [2][hl_nodes] id; 0 | NOT_FOCAL
    unsigned* root_path; // [N][stride]
    int* root_len;       // [N]
    unsigned* sol_global;  // [N][stride] when the paths do not fit the LDS
    // results
    int* status;         // [K]
    int* out_len;        // [K][N]
    unsigned* out_path;  // [K][N][stride]
    long long* out_count;  // [K][2] high-level, low-level expansions
};

struct Slot {  // what one wave works on
    uint4* nodes;
    unsigned *op_fg, *op_fo, *op_id, *seen;
    int* hl_meta;
    unsigned *hl_path, *hl_id, *hl_flag, *root_path;
    int* root_len;
    const unsigned char* mask;
    // LDS (sol: LDS or global)
    double* radius;
    unsigned *sol, *newpath, *savepath, *cons_tk, *cons_a, *cons_b;
    int *len, *owner;
};

__host__ __device__ __forceinline__ int cx(unsigned c) { return PackedCell{c}.x(); }
__host__ __device__ __forceinline__ int cy(unsigned c) { return PackedCell{c}.y(); }
__host__ __device__ __forceinline__ int cz(unsigned c) { return PackedCell{c}.z(); }
__device__ __forceinline__ unsigned pack_cell(int x, int y, int z) { return (unsigned)x | ((unsigned)y << 10) | ((unsigned)z << 20); }

__device__ __forceinline__ int wave_min(int v) {
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the minimum of (key, id) over the wave, with the position that came with it
__device__ __forceinline__ void wave_argmin(unsigned long long& key, unsigned& id, unsigned& pos) {
    for (int o = 32; o; o >>= 1) {
        const unsigned long long k2 = __shfl_xor(key, o);
        const unsigned i2 = __shfl_xor(id, o), p2 = __shfl_xor(pos, o);
        if (k2 < key || (k2 == key && i2 < id)) key = k2, id = i2, pos = p2;
    }
}

__device__ __forceinline__ bool vertex_conflict(double rr, double grid, unsigned a, unsigned b) {
    return ecbs_rules::vertex_conflict(rr, grid, PackedCell{a}, PackedCell{b});
}
__device__ __forceinline__ bool edge_conflict(double rr, double grid, unsigned a1, unsigned b1, unsigned a2, unsigned b2) {
    return ecbs_rules::edge_conflict(rr, grid, PackedCell{a1}, PackedCell{b1}, PackedCell{a2}, PackedCell{b2});
}

// state of agent i at time t: path[min(t, size - 1)]
__device__ __forceinline__ unsigned at(const Slot& s, int stride, int i, int len, int t) { return s.sol[i * stride + min(t, len - 1)]; }

// ecbs.cpp low_level.  Returns 1 with the path in s.newpath (out_len cells), 0 when the search fails, -1 when a device capacity is exceeded.
__device__ int low_level(const EcbsDev& d, const Slot& s, int lane, int agent, unsigned start, unsigned goal, int ncons, int lgc,
                         long long& expanded, int& out_len) {
    const int t_limit = 8 * (d.dim[0] + d.dim[1] + d.dim[2]) + 64 + lgc;
    const int gx = cx(goal), gy = cy(goal), gz = cz(goal);
    const int N = d.N, stride = d.stride, W = d.seen_words;
    const double ra = s.radius[agent], grid = d.grid;
    const float w = d.w;
    int n_nodes = 1, open_n = 1, max_layer = 0, rc = 0;
    const int f0 = abs(cx(start) - gx) + abs(cy(start) - gy) + abs(cz(start) - gz);
    if (lane == 0) {
        s.nodes[0] = make_uint4(start, (unsigned)f0, 0u, 0xffffffffu);
        s.op_fg[0] = ((unsigned)f0 << 16) | 65535u, s.op_fo[0] = 0u, s.op_id[0] = 0u;
        const int c = (cx(start) * d.dim[1] + cy(start)) * d.dim[2] + cz(start);
        s.seen[c >> 5] |= 1u << (c & 31);
    }
    __syncthreads();
    int best_f = f0;
    // lane -> (neighbour, stripe of the constraints) for the validity test: Wait, -x, +x, +y, -y, +z, -z
    const int nb_a = lane / 9, nb_s = lane - 9 * nb_a;
    const int ddx = nb_a == 1 ? -1 : nb_a == 2 ? 1 : 0, ddy = nb_a == 3 ? 1 : nb_a == 4 ? -1 : 0, ddz = nb_a == 5 ? 1 : nb_a == 6 ? -1 : 0;
    while (open_n > 0) {
        const int old_best = best_f;
        int minf = 0x7fffffff;
        unsigned long long key = ~0ull;
        unsigned id = ~0u, pos = 0;
        for (int p = lane; p < open_n; p += 64) {
            const unsigned fg = s.op_fg[p], fo = s.op_fo[p], i2 = s.op_id[p];
            minf = min(minf, (int)(fg >> 16));
            const unsigned long long k2 = ((unsigned long long)fo << 32) | fg;
            if (k2 < key || (k2 == key && i2 < id)) key = k2, id = i2, pos = (unsigned)p;
        }
        best_f = wave_min(minf);
        if (best_f > old_best) {  // a_star_epsilon.hpp:134-153: widen focal to the new bound
            key = ~0ull, id = ~0u, pos = 0;
            for (int p = lane; p < open_n; p += 64) {
                const unsigned fg = s.op_fg[p], i2 = s.op_id[p];
                unsigned fo = s.op_fo[p];
                const int f = (int)(fg >> 16);
                if ((fo & NOT_FOCAL) && !(f > best_f * w) && f > old_best * w) s.op_fo[p] = fo = fo & ~NOT_FOCAL;
                const unsigned long long k2 = ((unsigned long long)fo << 32) | fg;
                if (k2 < key || (k2 == key && i2 < id)) key = k2, id = i2, pos = (unsigned)p;
            }
        }
        wave_argmin(key, id, pos);
        if (key >> 63) break;  // nothing in focal (w < 1): the host has no answer here either
        const int cur = (int)id;
        const uint4 n = s.nodes[cur];
        const int nt = (int)(n.y >> 16), nfocal = (int)n.z;
        const int nx = cx(n.x), ny = cy(n.x), nz = cz(n.x);
        ++expanded;
        if (n.x == goal && nt > lgc) {
            if (nt > d.lcap) {
                rc = -1;
                break;
            }
            if (lane == 0) {
                int q = cur;
                for (int p = nt; p >= 0; --p) {
                    const uint4 m = s.nodes[q];
                    s.newpath[p] = m.x;
                    q = (int)m.w;
                }
            }
            out_len = nt + 1;
            rc = 1;
            break;
        }
        if (lane == 0) {  // erase: the last entry takes the popped one's place (any order does under a total order)
            const int last = open_n - 1;
            s.op_fg[pos] = s.op_fg[last], s.op_fo[pos] = s.op_fo[last], s.op_id[pos] = s.op_id[last];
        }
        --open_n;
        if (nt < t_limit) {
            const int t = nt + 1;
            if (t >= d.layers) {
                rc = -1;
                break;
            }
            // which of the 7 neighbours are free, unconstrained and not seen
            const int x = nx + ddx, y = ny + ddy, z = nz + ddz;
            bool bad = false;
            int cell_index = 0;
            if (nb_a < 7) {
                const bool inside = x >= 0 && y >= 0 && z >= 0 && x < d.dim[0] && y < d.dim[1] && z < d.dim[2];
                if (!inside) bad = true;
                else {
                    cell_index = (x * d.dim[1] + y) * d.dim[2] + z;
                    const unsigned nb = pack_cell(x, y, z);
                    if (nb_s == 0) bad = s.mask[cell_index] != 0 || ((s.seen[(size_t)t * W + (cell_index >> 5)] >> (cell_index & 31)) & 1u);
                    for (int c = nb_s; c < ncons; c += 9) {
                        const unsigned tk = s.cons_tk[c];
                        if (tk & 1u) bad = bad || (tk == (((unsigned)nt << 1) | 1u) && s.cons_a[c] == n.x && s.cons_b[c] == nb);
                        else bad = bad || (tk == ((unsigned)t << 1) && s.cons_a[c] == nb);
                    }
                }
            }
            const unsigned long long badmask = __ballot(bad);
            max_layer = max(max_layer, t);
            for (int a = 0; a < 7; ++a) {
                if ((badmask >> (9 * a)) & 0x1ffull) continue;
                const int ax = nx + (a == 1 ? -1 : a == 2 ? 1 : 0), ay = ny + (a == 3 ? 1 : a == 4 ? -1 : 0), az = nz + (a == 5 ? 1 : a == 6 ? -1 : 0);
                const unsigned nb = pack_cell(ax, ay, az);
                const int f2 = t + abs(ax - gx) + abs(ay - gy) + abs(az - gz);
                int foc = nfocal;
                for (int base = 0; base < N; base += 64) {  // focal_state + focal_trans (environment.hpp:392-422): lanes are the other agents
                    const int i = base + lane;
                    bool v = false, e = false;
                    if (i < N && i != agent) {
                        const int li = s.len[i];
                        if (li > 0) {
                            const double rr = ra + s.radius[i];
                            const unsigned o1 = at(s, stride, i, li, t);
                            v = vertex_conflict(rr, grid, nb, o1);
                            e = edge_conflict(rr, grid, n.x, nb, at(s, stride, i, li, nt), o1);
                        }
                    }
                    foc += __popcll(__ballot(v)) + __popcll(__ballot(e));
                }
                if (n_nodes >= ECBS_LL_NODES) {
                    rc = -1;
                    break;
                }
                if (lane == 0) {
                    s.nodes[n_nodes] = make_uint4(nb, ((unsigned)t << 16) | (unsigned)f2, (unsigned)foc, (unsigned)cur);
                    s.op_fg[open_n] = ((unsigned)f2 << 16) | (65535u - (unsigned)t);
                    s.op_fo[open_n] = (unsigned)foc | (f2 <= best_f * w ? 0u : NOT_FOCAL);
                    s.op_id[open_n] = (unsigned)n_nodes;
                    const int c = (ax * d.dim[1] + ay) * d.dim[2] + az;
                    s.seen[(size_t)t * W + (c >> 5)] |= 1u << (c & 31);
                }
                ++n_nodes, ++open_n;
            }
            if (rc < 0) break;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = lane; i < (max_layer + 1) * W; i += 64) s.seen[i] = 0u;  // only the time layers this search touched
    __syncthreads();
    return rc;
}

// ecbs.cpp count_conflicts (environment.hpp:425-460): per time step and agent i, lanes are the agents j > i
__device__ int count_conflicts(const EcbsDev& d, const Slot& s, int lane, int max_t) {
    const int N = d.N, stride = d.stride;
    int n = 0;
    for (int t = 0; t < max_t; ++t)
        for (int i = 0; i + 1 < N; ++i) {
            const int li = s.len[i];
            const unsigned a1 = at(s, stride, i, li, t), b1 = at(s, stride, i, li, t + 1);
            const double ri = s.radius[i];
            for (int j = i + 1 + lane; j < N; j += 64) {
                const int lj = s.len[j];
                const double rr = ri + s.radius[j];
                const unsigned a2 = at(s, stride, j, lj, t), b2 = at(s, stride, j, lj, t + 1);
                n += (int)vertex_conflict(rr, d.grid, a1, a2) + (int)edge_conflict(rr, d.grid, a1, b1, a2, b2);
            }
        }
    return wave_sum(n);
}

// ecbs.cpp first_conflict (environment.hpp:526-589): the first in the order t, vertex before edge, i, j
__device__ bool first_conflict(const EcbsDev& d, const Slot& s, int lane, int max_t, int& kind, int& ct, int& ci, int& cj) {
    const int N = d.N, stride = d.stride;
    for (int t = 0; t < max_t; ++t)
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i + 1 < N; ++i) {
                const int li = s.len[i];
                const unsigned a1 = at(s, stride, i, li, t), b1 = at(s, stride, i, li, t + 1);
                const double ri = s.radius[i];
                for (int base = i + 1; base < N; base += 64) {
                    const int j = base + lane;
                    bool hit = false;
                    if (j < N) {
                        const int lj = s.len[j];
                        const double rr = ri + s.radius[j];
                        const unsigned a2 = at(s, stride, j, lj, t);
                        hit = k == 0 ? vertex_conflict(rr, d.grid, a1, a2) : edge_conflict(rr, d.grid, a1, b1, a2, at(s, stride, j, lj, t + 1));
                    }
                    const unsigned long long m = __ballot(hit);
                    if (m) {
                        kind = k, ct = t, ci = i, cj = base + (int)__ffsll((long long)m) - 1;
                        return true;
                    }
                }
            }
    return false;
}

__device__ __forceinline__ int solution_max_t(const EcbsDev& d, const Slot& s, int lane) {
    int m = 0;
    for (int i = lane; i < d.N; i += 64) m = max(m, s.len[i] - 1);
    return wave_max(m);
}

// the solution of high-level node P into s.sol / s.len: every agent's path from the nearest ancestor that replanned it, else the root's
__device__ void load_solution(const EcbsDev& d, const Slot& s, int lane, int P) {
    const int N = d.N, stride = d.stride;
    for (int i = lane; i < N; i += 64) s.owner[i] = 0;
    __syncthreads();
    if (lane == 0)
        for (int c = P; c > 0; c = s.hl_meta[c * HL_WORDS + HL_PARENT]) {
            const int ag = s.hl_meta[c * HL_WORDS + HL_AGENT];
            if (s.owner[ag] == 0) s.owner[ag] = c;
        }
    __syncthreads();
    for (int i = lane; i < N; i += 64) s.len[i] = s.owner[i] ? s.hl_meta[s.owner[i] * HL_WORDS + HL_LEN] : s.root_len[i];
    for (int e = lane; e < N * stride; e += 64) {
        const int i = e / stride, p = e - i * stride, o = s.owner[i];
        s.sol[e] = o ? s.hl_path[(size_t)o * stride + p] : s.root_path[e];
    }
    __syncthreads();
}

// ecbs.cpp rbp_ecbs_plan_obstacles on mission k; returns its status
__device__ int plan_mission(const EcbsDev& d, const Slot& s, int lane, int k, long long& hl_expanded, long long& ll_expanded) {
    const int N = d.N, stride = d.stride;
    const float w = d.w;
    if (d.outside && d.outside[k]) return 1;
    // ecbs_planner.hpp:112-136: start / goal cells, occluded ones end the mission
    bool occluded = false;
    for (int i = lane; i < N; i += 64) {
        s.radius[i] = d.radius[(size_t)k * N + i];
        s.len[i] = 0;
        for (int e = 0; e < 2; ++e) {
            const int* c = (e ? d.goal : d.start) + ((size_t)k * N + i) * 3;
            const bool inside = c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] < d.dim[0] && c[1] < d.dim[1] && c[2] < d.dim[2];
            occluded = occluded || !inside || s.mask[((size_t)c[0] * d.dim[1] + c[1]) * d.dim[2] + c[2]] != 0;
        }
    }
    if (__any(occluded)) return 1;
    __syncthreads();
    auto cell_of = [&](const int* base, int i) {
        const int* c = base + ((size_t)k * N + i) * 3;
        return pack_cell(c[0], c[1], c[2]);
    };

    // the root: every agent in turn, against the agents planned so far
    int root_total = 0, len = 0;
    for (int i = 0; i < N; ++i) {
        const int rc = low_level(d, s, lane, i, cell_of(d.start, i), cell_of(d.goal, i), 0, -1, ll_expanded, len);
        if (rc <= 0) return rc < 0 ? 3 : 2;
        for (int p = lane; p < len; p += 64) s.sol[i * stride + p] = s.root_path[i * stride + p] = s.newpath[p];
        if (lane == 0) s.len[i] = s.root_len[i] = len;
        root_total += len - 1;
        __syncthreads();
    }
    const int root_conflicts = count_conflicts(d, s, lane, solution_max_t(d, s, lane));
    if (lane == 0) {
        int* m = s.hl_meta;
        m[HL_TOTAL] = root_total, m[HL_CONFLICTS] = root_conflicts, m[HL_AGENT] = -1, m[HL_PARENT] = -1;
        s.hl_id[0] = 0u, s.hl_flag[0] = 0u;
    }
    __syncthreads();

    int open_n = 1, next_id = 1, best_cost = root_total;
    while (open_n > 0) {
        const int old_best = best_cost;
        int minc = 0x7fffffff;
        unsigned long long key = ~0ull;
        unsigned id = ~0u, pos = 0;
        for (int pass = 0; pass < 2; ++pass) {  // the second pass only after a widening (ecbs.hpp:171-191)
            key = ~0ull, id = ~0u, pos = 0;
            for (int p = lane; p < open_n; p += 64) {
                const unsigned i2 = s.hl_id[p];
                unsigned fl = s.hl_flag[p];
                const int total = s.hl_meta[i2 * HL_WORDS + HL_TOTAL];
                minc = min(minc, total);
                if (pass && fl && !(total > best_cost * w) && total > old_best * w) s.hl_flag[p] = fl = 0u;
                const unsigned long long k2 = ((unsigned long long)(fl | (unsigned)s.hl_meta[i2 * HL_WORDS + HL_CONFLICTS]) << 32) | (unsigned)total;
                if (k2 < key || (k2 == key && i2 < id)) key = k2, id = i2, pos = (unsigned)p;
            }
            if (pass == 0) best_cost = wave_min(minc);
            if (!(best_cost > old_best)) break;
        }
        wave_argmin(key, id, pos);
        if (key >> 63) return 2;  // nothing in focal (w < 1)
        const int P = (int)id;
        if (lane == 0) s.hl_id[pos] = s.hl_id[open_n - 1], s.hl_flag[pos] = s.hl_flag[open_n - 1];
        --open_n;
        ++hl_expanded;
        load_solution(d, s, lane, P);
        int kind, ct, ci, cj;
        if (!first_conflict(d, s, lane, solution_max_t(d, s, lane), kind, ct, ci, cj)) return 0;  // the goal node: its solution is in s.sol
        if (hl_expanded > d.hl_budget) return 2;
        const int p_total = s.hl_meta[P * HL_WORDS + HL_TOTAL];
        for (int side = 0; side < 2; ++side) {
            const int ag = side == 0 ? ci : cj;
            const int child = next_id++;
            if (child >= d.hl_nodes) return 3;
            const int lag = s.len[ag];
            const unsigned ca = at(s, stride, ag, lag, ct), cb = kind ? at(s, stride, ag, lag, ct + 1) : ca;
            const unsigned goal = cell_of(d.goal, ag);
            // the agent's constraints: the new one (environment.hpp:593-609) and its ancestors', into LDS
            if (lane == 0) {
                int* m = s.hl_meta + child * HL_WORDS;
                m[HL_AGENT] = ag, m[HL_PARENT] = P, m[HL_CONS_TK] = (ct << 1) | kind, m[HL_CONS_A] = (int)ca, m[HL_CONS_B] = (int)cb;
                int nc = 0, lgc = -1;  // environment.hpp:373-383: the last vertex constraint on the goal cell
                for (int c = child; c > 0; c = s.hl_meta[c * HL_WORDS + HL_PARENT]) {
                    const int* q = s.hl_meta + c * HL_WORDS;
                    if (q[HL_AGENT] != ag) continue;
                    s.cons_tk[nc] = (unsigned)q[HL_CONS_TK], s.cons_a[nc] = (unsigned)q[HL_CONS_A], s.cons_b[nc] = (unsigned)q[HL_CONS_B];
                    if (!(q[HL_CONS_TK] & 1) && (unsigned)q[HL_CONS_A] == goal) lgc = max(lgc, q[HL_CONS_TK] >> 1);
                    ++nc;
                }
                s.owner[0] = nc, s.owner[1] = lgc;
            }
            __syncthreads();
            const int ncons = s.owner[0], lgc = s.owner[1];
            __syncthreads();
            const int rc = low_level(d, s, lane, ag, cell_of(d.start, ag), goal, ncons, lgc, ll_expanded, len);
            if (rc < 0) return 3;
            if (rc == 0) continue;  // (the id stays taken, as the host's `all` keeps a null entry)
            // the child's solution for its conflict count: the new path in place of the parent's, which comes back for the other side
            for (int p = lane; p < stride; p += 64) {
                s.savepath[p] = s.sol[ag * stride + p];
                if (p < len) s.sol[ag * stride + p] = s.hl_path[(size_t)child * stride + p] = s.newpath[p];
            }
            if (lane == 0) s.len[ag] = len;
            __syncthreads();
            const int total = p_total - (lag - 1) + (len - 1);
            const int conflicts = count_conflicts(d, s, lane, solution_max_t(d, s, lane));
            __syncthreads();
            for (int p = lane; p < stride; p += 64) s.sol[ag * stride + p] = s.savepath[p];
            if (lane == 0) {
                s.len[ag] = lag;
                int* m = s.hl_meta + child * HL_WORDS;
                m[HL_TOTAL] = total, m[HL_CONFLICTS] = conflicts, m[HL_LEN] = len;
                s.hl_id[open_n] = (unsigned)child, s.hl_flag[open_n] = total <= best_cost * w ? 0u : NOT_FOCAL;
            }
            ++open_n;
            __syncthreads();
        }
    }
    return 2;
}

__global__ __launch_bounds__(64) void ecbs_kernel(EcbsDev d) {
    extern __shared__ double ecbs_lds[];
    __shared__ int next_mission;
    const int lane = threadIdx.x, N = d.N, stride = d.stride, slot = blockIdx.x;
    Slot s;
    s.nodes = d.ll_nodes + (size_t)slot * ECBS_LL_NODES;
    s.op_fg = d.ll_open + (size_t)slot * 3 * ECBS_LL_NODES, s.op_fo = s.op_fg + ECBS_LL_NODES, s.op_id = s.op_fo + ECBS_LL_NODES;
    s.seen = d.seen + (size_t)slot * d.layers * d.seen_words;
    s.hl_meta = d.hl_meta + (size_t)slot * d.hl_nodes * HL_WORDS;
    s.hl_path = d.hl_path + (size_t)slot * d.hl_nodes * stride;
    s.hl_id = d.hl_open + (size_t)slot * 2 * d.hl_nodes, s.hl_flag = s.hl_id + d.hl_nodes;
    s.root_path = d.root_path + (size_t)slot * N * stride;
    s.root_len = d.root_len + (size_t)slot * N;
    s.radius = ecbs_lds;
    unsigned* u = reinterpret_cast<unsigned*>(ecbs_lds + N);
    s.newpath = u, u += stride;
    s.savepath = u, u += stride;
    s.cons_tk = u, u += ECBS_MAX_HL_BUDGET;
    s.cons_a = u, u += ECBS_MAX_HL_BUDGET;
    s.cons_b = u, u += ECBS_MAX_HL_BUDGET;
    s.len = reinterpret_cast<int*>(u), u += N;
    s.owner = reinterpret_cast<int*>(u), u += max(N, 2);
    s.sol = d.sol_in_lds ? u : d.sol_global + (size_t)slot * N * stride;
    for (;;) {
        __syncthreads();
        if (lane == 0) next_mission = (int)atomicAdd(d.counter, 1u);
        __syncthreads();
        const int k = next_mission;
        if (k >= d.K) break;
        s.mask = d.masks + (size_t)k * d.ncell;
        long long hl = 0, ll = 0;
        const int status = plan_mission(d, s, lane, k, hl, ll);
        __syncthreads();
        if (status == 0) {
            for (int i = lane; i < N; i += 64) d.out_len[(size_t)k * N + i] = s.len[i];
            for (int e = lane; e < N * stride; e += 64) d.out_path[(size_t)k * N * stride + e] = s.sol[e];
        }
        if (lane == 0) d.status[k] = status, d.out_count[2 * k] = hl, d.out_count[2 * k + 1] = ll;
    }
}

size_t ecbs_lds_bytes(int N, int stride, bool sol_in_lds) {
    return sizeof(double) * N + sizeof(unsigned) * (2 * (size_t)stride + 3 * ECBS_MAX_HL_BUDGET + N + std::max(N, 2) + (sol_in_lds ? (size_t)N * stride : 0));
}

int seen_layers(const int dim[3], int max_M) { return 8 * (dim[0] + dim[1] + dim[2]) + 64 + (max_M - 2) + 2; }

}  // namespace

int ecbs_check_arguments(const char* who, int32_t K, const int32_t* dim_in, const rbp_mission* missions, const rbp_param* param,
                         int64_t max_high_level_nodes, const rbp_ecbs_out* out, int32_t dim[3]) {
    auto bad = [&](const char* what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": " + what).c_str()); };
    if (K <= 0 || !missions || !param || !out) return bad("need K > 0, missions, param and out");
    if (!out->status || !out->M || !out->makespan || !out->sum_cost || !out->high_level_expanded || !out->low_level_expanded || !out->T || !out->init_traj)
        return bad("every array of rbp_ecbs_out must be given");
    return ecbs_check_search(who, K, dim_in, missions, param, max_high_level_nodes, out->max_M, dim);
}

int ecbs_check_search(const char* who, int32_t K, const int32_t* dim_in, const rbp_mission* missions, const rbp_param* param,
                      int64_t max_high_level_nodes, int32_t max_M, int32_t dim[3]) {
    auto bad = [&](const char* what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": " + what).c_str()); };
    if (K <= 0 || !missions || !param) return bad("need K > 0, missions and param");
    if (max_M < 2 || max_M > ECBS_MAX_SEGMENTS) return bad("max_M must be 2..4096");
    if (max_high_level_nodes < 1 || max_high_level_nodes > ECBS_MAX_HL_BUDGET) return bad("max_high_level_nodes must be 1..512 on the device");
    const int N = missions[0].N;
    if (N < 1 || N > ECBS_MAX_AGENTS) return bad("N must be 1..256");
    for (int k = 0; k < K; ++k) {
        if (missions[k].N != N) return bad("all missions of a call share N");
        if (!missions[k].start || !missions[k].goal || !missions[k].radius) return bad("a mission needs start, goal and radius");
    }
    double gmin[3], gmax[3], gres[3];
    int d[3];
    if (!ecbs_rules::planning_lattice(param, ECBS_MAX_DIM, gmin, gmax, gres, d)) return bad("the planning lattice needs 1..1024 cells per axis");
    if (dim_in && (dim_in[0] != d[0] || dim_in[1] != d[1] || dim_in[2] != d[2])) return bad("dim is not the planning lattice of param");
    const size_t seen_bytes = (size_t)seen_layers(d, max_M) * (((size_t)d[0] * d[1] * d[2] + 31) / 32) * 4;
    if (seen_bytes > ECBS_MAX_SEEN_BYTES) return bad("lattice x time layers beyond the 16 MB seen bitmap of a wave");
    for (int a = 0; a < 3; ++a) dim[a] = d[a];
    return RBP_OK;
}

// The search on K masks of the current device, launched and not waited for.  The workspace of the wave slots and the kernel's inputs come
// from `work`, what the search leaves behind (status, out_len, out_path, out_count) from `results`; gmin / gres receive the lattice.
static int ecbs_launch(const char* who, int32_t K, const int32_t dim[3], const unsigned char* d_masks, const unsigned* d_outside, const rbp_mission* missions,
                       const rbp_param* param, int64_t max_high_level_nodes, int max_M, DeviceBuffers& work, DeviceBuffers& results, EcbsDev& d,
                       double gmin[3], double gres[3]) {
    const int N = missions[0].N;
    double gmax[3];
    int gd[3];
    ecbs_rules::planning_lattice(param, ECBS_MAX_DIM, gmin, gmax, gres, gd);
    // ecbs_planner.hpp:112-136: the cells of the start and goal positions (anything off the lattice is "occluded")
    std::vector<int> start((size_t)K * N * 3), goal(start.size());
    std::vector<double> radius((size_t)K * N);
    auto cell = [&](double v, int a) { return ecbs_rules::position_to_cell(v, gmin[a], gres[a], gd[a]); };
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < N; ++i) {
            radius[(size_t)k * N + i] = missions[k].radius[i];
            for (int a = 0; a < 3; ++a) {
                start[((size_t)k * N + i) * 3 + a] = cell(missions[k].start[9 * i + a], a);
                goal[((size_t)k * N + i) * 3 + a] = cell(missions[k].goal[9 * i + a], a);
            }
        }

    d = EcbsDev{};
    d.K = K, d.N = N, d.ncell = dim[0] * dim[1] * dim[2];
    for (int a = 0; a < 3; ++a) d.dim[a] = dim[a];
    d.seen_words = (d.ncell + 31) / 32, d.layers = seen_layers(gd, max_M);
    d.lcap = max_M - 2, d.stride = (d.lcap + 1) | 1;
    d.hl_budget = (int)max_high_level_nodes, d.hl_nodes = 2 * d.hl_budget + 1;
    d.sol_in_lds = ecbs_lds_bytes(N, d.stride, true) <= ECBS_LDS_BYTES;
    d.w = (float)param->ecbs_w;  // stored as float, ecbs.hpp:107
    d.grid = param->grid_xy_res;
    d.masks = d_masks, d.outside = d_outside;

    auto fail = [&](hipError_t e, const char* what) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + what + ": " + hipGetErrorString(e)).c_str()); };
    int device = 0, cus = 0;
    hipError_t e = hipGetDevice(&device);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return fail(e, "device query");
    const int slots = std::min<int>(K, std::max(cus, 1) * ECBS_WAVES_PER_CU);
    const size_t path_cells = (size_t)N * d.stride;
    DeviceBuffers& b = work;
    d.start = b.upload(start), d.goal = b.upload(goal), d.radius = b.upload(radius);
    d.counter = b.get<unsigned>(1, true);
    d.ll_nodes = b.get<uint4>((size_t)slots * ECBS_LL_NODES);
    d.ll_open = b.get<unsigned>((size_t)slots * 3 * ECBS_LL_NODES);
    d.seen = b.get<unsigned>((size_t)slots * d.layers * d.seen_words, true);
    d.hl_meta = b.get<int>((size_t)slots * d.hl_nodes * HL_WORDS);
    d.hl_path = b.get<unsigned>((size_t)slots * d.hl_nodes * d.stride, true);
    d.hl_open = b.get<unsigned>((size_t)slots * 2 * d.hl_nodes);
    d.root_path = b.get<unsigned>((size_t)slots * path_cells, true);
    d.root_len = b.get<int>((size_t)slots * N);
    d.sol_global = d.sol_in_lds ? nullptr : b.get<unsigned>((size_t)slots * path_cells, true);
    if (b.err != hipSuccess) return fail(b.err, "workspace");
    d.status = results.get<int>(K);
    d.out_len = results.get<int>((size_t)K * N, true);
    d.out_path = results.get<unsigned>((size_t)K * path_cells, true);
    d.out_count = results.get<long long>((size_t)K * 2);
    if (results.err != hipSuccess) return fail(results.err, "workspace");
    hipLaunchKernelGGL(ecbs_kernel, dim3(slots), dim3(64), ecbs_lds_bytes(N, d.stride, d.sol_in_lds), 0, d);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(e, "launch");
    return RBP_OK;
}

int ecbs_plan_on_device(const char* who, int32_t K, const int32_t dim[3], const unsigned char* d_masks, const unsigned* d_outside,
                        const rbp_mission* missions, const rbp_param* param, int64_t max_high_level_nodes, rbp_ecbs_out* out) {
    const int N = missions[0].N, max_M = out->max_M;
    // every mission starts as "no result"
    const size_t t_stride = (size_t)max_M + 1, traj_stride = (size_t)N * t_stride * 3;
    for (int k = 0; k < K; ++k) out->status[k] = out->M[k] = out->makespan[k] = out->sum_cost[k] = 0, out->high_level_expanded[k] = out->low_level_expanded[k] = 0;
    memset(out->T, 0, sizeof(double) * K * t_stride);
    memset(out->init_traj, 0, sizeof(float) * K * traj_stride);

    EcbsDev d{};
    double gmin[3], gres[3];
    DeviceBuffers b;
    if (int rc = ecbs_launch(who, K, dim, d_masks, d_outside, missions, param, max_high_level_nodes, max_M, b, b, d, gmin, gres)) return rc;
    auto fail = [&](hipError_t e, const char* what) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + what + ": " + hipGetErrorString(e)).c_str()); };
    const size_t path_cells = (size_t)N * d.stride;
    std::vector<int> status(K), len((size_t)K * N);
    std::vector<unsigned> path((size_t)K * path_cells);
    std::vector<long long> count((size_t)K * 2);
    hipError_t e = hipMemcpy(status.data(), d.status, sizeof(int) * K, hipMemcpyDeviceToHost);  // (synchronises with the kernel)
    if (e == hipSuccess) e = hipMemcpy(len.data(), d.out_len, sizeof(int) * len.size(), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(path.data(), d.out_path, sizeof(unsigned) * path.size(), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(count.data(), d.out_count, sizeof(long long) * count.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(e, "results");

    for (int k = 0; k < K; ++k) {
        out->status[k] = status[k];
        if (status[k]) continue;
        auto len_of = [&](int a) { return len[(size_t)k * N + a]; };
        out->M[k] = ecbs_rules::plan_segments(N, len_of, &out->makespan[k], &out->sum_cost[k]);  // <= max_M: no path is longer than max_M - 2
        out->high_level_expanded[k] = count[2 * (size_t)k], out->low_level_expanded[k] = count[2 * (size_t)k + 1];
        ecbs_rules::write_plan(out->M[k], N, len_of, [&](int a, int p) { return PackedCell{path[((size_t)k * N + a) * d.stride + p]}; }, missions[k].start,
                               missions[k].goal, gmin, gres, param->time_step, t_stride, out->T + k * t_stride, out->init_traj + k * traj_stride);
    }
    return RBP_OK;
}

// The same search with its paths left on the device: only status, path lengths and counters come back, K x (N + 3) words, and the
// missions' states and limits go up once as packed arrays, for the kernels of kernels/handoff.hip to read beside the paths.
int ecbs_search_on_device(const char* who, int32_t K, const int32_t dim[3], const unsigned char* d_masks, const unsigned* d_outside,
                          const rbp_mission* missions, const rbp_param* param, int64_t max_high_level_nodes, int32_t max_M, rbp_dev_ecbs* h) {
    const int N = missions[0].N;
    EcbsDev d{};
    DeviceBuffers work;
    if (int rc = ecbs_launch(who, K, dim, d_masks, d_outside, missions, param, max_high_level_nodes, max_M, work, h->results, d, h->gmin, h->gres)) return rc;
    auto fail = [&](hipError_t e, const char* what) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + what + ": " + hipGetErrorString(e)).c_str()); };
    (void)hipGetDevice(&h->device);
    h->K = K, h->N = N, h->max_M = max_M, h->path_stride = d.stride, h->time_step = param->time_step;
    h->status = d.status, h->out_len = d.out_len, h->out_path = d.out_path, h->out_count = d.out_count;
    h->have_limits = true;
    for (int k = 0; k < K; ++k) h->have_limits = h->have_limits && missions[k].max_vel && missions[k].max_acc;
    // [K][N][9] start, [K][N][9] goal, [K][N] radius, [K][N][3] max_vel, [K][N][3] max_acc in one upload (limits that were not given stay zero)
    const size_t kn = (size_t)K * N;
    std::vector<double> packed(kn * 25, 0.0);
    double *ps = packed.data(), *pg = ps + kn * 9, *pr = pg + kn * 9, *pv = pr + kn, *pa = pv + kn * 3;
    for (int k = 0; k < K; ++k) {
        const size_t o = (size_t)k * N;
        memcpy(ps + o * 9, missions[k].start, sizeof(double) * N * 9), memcpy(pg + o * 9, missions[k].goal, sizeof(double) * N * 9);
        memcpy(pr + o, missions[k].radius, sizeof(double) * N);
        if (h->have_limits) memcpy(pv + o * 3, missions[k].max_vel, sizeof(double) * N * 3), memcpy(pa + o * 3, missions[k].max_acc, sizeof(double) * N * 3);
    }
    const double* dp = h->results.upload(packed);
    if (h->results.err != hipSuccess) return fail(h->results.err, "missions");
    h->start = dp, h->goal = dp + kn * 9, h->radius = dp + kn * 18, h->max_vel = dp + kn * 19, h->max_acc = dp + kn * 22;

    h->status_h.assign(K, 0), h->len_h.assign(kn, 0), h->count_h.assign((size_t)K * 2, 0);
    hipError_t e = hipMemcpy(h->status_h.data(), d.status, sizeof(int) * K, hipMemcpyDeviceToHost);  // (synchronises with the kernel)
    if (e == hipSuccess) e = hipMemcpy(h->len_h.data(), d.out_len, sizeof(int) * kn, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h->count_h.data(), d.out_count, sizeof(long long) * K * 2, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(e, "results");
    h->M_h.assign(K, 0), h->makespan_h.assign(K, 0), h->sum_cost_h.assign(K, 0);
    for (int k = 0; k < K; ++k) {
        if (h->status_h[k]) continue;
        auto len_of = [&](int a) { return h->len_h[(size_t)k * N + a]; };
        h->M_h[k] = ecbs_rules::plan_segments(N, len_of, &h->makespan_h[k], &h->sum_cost_h[k]);  // <= max_M: no path is longer than max_M - 2
    }
    return RBP_OK;
}

extern "C" int rbp_dev_ecbs_plan_masks(int device, int32_t K, const int32_t dim_in[3], const uint8_t* const* obstacle, const rbp_mission* missions,
                                       const rbp_param* param, int64_t max_high_level_nodes, rbp_ecbs_out* out) {
    const char* who = "rbp_dev_ecbs_plan_masks";
    if (!dim_in || !obstacle) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "rbp_dev_ecbs_plan_masks: need dim and the masks");
    int32_t dim[3];
    if (int rc = ecbs_check_arguments(who, K, dim_in, missions, param, max_high_level_nodes, out, dim)) return rc;
    for (int k = 0; k < K; ++k)
        if (!obstacle[k]) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "rbp_dev_ecbs_plan_masks: a mask is null");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rbp_set_error(RBP_ERR_NO_DEVICE, "no HIP device: the device search has no CPU fallback");
    if (device < 0) (void)hipGetDevice(&device);
    if (device < 0 || device >= ndev) return rbp_set_error(RBP_ERR_NO_DEVICE, "device index out of range");
    DeviceScope scope(device);
    const size_t ncell = (size_t)dim[0] * dim[1] * dim[2];
    std::vector<unsigned char> masks((size_t)K * ncell);
    for (int k = 0; k < K; ++k) memcpy(masks.data() + k * ncell, obstacle[k], ncell);
    unsigned char* d_masks = nullptr;
    hipError_t e = hipMalloc((void**)&d_masks, masks.size());
    if (e == hipSuccess) e = hipMemcpy(d_masks, masks.data(), masks.size(), hipMemcpyHostToDevice);
    const int rc = e == hipSuccess ? ecbs_plan_on_device(who, K, dim, d_masks, nullptr, missions, param, max_high_level_nodes, out)
                                   : rbp_set_error(RBP_ERR_HIP, (std::string("rbp_dev_ecbs_plan_masks: masks: ") + hipGetErrorString(e)).c_str());
    (void)hipFree(d_masks);
    return rc;
}

// ---- rbp_dev_ecbs: what a search left on the device (the search itself: rbp_dev_worlds_ecbs_search, kernels/edt.hip) ----------------------
extern "C" int rbp_dev_ecbs_count(const rbp_dev_ecbs* e) { return e ? e->K : 0; }

extern "C" void rbp_dev_ecbs_destroy(rbp_dev_ecbs* e) {
    if (!e) return;
    DeviceScope scope(e->device);
    delete e;  // (frees `results` on the handle's device)
}

extern "C" int rbp_dev_ecbs_download(const rbp_dev_ecbs* e, rbp_ecbs_out* out) {
    const char* who = "rbp_dev_ecbs_download";
    auto bad = [&](const char* what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": " + what).c_str()); };
    if (!e || !out) return bad("need the handle and out");
    if (!out->status || !out->M || !out->makespan || !out->sum_cost || !out->high_level_expanded || !out->low_level_expanded)
        return bad("every per-mission array of rbp_ecbs_out must be given (T and init_traj may be null)");
    if (out->max_M != e->max_M) return bad("out->max_M is not the max_M of the search");
    const int K = e->K, N = e->N;
    std::vector<int> Mj(K), src(K);
    for (int k = 0; k < K; ++k) {
        const bool ok = e->status_h[k] == 0;
        out->status[k] = e->status_h[k], out->M[k] = e->M_h[k], out->makespan[k] = e->makespan_h[k], out->sum_cost[k] = e->sum_cost_h[k];
        out->high_level_expanded[k] = ok ? e->count_h[2 * (size_t)k] : 0, out->low_level_expanded[k] = ok ? e->count_h[2 * (size_t)k + 1] : 0;
        Mj[k] = ok ? e->M_h[k] : -1, src[k] = k;
    }
    if (!out->T && !out->init_traj) return RBP_OK;
    auto fail = [&](hipError_t err) { return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(err)).c_str()); };
    DeviceScope scope(e->device);
    const size_t stride = (size_t)e->max_M + 1, nT = (size_t)K * stride, ntr = (size_t)K * N * stride * 3;
    DeviceBuffers b;
    const int *d_M = b.upload(Mj), *d_src = b.upload(src);
    double* d_T = b.get<double>(nT);
    float* d_tr = b.get<float>(ntr);
    if (b.err != hipSuccess) return fail(b.err);
    if (int rc = launch_ecbs_plan_write(*e, K, d_src, d_M, (int)stride, false, d_T, d_tr, 0)) return rc;
    hipError_t err = hipSuccess;
    if (out->T) err = hipMemcpy(out->T, d_T, sizeof(double) * nT, hipMemcpyDeviceToHost);  // (synchronises with the kernel)
    if (err == hipSuccess && out->init_traj) err = hipMemcpy(out->init_traj, d_tr, sizeof(float) * ntr, hipMemcpyDeviceToHost);
    return err == hipSuccess ? RBP_OK : fail(err);
}
