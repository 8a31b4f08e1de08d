// edt.hip — the distance grid of a world on gfx950 ("GPU EDT, later").
//
// Replaces, for the Corridor stage's input,
//     DynamicEDTOctomap distmap(maxDist, tree, world_min, world_max, false); distmap.update();
// (reference: swarm_planner/src/swarm_traj_planner_rbp_test_all.cpp:57-63, src/swarm_traj_planner_rbp.cpp:73-80) followed by
// getDistance() on every voxel centre of the bounding box, i.e. the float grid rbp_world describes.  The host library has the
// same function on the CPU (csrc/host/octomap_edt.cpp, rbp_world_build); the two are bit-identical (tests/test_gpu_edt.py).
//
// dynamicEDT3D clamps: maxDist_squared = ((int)(maxDist / res + 1))^2 cells, every voxel at or beyond keeps sqrt(maxDist_squared).
// So only obstacles closer than md = (int)(maxDist / res + 1) cells along EVERY axis can matter, and the exact squared Euclidean
// distance transform separates into three min-plus passes with a window of 2 md - 1 cells:
//     d2(x,y,z) = min_x' (x-x')^2 + [ min_y' (y-y')^2 + [ min_z' (z-z')^2 + occ(x',y',z') ] ]      (occ = 0 on obstacles, "infinity" elsewhere)
// in int32 (values <= 3 md^2): exact, no lower-envelope bookkeeping, one thread per voxel and pass, z fastest so the x and y passes
// read coalesced.  Wherever the true d2 is < md^2 the windowed minimum equals it (each component of the minimiser is < md); elsewhere
// both are >= md^2 and clamp to the same value.  11-cell windows on the 101 x 101 x 23 grids of the benchmark: 0.23 M voxels x 63 reads.
#include "rbp_dev.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common/ecbs_rules.h"

namespace {

constexpr int EDT_INF = 0x3f3f3f3f;

// ---- a SET of W worlds in one build (rbp_dev_worlds of include/rbp.h) ------------------------------------------------------------------
// The three min-plus passes, with the world index as a grid dimension: the leaf lists of all worlds lie in one buffer, every world has
// a descriptor (its own res, hence its own dim / key_min / md) and the float grids lie back to back in one allocation.  Per chunk of
// worlds (the int32 scratch is bounded, whatever W):
//   1. edt_set_raster_kernel   leaves -> one byte of occupancy per voxel (cleared by a memset before)
//   2. edt_set_zy_kernel       one workgroup per (world, x) slab of ny * nz cells: the z pass from the occupancy bytes into LDS, the y
//                              pass from LDS into the only int32 intermediate that reaches global memory (9.3 KB of LDS at 101 x 23)
//   3. edt_set_x_finish_kernel one thread per voxel: the x pass (2 md - 1 coalesced reads) and the finish: sqrt in double, rounded to float
//                              (dynamicEDT3D keeps float distances in cells), times the double resolution, rounded to float (getDistance)
// A slab of more than EDT_SLAB_MAX cells (64 KB of LDS) takes edt_set_z_kernel + edt_set_y_kernel through a second int32 buffer instead
// of kernel 2.  Integer minima are exact in any order, so both routes give the same floats, bit for bit, and so does a set of one
// (rbp_edt_build) or of fifty.
struct EdtWorldDesc {
    int dim[3];
    int kmin[3];
    int md;                // window half-width + 1 in cells: (int)(max_dist / res + 1)
    int n_leaves;
    long long leaf_off;    // first leaf of the world in the set's leaf buffer
    long long cell_off;    // first cell of the world in the set's float allocation
    long long chunk_off;   // first cell of the world in the chunk's scratch
    double res;
};

#ifndef EDT_SLAB_MAX_CELLS
#define EDT_SLAB_MAX_CELLS 16384  // (A/B builds: -DEDT_SLAB_MAX_CELLS=0 sends every set through the unfused passes, tools/dev_worlds_ab.py)
#endif
constexpr int EDT_SLAB_MAX = EDT_SLAB_MAX_CELLS;  // cells of a (world, x) slab the fused z + y kernel keeps in LDS as int32: 64 KB
constexpr long long EDT_CHUNK_CELLS = 1 << 22;  // scratch of a chunk of worlds: 4 M cells = 16 MB of int32 + 4 MB of occupancy
constexpr int EDT_CHUNK_WORLDS = 32768;         // (grid dimension y)

__global__ __launch_bounds__(256) void edt_set_raster_kernel(const EdtWorldDesc* __restrict__ desc, const int* __restrict__ keys,
                                                             unsigned char* __restrict__ occ) {
    const EdtWorldDesc& w = desc[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.n_leaves) return;
    const int* k = keys + 4 * (w.leaf_off + i);
    const int nx = w.dim[0], ny = w.dim[1], nz = w.dim[2];
    const int s = k[3];
    const int x0 = max(k[0] - w.kmin[0], 0), x1 = min(k[0] - w.kmin[0] + s - 1, nx - 1);
    const int y0 = max(k[1] - w.kmin[1], 0), y1 = min(k[1] - w.kmin[1] + s - 1, ny - 1);
    const int z0 = max(k[2] - w.kmin[2], 0), z1 = min(k[2] - w.kmin[2] + s - 1, nz - 1);
    unsigned char* g = occ + w.chunk_off;
    for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y)
            for (int z = z0; z <= z1; ++z) g[((size_t)x * ny + y) * nz + z] = 1;
}

// z pass of one cell from the occupancy bytes of its row: min over |d| < md of d^2 where occ(z + d) is set
__device__ __forceinline__ int edt_z_of_row(const unsigned char* __restrict__ row, int z, int nz, int md) {
    const int lo = max(-(md - 1), -z), hi = min(md - 1, nz - 1 - z);
    int best = EDT_INF;
    for (int d = lo; d <= hi; ++d)
        if (row[z + d]) best = min(best, d * d);
    return best;
}

// min over |d| < md of d^2 + in[d * stride] along an axis of n cells, for the cell at position p of it (`in` points at that cell)
template <class Ptr>
__device__ __forceinline__ int edt_window(Ptr in, int p, int n, long long stride, int md) {
    const int lo = max(-(md - 1), -p), hi = min(md - 1, n - 1 - p);
    int best = EDT_INF;
    for (int d = lo; d <= hi; ++d) {
        const int v = in[d * stride];
        best = min(best, v >= EDT_INF ? EDT_INF : v + d * d);
    }
    return best;
}

__global__ __launch_bounds__(256) void edt_set_zy_kernel(const EdtWorldDesc* __restrict__ desc, const unsigned char* __restrict__ occ,
                                                         int* __restrict__ d2) {
    extern __shared__ int slab[];  // [ny][nz]: the slab after the z pass
    const EdtWorldDesc& w = desc[blockIdx.y];
    const int x = blockIdx.x;
    if (x >= w.dim[0]) return;  // (uniform over the workgroup: before any barrier)
    const int ny = w.dim[1], nz = w.dim[2], md = w.md, n = ny * nz;
    const long long base = w.chunk_off + (long long)x * n;
    const unsigned char* o = occ + base;
    for (int c = threadIdx.x; c < n; c += blockDim.x) {
        const int y = c / nz, z = c - y * nz;
        slab[c] = edt_z_of_row(o + y * nz, z, nz, md);
    }
    __syncthreads();
    int* out = d2 + base;
    for (int c = threadIdx.x; c < n; c += blockDim.x) out[c] = edt_window(slab + c, c / nz, ny, (long long)nz, md);
}

// the same two passes unfused, for slabs that do not fit the LDS: one thread per voxel and pass
__global__ __launch_bounds__(256) void edt_set_z_kernel(const EdtWorldDesc* __restrict__ desc, const unsigned char* __restrict__ occ,
                                                        int* __restrict__ out) {
    const EdtWorldDesc& w = desc[blockIdx.y];
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (long long)w.dim[0] * w.dim[1] * w.dim[2]) return;
    const int nz = w.dim[2], z = (int)(c % nz);
    out[w.chunk_off + c] = edt_z_of_row(occ + w.chunk_off + (c - z), z, nz, w.md);
}

__global__ __launch_bounds__(256) void edt_set_y_kernel(const EdtWorldDesc* __restrict__ desc, const int* __restrict__ in, int* __restrict__ out) {
    const EdtWorldDesc& w = desc[blockIdx.y];
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (long long)w.dim[0] * w.dim[1] * w.dim[2]) return;
    const int ny = w.dim[1], nz = w.dim[2];
    out[w.chunk_off + c] = edt_window(in + w.chunk_off + c, (int)((c / nz) % ny), ny, (long long)nz, w.md);
}

__global__ __launch_bounds__(256) void edt_set_x_finish_kernel(const EdtWorldDesc* __restrict__ desc, const int* __restrict__ d2,
                                                               float* __restrict__ dist) {
    const EdtWorldDesc& w = desc[blockIdx.y];
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (long long)w.dim[0] * w.dim[1] * w.dim[2]) return;
    const long long stride = (long long)w.dim[1] * w.dim[2];
    const int sq = edt_window(d2 + w.chunk_off + c, (int)(c / stride), w.dim[0], stride, w.md);
    const int md2 = w.md * w.md;
    const float cells = (float)__dsqrt_rn((double)(sq < md2 ? sq : md2));  // dynamicEDT3D keeps float distances in cells
    dist[w.cell_off + c] = (float)((double)cells * w.res);                 // getDistance: float * double treeResolution -> float
}

// ---- the coarse obstacle mask of the ECBS front-end from a resident grid (ECBSPlanner::setObstacles, ecbs_planner.hpp:80-109) ----------
// One thread per sample (x, y, z) of the planning lattice: getDistance's lookup and `dist < r + grid_margin` in double.  xs / ys / zs hold the
// sample coordinates as float (octomap::point3d), cx / cy / cz the mask cell of each sample (-1: none), both made on the host by the
// reference's own loops (common/ecbs_rules.h lattice_samples).  A sample outside the grid sets *outside.
__device__ __forceinline__ void ecbs_obstacle_sample(const DevWorld& w, const float* __restrict__ xs, const float* __restrict__ ys,
                                                     const float* __restrict__ zs, const int* __restrict__ cx, const int* __restrict__ cy,
                                                     const int* __restrict__ cz, int sx, int sy, int sz, int dimy, int dimz, double limit,
                                                     unsigned char* __restrict__ mask, unsigned* __restrict__ outside) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sx * sy * sz) return;
    const int c = i % sz, b = (i / sz) % sy, a = i / (sz * sy);
    const double rf = 1.0 / w.res;
    const int kx = (int)floor(rf * (double)xs[a]) - w.key_min[0];
    const int ky = (int)floor(rf * (double)ys[b]) - w.key_min[1];
    const int kz = (int)floor(rf * (double)zs[c]) - w.key_min[2];
    if (kx < 0 || ky < 0 || kz < 0 || kx >= w.dim[0] || ky >= w.dim[1] || kz >= w.dim[2]) {
        atomicOr(outside, 1u);
        return;
    }
    const float d = w.dist[((size_t)kx * w.dim[1] + ky) * w.dim[2] + kz];
    if ((double)d < limit && cx[a] >= 0 && cy[b] >= 0 && cz[c] >= 0) mask[((size_t)cx[a] * dimy + cy[b]) * dimz + cz[c]] = 1;
}

// K missions in one launch (blockIdx.y): mission k reads worlds[k] against limits[k] and writes masks[k][ncell], outside[k]
__global__ __launch_bounds__(256) void ecbs_obstacle_set_kernel(const DevWorld* __restrict__ worlds, const double* __restrict__ limits,
                                                                const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                                const int* __restrict__ cx, const int* __restrict__ cy, const int* __restrict__ cz, int sx,
                                                                int sy, int sz, int dimx, int dimy, int dimz, unsigned char* __restrict__ masks,
                                                                unsigned* __restrict__ outside) {
    const int k = blockIdx.y;
    ecbs_obstacle_sample(worlds[k], xs, ys, zs, cx, cy, cz, sx, sy, sz, dimy, dimz, limits[k], masks + (size_t)k * dimx * dimy * dimz, outside + k);
}

int dims(double res, const double* bmin, const double* bmax, int* dim, int* kmin) {
    if (!(res > 0)) return 1;
    const double rf = 1.0 / res;  // octomap resolution_factor
    for (int a = 0; a < 3; ++a) {
        // octomap::point3d is float32; coordToKey(c) = (int)floor(resolution_factor * c) (+32768)
        kmin[a] = (int)floor(rf * (double)(float)bmin[a]);
        const int kmax = (int)floor(rf * (double)(float)bmax[a]);
        if (kmax < kmin[a]) return 1;
        dim[a] = kmax - kmin[a] + 1;
        if (dim[a] > 4096) return 1;
    }
    return 0;
}

}  // namespace

// W float grids in one allocation on one device, with what rbp_world needs of each
struct rbp_dev_worlds {
    int device = 0;
    float* dist = nullptr;
    std::vector<EdtWorldDesc> desc;
};

namespace {

// The obstacle masks of K missions on resident worlds, made where the grids are and left there: [K][ncell] bytes, padded to a word, then the
// K flag words (a lattice sample lay outside the world's grid).  The buffers (the kernel's inputs too) are freed with the struct.
struct EcbsMasks {
    DeviceBuffers buffers;
    unsigned char* mask = nullptr;
    size_t mask_bytes = 0;
    const unsigned* outside() const { return reinterpret_cast<const unsigned*>(mask + mask_bytes); }
};

// Fills `m` on the current device (that of `ws`) for missions that read worlds world_index[k], launches queued on the null stream; dim receives the lattice.
int ecbs_masks_on_device(const char* who, const rbp_dev_worlds* ws, int K, const int32_t* world_index, const rbp_mission* missions,
                         const rbp_param* param, int32_t dim[3], EcbsMasks& m) {
    auto bad = [&](const char* what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": " + what).c_str()); };
    double gmin[3], gmax[3], gres[3];
    if (!ecbs_rules::planning_lattice(param, 4096, gmin, gmax, gres, dim)) return bad("grid resolution must be positive, planning grid of 1..4096 cells per axis");
    std::vector<float> pos[3];
    std::vector<int> cell[3];
    ecbs_rules::lattice_samples(gmin, gmax, gres, dim, pos, cell);
    const int sx = (int)pos[0].size(), sy = (int)pos[1].size(), sz = (int)pos[2].size(), ns = sx + sy + sz;
    if ((double)sx * sy * sz > (double)(1 << 30)) return bad("more than 2^30 samples");
    const size_t ncell = (size_t)dim[0] * dim[1] * dim[2];
    m.mask_bytes = ((size_t)K * ncell + 3) & ~size_t(3);
    std::vector<int> up(2 * (size_t)ns);  // the sample coordinates of the three axes, then their mask cells
    for (int a = 0, o = 0; a < 3; o += (int)pos[a].size(), ++a) {
        memcpy(&up[o], pos[a].data(), sizeof(float) * pos[a].size());
        memcpy(&up[ns + o], cell[a].data(), sizeof(int) * cell[a].size());
    }
    std::vector<DevWorld> worlds(K);
    std::vector<double> limits(K);
    for (int k = 0; k < K; ++k) {
        const EdtWorldDesc& d = ws->desc[world_index[k]];
        for (int a = 0; a < 3; ++a) worlds[k].dim[a] = d.dim[a], worlds[k].key_min[a] = d.kmin[a];
        worlds[k].res = d.res, worlds[k].dist = ws->dist + d.cell_off;
        double r = 0;
        for (int qi = 0; qi < missions[k].N; ++qi) r = std::max(r, missions[k].radius[qi]);
        limits[k] = r + param->grid_margin;
    }
    const int* c = m.buffers.upload(up);
    const DevWorld* d_worlds = m.buffers.upload(worlds);
    const double* d_limits = m.buffers.upload(limits);
    m.mask = m.buffers.get<unsigned char>(m.mask_bytes + 4 * (size_t)K, true);
    hipError_t e = m.buffers.err;
    const float* f = reinterpret_cast<const float*>(c);
    c += ns;
    for (int k0 = 0; k0 < K && e == hipSuccess; k0 += 32768) {  // (grid dimension y)
        const int nk = std::min(K - k0, 32768);
        hipLaunchKernelGGL(ecbs_obstacle_set_kernel, dim3((unsigned)(((size_t)sx * sy * sz + 255) / 256), nk), dim3(256), 0, 0, d_worlds + k0, d_limits + k0, f,
                           f + sx, f + sx + sy, c, c + sx, c + sx + sy, sx, sy, sz, dim[0], dim[1], dim[2], m.mask + (size_t)k0 * ncell,
                           reinterpret_cast<unsigned*>(m.mask + m.mask_bytes) + k0);
        e = hipGetLastError();
    }
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(e)).c_str());
}

// builds the grids of `ws` (desc filled but for chunk_off; ws->dist allocated) on the current device; returns when they are complete
int build_set(rbp_dev_worlds* ws, const int32_t* const* leaf_keys) {
    const int W = (int)ws->desc.size();
    std::vector<int> keys_h;
    for (int w = 0; w < W; ++w)
        if (ws->desc[w].n_leaves > 0) keys_h.insert(keys_h.end(), leaf_keys[w], leaf_keys[w] + 4 * (size_t)ws->desc[w].n_leaves);
    // chunks of consecutive worlds whose cells fit the scratch (a world larger than the scratch is a chunk of its own)
    std::vector<int> chunk_begin{0};
    long long in_chunk = 0, scratch_cells = 0;
    bool any_unfused = false;
    for (int w = 0; w < W; ++w) {
        EdtWorldDesc& d = ws->desc[w];
        const long long nc = (long long)d.dim[0] * d.dim[1] * d.dim[2];
        if (w > chunk_begin.back() && (in_chunk + nc > EDT_CHUNK_CELLS || w - chunk_begin.back() >= EDT_CHUNK_WORLDS)) chunk_begin.push_back(w), in_chunk = 0;
        d.chunk_off = in_chunk;
        in_chunk += nc;
        scratch_cells = std::max(scratch_cells, in_chunk);
        any_unfused = any_unfused || d.dim[1] * d.dim[2] > EDT_SLAB_MAX;
    }
    chunk_begin.push_back(W);

    int* d_keys = nullptr;
    EdtWorldDesc* d_desc = nullptr;
    unsigned char* d_occ = nullptr;
    int *d_a = nullptr, *d_b = nullptr;
    hipError_t e = hipSuccess;
    auto done = [&](int rc, const std::string& msg) {
        (void)hipFree(d_keys), (void)hipFree(d_desc), (void)hipFree(d_occ), (void)hipFree(d_a), (void)hipFree(d_b);
        return rc == RBP_OK ? RBP_OK : rbp_set_error(rc, msg.c_str());
    };
#define EDT_TRY(expr)                                                                                  \
    do {                                                                                               \
        e = (expr);                                                                                    \
        if (e != hipSuccess) return done(RBP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e)); \
    } while (0)
    if (!keys_h.empty()) {
        EDT_TRY(hipMalloc((void**)&d_keys, sizeof(int) * keys_h.size()));
        EDT_TRY(hipMemcpy(d_keys, keys_h.data(), sizeof(int) * keys_h.size(), hipMemcpyHostToDevice));
    }
    EDT_TRY(hipMalloc((void**)&d_desc, sizeof(EdtWorldDesc) * W));
    EDT_TRY(hipMemcpy(d_desc, ws->desc.data(), sizeof(EdtWorldDesc) * W, hipMemcpyHostToDevice));
    EDT_TRY(hipMalloc((void**)&d_occ, (size_t)scratch_cells));
    EDT_TRY(hipMalloc((void**)&d_a, sizeof(int) * (size_t)scratch_cells));
    if (any_unfused) EDT_TRY(hipMalloc((void**)&d_b, sizeof(int) * (size_t)scratch_cells));
    for (size_t ci = 0; ci + 1 < chunk_begin.size(); ++ci) {
        const int w0 = chunk_begin[ci], nw = chunk_begin[ci + 1] - w0;
        long long cells = 0, max_cells = 0;
        int max_leaves = 0, max_nx = 0, max_slab = 0;
        for (int w = w0; w < w0 + nw; ++w) {
            const EdtWorldDesc& d = ws->desc[w];
            const long long nc = (long long)d.dim[0] * d.dim[1] * d.dim[2];
            cells += nc, max_cells = std::max(max_cells, nc);
            max_leaves = std::max(max_leaves, d.n_leaves), max_nx = std::max(max_nx, d.dim[0]), max_slab = std::max(max_slab, d.dim[1] * d.dim[2]);
        }
        const EdtWorldDesc* dd = d_desc + w0;
        const unsigned nb = (unsigned)((max_cells + 255) / 256);
        EDT_TRY(hipMemsetAsync(d_occ, 0, (size_t)cells, 0));
        if (max_leaves > 0)
            hipLaunchKernelGGL(edt_set_raster_kernel, dim3((unsigned)((max_leaves + 255) / 256), nw), dim3(256), 0, 0, dd, d_keys, d_occ);
        if (max_slab <= EDT_SLAB_MAX) {
            hipLaunchKernelGGL(edt_set_zy_kernel, dim3(max_nx, nw), dim3(256), sizeof(int) * (size_t)max_slab, 0, dd, d_occ, d_a);
            hipLaunchKernelGGL(edt_set_x_finish_kernel, dim3(nb, nw), dim3(256), 0, 0, dd, d_a, ws->dist);
        } else {
            hipLaunchKernelGGL(edt_set_z_kernel, dim3(nb, nw), dim3(256), 0, 0, dd, d_occ, d_a);
            hipLaunchKernelGGL(edt_set_y_kernel, dim3(nb, nw), dim3(256), 0, 0, dd, d_a, d_b);
            hipLaunchKernelGGL(edt_set_x_finish_kernel, dim3(nb, nw), dim3(256), 0, 0, dd, d_b, ws->dist);
        }
        EDT_TRY(hipGetLastError());
    }
    EDT_TRY(hipStreamSynchronize(0));
#undef EDT_TRY
    return done(RBP_OK, "");
}

// argument checks and descriptors of a set (no device work); nullptr + the error recorded on a bad argument
rbp_dev_worlds* describe_set(const char* who, int32_t W, const int32_t* const* leaf_keys, const int64_t* n_leaves, const double* res,
                             const double* bmin, const double* bmax, double max_dist) {
    auto bad = [&](const char* what) {
        rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": " + what).c_str());
        return (rbp_dev_worlds*)nullptr;
    };
    if (W <= 0 || !n_leaves || !res || !bmin || !bmax) return bad("need W > 0, n_leaves, res and the box");
    if (!(max_dist > 0)) return bad("need max_dist > 0");
    auto* ws = new rbp_dev_worlds();
    ws->desc.resize(W);
    long long cell_off = 0, leaf_off = 0;
    for (int w = 0; w < W; ++w) {
        EdtWorldDesc& d = ws->desc[w];
        const char* what = nullptr;
        if (n_leaves[w] < 0 || n_leaves[w] > 0x7fffffff / 4 || (n_leaves[w] > 0 && (!leaf_keys || !leaf_keys[w]))) what = "negative n_leaves, or leaves without keys";
        else if (dims(res[w], bmin, bmax, d.dim, d.kmin)) what = "need res > 0, bbx_min <= bbx_max, at most 4096 voxels per axis";
        else if (!(max_dist / res[w] + 1 < 4097.0)) what = "max_dist / res out of range";
        if (what) {
            delete ws;
            return bad(what);
        }
        d.md = (int)(max_dist / res[w] + 1);
        d.n_leaves = (int)n_leaves[w];
        d.leaf_off = leaf_off, d.cell_off = cell_off, d.chunk_off = 0, d.res = res[w];
        leaf_off += d.n_leaves, cell_off += (long long)d.dim[0] * d.dim[1] * d.dim[2];
    }
    return ws;
}

int create_set(const char* who, rbp_dev_worlds** out, int device, int32_t W, const int32_t* const* leaf_keys, const int64_t* n_leaves,
               const double* res, const double* bmin, const double* bmax, double max_dist) {
    rbp_dev_worlds* ws = describe_set(who, W, leaf_keys, n_leaves, res, bmin, bmax, max_dist);
    if (!ws) return RBP_ERR_BAD_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        delete ws;
        return rbp_set_error(RBP_ERR_NO_DEVICE, "no HIP device: the RBP path has no CPU fallback");
    }
    if (device < 0) (void)hipGetDevice(&device);
    if (device < 0 || device >= ndev) {
        delete ws;
        return rbp_set_error(RBP_ERR_NO_DEVICE, "device index out of range");
    }
    ws->device = device;
    DeviceScope scope(device);
    const EdtWorldDesc& last = ws->desc.back();
    const long long total = last.cell_off + (long long)last.dim[0] * last.dim[1] * last.dim[2];
    hipError_t e = hipMalloc((void**)&ws->dist, sizeof(float) * (size_t)total);
    int rc = e == hipSuccess ? build_set(ws, leaf_keys) : rbp_set_error(RBP_ERR_HIP, (std::string("hipMalloc: ") + hipGetErrorString(e)).c_str());
    if (rc) {
        (void)hipFree(ws->dist);
        delete ws;
        return rc;
    }
    *out = ws;
    return RBP_OK;
}

}  // namespace

extern "C" int rbp_edt_dims(double res, const double bbx_min[3], const double bbx_max[3], int32_t dim[3], int32_t key_min[3]) {
    if (!bbx_min || !bbx_max || !dim || !key_min || dims(res, bbx_min, bbx_max, dim, key_min))
        return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "rbp_edt_dims: need res > 0, bbx_min <= bbx_max, at most 4096 voxels per axis");
    return RBP_OK;
}

// one world, returned to the host: a set of one on the calling thread's current device, and the copy back
extern "C" int rbp_edt_build(const int32_t* leaf_keys, int64_t n_leaves, double res, const double bbx_min[3], const double bbx_max[3],
                             double max_dist, float* dist) {
    if (!dist) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "rbp_edt_build: bad argument");
    rbp_dev_worlds* ws = nullptr;
    int rc = create_set("rbp_edt_build", &ws, -1, 1, &leaf_keys, &n_leaves, &res, bbx_min, bbx_max, max_dist);
    if (rc) return rc;
    rc = rbp_dev_worlds_download(ws, 0, dist);
    rbp_dev_worlds_destroy(ws);
    return rc;
}

extern "C" int rbp_dev_worlds_create(rbp_dev_worlds** out, int device, int32_t W, const int32_t* const* leaf_keys, const int64_t* n_leaves,
                                     const double* res, const double bbx_min[3], const double bbx_max[3], double max_dist) {
    if (!out) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "rbp_dev_worlds_create: null out");
    *out = nullptr;
    return create_set("rbp_dev_worlds_create", out, device, W, leaf_keys, n_leaves, res, bbx_min, bbx_max, max_dist);
}

extern "C" int rbp_dev_worlds_count(const rbp_dev_worlds* ws) { return ws ? (int)ws->desc.size() : 0; }
int dev_worlds_device(const rbp_dev_worlds* ws) { return ws->device; }

extern "C" int rbp_dev_worlds_get(const rbp_dev_worlds* ws, int32_t w, rbp_world* out) {
    if (!ws || !out || w < 0 || w >= (int)ws->desc.size()) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "rbp_dev_worlds_get: null argument or world index out of range");
    const EdtWorldDesc& d = ws->desc[w];
    for (int a = 0; a < 3; ++a) out->dim[a] = d.dim[a], out->key_min[a] = d.kmin[a];
    out->res = d.res;
    out->dist = ws->dist + d.cell_off;
    return RBP_OK;
}

extern "C" int rbp_dev_worlds_download(const rbp_dev_worlds* ws, int32_t w, float* dist_host) {
    rbp_world g;
    if (!dist_host) return rbp_set_error(RBP_ERR_BAD_ARGUMENT, "rbp_dev_worlds_download: null buffer");
    if (int rc = rbp_dev_worlds_get(ws, w, &g)) return rc;
    DeviceScope scope(ws->device);
    const hipError_t e = hipMemcpy(dist_host, g.dist, sizeof(float) * (size_t)g.dim[0] * g.dim[1] * g.dim[2], hipMemcpyDeviceToHost);
    return e == hipSuccess ? RBP_OK : rbp_set_error(RBP_ERR_HIP, (std::string("hipMemcpy: ") + hipGetErrorString(e)).c_str());
}

extern "C" void rbp_dev_worlds_destroy(rbp_dev_worlds* ws) {
    if (!ws) return;
    if (ws->dist) {
        DeviceScope scope(ws->device);
        (void)hipFree(ws->dist);
    }
    delete ws;
}

extern "C" int rbp_dev_worlds_ecbs_obstacles(const rbp_dev_worlds* ws, int32_t w, const rbp_mission* mission, const rbp_param* param, int32_t dim[3],
                                             uint8_t* obstacle_host, size_t capacity) {
    const char* who = "rbp_dev_worlds_ecbs_obstacles";
    auto bad = [&](const char* what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": " + what).c_str()); };
    rbp_world g;
    if (!mission || !param || !dim || mission->N <= 0 || !mission->radius) return bad("null argument");
    if (int rc = rbp_dev_worlds_get(ws, w, &g)) return rc;
    double gmin[3], gmax[3], gres[3];
    if (!ecbs_rules::planning_lattice(param, 4096, gmin, gmax, gres, dim)) return bad("grid resolution must be positive, planning grid of 1..4096 cells per axis");
    if (!obstacle_host) return RBP_OK;  // (only the shape was asked for)
    const size_t ncell = (size_t)dim[0] * dim[1] * dim[2];
    if (capacity < ncell) return bad("obstacle buffer smaller than dim[0] * dim[1] * dim[2]");
    DeviceScope scope(ws->device);
    EcbsMasks m;
    if (int rc = ecbs_masks_on_device(who, ws, 1, &w, mission, param, dim, m)) return rc;
    std::vector<unsigned char> back(m.mask_bytes + 4);  // one buffer back: the mask, then the flag word
    const hipError_t e = hipMemcpy(back.data(), m.mask, back.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rbp_set_error(RBP_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(e)).c_str());
    memcpy(obstacle_host, back.data(), ncell);
    unsigned outside = 0;
    memcpy(&outside, back.data() + m.mask_bytes, 4);
    return outside ? 1 : RBP_OK;
}

// the device search of kernels/ecbs.hip on resident worlds: the masks of all K missions in one launch, handed to the search where they are
extern "C" int rbp_dev_worlds_ecbs_plan(const rbp_dev_worlds* ws, int32_t K, const int32_t* world_index, const rbp_mission* missions,
                                        const rbp_param* param, int64_t max_high_level_nodes, rbp_ecbs_out* out) {
    const char* who = "rbp_dev_worlds_ecbs_plan";
    auto bad = [&](const char* what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": " + what).c_str()); };
    if (!ws || !world_index) return bad("need the set of worlds and world_index");
    int32_t dim[3], sdim[3];
    if (int rc = ecbs_check_arguments(who, K, nullptr, missions, param, max_high_level_nodes, out, dim)) return rc;
    for (int k = 0; k < K; ++k)
        if (world_index[k] < 0 || world_index[k] >= (int)ws->desc.size()) return bad("world index out of range");
    DeviceScope scope(ws->device);
    EcbsMasks m;
    if (int rc = ecbs_masks_on_device(who, ws, K, world_index, missions, param, sdim, m)) return rc;
    return ecbs_plan_on_device(who, K, dim, m.mask, m.outside(), missions, param, max_high_level_nodes, out);
}

// the same search with its results left on the device (rbp_dev_ecbs; kernels/ecbs.hip ecbs_search_on_device): what
// rbp_session_create_from_ecbs builds a session from and rbp_dev_ecbs_download reads
extern "C" int rbp_dev_worlds_ecbs_search(const rbp_dev_worlds* ws, int32_t K, const int32_t* world_index, const rbp_mission* missions,
                                          const rbp_param* param, int64_t max_high_level_nodes, int32_t max_M, rbp_dev_ecbs** out) {
    const char* who = "rbp_dev_worlds_ecbs_search";
    auto bad = [&](const char* what) { return rbp_set_error(RBP_ERR_BAD_ARGUMENT, (std::string(who) + ": " + what).c_str()); };
    if (!out) return bad("null out");
    *out = nullptr;
    if (!ws || !world_index) return bad("need the set of worlds and world_index");
    int32_t dim[3], sdim[3];
    if (int rc = ecbs_check_search(who, K, nullptr, missions, param, max_high_level_nodes, max_M, dim)) return rc;
    for (int k = 0; k < K; ++k)
        if (world_index[k] < 0 || world_index[k] >= (int)ws->desc.size()) return bad("world index out of range");
    DeviceScope scope(ws->device);
    EcbsMasks m;
    if (int rc = ecbs_masks_on_device(who, ws, K, world_index, missions, param, sdim, m)) return rc;
    rbp_dev_ecbs* e = new rbp_dev_ecbs();
    e->ws = ws, e->world_index.assign(world_index, world_index + K);
    if (int rc = ecbs_search_on_device(who, K, dim, m.mask, m.outside(), missions, param, max_high_level_nodes, max_M, e)) {
        delete e;
        return rc;
    }
    *out = e;
    return RBP_OK;
}
