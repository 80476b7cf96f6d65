// pnr_mesh.hip -- mesh extraction for gfx950: the evaluation grid of src/util/recon.py (util.gen_grid, src/util/util.py:93-110,
// and the "fake" view directions of recon.py:54) and marching cubes on a density grid (recon.py:68-78, where the reference calls
// PyMCubes on the host).  Indexed mesh, bit-identical from run to run: every grid point owns its +x, +y, +z edges, the vertex of an
// edge is computed once by the edge's owner, vertex and triangle offsets come from one hand-written integer scan (block sums, a
// scan of the block sums, the add) -- no atomics anywhere.  The library allocates nothing: workspace and outputs are the caller's.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "pnr_common.h"
#include "pnr_wave.h"

namespace pnr {

// up to five triangles per case as cube-edge ids, -1 terminated (conventions: include/pixelnerf_hip.h, pnr_marching_cubes_tables)
static const signed char MC_TRI_HOST[256][16] = {
#include "pnr_mc_tables.inc"
};
__constant__ signed char MC_TRI[256][16] = {
#include "pnr_mc_tables.inc"
};

constexpr int MC_THREADS = 256;
constexpr int MC_ITEMS = 4;                          // consecutive grid points per thread of the scan
constexpr int MC_BLOCK = MC_THREADS * MC_ITEMS;      // grid points per scan block
constexpr int MC_TOP_THREADS = 1024;                 // the single workgroup that scans the block sums

typedef unsigned long long u64;

// workspace: off[N] u64 (low word: vertices in front of the point's first edge, high word: triangles in front of its cell) |
// info[N] u32 (bits 0-2: which owned edges carry a vertex, bits 8-15: the cell's case) | bsum[nb] u64 | bnf[nb] u32
struct McWorkspace {
    u64 *off;
    unsigned *info;
    u64 *bsum;
    unsigned *bnf;
};

static long long mc_blocks(long long N) { return (N + MC_BLOCK - 1) / MC_BLOCK; }
static size_t mc_pad8(size_t b) { return (b + 7) / 8 * 8; }

static McWorkspace mc_carve(void *workspace, long long N) {
    char *p = (char *)workspace;
    McWorkspace w;
    w.off = (u64 *)p;
    p += (size_t)N * 8;
    w.info = (unsigned *)p;
    p += mc_pad8((size_t)N * 4);
    w.bsum = (u64 *)p;
    p += (size_t)mc_blocks(N) * 8;
    w.bnf = (unsigned *)p;
    return w;
}

// a corner is inside iff its value is finite and above the level (a value equal to it is outside)
__device__ __forceinline__ bool mc_finite(float f) { return fabsf(f) <= 3.402823466e+38f; }
__device__ __forceinline__ bool mc_inside(float f, float iso) { return mc_finite(f) && f > iso; }

// classification + the scan's first level: per grid point the owned edges that carry a vertex and the case of the cell whose
// lowest corner it is; exclusive offsets within the block of MC_BLOCK points, the block's totals to bsum / bnf
__global__ void __launch_bounds__(MC_THREADS)
mc_classify_kernel(const float *__restrict__ field, int nx, int ny, int nz, float iso, McWorkspace ws) {
    __shared__ u64 wave_tot[MC_THREADS / 64];
    __shared__ unsigned wave_nf[MC_THREADS / 64];
    const long long N = (long long)nx * ny * nz;
    const long long sy = nz, sx = (long long)ny * nz;
    const long long p0 = (long long)blockIdx.x * MC_BLOCK + (long long)threadIdx.x * MC_ITEMS;
    u64 cnt[MC_ITEMS];
    u64 tsum = 0;
    unsigned nf = 0;
#pragma unroll
    for (int it = 0; it < MC_ITEMS; ++it) {
        const long long p = p0 + it;
        cnt[it] = 0;
        if (p >= N) continue;
        const int k = (int)(p % nz), j = (int)((p / nz) % ny), i = (int)(p / sx);
        const float f0 = field[p];
        nf += mc_finite(f0) ? 0u : 1u;
        const bool hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
        const bool c0 = mc_inside(f0, iso);
        const bool c1 = hx && mc_inside(field[p + sx], iso);
        const bool c2 = hy && mc_inside(field[p + sy], iso);
        const bool c4 = hz && mc_inside(field[p + 1], iso);
        unsigned mask = 0, cs = 0;
        if (hx && c0 != c1) mask |= 1u;
        if (hy && c0 != c2) mask |= 2u;
        if (hz && c0 != c4) mask |= 4u;
        if (hx && hy && hz) {
            const bool c3 = mc_inside(field[p + sx + sy], iso), c5 = mc_inside(field[p + sx + 1], iso);
            const bool c6 = mc_inside(field[p + sy + 1], iso), c7 = mc_inside(field[p + sx + sy + 1], iso);
            cs = (unsigned)c0 | (unsigned)c1 << 1 | (unsigned)c2 << 2 | (unsigned)c3 << 3 | (unsigned)c4 << 4 | (unsigned)c5 << 5 |
                 (unsigned)c6 << 6 | (unsigned)c7 << 7;
        }
        unsigned ntri = 0;
        while (ntri < 5 && MC_TRI[cs][3 * ntri] >= 0) ++ntri;
        ws.info[p] = mask | cs << 8;
        cnt[it] = (u64)__popc(mask) | (u64)ntri << 32;
        tsum += cnt[it];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 incl = wave_scan_add(tsum, lane);
    const unsigned nfw = wave_sum(nf);
    if (lane == 63) wave_tot[wv] = incl;
    if (lane == 0) wave_nf[wv] = nfw;
    __syncthreads();
    u64 base = incl - tsum;
    for (int w = 0; w < wv; ++w) base += wave_tot[w];
#pragma unroll
    for (int it = 0; it < MC_ITEMS; ++it) {
        const long long p = p0 + it;
        if (p < N) ws.off[p] = base;
        base += cnt[it];
    }
    if (threadIdx.x == 0) {
        u64 tot = 0;
        unsigned tnf = 0;
        for (int w = 0; w < MC_THREADS / 64; ++w) { tot += wave_tot[w]; tnf += wave_nf[w]; }
        ws.bsum[blockIdx.x] = tot;
        ws.bnf[blockIdx.x] = tnf;
    }
}

// the scan's second level, one workgroup: exclusive scan of the block sums in place, chunk by chunk with a running carry; the
// totals [n_vertices, n_triangles, n_nonfinite] to counts
__global__ void __launch_bounds__(MC_TOP_THREADS)
mc_scan_blocks_kernel(McWorkspace ws, long long nb, int *__restrict__ counts) {
    __shared__ u64 wave_tot[MC_TOP_THREADS / 64];
    __shared__ unsigned long long wave_nf[MC_TOP_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u64 carry = 0, nf_carry = 0;
    for (long long c0 = 0; c0 < nb; c0 += MC_TOP_THREADS) {
        const long long b = c0 + threadIdx.x;
        const u64 v = b < nb ? ws.bsum[b] : 0;
        u64 nf = b < nb ? (u64)ws.bnf[b] : 0;
        const u64 incl = wave_scan_add(v, lane);
        nf = wave_sum(nf);
        if (lane == 63) wave_tot[wv] = incl;
        if (lane == 0) wave_nf[wv] = nf;
        __syncthreads();
        u64 base = carry + incl - v, chunk = 0, chunk_nf = 0;
        for (int w = 0; w < MC_TOP_THREADS / 64; ++w) {
            if (w < wv) base += wave_tot[w];
            chunk += wave_tot[w];
            chunk_nf += wave_nf[w];
        }
        if (b < nb) ws.bsum[b] = base;
        carry += chunk;
        nf_carry += chunk_nf;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const u64 nt = carry >> 32;
        counts[0] = (int)(unsigned)(carry & 0xffffffffull);
        counts[1] = nt > (u64)INT_MAX ? INT_MAX : (int)nt;
        counts[2] = nf_carry > (u64)INT_MAX ? INT_MAX : (int)nf_carry;
    }
}

// the scan's third level: every point's offset becomes global
__global__ void __launch_bounds__(MC_THREADS) mc_add_offsets_kernel(McWorkspace ws, long long N) {
    const long long p = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (p < N) ws.off[p] += ws.bsum[p / MC_BLOCK];
}

#pragma clang fp contract(off)  // t, index + t and index * scale + c1 are separately rounded: the header states them so

// position of the vertex on the edge from a (lower index) to b, as a fraction of the edge.  A non-finite end counts as outside
// (mc_inside) and cannot be interpolated through: the vertex then sits on the finite end.
__device__ __forceinline__ float mc_edge_t(float fa, float fb, float iso) {
    if (!mc_finite(fb)) return 0.f;
    if (!mc_finite(fa)) return 1.f;
    return (iso - fa) / (fb - fa);
}

__global__ void __launch_bounds__(MC_THREADS)
mc_emit_kernel(const float *__restrict__ field, int nx, int ny, int nz, float iso, float c1x, float c1y, float c1z, float scx,
               float scy, float scz, McWorkspace ws, float *__restrict__ vertices, int *__restrict__ triangles) {
    const long long N = (long long)nx * ny * nz;
    const long long p = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (p >= N) return;
    const unsigned info = ws.info[p];
    const unsigned mask = info & 7u, cs = info >> 8;
    if (mask == 0 && (cs == 0 || cs == 255)) return;
    const long long sy = nz, sx = (long long)ny * nz;
    const u64 off = ws.off[p];
    if (mask) {
        const int k = (int)(p % nz), j = (int)((p / nz) % ny), i = (int)(p / sx);
        const float fa = field[p];
        size_t v = (size_t)(unsigned)(off & 0xffffffffull);
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            if (!(mask >> axis & 1u)) continue;
            const float t = mc_edge_t(fa, field[p + (axis == 0 ? sx : axis == 1 ? sy : 1)], iso);
            const float x = (float)i + (axis == 0 ? t : 0.f), y = (float)j + (axis == 1 ? t : 0.f), z = (float)k + (axis == 2 ? t : 0.f);
            vertices[3 * v] = x * scx + c1x;
            vertices[3 * v + 1] = y * scy + c1y;
            vertices[3 * v + 2] = z * scz + c1z;
            ++v;
        }
    }
    size_t tr = (size_t)(off >> 32);
    for (int n = 0; n < 5 && MC_TRI[cs][3 * n] >= 0; ++n, ++tr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int e = MC_TRI[cs][3 * n + c];
            const int axis = e >> 2, a = e & 1, b = (e >> 1) & 1;
            // lower end of edge e: the other two axes, in axis order, carry (a, b)
            const long long q = p + (axis == 0 ? a * sy + b : axis == 1 ? a * sx + b : a * sx + b * sy);
            const unsigned qmask = ws.info[q] & 7u;
            triangles[3 * tr + c] = (int)((unsigned)(ws.off[q] & 0xffffffffull) + (unsigned)__popc(qmask & ((1u << axis) - 1u)));
        }
    }
}

// util.gen_grid(..., ij_indexing=True) rows first .. first+count (x slowest) with numpy's linspace restated in fp64
// (numpy/_core/function_base.py: y = arange(n) * step + start, y[-1] = stop, cast to float32; step == 0: y / div * delta),
// and recon.py:54's direction -p / |p| (zero where |p| = 0)
struct GridAxis {
    double lo, hi, delta, step;
    int n;
};
__device__ __forceinline__ float grid_coord(const GridAxis &a, int i) {
    if (a.n > 1 && i == a.n - 1) return (float)a.hi;
    double y = (double)i;
    if (a.n > 1 && a.step != 0.0) y = y * a.step;
    else if (a.n > 1) y = y / (double)(a.n - 1) * a.delta;
    else y = y * a.delta;
    return (float)(y + a.lo);
}

// row r of the outputs = grid point p (both kernels below: one function, the same bits)
__device__ __forceinline__ void grid_point_row(const GridAxis &ax, const GridAxis &ay, const GridAxis &az, long long p, long long r,
                                               float *__restrict__ xyz, float *__restrict__ viewdirs) {
    const int k = (int)(p % az.n), j = (int)((p / az.n) % ay.n), i = (int)(p / ((long long)ay.n * az.n));
    const float x = grid_coord(ax, i), y = grid_coord(ay, j), z = grid_coord(az, k);
    xyz[3 * r] = x;
    xyz[3 * r + 1] = y;
    xyz[3 * r + 2] = z;
    if (viewdirs) {
        // the norm through fp64 (neither overflow nor a rounding worth mentioning): each component within 1 ulp of -p/|p|
        const double nrm = sqrt((double)x * x + (double)y * y + (double)z * z);
        const bool ok = nrm > 0.0;
        viewdirs[3 * r] = ok ? (float)(-(double)x / nrm) : 0.f;
        viewdirs[3 * r + 1] = ok ? (float)(-(double)y / nrm) : 0.f;
        viewdirs[3 * r + 2] = ok ? (float)(-(double)z / nrm) : 0.f;
    }
}

__global__ void __launch_bounds__(MC_THREADS)
gen_grid_points_kernel(GridAxis ax, GridAxis ay, GridAxis az, long long first, long long count, float *__restrict__ xyz,
                       float *__restrict__ viewdirs) {
    const long long r = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (r >= count) return;
    grid_point_row(ax, ay, az, first + r, r, xyz, viewdirs);
}

// the rows of a LIST of grid points (the kept points of a sparse baked volume); an id outside the grid gives a row of NaN
__global__ void __launch_bounds__(MC_THREADS)
gen_grid_points_at_kernel(GridAxis ax, GridAxis ay, GridAxis az, const int32_t *__restrict__ ids, long long count,
                          float *__restrict__ xyz, float *__restrict__ viewdirs) {
    const long long r = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (r >= count) return;
    const long long p = ids[r];
    if (p < 0 || p >= (long long)ax.n * ay.n * az.n) {
        const float nan = __int_as_float(0x7fc00000);
        xyz[3 * r] = xyz[3 * r + 1] = xyz[3 * r + 2] = nan;
        if (viewdirs) viewdirs[3 * r] = viewdirs[3 * r + 1] = viewdirs[3 * r + 2] = nan;
        return;
    }
    grid_point_row(ax, ay, az, p, r, xyz, viewdirs);
}
#pragma clang fp contract(fast)

static const char *mc_bad_dims(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return "every axis needs at least 2 grid points";
    if (3LL * nx * ny * nz >= (1LL << 31)) return "3 nx ny nz must stay below 2^31 (edge ids are int32)";
    return nullptr;
}

static int mc_fail(const char *entry, const char *why) {
    char msg[200];
    std::snprintf(msg, sizeof msg, "%s: %s", entry, why);
    return pnr_fail(PNR_E_INVALID, msg);  // (copies the text)
}

}  // namespace pnr

extern "C" int pnr_marching_cubes_tables(int *edge_mask, int *tri) {
    if (!edge_mask || !tri) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_tables: null argument");
    for (int cs = 0; cs < 256; ++cs) {
        int m = 0;
        for (int e = 0; e < 12; ++e) {
            const int axis = e >> 2, a = e & 1, b = (e >> 1) & 1;
            const int lo = axis == 0 ? 2 * a + 4 * b : axis == 1 ? a + 4 * b : a + 2 * b;
            if ((cs >> lo & 1) != (cs >> (lo + (1 << axis)) & 1)) m |= 1 << e;
        }
        edge_mask[cs] = m;
        for (int n = 0; n < 16; ++n) tri[cs * 16 + n] = pnr::MC_TRI_HOST[cs][n];
    }
    return PNR_OK;
}

extern "C" size_t pnr_marching_cubes_workspace_bytes(int nx, int ny, int nz) {
    if (pnr::mc_bad_dims(nx, ny, nz)) return 0;
    const long long N = (long long)nx * ny * nz, nb = pnr::mc_blocks(N);
    return (size_t)N * 8 + pnr::mc_pad8((size_t)N * 4) + (size_t)nb * 8 + pnr::mc_pad8((size_t)nb * 4);
}

extern "C" int pnr_marching_cubes_count(const float *field, int nx, int ny, int nz, float iso, void *workspace, int *counts_dev,
                                        void *stream) {
    if (const char *why = pnr::mc_bad_dims(nx, ny, nz)) return pnr::mc_fail("pnr_marching_cubes_count", why);
    if (!std::isfinite(iso)) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_count: iso must be finite");
    if (!field) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_count: field is null");
    if (!workspace || ((uintptr_t)workspace & 7)) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_count: workspace is null or not 8-byte aligned");
    if (!counts_dev) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_count: counts_dev is null");
    const long long N = (long long)nx * ny * nz, nb = pnr::mc_blocks(N);
    const pnr::McWorkspace ws = pnr::mc_carve(workspace, N);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pnr::mc_classify_kernel, dim3((unsigned)nb), dim3(pnr::MC_THREADS), 0, st, field, nx, ny, nz, iso, ws);
    hipLaunchKernelGGL(pnr::mc_scan_blocks_kernel, dim3(1), dim3(pnr::MC_TOP_THREADS), 0, st, ws, nb, counts_dev);
    hipLaunchKernelGGL(pnr::mc_add_offsets_kernel, dim3((unsigned)((N + pnr::MC_THREADS - 1) / pnr::MC_THREADS)), dim3(pnr::MC_THREADS),
                       0, st, ws, N);
    return pnr_check_launch("pnr_marching_cubes_count");
}

extern "C" int pnr_marching_cubes_emit(const float *field, int nx, int ny, int nz, float iso, const float *c1, const float *scale,
                                       const void *workspace, float *vertices, int *triangles, void *stream) {
    if (const char *why = pnr::mc_bad_dims(nx, ny, nz)) return pnr::mc_fail("pnr_marching_cubes_emit", why);
    if (!std::isfinite(iso)) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_emit: iso must be finite");
    if (!field) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_emit: field is null");
    if (!c1 || !scale) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_emit: c1 / scale is null (host arrays of 3 floats)");
    if (!workspace || ((uintptr_t)workspace & 7)) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_emit: workspace is null or not 8-byte aligned");
    if (!vertices || !triangles) return pnr_fail(PNR_E_INVALID, "pnr_marching_cubes_emit: vertices / triangles is null");
    const long long N = (long long)nx * ny * nz;
    const pnr::McWorkspace ws = pnr::mc_carve(const_cast<void *>(workspace), N);
    hipLaunchKernelGGL(pnr::mc_emit_kernel, dim3((unsigned)((N + pnr::MC_THREADS - 1) / pnr::MC_THREADS)), dim3(pnr::MC_THREADS), 0,
                       (hipStream_t)stream, field, nx, ny, nz, iso, c1[0], c1[1], c1[2], scale[0], scale[1], scale[2], ws, vertices,
                       triangles);
    return pnr_check_launch("pnr_marching_cubes_emit");
}

// c1, c2, reso of the two point entries -> the three axes; nullptr when they are usable
static const char *grid_axes(const double *c1, const double *c2, const int *reso, pnr::GridAxis *ax) {
    if (!c1 || !c2 || !reso) return "c1 / c2 / reso is null (host arrays of 3)";
    if (reso[0] < 1 || reso[1] < 1 || reso[2] < 1) return "reso must be positive";
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(c1[a]) || !std::isfinite(c2[a])) return "c1 / c2 must be finite";
        ax[a].lo = c1[a];
        ax[a].hi = c2[a];
        ax[a].n = reso[a];
        ax[a].delta = c2[a] - c1[a];
        ax[a].step = reso[a] > 1 ? ax[a].delta / (double)(reso[a] - 1) : 0.0;
    }
    return nullptr;
}

extern "C" int pnr_gen_grid_points(const double *c1, const double *c2, const int *reso, long long first, long long count, float *xyz,
                                   float *viewdirs, void *stream) {
    if (!c1 || !c2 || !reso) return pnr_fail(PNR_E_INVALID, "pnr_gen_grid_points: c1 / c2 / reso is null (host arrays of 3)");
    if (reso[0] < 1 || reso[1] < 1 || reso[2] < 1) return pnr_fail(PNR_E_INVALID, "pnr_gen_grid_points: reso must be positive");
    const long long N = (long long)reso[0] * reso[1] * reso[2];
    if (first < 0 || count < 0 || first > N || count > N - first)
        return pnr_fail(PNR_E_INVALID, "pnr_gen_grid_points: first .. first+count leaves the grid");
    if (count == 0) return PNR_OK;
    if (!xyz) return pnr_fail(PNR_E_INVALID, "pnr_gen_grid_points: xyz is null");
    pnr::GridAxis ax[3];
    if (const char *why = grid_axes(c1, c2, reso, ax)) return pnr::mc_fail("pnr_gen_grid_points", why);
    const long long blocks = (count + pnr::MC_THREADS - 1) / pnr::MC_THREADS;
    if (blocks > 0x7fffffffLL) return pnr_fail(PNR_E_INVALID, "pnr_gen_grid_points: count exceeds the grid limit");
    hipLaunchKernelGGL(pnr::gen_grid_points_kernel, dim3((unsigned)blocks), dim3(pnr::MC_THREADS), 0, (hipStream_t)stream, ax[0], ax[1],
                       ax[2], first, count, xyz, viewdirs);
    return pnr_check_launch("pnr_gen_grid_points");
}

extern "C" int pnr_gen_grid_points_at(const double *c1, const double *c2, const int *reso, const int32_t *ids, long long count,
                                      float *xyz, float *viewdirs, void *stream) {
    const char *entry = "pnr_gen_grid_points_at";
    pnr::GridAxis ax[3];
    if (const char *why = grid_axes(c1, c2, reso, ax)) return pnr::mc_fail(entry, why);
    if (count < 0) return pnr::mc_fail(entry, "bad sizes (count)");
    if (count == 0) return PNR_OK;
    if (!ids || !xyz) return pnr::mc_fail(entry, "ids / xyz is null");
    if (((uintptr_t)ids | (uintptr_t)xyz | (uintptr_t)viewdirs) & 3) return pnr::mc_fail(entry, "ids, xyz and viewdirs must be 4-byte aligned");
    const long long blocks = (count + pnr::MC_THREADS - 1) / pnr::MC_THREADS;
    if (blocks > 0x7fffffffLL) return pnr::mc_fail(entry, "count exceeds the launch limit");
    hipLaunchKernelGGL(pnr::gen_grid_points_at_kernel, dim3((unsigned)blocks), dim3(pnr::MC_THREADS), 0, (hipStream_t)stream, ax[0], ax[1],
                       ax[2], ids, count, xyz, viewdirs);
    return pnr_check_launch(entry);
}
