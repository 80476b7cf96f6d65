// pnr_meshfinish.hip -- what a density grid and its mesh still need before they are usable, for gfx950: the connected components
// of the grid's inside voxels (to drop the stray blobs a trained network leaves around the object, recon.remove_floaters and
// OccupancyGrid.from_density(keep_largest=)) and the field's gradient at the mesh vertices (vertex normals).  Nothing in the
// reference corresponds: src/util/recon.py:68-106 meshes whatever the grid holds and writes bare vertices.
// Semantics: include/pixelnerf_hip.h.  The library allocates nothing: every buffer is the caller's.
//
// Labelling: a lock-free union-find over `labels` (L) in global memory, three launches in stream order.
//   init    L[x] = inside(x) ? x : -1, sizes[x] = 0, counts = 0
//   union   every inside voxel unites itself with its inside +x, +y, +z neighbours
//   flatten L[x] = find(x); the component sizes and the two counts with integer atomics (they commute exactly)
// find follows L down to a fixed point; unite links the LARGER root under the smaller one with an atomic minimum and, when the
// value the atomic returns shows that the larger root had meanwhile been linked elsewhere, goes on from that returned value.
//   Invariant A: every value ever stored in L[x] of an inside voxel is <= x and >= 0 (init stores x; the atomic minimum only
//     lowers, and its operand is a root found from a neighbour, >= 0).  So every chain strictly descends and ends after at most x
//     steps, and every retry of unite starts from a strictly smaller pair (old < a): no loop waits for another thread.
//   Invariant B: the smallest index m of a component is never linked under anything -- the operand of an atomic minimum on L[m]
//     would be a root of the same component below m.  So L[m] == m for ever, the root that survives is m, and the labels are the
//     same bytes on every run whatever the scheduling.
// A stale or racing read of L[x] still yields a value some thread stored there, i.e. an ancestor-to-be of x within its component
// (A), so it costs steps, never correctness: the linking itself goes through the atomic's return value.  L is read inside the
// loops with relaxed agent-scope atomic loads (never from a line a CU cached before another CU's atomic).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "pnr_common.h"
#include "pnr_wave.h"

namespace pnr {

constexpr int MF_THREADS = 256;  // consecutive voxels (z fastest) / consecutive vertices per workgroup

__device__ __forceinline__ bool mf_finite(float f) { return fabsf(f) <= 3.402823466e+38f; }
// the mesher's rule (pnr_mesh.hip, mc_inside): finite and above the level; a value equal to it is outside
__device__ __forceinline__ bool mf_inside(float f, float thr) { return mf_finite(f) && f > thr; }

__device__ __forceinline__ int mf_load(const int *L, int x) { return __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as far as this thread can see: at most x steps (invariant A)
__device__ __forceinline__ int mf_find(const int *L, int x) {
    for (;;) {
        const int p = mf_load(L, x);
        if (p == x) return x;
        x = p;
    }
}

// a and b are inside voxels of one component.  Every pass either ends or replaces the larger root a by a value below it.
__device__ __forceinline__ void mf_unite(int *L, int a, int b) {
    for (;;) {
        a = mf_find(L, a);
        b = mf_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;  // a was still a root and now hangs under b
        a = old;               // a had been linked under old < a meanwhile (L[a] is now min(old, b)): unite old's tree with b's
    }
}

__global__ void __launch_bounds__(MF_THREADS)
components_init_kernel(const float *__restrict__ field, int N, float thr, int *__restrict__ L, int *__restrict__ sizes,
                       int *__restrict__ counts) {
    const long long p = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
    if (p == 0 && counts) { counts[0] = 0; counts[1] = 0; }
    if (p >= N) return;
    L[p] = mf_inside(field[p], thr) ? (int)p : -1;
    if (sizes) sizes[p] = 0;
}

__global__ void __launch_bounds__(MF_THREADS)
components_union_kernel(int nx, int ny, int nz, int *L) {
    const long long N = (long long)nx * ny * nz;
    const long long q = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
    if (q >= N) return;
    const int p = (int)q;
    if (mf_load(L, p) < 0) return;  // (outside voxels hold -1 from the init launch and are never written again)
    const int sy = nz, sx = ny * nz;  // nx ny nz < 2^31
    const int k = p % nz, j = (p / nz) % ny, i = p / sx;
    if (k + 1 < nz && mf_load(L, p + 1) >= 0) mf_unite(L, p, p + 1);
    if (j + 1 < ny && mf_load(L, p + sy) >= 0) mf_unite(L, p, p + sy);
    if (i + 1 < nx && mf_load(L, p + sx) >= 0) mf_unite(L, p, p + sx);
}

// L[x] = its root.  A voxel another thread has not flattened yet still holds an ancestor (A), a root holds itself (B): find is
// right before, during and after.  sizes: the lanes of a wave hold consecutive voxels, a run of equal labels adds its length once
// (its first lane does); counts: one add per wave.  No lane leaves before the cross-lane operations.
__global__ void __launch_bounds__(MF_THREADS)
components_flatten_kernel(int N, int *L, int *__restrict__ sizes, int *__restrict__ counts) {
    const long long q = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int lab = -1;
    if (q < N && mf_load(L, (int)q) >= 0) {
        lab = mf_find(L, (int)q);
        __hip_atomic_store(L + q, lab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (sizes) {
        const int prev = __shfl_up(lab, 1, 64);
        const bool head = lane == 0 || prev != lab;
        const unsigned long long heads = __ballot(head);
        if (head && lab >= 0) {
            const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
            const int len = rest ? __ffsll((long long)rest) : 64 - lane;  // up to the next run's first lane, or the wave's end
            atomicAdd(sizes + lab, len);
        }
    }
    if (counts) {
        const int n_in = wave_sum(lab >= 0 ? 1 : 0), n_root = wave_sum(lab >= 0 && lab == (int)q ? 1 : 0);
        if (lane == 0 && n_in) {
            atomicAdd(counts, n_in);
            if (n_root) atomicAdd(counts + 1, n_root);
        }
    }
}

#pragma clang fp contract(off)  // every difference, product and quotient below is separately rounded: the header states them so

struct MfGrid {
    float c1[3], scale[3];
    int n[3];
};

// d f / d index along one axis at a grid point: central difference, one-sided at the border (n >= 2)
__device__ __forceinline__ float mf_diff(const float *__restrict__ f, long long at, long long stride, int i, int n) {
    const bool lo = i > 0, hi = i < n - 1;
    const float d = f[hi ? at + stride : at] - f[lo ? at - stride : at];
    return lo && hi ? d * 0.5f : d;
}

__device__ __forceinline__ float mf_lerp(float a, float b, float t) { return a + t * (b - a); }

__global__ void __launch_bounds__(MF_THREADS)
grid_normals_kernel(const float *__restrict__ field, const MfGrid g, const float *__restrict__ vertices, long long V,
                    float *__restrict__ normals) {
    const long long v = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
    if (v >= V) return;
    int c[3];
    float t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float p = (vertices[3 * v + a] - g.c1[a]) / g.scale[a];
        p = fminf(fmaxf(p, 0.f), (float)(g.n[a] - 1));  // (a NaN coordinate lands on 0: every read stays in the grid)
        const int ci = (int)floorf(p);
        c[a] = ci < g.n[a] - 2 ? ci : g.n[a] - 2;
        t[a] = p - (float)c[a];
    }
    const long long sy = g.n[2], sx = (long long)g.n[1] * g.n[2];
    float gr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float corner[8];  // dx + 2 dy + 4 dz
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = c[0] + (q & 1), j = c[1] + (q >> 1 & 1), k = c[2] + (q >> 2);
            const long long at = i * sx + j * sy + k;
            corner[q] = a == 0 ? mf_diff(field, at, sx, i, g.n[0]) : a == 1 ? mf_diff(field, at, sy, j, g.n[1]) : mf_diff(field, at, 1, k, g.n[2]);
        }
        // trilinear blend: along x, then y, then z
        const float x00 = mf_lerp(corner[0], corner[1], t[0]), x10 = mf_lerp(corner[2], corner[3], t[0]);
        const float x01 = mf_lerp(corner[4], corner[5], t[0]), x11 = mf_lerp(corner[6], corner[7], t[0]);
        gr[a] = mf_lerp(mf_lerp(x00, x10, t[1]), mf_lerp(x01, x11, t[1]), t[2]) / g.scale[a];
    }
    // the norm through fp64, as pnr_mesh.hip's view directions: neither overflow nor a rounding worth mentioning
    const double nrm = sqrt((double)gr[0] * gr[0] + (double)gr[1] * gr[1] + (double)gr[2] * gr[2]);
    const bool ok = nrm > 0.0 && nrm <= 1.7976931348623157e308;  // (false for NaN too)
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * v + a] = ok ? (float)(-(double)gr[a] / nrm) : 0.f;
}
#pragma clang fp contract(fast)

}  // namespace pnr

extern "C" int pnr_grid_components(const float *field, int nx, int ny, int nz, float threshold, int *labels, int *sizes,
                                   int *counts_dev, void *stream) {
    if (nx < 1 || ny < 1 || nz < 1) return pnr_fail(PNR_E_INVALID, "pnr_grid_components: every axis needs at least 1 grid point");
    if ((long long)nx * ny >= (1LL << 31) || (long long)nx * ny * nz >= (1LL << 31))
        return pnr_fail(PNR_E_INVALID, "pnr_grid_components: nx ny nz must stay below 2^31 (labels are int32)");
    if (threshold != threshold) return pnr_fail(PNR_E_INVALID, "pnr_grid_components: threshold is NaN");
    if (!field || !labels) return pnr_fail(PNR_E_INVALID, "pnr_grid_components: field / labels is null");
    const int N = nx * ny * nz;
    const dim3 grid((unsigned)(((long long)N + pnr::MF_THREADS - 1) / pnr::MF_THREADS)), block(pnr::MF_THREADS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pnr::components_init_kernel, grid, block, 0, st, field, N, threshold, labels, sizes, counts_dev);
    hipLaunchKernelGGL(pnr::components_union_kernel, grid, block, 0, st, nx, ny, nz, labels);
    hipLaunchKernelGGL(pnr::components_flatten_kernel, grid, block, 0, st, N, labels, sizes, counts_dev);
    return pnr_check_launch("pnr_grid_components");
}

extern "C" int pnr_grid_normals(const float *field, int nx, int ny, int nz, const float *c1, const float *scale,
                                const float *vertices, long long V, float *normals, void *stream) {
    if (nx < 2 || ny < 2 || nz < 2) return pnr_fail(PNR_E_INVALID, "pnr_grid_normals: every axis needs at least 2 grid points");
    if ((long long)nx * ny >= (1LL << 31) || (long long)nx * ny * nz >= (1LL << 31))
        return pnr_fail(PNR_E_INVALID, "pnr_grid_normals: nx ny nz must stay below 2^31");
    if (!c1 || !scale) return pnr_fail(PNR_E_INVALID, "pnr_grid_normals: c1 / scale is null (host arrays of 3 floats)");
    pnr::MfGrid g;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(c1[a])) return pnr_fail(PNR_E_INVALID, "pnr_grid_normals: c1 must be finite");
        if (!std::isfinite(scale[a]) || scale[a] == 0.f) return pnr_fail(PNR_E_INVALID, "pnr_grid_normals: scale must be finite and not zero");
        g.c1[a] = c1[a];
        g.scale[a] = scale[a];
    }
    g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
    if (V < 0) return pnr_fail(PNR_E_INVALID, "pnr_grid_normals: V is negative");
    if (V == 0) return PNR_OK;
    if (!field || !vertices || !normals) return pnr_fail(PNR_E_INVALID, "pnr_grid_normals: field / vertices / normals is null");
    const long long blocks = (V + pnr::MF_THREADS - 1) / pnr::MF_THREADS;
    if (blocks > 0x7fffffffLL) return pnr_fail(PNR_E_INVALID, "pnr_grid_normals: V exceeds the grid limit");
    hipLaunchKernelGGL(pnr::grid_normals_kernel, dim3((unsigned)blocks), dim3(pnr::MF_THREADS), 0, (hipStream_t)stream, field, g,
                       vertices, V, normals);
    return pnr_check_launch("pnr_grid_normals");
}
