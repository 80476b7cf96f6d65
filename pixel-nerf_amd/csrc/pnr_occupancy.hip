// pnr_occupancy.hip -- occupancy-grid ray culling for gfx950 (inference).  The reference renders every ray it is given; for the
// object-centric workloads (eval/eval.py, eval/gen_video.py) most rays look through empty space.  A density grid of the encoded
// object -- sigma at the points of util.gen_grid, src/util/util.py:93-110, as src/util/recon.py:43-66 evaluates it -- becomes a
// bitfield of occupied cells (occupancy_build_kernel), rays are classified against it with a 3-D DDA (occupancy_clip_kernel), and the
// caller renders the survivors only; a culled ray gets what src/render/nerf.py:178-182,223-249 composites from sigma == 0.
// The rays that remain can also skip the network on their samples in empty cells: occupancy_mark_kernel classifies every sample,
// compact_* gathers the kept ones into a list of one-sample rays, expand_* puts the network's answers back between zeros.
// termination_mark_kernel feeds the same compaction with the samples of one stage of the fine pass whose ray has not gone opaque.
// Geometry and semantics: include/pixelnerf_hip.h.  One owner thread per output word / ray / sample, no atomics: the same bytes every run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "pnr_common.h"
#include "pnr_occgrid.h"
#include "pnr_wave.h"

namespace pnr {

constexpr int OCC_THREADS = 256;         // consecutive words / consecutive ray ids per wave: the rays of an image row are coherent
constexpr int OCC_COUNT_THREADS = 1024;  // the single workgroup that counts the occupied cells
constexpr int OCC_MAX_DILATE = 4;

typedef unsigned long long u64;

// a grid point makes its cells occupied iff its value is above the threshold or not finite (NaN, +-inf): culling errs towards
// rendering -- the opposite of pnr_mesh.hip's mc_inside, on purpose
__device__ __forceinline__ bool occ_point(float f, float thr) { return !(fabsf(f) <= 3.402823466e+38f) || f > thr; }

// One thread per 32-bit word = 32 consecutive cells (k fastest), cut into runs that stay inside one (i,j) row of cells.  A cell
// (i,j,k) is occupied iff a raw-occupied cell lies within Chebyshev distance d, i.e. iff any grid POINT of the box
// [max(0,i-d), min(nx-2,i+d)+1] x (same in j) x (same in k) passes occ_point.  Per run the (i,j) extent of that box is shared: the
// "any point of the (i,j) extent" flag of every k column goes into one 64-bit mask (a run has <= 32 cells, so <= 32 + 2d + 2 <= 42
// columns), and a cell's bit is a window of that mask.
__global__ void __launch_bounds__(OCC_THREADS)
occupancy_build_kernel(const float *__restrict__ field, int nx, int ny, int nz, float thr, int d, long long n_cells, long long n_words,
                       uint32_t *__restrict__ bits) {
    const long long w = (long long)blockIdx.x * OCC_THREADS + threadIdx.x;
    if (w >= n_words) return;
    const int cy = ny - 1, cz = nz - 1;
    long long cell = w * 32;
    const long long end = cell + 32 < n_cells ? cell + 32 : n_cells;
    uint32_t word = 0;
    while (cell < end) {
        const int k0 = (int)(cell % cz), j = (int)((cell / cz) % cy), i = (int)(cell / ((long long)cz * cy));
        const int len = (int)((end - cell) < (long long)(cz - k0) ? (end - cell) : (long long)(cz - k0));
        const int ilo = i - d > 0 ? i - d : 0, ihi = (i + d < nx - 2 ? i + d : nx - 2) + 1;
        const int jlo = j - d > 0 ? j - d : 0, jhi = (j + d < ny - 2 ? j + d : ny - 2) + 1;
        const int klo = k0 - d > 0 ? k0 - d : 0, khi = (k0 + len - 1 + d < nz - 2 ? k0 + len - 1 + d : nz - 2) + 1;
        u64 col = 0;
        for (int ii = ilo; ii <= ihi; ++ii)
            for (int jj = jlo; jj <= jhi; ++jj) {
                const float *row = field + ((size_t)ii * ny + jj) * nz;
                for (int kk = klo; kk <= khi; ++kk) col |= (u64)occ_point(row[kk], thr) << (kk - klo);
            }
        const int bit0 = (int)(cell - w * 32);
        for (int c = 0; c < len; ++c) {
            const int k = k0 + c;
            const int a = (k - d > 0 ? k - d : 0) - klo, b = (k + d < nz - 2 ? k + d : nz - 2) + 1 - klo;  // b - a + 1 <= 2d + 2 <= 10
            const u64 window = ((2ull << (b - a)) - 1ull) << a;
            word |= (uint32_t)((col & window) != 0) << (bit0 + c);
        }
        cell += len;
    }
    bits[w] = word;
}

// popcount of the bitfield by ONE workgroup: thread t adds words t, t + 1024, ...; the 16 wave sums are added in wave order
__global__ void __launch_bounds__(OCC_COUNT_THREADS)
occupancy_count_kernel(const uint32_t *__restrict__ bits, long long n_words, int *__restrict__ n_occupied) {
    __shared__ unsigned wave_tot[OCC_COUNT_THREADS / 64];
    unsigned n = 0;
    for (long long w = threadIdx.x; w < n_words; w += OCC_COUNT_THREADS) n += (unsigned)__popc(bits[w]);
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tot = 0;
        for (int v = 0; v < OCC_COUNT_THREADS / 64; ++v) tot += wave_tot[v];
        *n_occupied = (int)tot;  // < 2^31 cells
    }
}

#pragma clang fp contract(off)  // planes, differences and quotients are separately rounded: the header states them so

// plane i of axis a: c1 + i h, the last one c2 itself (as np.linspace ends on `stop`)
__device__ __forceinline__ float occ_plane(const OccGrid &g, int a, int i) { return i >= g.n[a] - 1 ? g.c2[a] : g.c1[a] + (float)i * g.h[a]; }

__global__ void __launch_bounds__(OCC_THREADS)
occupancy_clip_kernel(const float *__restrict__ rays, long long R, const uint32_t *__restrict__ bits, const OccGrid g, float pad,
                      float *__restrict__ t_bounds, int32_t *__restrict__ hit) {
    const long long r = (long long)blockIdx.x * OCC_THREADS + threadIdx.x;
    if (r >= R) return;
    const float *p = rays + (size_t)r * 8;
    const float o[3] = {p[0], p[1], p[2]}, dir[3] = {p[3], p[4], p[5]};
    const float near = p[6], far = p[7];
    float *tb = t_bounds + (size_t)r * 2;
    tb[0] = near;
    tb[1] = far;
    bool ok = occ_finite(near) && occ_finite(far) && near < far && (dir[0] != 0.f || dir[1] != 0.f || dir[2] != 0.f);
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && occ_finite(o[a]) && occ_finite(dir[a]);
    if (!ok) { hit[r] = 1; return; }  // not classifiable: render it, bounds unchanged

    // the segment inside the box [c1, c2] (slab test)
    float t0 = near, t1 = far;
    bool outside = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (dir[a] == 0.f) {
            outside = outside || o[a] < g.c1[a] || o[a] > g.c2[a];
        } else {
            const float ta = (g.c1[a] - o[a]) / dir[a], tc = (g.c2[a] - o[a]) / dir[a];
            t0 = fmaxf(t0, fminf(ta, tc));
            t1 = fminf(t1, fmaxf(ta, tc));
        }
    }
    if (t0 != t0 || t1 != t1) { hit[r] = 1; return; }  // (overflowed differences: not classifiable either)
    if (outside || !(t0 < t1)) { hit[r] = 0; return; }

    // the cell of the segment's first point, the DDA's state per axis: step, parameter of the next plane
    int idx[3], step[3];
    float tnext[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = o[a] + t0 * dir[a];
        const float c = floorf((x - g.c1[a]) / g.h[a]);
        idx[a] = (int)fminf(fmaxf(c, 0.f), (float)(g.n[a] - 2));
        step[a] = dir[a] > 0.f ? 1 : -1;
        tnext[a] = dir[a] == 0.f ? INFINITY : (occ_plane(g, a, idx[a] + (dir[a] > 0.f ? 1 : 0)) - o[a]) / dir[a];
    }
    const int cy = g.n[1] - 1, cz = g.n[2] - 1;
    const int max_cells = (g.n[0] - 1) + cy + cz;
    float t = t0, t_enter = 0.f, t_exit = 0.f;
    bool any = false;
    for (int s = 0; s < max_cells; ++s) {
        const float tout = fminf(fminf(tnext[0], tnext[1]), tnext[2]);
        const long long cell = ((long long)idx[0] * cy + idx[1]) * cz + idx[2];
        if (bits[cell >> 5] >> (cell & 31) & 1u) {
            if (!any) t_enter = t;
            any = true;
            t_exit = fmaxf(t, fminf(tout, t1));
        }
        if (!(tout < t1)) break;
        // the axis whose plane comes first (ties: x, then y -- the cell in between is visited with zero length); selects, not
        // indexing by a run-time axis, keep the three-element arrays in registers
        const bool sx = tnext[0] <= tnext[1] && tnext[0] <= tnext[2], sy = !sx && tnext[1] <= tnext[2];
        const int ni = sx ? idx[0] + step[0] : sy ? idx[1] + step[1] : idx[2] + step[2];
        if (ni < 0 || ni > (sx ? g.n[0] : sy ? g.n[1] : g.n[2]) - 2) break;  // left the box
        t = fmaxf(t, tout);
        if (sx) { idx[0] = ni; tnext[0] = (occ_plane(g, 0, ni + (step[0] > 0 ? 1 : 0)) - o[0]) / dir[0]; }
        else if (sy) { idx[1] = ni; tnext[1] = (occ_plane(g, 1, ni + (step[1] > 0 ? 1 : 0)) - o[1]) / dir[1]; }
        else { idx[2] = ni; tnext[2] = (occ_plane(g, 2, ni + (step[2] > 0 ? 1 : 0)) - o[2]) / dir[2]; }
    }
    hit[r] = any ? 1 : 0;
    if (any) {
        tb[0] = fmaxf(near, t_enter - pad);
        tb[1] = fminf(far, t_exit + pad);
    }
}

// ---- per-sample skipping: mark the samples in occupied cells, compact them, put the network's answers back ----
// One thread per sample, consecutive samples of a ray in consecutive lanes: the z reads are coalesced, the ray row is a broadcast.
// The point is ray_point's (pnr_geom.h): o + z d, the product and the sum rounded separately (contraction is off here).
__global__ void __launch_bounds__(OCC_THREADS)
occupancy_mark_kernel(const float *__restrict__ rays, const float *__restrict__ z, int K, int N, const uint32_t *__restrict__ bits,
                      const OccGrid g, uint8_t *__restrict__ keep) {
    const long long t = (long long)blockIdx.x * OCC_THREADS + threadIdx.x;
    if (t >= N) return;
    const int s = (int)t;
    const float *p = rays + (size_t)(s / K) * 8;
    const float zz = z[s];
    bool finite = occ_finite(zz), inside = true;
    int idx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float o = p[a], d = p[3 + a];
        finite = finite && occ_finite(o) && occ_finite(d);
        const float x = o + zz * d;
        inside = inside && x >= g.c1[a] && x <= g.c2[a];
        const float c = floorf((x - g.c1[a]) / g.h[a]);
        idx[a] = (int)fminf(fmaxf(c, 0.f), (float)(g.n[a] - 2));  // (fmaxf drops a NaN: always a cell of the grid)
    }
    const long long cell = ((long long)idx[0] * (g.n[1] - 1) + idx[1]) * (g.n[2] - 1) + idx[2];
    const bool occupied = inside && (bits[cell >> 5] >> (cell & 31) & 1u);
    keep[s] = (uint8_t)(!finite || occupied);  // not classifiable: evaluate it
}
#pragma clang fp contract(fast)

// Compaction, three launches in stream order.  A workgroup owns OCC_THREADS consecutive samples; no workgroup waits on another.
// (1) kept samples per workgroup: one ballot per wave, the 4 wave counts added in wave order.
__global__ void __launch_bounds__(OCC_THREADS)
compact_count_kernel(const uint8_t *__restrict__ keep, int N, int *__restrict__ totals) {
    __shared__ int wave_tot[OCC_THREADS / 64];
    const long long s = (long long)blockIdx.x * OCC_THREADS + threadIdx.x;
    const u64 m = __ballot(s < N && keep[s < N ? s : 0] != 0);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int v = 0; v < OCC_THREADS / 64; ++v) tot += wave_tot[v];
        totals[blockIdx.x] = tot;
    }
}

// (2) exclusive scan of the totals, in place, by ONE workgroup that walks them OCC_THREADS at a time with a running carry; the grand
// total is M
__global__ void __launch_bounds__(OCC_THREADS)
compact_scan_kernel(int *__restrict__ totals, int n_groups, int *__restrict__ count) {
    __shared__ int wave_tot[OCC_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;  // (the same value in every thread)
    for (int base = 0; base < n_groups; base += OCC_THREADS) {
        const int i = base + threadIdx.x;
        const int v = i < n_groups ? totals[i] : 0;
        const int incl = wave_scan_add(v, lane);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int off = carry, all = 0;
        for (int u = 0; u < OCC_THREADS / 64; ++u) {
            if (u < wave) off += wave_tot[u];
            all += wave_tot[u];
        }
        if (i < n_groups) totals[i] = off + incl - v;
        carry += all;
        __syncthreads();  // wave_tot is rewritten by the next round
    }
    if (threadIdx.x == 0) *count = carry;  // < 2^31 samples
}

// (3) the scatter: rank inside the wave from the ballot, the waves before it from LDS, the workgroups before it from the scan
__global__ void __launch_bounds__(OCC_THREADS)
compact_scatter_kernel(const uint8_t *__restrict__ keep, const float *__restrict__ rays, const float *__restrict__ z, int K, int N,
                       const int *__restrict__ offsets, int32_t *__restrict__ index, float *__restrict__ rays_c, float *__restrict__ z_c) {
    __shared__ int wave_tot[OCC_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long s = (long long)blockIdx.x * OCC_THREADS + threadIdx.x;
    const bool k = s < N && keep[s < N ? s : 0] != 0;
    const u64 m = __ballot(k);
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    if (!k) return;
    int at = offsets[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int u = 0; u < wave; ++u) at += wave_tot[u];
    index[at] = (int32_t)s;
    z_c[at] = z[s];
    const float4 *row = reinterpret_cast<const float4 *>(rays) + (size_t)(s / K) * 2;
    float4 *out = reinterpret_cast<float4 *>(rays_c) + (size_t)at * 2;
    out[0] = row[0];
    out[1] = row[1];
}

__global__ void __launch_bounds__(OCC_THREADS)
expand_zero_kernel(float4 *__restrict__ rgbsigma, long long N) {
    const long long s = (long long)blockIdx.x * OCC_THREADS + threadIdx.x;
    if (s < N) rgbsigma[s] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void __launch_bounds__(OCC_THREADS)
expand_scatter_kernel(const int32_t *__restrict__ index, const float4 *__restrict__ rgbsigma_c, int M, long long N,
                      float4 *__restrict__ rgbsigma) {
    const long long m = (long long)blockIdx.x * OCC_THREADS + threadIdx.x;
    if (m >= M) return;
    const long long s = index[m];
    if (s >= 0 && s < N) rgbsigma[s] = rgbsigma_c[m];  // (a row outside the output is the caller's error: skipped)
}

// ---- early ray termination: which samples of a stage still need the network ----
constexpr int TERM_WAVES = 4;  // rays per workgroup, one wavefront each (composite_kernel's shape)

// One wavefront per ray.  The transmittance in front of sample k_begin is composite_kernel's own value for that sample, formed
// the same way: chunks of 64 samples, the factor 1 - alpha + 1e-10 per lane, an inclusive product scan, the chunk totals carried
// (lane l of a scan reads lanes <= l only, so the lanes at and behind k_begin, which hold 1, do not enter).  Then the wave writes
// the ray's K keep bytes.  No atomics, no LDS, nothing behind k_begin is read from rgbsigma.
__global__ void __launch_bounds__(TERM_WAVES * 64)
termination_mark_kernel(const float *__restrict__ rays, const float *__restrict__ z, const float *__restrict__ rgbsigma, int R, int K,
                        int k_begin, int k_end, float eps, const uint8_t *__restrict__ keep_in, uint8_t *__restrict__ keep,
                        float *__restrict__ t_front) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * TERM_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;
    const float *zr = z + (size_t)r * K;
    float T = 1.f;  // prod_{j < c0} (1 - a_j + 1e-10), then of every j < k_begin
    for (int c0 = 0; c0 < k_begin; c0 += 64) {
        const int i = c0 + lane;
        float tfac = 1.f;
        if (i < k_begin) {
            const float znext = (i + 1 < K) ? zr[i + 1] : rays[(size_t)r * 8 + 7];  // nerf.py:181: the last delta is far - z_last
            const float delta = znext - zr[i];
            const float alpha = 1.f - expf(-delta * fmaxf(rgbsigma[((size_t)r * K + i) * 4 + 3], 0.f));  // :228
            tfac = 1.f - alpha + 1e-10f;                                                                  // :230-232
        }
        const float incl = wave_scan_mul(tfac, lane);
        const int last = k_begin - c0 < 64 ? k_begin - c0 - 1 : 63;  // the last lane in front of k_begin
        T = T * __shfl(incl, last, 64);
    }
    const bool alive = !(T <= eps);  // a NaN transmittance does not stop the ray
    if (t_front && lane == 0) t_front[r] = T;
    for (int k = lane; k < K; k += 64) {
        const size_t s = (size_t)r * K + k;
        keep[s] = (uint8_t)(alive && k >= k_begin && k < k_end && (!keep_in || keep_in[s] != 0));
    }
}

}  // namespace pnr

extern "C" size_t pnr_occupancy_bytes(int nx, int ny, int nz) {
    if (pnr::occ_bad_dims(nx, ny, nz)) return 0;
    const long long cells = (long long)(nx - 1) * (ny - 1) * (nz - 1);
    return (size_t)((cells + 31) / 32) * 4;
}

extern "C" int pnr_occupancy_build(const float *field, int nx, int ny, int nz, float threshold, int dilate, uint32_t *bits,
                                   int *n_occupied_dev, void *stream) {
    if (const char *why = pnr::occ_bad_dims(nx, ny, nz)) return pnr::occ_fail("pnr_occupancy_build", why);
    if (dilate < 0 || dilate > pnr::OCC_MAX_DILATE) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_build: dilate must be in [0, 4]");
    if (threshold != threshold) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_build: threshold is NaN");
    if (!field) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_build: field is null");
    if (!bits) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_build: bits is null");
    const long long cells = (long long)(nx - 1) * (ny - 1) * (nz - 1), words = (cells + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pnr::occupancy_build_kernel, dim3((unsigned)((words + pnr::OCC_THREADS - 1) / pnr::OCC_THREADS)),
                       dim3(pnr::OCC_THREADS), 0, st, field, nx, ny, nz, threshold, dilate, cells, words, bits);
    if (n_occupied_dev)
        hipLaunchKernelGGL(pnr::occupancy_count_kernel, dim3(1), dim3(pnr::OCC_COUNT_THREADS), 0, st, bits, words, n_occupied_dev);
    return pnr_check_launch("pnr_occupancy_build");
}

extern "C" int pnr_occupancy_clip_rays(const float *rays, long long R, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                       const float *c2, float pad, float *t_bounds, int32_t *hit, void *stream) {
    if (const char *why = pnr::occ_bad_dims(nx, ny, nz)) return pnr::occ_fail("pnr_occupancy_clip_rays", why);
    if (R < 0) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_clip_rays: bad sizes");
    if (!(pad >= 0.f) || !std::isfinite(pad)) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_clip_rays: pad must be finite and >= 0");
    pnr::OccGrid g;
    if (const char *why = pnr::occ_grid(nx, ny, nz, c1, c2, g)) return pnr::occ_fail("pnr_occupancy_clip_rays", why);
    if (R == 0) return PNR_OK;
    if (!rays || !bits || !t_bounds || !hit) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_clip_rays: null argument");
    const long long blocks = (R + pnr::OCC_THREADS - 1) / pnr::OCC_THREADS;
    if (blocks > 0x7fffffffLL) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_clip_rays: R exceeds the launch limit");
    hipLaunchKernelGGL(pnr::occupancy_clip_kernel, dim3((unsigned)blocks), dim3(pnr::OCC_THREADS), 0, (hipStream_t)stream, rays, R, bits, g,
                       pad, t_bounds, hit);
    return pnr_check_launch("pnr_occupancy_clip_rays");
}

extern "C" int pnr_occupancy_mark_samples(const float *rays, const float *z, int R, int K, const uint32_t *bits, int nx, int ny, int nz,
                                          const float *c1, const float *c2, uint8_t *keep, void *stream) {
    if (const char *why = pnr::occ_bad_dims(nx, ny, nz)) return pnr::occ_fail("pnr_occupancy_mark_samples", why);
    if (R < 0 || K < 1) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_mark_samples: bad sizes");
    if ((long long)R * K >= (1LL << 31)) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_mark_samples: R * K must be below 2^31");
    pnr::OccGrid g;
    if (const char *why = pnr::occ_grid(nx, ny, nz, c1, c2, g)) return pnr::occ_fail("pnr_occupancy_mark_samples", why);
    if (R == 0) return PNR_OK;
    if (!rays || !z || !bits || !keep) return pnr_fail(PNR_E_INVALID, "pnr_occupancy_mark_samples: null argument");
    const int N = R * K;
    hipLaunchKernelGGL(pnr::occupancy_mark_kernel, dim3((unsigned)(((long long)N + pnr::OCC_THREADS - 1) / pnr::OCC_THREADS)),
                       dim3(pnr::OCC_THREADS), 0, (hipStream_t)stream, rays, z, K, N, bits, g, keep);
    return pnr_check_launch("pnr_occupancy_mark_samples");
}

extern "C" int pnr_termination_mark(const float *rays, const float *z, const float *rgbsigma, int R, int K, int k_begin, int k_end,
                                    float eps, const uint8_t *keep_in, uint8_t *keep, float *t_front, void *stream) {
    if (R < 0 || K < 1) return pnr_fail(PNR_E_INVALID, "pnr_termination_mark: bad sizes");
    if ((long long)R * K >= (1LL << 31)) return pnr_fail(PNR_E_INVALID, "pnr_termination_mark: R * K must be below 2^31");
    if (k_begin < 0 || k_begin > k_end || k_end > K)
        return pnr_fail(PNR_E_INVALID, "pnr_termination_mark: the stage must satisfy 0 <= k_begin <= k_end <= K");
    if (!(eps > 0.f && eps < 1.f)) return pnr_fail(PNR_E_INVALID, "pnr_termination_mark: eps must lie in (0, 1)");  // (refuses a NaN)
    if (R == 0) return PNR_OK;
    if (!rays || !z || !rgbsigma || !keep) return pnr_fail(PNR_E_INVALID, "pnr_termination_mark: null argument");
    hipLaunchKernelGGL(pnr::termination_mark_kernel, dim3((unsigned)((R + pnr::TERM_WAVES - 1) / pnr::TERM_WAVES)),
                       dim3(pnr::TERM_WAVES * 64), 0, (hipStream_t)stream, rays, z, rgbsigma, R, K, k_begin, k_end, eps, keep_in, keep, t_front);
    return pnr_check_launch("pnr_termination_mark");
}

extern "C" size_t pnr_compact_samples_workspace_bytes(long long N) {
    if (N <= 0 || N >= (1LL << 31)) return 0;
    return (size_t)((N + pnr::OCC_THREADS - 1) / pnr::OCC_THREADS) * sizeof(int);
}

extern "C" int pnr_compact_samples(const uint8_t *keep, const float *rays, const float *z, int R, int K, int32_t *index, float *rays_c,
                                   float *z_c, int *count_dev, void *workspace, size_t workspace_bytes, void *stream) {
    if (R < 0 || K < 1) return pnr_fail(PNR_E_INVALID, "pnr_compact_samples: bad sizes");
    if ((long long)R * K >= (1LL << 31)) return pnr_fail(PNR_E_INVALID, "pnr_compact_samples: R * K must be below 2^31");
    if (R == 0) return PNR_OK;
    if (!keep || !rays || !z || !index || !rays_c || !z_c || !count_dev || !workspace)
        return pnr_fail(PNR_E_INVALID, "pnr_compact_samples: null argument");
    if (pnr::occ_misaligned16(rays) || pnr::occ_misaligned16(rays_c))
        return pnr_fail(PNR_E_INVALID, "pnr_compact_samples: rays and rays_c must be 16-byte aligned");
    const int N = R * K;
    if (workspace_bytes < pnr_compact_samples_workspace_bytes(N) || (reinterpret_cast<uintptr_t>(workspace) & 3u))
        return pnr_fail(PNR_E_INVALID, "pnr_compact_samples: workspace smaller than pnr_compact_samples_workspace_bytes(R * K), or not 4-byte aligned");
    const int groups = (int)(((long long)N + pnr::OCC_THREADS - 1) / pnr::OCC_THREADS);
    int *totals = static_cast<int *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pnr::compact_count_kernel, dim3((unsigned)groups), dim3(pnr::OCC_THREADS), 0, st, keep, N, totals);
    hipLaunchKernelGGL(pnr::compact_scan_kernel, dim3(1), dim3(pnr::OCC_THREADS), 0, st, totals, groups, count_dev);
    hipLaunchKernelGGL(pnr::compact_scatter_kernel, dim3((unsigned)groups), dim3(pnr::OCC_THREADS), 0, st, keep, rays, z, K, N,
                       (const int *)totals, index, rays_c, z_c);
    return pnr_check_launch("pnr_compact_samples");
}

extern "C" int pnr_expand_rgbsigma(const int32_t *index, const float *rgbsigma_c, int M, long long N, float *rgbsigma, void *stream) {
    if (M < 0 || N < 0 || (long long)M > N) return pnr_fail(PNR_E_INVALID, "pnr_expand_rgbsigma: bad sizes (0 <= M <= N)");
    if (N >= (1LL << 31)) return pnr_fail(PNR_E_INVALID, "pnr_expand_rgbsigma: N must be below 2^31");
    if (N == 0) return PNR_OK;
    if (!rgbsigma || (M > 0 && (!index || !rgbsigma_c))) return pnr_fail(PNR_E_INVALID, "pnr_expand_rgbsigma: null argument");
    if (pnr::occ_misaligned16(rgbsigma) || (M > 0 && pnr::occ_misaligned16(rgbsigma_c)))
        return pnr_fail(PNR_E_INVALID, "pnr_expand_rgbsigma: rgbsigma and rgbsigma_c must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pnr::expand_zero_kernel, dim3((unsigned)((N + pnr::OCC_THREADS - 1) / pnr::OCC_THREADS)), dim3(pnr::OCC_THREADS), 0, st,
                       reinterpret_cast<float4 *>(rgbsigma), N);
    if (M > 0)
        hipLaunchKernelGGL(pnr::expand_scatter_kernel, dim3((unsigned)((M + pnr::OCC_THREADS - 1) / pnr::OCC_THREADS)), dim3(pnr::OCC_THREADS), 0,
                           st, index, reinterpret_cast<const float4 *>(rgbsigma_c), M, N, reinterpret_cast<float4 *>(rgbsigma));
    return pnr_check_launch("pnr_expand_rgbsigma");
}
