// pnr_baked.h -- what every march through a baked volume shares (pnr_baked.hip, pnr_baked_grad.hip, pnr_baked_scene.hip,
// pnr_baked_tv.hip, pnr_baked_visibility.hip, pnr_baked_resample.hip).  Semantics: include/pixelnerf_hip.h ("baked volumes").
// Structure.  Device: ONE march (baked_march, pnr_baked.hip) and ONE kernel template (baked_march_kernel<Corner, Rows>) around it.
// Corner says what the march reads at a corner of a cell (RgbaCornerOf / ShCorner<B>) and what a stored number is (float4 or Half4,
// widened exactly on load: everything after the load is the same code); Rows says where a pair of corners lies (DenseRows: rows
// p, p + 1 of the dense array; SparseRows: rows index[p], index[p] + 1 of the kept ones).  4 kinds x 2 storages x 2 layouts = 16
// kernels.  The per-sample part of the march -- the point, its cell and fractions, whether it contributes, the rows of its corners,
// the blend, alpha -- lives in device functions here that every kernel of the family calls, so the backward's samples are the
// forward's and a scene of one object at the identity is the single march.  Some pieces stand IN PLACE in more than one kernel,
// each with a comment that names the measurement that keeps it there (profiles/baked_notes.md, "A file per concern"): the five
// lines of the sample count and the compositing of a chunk with the pixel write in the two forward kernels, the scene forward's
// two object loops and per-object steps, and the walk of the backward (upstream gradient, first walk, scan step, corner weights, row
// write) in the three backward kernels.
// Host: an entry builds its ray source (baked_explicit_rays / baked_camera_rays: the checks of the rays travel with them), says
// what it was handed (BakedVolumeDesc: pointer, degree, storage, index + M, and the words of its refusals) and calls its family's
// function, which runs baked_check -- every check, in one order for all entries -- and baked_dispatch, which decides layout,
// storage and kind once each.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "pnr_common.h"
#include "pnr_occgrid.h"
#include "pnr_raysrc.h"
#include "pnr_wave.h"

namespace pnr {

// A 128 x 128 view is 16 k rays: one THREAD per ray would leave one wave on each CU and nothing to hide the latency of the corner
// gathers behind.  One WAVE per ray gives 16 k waves, lane l of chunk c takes sample 64 c + l, so 64 x 8 independent 16-byte
// loads are in flight per wave.
constexpr int BAKED_WAVES = 4;             // rays per workgroup
constexpr float BAKED_MAX_SAMPLES = 1048576.f;  // 2^20 samples per ray; (float)i + 0.5f is exact far beyond it

struct BakedParams {
    const uint32_t *bits;  // pnr_occupancy_build's bitfield of the same grid, or NULL
    OccGrid g;
    float step, eps;       // eps == 0: no termination
    int white_bkgd;
};

#pragma clang fp contract(off)  // every product, sum and quotient below is rounded on its own: the header states them so

// a + f (b - a) on all four channels
__device__ __forceinline__ float4 baked_lerp(const float4 a, const float4 b, float f) {
    return make_float4(a.x + f * (b.x - a.x), a.y + f * (b.y - a.y), a.z + f * (b.z - a.z), a.w + f * (b.w - a.w));
}

// What a stored (r,g,b,sigma) is: a float4, or four fp16 numbers in 8 bytes (the half entries).  baked_widen is the ONLY place the
// two differ: fp16 -> fp32 is exact (one v_cvt_f32_f16 per component; subnormals, -0 and 65504 keep their value), so the march of
// a half volume performs the fp32 march's operations on the widened values and gives its bytes.  One 8-byte load per coefficient:
// legal at every point (a pair of corners is 16-byte aligned only where the point's parity allows).
struct alignas(8) Half4 {
    _Float16 x, y, z, w;
};
__device__ __forceinline__ float4 baked_widen(const float4 v) { return v; }
__device__ __forceinline__ float4 baked_widen(const Half4 v) { return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w); }

// the backward's scatter: one fp32 atomic per channel of a stored (r,g,b,sigma), exact zeros skipped (most of a clamped corner)
__device__ __forceinline__ void baked_add4(float *__restrict__ dst, const float4 g) {
    if (g.x != 0.f) atomicAdd(dst + 0, g.x);
    if (g.y != 0.f) atomicAdd(dst + 1, g.y);
    if (g.z != 0.f) atomicAdd(dst + 2, g.z);
    if (g.w != 0.f) atomicAdd(dst + 3, g.w);
}

// What the march reads at a corner of a cell; `data` is the stored array the entry was handed (the kernel sets it).  RGBA volume:
// the (r,g,b,sigma) of the grid point.
template <class Stored>
struct RgbaCornerOf {
    using stored_t = Stored;
    const Stored *data;  // (nx,ny,nz) x (r,g,b,sigma)
    __device__ __forceinline__ void set_ray(const Ray8 &) {}
    static constexpr int PAIRS_IN_FLIGHT = 4;  // 8 loads: all in flight at once
    __device__ __forceinline__ float4 at(long long point) const { return baked_widen(data[point]); }
    // backward: g = weight x dL/d(blended value) of this corner goes to the stored numbers as it is (no clamp, no relu)
    __device__ __forceinline__ void scatter(float *__restrict__ d_stored, long long point, const float4 g) const {
        baked_add4(d_stored + point * 4, g);
    }
};

// fp32(sqrt 3), fp32(sqrt 15), fp32(sqrt 5 / 2), fp32(sqrt 15 / 2): rounded once from the fp64 values
constexpr float SH_C1 = 1.7320508075688772f, SH_C2 = 3.872983346207417f, SH_C20 = 1.118033988749895f, SH_C22 = 1.9364916731037085f;

// SH volume: the B contiguous float4s of the grid point, reduced with the ray's basis values to one float4 and clamped.  y[k - 1]
// holds Y_k of the header for k >= 1 (Y_0 = 1 is not stored: c * 1 is c); a per-ray constant.
template <int B, class Stored>
struct ShCorner {
    using stored_t = Stored;
    const Stored *data;  // (nx,ny,nz,B) x (r,g,b,sigma)
    float y[B > 1 ? B - 1 : 1];
    __device__ __forceinline__ void set_ray(const Ray8 &ray) {
        const float n2 = ray.dx * ray.dx + ray.dy * ray.dy + ray.dz * ray.dz;
        const bool ok = occ_finite(n2) && n2 != 0.f;
        const float s = sqrtf(n2);
        const float x = ray.dx / s, yy = ray.dy / s, z = ray.dz / s;
        float v[8] = {SH_C1 * yy, SH_C1 * z, SH_C1 * x, SH_C2 * (x * yy), SH_C2 * (yy * z), SH_C20 * (3.f * (z * z) - 1.f),
                      SH_C2 * (x * z), SH_C22 * (x * x - yy * yy)};
#pragma unroll
        for (int k = 0; k + 1 < B; ++k) y[k] = ok ? v[k] : 0.f;
    }
    // A pair of corners along z is 2 B contiguous float4s.  All 8 B in flight would be 72 float4s at B = 9, a wave per SIMD; the
    // march keeps this many pairs in flight instead and leaves the wait to the other waves of the SIMD.
    // The half instantiations keep the same numbers: their in-flight loads hold half the registers, but the fp32 form measured
    // no gain from more pairs in flight (profiles/baked_notes.md); the outputs do not depend on the choice.
    static constexpr int PAIRS_IN_FLIGHT = B == 1 ? 4 : B == 4 ? 2 : 1;
    // the sum over the basis, before the clamps
    __device__ __forceinline__ float4 unclamped(long long point) const {
        const Stored *c = data + point * B;
        float4 v = baked_widen(c[0]);
#pragma unroll
        for (int k = 1; k < B; ++k) {
            const float4 a = baked_widen(c[k]);
            v.x = v.x + a.x * y[k - 1]; v.y = v.y + a.y * y[k - 1]; v.z = v.z + a.z * y[k - 1]; v.w = v.w + a.w * y[k - 1];
        }
        return v;
    }
    __device__ __forceinline__ float4 at(long long point) const {
        float4 v = unclamped(point);
        // per corner, before the blend; written so that a value inside the range keeps its bits (-0 included)
        v.x = v.x < 0.f ? 0.f : v.x; v.y = v.y < 0.f ? 0.f : v.y; v.z = v.z < 0.f ? 0.f : v.z; v.w = v.w < 0.f ? 0.f : v.w;
        v.x = v.x > 1.f ? 1.f : v.x; v.y = v.y > 1.f ? 1.f : v.y; v.z = v.z > 1.f ? 1.f : v.z;
        return v;
    }
    // backward: g = weight x dL/d(blended value) of this corner, through the clamps (torch.clamp's derivative: 1 where the
    // unclamped value lies in the closed range, 0 outside and for a NaN).  The unclamped value is summed again from the
    // coefficients the forward just read.
    __device__ __forceinline__ float4 mask(long long point, float4 g) const {
        const float4 v = unclamped(point);
        g.x = v.x >= 0.f && v.x <= 1.f ? g.x : 0.f;
        g.y = v.y >= 0.f && v.y <= 1.f ? g.y : 0.f;
        g.z = v.z >= 0.f && v.z <= 1.f ? g.z : 0.f;
        g.w = v.w >= 0.f ? g.w : 0.f;
        return g;
    }
    // ... and to coefficient k as g Y_k, Y_0 = 1
    __device__ __forceinline__ void scatter(float *__restrict__ d_stored, long long point, float4 g) const {
        g = mask(point, g);
        if (g.x == 0.f && g.y == 0.f && g.z == 0.f && g.w == 0.f) return;
        float *dst = d_stored + point * (B * 4);
        baked_add4(dst, g);
#pragma unroll
        for (int k = 1; k < B; ++k)
            baked_add4(dst + k * 4, make_float4(g.x * y[k - 1], g.y * y[k - 1], g.z * y[k - 1], g.w * y[k - 1]));
    }
};

// Where the rows of a pair of corners along z (grid points p, p + 1) lie in the array a Corner reads.  Dense: rows p and p + 1.
struct DenseRows {
    struct Pairs {};
    __device__ __forceinline__ bool find(long long, long long, long long, Pairs &) const { return true; }
    // pair j = 2 ix + iy of the cell, whose base is grid point p
    __device__ __forceinline__ long long row(const Pairs &, int, long long p) const { return p; }
};

// Sparse: rows r = index[p] and r + 1 of the kept rows (the pair closure of the kept set puts the two corners of a pair of an
// occupied cell next to each other).  The four index values are independent 4-byte loads, issued together; a sample any of whose
// four rows is not in [0, last] reads no row and keeps sigma = 0 (last = M - 2; below 0 the index is not read either).
struct SparseRows {
    const int32_t *index;  // (nx,ny,nz): the rank of a kept point, -1 elsewhere
    int last;
    struct Pairs {
        int r[4];
    };
    __device__ __forceinline__ bool find(long long p000, long long sx, long long sy, Pairs &pr) const {
        if (last < 0) return false;
        pr.r[0] = index[p000];
        pr.r[1] = index[p000 + sy];
        pr.r[2] = index[p000 + sx];
        pr.r[3] = index[p000 + sx + sy];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) ok = ok && pr.r[j] >= 0 && pr.r[j] <= last;
        return ok;
    }
    __device__ __forceinline__ long long row(const Pairs &pr, int j, long long) const {
        return j == 0 ? pr.r[0] : j == 1 ? pr.r[1] : j == 2 ? pr.r[2] : pr.r[3];
    }
};

// ---- what the forward march and its backward share: the samples of a ray and the value at each.  Both kernels call these, so
// the set of samples a gradient is given for is the set the forward composited, decided by the same operations in the same order.

// the number of samples; a ray that cannot be sampled (near >= far, a non-finite component, more than 2^20 samples) keeps
// n = 0, reads nothing and gets the background.  (The backward calls this; the forward kernels hold the same five lines in place.)
__device__ __forceinline__ int baked_sample_count(const Ray8 &ray, float step) {
    const float o[3] = {ray.ox, ray.oy, ray.oz}, d[3] = {ray.dx, ray.dy, ray.dz};
    bool ok = occ_finite(ray.near) && occ_finite(ray.far) && ray.near < ray.far;
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && occ_finite(o[a]) && occ_finite(d[a]);
    const float count = ceilf((ray.far - ray.near) / step);
    return ok && count <= BAKED_MAX_SAMPLES ? (int)count : 0;  // (a NaN count compares false)
}

// sample i of a ray of n: its depth, whether it contributes (i < n, inside the box, its cell's bit on), its cell and its place in it
struct BakedSample {
    float t;
    bool active;
    int idx[3];
    float f[3];
};

__device__ __forceinline__ BakedSample baked_sample(const Ray8 &ray, const BakedParams &q, int i, int n) {
    const float o[3] = {ray.ox, ray.oy, ray.oz}, d[3] = {ray.dx, ray.dy, ray.dz};
    BakedSample s;
    s.t = ray.near + ((float)i + 0.5f) * q.step;
    s.active = i < n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = o[a] + s.t * d[a];                    // ray_point's operations (pnr_geom.h)
        s.active = s.active && p >= q.g.c1[a] && p <= q.g.c2[a];  // (a NaN or infinite coordinate is outside)
        const float u = (p - q.g.c1[a]) / q.g.h[a];
        const float c = fminf(fmaxf(floorf(u), 0.f), (float)(q.g.n[a] - 2));  // (fmaxf drops a NaN: always a cell of the grid)
        s.idx[a] = (int)c;
        s.f[a] = fminf(fmaxf(u - c, 0.f), 1.f);
    }
    if (q.bits) {
        const long long cy = q.g.n[2] - 1, cx = (long long)(q.g.n[1] - 1) * (q.g.n[2] - 1);  // cell strides of the bitfield
        const long long cell = s.idx[0] * cx + s.idx[1] * cy + s.idx[2];
        s.active = s.active && (q.bits[cell >> 5] >> (cell & 31) & 1u);
    }
    return s;
}

// where the eight corners of an active sample's cell lie: base point p000, the rows of its four pairs along z
template <class Rows>
struct BakedCell {
    long long p000, sx, sy;  // point strides in float4s; z is the fastest axis
    typename Rows::Pairs pr;
    // the row of corner iz = 0 of pair j = 2 ix + iy (corner iz = 1 is the next row)
    __device__ __forceinline__ long long row(const Rows &rows, int j) const {
        return rows.row(pr, j, p000 + (j >> 1) * sx + (j & 1) * sy);
    }
};

// false: the sample reads no row (a sparse volume that does not hold its corners) and keeps sigma = 0
template <class Rows>
__device__ __forceinline__ bool baked_find_cell(const BakedParams &q, const Rows &rows, const BakedSample &s, BakedCell<Rows> &cell) {
    cell.sy = q.g.n[2];
    cell.sx = (long long)q.g.n[1] * q.g.n[2];
    cell.p000 = s.idx[0] * cell.sx + s.idx[1] * cell.sy + s.idx[2];
    return rows.find(cell.p000, cell.sx, cell.sy, cell.pr);
}

// the trilinear blend of the cell's eight corner values
template <class Corner, class Rows>
__device__ __forceinline__ float4 baked_blend(const Corner &corner, const Rows &rows, const BakedCell<Rows> &cell, const float (&f)[3],
                                              float4 cs /*zeros*/) {
    const long long p000 = cell.p000, sx = cell.sx, sy = cell.sy;
    const typename Rows::Pairs &pr = cell.pr;
    // along z (a pair of corners is contiguous in memory: each pair is reduced before the next is needed), then y, then x
    if constexpr (Corner::PAIRS_IN_FLIGHT == 4) {
        const long long r00 = rows.row(pr, 0, p000), r01 = rows.row(pr, 1, p000 + sy), r10 = rows.row(pr, 2, p000 + sx),
                        r11 = rows.row(pr, 3, p000 + sx + sy);
        const float4 v00 = baked_lerp(corner.at(r00), corner.at(r00 + 1), f[2]);
        const float4 v01 = baked_lerp(corner.at(r01), corner.at(r01 + 1), f[2]);
        const float4 v10 = baked_lerp(corner.at(r10), corner.at(r10 + 1), f[2]);
        const float4 v11 = baked_lerp(corner.at(r11), corner.at(r11 + 1), f[2]);
        cs = baked_lerp(baked_lerp(v00, v01, f[1]), baked_lerp(v10, v11, f[1]), f[0]);
    } else if constexpr (Corner::PAIRS_IN_FLIGHT == 2) {
        // the same operations on the same values; a real loop over x, so that the pairs of x + 1 are asked for after
        // those of x have been reduced (the gathers are independent: straight-line code issues them all first)
        float4 vy[2];
#pragma unroll 1
        for (int ix = 0; ix < 2; ++ix) {
            const long long p = p000 + ix * sx;
            const long long r0 = rows.row(pr, 2 * ix, p);
            const float4 v0 = baked_lerp(corner.at(r0), corner.at(r0 + 1), f[2]);
            const long long r1 = rows.row(pr, 2 * ix + 1, p + sy);
            const float4 v1 = baked_lerp(corner.at(r1), corner.at(r1 + 1), f[2]);
            vy[1] = baked_lerp(v0, v1, f[1]);
            if (ix == 0) vy[0] = vy[1];
        }
        cs = baked_lerp(vy[0], vy[1], f[0]);
    } else {
        // one pair at a time: j = 2 ix + iy
        float4 vz = cs, vy[2] = {cs, cs};
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const long long p = rows.row(pr, j, p000 + (j >> 1) * sx + (j & 1) * sy);
            const float4 v = baked_lerp(corner.at(p), corner.at(p + 1), f[2]);
            if (j & 1) {
                vy[1] = baked_lerp(vz, v, f[1]);
                if (j == 1) vy[0] = vy[1];
            }
            vz = v;
        }
        cs = baked_lerp(vy[0], vy[1], f[0]);
    }
    return cs;
}

// the (r,g,b,sigma) of a sample: the blend where the sample is active and finds its rows, zeros elsewhere
template <class Corner, class Rows>
__device__ __forceinline__ float4 baked_value(const BakedParams &q, const Corner &corner, const Rows &rows, const BakedSample &s,
                                              BakedCell<Rows> &cell, bool &found) {
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
    found = false;
    if (s.active) {
        if (baked_find_cell(q, rows, s, cell)) {
            found = true;
            cs = baked_blend(corner, rows, cell, s.f, cs);
        }
    }
    return cs;
}

// alpha of a sample and what it leaves of the transmittance; ex = exp(-step sigma) is d alpha / d sigma / step
struct BakedAlpha {
    float ex, a, tfac;
};
__device__ __forceinline__ BakedAlpha baked_alpha(float step, float sigma) {
    BakedAlpha r;
    r.ex = expf(-(step * sigma));
    r.a = 1.f - r.ex;            // nerf.py:228 with delta = step; exactly 0 for sigma == 0
    r.tfac = 1.f - r.a + 1e-10f;  // :230-232; exactly 1 for a == 0
    return r;
}

#pragma clang fp contract(fast)

// ---- host only from here.  The rays of a march with their own checks, made where the entry's arguments are (pnr_entry.h's
// explicit_rays for the baked entries).  defect: what is wrong with them (NULL: nothing); baked_check reports it after the
// entry's degree check, which every entry makes first.

static inline bool baked_misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }
static inline bool baked_misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

struct BakedRays {
    RaySrc src;
    long long R;
    const char *defect;
};

static inline BakedRays baked_explicit_rays(const float *rays, long long R) {
    BakedRays s = {};
    s.src.rays = rays;
    s.R = R;
    s.defect = R < 0 ? "bad sizes (R)" : R > 0 && !rays ? "null argument"
               : baked_misaligned4(rays) ? "rays must be 4-byte aligned" : nullptr;
    return s;
}

static inline BakedRays baked_camera_rays(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                          float z_far) {
    BakedRays s = {};
    s.src.poses = poses;
    s.src.W = W; s.src.H = H;
    s.src.fx = fx; s.src.fy = fy; s.src.cx = cx; s.src.cy = cy;
    s.src.z_near = z_near; s.src.z_far = z_far;
    s.R = (long long)NV * W * H;
    s.defect = NV < 0 || W <= 0 || H <= 0 ? "bad sizes (NV, W, H)" : NV > 0 && !poses ? "null argument"
               : baked_misaligned4(poses) ? "poses must be 4-byte aligned" : nullptr;
    return s;
}

// What an entry was handed to march through, and the words of its refusals.
struct BakedVolumeDesc {
    const void *stored;       // dense: (nx,ny,nz) x B x (r,g,b,sigma); sparse: the M kept rows of that array
    int degree;               // -1: an RGBA volume (B = 1, no basis); 0..2: the coefficient volume of that degree, B = (degree+1)^2
    bool half;                // an (r,g,b,sigma) is four fp16 numbers (Half4), else a float4
    bool sparse;              // `stored` holds kept rows, found through index; bits are then mandatory
    const int32_t *index;     // sparse: (nx,ny,nz), the rank of a kept point, -1 elsewhere
    long long M;              // sparse: the number of kept rows
    const char *name;         // what the header calls `stored`: "vol", "coef" or "rows"
    int min_degree;           // the entry's degree argument lies in [min_degree, 2] ...
    const char *degree_rule;  // ... or the entry refuses with these words (the RGBA entries take no degree: never said)
    bool bad_storage = false; // the entry takes a storage_half argument and it was neither 0 nor 1
};
constexpr const char *DEGREE_SH = "degree must be 0, 1 or 2", *DEGREE_SPARSE = "degree must be -1 (RGBA rows), 0, 1 or 2",
                     *DEGREE_HALF = "degree must be -1 (RGBA), 0, 1 or 2";

static inline BakedVolumeDesc baked_dense(const void *stored, int degree, bool half, const char *name, int min_degree,
                                          const char *degree_rule) {
    return {stored, degree, half, false, nullptr, 0, name, min_degree, degree_rule};
}
static inline BakedVolumeDesc baked_sparse(const void *rows, long long M, const int32_t *index, int degree, bool half,
                                           const char *degree_rule) {
    return {rows, degree, half, true, index, M, "rows", -1, degree_rule};
}
// `stored` of the backward, TV and scene entries: storage_half 0 or 1 (anything else is refused), index == NULL: a dense volume,
// M is then not looked at
static inline BakedVolumeDesc baked_stored(const void *stored, int storage_half, long long M, int degree, const int32_t *index) {
    BakedVolumeDesc v = {stored, degree, storage_half == 1, index != nullptr, index, index ? M : 0, "stored", -1, DEGREE_HALF};
    v.bad_storage = storage_half != 0 && storage_half != 1;
    return v;
}

// the grid, the march settings, the outputs and the stream: the tail of every entry's argument list, in its order
struct BakedMarchArgs {
    const uint32_t *bits;
    int nx, ny, nz;
    const float *c1, *c2;
    float step;
    int white_bkgd;
    float terminate;
    float *rgb, *depth, *alpha;
    void *stream;
};

template <class T>
struct BakedType {
    using type = T;
};

// what a backward entry takes next to the march arguments: the upstream gradients (each NULL: zeros) and the buffer it adds into
// (d_stored) or writes every row of (d_rays), with the name the header gives it
struct BakedGrads {
    const float *d_rgb, *d_depth, *d_alpha;
    float *out;
    const char *out_name = "d_stored";
    bool out_nullable = false;  // a scene's stored backward: NULL = this object is frozen
};

// ranks are int32: a row beyond 2^31 - 2 cannot be named.  M < 2 (last < 0): no sample finds its rows, nothing is read
static inline SparseRows baked_sparse_rows(const BakedVolumeDesc &v) {
    return SparseRows{v.index, (int)(v.M - 2 < 0x7ffffffeLL ? v.M - 2 : 0x7ffffffeLL)};
}

// every check of every entry, forward (grads == NULL: a's rgb, depth and alpha are written) and backward, in one order.
// -> PNR_OK with `blocks` workgroups to launch (0: no rays, nothing to do) and the march settings in q
static inline int baked_check(const char *entry, const BakedRays &rays, const BakedVolumeDesc &v, const BakedMarchArgs &a,
                              const BakedGrads *grads, BakedParams &q, long long &blocks) {
    blocks = 0;
    if (v.degree < v.min_degree || v.degree > 2) return occ_fail(entry, v.degree_rule);
    if (v.bad_storage) return occ_fail(entry, "storage_half must be 0 or 1");
    if (rays.defect) return occ_fail(entry, rays.defect);
    if (v.sparse && v.M < 0) return occ_fail(entry, "bad sizes (M)");
    if (const char *why = occ_bad_dims(a.nx, a.ny, a.nz)) return occ_fail(entry, why);
    if (const char *why = occ_grid(a.nx, a.ny, a.nz, a.c1, a.c2, q.g)) return occ_fail(entry, why);
    if (!(a.step > 0.f) || !std::isfinite(a.step)) return occ_fail(entry, "step must be finite and > 0");
    if (!(a.terminate >= 0.f && a.terminate < 1.f)) return occ_fail(entry, "terminate must lie in [0, 1)");  // (refuses a NaN)
    const long long R = rays.R;
    if (R == 0) return PNR_OK;
    if (grads ? !grads->out && !grads->out_nullable : !a.rgb || !a.depth || !a.alpha) return occ_fail(entry, "null argument");
    if (v.sparse ? v.M > 0 && (!v.stored || !v.index || !a.bits) : !v.stored) return occ_fail(entry, "null argument");
    if (occ_misaligned16(v.stored)) {
        char why[40];
        std::snprintf(why, sizeof(why), "%s must be 16-byte aligned", v.name);
        return occ_fail(entry, why);
    }
    if (v.sparse && baked_misaligned4(v.index)) return occ_fail(entry, "index must be 4-byte aligned");
    if (grads) {
        if (baked_misaligned4(a.bits) || baked_misaligned4(grads->d_rgb) || baked_misaligned4(grads->d_depth) ||
            baked_misaligned4(grads->d_alpha) || baked_misaligned4(grads->out)) {
            char why[80];
            std::snprintf(why, sizeof(why), "bits, d_rgb, d_depth, d_alpha and %s must be 4-byte aligned", grads->out_name);
            return occ_fail(entry, why);
        }
    } else if (baked_misaligned4(a.bits) || baked_misaligned4(a.rgb) || baked_misaligned4(a.depth) || baked_misaligned4(a.alpha)) {
        return occ_fail(entry, "bits, rgb, depth and alpha must be 4-byte aligned");
    }
    blocks = (R + BAKED_WAVES - 1) / BAKED_WAVES;
    if (blocks > 0x7fffffffLL) return occ_fail(entry, "the number of rays exceeds the launch limit");
    q.bits = a.bits;
    q.step = a.step;
    q.eps = a.terminate;
    q.white_bkgd = a.white_bkgd;
    return PNR_OK;
}

// layout, storage and kind of a checked volume, each decided once: launch(BakedType<Corner>{}, rows) on one of the 2 x 2 x 4
// instantiations.  rows is DenseRows{} or the volume's SparseRows (a scene takes its type alone: every object has rows of its own)
template <class Launch>
static inline void baked_dispatch(const BakedVolumeDesc &v, const Launch &launch) {
    const auto by_kind = [&](auto stored, auto rows) {
        using Stored = typename decltype(stored)::type;
        if (v.degree < 0) launch(BakedType<RgbaCornerOf<Stored>>{}, rows);
        else if (v.degree == 0) launch(BakedType<ShCorner<1, Stored>>{}, rows);
        else if (v.degree == 1) launch(BakedType<ShCorner<4, Stored>>{}, rows);
        else launch(BakedType<ShCorner<9, Stored>>{}, rows);
    };
    const auto by_storage = [&](auto rows) {
        if (v.half) by_kind(BakedType<Half4>{}, rows);
        else by_kind(BakedType<float4>{}, rows);
    };
    if (v.sparse) by_storage(baked_sparse_rows(v));
    else by_storage(DenseRows{});
}

}  // namespace pnr
