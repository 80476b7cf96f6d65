// pnr_baked.hip -- ray marching through a baked RGBA volume for gfx950 (inference).  The network of an encoded object is evaluated
// ONCE on the points of its grid (util.bake.BakedVolume.from_model: rgb and sigma at the points of pnr_gen_grid_points); any number
// of views is then rendered from the grid alone: equidistant samples along the ray, a trilinear blend of the cell's eight corners,
// the compositing of src/render/nerf.py:178-182,223-249 with a constant delta.  No network behind a pixel; the image is an
// approximation of the network's render (trilinear in space, one view direction per grid point, no importance sampling).
// Semantics: include/pixelnerf_hip.h ("baked volumes").  One wavefront per ray, composite_kernel's scan; no atomics, no LDS, no
// workspace: the same bytes on every call.
// The view-dependent form (pnr_baked_sh_render_*) keeps B = (L+1)^2 float4s of real spherical-harmonic coefficients per grid point
// and evaluates them for each ray's own direction; the sparse form (pnr_baked_sparse_render_*) keeps only the rows of the grid
// points that occupied cells read (the kept set of pnr_sparse_points_mark) and an int32 index over the grid; the half forms
// (pnr_baked_half_render_* / pnr_baked_sparse_half_render_*) store four fp16 numbers where the others store a float4.
// Structure.  Device: ONE march (baked_march) and ONE kernel template (baked_march_kernel<Corner, Rows>) around it.  Corner says
// what the march reads at a corner of a cell (RgbaCornerOf / ShCorner<B>) and what a stored number is (float4 or Half4, widened
// exactly on load: everything after the load is the same code); Rows says where a pair of corners lies (DenseRows: rows p, p + 1
// of the dense array; SparseRows: rows index[p], index[p] + 1 of the kept ones).  4 kinds x 2 storages x 2 layouts = 16 kernels.
// Host: an entry builds its ray source (baked_explicit_rays / baked_camera_rays: the checks of the rays travel with them), says
// what it was handed (BakedVolumeDesc: pointer, degree, storage, index + M, and the words of its refusals) and calls
// baked_render, which holds every check, in one order for all ten entries, and dispatches layout, storage and kind once each.
// Backward (pnr_baked_backward_rays / _views: dL/d stored, what fitting a volume needs).  The per-sample part of the march --
// the point, its cell and fractions, whether it contributes, the rows of its corners, the blend, alpha -- lives in device functions
// that baked_march and baked_march_bwd_kernel both call, so the backward's samples are the forward's (the sample count: the same
// five lines, in place in the forward and as baked_sample_count in the backward).  The
// backward is the ONE path here with atomics (fp32 atomicAdd into the caller's zeroed buffer): not bit-reproducible from run to run.
// fp32 storage only; baked_check holds the checks of both directions.
// Ray backward (pnr_baked_ray_backward_rays / _views: dL/d rays, what registering a camera needs): baked_march_ray_bwd_kernel, the
// same walk over the same samples, through the spatial derivative of the blend (baked_blend_grad) instead of its corner weights;
// every storage and layout (the forward's 16 instantiations), no atomics, every row written.
// Scenes (pnr_baked_scene_render_rays / _views: up to 8 posed volumes of one kind in one image): baked_scene_march_kernel, the
// forward's walk with an inner loop over the objects, each seeing the world ray in its own frame; the same 16 instantiations.
// Scene backward (pnr_baked_scene_backward_rays / _views: dL/d world rays and dL/d object poses, what placing an object needs):
// baked_scene_ray_bwd_kernel, the ray backward's walk on the scene's mixture, and two small kernels that reduce the poses'
// gradient over the rays in a fixed order; no atomics, no LDS.  The four scene entries share one checking function.
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
    // unclamped value lies in the closed range, 0 outside and for a NaN) to coefficient k as g Y_k, Y_0 = 1.  The unclamped value
    // is summed again from the coefficients the forward just read.
    __device__ __forceinline__ void scatter(float *__restrict__ d_stored, long long point, float4 g) const {
        const float4 v = unclamped(point);
        g.x = v.x >= 0.f && v.x <= 1.f ? g.x : 0.f;
        g.y = v.y >= 0.f && v.y <= 1.f ? g.y : 0.f;
        g.z = v.z >= 0.f && v.z <= 1.f ? g.z : 0.f;
        g.w = v.w >= 0.f ? g.w : 0.f;
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
// n = 0, reads nothing and gets the background.  (The backward calls this; baked_march holds the same five lines in place.)
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

template <class Corner, class Rows>
__device__ __forceinline__ void baked_march(const RaySrc &rs, long long R, const BakedParams &q, Corner corner, const Rows rows,
                                            float *__restrict__ rgb, float *__restrict__ depth, float *__restrict__ alpha_out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * BAKED_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;  // the idle waves of the last workgroup (nothing below synchronises across waves)
    const Ray8 ray = load_ray(rs, r);
    corner.set_ray(ray);
    // baked_sample_count's five lines, in place: as a call the degree-2 march took 19 % longer (2.61 against 2.21 ms at 128^3, the
    // same instructions scheduled otherwise; profiles/baked_notes.md, "Backward and fitting").  Keep the two texts the same.
    const float o[3] = {ray.ox, ray.oy, ray.oz}, d[3] = {ray.dx, ray.dy, ray.dz};
    bool ok = occ_finite(ray.near) && occ_finite(ray.far) && ray.near < ray.far;
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && occ_finite(o[a]) && occ_finite(d[a]);
    const float count = ceilf((ray.far - ray.near) / q.step);
    const int n = ok && count <= BAKED_MAX_SAMPLES ? (int)count : 0;  // (a NaN count compares false)
    float carry = 1.f;  // transmittance in front of this chunk: prod_{j < c0} (1 - a_j + 1e-10)
    float acc_r = 0.f, acc_g = 0.f, acc_b = 0.f, acc_d = 0.f, acc_w = 0.f;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const BakedSample s = baked_sample(ray, q, c0 + lane, n);
        if (__ballot(s.active) == 0ull) continue;  // every factor of the chunk is exactly 1: the carry and the sums stay as they are
        BakedCell<Rows> cell;
        bool found;
        const float4 cs = baked_value(q, corner, rows, s, cell, found);
        const BakedAlpha al = baked_alpha(q.step, cs.w);
        const float incl = wave_scan_mul(al.tfac, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.f;
        const float w = al.a * (carry * excl);  // :234-236
        acc_r += w * cs.x; acc_g += w * cs.y; acc_b += w * cs.z;
        acc_d += w * s.t;
        acc_w += w;
        carry = carry * __shfl(incl, 63, 64);
        if (q.eps > 0.f && carry <= q.eps) break;  // wave-uniform; a NaN transmittance does not stop the ray
    }
    acc_r = wave_sum(acc_r); acc_g = wave_sum(acc_g); acc_b = wave_sum(acc_b);
    acc_d = wave_sum(acc_d); acc_w = wave_sum(acc_w);
    if (lane == 0) {
        if (q.white_bkgd) {  // :241-244
            acc_r = acc_r + 1.f - acc_w; acc_g = acc_g + 1.f - acc_w; acc_b = acc_b + 1.f - acc_w;
        }
        rgb[r * 3 + 0] = acc_r; rgb[r * 3 + 1] = acc_g; rgb[r * 3 + 2] = acc_b;
        depth[r] = acc_d;
        alpha_out[r] = acc_w;
    }
}

// THE kernel of every entry.  `stored` is the dense volume or the kept rows, (M,4) / (M,B,4); the Corner is built here, and
// ShCorner::y stays what it is: per-ray state that set_ray fills, not an argument.
template <class Corner, class Rows>
__global__ void __launch_bounds__(BAKED_WAVES * 64)
baked_march_kernel(const RaySrc rs, long long R, const BakedParams q, const Rows rows, const typename Corner::stored_t *__restrict__ stored,
                   float *__restrict__ rgb, float *__restrict__ depth, float *__restrict__ alpha_out) {
    Corner corner;
    corner.data = stored;
    baked_march(rs, R, q, corner, rows, rgb, depth, alpha_out);
}

// ---- scenes of several posed volumes (pnr_baked_scene_render_*; include/pixelnerf_hip.h, "Scenes of several baked volumes").
// The march above with an inner loop over objects: the samples are the WORLD ray's, every object sees the ray in its own frame,
// and the values of the objects that contribute to a sample are mixed before alpha and the scan.  The per-sample work is the
// device functions of the single march, so one object at the identity renders that march's bytes.

// One posed volume as the kernel sees it: what baked_check made of a PnrBakedObject.  The scene travels BY VALUE as a kernel
// argument (8 x 128 bytes) and the object loop's index is wave-uniform: the fields are scalar loads from the kernarg segment.
struct BakedSceneObject {
    const void *stored;
    const uint32_t *bits;
    const int32_t *index;  // sparse only
    int last;              // sparse only: SparseRows::last
    OccGrid g;             // the object's own box and grid
    float rot[9], t[3];    // object-to-world [R | t]; the kernel applies the inverse, R^T (x - t)
};
struct BakedSceneDesc {
    BakedSceneObject obj[PNR_BAKED_SCENE_MAX_OBJECTS];
    int n;
};
static_assert(sizeof(BakedSceneObject) == 128, "eight objects are 1 KiB of kernel arguments");

template <class Rows>
__device__ __forceinline__ Rows baked_scene_rows(const BakedSceneObject &ob) {
    if constexpr (std::is_same<Rows, SparseRows>::value) return SparseRows{ob.index, ob.last};
    else return DenseRows{};
}

// the world ray in the object's frame: q = o - t, then R^T q and R^T d, each as (x R_xa + y R_ya) + z R_za; near and far are shared
__device__ __forceinline__ Ray8 baked_scene_ray(const Ray8 &w, const BakedSceneObject &ob) {
    const float qx = w.ox - ob.t[0], qy = w.oy - ob.t[1], qz = w.oz - ob.t[2];
    Ray8 r;
    r.ox = (qx * ob.rot[0] + qy * ob.rot[3]) + qz * ob.rot[6];
    r.oy = (qx * ob.rot[1] + qy * ob.rot[4]) + qz * ob.rot[7];
    r.oz = (qx * ob.rot[2] + qy * ob.rot[5]) + qz * ob.rot[8];
    r.dx = (w.dx * ob.rot[0] + w.dy * ob.rot[3]) + w.dz * ob.rot[6];
    r.dy = (w.dx * ob.rot[1] + w.dy * ob.rot[4]) + w.dz * ob.rot[7];
    r.dz = (w.dx * ob.rot[2] + w.dy * ob.rot[5]) + w.dz * ob.rot[8];
    r.near = w.near;
    r.far = w.far;
    return r;
}

// The value of one object at sample i of the world ray: what baked_march computes for the ray in the object's frame.  -> whether
// the sample contributes (active, and its rows found); `active`: baked_sample's.  The ray is transformed anew for every chunk
// (21 operations, nothing kept per object), and the basis of a coefficient volume is evaluated only for a chunk that reads.
template <class Corner, class Rows>
__device__ __forceinline__ bool baked_scene_value(const BakedSceneObject &ob, const Ray8 &world, float step, int i, int n, bool &active,
                                                  float4 &cs) {
    const Ray8 ray = baked_scene_ray(world, ob);
    active = false;
    cs = make_float4(0.f, 0.f, 0.f, 0.f);
    // baked_sample's inside test alone, first -- the same operations on the same numbers, so exactly its answer -- and nothing
    // more for a chunk that does not touch the object's box: most (chunk, object) pairs of a scene end here, before the divisions
    const float t = ray.near + ((float)i + 0.5f) * step;
    const float o[3] = {ray.ox, ray.oy, ray.oz}, d[3] = {ray.dx, ray.dy, ray.dz};
    bool inside = i < n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = o[a] + t * d[a];
        inside = inside && p >= ob.g.c1[a] && p <= ob.g.c2[a];
    }
    if (__ballot(inside) == 0ull) return false;
    BakedParams q;
    q.bits = ob.bits;
    q.g = ob.g;
    q.step = step;
    q.eps = 0.f;
    q.white_bkgd = 0;
    const BakedSample s = baked_sample(ray, q, i, n);
    active = s.active;
    if (__ballot(s.active) == 0ull) return false;  // nothing of this object in the chunk: no loads
    Corner corner;
    corner.data = static_cast<const typename Corner::stored_t *>(ob.stored);
    corner.set_ray(ray);
    const Rows rows = baked_scene_rows<Rows>(ob);
    BakedCell<Rows> cell;
    bool found;
    cs = baked_value(q, corner, rows, s, cell, found);
    return found;
}

template <class Corner, class Rows>
__global__ void __launch_bounds__(BAKED_WAVES * 64)
baked_scene_march_kernel(const RaySrc rs, long long R, const BakedSceneDesc sc, float step, float eps, int white_bkgd,
                         float *__restrict__ rgb, float *__restrict__ depth, float *__restrict__ alpha_out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * BAKED_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;
    const Ray8 ray = load_ray(rs, r);
    // baked_sample_count's five lines on the WORLD ray, in place as in baked_march
    const float o[3] = {ray.ox, ray.oy, ray.oz}, d[3] = {ray.dx, ray.dy, ray.dz};
    bool ok = occ_finite(ray.near) && occ_finite(ray.far) && ray.near < ray.far;
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && occ_finite(o[a]) && occ_finite(d[a]);
    const float count = ceilf((ray.far - ray.near) / step);
    const int n = ok && count <= BAKED_MAX_SAMPLES ? (int)count : 0;
    float carry = 1.f;
    float acc_r = 0.f, acc_g = 0.f, acc_b = 0.f, acc_d = 0.f, acc_w = 0.f;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        const float t = ray.near + ((float)i + 0.5f) * step;  // baked_sample's depth
        // first pass: sigma = sum sigma_j over the objects that contribute, in list order; the first such value is kept
        float4 first = make_float4(0.f, 0.f, 0.f, 0.f);
        float sigma = 0.f;
        int cnt = 0;
        bool any = false;
#pragma unroll 1
        for (int j = 0; j < sc.n; ++j) {
            bool active;
            float4 cs;
            const bool found = baked_scene_value<Corner, Rows>(sc.obj[j], ray, step, i, n, active, cs);
            any = any || active;
            if (found) {
                if (cnt == 0) first = cs;
                sigma = sigma + cs.w;
                ++cnt;
            }
        }
        if (__ballot(any) == 0ull) continue;  // every factor of the chunk is exactly 1: the carry and the sums stay as they are
        // c = sum (sigma_j / sigma) c_j.  One contributor (all but the samples where boxes overlap): the kept value.  More: the
        // weights need the finished sum, so those lanes walk the objects again -- the same loads, the same values -- instead of
        // keeping eight float4s per lane.
        float cr = 0.f, cg = 0.f, cb = 0.f;
        if (cnt == 1 && sigma > 0.f) {
            const float wj = first.w / sigma;
            cr = wj * first.x; cg = wj * first.y; cb = wj * first.z;
        }
        if (__ballot(cnt >= 2) != 0ull) {
            if (cnt >= 2 && sigma > 0.f) {
#pragma unroll 1
                for (int j = 0; j < sc.n; ++j) {
                    bool active;
                    float4 cs;
                    if (baked_scene_value<Corner, Rows>(sc.obj[j], ray, step, i, n, active, cs)) {
                        const float wj = cs.w / sigma;
                        cr = cr + wj * cs.x; cg = cg + wj * cs.y; cb = cb + wj * cs.z;
                    }
                }
            }
        }
        const BakedAlpha al = baked_alpha(step, sigma);
        const float incl = wave_scan_mul(al.tfac, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.f;
        const float w = al.a * (carry * excl);
        acc_r += w * cr; acc_g += w * cg; acc_b += w * cb;
        acc_d += w * t;
        acc_w += w;
        carry = carry * __shfl(incl, 63, 64);
        if (eps > 0.f && carry <= eps) break;  // wave-uniform; a NaN transmittance does not stop the ray
    }
    acc_r = wave_sum(acc_r); acc_g = wave_sum(acc_g); acc_b = wave_sum(acc_b);
    acc_d = wave_sum(acc_d); acc_w = wave_sum(acc_w);
    if (lane == 0) {
        if (white_bkgd) {
            acc_r = acc_r + 1.f - acc_w; acc_g = acc_g + 1.f - acc_w; acc_b = acc_b + 1.f - acc_w;
        }
        rgb[r * 3 + 0] = acc_r; rgb[r * 3 + 1] = acc_g; rgb[r * 3 + 2] = acc_b;
        depth[r] = acc_d;
        alpha_out[r] = acc_w;
    }
}

// ---- backward of the march with respect to the stored values (pnr_baked_backward_*; fp32 storage only).
// w_i = a_i T_i, T_i = prod_{j<i} tf_j, tf_j = 1 - a_j + 1e-10, a_i = 1 - exp(-step sigma_i); with the upstream gradients of a ray
//   g_i = dL/dw_i = d_rgb . c_i + d_depth t_i + d_alpha - [white] sum(d_rgb)
//   dL/da_i = T_i (g_i - S_i),  S_i = sum_{j>i} g_j a_j prod_{i<k<j} tf_k = g_{i+1} a_{i+1} + tf_{i+1} S_{i+1}
//   dL/dsigma_i = dL/da_i step exp(-step sigma_i),  dL/dc_i = w_i d_rgb
// composite_bwd_kernel's walk (pnr_bwd.hip): the 64-sample chunks from the last to the first, per chunk a reverse wave scan of the
// maps S -> g_j a_j + tf_j S carried across chunks -- the suffix is never a difference of sums and nothing is divided by tf -- and
// T_i from the forward product scan, formed as the forward forms it.  A first walk in the forward's direction finds the chunk the
// forward stopped after (terminate) and leaves the transmittance at the head of chunk c < 64 in lane c; the chunks beyond 4096
// samples rebuild theirs from chunk 63's.  No workspace.
// Then through the blend: corner (ix,iy,iz) of the cell gets the product of f or 1 - f per axis (the derivative of the nested
// baked_lerps) times (dL/dc_i, dL/dsigma_i), and Corner::scatter adds it to the stored numbers with fp32 atomics.

// prod of tf over chunk c (every lane), with the forward's operations
template <class Corner, class Rows>
__device__ __forceinline__ float baked_chunk_product(const Ray8 &ray, const BakedParams &q, const Corner &corner, const Rows &rows, int c,
                                                     int n, int lane) {
    const BakedSample s = baked_sample(ray, q, c * 64 + lane, n);
    if (__ballot(s.active) == 0ull) return 1.f;
    BakedCell<Rows> cell;
    bool found;
    const float4 cs = baked_value(q, corner, rows, s, cell, found);
    return __shfl(wave_scan_mul(baked_alpha(q.step, cs.w).tfac, lane), 63, 64);
}

template <class Corner, class Rows>
__global__ void __launch_bounds__(BAKED_WAVES * 64)
baked_march_bwd_kernel(const RaySrc rs, long long R, const BakedParams q, const Rows rows, const typename Corner::stored_t *__restrict__ stored,
                       const float *__restrict__ d_rgb, const float *__restrict__ d_depth, const float *__restrict__ d_alpha,
                       float *__restrict__ d_stored) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * BAKED_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;
    float3 drgb = make_float3(0.f, 0.f, 0.f);
    if (d_rgb) drgb = make_float3(d_rgb[r * 3], d_rgb[r * 3 + 1], d_rgb[r * 3 + 2]);
    const float ddepth = d_depth ? d_depth[r] : 0.f, dalpha = d_alpha ? d_alpha[r] : 0.f;
    if (drgb.x == 0.f && drgb.y == 0.f && drgb.z == 0.f && ddepth == 0.f && dalpha == 0.f) return;  // nothing to send back
    const float gwhite = q.white_bkgd ? (drgb.x + drgb.y + drgb.z) : 0.f;  // rgb += 1 - sum w
    Corner corner;
    corner.data = stored;
    const Ray8 ray = load_ray(rs, r);
    corner.set_ray(ray);
    const int n = baked_sample_count(ray, q.step);
    int nc = (n + 63) >> 6;

    // the forward's walk: T at the head of chunk c < 64 into lane c, and the chunk it stopped after
    float heads = 1.f, carry = 1.f;
    for (int c = 0; c < nc; ++c) {
        if (lane == c) heads = carry;
        const BakedSample s = baked_sample(ray, q, c * 64 + lane, n);
        if (__ballot(s.active) == 0ull) continue;
        BakedCell<Rows> cell;
        bool found;
        const float4 cs = baked_value(q, corner, rows, s, cell, found);
        carry = carry * __shfl(wave_scan_mul(baked_alpha(q.step, cs.w).tfac, lane), 63, 64);
        if (q.eps > 0.f && carry <= q.eps) nc = c + 1;  // the forward's break, in its words
    }

    float S_in = 0.f;  // S of the chunk's last sample
    for (int c = nc - 1; c >= 0; --c) {
        const BakedSample s = baked_sample(ray, q, c * 64 + lane, n);
        if (__ballot(s.active) == 0ull) continue;  // 64 identity maps: S stays, nothing to scatter
        carry = __shfl(heads, c < 64 ? c : 63, 64);
        for (int cc = 63; cc < c; ++cc) carry = carry * baked_chunk_product(ray, q, corner, rows, cc, n, lane);
        BakedCell<Rows> cell;
        bool found;
        const float4 cs = baked_value(q, corner, rows, s, cell, found);
        const BakedAlpha al = baked_alpha(q.step, cs.w);
        const float incl = wave_scan_mul(al.tfac, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.f;
        const float T = carry * excl;
        const float w = al.a * T;
        // a sample that is not active, or found no rows, has a = 0 and tf = 1: the identity map
        const float g = found ? drgb.x * cs.x + drgb.y * cs.y + drgb.z * cs.z + ddepth * s.t + dalpha - gwhite : 0.f;
        float m = found ? al.tfac : 1.f, b = found ? g * al.a : 0.f;
        wave_rscan_affine(m, b, lane);
        const float mn = __shfl_down(m, 1, 64), bn = __shfl_down(b, 1, 64);
        const float S = lane == 63 ? S_in : bn + mn * S_in;
        S_in = __shfl(b + m * S_in, 0, 64);  // S of sample 64 c - 1
        if (found) {  // (no wave operation below: the lanes part here and meet again at the head of the loop)
            const float da = T * (g - S);
            const float4 dcs = make_float4(w * drgb.x, w * drgb.y, w * drgb.z, da * q.step * al.ex);
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {  // pair j = 2 ix + iy
                const long long row = cell.row(rows, j);
                const float wxy = (j >> 1 ? s.f[0] : 1.f - s.f[0]) * (j & 1 ? s.f[1] : 1.f - s.f[1]);
#pragma unroll
                for (int iz = 0; iz < 2; ++iz) {
                    const float wt = wxy * (iz ? s.f[2] : 1.f - s.f[2]);
                    if (wt != 0.f) corner.scatter(d_stored, row + iz, make_float4(wt * dcs.x, wt * dcs.y, wt * dcs.z, wt * dcs.w));
                }
            }
        }
    }
}

// ---- backward of the march with respect to the RAYS (pnr_baked_ray_backward_*; every storage): what registering a camera against
// a volume needs.  The walk, the samples and g_i, S_i, T_i, w_i, dL/da_i, dL/dsigma_i, dL/dc_i are baked_march_bwd_kernel's; what
// a sample sends back goes through the SPATIAL derivative of the blend instead of its corner weights:
//   dL/dp_i = sum_c dL/dval_{i,c} (d val_c / d f_a) / h_a,   dL/dval_i = (w_i d_rgb, dL/dsigma_i)
//   dL/dt_i = dL/dp_i . d + d_depth w_i                       (depth = sum w_i t_i; t_i moves with near alone)
//   d_o += dL/dp_i,  d_d += t_i dL/dp_i,  d_near += dL/dt_i,  d_far = 0
// and, for a view-dependent volume, dL/dY_k through Y(d / |d|) to d_d.  n, the inside test, the skip bits, the stop chunk, the cell
// and the regions of the clamps are constants: the exact derivative wherever the march is smooth in the ray, and on a cell plane
// the one-sided derivative of the cell that floor() names.  Everything of a ray is summed in its own wave (per-lane sums over the
// chunks, then wave_sum's butterfly, in fp64) and one lane writes the row: no atomics, no LDS, no workspace, the same bytes on every call,
// and EVERY row is written (exact zeros for a ray with no samples or no upstream gradient): the caller zeroes nothing.

__device__ __forceinline__ float4 baked_sub(const float4 b, const float4 a) { return make_float4(b.x - a.x, b.y - a.y, b.z - a.z, b.w - a.w); }
__device__ __forceinline__ float baked_dot(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// the blend and its partials along the fractions f: x = (vy[1] - vy[0]), y = the x-blend of the z-blended (y1 - y0), z = the
// x,y-blend of (v[..][..][1] - v[..][..][0]).  val is baked_blend's: the same operations on the same values
struct BakedBlendGrad {
    float4 val, x, y, z;
};

// a pair of corners along z, reduced: its value at f[2] and its slope
struct BakedPairGrad {
    float4 v, z;
};
template <class Corner>
__device__ __forceinline__ BakedPairGrad baked_pair_grad(const Corner &corner, long long row, float fz) {
    const float4 c0 = corner.at(row), c1 = corner.at(row + 1);
    return {baked_lerp(c0, c1, fz), baked_sub(c1, c0)};
}

// two reduced pairs (iy = 0, 1) of one ix, reduced along y: value, slope along y, slope along z
struct BakedFaceGrad {
    float4 v, y, z;
};
__device__ __forceinline__ BakedFaceGrad baked_face_grad(const BakedPairGrad &p0, const BakedPairGrad &p1, float fy) {
    return {baked_lerp(p0.v, p1.v, fy), baked_sub(p1.v, p0.v), baked_lerp(p0.z, p1.z, fy)};
}

template <class Corner, class Rows>
__device__ __forceinline__ BakedBlendGrad baked_blend_grad(const Corner &corner, const Rows &rows, const BakedCell<Rows> &cell,
                                                           const float (&f)[3]) {
    BakedFaceGrad face[2];
    // baked_blend's three forms: as many pairs in flight as the forward keeps (the slopes are differences of what it reads)
    if constexpr (Corner::PAIRS_IN_FLIGHT == 4) {
        const BakedPairGrad p00 = baked_pair_grad(corner, cell.row(rows, 0), f[2]), p01 = baked_pair_grad(corner, cell.row(rows, 1), f[2]),
                            p10 = baked_pair_grad(corner, cell.row(rows, 2), f[2]), p11 = baked_pair_grad(corner, cell.row(rows, 3), f[2]);
        face[0] = baked_face_grad(p00, p01, f[1]);
        face[1] = baked_face_grad(p10, p11, f[1]);
    } else if constexpr (Corner::PAIRS_IN_FLIGHT == 2) {
#pragma unroll 1
        for (int ix = 0; ix < 2; ++ix) {
            const BakedPairGrad p0 = baked_pair_grad(corner, cell.row(rows, 2 * ix), f[2]);
            const BakedPairGrad p1 = baked_pair_grad(corner, cell.row(rows, 2 * ix + 1), f[2]);
            face[1] = baked_face_grad(p0, p1, f[1]);
            if (ix == 0) face[0] = face[1];
        }
    } else {
        BakedPairGrad last = {};
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {  // pair j = 2 ix + iy
            const BakedPairGrad p = baked_pair_grad(corner, cell.row(rows, j), f[2]);
            if (j & 1) {
                face[1] = baked_face_grad(last, p, f[1]);
                if (j == 1) face[0] = face[1];
            }
            last = p;
        }
    }
    return {baked_lerp(face[0].v, face[1].v, f[0]), baked_sub(face[1].v, face[0].v), baked_lerp(face[0].y, face[1].y, f[0]),
            baked_lerp(face[0].z, face[1].z, f[0])};
}

// d f_a / d u_a of a sample, f = clamp(u - cell, 0, 1) under torch.clamp's convention: 1 on the closed range, 0 outside and for a
// NaN.  u - cell is formed again with baked_sample's operations (the clamped f cannot tell 0 from "below 0")
__device__ __forceinline__ void baked_frac_slope(const Ray8 &ray, const BakedParams &q, const BakedSample &s, float (&slope)[3]) {
    const float o[3] = {ray.ox, ray.oy, ray.oz}, d[3] = {ray.dx, ray.dy, ray.dz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = o[a] + s.t * d[a];
        const float raw = (p - q.g.c1[a]) / q.g.h[a] - (float)s.idx[a];
        slope[a] = raw >= 0.f && raw <= 1.f ? 1.f : 0.f;
    }
}

// alpha and the transmittance factor for the ray gradient: a = -expm1f(-step sigma) in fp32, tf = 1 - a + 1e-10 in fp64, and the
// products of tf (T) and the affine maps of S carried in fp64.  Two things the forward's fp32 chain does to a LONG ray (measured on
// the 4500-sample case, tests/test_hip_baked_ray_grad.py): baked_alpha's 1 - expf(-x) carries expf's rounding of a number next to 1
// into a, and where that rounding leans one way (gfx950: a tenth of an ulp low below x = 3e-3) thousands of factors of T lean with
// it -- 2.6e-5 of T after 4500 thin samples --; and each factor rounded to fp32 moves T by up to 3e-8, a random walk of 1e-6 .. 3e-6
// by the end of the ray.  Neither averages away in a sum over samples whose terms cancel (d_o across a blob: 880 to 1 on one ray of
// that case), because the drift weighs the front of the ray and its back differently.  The derivative is taken of the march as the
// header defines it, not of those roundings: the alphas differ from the forward's by less than an ulp of 1, with the same exact 0
// for sigma == 0 and the same 1 for an opaque sample.  Where the forward STOPPED is still decided by its own fp32 factors.
struct BakedAlphaExact {
    float a, ex;  // ex = 1 - a = d alpha / d sigma / step
    double tf;
};
__device__ __forceinline__ BakedAlphaExact baked_alpha_exact(float step, float sigma) {
    BakedAlphaExact r;
    r.a = -expm1f(-(step * sigma));
    r.ex = 1.f - r.a;
    r.tf = 1.0 - (double)r.a + 1e-10;
    return r;
}

// pnr_wave.h's wave_scan_mul and wave_rscan_affine on doubles: the same lanes in the same order
__device__ __forceinline__ double wave_scan_mul64(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o, 64);
        if (lane >= o) v *= t;
    }
    return v;
}
__device__ __forceinline__ void wave_rscan_affine64(double &m, double &b, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double mt = __shfl_down(m, o, 64), bt = __shfl_down(b, o, 64);
        if (lane + o < 64) {
            b += m * bt;
            m *= mt;
        }
    }
}

// the factor of sample s for the fp64 product: 1 where the forward's is exactly 1 (not active, or no rows)
template <class Corner, class Rows>
__device__ __forceinline__ double baked_tf_exact(const BakedParams &q, const Corner &corner, const Rows &rows, const BakedSample &s,
                                                 float &sigma) {
    BakedCell<Rows> cell;
    bool found;
    sigma = baked_value(q, corner, rows, s, cell, found).w;
    return found ? baked_alpha_exact(q.step, sigma).tf : 1.0;
}

// baked_chunk_product with those factors
template <class Corner, class Rows>
__device__ __forceinline__ double baked_chunk_product_exact(const Ray8 &ray, const BakedParams &q, const Corner &corner, const Rows &rows, int c,
                                                            int n, int lane) {
    const BakedSample s = baked_sample(ray, q, c * 64 + lane, n);
    if (__ballot(s.active) == 0ull) return 1.0;
    float sigma;
    return __shfl(wave_scan_mul64(baked_tf_exact(q, corner, rows, s, sigma), lane), 63, 64);
}

// how many basis values of a Corner depend on the direction of the ray: Y_1 .. Y_{B-1}
template <class Corner>
struct BakedBasis {
    static constexpr int N = 0;
};
template <int B, class Stored>
struct BakedBasis<ShCorner<B, Stored>> {
    static constexpr int N = B - 1;
};

// dL/dY_k += sum_c mask_c coef[point][k][c] g_c for k >= 1; g = weight x dL/d(blended value) of this corner, mask the derivative
// of the clamps as ShCorner::scatter forms it
template <class Stored, int N>
__device__ __forceinline__ void baked_basis_grad(const RgbaCornerOf<Stored> &, long long, float4, float (&)[N]) {}
template <int B, class Stored, int N>
__device__ __forceinline__ void baked_basis_grad(const ShCorner<B, Stored> &corner, long long point, float4 g, float (&dY)[N]) {
    const float4 v = corner.unclamped(point);
    g.x = v.x >= 0.f && v.x <= 1.f ? g.x : 0.f;
    g.y = v.y >= 0.f && v.y <= 1.f ? g.y : 0.f;
    g.z = v.z >= 0.f && v.z <= 1.f ? g.z : 0.f;
    g.w = v.w >= 0.f ? g.w : 0.f;
    if (g.x == 0.f && g.y == 0.f && g.z == 0.f && g.w == 0.f) return;
    const Stored *c = corner.data + point * B;
#pragma unroll
    for (int k = 1; k < B; ++k) dY[k - 1] += baked_dot(baked_widen(c[k]), g);
}

// dL/dY_k, k = 1..N, through Y(n), n = d / |d|, and through the normalisation: (I - n n^T) / |d| . sum_k dL/dY_k grad Y_k(n) is
// added to (gx, gy, gz).  ShCorner::set_ray's n and its test: a direction it gives no basis gets no term
template <int N>
__device__ __forceinline__ void baked_basis_to_dir(const Ray8 &ray, const float (&dY)[N], float &gx, float &gy, float &gz) {
    const float n2 = ray.dx * ray.dx + ray.dy * ray.dy + ray.dz * ray.dz;
    if (!(occ_finite(n2) && n2 != 0.f)) return;
    const float s = sqrtf(n2);
    const float x = ray.dx / s, y = ray.dy / s, z = ray.dz / s;
    float ax = SH_C1 * dY[2], ay = SH_C1 * dY[0], az = SH_C1 * dY[1];  // Y_1 = c y, Y_2 = c z, Y_3 = c x
    if constexpr (N == 8) {
        // Y_4 = c2 x y, Y_5 = c2 y z, Y_6 = c20 (3 z^2 - 1), Y_7 = c2 x z, Y_8 = c22 (x^2 - y^2)
        ax = ax + SH_C2 * (y * dY[3]) + SH_C2 * (z * dY[6]) + (2.f * SH_C22) * (x * dY[7]);
        ay = ay + SH_C2 * (x * dY[3]) + SH_C2 * (z * dY[4]) - (2.f * SH_C22) * (y * dY[7]);
        az = az + SH_C2 * (y * dY[4]) + (6.f * SH_C20) * (z * dY[5]) + SH_C2 * (x * dY[6]);
    }
    const float along = ax * x + ay * y + az * z;
    gx += (ax - x * along) / s;
    gy += (ay - y * along) / s;
    gz += (az - z * along) / s;
}

template <class Corner, class Rows>
__global__ void __launch_bounds__(BAKED_WAVES * 64)
baked_march_ray_bwd_kernel(const RaySrc rs, long long R, const BakedParams q, const Rows rows, const typename Corner::stored_t *__restrict__ stored,
                           const float *__restrict__ d_rgb, const float *__restrict__ d_depth, const float *__restrict__ d_alpha,
                           float *__restrict__ d_rays) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * BAKED_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;
    float *__restrict__ out = d_rays + r * 8;
    float3 drgb = make_float3(0.f, 0.f, 0.f);
    if (d_rgb) drgb = make_float3(d_rgb[r * 3], d_rgb[r * 3 + 1], d_rgb[r * 3 + 2]);
    const float ddepth = d_depth ? d_depth[r] : 0.f, dalpha = d_alpha ? d_alpha[r] : 0.f;
    if (drgb.x == 0.f && drgb.y == 0.f && drgb.z == 0.f && ddepth == 0.f && dalpha == 0.f) {  // nothing to send back: the row of zeros
        if (lane < 8) out[lane] = 0.f;
        return;
    }
    const float gwhite = q.white_bkgd ? (drgb.x + drgb.y + drgb.z) : 0.f;  // rgb += 1 - sum w
    Corner corner;
    corner.data = stored;
    const Ray8 ray = load_ray(rs, r);
    corner.set_ray(ray);
    const int n = baked_sample_count(ray, q.step);
    int nc = (n + 63) >> 6;

    // the forward's walk: T at the head of chunk c < 64 into lane c, and -- by the forward's own factors -- the chunk it stopped after
    double heads = 1.0, carry = 1.0;
    float stop = 1.f;
    for (int c = 0; c < nc; ++c) {
        if (lane == c) heads = carry;
        const BakedSample s = baked_sample(ray, q, c * 64 + lane, n);
        if (__ballot(s.active) == 0ull) continue;
        float sigma;
        carry = carry * __shfl(wave_scan_mul64(baked_tf_exact(q, corner, rows, s, sigma), lane), 63, 64);
        if (q.eps > 0.f) {  // (wave-uniform)
            stop = stop * __shfl(wave_scan_mul(baked_alpha(q.step, sigma).tfac, lane), 63, 64);
            if (stop <= q.eps) nc = c + 1;  // the forward's break, in its words
        }
    }

    constexpr int NY = BakedBasis<Corner>::N;
    double d_o[3] = {0.0, 0.0, 0.0}, d_d[3] = {0.0, 0.0, 0.0}, d_near = 0.0;  // this lane's part of the row
    float dY[NY > 0 ? NY : 1] = {};
    const float dir[3] = {ray.dx, ray.dy, ray.dz};
    double S_in = 0.0;  // S of the chunk's last sample
    for (int c = nc - 1; c >= 0; --c) {
        const BakedSample s = baked_sample(ray, q, c * 64 + lane, n);
        if (__ballot(s.active) == 0ull) continue;  // 64 identity maps: S stays, nothing to send back
        carry = __shfl(heads, c < 64 ? c : 63, 64);
        for (int cc = 63; cc < c; ++cc) carry = carry * baked_chunk_product_exact(ray, q, corner, rows, cc, n, lane);
        BakedCell<Rows> cell;
        bool found = false;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        BakedBlendGrad bg = {zero, zero, zero, zero};
        if (s.active) {
            if (baked_find_cell(q, rows, s, cell)) {
                found = true;
                bg = baked_blend_grad(corner, rows, cell, s.f);
            }
        }
        const float4 cs = bg.val;
        const BakedAlphaExact al = baked_alpha_exact(q.step, cs.w);
        // a sample that is not active, or found no rows, has a = 0 and tf = 1: the identity map
        double m = found ? al.tf : 1.0;
        const double incl = wave_scan_mul64(m, lane);
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0;
        const double T = carry * excl;
        const double g = found ? (double)(drgb.x * cs.x + drgb.y * cs.y + drgb.z * cs.z + ddepth * s.t + dalpha - gwhite) : 0.0;
        double b = found ? g * (double)al.a : 0.0;
        wave_rscan_affine64(m, b, lane);
        const double mn = __shfl_down(m, 1, 64), bn = __shfl_down(b, 1, 64);
        const double S = lane == 63 ? S_in : bn + mn * S_in;
        S_in = __shfl(b + m * S_in, 0, 64);  // S of sample 64 c - 1
        if (found) {  // (no wave operation below: the lanes part here and meet again at the head of the loop)
            const float w = (float)((double)al.a * T);
            const float da = (float)(T * (g - S));
            const float4 dcs = make_float4(w * drgb.x, w * drgb.y, w * drgb.z, da * q.step * al.ex);
            float slope[3];
            baked_frac_slope(ray, q, s, slope);
            const float dp[3] = {slope[0] * baked_dot(dcs, bg.x) / q.g.h[0], slope[1] * baked_dot(dcs, bg.y) / q.g.h[1],
                                 slope[2] * baked_dot(dcs, bg.z) / q.g.h[2]};
            float dt = ddepth * w;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                d_o[a] += (double)dp[a];
                d_d[a] += (double)s.t * (double)dp[a];
                dt += dp[a] * dir[a];
            }
            d_near += (double)dt;
            if constexpr (NY > 0) {
#pragma unroll 1
                for (int j = 0; j < 4; ++j) {  // pair j = 2 ix + iy
                    const long long row = cell.row(rows, j);
                    const float wxy = (j >> 1 ? s.f[0] : 1.f - s.f[0]) * (j & 1 ? s.f[1] : 1.f - s.f[1]);
#pragma unroll
                    for (int iz = 0; iz < 2; ++iz) {
                        const float wt = wxy * (iz ? s.f[2] : 1.f - s.f[2]);
                        if (wt != 0.f) baked_basis_grad(corner, row + iz, make_float4(wt * dcs.x, wt * dcs.y, wt * dcs.z, wt * dcs.w), dY);
                    }
                }
            }
        }
    }
    // the 64 lanes of the ray, in wave_sum's fixed order; then the basis values' share of d_d
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d_o[a] = wave_sum(d_o[a]);
        d_d[a] = wave_sum(d_d[a]);
    }
    d_near = wave_sum(d_near);
    float basis[3] = {0.f, 0.f, 0.f};
    if constexpr (NY > 0) {
#pragma unroll
        for (int k = 0; k < NY; ++k) dY[k] = wave_sum(dY[k]);
        baked_basis_to_dir(ray, dY, basis[0], basis[1], basis[2]);
    }
    if (lane == 0) {
        out[0] = (float)d_o[0]; out[1] = (float)d_o[1]; out[2] = (float)d_o[2];
        out[3] = (float)(d_d[0] + (double)basis[0]); out[4] = (float)(d_d[1] + (double)basis[1]); out[5] = (float)(d_d[2] + (double)basis[2]);
        out[6] = (float)d_near;
        out[7] = 0.f;  // far enters through the sample count alone
    }
}

// ---- backward of the SCENE march with respect to the world rays and the objects' poses (pnr_baked_scene_backward_*;
// include/pixelnerf_hip.h, "Gradients of the scene march").  baked_march_ray_bwd_kernel's walk on the mixture (c, sigma) of
// baked_scene_march_kernel: the first walk, the fp64 heads, the reverse affine scan and the rebuild beyond 4096 samples are that
// kernel's, with the mixed sigma where it has the blended one.  What a sample sends back goes through the mixing to every object
// that contributes, through that object's blend in ITS frame -- dp'_ij, on the ray (o', d') of baked_scene_ray -- and back to the
// world through R_j.  The world row keeps the single kernel's per-lane fp64 sums, so one object at [I | 0] gives its bytes; the
// six numbers of an object (dL/do', dL/dd') are summed per chunk by wave_sum and added into the ONE lane that owns accumulator
// (j, k): a pair of registers for all eight objects.  The basis sums of a coefficient volume stay per lane and per object (fp32,
// the single kernel's order: they reach d_rays through a rotation alone and must give its bytes).  No atomics, no LDS.

// first pass of the forward's mixing at sample i: sigma = sum sigma_j in list order, the first contributor's value, their number
// -> whether any object is active at the sample.  baked_scene_march_kernel's first loop, in its words
template <class Corner, class Rows>
__device__ __forceinline__ bool baked_scene_sigma(const BakedSceneDesc &sc, const Ray8 &ray, float step, int i, int n, float4 &first,
                                                  float &sigma, int &cnt) {
    first = make_float4(0.f, 0.f, 0.f, 0.f);
    sigma = 0.f;
    cnt = 0;
    bool any = false;
#pragma unroll 1
    for (int j = 0; j < sc.n; ++j) {
        bool active;
        float4 cs;
        const bool found = baked_scene_value<Corner, Rows>(sc.obj[j], ray, step, i, n, active, cs);
        any = any || active;
        if (found) {
            if (cnt == 0) first = cs;
            sigma = sigma + cs.w;
            ++cnt;
        }
    }
    return any;
}

// second pass: c = sum (sigma_j / sigma) c_j; the forward's lines after its first loop
template <class Corner, class Rows>
__device__ __forceinline__ float3 baked_scene_colour(const BakedSceneDesc &sc, const Ray8 &ray, float step, int i, int n, const float4 first,
                                                     float sigma, int cnt) {
    float cr = 0.f, cg = 0.f, cb = 0.f;
    if (cnt == 1 && sigma > 0.f) {
        const float wj = first.w / sigma;
        cr = wj * first.x; cg = wj * first.y; cb = wj * first.z;
    }
    if (__ballot(cnt >= 2) != 0ull) {
        if (cnt >= 2 && sigma > 0.f) {
#pragma unroll 1
            for (int j = 0; j < sc.n; ++j) {
                bool active;
                float4 cs;
                if (baked_scene_value<Corner, Rows>(sc.obj[j], ray, step, i, n, active, cs)) {
                    const float wj = cs.w / sigma;
                    cr = cr + wj * cs.x; cg = cg + wj * cs.y; cb = cb + wj * cs.z;
                }
            }
        }
    }
    return make_float3(cr, cg, cb);
}

// prod of the fp64 factors of the mixture over chunk c (every lane): baked_chunk_product_exact for a scene
template <class Corner, class Rows>
__device__ __forceinline__ double baked_scene_chunk_product_exact(const BakedSceneDesc &sc, const Ray8 &ray, float step, int c, int n, int lane) {
    float4 first;
    float sigma;
    int cnt;
    const bool any = baked_scene_sigma<Corner, Rows>(sc, ray, step, c * 64 + lane, n, first, sigma, cnt);
    if (__ballot(any) == 0ull) return 1.0;
    return __shfl(wave_scan_mul64(cnt > 0 ? baked_alpha_exact(step, sigma).tf : 1.0, lane), 63, 64);
}

// v rotated into the world by object-to-world R: each component (R_a0 x + R_a1 y) + R_a2 z
__device__ __forceinline__ void baked_scene_rotate(const BakedSceneObject &ob, float x, float y, float z, float (&out)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = (ob.rot[3 * a] * x + ob.rot[3 * a + 1] * y) + ob.rot[3 * a + 2] * z;
}

template <class Corner, class Rows>
__global__ void __launch_bounds__(BAKED_WAVES * 64)
baked_scene_ray_bwd_kernel(const RaySrc rs, long long R, const BakedSceneDesc sc, float step, float eps, int white_bkgd,
                           const float *__restrict__ d_rgb, const float *__restrict__ d_depth, const float *__restrict__ d_alpha,
                           float *__restrict__ d_rays, float *__restrict__ d_local) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * BAKED_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;
    float *__restrict__ out = d_rays + r * 8;
    float *__restrict__ loc_out = d_local + r * (6 * sc.n);  // lane j * 6 + k owns number k of object j
    float3 drgb = make_float3(0.f, 0.f, 0.f);
    if (d_rgb) drgb = make_float3(d_rgb[r * 3], d_rgb[r * 3 + 1], d_rgb[r * 3 + 2]);
    const float ddepth = d_depth ? d_depth[r] : 0.f, dalpha = d_alpha ? d_alpha[r] : 0.f;
    if (drgb.x == 0.f && drgb.y == 0.f && drgb.z == 0.f && ddepth == 0.f && dalpha == 0.f) {  // nothing to send back: 8 + 6 n zeros
        if (lane < 8) out[lane] = 0.f;
        if (lane < 6 * sc.n) loc_out[lane] = 0.f;
        return;
    }
    const float gwhite = white_bkgd ? (drgb.x + drgb.y + drgb.z) : 0.f;  // rgb += 1 - sum w
    const Ray8 ray = load_ray(rs, r);
    const int n = baked_sample_count(ray, step);  // the WORLD ray decides the samples
    int nc = (n + 63) >> 6;

    // the forward's walk: T at the head of chunk c < 64 into lane c, and -- by the forward's own factors -- the chunk it stopped after
    double heads = 1.0, carry = 1.0;
    float stop = 1.f;
    for (int c = 0; c < nc; ++c) {
        if (lane == c) heads = carry;
        float4 first;
        float sigma;
        int cnt;
        const bool any = baked_scene_sigma<Corner, Rows>(sc, ray, step, c * 64 + lane, n, first, sigma, cnt);
        if (__ballot(any) == 0ull) continue;
        carry = carry * __shfl(wave_scan_mul64(cnt > 0 ? baked_alpha_exact(step, sigma).tf : 1.0, lane), 63, 64);
        if (eps > 0.f) {  // (wave-uniform)
            stop = stop * __shfl(wave_scan_mul(baked_alpha(step, sigma).tfac, lane), 63, 64);
            if (stop <= eps) nc = c + 1;  // the forward's break, in its words
        }
    }

    constexpr int NY = BakedBasis<Corner>::N;
    constexpr int NYA = NY > 0 ? NY : 1;
    double d_o[3] = {0.0, 0.0, 0.0}, d_d[3] = {0.0, 0.0, 0.0}, d_near = 0.0;  // this lane's part of the world row
    double loc = 0.0;  // lane j * 6 + k: number k of (dL/do', dL/dd') of object j
    float dY[NY > 0 ? PNR_BAKED_SCENE_MAX_OBJECTS : 1][NYA] = {};  // this lane's part of dL/dY_k of every object
    double S_in = 0.0;  // S of the chunk's last sample
    for (int c = nc - 1; c >= 0; --c) {
        const int i = c * 64 + lane;
        const float t = ray.near + ((float)i + 0.5f) * step;  // baked_sample's depth
        float4 first;
        float sigma;
        int cnt;
        const bool any = baked_scene_sigma<Corner, Rows>(sc, ray, step, i, n, first, sigma, cnt);
        if (__ballot(any) == 0ull) continue;  // 64 identity maps: S stays, nothing to send back
        const float3 col = baked_scene_colour<Corner, Rows>(sc, ray, step, i, n, first, sigma, cnt);
        carry = __shfl(heads, c < 64 ? c : 63, 64);
        for (int cc = 63; cc < c; ++cc) carry = carry * baked_scene_chunk_product_exact<Corner, Rows>(sc, ray, step, cc, n, lane);
        const bool mixed = cnt > 0;  // the single kernel's `found`
        const BakedAlphaExact al = baked_alpha_exact(step, sigma);
        double m = mixed ? al.tf : 1.0;
        const double incl = wave_scan_mul64(m, lane);
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0;
        const double T = carry * excl;
        const double g = mixed ? (double)(drgb.x * col.x + drgb.y * col.y + drgb.z * col.z + ddepth * t + dalpha - gwhite) : 0.0;
        double b = mixed ? g * (double)al.a : 0.0;
        wave_rscan_affine64(m, b, lane);
        const double mn = __shfl_down(m, 1, 64), bn = __shfl_down(b, 1, 64);
        const double S = lane == 63 ? S_in : bn + mn * S_in;
        S_in = __shfl(b + m * S_in, 0, 64);  // S of sample 64 c - 1
        // dL/dc_i and dL/dsigma_i of the mixture; zeros in a lane nothing contributes to
        const float w = mixed ? (float)((double)al.a * T) : 0.f;
        const float da = mixed ? (float)(T * (g - S)) : 0.f;
        const float3 dc = make_float3(w * drgb.x, w * drgb.y, w * drgb.z);
        const float dsig = da * step * al.ex;
        float dpw[3] = {0.f, 0.f, 0.f};  // dL/dp_i in the world: sum_j R_j dp'_ij, objects in list order
        // dL/dt_i = d_depth w_i + sum_j dp'_ij . d'_j.  Per object the single kernel's fp32 chain ((d_depth w_i + x) + y) + z, the
        // chains summed in fp64 and the (cnt - 1) extra d_depth w_i taken off again: one contributor is that kernel's number, two commute
        const float dt0 = ddepth * w;
        double dtsum = 0.0;
#pragma unroll 1
        for (int j = 0; j < sc.n; ++j) {
            const BakedSceneObject &ob = sc.obj[j];
            // baked_scene_value's steps, with the partials of the blend where it takes the value
            const Ray8 oray = baked_scene_ray(ray, ob);
            const float oo[3] = {oray.ox, oray.oy, oray.oz}, od[3] = {oray.dx, oray.dy, oray.dz};
            bool inside = i < n;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float p = oo[a] + t * od[a];
                inside = inside && p >= ob.g.c1[a] && p <= ob.g.c2[a];
            }
            if (__ballot(inside) == 0ull) continue;
            BakedParams q;
            q.bits = ob.bits;
            q.g = ob.g;
            q.step = step;
            q.eps = 0.f;
            q.white_bkgd = 0;
            const BakedSample s = baked_sample(oray, q, i, n);
            if (__ballot(s.active) == 0ull) continue;
            Corner corner;
            corner.data = static_cast<const typename Corner::stored_t *>(ob.stored);
            corner.set_ray(oray);
            const Rows rows = baked_scene_rows<Rows>(ob);
            BakedCell<Rows> cell;
            bool found = false;
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            BakedBlendGrad bg = {zero, zero, zero, zero};
            if (s.active) {
                if (baked_find_cell(q, rows, s, cell)) {
                    found = true;
                    bg = baked_blend_grad(corner, rows, cell, s.f);
                }
            }
            if (__ballot(found) == 0ull) continue;
            float dp[3] = {0.f, 0.f, 0.f};  // dp'_ij
            float ys[NYA];
            if constexpr (NY > 0) {
#pragma unroll
                for (int jj = 0; jj < PNR_BAKED_SCENE_MAX_OBJECTS; ++jj)
                    if (jj == j) {
#pragma unroll
                        for (int k = 0; k < NY; ++k) ys[k] = dY[jj][k];
                    }
            }
            if (found) {
                const float4 cs = bg.val;
                // through the mixing; where sigma is not > 0 the forward's colour is the constant 0
                float wj = 0.f, dsj = dsig;
                if (sigma > 0.f) {
                    wj = cs.w / sigma;
                    dsj = dsig + ((cs.x - col.x) * dc.x + (cs.y - col.y) * dc.y + (cs.z - col.z) * dc.z) / sigma;
                }
                const float4 dcs = make_float4(wj * dc.x, wj * dc.y, wj * dc.z, dsj);
                float slope[3];
                baked_frac_slope(oray, q, s, slope);
                dp[0] = slope[0] * baked_dot(dcs, bg.x) / q.g.h[0];
                dp[1] = slope[1] * baked_dot(dcs, bg.y) / q.g.h[1];
                dp[2] = slope[2] * baked_dot(dcs, bg.z) / q.g.h[2];
                float rot[3];
                baked_scene_rotate(ob, dp[0], dp[1], dp[2], rot);
                float dt = dt0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    dpw[a] += rot[a];
                    dt += dp[a] * od[a];
                }
                dtsum += (double)dt;
                if constexpr (NY > 0) {
#pragma unroll 1
                    for (int pj = 0; pj < 4; ++pj) {  // pair pj = 2 ix + iy
                        const long long row = cell.row(rows, pj);
                        const float wxy = (pj >> 1 ? s.f[0] : 1.f - s.f[0]) * (pj & 1 ? s.f[1] : 1.f - s.f[1]);
#pragma unroll
                        for (int iz = 0; iz < 2; ++iz) {
                            const float wt = wxy * (iz ? s.f[2] : 1.f - s.f[2]);
                            if (wt != 0.f) baked_basis_grad(corner, row + iz, make_float4(wt * dcs.x, wt * dcs.y, wt * dcs.z, wt * dcs.w), ys);
                        }
                    }
                }
            }
            if constexpr (NY > 0) {
#pragma unroll
                for (int jj = 0; jj < PNR_BAKED_SCENE_MAX_OBJECTS; ++jj)
                    if (jj == j) {
#pragma unroll
                        for (int k = 0; k < NY; ++k) dY[jj][k] = ys[k];
                    }
            }
            // the object's six numbers of this chunk: the butterfly, then into the lane that owns (j, k)
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double v = wave_sum(k < 3 ? (double)dp[k] : (double)t * (double)dp[k - 3]);
                if (lane == j * 6 + k) loc += v;
            }
        }
        if (mixed) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                d_o[a] += (double)dpw[a];
                d_d[a] += (double)t * (double)dpw[a];
            }
            d_near += cnt > 1 ? dtsum - (double)(cnt - 1) * (double)dt0 : dtsum;
        }
    }
    // the 64 lanes of the ray, in wave_sum's fixed order; then the basis values' share of d_d, object by object
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d_o[a] = wave_sum(d_o[a]);
        d_d[a] = wave_sum(d_d[a]);
    }
    d_near = wave_sum(d_near);
    float basis[3] = {0.f, 0.f, 0.f};
    if constexpr (NY > 0) {
#pragma unroll
        for (int jj = 0; jj < PNR_BAKED_SCENE_MAX_OBJECTS; ++jj) {
            if (jj < sc.n) {
                float ys[NY];
#pragma unroll
                for (int k = 0; k < NY; ++k) ys[k] = wave_sum(dY[jj][k]);
                float bo[3] = {0.f, 0.f, 0.f};
                baked_basis_to_dir(baked_scene_ray(ray, sc.obj[jj]), ys, bo[0], bo[1], bo[2]);
                float rot[3];
                baked_scene_rotate(sc.obj[jj], bo[0], bo[1], bo[2], rot);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    basis[a] += rot[a];
                    if (lane == jj * 6 + 3 + a) loc += (double)bo[a];
                }
            }
        }
    }
    if (lane == 0) {
        out[0] = (float)d_o[0]; out[1] = (float)d_o[1]; out[2] = (float)d_o[2];
        out[3] = (float)(d_d[0] + (double)basis[0]); out[4] = (float)(d_d[1] + (double)basis[1]); out[5] = (float)(d_d[2] + (double)basis[2]);
        out[6] = (float)d_near;
        out[7] = 0.f;  // far enters through the sample count alone
    }
    if (lane < 6 * sc.n) loc_out[lane] = (float)loc;
}

// ---- the poses' gradient from d_local: dL/dR_j[r][a] = sum_rays (q_r d_local.o'_a + d_r d_local.d'_a), q = o - t_j as the march
// forms it, and dL/dt_j[r] = - sum_rays sum_a R_j[r][a] d_local.o'_a.  Blocks of ONE wave (no LDS): a thread over the rays it owns,
// the lanes by wave_sum's butterfly, one partial of 12 doubles per (block, object); then one wave per object over the block
// partials.  Every order is fixed by R and n_objects alone.  The rays are regenerated from the march's ray source.
constexpr int POSE_MAX_BLOCKS = 512;

__global__ void __launch_bounds__(64)
baked_scene_pose_partial_kernel(const RaySrc rs, long long R, const BakedSceneDesc sc, const float *__restrict__ d_local,
                                double *__restrict__ partials /*(gridDim.x, n, 12)*/) {
    const int j = blockIdx.y;
    const BakedSceneObject &ob = sc.obj[j];
    double acc[12] = {};
    for (long long r = (long long)blockIdx.x * 64 + threadIdx.x; r < R; r += (long long)gridDim.x * 64) {
        const float *__restrict__ g = d_local + (r * sc.n + j) * 6;
        const float go[3] = {g[0], g[1], g[2]}, gd[3] = {g[3], g[4], g[5]};
        if (go[0] == 0.f && go[1] == 0.f && go[2] == 0.f && gd[0] == 0.f && gd[1] == 0.f && gd[2] == 0.f) continue;  // the ray misses the object
        const Ray8 ray = load_ray(rs, r);
        const float q[3] = {ray.ox - ob.t[0], ray.oy - ob.t[1], ray.oz - ob.t[2]}, d[3] = {ray.dx, ray.dy, ray.dz};
#pragma unroll
        for (int row = 0; row < 3; ++row) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                acc[4 * row + a] += (double)q[row] * (double)go[a] + (double)d[row] * (double)gd[a];
                acc[4 * row + 3] -= (double)ob.rot[3 * row + a] * (double)go[a];
            }
        }
    }
    double *__restrict__ dst = partials + ((long long)blockIdx.x * sc.n + j) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double v = wave_sum(acc[k]);
        if (threadIdx.x == 0) dst[k] = v;
    }
}

// one wave per object over the block partials -> d_poses (n,12), rounded to fp32 once; blocks == 0 (no rays): zeros
__global__ void __launch_bounds__(64)
baked_scene_pose_final_kernel(const double *__restrict__ partials, int blocks, int n_objects, float *__restrict__ d_poses) {
    const int j = blockIdx.x;
    double acc[12] = {};
    for (int b = threadIdx.x; b < blocks; b += 64) {
        const double *__restrict__ src = partials + ((long long)b * n_objects + j) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[k] += src[k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double v = wave_sum(acc[k]);
        if (threadIdx.x == 0) d_poses[j * 12 + k] = (float)v;
    }
}
#pragma clang fp contract(fast)

static bool baked_misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// ---- host only from here.  The rays of a march with their own checks, made where the entry's arguments are (pnr_entry.h's
// explicit_rays for the baked entries).  defect: what is wrong with them (NULL: nothing); baked_render reports it after the
// entry's degree check, which every entry makes first.
struct BakedRays {
    RaySrc src;
    long long R;
    const char *defect;
};

static BakedRays baked_explicit_rays(const float *rays, long long R) {
    BakedRays s = {};
    s.src.rays = rays;
    s.R = R;
    s.defect = R < 0 ? "bad sizes (R)" : R > 0 && !rays ? "null argument"
               : baked_misaligned4(rays) ? "rays must be 4-byte aligned" : nullptr;
    return s;
}

static BakedRays baked_camera_rays(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
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

static BakedVolumeDesc baked_dense(const void *stored, int degree, bool half, const char *name, int min_degree, const char *degree_rule) {
    return {stored, degree, half, false, nullptr, 0, name, min_degree, degree_rule};
}
static BakedVolumeDesc baked_sparse(const void *rows, long long M, const int32_t *index, int degree, bool half, const char *degree_rule) {
    return {rows, degree, half, true, index, M, "rows", -1, degree_rule};
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
};

// ranks are int32: a row beyond 2^31 - 2 cannot be named.  M < 2 (last < 0): no sample finds its rows, nothing is read
static SparseRows baked_sparse_rows(const BakedVolumeDesc &v) {
    return SparseRows{v.index, (int)(v.M - 2 < 0x7ffffffeLL ? v.M - 2 : 0x7ffffffeLL)};
}

// every check of every entry, forward (grads == NULL: a's rgb, depth and alpha are written) and backward, in one order.
// -> PNR_OK with `blocks` workgroups to launch (0: no rays, nothing to do) and the march settings in q
static int baked_check(const char *entry, const BakedRays &rays, const BakedVolumeDesc &v, const BakedMarchArgs &a, const BakedGrads *grads,
                       BakedParams &q, long long &blocks) {
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
    if (grads ? !grads->out : !a.rgb || !a.depth || !a.alpha) return occ_fail(entry, "null argument");
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

// The backward entries: fp32 storage, dense (index == NULL) or sparse rows, degree -1..2: 2 x 4 instantiations.
static int baked_backward(const char *entry, const BakedRays &rays, const void *stored, long long M, int degree, const int32_t *index,
                          const BakedMarchArgs &a, const BakedGrads &grads) {
    const BakedVolumeDesc v = {stored, degree, false, index != nullptr, index, index ? M : 0, "stored", -1, DEGREE_HALF};
    BakedParams q;
    long long blocks;
    if (const int rc = baked_check(entry, rays, v, a, &grads, q, blocks)) return rc;
    if (blocks == 0) return PNR_OK;
    const auto launch = [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        hipLaunchKernelGGL((baked_march_bwd_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                           (hipStream_t)a.stream, rays.src, rays.R, q, rows, static_cast<const float4 *>(v.stored), grads.d_rgb,
                           grads.d_depth, grads.d_alpha, grads.out);
    };
    const auto by_kind = [&](auto rows) {
        if (v.degree < 0) launch(BakedType<RgbaCornerOf<float4>>{}, rows);
        else if (v.degree == 0) launch(BakedType<ShCorner<1, float4>>{}, rows);
        else if (v.degree == 1) launch(BakedType<ShCorner<4, float4>>{}, rows);
        else launch(BakedType<ShCorner<9, float4>>{}, rows);
    };
    if (v.sparse) by_kind(baked_sparse_rows(v));
    else by_kind(DenseRows{});
    return pnr_check_launch(entry);
}

// The ray-gradient entries: fp32 or fp16 storage, dense (index == NULL) or sparse rows, degree -1..2: the forward's 16 instantiations.
static int baked_ray_backward(const char *entry, const BakedRays &rays, const void *stored, int storage_half, long long M, int degree,
                              const int32_t *index, const BakedMarchArgs &a, const BakedGrads &grads) {
    BakedVolumeDesc v = {stored, degree, storage_half == 1, index != nullptr, index, index ? M : 0, "stored", -1, DEGREE_HALF};
    v.bad_storage = storage_half != 0 && storage_half != 1;
    BakedParams q;
    long long blocks;
    if (const int rc = baked_check(entry, rays, v, a, &grads, q, blocks)) return rc;
    if (blocks == 0) return PNR_OK;
    const auto launch = [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        hipLaunchKernelGGL((baked_march_ray_bwd_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                           (hipStream_t)a.stream, rays.src, rays.R, q, rows, static_cast<const typename Corner::stored_t *>(v.stored),
                           grads.d_rgb, grads.d_depth, grads.d_alpha, grads.out);
    };
    const auto by_kind = [&](auto stored_type, auto rows) {
        using Stored = typename decltype(stored_type)::type;
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
    return pnr_check_launch(entry);
}

// the forward entries: the checks, then the launch
static int baked_render(const char *entry, const BakedRays &rays, const BakedVolumeDesc &v, const BakedMarchArgs &a) {
    BakedParams q;
    long long blocks;
    if (const int rc = baked_check(entry, rays, v, a, nullptr, q, blocks)) return rc;
    if (blocks == 0) return PNR_OK;
    const long long R = rays.R;
    // layout, storage and kind, each decided once: 2 x 2 x 4 instantiations of the one kernel
    const auto launch = [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        hipLaunchKernelGGL((baked_march_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                           (hipStream_t)a.stream, rays.src, R, q, rows, static_cast<const typename Corner::stored_t *>(v.stored), a.rgb,
                           a.depth, a.alpha);
    };
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
    return pnr_check_launch(entry);
}

// [R | t] of a PnrBakedObject: finite, max |R^T R - I| <= 1e-4 and det R > 0, in fp64
static bool baked_pose_rigid(const float *pose) {
    double m[3][3];
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(pose[k])) return false;
    for (int r = 0; r < 3; ++r)
        for (int a = 0; a < 3; ++a) m[r][a] = pose[4 * r + a];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double dot = m[0][a] * m[0][b] + m[1][a] * m[1][b] + m[2][a] * m[2][b];
            if (!(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-4)) return false;
        }
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    return det > 0.0;
}

static bool baked_misaligned8(const void *p);

// what a scene entry writes.  Forward: rgb, depth, alpha (grads == NULL).  Backward: d_rays and d_local stand in their place
// (out[2] repeats d_local), grads holds the upstream gradients, and d_poses (nullable) needs the workspace.
struct BakedSceneOut {
    float *out[3];
    const BakedGrads *grads;
    float *d_poses;
    void *workspace;
};

// Every check of the four scene entries, in one order: what concerns the call as a whole, then every object through baked_check
// under "entry: object j".  -> PNR_OK with the scene as the kernels take it, the kind in v0 and `blocks` workgroups (0: no rays)
static int baked_scene_check(const char *entry, const BakedRays &rays, const PnrBakedObject *objects, int n_objects, float step,
                             int white_bkgd, float terminate, const BakedSceneOut &o, void *stream, BakedSceneDesc &sc, BakedVolumeDesc &v0,
                             long long &blocks) {
    float *const rgb = o.out[0], *const depth = o.out[1], *const alpha = o.out[2];
    blocks = 0;
    if (n_objects < 1 || n_objects > PNR_BAKED_SCENE_MAX_OBJECTS) return occ_fail(entry, "n_objects must lie in [1, 8]");
    if (!objects) return occ_fail(entry, "null argument (objects)");
    char where[96], why[96];
    for (int j = 0; j < n_objects; ++j) {
        const PnrBakedObject &ob = objects[j], &ob0 = objects[0];
        if (ob.reserved != 0) {
            std::snprintf(why, sizeof(why), "object %d: reserved must be 0", j);
            return occ_fail(entry, why);
        }
        if (ob.degree != ob0.degree || ob.storage_half != ob0.storage_half || (ob.index != nullptr) != (ob0.index != nullptr)) {
            std::snprintf(why, sizeof(why), "object %d: mixed kinds (degree, storage_half and index must be those of object 0)", j);
            return occ_fail(entry, why);
        }
    }
    if (rays.defect) return occ_fail(entry, rays.defect);
    if (!(step > 0.f) || !std::isfinite(step)) return occ_fail(entry, "step must be finite and > 0");
    if (!(terminate >= 0.f && terminate < 1.f)) return occ_fail(entry, "terminate must lie in [0, 1)");
    if (rays.R > 0 && (!rgb || !depth || !alpha)) return occ_fail(entry, "null argument");
    if (o.grads) {  // (a misaligned d_poses is wrong whatever R: it is written at R = 0 too)
        if (baked_misaligned4(o.grads->d_rgb) || baked_misaligned4(o.grads->d_depth) || baked_misaligned4(o.grads->d_alpha) ||
            baked_misaligned4(rgb) || baked_misaligned4(depth) || baked_misaligned4(o.d_poses))
            return occ_fail(entry, "d_rgb, d_depth, d_alpha, d_rays, d_local and d_poses must be 4-byte aligned");
        if (o.d_poses && (!o.workspace || baked_misaligned8(o.workspace)))
            return occ_fail(entry, "d_poses needs the workspace of pnr_baked_scene_backward_workspace_bytes(), 8-byte aligned");
    } else if (rays.R > 0 && (baked_misaligned4(rgb) || baked_misaligned4(depth) || baked_misaligned4(alpha))) {
        return occ_fail(entry, "rgb, depth and alpha must be 4-byte aligned");
    }
    sc = {};
    sc.n = n_objects;
    v0 = {};
    for (int j = 0; j < n_objects; ++j) {
        const PnrBakedObject &ob = objects[j];
        std::snprintf(where, sizeof(where), "%s: object %d", entry, j);
        BakedVolumeDesc v = {ob.stored, ob.degree, ob.storage_half == 1, ob.index != nullptr, ob.index, ob.index ? ob.M : 0, "stored", -1,
                             DEGREE_HALF};
        v.bad_storage = ob.storage_half != 0 && ob.storage_half != 1;
        BakedParams q;
        if (const int rc = baked_check(where, rays, v, {ob.bits, ob.nx, ob.ny, ob.nz, ob.c1, ob.c2, step, white_bkgd, terminate, rgb, depth,
                                                        alpha, stream}, o.grads, q, blocks))
            return rc;
        if (!baked_pose_rigid(ob.pose)) return occ_fail(where, "pose must be finite and rigid (max |R^T R - I| <= 1e-4, det R > 0)");
        BakedSceneObject &o = sc.obj[j];
        o.stored = ob.stored;
        o.bits = ob.bits;
        o.index = ob.index;
        o.last = v.sparse ? baked_sparse_rows(v).last : -1;
        o.g = q.g;
        for (int r = 0; r < 3; ++r) {
            for (int a = 0; a < 3; ++a) o.rot[3 * r + a] = ob.pose[4 * r + a];
            o.t[r] = ob.pose[4 * r + 3];
        }
        if (j == 0) v0 = v;
    }
    return PNR_OK;
}

// layout, storage and kind of a scene, each decided once: launch(BakedType<Corner>, BakedType<Rows>) on one of 16 instantiations
template <class Launch>
static void baked_scene_dispatch(const BakedVolumeDesc &v0, const Launch &launch) {
    const auto by_kind = [&](auto stored, auto rows) {
        using Stored = typename decltype(stored)::type;
        if (v0.degree < 0) launch(BakedType<RgbaCornerOf<Stored>>{}, rows);
        else if (v0.degree == 0) launch(BakedType<ShCorner<1, Stored>>{}, rows);
        else if (v0.degree == 1) launch(BakedType<ShCorner<4, Stored>>{}, rows);
        else launch(BakedType<ShCorner<9, Stored>>{}, rows);
    };
    const auto by_storage = [&](auto rows) {
        if (v0.half) by_kind(BakedType<Half4>{}, rows);
        else by_kind(BakedType<float4>{}, rows);
    };
    if (v0.sparse) by_storage(BakedType<SparseRows>{});
    else by_storage(BakedType<DenseRows>{});
}

// the scene's forward entries: the checks, then the launch
static int baked_scene_render(const char *entry, const BakedRays &rays, const PnrBakedObject *objects, int n_objects, float step,
                              int white_bkgd, float terminate, float *rgb, float *depth, float *alpha, void *stream) {
    BakedSceneDesc sc;
    BakedVolumeDesc v0;
    long long blocks;
    if (const int rc = baked_scene_check(entry, rays, objects, n_objects, step, white_bkgd, terminate, {{rgb, depth, alpha}, nullptr, nullptr, nullptr},
                                         stream, sc, v0, blocks))
        return rc;
    if (blocks == 0) return PNR_OK;
    baked_scene_dispatch(v0, [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        hipLaunchKernelGGL((baked_scene_march_kernel<Corner, typename decltype(rows)::type>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64),
                           0, (hipStream_t)stream, rays.src, rays.R, sc, step, terminate, white_bkgd, rgb, depth, alpha);
    });
    return pnr_check_launch(entry);
}

// the scene's backward entries: the same checks, the march's backward, then -- with d_poses -- the reduction over the rays
static int baked_scene_backward(const char *entry, const BakedRays &rays, const PnrBakedObject *objects, int n_objects, float step,
                                int white_bkgd, float terminate, const float *d_rgb, const float *d_depth, const float *d_alpha, float *d_rays,
                                float *d_local, float *d_poses, void *workspace, void *stream) {
    const BakedGrads grads = {d_rgb, d_depth, d_alpha, d_rays, "d_rays"};
    BakedSceneDesc sc;
    BakedVolumeDesc v0;
    long long blocks;
    if (const int rc = baked_scene_check(entry, rays, objects, n_objects, step, white_bkgd, terminate,
                                         {{d_rays, d_local, d_local}, &grads, d_poses, workspace}, stream, sc, v0, blocks))
        return rc;
    if (blocks > 0) {
        baked_scene_dispatch(v0, [&](auto corner, auto rows) {
            using Corner = typename decltype(corner)::type;
            hipLaunchKernelGGL((baked_scene_ray_bwd_kernel<Corner, typename decltype(rows)::type>), dim3((unsigned)blocks),
                               dim3(BAKED_WAVES * 64), 0, (hipStream_t)stream, rays.src, rays.R, sc, step, terminate, white_bkgd, d_rgb, d_depth,
                               d_alpha, d_rays, d_local);
        });
        if (const int rc = pnr_check_launch(entry)) return rc;
    }
    if (!d_poses) return PNR_OK;
    const long long waves = (rays.R + 63) / 64;
    const int pblocks = (int)(waves < POSE_MAX_BLOCKS ? waves : POSE_MAX_BLOCKS);  // 0: no rays, the poses' gradient is zeros
    double *partials = static_cast<double *>(workspace);
    if (pblocks > 0) {
        hipLaunchKernelGGL(baked_scene_pose_partial_kernel, dim3((unsigned)pblocks, (unsigned)n_objects), dim3(64), 0, (hipStream_t)stream,
                           rays.src, rays.R, sc, d_local, partials);
        if (const int rc = pnr_check_launch(entry)) return rc;
    }
    hipLaunchKernelGGL(baked_scene_pose_final_kernel, dim3((unsigned)n_objects), dim3(64), 0, (hipStream_t)stream, partials, pblocks, n_objects,
                       d_poses);
    return pnr_check_launch(entry);
}
// keep[p] for the pair (2 j, 2 j + 1) of grid points: a point is a corner of the cells (i - a, j - b, k - c), a, b, c in {0, 1},
// that exist; the pair is kept whole when either point is a corner of an occupied one
constexpr int SPARSE_MARK_THREADS = 256;

__device__ __forceinline__ bool sparse_is_corner(const uint32_t *__restrict__ bits, long long p, int nx, int ny, int nz) {
    const int k = (int)(p % nz), j = (int)((p / nz) % ny), i = (int)(p / ((long long)ny * nz));
    bool on = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ci = i - (c >> 2), cj = j - ((c >> 1) & 1), ck = k - (c & 1);
        if (ci < 0 || cj < 0 || ck < 0 || ci > nx - 2 || cj > ny - 2 || ck > nz - 2) continue;  // no such cell: the point is on a face
        const long long cell = ((long long)ci * (ny - 1) + cj) * (nz - 1) + ck;
        on = on || (bits[cell >> 5] >> (cell & 31) & 1u);
    }
    return on;
}

__global__ void __launch_bounds__(SPARSE_MARK_THREADS)
sparse_points_mark_kernel(const uint32_t *__restrict__ bits, int nx, int ny, int nz, long long P, uint8_t *__restrict__ keep) {
    const long long pair = (long long)blockIdx.x * SPARSE_MARK_THREADS + threadIdx.x;
    const long long p = 2 * pair;
    if (p >= P) return;
    bool on = sparse_is_corner(bits, p, nx, ny, nz);
    if (p + 1 < P) on = sparse_is_corner(bits, p + 1, nx, ny, nz) || on;  // (an odd P: the last point has no partner)
    keep[p] = on ? 1 : 0;
    if (p + 1 < P) keep[p + 1] = on ? 1 : 0;
}

// ---- total variation of the stored values (pnr_baked_tv; include/pixelnerf_hip.h, "Total-variation prior"): the smoothness prior
// of a fit.  The array is taken as float4s -- a row is B of them, z the fastest grid axis -- and one thread takes one float4
// (point p, basis k): consecutive lanes read consecutive 16-byte words, and the neighbour of p along an axis is a fixed offset
// (dense) or the row index[p +- offset] (sparse).  One pass gives both halves; at most TV_MAX_BLOCKS workgroups, each walking its
// slab of the array with the stride of the workgroups that share the slab.  The value: each thread adds w . n(p) in fp64, a
// block leaves one partial, baked_tv_final_kernel adds the partials; every order is fixed by the launch, which depends on the
// sizes alone.  The gradient in GATHER form: the thread that owns S[p] recomputes the norms of its three back neighbours (a
// 13-point stencil) and adds into grad[p] alone -- no atomics, the same bytes on every call.
constexpr int TV_THREADS = 256;
constexpr int TV_MAX_BLOCKS = 2048;  // 8 workgroups on each of 256 CUs; a larger volume is walked with the grid's stride

struct TvWeights {
    float w[36], wn[36];  // per element of a row: the weight, and fp32(weight / N) rounded once from fp64
};

struct TvParams {
    int nx, ny, nz;
    long long P, rows;           // nx ny nz; N: P, or the M kept rows
    const int32_t *index, *ids;  // sparse: (nx,ny,nz) ranks, (M) linear ids
    float eps;
    const float *scale;          // one float on the device, or NULL: 1
};

#pragma clang fp contract(off)  // differences, squares, sums, square roots and quotients: each rounded on its own

__device__ __forceinline__ float4 tv_diff(const float4 b, const float4 a) { return make_float4(b.x - a.x, b.y - a.y, b.z - a.z, b.w - a.w); }

__device__ __forceinline__ float4 tv_norm(const float4 dx, const float4 dy, const float4 dz, float eps) {
    return make_float4(sqrtf(dx.x * dx.x + dy.x * dy.x + dz.x * dz.x + eps), sqrtf(dx.y * dx.y + dy.y * dy.y + dz.y * dz.y + eps),
                       sqrtf(dx.z * dx.z + dy.z * dy.z + dz.z * dz.z + eps), sqrtf(dx.w * dx.w + dy.w * dy.w + dz.w * dz.w + eps));
}

// the four partials of a block in wave order; thread 0 returns the block's sum
__device__ __forceinline__ double tv_block_sum(double acc, double *wave_part) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

template <int B, bool SPARSE, bool GRAD>
__global__ void __launch_bounds__(TV_THREADS)
baked_tv_kernel(const float4 *__restrict__ S, float4 *__restrict__ grad, const TvParams q, const TvWeights wt, double *__restrict__ partials) {
    __shared__ float4 sw[B], swn[B];
    __shared__ double wave_part[TV_THREADS / 64];
#pragma unroll
    for (int b = 0; b < B; ++b) {  // (constant indices into the kernel's arguments)
        if (threadIdx.x == b) {
            sw[b] = make_float4(wt.w[4 * b], wt.w[4 * b + 1], wt.w[4 * b + 2], wt.w[4 * b + 3]);
            swn[b] = make_float4(wt.wn[4 * b], wt.wn[4 * b + 1], wt.wn[4 * b + 2], wt.wn[4 * b + 3]);
        }
    }
    __syncthreads();
    const long long total = q.rows * B, sx = (long long)q.ny * q.nz, sy = q.nz;
    const bool small = q.P <= 0xffffffffLL;  // the point's coordinates by 32-bit divisions
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 1.f;
    if (GRAD && q.scale) s = *q.scale;
    double acc = 0.0;
    // Consecutive workgroups go to different XCDs, each with an L2 of its own, and 6 of a gradient thread's 13 reads lie one x-plane
    // away.  So the array is cut into 8 contiguous slabs and workgroup b walks slab b % 8: a plane read as "own" in one step is the
    // "x - 1" / "x + 1" plane of the same L2's neighbouring steps (measured: 12 - 14 % on the large volumes, profiles/baked_notes.md).
    // Which slab a float4 falls in depends on the sizes alone.  A grid that is no multiple of 8 is small: one plain stride.
    const bool slabs = (gridDim.x & 7) == 0;
    const long long per = slabs ? (total + 8 * TV_THREADS - 1) / (8 * TV_THREADS) * TV_THREADS : total;
    const long long first = slabs ? (long long)(blockIdx.x & 7) * per : 0;
    const long long lb = slabs ? blockIdx.x >> 3 : blockIdx.x, nb = slabs ? gridDim.x >> 3 : gridDim.x;
    for (long long u = lb * TV_THREADS + threadIdx.x; u < per; u += nb * TV_THREADS) {
        const long long t = first + u;
        if (t >= total) continue;  // (the last slab may be short)
        const long long m = t / B;
        const int kb = (int)(t - m * B);
        long long p = m;
        if (SPARSE) {
            p = q.ids[m];
            if (p < 0 || p >= q.P) continue;  // not a point of the grid: nothing is read for it
        }
        int i, j, k;
        if (small) {
            const uint32_t u = (uint32_t)p, r = u / (uint32_t)q.nz;
            k = (int)(u - r * (uint32_t)q.nz);
            i = (int)(r / (uint32_t)q.ny);
            j = (int)(r - (uint32_t)i * (uint32_t)q.ny);
        } else {
            const long long r = p / q.nz;
            k = (int)(p - r * q.nz);
            i = (int)(r / q.ny);
            j = (int)(r - (long long)i * q.ny);
        }
        // the float4 (p + delta, kb) for a point p + delta INSIDE the grid; -1: that point is not kept
        const auto at = [&](long long delta) -> long long {
            if (!SPARSE) return t + delta * B;
            const long long r = q.index[p + delta];
            return r >= 0 && r < q.rows ? r * B + kb : -1;
        };
        // S[from + e_a] - base, or zeros where there is no such point
        const auto forward = [&](bool inside, long long delta, const float4 base) -> float4 {
            if (!inside) return zero;
            const long long e = at(delta);
            return e >= 0 ? tv_diff(S[e], base) : zero;
        };
        const bool fx = i + 1 < q.nx, fy = j + 1 < q.ny, fz = k + 1 < q.nz;
        const float4 v = S[t];
        const float4 dx = forward(fx, sx, v), dy = forward(fy, sy, v), dz = forward(fz, 1, v);
        const float4 n = tv_norm(dx, dy, dz, q.eps);
        if (partials) {
            const float4 w = sw[kb];
            acc += (((double)w.x * (double)n.x + (double)w.y * (double)n.y) + (double)w.z * (double)n.z) + (double)w.w * (double)n.w;
        }
        if (GRAD) {
            float4 g = make_float4(-((dx.x + dy.x + dz.x) / n.x), -((dx.y + dy.y + dz.y) / n.y), -((dx.z + dy.z + dz.z) / n.z),
                                   -((dx.w + dy.w + dz.w) / n.w));
            // the back neighbour q = p - e_a: its own difference along a ends at p, its other two end at p - e_a + e_b
            const auto back = [&](bool inside, long long delta, int axis) {
                if (!inside) return;
                const long long e = at(delta);
                if (e < 0) return;
                const float4 vq = S[e];
                const float4 da = tv_diff(v, vq);
                const float4 qx = axis == 0 ? da : forward(fx, delta + sx, vq);
                const float4 qy = axis == 1 ? da : forward(fy, delta + sy, vq);
                const float4 qz = axis == 2 ? da : forward(fz, delta + 1, vq);
                const float4 nq = tv_norm(qx, qy, qz, q.eps);
                g = make_float4(g.x + da.x / nq.x, g.y + da.y / nq.y, g.z + da.z / nq.z, g.w + da.w / nq.w);
            };
            back(i > 0, -sx, 0);
            back(j > 0, -sy, 1);
            back(k > 0, -1, 2);
            const float4 wn = swn[kb];
            float4 o = grad[t];
            o.x += s * (wn.x * g.x);
            o.y += s * (wn.y * g.y);
            o.z += s * (wn.z * g.z);
            o.w += s * (wn.w * g.w);
            grad[t] = o;
        }
    }
    if (partials) {  // (the same in every thread)
        const double sum = tv_block_sum(acc, wave_part);
        if (threadIdx.x == 0) partials[blockIdx.x] = sum;
    }
}

// the block partials in a fixed order -> sum / N as one fp64 and one fp32 number; n == 0 (no rows): 0
__global__ void __launch_bounds__(TV_THREADS)
baked_tv_final_kernel(const double *__restrict__ partials, int n, double rows, float *__restrict__ value32, double *__restrict__ value64) {
    __shared__ double wave_part[TV_THREADS / 64];
    double acc = 0.0;
    for (int b = threadIdx.x; b < n; b += TV_THREADS) acc += partials[b];
    const double sum = tv_block_sum(acc, wave_part);
    if (threadIdx.x == 0) {
        const double value = n > 0 ? sum / rows : 0.0;
        if (value64) *value64 = value;
        if (value32) *value32 = (float)value;
    }
}
#pragma clang fp contract(fast)

static bool baked_misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

}  // namespace pnr

// Every entry: its ray source, what it was handed, the tail of its argument list.

extern "C" int pnr_baked_render_rays(const float *rays, long long R, const float *vol, const uint32_t *bits, int nx, int ny, int nz,
                                     const float *c1, const float *c2, float step, int white_bkgd, float terminate, float *rgb,
                                     float *depth, float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_render_rays", pnr::baked_explicit_rays(rays, R),
                             pnr::baked_dense(vol, -1, false, "vol", -1, nullptr),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

extern "C" int pnr_baked_render_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                      float z_far, const float *vol, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                      const float *c2, float step, int white_bkgd, float terminate, float *rgb, float *depth,
                                      float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_render_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                             pnr::baked_dense(vol, -1, false, "vol", -1, nullptr),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

extern "C" int pnr_baked_sh_render_rays(const float *rays, long long R, const float *coef, int degree, const uint32_t *bits, int nx,
                                        int ny, int nz, const float *c1, const float *c2, float step, int white_bkgd, float terminate,
                                        float *rgb, float *depth, float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_sh_render_rays", pnr::baked_explicit_rays(rays, R),
                             pnr::baked_dense(coef, degree, false, "coef", 0, pnr::DEGREE_SH),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

extern "C" int pnr_baked_sh_render_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                         float z_far, const float *coef, int degree, const uint32_t *bits, int nx, int ny, int nz,
                                         const float *c1, const float *c2, float step, int white_bkgd, float terminate, float *rgb,
                                         float *depth, float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_sh_render_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                             pnr::baked_dense(coef, degree, false, "coef", 0, pnr::DEGREE_SH),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

extern "C" int pnr_sparse_points_mark(const uint32_t *bits, int nx, int ny, int nz, uint8_t *keep, void *stream) {
    const char *entry = "pnr_sparse_points_mark";
    if (const char *why = pnr::occ_bad_dims(nx, ny, nz)) return pnr::occ_fail(entry, why);
    const long long P = (long long)nx * ny * nz;
    if (P >= (1LL << 31)) return pnr::occ_fail(entry, "the grid must have fewer than 2^31 points (ranks are int32)");
    if (!bits || !keep) return pnr::occ_fail(entry, "null argument");
    if (pnr::baked_misaligned4(bits)) return pnr::occ_fail(entry, "bits must be 4-byte aligned");
    const long long pairs = (P + 1) / 2, blocks = (pairs + pnr::SPARSE_MARK_THREADS - 1) / pnr::SPARSE_MARK_THREADS;
    hipLaunchKernelGGL(pnr::sparse_points_mark_kernel, dim3((unsigned)blocks), dim3(pnr::SPARSE_MARK_THREADS), 0, (hipStream_t)stream, bits,
                       nx, ny, nz, P, keep);
    return pnr_check_launch(entry);
}

extern "C" int pnr_baked_sparse_render_rays(const float *rays, long long R, const float *rows, long long M, int degree,
                                            const int32_t *index, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                            const float *c2, float step, int white_bkgd, float terminate, float *rgb, float *depth,
                                            float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_sparse_render_rays", pnr::baked_explicit_rays(rays, R),
                             pnr::baked_sparse(rows, M, index, degree, false, pnr::DEGREE_SPARSE),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

extern "C" int pnr_baked_sparse_render_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                             float z_near, float z_far, const float *rows, long long M, int degree,
                                             const int32_t *index, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                             const float *c2, float step, int white_bkgd, float terminate, float *rgb, float *depth,
                                             float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_sparse_render_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                             pnr::baked_sparse(rows, M, index, degree, false, pnr::DEGREE_SPARSE),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

// ---- half-precision storage: the entries above on (r,g,b,sigma) kept as four fp16 numbers.  degree -1: the RGBA march

extern "C" int pnr_baked_half_render_rays(const float *rays, long long R, const uint16_t *vol, int degree, const uint32_t *bits, int nx,
                                          int ny, int nz, const float *c1, const float *c2, float step, int white_bkgd,
                                          float terminate, float *rgb, float *depth, float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_half_render_rays", pnr::baked_explicit_rays(rays, R),
                             pnr::baked_dense(vol, degree, true, "vol", -1, pnr::DEGREE_HALF),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

extern "C" int pnr_baked_half_render_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                           float z_near, float z_far, const uint16_t *vol, int degree, const uint32_t *bits, int nx,
                                           int ny, int nz, const float *c1, const float *c2, float step, int white_bkgd,
                                           float terminate, float *rgb, float *depth, float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_half_render_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                             pnr::baked_dense(vol, degree, true, "vol", -1, pnr::DEGREE_HALF),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

extern "C" int pnr_baked_sparse_half_render_rays(const float *rays, long long R, const uint16_t *rows, long long M, int degree,
                                                 const int32_t *index, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                                 const float *c2, float step, int white_bkgd, float terminate, float *rgb,
                                                 float *depth, float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_sparse_half_render_rays", pnr::baked_explicit_rays(rays, R),
                             pnr::baked_sparse(rows, M, index, degree, true, pnr::DEGREE_HALF),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

extern "C" int pnr_baked_sparse_half_render_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                                  float z_near, float z_far, const uint16_t *rows, long long M, int degree,
                                                  const int32_t *index, const uint32_t *bits, int nx, int ny, int nz,
                                                  const float *c1, const float *c2, float step, int white_bkgd, float terminate,
                                                  float *rgb, float *depth, float *alpha, void *stream) {
    return pnr::baked_render("pnr_baked_sparse_half_render_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                             pnr::baked_sparse(rows, M, index, degree, true, pnr::DEGREE_HALF),
                             {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream});
}

// ---- scenes of several posed volumes of one kind (objects: a HOST array)

extern "C" int pnr_baked_scene_render_rays(const float *rays, long long R, const PnrBakedObject *objects, int n_objects, float step,
                                           int white_bkgd, float terminate, float *rgb, float *depth, float *alpha, void *stream) {
    return pnr::baked_scene_render("pnr_baked_scene_render_rays", pnr::baked_explicit_rays(rays, R), objects, n_objects, step, white_bkgd,
                                   terminate, rgb, depth, alpha, stream);
}

extern "C" int pnr_baked_scene_render_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                            float z_far, const PnrBakedObject *objects, int n_objects, float step, int white_bkgd,
                                            float terminate, float *rgb, float *depth, float *alpha, void *stream) {
    return pnr::baked_scene_render("pnr_baked_scene_render_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                                   objects, n_objects, step, white_bkgd, terminate, rgb, depth, alpha, stream);
}

// ---- gradients of the scene march with respect to the world rays and the objects' poses

extern "C" size_t pnr_baked_scene_backward_workspace_bytes(void) {
    return (size_t)pnr::POSE_MAX_BLOCKS * PNR_BAKED_SCENE_MAX_OBJECTS * 12 * sizeof(double);
}

extern "C" int pnr_baked_scene_backward_rays(const float *rays, long long R, const PnrBakedObject *objects, int n_objects, float step,
                                             int white_bkgd, float terminate, const float *d_rgb, const float *d_depth, const float *d_alpha,
                                             float *d_rays, float *d_local, float *d_poses, void *workspace, void *stream) {
    return pnr::baked_scene_backward("pnr_baked_scene_backward_rays", pnr::baked_explicit_rays(rays, R), objects, n_objects, step, white_bkgd,
                                     terminate, d_rgb, d_depth, d_alpha, d_rays, d_local, d_poses, workspace, stream);
}

extern "C" int pnr_baked_scene_backward_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                              float z_far, const PnrBakedObject *objects, int n_objects, float step, int white_bkgd,
                                              float terminate, const float *d_rgb, const float *d_depth, const float *d_alpha, float *d_rays,
                                              float *d_local, float *d_poses, void *workspace, void *stream) {
    return pnr::baked_scene_backward("pnr_baked_scene_backward_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                                     objects, n_objects, step, white_bkgd, terminate, d_rgb, d_depth, d_alpha, d_rays, d_local, d_poses,
                                     workspace, stream);
}

// ---- gradients with respect to the stored values (fp32 storage; index == NULL: a dense volume, M is then not looked at)

extern "C" int pnr_baked_backward_rays(const float *rays, long long R, const float *stored, long long M, int degree, const int32_t *index,
                                       const uint32_t *bits, int nx, int ny, int nz, const float *c1, const float *c2, float step,
                                       int white_bkgd, float terminate, const float *d_rgb, const float *d_depth, const float *d_alpha,
                                       float *d_stored, void *stream) {
    return pnr::baked_backward("pnr_baked_backward_rays", pnr::baked_explicit_rays(rays, R), stored, M, degree, index,
                               {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, nullptr, nullptr, nullptr, stream},
                               {d_rgb, d_depth, d_alpha, d_stored});
}

extern "C" int pnr_baked_backward_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                        float z_far, const float *stored, long long M, int degree, const int32_t *index,
                                        const uint32_t *bits, int nx, int ny, int nz, const float *c1, const float *c2, float step,
                                        int white_bkgd, float terminate, const float *d_rgb, const float *d_depth, const float *d_alpha,
                                        float *d_stored, void *stream) {
    return pnr::baked_backward("pnr_baked_backward_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far), stored,
                               M, degree, index, {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, nullptr, nullptr, nullptr, stream},
                               {d_rgb, d_depth, d_alpha, d_stored});
}

// ---- gradients with respect to the rays (fp32 or fp16 storage; index == NULL: a dense volume, M is then not looked at)

extern "C" int pnr_baked_ray_backward_rays(const float *rays, long long R, const void *stored, int storage_half, long long M, int degree,
                                           const int32_t *index, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                           const float *c2, float step, int white_bkgd, float terminate, const float *d_rgb,
                                           const float *d_depth, const float *d_alpha, float *d_rays, void *stream) {
    return pnr::baked_ray_backward("pnr_baked_ray_backward_rays", pnr::baked_explicit_rays(rays, R), stored, storage_half, M, degree, index,
                                   {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, nullptr, nullptr, nullptr, stream},
                                   {d_rgb, d_depth, d_alpha, d_rays, "d_rays"});
}

extern "C" int pnr_baked_ray_backward_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                            float z_far, const void *stored, int storage_half, long long M, int degree,
                                            const int32_t *index, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                            const float *c2, float step, int white_bkgd, float terminate, const float *d_rgb,
                                            const float *d_depth, const float *d_alpha, float *d_rays, void *stream) {
    return pnr::baked_ray_backward("pnr_baked_ray_backward_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                                   stored, storage_half, M, degree, index,
                                   {bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, nullptr, nullptr, nullptr, stream},
                                   {d_rgb, d_depth, d_alpha, d_rays, "d_rays"});
}

// ---- total variation of the stored values: the value, and its gradient ADDED into `grad` (fp32 storage; index == NULL: dense)

extern "C" size_t pnr_baked_tv_workspace_bytes(void) { return pnr::TV_MAX_BLOCKS * sizeof(double); }

extern "C" int pnr_baked_tv(const float *stored, long long M, int degree, const int32_t *index, const int32_t *ids, int nx, int ny, int nz,
                            const float *w, float eps, const float *scale, float *value32, double *value64, float *grad, void *workspace,
                            void *stream) {
    using namespace pnr;
    const char *entry = "pnr_baked_tv";
    const BakedVolumeDesc v = {stored, degree, false, index != nullptr, index, index ? M : 0, "stored", -1, DEGREE_HALF};
    if (v.degree < v.min_degree || v.degree > 2) return occ_fail(entry, v.degree_rule);
    if ((index != nullptr) != (ids != nullptr)) return occ_fail(entry, "index and ids go together (both, or neither for a dense volume)");
    if (v.sparse && v.M < 0) return occ_fail(entry, "bad sizes (M)");
    if (const char *why = occ_bad_dims(nx, ny, nz)) return occ_fail(entry, why);
    const long long P = (long long)nx * ny * nz;
    if (v.sparse && P >= (1LL << 31)) return occ_fail(entry, "the grid must have fewer than 2^31 points (ranks are int32)");
    if (!(eps > 0.f) || !std::isfinite(eps)) return occ_fail(entry, "eps must be finite and > 0");
    if (!w) return occ_fail(entry, "null argument (w)");
    const int B = v.degree < 0 ? 1 : (v.degree + 1) * (v.degree + 1);
    const long long rows = v.sparse ? v.M : P;
    TvWeights wt = {};
    for (int e = 0; e < 4 * B; ++e) {
        if (!(w[e] >= 0.f) || !std::isfinite(w[e])) return occ_fail(entry, "every weight must be finite and >= 0");
        wt.w[e] = w[e];
        wt.wn[e] = rows > 0 ? (float)((double)w[e] / (double)rows) : 0.f;
    }
    const bool want_value = value32 || value64;
    if (!want_value && !grad) return PNR_OK;
    if (want_value && !workspace) return occ_fail(entry, "a value needs the workspace of pnr_baked_tv_workspace_bytes()");
    if (rows > 0 && !v.stored) return occ_fail(entry, "null argument");
    if (occ_misaligned16(v.stored) || occ_misaligned16(grad)) return occ_fail(entry, "stored and grad must be 16-byte aligned");
    if (baked_misaligned4(index) || baked_misaligned4(ids) || baked_misaligned4(scale) || baked_misaligned4(value32) ||
        baked_misaligned8(value64) || baked_misaligned8(workspace))
        return occ_fail(entry, "index, ids, scale and value32 must be 4-byte aligned, value64 and workspace 8-byte aligned");
    const long long threads = rows * B;
    const int blocks = (int)((threads + TV_THREADS - 1) / TV_THREADS < TV_MAX_BLOCKS ? (threads + TV_THREADS - 1) / TV_THREADS : TV_MAX_BLOCKS);
    double *partials = want_value ? static_cast<double *>(workspace) : nullptr;
    if (blocks > 0) {
        const TvParams q = {nx, ny, nz, P, rows, index, ids, eps, scale};
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(TV_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(v.stored),
                               reinterpret_cast<float4 *>(grad), q, wt, partials);
        };
        // B, layout, and whether a gradient is asked for, each decided once: 3 x 2 x 2 instantiations
        const auto by_grad = [&](auto b, auto sparse) {
            constexpr int NB = decltype(b)::value;
            constexpr bool SP = decltype(sparse)::value;
            if (grad) launch(baked_tv_kernel<NB, SP, true>);
            else launch(baked_tv_kernel<NB, SP, false>);
        };
        const auto by_layout = [&](auto b) {
            if (v.sparse) by_grad(b, std::true_type{});
            else by_grad(b, std::false_type{});
        };
        if (B == 1) by_layout(std::integral_constant<int, 1>{});
        else if (B == 4) by_layout(std::integral_constant<int, 4>{});
        else by_layout(std::integral_constant<int, 9>{});
        if (const int rc = pnr_check_launch(entry)) return rc;
    }
    if (want_value) {
        hipLaunchKernelGGL(baked_tv_final_kernel, dim3(1), dim3(TV_THREADS), 0, (hipStream_t)stream, partials, blocks, (double)rows, value32,
                           value64);
        return pnr_check_launch(entry);
    }
    return PNR_OK;
}
