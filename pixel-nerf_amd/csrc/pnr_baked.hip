// pnr_baked.hip -- ray marching through a baked RGBA volume for gfx950 (inference).  The network of an encoded object is evaluated
// ONCE on the points of its grid (util.bake.BakedVolume.from_model: rgb and sigma at the points of pnr_gen_grid_points); any number
// of views is then rendered from the grid alone: equidistant samples along the ray, a trilinear blend of the cell's eight corners,
// the compositing of src/render/nerf.py:178-182,223-249 with a constant delta.  No network behind a pixel; the image is an
// approximation of the network's render (trilinear in space, one view direction per grid point, no importance sampling).
// Semantics: include/pixelnerf_hip.h ("baked volumes").  One wavefront per ray, composite_kernel's scan; no atomics, no LDS, no
// workspace: the same bytes on every call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

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
    const float4 *vol;     // (nx,ny,nz) x (r,g,b,sigma)
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

__global__ void __launch_bounds__(BAKED_WAVES * 64)
baked_march_kernel(const RaySrc rs, long long R, const BakedParams q, float *__restrict__ rgb, float *__restrict__ depth,
                   float *__restrict__ alpha_out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * BAKED_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;  // the idle waves of the last workgroup (nothing below synchronises across waves)
    const Ray8 ray = load_ray(rs, r);
    const float o[3] = {ray.ox, ray.oy, ray.oz}, d[3] = {ray.dx, ray.dy, ray.dz};
    // the number of samples; a ray that cannot be sampled (near >= far, a non-finite component, more than 2^20 samples) keeps
    // n = 0, reads nothing and gets the background
    bool ok = occ_finite(ray.near) && occ_finite(ray.far) && ray.near < ray.far;
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && occ_finite(o[a]) && occ_finite(d[a]);
    const float count = ceilf((ray.far - ray.near) / q.step);
    const int n = ok && count <= BAKED_MAX_SAMPLES ? (int)count : 0;  // (a NaN count compares false)

    const long long sy = q.g.n[2], sx = (long long)q.g.n[1] * q.g.n[2];  // point strides in float4s; z is the fastest axis
    const long long cy = q.g.n[2] - 1, cx = (long long)(q.g.n[1] - 1) * (q.g.n[2] - 1);  // cell strides of the bitfield
    float carry = 1.f;  // transmittance in front of this chunk: prod_{j < c0} (1 - a_j + 1e-10)
    float acc_r = 0.f, acc_g = 0.f, acc_b = 0.f, acc_d = 0.f, acc_w = 0.f;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        const float t = ray.near + ((float)i + 0.5f) * q.step;
        bool active = i < n;
        int idx[3];
        float f[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float p = o[a] + t * d[a];                    // ray_point's operations (pnr_geom.h)
            active = active && p >= q.g.c1[a] && p <= q.g.c2[a];  // (a NaN or infinite coordinate is outside)
            const float u = (p - q.g.c1[a]) / q.g.h[a];
            const float c = fminf(fmaxf(floorf(u), 0.f), (float)(q.g.n[a] - 2));  // (fmaxf drops a NaN: always a cell of the grid)
            idx[a] = (int)c;
            f[a] = fminf(fmaxf(u - c, 0.f), 1.f);
        }
        if (q.bits) {
            const long long cell = idx[0] * cx + idx[1] * cy + idx[2];
            active = active && (q.bits[cell >> 5] >> (cell & 31) & 1u);
        }
        if (__ballot(active) == 0ull) continue;  // every factor of the chunk is exactly 1: the carry and the sums stay as they are
        float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active) {
            const float4 *c000 = q.vol + (idx[0] * sx + idx[1] * sy + idx[2]);
            const float4 v000 = c000[0], v001 = c000[1], v010 = c000[sy], v011 = c000[sy + 1];
            const float4 v100 = c000[sx], v101 = c000[sx + 1], v110 = c000[sx + sy], v111 = c000[sx + sy + 1];
            // along z, then y, then x
            const float4 v00 = baked_lerp(v000, v001, f[2]), v01 = baked_lerp(v010, v011, f[2]);
            const float4 v10 = baked_lerp(v100, v101, f[2]), v11 = baked_lerp(v110, v111, f[2]);
            cs = baked_lerp(baked_lerp(v00, v01, f[1]), baked_lerp(v10, v11, f[1]), f[0]);
        }
        const float a_i = 1.f - expf(-(q.step * cs.w));  // nerf.py:228 with delta = step; exactly 0 for sigma == 0
        const float tfac = 1.f - a_i + 1e-10f;           // :230-232; exactly 1 for a_i == 0
        const float incl = wave_scan_mul(tfac, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.f;
        const float w = a_i * (carry * excl);  // :234-236
        acc_r += w * cs.x; acc_g += w * cs.y; acc_b += w * cs.z;
        acc_d += w * t;
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
#pragma clang fp contract(fast)

static bool baked_misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// the checks both entries share, then the launch; src holds the rays or the camera, already checked
static int baked_launch(const char *entry, const RaySrc &src, long long R, const float *vol, const uint32_t *bits, int nx, int ny, int nz,
                        const float *c1, const float *c2, float step, int white_bkgd, float terminate, float *rgb, float *depth,
                        float *alpha, void *stream) {
    if (const char *why = occ_bad_dims(nx, ny, nz)) return occ_fail(entry, why);
    BakedParams q;
    if (const char *why = occ_grid(nx, ny, nz, c1, c2, q.g)) return occ_fail(entry, why);
    if (!(step > 0.f) || !std::isfinite(step)) return occ_fail(entry, "step must be finite and > 0");
    if (!(terminate >= 0.f && terminate < 1.f)) return occ_fail(entry, "terminate must lie in [0, 1)");  // (refuses a NaN)
    if (R == 0) return PNR_OK;
    if (!vol || !rgb || !depth || !alpha) return occ_fail(entry, "null argument");
    if (occ_misaligned16(vol)) return occ_fail(entry, "vol must be 16-byte aligned");
    if (baked_misaligned4(bits) || baked_misaligned4(rgb) || baked_misaligned4(depth) || baked_misaligned4(alpha))
        return occ_fail(entry, "bits, rgb, depth and alpha must be 4-byte aligned");
    const long long blocks = (R + BAKED_WAVES - 1) / BAKED_WAVES;
    if (blocks > 0x7fffffffLL) return occ_fail(entry, "the number of rays exceeds the launch limit");
    q.vol = reinterpret_cast<const float4 *>(vol);
    q.bits = bits;
    q.step = step;
    q.eps = terminate;
    q.white_bkgd = white_bkgd;
    hipLaunchKernelGGL(baked_march_kernel, dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0, (hipStream_t)stream, src, R, q, rgb, depth,
                       alpha);
    return pnr_check_launch(entry);
}

}  // namespace pnr

extern "C" int pnr_baked_render_rays(const float *rays, long long R, const float *vol, const uint32_t *bits, int nx, int ny, int nz,
                                     const float *c1, const float *c2, float step, int white_bkgd, float terminate, float *rgb,
                                     float *depth, float *alpha, void *stream) {
    const char *entry = "pnr_baked_render_rays";
    if (R < 0) return pnr::occ_fail(entry, "bad sizes (R)");
    if (R > 0 && !rays) return pnr::occ_fail(entry, "null argument");
    if (pnr::baked_misaligned4(rays)) return pnr::occ_fail(entry, "rays must be 4-byte aligned");
    pnr::RaySrc src = {};
    src.rays = rays;
    return pnr::baked_launch(entry, src, R, vol, bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth, alpha, stream);
}

extern "C" int pnr_baked_render_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                      float z_far, const float *vol, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                      const float *c2, float step, int white_bkgd, float terminate, float *rgb, float *depth,
                                      float *alpha, void *stream) {
    const char *entry = "pnr_baked_render_views";
    if (NV < 0 || W <= 0 || H <= 0) return pnr::occ_fail(entry, "bad sizes (NV, W, H)");
    if (NV > 0 && !poses) return pnr::occ_fail(entry, "null argument");
    if (pnr::baked_misaligned4(poses)) return pnr::occ_fail(entry, "poses must be 4-byte aligned");
    pnr::RaySrc src = {};
    src.poses = poses;
    src.W = W; src.H = H;
    src.fx = fx; src.fy = fy; src.cx = cx; src.cy = cy;
    src.z_near = z_near; src.z_far = z_far;
    return pnr::baked_launch(entry, src, (long long)NV * W * H, vol, bits, nx, ny, nz, c1, c2, step, white_bkgd, terminate, rgb, depth,
                             alpha, stream);
}
