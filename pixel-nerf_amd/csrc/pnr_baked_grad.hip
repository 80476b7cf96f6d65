// pnr_baked_grad.hip -- backward of the baked-volume march for gfx950: with respect to the stored values (pnr_baked_backward_rays
// / _views: what fitting a volume needs) and with respect to the rays (pnr_baked_ray_backward_rays / _views: what registering a
// camera needs).  Semantics: include/pixelnerf_hip.h.  The samples are the forward's: the per-sample device functions of
// pnr_baked.h, which baked_march calls too.  The stored-value backward is the ONE path of the family with atomics (fp32 atomicAdd
// into the caller's zeroed buffer): not bit-reproducible from run to run; fp32 storage only.  The ray backward takes every storage
// and layout (the forward's 16 instantiations), has no atomics and writes every row.
#include "pnr_baked_grad.h"

namespace pnr {

#pragma clang fp contract(off)  // every product, sum and quotient below is rounded on its own: the header states them so

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
#pragma clang fp contract(fast)

// The backward entries: fp32 storage, dense (index == NULL) or sparse rows, degree -1..2: 2 x 4 instantiations.
static int baked_backward(const char *entry, const BakedRays &rays, const void *stored, long long M, int degree, const int32_t *index,
                          const BakedMarchArgs &a, const BakedGrads &grads) {
    const BakedVolumeDesc v = baked_stored(stored, 0, M, degree, index);
    BakedParams q;
    long long blocks;
    if (const int rc = baked_check(entry, rays, v, a, &grads, q, blocks)) return rc;
    if (blocks == 0) return PNR_OK;
    baked_dispatch(v, [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        if constexpr (std::is_same<typename Corner::stored_t, float4>::value)  // (no fp16 instantiation: v is never half)
            hipLaunchKernelGGL((baked_march_bwd_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                               (hipStream_t)a.stream, rays.src, rays.R, q, rows, static_cast<const float4 *>(v.stored), grads.d_rgb,
                               grads.d_depth, grads.d_alpha, grads.out);
    });
    return pnr_check_launch(entry);
}

// The ray-gradient entries: fp32 or fp16 storage, dense (index == NULL) or sparse rows, degree -1..2: the forward's 16 instantiations.
static int baked_ray_backward(const char *entry, const BakedRays &rays, const void *stored, int storage_half, long long M, int degree,
                              const int32_t *index, const BakedMarchArgs &a, const BakedGrads &grads) {
    const BakedVolumeDesc v = baked_stored(stored, storage_half, M, degree, index);
    BakedParams q;
    long long blocks;
    if (const int rc = baked_check(entry, rays, v, a, &grads, q, blocks)) return rc;
    if (blocks == 0) return PNR_OK;
    baked_dispatch(v, [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        hipLaunchKernelGGL((baked_march_ray_bwd_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                           (hipStream_t)a.stream, rays.src, rays.R, q, rows, static_cast<const typename Corner::stored_t *>(v.stored),
                           grads.d_rgb, grads.d_depth, grads.d_alpha, grads.out);
    });
    return pnr_check_launch(entry);
}

}  // namespace pnr

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
