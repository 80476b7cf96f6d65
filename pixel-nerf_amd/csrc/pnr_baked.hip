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
// This file: the forward kernel, its ten entries and pnr_sparse_points_mark.  What every march shares, device and host, and the
// structure of the family: pnr_baked.h.  The backward kernels (dL/d stored, dL/d rays): pnr_baked_grad.hip.  Scenes of several posed
// volumes and their gradients: pnr_baked_scene.hip.  The total-variation prior: pnr_baked_tv.hip.  What the rays see:
// pnr_baked_visibility.hip.  A volume on another grid: pnr_baked_resample.hip.
#include "pnr_baked.h"

namespace pnr {

#pragma clang fp contract(off)  // every product, sum and quotient below is rounded on its own: the header states them so

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
        // The compositing of a chunk and the pixel write below stand a second time in baked_scene_march_kernel (pnr_baked_scene.hip).
        // As one device function for both, a scene kernel took 2 more VGPRs and lost a wave per SIMD, and no forward kernel kept its
        // instructions (profiles/baked_notes.md, "A file per concern").  Keep the two texts the same.
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
#pragma clang fp contract(fast)

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

// the forward entries: the checks, then the launch
static int baked_render(const char *entry, const BakedRays &rays, const BakedVolumeDesc &v, const BakedMarchArgs &a) {
    BakedParams q;
    long long blocks;
    if (const int rc = baked_check(entry, rays, v, a, nullptr, q, blocks)) return rc;
    if (blocks == 0) return PNR_OK;
    baked_dispatch(v, [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        hipLaunchKernelGGL((baked_march_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                           (hipStream_t)a.stream, rays.src, rays.R, q, rows, static_cast<const typename Corner::stored_t *>(v.stored), a.rgb,
                           a.depth, a.alpha);
    });
    return pnr_check_launch(entry);
}

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
