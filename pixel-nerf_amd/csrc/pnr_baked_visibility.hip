// pnr_baked_visibility.hip -- which grid points the rays of a march SEE, for gfx950 (pnr_baked_visibility_rays / _views;
// include/pixelnerf_hip.h, "Visibility of a baked volume"): per stored row the largest compositing weight any sample of any ray
// gave it, vis[row] = max over samples i and corners c of w_i omega_c.  The pruning criterion of a fitted volume, and the picture of
// what a set of views constrains.  The samples are the forward's: the per-sample device functions of pnr_baked.h and baked_march's
// product scan and carry, so w_i is the forward's weight bit for bit and the walk stops after the chunk the forward stops after.
// One wavefront per ray as the forward; the pass only READS the volume.  No scratch, no LDS, no workspace.
// The one write is an unsigned-integer atomic max on the bit pattern of the float (a vector atomic): every proposal is a positive
// finite float, and on those the order of the bit patterns is the order of the values.  Maximum is commutative and associative
// EXACTLY, so -- unlike the stored backward's fp32 atomicAdd -- the result has equal bytes on every call, for any order of the rays
// and for any split of them into accumulating calls.
// Out of scope: scenes (BakedScene gets no visibility).
#include "pnr_baked.h"

namespace pnr {

#pragma clang fp contract(off)  // every product, sum and quotient below is rounded on its own: the header states them so

// vis[row] = max(vis[row], v) for v > 0 (a zero, a negative number and a NaN are dropped: `v > 0` is false for each).
// The plain load in front of the atomic only FILTERS: a proposal that cannot raise the value it reads is skipped.  The value only
// ever grows, so a stale read -- the L1 is not coherent with other CUs' atomics, which are performed in the L2 -- is a value
// that is too SMALL: it can let a needless atomic through, it can never drop a maximum.  That is why the filter is safe here.
// Measured against the bare atomic (profiles/baked_notes.md, "Coarse to fine"): 0.6 - 0.7 x its time on dense RGBA volumes, level at
// degree 2, 0.1 - 0.5 x on every repeated pass, 1.2 - 1.5 x on the first pass over small sparse volumes.  Kept; a variant build
// with PNR_VIS_NO_FILTER has the bare form.
__device__ __forceinline__ void baked_vis_propose(uint32_t *vis, long long row, float v) {
    if (!(v > 0.f)) return;
    const uint32_t b = __float_as_uint(v);
#if !(defined(PNR_VARIANT) && defined(PNR_VIS_NO_FILTER))
    if (b <= vis[row]) return;
#endif
    atomicMax(vis + row, b);
}

template <class Corner, class Rows>
__global__ void __launch_bounds__(BAKED_WAVES * 64)
baked_visibility_kernel(const RaySrc rs, long long R, const BakedParams q, const Rows rows, const typename Corner::stored_t *__restrict__ stored,
                        uint32_t *vis) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * BAKED_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;  // the idle waves of the last workgroup (nothing below synchronises across waves)
    Corner corner;
    corner.data = stored;
    const Ray8 ray = load_ray(rs, r);
    corner.set_ray(ray);
    const int n = baked_sample_count(ray, q.step);
    float carry = 1.f;  // transmittance in front of this chunk, as baked_march carries it
    for (int c0 = 0; c0 < n; c0 += 64) {
        const BakedSample s = baked_sample(ray, q, c0 + lane, n);
        if (__ballot(s.active) == 0ull) continue;  // every factor of the chunk is exactly 1 and every weight 0
        BakedCell<Rows> cell;
        bool found;
        const float4 cs = baked_value(q, corner, rows, s, cell, found);
        const BakedAlpha al = baked_alpha(q.step, cs.w);
        const float incl = wave_scan_mul(al.tfac, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.f;
        const float w = al.a * (carry * excl);  // baked_march's w_i, by its operations
        carry = carry * __shfl(incl, 63, 64);
        if (found) {  // (no wave operation below: the lanes part here and meet again at the stop test)
            // the corner weights of baked_march_bwd_kernel, formed in its order: (x part * y part) * z part
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {  // pair j = 2 ix + iy
                const long long row = cell.row(rows, j);
                const float wxy = (j >> 1 ? s.f[0] : 1.f - s.f[0]) * (j & 1 ? s.f[1] : 1.f - s.f[1]);
#pragma unroll
                for (int iz = 0; iz < 2; ++iz) {
                    const float wt = wxy * (iz ? s.f[2] : 1.f - s.f[2]);
                    baked_vis_propose(vis, row + iz, w * wt);
                }
            }
        }
        if (q.eps > 0.f && carry <= q.eps) break;  // the forward's break, in its words (wave-uniform)
    }
}
#pragma clang fp contract(fast)

// The visibility entries: fp32 or fp16 storage, dense (index == NULL) or sparse rows, degree -1..2: the forward's 16 instantiations.
// The checks are pnr_baked_ray_backward_*'s, vis in the place of d_rays and no upstream gradients.
static int baked_visibility(const char *entry, const BakedRays &rays, const void *stored, int storage_half, long long M, int degree,
                            const int32_t *index, const BakedMarchArgs &a, float *vis) {
    const BakedVolumeDesc v = baked_stored(stored, storage_half, M, degree, index);
    const BakedGrads grads = {nullptr, nullptr, nullptr, vis, "vis"};
    BakedParams q;
    long long blocks;
    if (const int rc = baked_check(entry, rays, v, a, &grads, q, blocks)) return rc;
    if (blocks == 0) return PNR_OK;
    baked_dispatch(v, [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        hipLaunchKernelGGL((baked_visibility_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                           (hipStream_t)a.stream, rays.src, rays.R, q, rows, static_cast<const typename Corner::stored_t *>(v.stored),
                           reinterpret_cast<uint32_t *>(vis));
    });
    return pnr_check_launch(entry);
}

}  // namespace pnr

extern "C" int pnr_baked_visibility_rays(const float *rays, long long R, const void *stored, int storage_half, long long M, int degree,
                                         const int32_t *index, const uint32_t *bits, int nx, int ny, int nz, const float *c1,
                                         const float *c2, float step, float terminate, float *vis, void *stream) {
    return pnr::baked_visibility("pnr_baked_visibility_rays", pnr::baked_explicit_rays(rays, R), stored, storage_half, M, degree, index,
                                 {bits, nx, ny, nz, c1, c2, step, 0, terminate, nullptr, nullptr, nullptr, stream}, vis);
}

extern "C" int pnr_baked_visibility_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy, float z_near,
                                          float z_far, const void *stored, int storage_half, long long M, int degree, const int32_t *index,
                                          const uint32_t *bits, int nx, int ny, int nz, const float *c1, const float *c2, float step,
                                          float terminate, float *vis, void *stream) {
    return pnr::baked_visibility("pnr_baked_visibility_views", pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far),
                                 stored, storage_half, M, degree, index,
                                 {bits, nx, ny, nz, c1, c2, step, 0, terminate, nullptr, nullptr, nullptr, stream}, vis);
}
