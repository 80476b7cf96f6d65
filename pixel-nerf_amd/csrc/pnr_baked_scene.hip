// pnr_baked_scene.hip -- scenes of several posed baked volumes for gfx950 (include/pixelnerf_hip.h, "Scenes of several baked
// volumes" and "Gradients of the scene march"): up to 8 posed volumes of one kind in one image.
// Forward (pnr_baked_scene_render_rays / _views): baked_scene_march_kernel, the single march (pnr_baked.hip) with an inner loop over
// the objects: the samples are the WORLD ray's, every object sees the ray in its own frame, and the values of the objects that
// contribute to a sample are mixed before alpha and the scan.  The per-sample work is the device functions of the single march
// (pnr_baked.h) and the compositing is its text, so one object at the identity renders that march's bytes.  The same 16
// instantiations.
// Backward (pnr_baked_scene_backward_rays / _views: dL/d world rays and dL/d object poses, what placing an object needs):
// baked_scene_ray_bwd_kernel, the ray backward's walk (pnr_baked_grad.hip) on the scene's mixture with the device functions of
// pnr_baked_grad.h, and two small kernels that reduce the poses' gradient over the rays in a fixed order; no atomics, no LDS.
// The walk itself (upstream gradient, first walk, scan step, row write) is baked_march_ray_bwd_kernel's, written out here as
// there: shared, it cost this kernel 3 to 10 % (profiles/baked_notes.md, "A file per concern").
// Stored backward (pnr_baked_scene_stored_backward_rays / _views: dL/d every object's stored values, what fitting a scene needs):
// baked_scene_stored_bwd_kernel, the same walk on the mixture, then baked_march_bwd_kernel's corner weights and Corner::scatter
// per contributing object; fp32 storage only, fp32 atomics into the caller's buffers, not bit-reproducible from run to run.
// The six entries share one checking function, baked_scene_check.
#include "pnr_baked_grad.h"

namespace pnr {

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

#pragma clang fp contract(off)  // every product, sum and quotient below is rounded on its own: the header states them so

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
// the sample contributes (active, and its rows found); `active`: baked_sample's.  The basis of a coefficient volume is evaluated
// only for a chunk that reads.  The same steps stand a second time in baked_scene_ray_bwd_kernel's object loop, with the partials of
// the blend where this takes the value: as one function for both (ray, settings and sample handed back by reference) the 16
// forward kernels took 2 to 22 more VGPRs and seven of them lost a wave per SIMD (profiles/baked_notes.md, "A file per concern").
template <class Corner, class Rows>
__device__ __forceinline__ bool baked_scene_value(const BakedSceneObject &ob, const Ray8 &world, float step, int i, int n, bool &active,
                                                  float4 &cs) {
    const Ray8 ray = baked_scene_ray(world, ob);
    active = false;
    cs = make_float4(0.f, 0.f, 0.f, 0.f);
    const float t = ray.near + ((float)i + 0.5f) * step;
    const float o[3] = {ray.ox, ray.oy, ray.oz}, d[3] = {ray.dx, ray.dy, ray.dz};
    bool inside = i < n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = o[a] + t * d[a];
        inside = inside && p >= ob.g.c1[a] && p <= ob.g.c2[a];
    }
    // baked_sample's inside test alone, first -- the same operations on the same numbers, so exactly its answer -- and nothing
    // more for a chunk that does not touch the object's box: most (chunk, object) pairs of a scene end here, before the divisions
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

// first pass of the mixing at sample i: sigma = sum sigma_j over the objects that contribute, in list order, the first
// contributor's value, their number -> whether any object is active at the sample
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

// second pass: c = sum (sigma_j / sigma) c_j.  One contributor (all but the samples where boxes overlap): the kept value.  More: the
// weights need the finished sum, so those lanes walk the objects again -- the same loads, the same values -- instead of keeping
// eight float4s per lane.
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
        // baked_scene_sigma and baked_scene_colour IN PLACE (the backward calls them), then baked_march's compositing and pixel write
        // IN PLACE: as calls the 16 kernels moved by -46 .. +39 instructions and three lost a wave per SIMD; with the compositing
        // shared, one did (profiles/baked_notes.md, "A file per concern").  Keep each pair of texts the same.
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

// ---- backward of the SCENE march with respect to the world rays and the objects' poses (pnr_baked_scene_backward_*).
// baked_march_ray_bwd_kernel's walk on the mixture (c, sigma) of baked_scene_march_kernel: the first walk, the fp64 heads, the
// reverse affine scan and the rebuild beyond 4096 samples are that kernel's (pnr_baked_grad.h), with the mixed sigma where it has
// the blended one.  What a sample sends back goes through the mixing to every object
// that contributes, through that object's blend in ITS frame -- dp'_ij, on the ray (o', d') of baked_scene_ray -- and back to the
// world through R_j.  The world row keeps the single kernel's per-lane fp64 sums, so one object at [I | 0] gives its bytes; the
// six numbers of an object (dL/do', dL/dd') are summed per chunk by wave_sum and added into the ONE lane that owns accumulator
// (j, k): a pair of registers for all eight objects.  The basis sums of a coefficient volume stay per lane and per object (fp32,
// the single kernel's order: they reach d_rays through a rotation alone and must give its bytes).  No atomics, no LDS.

// v rotated into the world by object-to-world R: each component (R_a0 x + R_a1 y) + R_a2 z
__device__ __forceinline__ void baked_scene_rotate(const BakedSceneObject &ob, float x, float y, float z, float (&out)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = (ob.rot[3 * a] * x + ob.rot[3 * a + 1] * y) + ob.rot[3 * a + 2] * z;
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

// ---- backward of the SCENE march with respect to every object's STORED VALUES (pnr_baked_scene_stored_backward_*; fp32 storage
// only): what fitting the contents of a scene to images of the scene needs.  The walk is baked_scene_ray_bwd_kernel's on the
// mixture -- the first walk with the fp64 heads and the forward's own fp32 factors for the stop chunk, the reverse affine scan in
// fp64, the rebuild beyond 4096 samples -- and gives dL/dc_i = w_i d_rgb and dL/dsigma_i of the mixture.  Through the mixing to every
// contributing object j (that kernel's convention: where sigma is not > 0 the colour is the constant 0), then through the object's
// blend in ITS frame as baked_march_bwd_kernel does: corner (ix,iy,iz) gets the product of f or 1 - f per axis, and
// Corner::scatter adds it into d_stored[j] with fp32 atomics.  A NULL d_stored[j] is a frozen object: it mixes and attenuates (the
// mixture above is formed over ALL objects) and the loop below passes it over, on a scalar test.  No workspace, no LDS.

// the buffers dL/d stored_j is added into, by value next to the scene; NULL: object j is frozen
struct BakedSceneStoredGrads {
    float *p[PNR_BAKED_SCENE_MAX_OBJECTS];
};

template <class Corner, class Rows>
__global__ void __launch_bounds__(BAKED_WAVES * 64)
baked_scene_stored_bwd_kernel(const RaySrc rs, long long R, const BakedSceneDesc sc, const BakedSceneStoredGrads out, float step, float eps,
                              int white_bkgd, const float *__restrict__ d_rgb, const float *__restrict__ d_depth,
                              const float *__restrict__ d_alpha) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * BAKED_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;
    float3 drgb = make_float3(0.f, 0.f, 0.f);
    if (d_rgb) drgb = make_float3(d_rgb[r * 3], d_rgb[r * 3 + 1], d_rgb[r * 3 + 2]);
    const float ddepth = d_depth ? d_depth[r] : 0.f, dalpha = d_alpha ? d_alpha[r] : 0.f;
    if (drgb.x == 0.f && drgb.y == 0.f && drgb.z == 0.f && ddepth == 0.f && dalpha == 0.f) return;  // nothing to send back
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

    double S_in = 0.0;  // S of the chunk's last sample
    for (int c = nc - 1; c >= 0; --c) {
        const int i = c * 64 + lane;
        const float t = ray.near + ((float)i + 0.5f) * step;  // baked_sample's depth
        float4 first;
        float sigma;
        int cnt;
        const bool any = baked_scene_sigma<Corner, Rows>(sc, ray, step, i, n, first, sigma, cnt);
        if (__ballot(any) == 0ull) continue;  // 64 identity maps: S stays, nothing to scatter
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
#pragma unroll 1
        for (int j = 0; j < sc.n; ++j) {
            float *__restrict__ dst = out.p[j];
            if (!dst) continue;  // a frozen object (j is wave-uniform: a scalar test)
            const BakedSceneObject &ob = sc.obj[j];
            // baked_scene_value's steps, keeping the cell for the scatter
            const Ray8 oray = baked_scene_ray(ray, ob);
            BakedParams q;
            q.bits = ob.bits;
            q.g = ob.g;
            q.step = step;
            q.eps = 0.f;
            q.white_bkgd = 0;
            const BakedSample s = baked_sample(oray, q, i, n);
            if (__ballot(s.active) == 0ull) continue;  // nothing of this object in the chunk: no loads
            Corner corner;
            corner.data = static_cast<const typename Corner::stored_t *>(ob.stored);
            corner.set_ray(oray);
            const Rows rows = baked_scene_rows<Rows>(ob);
            BakedCell<Rows> cell;
            bool found;
            const float4 cs = baked_value(q, corner, rows, s, cell, found);
            if (found) {  // (no wave operation below; found implies mixed)
                // through the mixing; where sigma is not > 0 the forward's colour is the constant 0
                float wj = 0.f, dsj = dsig;
                if (sigma > 0.f) {
                    wj = cs.w / sigma;
                    dsj = dsig + ((cs.x - col.x) * dc.x + (cs.y - col.y) * dc.y + (cs.z - col.z) * dc.z) / sigma;
                }
                const float4 dcs = make_float4(wj * dc.x, wj * dc.y, wj * dc.z, dsj);
#pragma unroll 1
                for (int pj = 0; pj < 4; ++pj) {  // pair pj = 2 ix + iy
                    const long long row = cell.row(rows, pj);
                    const float wxy = (pj >> 1 ? s.f[0] : 1.f - s.f[0]) * (pj & 1 ? s.f[1] : 1.f - s.f[1]);
#pragma unroll
                    for (int iz = 0; iz < 2; ++iz) {
                        const float wt = wxy * (iz ? s.f[2] : 1.f - s.f[2]);
                        if (wt != 0.f) corner.scatter(dst, row + iz, make_float4(wt * dcs.x, wt * dcs.y, wt * dcs.z, wt * dcs.w));
                    }
                }
            }
        }
    }
}
#pragma clang fp contract(fast)

// ---- host only from here

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

// what a scene entry writes.  Forward (grads == NULL): rgb, depth, alpha.  Backward: grads holds the upstream gradients and d_rays
// (grads->out); d_local; and d_poses (nullable), which needs the workspace.
struct BakedSceneOut {
    float *rgb, *depth, *alpha;
    const BakedGrads *grads;
    float *d_local, *d_poses;
    void *workspace;
    float *const *d_stored = nullptr;  // the stored backward alone (stored_grads): the HOST array of n_objects device pointers
    bool stored_grads = false;
};

// Every check of the six scene entries, in one order: what concerns the call as a whole, then every object through baked_check
// under "entry: object j".  -> PNR_OK with the scene as the kernels take it, the kind in v0 and `blocks` workgroups (0: no rays)
static int baked_scene_check(const char *entry, const BakedRays &rays, const PnrBakedObject *objects, int n_objects, float step,
                             int white_bkgd, float terminate, const BakedSceneOut &o, void *stream, BakedSceneDesc &sc, BakedVolumeDesc &v0,
                             long long &blocks) {
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
    if (o.stored_grads && objects[0].storage_half != 0)
        return occ_fail(entry, "gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards");
    if (rays.defect) return occ_fail(entry, rays.defect);
    if (!(step > 0.f) || !std::isfinite(step)) return occ_fail(entry, "step must be finite and > 0");
    if (!(terminate >= 0.f && terminate < 1.f)) return occ_fail(entry, "terminate must lie in [0, 1)");
    if (o.stored_grads) {
        if (rays.R > 0 && !o.d_stored) return occ_fail(entry, "null argument (d_stored)");
        bool bad = baked_misaligned4(o.grads->d_rgb) || baked_misaligned4(o.grads->d_depth) || baked_misaligned4(o.grads->d_alpha);
        for (int j = 0; o.d_stored && j < n_objects; ++j) bad = bad || baked_misaligned4(o.d_stored[j]);
        if (bad) return occ_fail(entry, "d_rgb, d_depth, d_alpha and every d_stored[j] must be 4-byte aligned");
    } else if (rays.R > 0 && (o.grads ? !o.grads->out || !o.d_local : !o.rgb || !o.depth || !o.alpha)) {
        return occ_fail(entry, "null argument");
    } else if (o.grads) {  // (a misaligned d_poses is wrong whatever R: it is written at R = 0 too)
        if (baked_misaligned4(o.grads->d_rgb) || baked_misaligned4(o.grads->d_depth) || baked_misaligned4(o.grads->d_alpha) ||
            baked_misaligned4(o.grads->out) || baked_misaligned4(o.d_local) || baked_misaligned4(o.d_poses))
            return occ_fail(entry, "d_rgb, d_depth, d_alpha, d_rays, d_local and d_poses must be 4-byte aligned");
        if (o.d_poses && (!o.workspace || baked_misaligned8(o.workspace)))
            return occ_fail(entry, "d_poses needs the workspace of pnr_baked_scene_backward_workspace_bytes(), 8-byte aligned");
    } else if (rays.R > 0 && (baked_misaligned4(o.rgb) || baked_misaligned4(o.depth) || baked_misaligned4(o.alpha))) {
        return occ_fail(entry, "rgb, depth and alpha must be 4-byte aligned");
    }
    sc = {};
    sc.n = n_objects;
    v0 = {};
    for (int j = 0; j < n_objects; ++j) {
        const PnrBakedObject &ob = objects[j];
        std::snprintf(where, sizeof(where), "%s: object %d", entry, j);
        const BakedVolumeDesc v = baked_stored(ob.stored, ob.storage_half, ob.M, ob.degree, ob.index);
        BakedParams q;
        BakedGrads og;
        if (o.grads) og = *o.grads;
        if (o.stored_grads) {  // this object's own buffer; NULL: frozen
            og.out = o.d_stored ? o.d_stored[j] : nullptr;
            og.out_nullable = true;
        }
        if (const int rc = baked_check(where, rays, v, {ob.bits, ob.nx, ob.ny, ob.nz, ob.c1, ob.c2, step, white_bkgd, terminate, o.rgb,
                                                        o.depth, o.alpha, stream}, o.grads ? &og : nullptr, q, blocks))
            return rc;
        if (!baked_pose_rigid(ob.pose)) return occ_fail(where, "pose must be finite and rigid (max |R^T R - I| <= 1e-4, det R > 0)");
        BakedSceneObject &so = sc.obj[j];
        so.stored = ob.stored;
        so.bits = ob.bits;
        so.index = ob.index;
        so.last = v.sparse ? baked_sparse_rows(v).last : -1;
        so.g = q.g;
        for (int r = 0; r < 3; ++r) {
            for (int a = 0; a < 3; ++a) so.rot[3 * r + a] = ob.pose[4 * r + a];
            so.t[r] = ob.pose[4 * r + 3];
        }
        if (j == 0) v0 = v;
    }
    return PNR_OK;
}

// the scene's forward entries: the checks, then the launch
static int baked_scene_render(const char *entry, const BakedRays &rays, const PnrBakedObject *objects, int n_objects, float step,
                              int white_bkgd, float terminate, float *rgb, float *depth, float *alpha, void *stream) {
    BakedSceneDesc sc;
    BakedVolumeDesc v0;
    long long blocks;
    if (const int rc = baked_scene_check(entry, rays, objects, n_objects, step, white_bkgd, terminate,
                                         {rgb, depth, alpha, nullptr, nullptr, nullptr, nullptr}, stream, sc, v0, blocks))
        return rc;
    if (blocks == 0) return PNR_OK;
    baked_dispatch(v0, [&](auto corner, auto rows) {  // (every object has rows of its own: the type alone)
        using Corner = typename decltype(corner)::type;
        hipLaunchKernelGGL((baked_scene_march_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                           (hipStream_t)stream, rays.src, rays.R, sc, step, terminate, white_bkgd, rgb, depth, alpha);
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
                                         {nullptr, nullptr, nullptr, &grads, d_local, d_poses, workspace}, stream, sc, v0, blocks))
        return rc;
    if (blocks > 0) {
        baked_dispatch(v0, [&](auto corner, auto rows) {
            using Corner = typename decltype(corner)::type;
            hipLaunchKernelGGL((baked_scene_ray_bwd_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                               (hipStream_t)stream, rays.src, rays.R, sc, step, terminate, white_bkgd, d_rgb, d_depth, d_alpha, d_rays,
                               d_local);
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

// the scene's stored-value backward entries: the same checks, then one launch that adds into every buffer that is not NULL
static int baked_scene_stored_backward(const char *entry, const BakedRays &rays, const PnrBakedObject *objects, int n_objects, float step,
                                       int white_bkgd, float terminate, const float *d_rgb, const float *d_depth, const float *d_alpha,
                                       float *const *d_stored, void *stream) {
    const BakedGrads grads = {d_rgb, d_depth, d_alpha, nullptr};
    BakedSceneOut o = {nullptr, nullptr, nullptr, &grads, nullptr, nullptr, nullptr};
    o.d_stored = d_stored;
    o.stored_grads = true;
    BakedSceneDesc sc;
    BakedVolumeDesc v0;
    long long blocks;
    if (const int rc = baked_scene_check(entry, rays, objects, n_objects, step, white_bkgd, terminate, o, stream, sc, v0, blocks)) return rc;
    if (blocks == 0) return PNR_OK;
    BakedSceneStoredGrads out = {};
    bool any = false;
    for (int j = 0; j < n_objects; ++j) {
        out.p[j] = d_stored[j];
        any = any || d_stored[j];
    }
    if (!any) return PNR_OK;  // every object frozen: nothing to add
    baked_dispatch(v0, [&](auto corner, auto rows) {
        using Corner = typename decltype(corner)::type;
        if constexpr (std::is_same<typename Corner::stored_t, float4>::value)  // (no fp16 instantiation: the check refused it)
            hipLaunchKernelGGL((baked_scene_stored_bwd_kernel<Corner, decltype(rows)>), dim3((unsigned)blocks), dim3(BAKED_WAVES * 64), 0,
                               (hipStream_t)stream, rays.src, rays.R, sc, out, step, terminate, white_bkgd, d_rgb, d_depth, d_alpha);
    });
    return pnr_check_launch(entry);
}

}  // namespace pnr

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

// ---- gradients of the scene march with respect to every object's stored values (fp32 storage; d_stored: a HOST array)

extern "C" int pnr_baked_scene_stored_backward_rays(const float *rays, long long R, const PnrBakedObject *objects, int n_objects, float step,
                                                    int white_bkgd, float terminate, const float *d_rgb, const float *d_depth,
                                                    const float *d_alpha, float *const *d_stored, void *stream) {
    return pnr::baked_scene_stored_backward("pnr_baked_scene_stored_backward_rays", pnr::baked_explicit_rays(rays, R), objects, n_objects,
                                            step, white_bkgd, terminate, d_rgb, d_depth, d_alpha, d_stored, stream);
}

extern "C" int pnr_baked_scene_stored_backward_views(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                                     float z_near, float z_far, const PnrBakedObject *objects, int n_objects, float step,
                                                     int white_bkgd, float terminate, const float *d_rgb, const float *d_depth,
                                                     const float *d_alpha, float *const *d_stored, void *stream) {
    return pnr::baked_scene_stored_backward("pnr_baked_scene_stored_backward_views",
                                            pnr::baked_camera_rays(poses, NV, W, H, fx, fy, cx, cy, z_near, z_far), objects, n_objects, step,
                                            white_bkgd, terminate, d_rgb, d_depth, d_alpha, d_stored, stream);
}
