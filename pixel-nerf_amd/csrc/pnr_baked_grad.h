// pnr_baked_grad.h -- what the two ray-gradient kernels of the baked march share (baked_march_ray_bwd_kernel, pnr_baked_grad.hip: one
// volume; baked_scene_ray_bwd_kernel, pnr_baked_scene.hip: a scene): the spatial derivative of the blend, the slope of the fractions,
// the fp64 factors of the transmittance and the basis functions' derivative.  The walk itself -- upstream gradient, first walk, scan
// step, row write -- stands in each kernel: profiles/baked_notes.md, "A file per concern".  The mathematics: pnr_baked_grad.hip.
#pragma once
#include "pnr_baked.h"

namespace pnr {

#pragma clang fp contract(off)  // as in pnr_baked.h: every product, sum and quotient is rounded on its own

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

// the factor of sample s for the fp64 product: 1 where the forward's is exactly 1 (not active, or no rows)
template <class Corner, class Rows>
__device__ __forceinline__ double baked_tf_exact(const BakedParams &q, const Corner &corner, const Rows &rows, const BakedSample &s,
                                                 float &sigma) {
    BakedCell<Rows> cell;
    bool found;
    sigma = baked_value(q, corner, rows, s, cell, found).w;
    return found ? baked_alpha_exact(q.step, sigma).tf : 1.0;
}

// prod of those factors over chunk c (every lane)
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
// of the clamps (ShCorner::mask)
template <class Stored, int N>
__device__ __forceinline__ void baked_basis_grad(const RgbaCornerOf<Stored> &, long long, float4, float (&)[N]) {}
template <int B, class Stored, int N>
__device__ __forceinline__ void baked_basis_grad(const ShCorner<B, Stored> &corner, long long point, float4 g, float (&dY)[N]) {
    g = corner.mask(point, g);
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

#pragma clang fp contract(fast)

}  // namespace pnr
