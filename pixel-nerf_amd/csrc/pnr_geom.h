// pnr_geom.h -- the one definition of a sample's geometry: sample -> world point -> rotated point -> grid coordinates ->
// bilinear corners.  The forward kernels (geometry_item / project_point in pnr_device.h, feat_f32_kernel), the sparse fold's
// row marking (fold_mark_kernel), the latent scatter kernels and the two position-gradient kernels all take it from here, so
// the texels one of them marks, scatters to or differentiates are by construction the texels the forward reads.
// Included by pnr_device.h behind EvalParams; reach it through that header.
#pragma once
#include "pnr_wave.h"

namespace pnr {

struct RayPoint {
    int r;                // ray index
    float zz;             // depth along the ray
    float X, Y, Z;        // world point o + z d (nerf.py:185)
    float dx, dy, dz;     // ray direction
};
struct SamplePoint : RayPoint {
    int obj;
    const float *pose;    // (3,4) of (obj, view), row obj * NS + view
    float xr0, xr1, xr2;  // xyz_rot = R x (models.py:162-164)
};

// Sample g of the explicit-rays form (q.rays, q.z), its world point and the rotation into a source view.  Written once and
// compiled in both contraction states: as the reference's separately rounded operations for everything that has to agree with
// the forward kernels to the bit (rotate_point, ray_point, sample_point), and contracted for position_bwd_kernel and
// camera_record_kernel (the *_fused names), which have always formed the point with fused multiply-adds -- see point_grad.
#define PNR_SAMPLE_POINT_FUNCTIONS(ROTATE, RAY_POINT, SAMPLE_POINT)                                                            \
    __device__ __forceinline__ float3 ROTATE(const float *pose, float X, float Y, float Z) {                                   \
        return make_float3(pose[0] * X + pose[1] * Y + pose[2] * Z, pose[4] * X + pose[5] * Y + pose[6] * Z,                   \
                           pose[8] * X + pose[9] * Y + pose[10] * Z);                                                          \
    }                                                                                                                          \
    __device__ __forceinline__ RayPoint RAY_POINT(const EvalParams &q, int g) {                                                \
        RayPoint s;                                                                                                            \
        s.r = g / q.K;                                                                                                         \
        const float *ray = q.rays + (size_t)s.r * 8;                                                                           \
        s.zz = q.z[g];                                                                                                         \
        s.dx = ray[3]; s.dy = ray[4]; s.dz = ray[5];                                                                           \
        s.X = ray[0] + s.zz * s.dx; s.Y = ray[1] + s.zz * s.dy; s.Z = ray[2] + s.zz * s.dz;                                    \
        return s;                                                                                                              \
    }                                                                                                                          \
    __device__ __forceinline__ SamplePoint SAMPLE_POINT(const EvalParams &q, int g, int view) {                                \
        SamplePoint s;                                                                                                         \
        static_cast<RayPoint &>(s) = RAY_POINT(q, g);                                                                          \
        s.obj = s.r / q.per_obj;                                                                                               \
        s.pose = q.poses + (size_t)(s.obj * q.NS + view) * 12;                                                                 \
        const float3 xr = ROTATE(s.pose, s.X, s.Y, s.Z);                                                                       \
        s.xr0 = xr.x; s.xr1 = xr.y; s.xr2 = xr.z;                                                                              \
        return s;                                                                                                              \
    }
#pragma clang fp contract(fast)  // position_bwd_kernel / camera_record_kernel: only sample_point_fused is called, it pulls the other two
PNR_SAMPLE_POINT_FUNCTIONS(rotate_point_fused, ray_point_fused, sample_point_fused)

// ---------------------------------------------------------------- the reference's fp32 op order (no FMA contraction)
// Camera-space point and pinhole projection (models.py:165,206-212), SpatialEncoder.index scaling (encoder.py:96-99,161-163)
// and grid_sample(bilinear, border, align_corners=True) corner cells / weights, every operation rounded on its own like the
// PyTorch eager path.  This is the authoritative order: whoever needs the forward's bits calls these, nobody retypes them.
#pragma clang fp contract(off)
PNR_SAMPLE_POINT_FUNCTIONS(rotate_point, ray_point, sample_point)
#undef PNR_SAMPLE_POINT_FUNCTIONS

// rotated point -> clamped position (ix, iy) on the latent grid of (obj, view); NaN for a point on the camera plane, which
// every caller maps to texel 0 by its own rule
__device__ __forceinline__ float2 grid_coords(const EvalParams &q, const float *pose, int obj, float xr0, float xr1, float xr2) {
    const float xc0 = xr0 + pose[3], xc1 = xr1 + pose[7], xc2 = xr2 + pose[11];
    // CODE GENERATION NOTE (re-check when the compiler changes: dump pnr_mlp.hip / pnr_split.hip with --cuda-device-only -S and
    // compare with the previous build).  `row` is a 64-bit local so that both conditionals below are selects over values that exist
    // anyway; written as `q.n_focal > 1 ? obj * 2 : 0` they are branches, this helper ends in more than one block, and the
    // optimiser then moves the three adds above behind the loads: eval_kernel and eval_split_kernel came out with another
    // instruction order (same registers, same results).  pick() below serves the same purpose in bilinear_corners.
    const long long row = obj * 2;
    const float *fo = q.focal + (q.n_focal > 1 ? row : 0);
    const float *cc = q.c + (q.n_c > 1 ? row : 0);
    float u = -xc0 / xc2; u = u * fo[0]; u = u + cc[0];
    float v = -xc1 / xc2; v = v * fo[1]; v = v + cc[1];
    const float Wl = (float)q.Wl, Hl = (float)q.Hl;
    const float lsx = Wl / (Wl - 1.f) * 2.f, lsy = Hl / (Hl - 1.f) * 2.f;
    const float gx = u * (lsx / q.img_w) - 1.f, gy = v * (lsy / q.img_h) - 1.f;
    float ix = ((gx + 1.f) / 2.f) * (Wl - 1.f), iy = ((gy + 1.f) / 2.f) * (Hl - 1.f);
    ix = fminf(Wl - 1.f, fmaxf(ix, 0.f));
    iy = fminf(Hl - 1.f, fmaxf(iy, 0.f));
    return make_float2(ix, iy);
}

// Conditions in this block are selects over values that are computed anyway, so each helper is one straight block and the
// compiler keeps its order of operations wherever it inlines it (see the note in grid_coords).
__device__ __forceinline__ float pick(bool c, float a, float b) { return c ? a : b; }

// the cell of a grid position and its four corners nw, ne, sw, se; a corner beyond the last column / row is clamped onto it
// and carries weight 0
struct Corners {
    float ix0, iy0, ix1, iy1;
    int x0, y0, xl, yl;  // the cell; last column / row of the grid
    float w[4];          // weights of the position the cell was made from
    // east column / south row, clamped onto the grid (the corner then carries weight 0)
    __device__ __forceinline__ int x1() const { return min(x0 + 1, xl); }
    __device__ __forceinline__ int y1() const { return min(y0 + 1, yl); }
    __device__ __forceinline__ void products(float px, float py, float (&wt)[4]) const {
        wt[0] = (ix1 - px) * (iy1 - py); wt[1] = (px - ix0) * (iy1 - py);
        wt[2] = (ix1 - px) * (py - iy0); wt[3] = (px - ix0) * (py - iy0);
    }
    __device__ __forceinline__ void zero_outside(float (&wt)[4]) const {
        const bool x_out = x0 + 1 > xl;  // no column behind the cell
        wt[1] = pick(x_out, 0.f, wt[1]);
        const bool y_out = y0 + 1 > yl;  // no row
        wt[3] = pick(y_out, 0.f, pick(x_out, 0.f, wt[3])); wt[2] = pick(y_out, 0.f, wt[2]);
    }
    // weights of a position inside the cell
    __device__ __forceinline__ void weights(float px, float py, float (&wt)[4]) const {
        products(px, py, wt);
        zero_outside(wt);
    }
};
__device__ __forceinline__ Corners bilinear_corners(float ix, float iy, int Wl, int Hl) {
    Corners k;
    k.ix0 = floorf(ix); k.iy0 = floorf(iy);
    k.ix1 = k.ix0 + 1.f; k.iy1 = k.iy0 + 1.f;
    k.products(ix, iy, k.w);
    k.x0 = (int)k.ix0; k.y0 = (int)k.iy0;
    k.xl = Wl - 1; k.yl = Hl - 1;
    k.zero_outside(k.w);
    return k;
}

// Latent scatter: a segment is at most SEG_B consecutive samples of a ray that share a cell (scatter_segments_kernel cuts
// there; SEG_B divides 64, so a wave boundary is a cut).  acc[c] = sum over the segment of w_c * gradient for the four corners
// of that cell; slots beyond the segment carry zero gradients.
constexpr int SEG_B = 4;
__device__ __forceinline__ Corners segment_corner_sums(const float2 (&pos)[SEG_B], const f32x4 (&v)[SEG_B], int Wl, int Hl,
                                                       f32x4 (&acc)[4]) {
    const Corners k = bilinear_corners(pos[0].x, pos[0].y, Wl, Hl);  // the segment's cell
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < SEG_B; ++b) {
        float w[4];
        k.weights(pos[b].x, pos[b].y, w);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[c][e] += w[c] * v[b][e];
    }
    return k;
}

// XCD-aware placement of the slab kernels' workgroups: the GRP channel slices that share 128-byte lines of a gradient row form
// a group, and a group gets consecutive slots of ONE XCD (workgroups are dealt to the 8 XCDs round-robin), so a line is
// fetched into one L2 once.  Workgroup lid of ngroups * GRP -> (group, slice inside it).
__device__ __forceinline__ void xcd_group_slot(int lid, int ngroups, int GRP, int &grp, int &sub) {
    const int full = (ngroups >> 3) * (8 * GRP);
    if (lid < full) { const int k = lid >> 3; grp = (k / GRP) * 8 + (lid & 7); sub = k % GRP; }
    else { const int rem = lid - full; grp = full / GRP + rem / GRP; sub = rem % GRP; }
}

// ---------------------------------------------------------------- position gradient (contracted)
#pragma clang fp contract(fast)
// dL/d(camera-space point) of sample (view, point) = row idx of d_in42 / d_zlat, through the bilinear lookup (du, dv: dL/d of
// the pixel coordinates; gm: their chain to the camera-space point xc) and through the positional code (gc).  One wavefront
// per sample: lane l reads channels 8l..8l+7 of the four corner rows, lanes 0..20 differentiate the code; the results are
// wave sums, valid in every lane.
// KNOWN DIFFERENCE, kept on purpose: this is the backward's own arithmetic -- the sample comes from sample_point_fused and
// ix is ((u sx - 1 + 1) / 2)(Wl - 1) with sx = lsx / img_w folded in and contraction allowed, where the forward
// (grid_coords) rounds every operation.  A coordinate within an ulp of a texel boundary can therefore be differentiated in
// the neighbouring cell (known differences); aligning the two changes results and is left to a later change.
struct PointGrad {
    float du, dv;            // dL/du, dL/dv (0 where grid_sample's border clip is active)
    float gm0, gm1, gm2;     // their chain to xc
    float g0, g1, g2;        // gm + (the positional code's dL/d xr): dL/d xr (xc = xr + t)
    float xc0, xc1, xc2;     // camera-space point xr + t
};
__device__ __forceinline__ PointGrad point_grad(const EvalParams &q, const SamplePoint &s, int view, long long idx,
                                                const float *__restrict__ d_in42, const float *__restrict__ d_zlat, int lane) {
    PointGrad o;
    const float xr0 = s.xr0, xr1 = s.xr1, xr2 = s.xr2;
    const float xc0 = xr0 + s.pose[3], xc1 = xr1 + s.pose[7], xc2 = xr2 + s.pose[11];
    const float *fo = q.focal + (q.n_focal > 1 ? s.obj * 2 : 0);
    const float *cc = q.c + (q.n_c > 1 ? s.obj * 2 : 0);
    const float u = -xc0 / xc2 * fo[0] + cc[0], v = -xc1 / xc2 * fo[1] + cc[1];
    const float Wl = (float)q.Wl, Hl = (float)q.Hl;
    const float sx = Wl / (Wl - 1.f) * 2.f / q.img_w, sy = Hl / (Hl - 1.f) * 2.f / q.img_h;
    float ix = ((u * sx - 1.f + 1.f) / 2.f) * (Wl - 1.f), iy = ((v * sy - 1.f + 1.f) / 2.f) * (Hl - 1.f);
    // grid_sample border padding: clip_coordinates_set_grad -> gradient 0 outside (0, size-1)
    const bool gx_on = ix > 0.f && ix < Wl - 1.f, gy_on = iy > 0.f && iy < Hl - 1.f;
    ix = fminf(Wl - 1.f, fmaxf(ix, 0.f));
    iy = fminf(Hl - 1.f, fmaxf(iy, 0.f));
    float six = 0.f, siy = 0.f;
    if ((gx_on || gy_on) && ix == ix && iy == iy) {
        const Corners k = bilinear_corners(ix, iy, q.Wl, q.Hl);
        const float ax = ix - k.ix0, ay = iy - k.iy0;  // fractional parts
        const size_t rowbase = (size_t)(s.obj * q.NS + view) * (size_t)(q.Hl * q.Wl);
        const int x0 = k.x0, y0 = k.y0, x1 = k.x1(), y1 = k.y1();
        const float *nw = q.latent + (rowbase + (size_t)y0 * q.Wl + x0) * C_LAT + lane * 8;
        const float *ne = q.latent + (rowbase + (size_t)y0 * q.Wl + x1) * C_LAT + lane * 8;
        const float *sw = q.latent + (rowbase + (size_t)y1 * q.Wl + x0) * C_LAT + lane * 8;
        const float *se = q.latent + (rowbase + (size_t)y1 * q.Wl + x1) * C_LAT + lane * 8;
        const float *dz = d_zlat + (size_t)idx * C_LAT + lane * 8;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {  // 16-byte loads: 10 in flight per lane
            const f32x4 a = *reinterpret_cast<const f32x4 *>(nw + 4 * hh), b = *reinterpret_cast<const f32x4 *>(ne + 4 * hh);
            const f32x4 c = *reinterpret_cast<const f32x4 *>(sw + 4 * hh), d = *reinterpret_cast<const f32x4 *>(se + 4 * hh);
            const f32x4 gq = *reinterpret_cast<const f32x4 *>(dz + 4 * hh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                six += gq[e] * ((1.f - ay) * (b[e] - a[e]) + ay * (d[e] - c[e]));   // d zlat / d ix
                siy += gq[e] * ((1.f - ax) * (c[e] - a[e]) + ax * (d[e] - b[e]));   // d zlat / d iy
            }
        }
    }
    // positional code: [x, sin(f_k x), sin(f_k x + pi/2)] , f_k = 1.5 * 2^k  (code.py:37-41).  Lane l < 18 differentiates
    // band k = l / 3 of coordinate c = l % 3; lanes 18..20 carry the identity part; summed per coordinate below
    float gc0 = 0.f, gc1 = 0.f, gc2 = 0.f;
    if (lane < 21) {
        const float *gi = d_in42 + (size_t)idx * D_IN;
        const float HALF_PI = 1.57079637050628662109375f;
        const int k = lane / 3, c = lane - 3 * k;
        const float xc = c == 0 ? xr0 : (c == 1 ? xr1 : xr2);
        float term;
        if (k < 6) {
            const float f = 1.5f * (float)(1 << k), a = xc * f;
            term = f * (cosf(a) * gi[3 + 6 * k + c] + cosf(__builtin_fmaf(xc, f, HALF_PI)) * gi[3 + 6 * k + 3 + c]);
        } else {
            term = gi[c];
        }
        gc0 = c == 0 ? term : 0.f; gc1 = c == 1 ? term : 0.f; gc2 = c == 2 ? term : 0.f;
    }
    gc0 = wave_sum(gc0); gc1 = wave_sum(gc1); gc2 = wave_sum(gc2);
    six = wave_sum(six);
    siy = wave_sum(siy);
    o.du = gx_on ? six * (Wl - 1.f) * 0.5f * sx : 0.f;
    o.dv = gy_on ? siy * (Hl - 1.f) * 0.5f * sy : 0.f;
    // u = -xc0/xc2 fx + cx ; v = -xc1/xc2 fy + cy   (fy already negated in `focal`): gm = d/d xc
    o.gm0 = -fo[0] / xc2 * o.du;
    o.gm1 = -fo[1] / xc2 * o.dv;
    o.gm2 = (xc0 * fo[0] * o.du + xc1 * fo[1] * o.dv) / (xc2 * xc2);
    o.g0 = o.gm0 + gc0; o.g1 = o.gm1 + gc1; o.g2 = o.gm2 + gc2;
    o.xc0 = xc0; o.xc1 = xc1; o.xc2 = xc2;
    return o;
}

}  // namespace pnr
