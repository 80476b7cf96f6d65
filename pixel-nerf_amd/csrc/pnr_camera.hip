// pnr_camera.hip -- gradients with respect to the rays and the cameras (training / pose refinement), gfx950.
//
//   camera_record_kernel  one wavefront per (view, sample): the world-space gradient of the sample point through the
//                         positional code, the projection and the bilinear lookup (point_grad in pnr_geom.h, which
//                         position_bwd_kernel calls too), kept whole instead of collapsed to dL/dz -- a ray record
//                         (8 floats) and a camera record (16).
//   ray_reduce_kernel     thread per ray: the ray records summed over (sample, view) in a fixed order, dL/dz pushed through
//                         the sampling maps to near / far (nerf.py:98-161), the last compositing delta added to far.
//   cam_partial_kernel    per source view: the camera records of that view's object summed in fixed chunks (no atomics),
//   cam_final_kernel      the chunks summed in order -> d poses (NV,3,4), d focal / d c (1 or SB rows).
//   gen_rays_bwd_kernel   util.gen_rays backward: d rays (NV,H,W,8) -> d camera-to-world (NV,3,4), workgroup per pose.
// Every sum has a fixed order: the gradients are bit-reproducible.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pnr_common.h"
#include "pnr_device.h"
#include "pnr_entry.h"
#include "pnr_layout.h"

namespace pnr {
namespace {

constexpr int CAM_CW = 4;          // wavefronts per block of the record kernel
constexpr int CAM_REC = 16;        // camera record: dR (9, row-major), dt (3), d(fx, fy), d(cx, cy)
constexpr int RAY_REC = 8;         // ray record: gp (3), z gp + R^T g_vd (3), d . gp, 0
constexpr int CAM_CHUNK = 2048;    // samples per partial sum of cam_partial_kernel
constexpr int CAM_NT = 256;

#pragma clang fp contract(fast)
__global__ void __launch_bounds__(CAM_CW * 64)
camera_record_kernel(const EvalParams q, const float *__restrict__ d_in42, const float *__restrict__ d_zlat,
                     float *__restrict__ ray_rec, float *__restrict__ cam_rec) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long idx = (long long)blockIdx.x * CAM_CW + wv;  // view * P + point
    if (idx >= q.P * q.NS) return;
    const int view = (int)(idx / q.P);
    const int g = (int)(idx - (long long)view * q.P);
    const SamplePoint sp = sample_point_fused(q, g, view);
    const PointGrad pg = point_grad(q, sp, view, idx, d_in42, d_zlat, lane);
    if (lane != 0) return;
    const float *pose = sp.pose, *gi = d_in42 + (size_t)idx * D_IN;
    const float X = sp.X, Y = sp.Y, Z = sp.Z, zz = sp.zz, xc0 = pg.xc0, xc1 = pg.xc1, xc2 = pg.xc2;
    const float du = pg.du, dv = pg.dv, gm0 = pg.gm0, gm1 = pg.gm1, gm2 = pg.gm2, g0 = pg.g0, g1 = pg.g1, g2 = pg.g2;
    // view direction R d (models.py:188-196) enters the network as columns 39..41
    const float v0 = gi[39], v1 = gi[40], v2 = gi[41];
    const float d0 = sp.dx, d1 = sp.dy, d2 = sp.dz;
    // world gradient gp = R^T g ; direction: z gp + R^T g_vd
    const float wx = pose[0] * g0 + pose[4] * g1 + pose[8] * g2;
    const float wy = pose[1] * g0 + pose[5] * g1 + pose[9] * g2;
    const float wz = pose[2] * g0 + pose[6] * g1 + pose[10] * g2;
    const float vx = pose[0] * v0 + pose[4] * v1 + pose[8] * v2;
    const float vy = pose[1] * v0 + pose[5] * v1 + pose[9] * v2;
    const float vz = pose[2] * v0 + pose[6] * v1 + pose[10] * v2;
    float4 *rr = reinterpret_cast<float4 *>(ray_rec + (size_t)idx * RAY_REC);
    float4 *cr = reinterpret_cast<float4 *>(cam_rec + (size_t)idx * CAM_REC);
    // a point on a source camera's plane (xc2 == 0) or a non-finite upstream gradient: the record is dropped, as
    // position_bwd_kernel drops its dL/dz, instead of poisoning every sum it enters
    if (!__builtin_isfinite(g0 + g1 + g2 + gm0 + gm1 + gm2 + v0 + v1 + v2 + du * xc0 / xc2 + dv * xc1 / xc2)) {
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        rr[0] = z4; rr[1] = z4; cr[0] = z4; cr[1] = z4; cr[2] = z4; cr[3] = z4;
        return;
    }
    rr[0] = make_float4(wx, wy, wz, zz * wx + vx);
    rr[1] = make_float4(zz * wy + vy, zz * wz + vz, d0 * wx + d1 * wy + d2 * wz, 0.f);
    // dR = (g_code + g_cam) (x) p + g_vd (x) d, dt = g_cam
    cr[0] = make_float4(g0 * X + v0 * d0, g0 * Y + v0 * d1, g0 * Z + v0 * d2, g1 * X + v1 * d0);
    cr[1] = make_float4(g1 * Y + v1 * d1, g1 * Z + v1 * d2, g2 * X + v2 * d0, g2 * Y + v2 * d1);
    cr[2] = make_float4(g2 * Z + v2 * d2, gm0, gm1, gm2);
    cr[3] = make_float4(du * (-xc0 / xc2), dv * (-xc1 / xc2), du, dv);
}

// dz/d(near), dz/d(far) of a sample on the stratified / importance map z(s) = near (1 - s) + far s (lindisp: 1/z linear in s),
// with s recovered from z (nerf.py:98-148).  far == near: every z equals both and s cannot be recovered (0/0); dn + df = 1
// holds for both maps there, so the sample's gradient goes half to near and half to far -- their sum is exact.
__device__ __forceinline__ void sample_bounds_grad(float z, float near, float far, bool lindisp, float &dn, float &df) {
    if (far == near) {
        dn = 0.5f; df = 0.5f;
        return;
    }
    if (!lindisp) {
        const float s = (z - near) / (far - near);
        dn = 1.f - s; df = s;
    } else {
        const float in = 1.f / near, ifa = 1.f / far;
        const float s = (1.f / z - in) / (ifa - in);
        const float z2 = z * z;
        dn = z2 * (1.f - s) * in * in; df = z2 * s * ifa * ifa;
    }
}

struct RayReduce {
    const float *rays, *z;
    const float *ray_rec;   // (NS, R*K, 8), or null with NS = 0 (sampling maps only)
    const float *dz_comp;   // (R, K) nullable
    const float *d_far;     // (R) nullable: dL/d(last delta)
    const int *ranks;       // (R, Kfd) nullable: sorted positions of the depth samples
    const float *n4, *depth_c;
    float depth_std;
    int Kfd, R, K, NS, lindisp;
    const float *dz_extra;  // (R, K) nullable: dL/dz of the sample positions (sampling-only form)
    float *d_rays;          // (R, 8) out
};

__global__ void __launch_bounds__(256) ray_reduce_kernel(const RayReduce a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.R) return;
    const float near = a.rays[(size_t)r * 8 + 6], far = a.rays[(size_t)r * 8 + 7];
    const long long P = (long long)a.R * a.K;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f, dnear = 0.f, dfar = a.d_far ? a.d_far[r] : 0.f;
    for (int k = 0; k < a.K; ++k) {
        const long long g = (long long)r * a.K + k;
        float dz = (a.dz_comp ? a.dz_comp[g] : 0.f) + (a.dz_extra ? a.dz_extra[g] : 0.f);
        for (int v = 0; v < a.NS; ++v) {
            const float4 *rr = reinterpret_cast<const float4 *>(a.ray_rec + ((size_t)v * P + g) * RAY_REC);
            const float4 p = rr[0], s = rr[1];
            o0 += p.x; o1 += p.y; o2 += p.z;
            e0 += p.w; e1 += s.x; e2 += s.y;
            dz += s.z;
        }
        int jd = -1;
        for (int j = 0; j < a.Kfd && a.ranks; ++j)
            if (a.ranks[(size_t)r * a.Kfd + j] == k) jd = j;
        if (jd >= 0) {
            // depth sample z = max(min(depth + n std, far), near) (nerf.py:157-160): near / far only where the clamp is active;
            // the unclamped ones go to the coarse depth (pnr_depth_sample_backward)
            const float zraw = a.depth_c[r] + a.n4[(size_t)r * a.Kfd + jd] * a.depth_std;
            if (zraw >= far) dfar += dz;
            else if (zraw <= near) dnear += dz;
        } else {
            float dn, df;
            sample_bounds_grad(a.z[g], near, far, a.lindisp != 0, dn, df);
            dnear += dz * dn;
            dfar += dz * df;
        }
    }
    float4 *out = reinterpret_cast<float4 *>(a.d_rays + (size_t)r * 8);
    out[0] = make_float4(o0, o1, o2, e0);
    out[1] = make_float4(e1, e2, dnear, dfar);
}

// grid (chunks, SB*NS): block sums chunk `blockIdx.x` of the samples of source view row nv = obj * NS + view
__global__ void __launch_bounds__(CAM_NT) cam_partial_kernel(const float *__restrict__ cam_rec, long long P, int NS,
                                                             long long per_obj_pts, int nchunk, float *__restrict__ part) {
    __shared__ float red[CAM_NT];
    const int nv = blockIdx.y, obj = nv / NS, view = nv - obj * NS;
    const int comp = threadIdx.x & (CAM_REC - 1), lane = threadIdx.x / CAM_REC;  // 16 sample lanes x 16 components
    const long long lo = (long long)blockIdx.x * CAM_CHUNK;
    const long long hi = min(lo + CAM_CHUNK, per_obj_pts);
    const float *base = cam_rec + ((size_t)view * P + (size_t)obj * per_obj_pts) * CAM_REC;
    float acc = 0.f;
    for (long long i = lo + lane; i < hi; i += CAM_NT / CAM_REC) acc += base[(size_t)i * CAM_REC + comp];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (lane == 0) {
        float s = 0.f;
        for (int l = 0; l < CAM_NT / CAM_REC; ++l) s += red[l * CAM_REC + comp];
        part[((size_t)nv * nchunk + blockIdx.x) * CAM_REC + comp] = s;
    }
}

// one block: thread t < NV*12 -> d pose[nv][t%12]; then the intrinsics rows (1 = shared: summed over every object)
__global__ void __launch_bounds__(CAM_NT) cam_final_kernel(const float *__restrict__ part, int SB, int NS, int nchunk,
                                                           int n_focal, int n_c, float *__restrict__ d_poses,
                                                           float *__restrict__ d_focal, float *__restrict__ d_c) {
    const int NV = SB * NS;
    for (int t = threadIdx.x; t < NV * 12 + 2 * n_focal + 2 * n_c; t += blockDim.x) {
        if (t < NV * 12) {
            const int nv = t / 12, e = t - nv * 12, i = e / 4, j = e - i * 4;
            const int comp = j < 3 ? i * 3 + j : 9 + i;  // (3,4) layout: R columns 0..2, t column 3
            if (!d_poses) continue;
            float s = 0.f;
            for (int ch = 0; ch < nchunk; ++ch) s += part[((size_t)nv * nchunk + ch) * CAM_REC + comp];
            d_poses[t] = s;
            continue;
        }
        int u = t - NV * 12;
        const bool is_f = u < 2 * n_focal;
        if (!is_f) u -= 2 * n_focal;
        float *dst = is_f ? d_focal : d_c;
        if (!dst) continue;
        const int rows = is_f ? n_focal : n_c;
        const int row = u / 2, comp = (is_f ? 12 : 14) + (u - row * 2);
        const int o_lo = rows > 1 ? row : 0, o_hi = rows > 1 ? row + 1 : SB;
        float s = 0.f;
        for (int o = o_lo; o < o_hi; ++o)
            for (int v = 0; v < NS; ++v)
                for (int ch = 0; ch < nchunk; ++ch) s += part[((size_t)(o * NS + v) * nchunk + ch) * CAM_REC + comp];
        dst[u] = s;
    }
}

// util.gen_rays (util.py:238-276, ndc=False): rays = (t, R dir(px), near, far); workgroup per pose, fixed-order tree sum
#pragma clang fp contract(off)  // the forward's direction, bit for bit (gen_rays_kernel)
__global__ void __launch_bounds__(CAM_NT) gen_rays_bwd_kernel(const float *__restrict__ d_rays, int W, int H, float fx,
                                                              float fy, float cx, float cy, float *__restrict__ d_poses) {
    __shared__ float red[12][CAM_NT];
    const int n = blockIdx.x;
    float acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.f;
    const long long npx = (long long)W * H;
    for (long long i = threadIdx.x; i < npx; i += CAM_NT) {
        const int px = (int)(i % W), py = (int)(i / W);
        const float X = ((float)px - cx) / fx, Y = ((float)py - cy) / fy;
        float d0 = X, d1 = -Y, d2 = -1.f;
        const float nrm = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
        d0 /= nrm; d1 /= nrm; d2 /= nrm;
        const float *g = d_rays + ((size_t)n * npx + i) * 8;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[a * 4 + 0] += g[3 + a] * d0;
            acc[a * 4 + 1] += g[3 + a] * d1;
            acc[a * 4 + 2] += g[3 + a] * d2;
            acc[a * 4 + 3] += g[a];
        }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) red[e][threadIdx.x] = acc[e];
    __syncthreads();
    for (int s = CAM_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int e = 0; e < 12; ++e) red[e][threadIdx.x] += red[e][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 12) d_poses[(size_t)n * 12 + threadIdx.x] = red[threadIdx.x][0];
}
#pragma clang fp contract(fast)

}  // namespace
}  // namespace pnr

using namespace pnr;

extern "C" size_t pnr_camera_backward_workspace_bytes(int R, int K, int rays_per_obj, int NS) {
    if (R <= 0 || K <= 0 || rays_per_obj <= 0 || NS <= 0) return 0;
    const long long P = (long long)R * K, per_obj_pts = (long long)rays_per_obj * K;
    const long long nchunk = (per_obj_pts + CAM_CHUNK - 1) / CAM_CHUNK;
    const long long SB = R / rays_per_obj;
    return (size_t)(P * NS * (RAY_REC + CAM_REC) + SB * NS * nchunk * CAM_REC) * sizeof(float);
}

extern "C" int pnr_camera_backward(const PnrScene *s, const float *rays, const float *z, int R, int rays_per_obj, int K,
                                   int lindisp, const float *d_in42, const float *d_zlat, const float *dz_comp,
                                   const float *d_far, const int *ranks, const float *n4, int Kfd, const float *depth_c,
                                   float depth_std, float *d_rays, float *d_poses, float *d_focal, float *d_c,
                                   void *workspace, void *stream) {
    EvalParams q = {};  // (camera_record_kernel holds a point index in an int)
    if (int rc = ray_samples(q, "pnr_camera_backward", s, rays, z, R, rays_per_obj, K, false, {0, INDEX_I32, 0})) return rc;
    if (!d_in42 || !d_zlat || !workspace) return pnr_fail(PNR_E_INVALID, "pnr_camera_backward: bad argument");
    if (ranks && (!n4 || !depth_c || Kfd <= 0 || Kfd > K)) return pnr_fail(PNR_E_INVALID, "pnr_camera_backward: depth samples");
    const long long n = q.P * q.NS;
    float *ray_rec = (float *)workspace;
    float *cam_rec = ray_rec + n * RAY_REC;
    const long long per_obj_pts = (long long)rays_per_obj * K;
    const int nchunk = (int)((per_obj_pts + CAM_CHUNK - 1) / CAM_CHUNK);
    float *part = cam_rec + n * CAM_REC;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(camera_record_kernel, dim3((unsigned)((n + CAM_CW - 1) / CAM_CW)), dim3(CAM_CW * 64), 0, st, q, d_in42,
                       d_zlat, ray_rec, cam_rec);
    if (d_rays) {
        RayReduce a = {rays, z, ray_rec, dz_comp, d_far, ranks, n4, depth_c, depth_std, ranks ? Kfd : 0, R, K, s->NS,
                       lindisp, nullptr, d_rays};
        hipLaunchKernelGGL(ray_reduce_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, a);
    }
    if (d_poses || d_focal || d_c) {
        hipLaunchKernelGGL(cam_partial_kernel, dim3((unsigned)nchunk, (unsigned)(s->SB * s->NS)), dim3(CAM_NT), 0, st, cam_rec,
                           q.P, s->NS, per_obj_pts, nchunk, part);
        hipLaunchKernelGGL(cam_final_kernel, dim3(1), dim3(CAM_NT), 0, st, part, s->SB, s->NS, nchunk, s->n_focal, s->n_c,
                           d_poses, d_focal, d_c);
    }
    return pnr_check_launch("pnr_camera_backward");
}

extern "C" int pnr_gen_rays_backward(const float *d_rays, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                     float *d_poses, void *stream) {
    if (!d_rays || !d_poses || NV <= 0 || W <= 0 || H <= 0) return pnr_fail(PNR_E_INVALID, "pnr_gen_rays_backward: bad argument");
    hipLaunchKernelGGL(gen_rays_bwd_kernel, dim3((unsigned)NV), dim3(CAM_NT), 0, (hipStream_t)stream, d_rays, W, H, fx, fy, cx,
                       cy, d_poses);
    return pnr_check_launch("pnr_gen_rays_backward");
}

extern "C" int pnr_sample_bounds_backward(const float *rays, const float *z, const float *dz, int R, int K, int lindisp,
                                          const int *ranks, const float *n4, int Kfd, const float *depth_c, float depth_std,
                                          const float *d_far, float *d_rays, void *stream) {
    if (!rays || !z || !dz || !d_rays || R < 0 || K <= 0) return pnr_fail(PNR_E_INVALID, "pnr_sample_bounds_backward: bad argument");
    if (ranks && (!n4 || !depth_c || Kfd <= 0 || Kfd > K))
        return pnr_fail(PNR_E_INVALID, "pnr_sample_bounds_backward: depth samples");
    if (R == 0) return PNR_OK;
    RayReduce a = {rays, z, nullptr, nullptr, d_far, ranks, n4, depth_c, depth_std, ranks ? Kfd : 0, R, K, 0, lindisp, dz, d_rays};
    hipLaunchKernelGGL(ray_reduce_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return pnr_check_launch("pnr_sample_bounds_backward");
}
