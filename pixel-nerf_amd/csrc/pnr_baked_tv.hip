// pnr_baked_tv.hip -- total variation of the stored values of a baked volume for gfx950 (pnr_baked_tv; include/pixelnerf_hip.h,
// "Total-variation prior"): the smoothness prior of a fit.  The array is taken as float4s -- a row is B of them, z the fastest grid
// axis -- and one thread takes one float4
// (point p, basis k): consecutive lanes read consecutive 16-byte words, and the neighbour of p along an axis is a fixed offset
// (dense) or the row index[p +- offset] (sparse).  One pass gives both halves; at most TV_MAX_BLOCKS workgroups, each walking its
// slab of the array with the stride of the workgroups that share the slab.  The value: each thread adds w . n(p) in fp64, a
// block leaves one partial, baked_tv_final_kernel adds the partials; every order is fixed by the launch, which depends on the
// sizes alone.  The gradient in GATHER form: the thread that owns S[p] recomputes the norms of its three back neighbours (a
// 13-point stencil) and adds into grad[p] alone -- no atomics, the same bytes on every call.
#include "pnr_baked.h"

namespace pnr {

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

}  // namespace pnr

// ---- total variation of the stored values: the value, and its gradient ADDED into `grad` (fp32 storage; index == NULL: dense)

extern "C" size_t pnr_baked_tv_workspace_bytes(void) { return pnr::TV_MAX_BLOCKS * sizeof(double); }

extern "C" int pnr_baked_tv(const float *stored, long long M, int degree, const int32_t *index, const int32_t *ids, int nx, int ny, int nz,
                            const float *w, float eps, const float *scale, float *value32, double *value64, float *grad, void *workspace,
                            void *stream) {
    using namespace pnr;
    const char *entry = "pnr_baked_tv";
    const BakedVolumeDesc v = baked_stored(stored, 0, M, degree, index);
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
