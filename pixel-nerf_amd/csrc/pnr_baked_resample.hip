// pnr_baked_resample.hip -- the stored values of a baked volume on another point count over the SAME box, for gfx950
// (pnr_baked_resample; include/pixelnerf_hip.h, "Resampling a baked volume"): what lets a fitted volume change resolution without
// another bake.  The array is taken as float4s -- a row is B of them, z the fastest grid axis -- and one thread writes one
// destination float4 (point, basis k), k fastest, then z: consecutive lanes store consecutive 16-byte words.  A GATHER: a thread
// reads the eight source float4s around its point and writes its own word alone -- no atomics, the same bytes on every call.
// Where a destination point lies in the source grid is INTEGER arithmetic, so a refinement (n' - 1 = m (n - 1)) is exact: the old
// points are found at fraction 0 and copied.  A view-dependent volume interpolates its COEFFICIENTS: no basis, no clamp.
// Out of scope: autograd through the resampling, changing the box, fp16 destinations.
#include "pnr_baked.h"

namespace pnr {

constexpr int RESAMPLE_THREADS = 256;

struct ResampleParams {
    int nsx, nsy, nsz, ndx, ndy, ndz;  // source and destination points per axis
    long long Pd, rows_src;      // destination points; the kept rows of a sparse source
    long long total;             // destination float4s: rows x B
    const int32_t *index;        // sparse source: (ns) ranks, -1 elsewhere
    const int32_t *ids_dst;      // the destination rows' linear ids, or NULL: every point in order
};

#pragma clang fp contract(off)  // a + f (b - a): the product, the difference and the sum each rounded on its own

// the 1-D blend of the march, as a SELECT at f == 0: a coincident point copies its source value, -0 included
__device__ __forceinline__ float4 resample_lerp(const float4 a, const float4 b, float f) {
    const float4 v = baked_lerp(a, b, f);
    return f == 0.f ? a : v;
}

// where point i of n_dst lies among n_src: num = i (n_src - 1), cell q = num / (n_dst - 1), fraction rem / (n_dst - 1) -- one rounding
__device__ __forceinline__ void resample_axis(int i, int n_src, int n_dst, int &i0, int &i1, float &f) {
    const long long num = (long long)i * (n_src - 1), den = n_dst - 1;
    const long long q = num / den, rem = num % den;
    i0 = (int)q;
    i1 = (int)(q + 1 < n_src - 1 ? q + 1 : n_src - 1);
    f = (float)rem / (float)den;
}

template <int B, class Stored, bool SPARSE>
__global__ void __launch_bounds__(RESAMPLE_THREADS)
baked_resample_kernel(const Stored *__restrict__ src, float4 *__restrict__ dst, const ResampleParams q) {
    const long long t = (long long)blockIdx.x * RESAMPLE_THREADS + threadIdx.x;
    if (t >= q.total) return;
    const long long m = t / B;
    const int kb = (int)(t - m * B);
    long long p = m;
    if (q.ids_dst) {
        p = q.ids_dst[m];
        if (p < 0 || p >= q.Pd) {  // not a point of the destination grid: a row of zeros, nothing is read for it
            dst[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
    }
    const long long rz = p / q.ndz;
    const int k = (int)(p - rz * q.ndz), i = (int)(rz / q.ndy), j = (int)(rz - (long long)i * q.ndy);
    int x0, x1, y0, y1, z0, z1;
    float fx, fy, fz;
    resample_axis(i, q.nsx, q.ndx, x0, x1, fx);
    resample_axis(j, q.nsy, q.ndy, y0, y1, fy);
    resample_axis(k, q.nsz, q.ndz, z0, z1, fz);
    // the source float4 (point, kb); a sparse source reads a corner that is not kept as zeros (what to_dense() holds there)
    const auto at = [&](int xi, int yi, int zi) -> float4 {
        const long long point = ((long long)xi * q.nsy + yi) * q.nsz + zi;
        if (!SPARSE) return baked_widen(src[point * B + kb]);
        const long long r = q.index[point];
        return r >= 0 && r < q.rows_src ? baked_widen(src[r * B + kb]) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    // the nested blend of the march: along z, then y, then x
    const float4 v00 = resample_lerp(at(x0, y0, z0), at(x0, y0, z1), fz), v01 = resample_lerp(at(x0, y1, z0), at(x0, y1, z1), fz);
    const float4 v10 = resample_lerp(at(x1, y0, z0), at(x1, y0, z1), fz), v11 = resample_lerp(at(x1, y1, z0), at(x1, y1, z1), fz);
    dst[t] = resample_lerp(resample_lerp(v00, v01, fy), resample_lerp(v10, v11, fy), fx);
}
#pragma clang fp contract(fast)

// nx ny nz, or -1 when the grid has 2^31 points or more (no product overflows: each factor is below 2^31)
static inline long long resample_points(int nx, int ny, int nz) {
    const long long xy = (long long)nx * ny;
    if (xy >= (1LL << 31)) return -1;
    const long long P = xy * nz;
    return P >= (1LL << 31) ? -1 : P;
}

}  // namespace pnr

extern "C" int pnr_baked_resample(const void *src, int storage_half, long long M, int degree, const int32_t *index, int nx, int ny, int nz,
                                  float *dst, long long M_dst, const int32_t *ids_dst, int nx_dst, int ny_dst, int nz_dst, void *stream) {
    using namespace pnr;
    const char *entry = "pnr_baked_resample";
    if (degree < -1 || degree > 2) return occ_fail(entry, DEGREE_HALF);
    if (storage_half != 0 && storage_half != 1) return occ_fail(entry, "storage_half must be 0 or 1");
    if (nx < 2 || ny < 2 || nz < 2 || nx_dst < 2 || ny_dst < 2 || nz_dst < 2) return occ_fail(entry, "every axis needs at least 2 grid points");
    const long long Ps = resample_points(nx, ny, nz), Pd = resample_points(nx_dst, ny_dst, nz_dst);
    if (Ps < 0 || Pd < 0) return occ_fail(entry, "the grid must have fewer than 2^31 points");
    const bool sparse = index != nullptr;
    if ((sparse && M < 0) || (ids_dst && M_dst < 0)) return occ_fail(entry, "bad sizes (M)");
    const int B = degree < 0 ? 1 : (degree + 1) * (degree + 1);
    const long long rows_src = sparse ? M : Ps, rows_dst = ids_dst ? M_dst : Pd;
    if (rows_dst == 0) return PNR_OK;  // nothing to write
    if (!dst || (rows_src > 0 && !src)) return occ_fail(entry, "null argument");
    if (storage_half ? baked_misaligned8(src) : occ_misaligned16(src))
        return occ_fail(entry, storage_half ? "src must be 8-byte aligned" : "src must be 16-byte aligned");
    if (occ_misaligned16(dst)) return occ_fail(entry, "dst must be 16-byte aligned");
    if (baked_misaligned4(index) || baked_misaligned4(ids_dst)) return occ_fail(entry, "index and ids_dst must be 4-byte aligned");
    ResampleParams q = {nx, ny, nz, nx_dst, ny_dst, nz_dst, Pd, rows_src, rows_dst * B, index, ids_dst};
    const long long blocks = (q.total + RESAMPLE_THREADS - 1) / RESAMPLE_THREADS;  // < 2^31 x 9 / 256
    const auto launch = [&](auto kernel, auto stored) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(RESAMPLE_THREADS), 0, (hipStream_t)stream,
                           static_cast<const typename decltype(stored)::type *>(src), reinterpret_cast<float4 *>(dst), q);
    };
    // B, storage and layout, each decided once: 3 x 2 x 2 instantiations
    const auto by_layout = [&](auto b, auto stored) {
        constexpr int NB = decltype(b)::value;
        using Stored = typename decltype(stored)::type;
        if (sparse) launch(baked_resample_kernel<NB, Stored, true>, stored);
        else launch(baked_resample_kernel<NB, Stored, false>, stored);
    };
    const auto by_storage = [&](auto b) {
        if (storage_half) by_layout(b, BakedType<Half4>{});
        else by_layout(b, BakedType<float4>{});
    };
    if (B == 1) by_storage(std::integral_constant<int, 1>{});
    else if (B == 4) by_storage(std::integral_constant<int, 4>{});
    else by_storage(std::integral_constant<int, 9>{});
    return pnr_check_launch(entry);
}
