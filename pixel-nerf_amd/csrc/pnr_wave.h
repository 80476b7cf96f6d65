// pnr_wave.h -- reductions and inclusive scans across the 64 lanes of a wavefront (shuffles, no LDS).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

namespace pnr {

// butterfly sum: every lane ends with the total
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// inclusive scans: lane l ends with v_0 (+|*) ... (+|*) v_l
template <typename T> __device__ __forceinline__ T wave_scan_add(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ float wave_scan_mul(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v *= t;
    }
    return v;
}

// reverse inclusive scan of affine maps f_l(S) = b_l + m_l S under composition: lane l ends with (m, b) of
// f_l o f_{l+1} o ... o f_63 (f_63 applied first).  (m1, b1) o (m2, b2) = (m1 m2, b1 + m1 b2) is associative, so the
// suffix recurrence S_{l-1} = b_l + m_l S_l becomes S_{l-1} = b + m S_63 with no division and no subtraction of sums.
__device__ __forceinline__ void wave_rscan_affine(float &m, float &b, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float mt = __shfl_down(m, o, 64), bt = __shfl_down(b, o, 64);
        if (lane + o < 64) {
            b += m * bt;
            m *= mt;
        }
    }
}

// wave_scan_mul and wave_rscan_affine on doubles: the same lanes in the same order.  Every product and sum is rounded on its own
// (the fp32 twins above leave contraction to the compiler; the ray gradients of the baked march state their operations).  The
// pragma stands inside each body, so including this header changes nothing for the text after the include.
__device__ __forceinline__ double wave_scan_mul64(double v, int lane) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o, 64);
        if (lane >= o) v *= t;
    }
    return v;
}
__device__ __forceinline__ void wave_rscan_affine64(double &m, double &b, int lane) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double mt = __shfl_down(m, o, 64), bt = __shfl_down(b, o, 64);
        if (lane + o < 64) {
            b += m * bt;
            m *= mt;
        }
    }
}

}  // namespace pnr
