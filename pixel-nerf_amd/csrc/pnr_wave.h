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

}  // namespace pnr
