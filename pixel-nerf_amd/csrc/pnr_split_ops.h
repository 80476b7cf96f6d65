// pnr_split_ops.h -- what the split-operand kernels share (gfx950): the forward network (pnr_split.hip, eval_split_kernel, its
// 32x32x16 core) and the data-gradient chain behind it (pnr_bwd_split.hip, bwd_split_kernel).  Every operand is a (head, tail)
// pair of f16 values, w = wh + wl, and a product is three MFMAs (pnr_split.hip's header has the arithmetic):
//   SplitTileT   the LDS map: two activation images, two lin_in operand images, corner metadata, lin_out partials
//   SplitRing    the weight ring over a (head, tail) pair of packed streams, its cursor policies SplitAdvFwd / SplitAdvBwd
//   gemm_split   the tile GEMM from a pair of images, with its pinned issue order
//   split8, write_split   fp32 values -> (head, tail), accumulator set -> the two images
#pragma once
#include <hip/hip_runtime.h>

#include "pnr_common.h"
#include "pnr_device.h"
#include "pnr_layout.h"

namespace pnr {

typedef Prec<PNR_PREC_F16> PH;
typedef PH::T8 h8;

// The split kernels are generic in the wave count (stage_own, gemm_split_rot, the geometry loop, the own-K packing: IT = 4, BODIES = 2
// at NW = 4), but only the 8-wave form is parity-tested; the 4-wave build exists for timing (profiles/r05_split_gemm_ubench.txt: -13 %)
// and has to ask for itself.
#if !defined(PNR_VARIANT)
static_assert(NW == 8, "split-operand kernels: the product build is 8 waves per workgroup (other wave counts: variant builds, timing only)");
#endif

// LDS map: two activation images (head / tail), two lin_in operand images, corner metadata, lin_out partials.
// The fp32 table rows (2 KiB + 16 B pad per point) are looked up into the space of the two activation images
// while those are free (tile start, and after fc_1 of blocks 0-1 has finished reading).
template <int MT_> struct SplitTileT {
    static_assert(MT_ == 64, "64-point tiles");
    static constexpr int MT = MT_, JT = MT_ / 32;
    static constexpr int A_HI = 0;
    static constexpr int A_LO = MT * ROW_ACT;             // 66,560 (64)
    static constexpr int LDS_IN = 2 * MT * ROW_ACT;        // 133,120 (head image of the lin_in operand)
    static constexpr int IN_LO_DELTA = MT * ROW_IN;        // tail image right behind it
    static constexpr int LDS_META = LDS_IN + 2 * MT * ROW_IN;
    static constexpr int LDS_OUT = LDS_META + MT * 32;
    static constexpr int LDS_TOTAL = LDS_OUT + NW * MT * 16;  // 161,792 B
    static constexpr int ROW_TAB = D_HID * 4 + 16;          // fp32 table row: 2064 B (129 16-B slots: conflict-free)
    static constexpr int LDS_Z = 0;                         // (geometry_item only needs LDS_IN / LDS_META)
    static_assert(MT * ROW_TAB <= LDS_IN, "table image must fit in the space of the two activation images");
    static_assert(LDS_TOTAL <= 160 * 1024, "LDS budget");
};

struct SplitRing {
    h8 h[4][IT], l[4][IT];
    const char *base_h, *base_l;  // this wave's head / tail stream + lane*16
    int pf_rs, pf_view;
};

// prefetch cursor: the per-view segment [0, RS_VIEW_END_F) is consumed NS times, then the pooled tail, then wrap
__device__ __forceinline__ void ring_advance(SplitRing &R, int NS) {
    int rs = R.pf_rs + 4, v = R.pf_view;
    if (rs == RS_VIEW_END_F && v + 1 < NS) { v += 1; rs = 0; }
    else if (rs == RS_TOTAL_F) { rs = 0; v = 0; }
    R.pf_rs = rs; R.pf_view = v;
}

// the fp32-class BACKWARD chain (bwd_split_kernel, pnr_bwd_split.hip) walks a transposed stream in the layout of pnr_layout.h's backward
// stream: pooled head [0, BRS_HEAD_END) once, then the per-view segment [BRS_HEAD_END, BSRS_TOTAL) NS times, then wrap
// (lin_out^T, fc_1[4]^T fc_0[4]^T fc_1[3]^T fc_0[3]^T | fc_1[2]^T ... fc_0[0]^T, lin_z[2]^T lin_z[1]^T lin_z[0]^T, lin_in^T)
constexpr int BSRS_TOTAL = BRS_TOTAL;  // 424
static_assert(BSRS_TOTAL % 4 == 0, "ring depth 4 needs aligned segments");
constexpr size_t BSPACKED_BYTES = (size_t)BSRS_TOTAL * IT * 1024 * NW;  // one blob (head or tail): 5,308,416 B
struct SplitAdvFwd {
    static __device__ __forceinline__ void step(SplitRing &R, int NS) { ring_advance(R, NS); }
};
struct SplitAdvBwd {
    static __device__ __forceinline__ void step(SplitRing &R, int NS) {
        int rs = R.pf_rs + 4, v = R.pf_view;
        if (rs == BSRS_TOTAL) {
            if (v + 1 < NS) { v += 1; rs = BRS_HEAD_END; }
            else { rs = 0; v = 0; }
        }
        R.pf_rs = rs; R.pf_view = v;
    }
};

__device__ __forceinline__ f32x16 mf(h8 a, h8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// acc[it][jt] += (Wh + Wl)(Xh + Xl) without the tail-tail term; B rows at bhi0 + jt*jstride (+ lo_delta for the tails)
template <int JT, typename ADV = SplitAdvFwd>
__device__ __forceinline__ void gemm_split(f32x16 (&acc)[IT][JT], const char *smem, uint32_t bhi0, uint32_t jstride,
                                           uint32_t lo_delta, int nbody, SplitRing &R, int NS) {
    h8 bh[2][JT], bl[2][JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        bh[0][jt] = lds8<PH>(smem, bhi0 + jt * jstride);
        bl[0][jt] = lds8<PH>(smem, bhi0 + jt * jstride + lo_delta);
    }
#pragma unroll 1
    for (int body = 0; body < nbody; ++body) {
        const size_t pf = (size_t)R.pf_rs * (IT * 1024);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cur = j & 1;
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                bh[cur ^ 1][jt] = lds8<PH>(smem, bhi0 + jt * jstride + (j + 1) * 32);
                bl[cur ^ 1][jt] = lds8<PH>(smem, bhi0 + jt * jstride + lo_delta + (j + 1) * 32);
            }
            h8 ah[IT], al[IT];
#pragma unroll
            for (int it = 0; it < IT; ++it) { ah[it] = R.h[j][it]; al[it] = R.l[j][it]; }
            // the three products of one accumulator are spread over the step so that consecutive MFMAs are independent
#pragma unroll
            for (int it = 0; it < IT; ++it)
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) acc[it][jt] = mf(ah[it], bh[cur][jt], acc[it][jt]);
#pragma unroll
            for (int it = 0; it < IT; ++it)
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) acc[it][jt] = mf(ah[it], bl[cur][jt], acc[it][jt]);
#pragma unroll
            for (int it = 0; it < IT; ++it)
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) acc[it][jt] = mf(al[it], bh[cur][jt], acc[it][jt]);
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                R.h[j][it] = gload8<PH>(R.base_h + pf + j * (IT * 1024) + it * 1024);
                R.l[j][it] = gload8<PH>(R.base_l + pf + j * (IT * 1024) + it * 1024);
            }
            // Issue order of one k-step, pinned (round 3): hipcc batches the 16 refills of a loop body behind its last MFMA and
            // clusters the LDS reads; here every LDS read of the next step's B fragments follows ONE MFMA and every weight
            // refill follows TWO -- (M L) x 2JT, (M M G) x 2IT.  Same-box A/B on sn64 / srn_car / DTU: +2.7 ... +6 % in four
            // runs (profiles/r03_split_kernel_ab.txt, which also lists the eleven other orders tried: -6 ... +4 %; the order
            // matters here, unlike in the f16 kernel where the same kind of pinning measured -1.9 %).  Results unchanged.
#pragma unroll
            for (int i = 0; i < 2 * JT; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 LDS read
            }
#pragma unroll
            for (int i = 0; i < 2 * IT; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // 2 MFMAs
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
            }
            if constexpr (3 * IT * JT - 2 * JT - 4 * IT > 0) __builtin_amdgcn_sched_group_barrier(0x008, 3 * IT * JT - 2 * JT - 4 * IT, 0);
        }
        bhi0 += 128;
        ADV::step(R, NS);
    }
}

// head / tail of 8 fp32 values (optionally through relu); MODE.FP16_OVFL is set: heads saturate at 65504.
// tail = f16(v - head): one v_fma_mix{lo,hi}_f16 per value (fp32 FMA of the f16 head taken straight out of its packed
// register, times -1, plus v; result rounded once to f16) -- the same bits as convert-back + subtract + convert
// (v - head is exact in fp32), 5 VALU operations per pair instead of 8.
// GUARD: `amax` (a packed f16 pair) follows the largest HEAD produced, one v_pk_maximum3_f16 per FOUR values (gfx950; the
// IEEE-2019 maximum: a NaN head sticks): the fp16-range guard (PnrSplitAux.sat_flag).  Half the VALU cost of following the
// fp32 inputs with v_max3_f32 (round 5), which is what lets the guard run on every inference call (round 6).  Heads are >= 0
// behind the relu, so no magnitudes are needed; a head of 65504 means v >= 65488 (round to nearest): the guard fires 16 below
// the exact saturation point.
template <bool RELU, bool GUARD = false>
__device__ __forceinline__ void split8(const float (&v)[8], h8 &hi, h8 &lo, [[maybe_unused]] uint32_t *amax = nullptr) {
    static_assert(RELU || !GUARD, "the guard follows relu'd heads");
    u32x4 uh, ul;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f32x2 p = {v[2 * k], v[2 * k + 1]};
        if (RELU) {
            // one v_med3_f32 per value: median(v, 0, FLT_MAX) = max(v, 0) for every finite v (the head saturates at 65504 anyway;
            // with +inf as the upper bound LLVM folds the median back into the two-instruction maxnum).  NOT an inline-asm
            // v_max_f32: the accumulators come straight out of the MFMA pipe and hipcc does not place the MFMA -> VALU wait
            // states in front of inline asm -- that form read stale registers in the multi-view instantiations.
            p[0] = __builtin_amdgcn_fmed3f(p[0], 0.f, 3.402823466e38f); p[1] = __builtin_amdgcn_fmed3f(p[1], 0.f, 3.402823466e38f);
        }
        const f16x2 h = __builtin_convertvector(p, f16x2);
        uh[k] = __builtin_bit_cast(uint32_t, h);
        uint32_t l;
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l) : "v"(uh[k]), "v"(p[0]));
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(uh[k]), "v"(p[1]));
        ul[k] = l;
    }
    if constexpr (GUARD) {  // (the operands are v_cvt_pk results, never straight MFMA outputs: inline asm is safe here)
        uint32_t m = *amax;
        asm("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(m) : "v"(uh[0]), "v"(uh[1]));
        asm("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(m) : "v"(uh[2]), "v"(uh[3]));
        *amax = m;
    }
    hi = __builtin_bit_cast(h8, uh);
    lo = __builtin_bit_cast(h8, ul);
}

// [relu](acc) -> head / tail images (storage order, like write_act)
template <typename ST, bool RELU = true, int JT>
__device__ __forceinline__ void write_split(const f32x16 (&acc)[IT][JT], char *smem, uint32_t waddr) {
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const f32x16 &a = acc[it][jt];
            const uint32_t ad = waddr + jt * 32 * ROW_ACT + it * 64;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = a[8 * half + e];
                h8 hi, lo;
                split8<RELU>(v, hi, lo);
                *reinterpret_cast<h8 *>(smem + ST::A_HI + ad + 16 * half) = hi;
                *reinterpret_cast<h8 *>(smem + ST::A_LO + ad + 16 * half) = lo;
            }
        }
}

}  // namespace pnr
