// pnr_split.hip -- the fused per-point network at fp32-class accuracy on the f16 matrix cores (gfx950).
//
// fp32 MFMA peaks at 157 TFLOP/s on MI355X, 1/16 of the f16 rate; an fp32 product, however, is recovered from
// three f16 products when both operands are split into a rounded-to-f16 head and an f16 tail,
//       w = wh + wl,  x = xh + xl :   w x ~= wh xh + wh xl + wl xh        (the dropped wl xl is <= 2^-22 |w x|),
// each product exact in the fp32 accumulator (11 x 11 significand bits).  The representation itself is ~19 bits for the
// weights, not 22: the tail of a typical |w| ~ 0.05 weight (|w - wh| <= 1.5e-5 < 6.1e-5) lies in the fp16 SUBNORMAL range and
// carries ~8 bits.  Measured per-point error against the reference's fp32 outputs: 1.2-1.9e-6 (bar 2e-5).  This kernel runs the SAME fused chain
// as pnr_mlp.hip -- residual stream in the accumulators, weights streamed L2 -> VGPR, activations through LDS,
// lin_z folded into per-texel tables (fp32 tables here) -- with every operand carried as such a pair:
//   weights      two packed streams (head, tail) with the layout of the 16-bit folded stream   (pnr_pack_mlp_split)
//   activations  two LDS images (head, tail); relu(v) -> h = f16(v), l = f16(v - h)
//   tables       fp32 rows, bilinear blend in fp32, added to the accumulators as they are       (pnr_fold_latent_f32)
// 3 MFMAs per (weight fragment, activation fragment) instead of 1, 2x the operand bytes: ~1/3 of the f16 kernel's
// rate, several times the fp32-MFMA ceiling, at the accuracy class of the reference's own fp32 arithmetic
// (tests/test_hip_split.py holds it to the bars of tests/test_hip_f32.py: per-point |rgb| <= 2e-5).
// Folded form; 64-point tiles (several source views: the view sum parked in a per-workgroup scratch).  The unfused fp32-MFMA
// path (pnr_f32.hip) remains the implementation-independent yardstick.
//
// Round 4: every 512-wide linear starts with the products against the wave's OWN 64 features, taken from its accumulators (they
// are B fragments as they are), while the same fragments go to the operand images for the other waves: stage_own / gemm_split_rot.
//
// Round 7: two MFMA cores behind one kernel body.  The INFERENCE instantiations (TRAIN = false) run every product on
// v_mfma_f32_16x16x32_f16 (4 x 4 tiles of 16 features x 16 points per wave; "the 16x16x32 core" below), the training forward keeps
// v_mfma_f32_32x32x16_f16 with its masks and dumps, bit for bit.  Same arithmetic, same packed streams, same bias / table layout;
// the chip holds 1.99 GHz under the new core against 1.88 GHz under the old one and needs 3 % fewer cycles: sn64 +9.9 %, srn_car
// +6.8 %, DTU +7.4 % same-box (profiles/r07_split_kernel_ab.txt).
//
// The kernel of this file:
//   eval_split_kernel<RAYS, MV, TIMING, TRAIN, GUARD, SC>   the fused network (SC: the stream-scale / range-probe forms, below).  GUARD = the fp16-range guard (PnrSplitAux.sat_flag): the
//                                                same bits, plus one flag bit per layer whose operand image received a value >= 65504.
//                                                TRAIN = the fp32-class TRAINING forward: the same launch also
//                                                copies every wide linear's (head, tail) operand image out of LDS (relu(x) /
//                                                relu(net): the operands of the weight gradients), writes 1-bit relu masks and
//                                                the stream in front of lin_out; the inference instantiations compile to the
//                                                code they had before the flag existed.
// What it shares with the data-gradient chain behind it (bwd_split_kernel, pnr_bwd_split.hip) -- the LDS map, the ring, the
// 32x32x16 GEMM, the (head, tail) split -- is pnr_split_ops.h.  The weight gradients over the dumped images are dw_split_kernel
// (pnr_bwd.hip); host side of the training path: pnr_f32.hip (pnr_*_split_train).
#include <hip/hip_runtime.h>

#include "pnr_common.h"
#include "pnr_device.h"
#include "pnr_entry.h"
#include "pnr_internal.h"
#include "pnr_layout.h"
#include "pnr_split_ops.h"

namespace pnr {

// ---- "own K block first" form of the 512 x 512 linears (round 4) -----------------------------------------------------------
// A wave's accumulators ARE B fragments of the next linear: lane (point pl, half h) holds, in registers 8 rr .. 8 rr + 7 of
// feature tile `it`, exactly the 8 K-elements an MFMA B operand wants from that lane for the 16 features
// feat_of(wv IT + it, {0,1}, 8 rr + {0..7}) (the property lin_out has always used).  So the next GEMM's products against THIS
// wave's 64 features need no LDS round trip and no barrier: relu + (head, tail) split of 16 accumulator values yields the B
// fragments of one k-step, which are multiplied right away (12 MFMAs) AND stored into the operand images for the other seven
// waves.  The split epilogue (VALU-bound: ~170 operations per wave and GEMM, 8 % of a tile with the matrix pipe idle) thereby
// runs in the shadow of 48 MFMAs per wave that had to be issued anyway, and the barrier that publishes the images is crossed
// with an eighth of the GEMM already done.  The packed stream carries each wave's own K block first, in register order, then
// the blocks of waves wv+1 .. wv+7 (mod 8) in the image's storage order (pnr_pack.hip, OWNK).  Per output element the 512
// products are summed in a wave-dependent block order -- fixed per (feature, wave), identical for every point and tile size:
// chunked = whole and sharded = unsharded stay bit for bit.
struct NoMark { __device__ __forceinline__ void operator()(int) const {} };
// MARK: the TIMING instantiation's clock (sub-phases PH_OWN_PROLOGUE / PH_OWN_KSTEPS); a no-op everywhere else
template <typename ST, int JT, bool GUARD, typename MARK = NoMark>
__device__ __forceinline__ void stage_own(f32x16 (&acc)[IT][JT], const f32x16 (&src)[IT][JT], char *smem, uint32_t waddr,
                                          SplitRing &R, int NS, [[maybe_unused]] uint32_t *amax, MARK mark = MARK()) {
    // k-step jj of the own block = (feature tile jj >> 1, register half jj & 1); 2 IT k-steps = IT / 2 ring bodies of 4
    static_assert(IT % 2 == 0, "whole ring bodies");
    h8 bh[2][JT], bl[2][JT];
    auto make = [&](int jj, int buf) {
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = src[jj >> 1][jt][8 * (jj & 1) + e];
            split8<true, GUARD>(v, bh[buf][jt], bl[buf][jt], amax);
        }
    };
    make(0, 0);
    mark(PH_OWN_PROLOGUE);  // accumulator drain + the first k-step's split
#pragma unroll
    for (int body = 0; body < IT / 2; ++body) {
        const size_t pf = (size_t)R.pf_rs * (IT * 1024);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int jj = body * 4 + j;
            const int cur = jj & 1;
            if (jj + 1 < 2 * IT) make(jj + 1, cur ^ 1);
            h8 ah[IT], al[IT];
#pragma unroll
            for (int it = 0; it < IT; ++it) { ah[it] = R.h[j][it]; al[it] = R.l[j][it]; }
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
            // the same fragments, for the other waves: storage position of (feature tile jj >> 1, register half jj & 1), as write_split
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                const uint32_t ad = waddr + jt * 32 * ROW_ACT + (jj >> 1) * 64 + 16 * (jj & 1);
                *reinterpret_cast<h8 *>(smem + ST::A_HI + ad) = bh[cur][jt];
                *reinterpret_cast<h8 *>(smem + ST::A_LO + ad) = bl[cur][jt];
            }
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                R.h[j][it] = gload8<PH>(R.base_h + pf + j * (IT * 1024) + it * 1024);
                R.l[j][it] = gload8<PH>(R.base_l + pf + j * (IT * 1024) + it * 1024);
            }
            // issue order of one k-step, pinned: the split of the NEXT k-step's 16 values (~40 VALU) is spread over this step's
            // MFMAs, the image stores and the ring refills of THIS step sit behind its later MFMAs -- left to itself hipcc puts
            // all refills behind the stage's last MFMA and runs the last MFMAs back to back with the VALU work in front of them
            if constexpr (IT == 2) {
#pragma unroll
                for (int i = 0; i < 3 * IT * JT; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                          // up to 4 VALU
                    if (i >= 4 && i % 2 == 0) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // 1 LDS write  (i = 4, 6, 8, 10)
                    if (i >= 5 && i % 2 == 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read  (i = 5, 7, 9, 11)
                }
            } else {
                // 3 IT JT MFMAs, 2 JT image stores, 2 IT refills, ~20 JT VALU of the next k-step's split
                constexpr int NM = 3 * IT * JT;
#pragma unroll
                for (int i = 0; i < NM; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                    if (i >= 4 && i < 4 + 2 * JT) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                    if (i >= NM - 2 * IT - 2 && i < NM - 2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
            }
        }
        ring_advance(R, NS);
    }
    mark(PH_OWN_KSTEPS);
}

// the other seven K blocks of the same linear, from the operand images: blocks (wv + 1) .. (wv + 7) mod 8, the order the stream
// carries them in.  Loop body and pinned issue order of gemm_split.
template <int JT>
__device__ __forceinline__ void gemm_split_rot(f32x16 (&acc)[IT][JT], const char *smem, uint32_t a_rd0, uint32_t jstride,
                                               uint32_t lo_delta, int wv, SplitRing &R, int NS) {
    constexpr int BLK = SL * 2;         // bytes of one wave's K block in an image row (128 at 8 waves)
    constexpr int BODIES = SL / 64;     // ring bodies (4 k-steps of 16) per block
    h8 bh[2][JT], bl[2][JT];
    uint32_t bhi0 = a_rd0 + (uint32_t)((wv + 1) & (NW - 1)) * BLK;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        bh[0][jt] = lds8<PH>(smem, bhi0 + jt * jstride);
        bl[0][jt] = lds8<PH>(smem, bhi0 + jt * jstride + lo_delta);
    }
#pragma unroll 1
    for (int mb = 2 * BODIES; mb < (NW + 1) * BODIES; ++mb) {   // body index counted in ring bodies: block m = mb / BODIES
        const int m = mb / BODIES, sub = mb % BODIES;
        // after this body's last k-step: the next 64 K of the same block, or the start of the next block
        // (after the last block: this wave's own, read and dropped)
        const uint32_t nxt = sub + 1 < BODIES ? bhi0 + 128 : a_rd0 + (uint32_t)((wv + m) & (NW - 1)) * BLK;
        const size_t pf = (size_t)R.pf_rs * (IT * 1024);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cur = j & 1;
            const uint32_t rd = j < 3 ? bhi0 + (j + 1) * 32 : nxt;
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                bh[cur ^ 1][jt] = lds8<PH>(smem, rd + jt * jstride);
                bl[cur ^ 1][jt] = lds8<PH>(smem, rd + jt * jstride + lo_delta);
            }
            h8 ah[IT], al[IT];
#pragma unroll
            for (int it = 0; it < IT; ++it) { ah[it] = R.h[j][it]; al[it] = R.l[j][it]; }
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
            constexpr int NM = 3 * IT * JT, PER = (NM - 2 * JT) / (2 * IT);
#pragma unroll
            for (int i = 0; i < 2 * JT; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 LDS read
            }
#pragma unroll
            for (int i = 0; i < 2 * IT; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);  // PER MFMAs (2 at IT = JT = 2)
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);    // 1 VMEM read
            }
            if constexpr (NM - 2 * JT - PER * 2 * IT > 0) __builtin_amdgcn_sched_group_barrier(0x008, NM - 2 * JT - PER * 2 * IT, 0);
        }
        bhi0 = nxt;
        ring_advance(R, NS);
    }
}

// fp32 bilinear lookup of table b: wave handles points wave*8..+7; lane handles storage slots 4*lane..+3 and 256 + 4*lane..+3
// (two fully coalesced 1 KiB loads per corner, and two 16-byte LDS writes per point at a 16-byte lane stride -- a 32-byte
// lane stride put lanes l and l+8 on the same banks: 5.9 % of the LDS cycles of the round-2 kernel were conflicts);
// rows land in the table image (ROW_TAB stride) at offset 0
template <int GB, typename ST>
__device__ __forceinline__ void gather_table_f32(const EvalParams &q, char *smem, int wv, int lane, int b) {
    static_assert(GB == 2, "pairs of consecutive points");
    const float *tab = reinterpret_cast<const float *>(q.tables) + (size_t)b * q.table_stride + lane * 4;
    // A wave's 8 points are consecutive samples of ONE ray (tiles never straddle rays: K is a multiple of the tile), and consecutive
    // samples mostly fall into the same cell of the feature grid (sn64: 4-12 samples per texel): a point whose four corner offsets
    // equal its predecessor's re-uses the predecessor's rows from registers instead of loading 8 KiB again.  The comparison is
    // wave-uniform (every lane reads the same META words), the arithmetic per point is unchanged (same rows, same order).
    // Same-box A/B against loading every point's rows (profiles/r04_split_kernel_ab.txt, session 9): lookups 30.2 k -> 19.7 k
    // cycles per tile; sn64 +1.1 %, srn_car +3.4 %, DTU +2.0 %.
    // (Wave-per-point, lanes along the channels: whole 1 KiB pieces of a row per instruction.  The LDS-free alternative -- every lane
    // reading the 64 bytes of its own point's row that hold its own 16 features, blended straight into the accumulators, no barrier
    // pair -- measured -2.4 % on sn64 / srn_car and -11.7 % on DTU: eight waves then fetch eight slices of every row at eight
    // different times.  profiles/r05_split_kernel_ab.txt.)
    // (The rows are ordinary, L2-allocating loads on purpose: neighbouring points and tiles hit the same texels.  Non-temporal loads
    // measured -3 % on sn64, -5 % on srn_car, -11 % on DTU, same box: profiles/r05_split_kernel_ab.txt.)
    f32x4 v[GB][4][2];
    uint32_t last[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};  // offsets of the rows held in v[1]
#pragma unroll 1
    for (int i = 0; i < ST::MT / NW; i += GB) {
        f32x4 w[GB];
        uint32_t off[GB][4];
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            const int p = wv * (ST::MT / NW) + i + u;
            const u32x4 o = *reinterpret_cast<const u32x4 *>(smem + ST::LDS_META + p * 32);
            w[u] = *reinterpret_cast<const f32x4 *>(smem + ST::LDS_META + p * 32 + 16);
#pragma unroll
            for (int c = 0; c < 4; ++c) off[u][c] = __builtin_amdgcn_readfirstlane(o[c]);
        }
        const bool keep0 = off[0][0] == last[0] && off[0][1] == last[1] && off[0][2] == last[2] && off[0][3] == last[3];
        const bool keep1 = off[1][0] == off[0][0] && off[1][1] == off[0][1] && off[1][2] == off[0][2] && off[1][3] == off[0][3];
        if (keep0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { v[0][c][0] = v[1][c][0]; v[0][c][1] = v[1][c][1]; }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[0][c][0] = *reinterpret_cast<const f32x4 *>(tab + off[0][c]);
                v[0][c][1] = *reinterpret_cast<const f32x4 *>(tab + off[0][c] + D_HID / 2);
            }
        }
        if (keep1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { v[1][c][0] = v[0][c][0]; v[1][c][1] = v[0][c][1]; }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[1][c][0] = *reinterpret_cast<const f32x4 *>(tab + off[1][c]);
                v[1][c][1] = *reinterpret_cast<const f32x4 *>(tab + off[1][c] + D_HID / 2);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) last[c] = off[1][c];
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            const int p = wv * (ST::MT / NW) + i + u;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                f32x4 r = v[u][0][hh] * w[u][0];
                r += v[u][1][hh] * w[u][1];
                r += v[u][2][hh] * w[u][2];
                r += v[u][3][hh] * w[u][3];
                *reinterpret_cast<f32x4 *>(smem + p * ST::ROW_TAB + hh * (D_HID * 2) + lane * 16) = r;
            }
        }
    }
}

// x += this lane's slots of the fp32 table rows (SCALED: x += c * t, one FMA: the stream is carried at c = 2^-s, the tables are not)
template <typename ST, bool SCALED = false, int JT>
__device__ __forceinline__ void add_from_table(f32x16 (&x)[IT][JT], const char *smem, int pl, int h, int wv, [[maybe_unused]] float c = 1.f) {
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const char *row = smem + (jt * 32 + pl) * ST::ROW_TAB + ((wv * IT + it) * 32 + h * 16) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 t = *reinterpret_cast<const f32x4 *>(row + 16 * k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (SCALED) x[it][jt][4 * k + e] = __builtin_fmaf(c, t[e], x[it][jt][4 * k + e]);
                    else x[it][jt][4 * k + e] += t[e];
                }
            }
        }
}

// ---- the 16x16x32 core of the INFERENCE instantiations (round 7) -------------------------------------------------------------
// The kernel is power-limited and the chip holds a higher clock on v_mfma_f32_16x16x32_f16 than on 32x32x16 at equal cycles per
// FLOP (tools/ubench/split_gemm.hip, profiles/r07_split_gemm_16x16x32.txt: the GEMM loop of this kernel x1.16 by wall).  Same
// footprint: 8 waves x 64 features x 64 points, x + net = 128 accumulators, 16 KiB of weight ring per wave; the images, tables and
// biases keep their storage order (pnr_layout.h, slot16).  Lane (c = l & 15, g = l >> 4); accumulator (t, jt) = 16 features x 16
// points; one ring step = one K = 32 step = 4 A fragments per blob, ring of 2; the B fragment pair of ONE point tile is fetched
// just in time (two pairs in rotation: 16 registers, each pair feeds 12 MFMAs) -- a whole K-step of B, double-buffered, spills.
// The A fragments are 16-byte pieces of the SAME packed streams the 32x32x16 core reads, addressed per lane (pnr_layout.h,
// a16_lane_off): one blob, one pack, nothing new on the host side.
// The TRAIN instantiations keep the 32x32x16 core above, its masks and dumps.
struct SplitRing16 {
    h8 h[2][NT16], l[2][NT16];
    const char *base_h, *base_l;  // this wave's head / tail stream
    uint32_t off_gen, off_own;    // this lane's piece inside a K = 32 step: image K order / the own block's register K order
    int pf_rs, pf_view;           // prefetch cursor in K = 32 steps
};
// byte offset of the cursor's step for this lane: the first two steps of every 512-wide linear are the wave's own block
__device__ __forceinline__ size_t ring_pf16(const SplitRing16 &R) {
    const int r = R.pf_rs - KS16_IN;
    const bool own = r >= 0 && R.pf_rs < RS16_TOTAL - KS16_OUT && (r & (KS16_BIG - 1)) == 0;
    return (size_t)R.pf_rs * RS16_BYTES + (own ? R.off_own : R.off_gen);
}
__device__ __forceinline__ void ring_advance16(SplitRing16 &R, int NS) {
    int rs = R.pf_rs + 2, v = R.pf_view;
    if (rs == RS16_VIEW_END && v + 1 < NS) { v += 1; rs = 0; }
    else if (rs == RS16_TOTAL) { rs = 0; v = 0; }
    R.pf_rs = rs; R.pf_view = v;
}
__device__ __forceinline__ f32x4 mf16(h8 a, h8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// the 12 MFMAs of one (K-step j, point tile jt): head x head, head x tail, tail x head, the four row tiles side by side
__device__ __forceinline__ void mfma12(f32x4 (&acc)[NT16][NJ16], int jt, const h8 (&ah)[NT16], const h8 (&al)[NT16], h8 bh, h8 bl) {
#pragma unroll
    for (int t = 0; t < NT16; ++t) acc[t][jt] = mf16(ah[t], bh, acc[t][jt]);
#pragma unroll
    for (int t = 0; t < NT16; ++t) acc[t][jt] = mf16(ah[t], bl, acc[t][jt]);
#pragma unroll
    for (int t = 0; t < NT16; ++t) acc[t][jt] = mf16(al[t], bh, acc[t][jt]);
}
__device__ __forceinline__ void refill16(SplitRing16 &R, int j, size_t pf) {
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
        R.h[j][t] = gload8<PH>(R.base_h + pf + j * RS16_BYTES + (t >> 1) * 1024 + (t & 1) * 128);
        R.l[j][t] = gload8<PH>(R.base_l + pf + j * RS16_BYTES + (t >> 1) * 1024 + (t & 1) * 128);
    }
}

// One ring body from an image: 2 K-steps x 4 point tiles, B fragments at base + 64 j + jt jstride (+ lo_delta for the tails);
// bh[0] / bl[0] hold the first pair on entry and the pair at `nxt` on exit.  Pinned issue order per point tile: (M L) x 2, then
// the other 10 MFMAs; a step's 8 refills ride on the last pass (tail x head, the last reader of a tile's fragments) of its last
// point tile, 2 per MFMA.
__device__ __forceinline__ void body16(f32x4 (&acc)[NT16][NJ16], const char *smem, h8 (&bh)[2], h8 (&bl)[2], uint32_t base,
                                       uint32_t jstride, uint32_t lo_delta, uint32_t nxt, SplitRing16 &R) {
    const size_t pf = ring_pf16(R);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int jt = 0; jt < NJ16; ++jt) {
            const int cur = (j * NJ16 + jt) & 1;
            const bool lastj = jt == NJ16 - 1;
            const uint32_t rd = lastj ? (j == 1 ? nxt : base + 64) : base + 64 * j + (jt + 1) * jstride;
            bh[cur ^ 1] = lds8<PH>(smem, rd);
            bl[cur ^ 1] = lds8<PH>(smem, rd + lo_delta);
            mfma12(acc, jt, R.h[j], R.l[j], bh[cur], bl[cur]);
            if (lastj) refill16(R, j, pf);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 LDS read
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (lastj) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * NT16 - 2, 0);
#pragma unroll
                for (int t = 0; t < NT16; ++t) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);  // 2 VMEM reads
                }
            } else {
                __builtin_amdgcn_sched_group_barrier(0x008, 3 * NT16 - 2, 0);
            }
        }
}

// lin_in: K = 64 = one ring body, B rows in the lin_in operand images
__device__ __forceinline__ void gemm_split16_in(f32x4 (&acc)[NT16][NJ16], const char *smem, uint32_t rd0, uint32_t jstride,
                                                uint32_t lo_delta, SplitRing16 &R, int NS) {
    h8 bh[2], bl[2];
    bh[0] = lds8<PH>(smem, rd0);
    bl[0] = lds8<PH>(smem, rd0 + lo_delta);
    body16(acc, smem, bh, bl, rd0, jstride, lo_delta, rd0, R);  // (after the last pair: the first again, read and dropped)
    ring_advance16(R, NS);
}

// stage_own on this core: K-step m of the wave's own block is, per point tile, registers 0..3 of accumulator tiles 2m and 2m + 1
// (pnr_layout.h, slot16_own_k): relu + (head, tail) split of those 8 values = the B fragment pair, multiplied at once (12 MFMAs)
// and stored -- the same 16 bytes the 32x32x16 core stores there -- to both images for the other seven waves.
template <typename ST, bool GUARD, typename MARK = NoMark>
__device__ __forceinline__ void stage_own16(f32x4 (&acc)[NT16][NJ16], const f32x4 (&src)[NT16][NJ16], char *smem, uint32_t waddr,
                                            SplitRing16 &R, int NS, [[maybe_unused]] uint32_t *amax, MARK mark = MARK()) {
    h8 bh[2], bl[2];
    auto make = [&](int q, int buf) {
        const int m = q / NJ16, jt = q % NJ16;
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = src[2 * m][jt][e]; v[4 + e] = src[2 * m + 1][jt][e]; }
        split8<true, GUARD>(v, bh[buf], bl[buf], amax);
    };
    make(0, 0);
    mark(PH_OWN_PROLOGUE);
    const size_t pf = ring_pf16(R);
#pragma unroll
    for (int q = 0; q < 2 * NJ16; ++q) {
        const int m = q / NJ16, jt = q % NJ16, cur = q & 1;
        const bool lastj = jt == NJ16 - 1;
        if (q + 1 < 2 * NJ16) make(q + 1, cur ^ 1);
        mfma12(acc, jt, R.h[m], R.l[m], bh[cur], bl[cur]);
        const uint32_t ad = waddr + jt * 16 * ROW_ACT + m * 64;
        *reinterpret_cast<h8 *>(smem + ST::A_HI + ad) = bh[cur];
        *reinterpret_cast<h8 *>(smem + ST::A_LO + ad) = bl[cur];
        if (lastj) refill16(R, m, pf);
        // pinned: the split of the NEXT pair (~24 VALU) spread under this pair's MFMAs, the two image stores behind the 5th and
        // the 7th, a step's refills behind the last four MFMAs of its last point tile
#pragma unroll
        for (int i = 0; i < 3 * NT16; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                   // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                                   // up to 3 VALU
            if (i == 4 || i == 6) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);             // 1 LDS write
            if (lastj && i >= 2 * NT16) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);       // 2 VMEM reads
        }
    }
    ring_advance16(R, NS);
    mark(PH_OWN_KSTEPS);
}

// the other seven K blocks, from the operand images: blocks (wv + 1) .. (wv + 7) mod 8, one ring body each
__device__ __forceinline__ void gemm_split_rot16(f32x4 (&acc)[NT16][NJ16], const char *smem, uint32_t a_rd0, uint32_t jstride,
                                                 uint32_t lo_delta, int wv, SplitRing16 &R, int NS) {
    static_assert(SL == 64, "one ring body per wave block");
    h8 bh[2], bl[2];
    uint32_t base = a_rd0 + (uint32_t)((wv + 1) & (NW - 1)) * 128;
    bh[0] = lds8<PH>(smem, base);
    bl[0] = lds8<PH>(smem, base + lo_delta);
#pragma unroll 1
    for (int m = 2; m <= NW; ++m) {  // (after the last block: this wave's own, read and dropped)
        const uint32_t nxt = a_rd0 + (uint32_t)((wv + m) & (NW - 1)) * 128;
        body16(acc, smem, bh, bl, base, jstride, lo_delta, nxt, R);
        base = nxt;
        ring_advance16(R, NS);
    }
}

template <bool INIT>
__device__ __forceinline__ void add_bias16(f32x4 (&acc)[NT16][NJ16], const float *bias_wave, int g, int slot) {
    // bias_wave = bias + wave * BIAS_FLOATS_PER_WAVE: the wave's 64 values of a slot in storage order
    const float *b = bias_wave + (size_t)slot * (NW * BIAS_FLOATS_PER_WAVE);
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(b + slot16(t, g, 0));
#pragma unroll
        for (int jt = 0; jt < NJ16; ++jt) {
            if (INIT) acc[t][jt] = v;
            else acc[t][jt] += v;
        }
    }
}

template <typename ST, bool SCALED = false>
__device__ __forceinline__ void add_from_table16(f32x4 (&x)[NT16][NJ16], const char *smem, int c, int g, int wv, [[maybe_unused]] float sc = 1.f) {
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
        for (int jt = 0; jt < NJ16; ++jt) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(smem + (jt * 16 + c) * ST::ROW_TAB + (wv * SL + slot16(t, g, 0)) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (SCALED) x[t][jt][e] = __builtin_fmaf(sc, v[e], x[t][jt][e]);
                else x[t][jt][e] += v[e];
            }
        }
}

// accumulator set, ring and tile counts of a core
template <bool M16> struct SplitCore {
    typedef f32x16 acc_t;
    typedef SplitRing ring_t;
    static constexpr int AI = IT, AJ = JT, AR = 16;
};
template <> struct SplitCore<true> {
    typedef f32x4 acc_t;
    typedef SplitRing16 ring_t;
    static constexpr int AI = NT16, AJ = NJ16, AR = 4;
};

// MV: views go through blocks 0-2 one after the other on the same 64 points; the running view sum (util.combine_interleaved,
// util.py:461-466) does not fit the registers next to x + net + the 64-register head/tail ring, so it is PARKED in a
// per-workgroup scratch (q.mv_ws, [slot][thread] layout: every lane re-reads only what it wrote itself, no synchronisation;
// 128 KiB per workgroup, L2-resident) and read-modify-written once per view and tile -- 256 KiB of traffic against the 6.6 MB
// of weights the same view streams.  (Round 2 ran multi-view scenes on 32-point tiles with the sum in registers: twice the
// weight stream per point, 105-147 k rays/s.)  Fixed summation order (view 0 + view 1) + ...: bit-identical to the
// in-register form.
//
// SC: the stream scale (PnrMlpWeights.stream_scale_log2 = s, word BOUT_SCALE_INDEX of the blob's tail).  SC = 0 is the kernel as
// it always was (blobs packed at s = 0: the same instructions).  SC = 1 carries x and net at c = 2^-s:
//   x *= c behind lin_in + table 0 | x += c t for tables 1, 2 | block biases arrive as c b (pack_bias_kernel) |
//   the lin_out partial sum times 2^(s - t) in front of lin_out's bias (t: the lift lin_out's weights were packed with, pnr_pack.hip)
// -- four fp32 sites, all exact; nothing stored as fp16 is shifted, the hidden weights are untouched, view pooling (mean and
// max) is homogeneous.  SC = 2: the same with the range probe (PnrSplitAux.range_probe): the fp32 values about to enter split8 -- the
// accumulator tiles a stage_own / lin_out is about to split -- are followed with v_max3_f32 in FRONT of the stage (relu'd: the
// running maximum starts at 0), the round-5 form of the guard; it says how far beyond the range a value went, which saturated
// heads cannot.  Per-layer maxima are collected in 12 LDS words behind the tile map (non-negative floats order like their bit
// patterns: ds_max_u32), one global atomic max per layer and workgroup at the end, in true units (times 2^s).  The stages
// themselves are the guarded scaled kernel's, instruction for instruction: the probe keeps the guard's bits and its result.
template <bool RAYS, bool MV, bool TIMING = false, bool TRAIN = false, bool GUARD = false, int SC = 0>
__global__ void __launch_bounds__(NTHREADS, NW / 4) eval_split_kernel(const EvalParams q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef SplitTileT<64> ST;
    constexpr bool PROBE = SC == 2;
    constexpr bool M16 = !TRAIN;  // the inference instantiations run the 16x16x32 core, the training forward the 32x32x16 core
    typedef SplitCore<M16> CORE;
    typedef typename CORE::acc_t acc_t;
    typedef typename CORE::ring_t ring_t;
    constexpr int AI = CORE::AI, AJ = CORE::AJ, AR = CORE::AR;  // accumulator tiles per wave and registers per tile
    static_assert(!(SC && (TRAIN || TIMING || !GUARD)), "the stream scale is an inference form, instantiated with the guard on");
    [[maybe_unused]] float sc_c = 1.f, sc_inv = 1.f, sc_out = 1.f;
    if constexpr (SC != 0) {
        const int s = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(q.bout)[BOUT_SCALE_INDEX]);
        const int t = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(q.bout)[BOUT_LIFT_INDEX]);
        sc_c = __builtin_bit_cast(float, (uint32_t)(127 - s) << 23);
        sc_inv = __builtin_bit_cast(float, (uint32_t)(127 + s) << 23);
        sc_out = __builtin_bit_cast(float, (uint32_t)(127 + s - t) << 23);  // s, t in [0, 30]
    }
    [[maybe_unused]] uint32_t *probe_lds = reinterpret_cast<uint32_t *>(smem + ST::LDS_TOTAL);
    if constexpr (PROBE) {
        if (threadIdx.x < PROBE_WORDS) probe_lds[threadIdx.x] = 0u;  // (published by the tile loop's first barrier)
    }
    constexpr int JT = ST::JT, MT = ST::MT;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // lane = (point pl, K half h) on the 32x32x16 core, (point pl, K group h) on the 16x16x32 core
    const int pl = M16 ? lane & 15 : lane & 31, h = M16 ? lane >> 4 : lane >> 5;
    const int NS = MV ? q.NS : 1;

    // 16x16x32 core: a ds_read_b128 is served in four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same
    // + 32 -- i.e. points {0-3, 12-15} of one K group next to points {4-11} of its neighbour; with 65 slots per row those two
    // runs of 8 slots overlap in one slot whatever the odd pad (2-way).  So rows 4..11 (mod 16) of the INFERENCE kernel's
    // activation images hold each pair of 16-byte chunks swapped: both runs then start at the same slot and tile the 16 slots.
    // SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE over the kernel: 0.415 plain, 0.186 swapped (what is left: the table and lin_in
    // reads and the image stores), 0.004 on the 32x32x16 core (profiles/r07_split_kernel_ab.txt, counter passes of their own).
    // Writer (stage_own16) and readers share `a_sw`; the images never leave this kernel (the training forward, which dumps them,
    // keeps the plain order, and so does every buffer another kernel or the host sees).
    const uint32_t a_sw = M16 ? ((uint32_t)(h ^ (((pl + 4) >> 3) & 1))) * 16 : h * 16;
    const uint32_t a_rd0 = ST::A_HI + pl * ROW_ACT + a_sw;
    const uint32_t in_rd0 = ST::LDS_IN + pl * ROW_IN + h * 16;
    const uint32_t a_wr = pl * ROW_ACT + wv * (SL * 2) + (M16 ? a_sw : h * 32);
    const float *bias_lane = q.bias + wv * BIAS_FLOATS_PER_WAVE + (M16 ? 0 : h * 16);

    f16_ovfl_mode<PH>();
    // static priority for the second-dispatched half of the workgroup (the arbitration loser of every segment when both waves of
    // a SIMD run at priority 0; MI355X_MICROARCH.md, "two waves per SIMD", item 4): one s_setprio before the main loop, no flips.
    // Same-box A/B: +0.9 % on sn64 / srn_car / DTU (profiles/r03_split_kernel_ab.txt).  Does not touch results.
    if (NW > 4 && wv >= NW / 2) __builtin_amdgcn_s_setprio(1);
    ring_t R;
    if constexpr (M16) {  // the same two blobs, pieces addressed for the 16x16x32 shape
        R.base_h = q.wstream + (size_t)wv * (RS_TOTAL_F * IT * 1024);
        R.base_l = R.base_h + PACKED_BYTES;
        R.off_gen = a16_lane_off(pl, h, false);
        R.off_own = a16_lane_off(pl, h, true);
        refill16(R, 0, R.off_gen);
        refill16(R, 1, R.off_gen);
        R.pf_rs = 2;
    } else {
        R.base_h = q.wstream + (size_t)wv * (RS_TOTAL_F * IT * 1024) + lane * 16;
        R.base_l = R.base_h + PACKED_BYTES;  // the tail blob follows the head blob (pnr_pack_mlp_split)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                R.h[j][it] = gload8<PH>(R.base_h + j * (IT * 1024) + it * 1024);
                R.l[j][it] = gload8<PH>(R.base_l + j * (IT * 1024) + it * 1024);
            }
        R.pf_rs = 4;
    }
    R.pf_view = 0;
    [[maybe_unused]] unsigned long long *tim = q.tim;
    [[maybe_unused]] unsigned long long tlast = TIMING ? __builtin_readcyclecounter() : 0ull;

    // TRAIN: an accumulator tile set leaves as fp32 rows in natural feature order (D register r of tile (it, jt) = feature
    // 64 wv + 32 it + (r&3) + 8 (r>>2) + 4 h of point 32 jt + pl): 16-byte pieces, `rows` = first row of the tile in dst
    [[maybe_unused]] auto dump_rows = [&](const f32x16 (&a)[IT][JT], float *dst, long long rows, long long rows_left) {
        float *d = dst + ((size_t)rows + pl) * D_HID + (wv * IT) * 32 + 4 * h;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            if (jt * 32 + pl >= rows_left) continue;
#pragma unroll
            for (int it = 0; it < IT; ++it)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f32x4 v = {a[it][jt][4 * k], a[it][jt][4 * k + 1], a[it][jt][4 * k + 2], a[it][jt][4 * k + 3]};
                    __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(d + (size_t)jt * 32 * D_HID + it * 32 + 8 * k));  // streamed past the L2 (dump_image)
                }
        }
    };
    // TRAIN: where the current tile's rows live (set by the tile / view loops; the inference instantiations never touch them)
    [[maybe_unused]] long long tr_rows_view = 0, tr_rows_pooled = 0, tr_rows_left = 0;
    // TRAIN: relu masks for the fused backward chain, one 64-bit word per thread and layer in the layout of the 16-bit training
    // kernels (pnr_device.h: bit (it JT + jt) 16 + r = "register r of accumulator tile (it, jt) is positive"; layer 2b = x
    // entering block b, 2b + 1 = its fc_0 output, 10 = the stream in front of lin_out; [layer][view][tile][thread])
    [[maybe_unused]] size_t tr_mask_view = 0, tr_mask_pooled = 0;
    [[maybe_unused]] const size_t tr_mask_layer = (size_t)NS * (size_t)q.ntiles * NTHREADS;
    [[maybe_unused]] auto put_mask = [&](const f32x16 (&a)[IT][JT], int layer, size_t word) {
        unsigned long long m = 0ull;
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                uint32_t m16 = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) m16 |= (a[it][jt][r] > 0.f ? 1u : 0u) << r;
                m |= (unsigned long long)m16 << ((it * JT + jt) * 16);
            }
        __builtin_nontemporal_store(m, q.d_mask + (size_t)layer * tr_mask_layer + word);
    };
    // TRAIN: the operand images just published (head, tail) -> their 16-bit row sets, whole 1 KiB rows per wave instruction
    [[maybe_unused]] auto dump_pair = [&](char *head, int b) {
        const long long rows = b < COMBINE_LAYER ? tr_rows_view : tr_rows_pooled;
        const size_t total = (size_t)(b < COMBINE_LAYER ? (long long)NS * q.P : q.P) * (D_HID * 2);
        dump_image<MT>(smem, ST::A_HI, head + (size_t)rows * (D_HID * 2), tr_rows_left, wv, lane);
        dump_image<MT>(smem, ST::A_LO, head + total + (size_t)rows * (D_HID * 2), tr_rows_left, wv, lane);
    };
    // fp16-range guard (GUARD instantiation, PnrSplitAux.sat_flag): bit l of sat_bits = "a head of 65504 (the largest fp16: heads
    // saturate there; i.e. a value >= 65488) went into the operand image of layer l" (2b: relu(x) entering blocks[b].fc_0, 2b+1: relu(net) entering
    // fc_1, 10: the stream in front of lin_out), bit 11 = a non-finite network output
    [[maybe_unused]] uint32_t sat_bits = 0;
    [[maybe_unused]] uint32_t amax = 0u;  // packed f16 pair: the running maximum of the heads (split8)
    [[maybe_unused]] auto sat_note = [&](int layer) {
        if constexpr (GUARD) {  // either half >= 0x7BFF: 65504, +inf or a NaN
            if ((amax & 0x7FFFu) >= 0x7BFFu || (amax & 0x7FFF0000u) >= 0x7BFF0000u) sat_bits |= 1u << layer;
            amax = 0u;
        }
    };
    // PROBE: the largest relu'd value of the accumulator tiles a stage is about to split -> LDS word `layer`.  One LDS max per
    // lane, straight-line (an atomicMax() becomes a branch + a wave-reduction loop); the file has no static LDS, so the dynamic
    // block starts at LDS address 0.  NaNs are skipped (fmaxf); an inf arrives as inf.
    [[maybe_unused]] auto probe_note = [&](const acc_t (&a)[AI][AJ], int layer) {
        if constexpr (PROBE) {
            float m = 0.f;
#pragma unroll
            for (int it = 0; it < AI; ++it)
#pragma unroll
                for (int jt = 0; jt < AJ; ++jt)
#pragma unroll
                    for (int r = 0; r < AR; r += 2) m = fmaxf(fmaxf(m, a[it][jt][r]), a[it][jt][r + 1]);
            const uint32_t ad = ST::LDS_TOTAL + 4u * (uint32_t)layer;
            asm volatile("ds_max_u32 %0, %1" : : "v"(ad), "v"(m) : "memory");
        }
    };
    [[maybe_unused]] auto own_mark = [&](int ph) { PNR_T(ph); };
    // the stages of a 512-wide linear on this instantiation's core
    auto bias_set = [&](acc_t (&a)[AI][AJ], int slot) {
        if constexpr (M16) add_bias16<true>(a, bias_lane, h, slot);
        else add_bias<true>(a, bias_lane, slot);
    };
    auto bias_add = [&](acc_t (&a)[AI][AJ], int slot) {
        if constexpr (M16) add_bias16<false>(a, bias_lane, h, slot);
        else add_bias<false>(a, bias_lane, slot);
    };
    auto own = [&](acc_t (&a)[AI][AJ], const acc_t (&src)[AI][AJ]) {
        if constexpr (M16) stage_own16<ST, GUARD>(a, src, smem, a_wr, R, NS, &amax, own_mark);
        else stage_own<ST, JT, GUARD>(a, src, smem, a_wr, R, NS, &amax, own_mark);
    };
    auto rot = [&](acc_t (&a)[AI][AJ]) {
        if constexpr (M16) gemm_split_rot16(a, smem, a_rd0, 16 * ROW_ACT, ST::A_LO - ST::A_HI, wv, R, NS);
        else gemm_split_rot<JT>(a, smem, a_rd0, 32 * ROW_ACT, ST::A_LO - ST::A_HI, wv, R, NS);
    };
    auto table_add = [&](acc_t (&a)[AI][AJ], auto scaled, float sc) {
        if constexpr (M16) add_from_table16<ST, decltype(scaled)::value>(a, smem, pl, h, wv, sc);
        else add_from_table<ST, decltype(scaled)::value>(a, smem, pl, h, wv, sc);
    };
    // one residual block on x (resnetfc.py:66-88); lookup: lin_z[b+1] via table b+1 behind it.
    // Every 512-wide linear = stage_own (split epilogue + this wave's own K block, from registers) | barrier | gemm_split_rot
    auto block = [&](acc_t (&x)[AI][AJ], int b, bool lookup) {
        if constexpr (TRAIN) put_mask(x, 2 * b, b < COMBINE_LAYER ? tr_mask_view : tr_mask_pooled);
        __syncthreads();  // table rows / previous operand images are no longer read
        PNR_T(PH_BAR1);
        {
            acc_t net[AI][AJ];
            bias_set(net, 1 + 2 * b);
            if constexpr (TIMING) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the bias has ARRIVED when the stage's clock starts (diagnostic: also drains the ring)
            own_mark(PH_OWN_BIAS);
            probe_note(x, 2 * b);
            own(net, x);                                                                           // fc_0, own block
            sat_note(2 * b);
            PNR_T(PH_WRITE_X);
            __syncthreads();
            PNR_T(PH_BAR2);
            if constexpr (TRAIN) dump_pair(q.s_a[b], b);
            rot(net);                                                                              // fc_0, blocks of the other waves
            PNR_T(PH_GEMM_FC0);
            if constexpr (TRAIN) put_mask(net, 2 * b + 1, b < COMBINE_LAYER ? tr_mask_view : tr_mask_pooled);
            __syncthreads();
            PNR_T(PH_BAR3);
            bias_add(x, 2 + 2 * b);
            own_mark(PH_OWN_BIAS);
            probe_note(net, 2 * b + 1);
            own(x, net);                                                                           // fc_1, own block
            sat_note(2 * b + 1);
            PNR_T(PH_WRITE_NET);
        }
        __syncthreads();
        PNR_T(PH_BAR4);
        if constexpr (TRAIN) dump_pair(q.s_n[b], b);
        rot(x);                                                                                    // fc_1
        PNR_T(PH_GEMM_FC1_Z);
        if (lookup) {
            __syncthreads();
            gather_table_f32<2, ST>(q, smem, wv, lane, b + 1);
            __syncthreads();
            table_add(x, std::integral_constant<bool, SC != 0>(), sc_c);
            PNR_T(PH_TABLE);
        }
    };

    // XCD-aware tile order (pnr_device.h tile_range; which tile a workgroup runs does not touch any result)
    const TileRange order = tile_range(q.ntiles, q.n_xcd);
    for (int tile = order.begin; tile < order.end; tile += order.step) {
        acc_t x[AI][AJ];
#pragma unroll 1
        for (int view = 0; view < NS; ++view) {
            __syncthreads();  // previous tile / view: every reader of the images / IN / META is done
            PNR_T(PH_SYNC_TOP);
            // 8 work items per point (projection, six frequency bands, padding): MT * 8 items over the workgroup's threads
            if constexpr (MT * 8 <= NTHREADS) {
                if (MT * 8 == NTHREADS || tid < MT * 8) geometry_item<PH, RAYS, ST>(q, smem, tile, view, tid % MT, tid / MT);
            } else {
#pragma unroll 1
                for (int wi = tid; wi < MT * 8; wi += NTHREADS) geometry_item<PH, RAYS, ST>(q, smem, tile, view, wi % MT, wi / MT);
            }
            __syncthreads();
            PNR_T(PH_GEOMETRY);
            gather_table_f32<2, ST>(q, smem, wv, lane, 0);
            PNR_T(PH_GATHER);
            bias_set(x, B_IN_Z0);
            if constexpr (M16) gemm_split16_in(x, smem, in_rd0, 16 * ROW_IN, ST::IN_LO_DELTA, R, NS);
            else gemm_split(x, smem, in_rd0, 32 * ROW_IN, ST::IN_LO_DELTA, KS_IN / 4, R, NS);  // lin_in   resnetfc.py:147
            __syncthreads();  // table rows of every wave are in place
            table_add(x, std::false_type(), 1.f);                                             // lin_z[0] via table 0
            if constexpr (SC != 0) {  // from here on the stream is c x
#pragma unroll
                for (int it = 0; it < AI; ++it)
#pragma unroll
                    for (int jt = 0; jt < AJ; ++jt) x[it][jt] *= sc_c;
            }
            PNR_T(PH_GEMM_IN_Z0);
            if constexpr (TRAIN) {
                tr_rows_pooled = (long long)tile * MT;
                tr_rows_view = (long long)view * q.P + tr_rows_pooled;
                tr_rows_left = q.P - tr_rows_pooled;
                tr_mask_pooled = (size_t)tile * NTHREADS + tid;
                tr_mask_view = tr_mask_pooled + (size_t)view * (size_t)q.ntiles * NTHREADS;
            }
#pragma unroll 1
            for (int b = 0; b < COMBINE_LAYER; ++b) block(x, b, b + 1 < COMBINE_LAYER);
            if constexpr (MV) {
                static_assert(AI * AJ * AR == IT * JT * 16, "both cores park 16 slots of 16 bytes per thread");
                f32x4 *ws = reinterpret_cast<f32x4 *>(q.mv_ws) + (size_t)blockIdx.x * (IT * JT * 4 * NTHREADS) + tid;
                const float inv = 1.f / (float)NS;
                const bool first = view == 0, last = view + 1 == NS;
                // util.combine_interleaved (util.py:461-471): mean, or -- network flag -- the maximum over the source views
                const bool cmax = (reinterpret_cast<const int *>(q.bout)[BOUT_FLAGS_INDEX] & 1) != 0;
#pragma unroll
                for (int it = 0; it < AI; ++it)
#pragma unroll
                    for (int jt = 0; jt < AJ; ++jt) {
                        if (AR == 16 || jt == 0) __builtin_amdgcn_sched_barrier(0);  // 4 loads in flight at a time: no register spike
#pragma unroll
                        for (int k = 0; k < AR / 4; ++k) {
                            const int i = (it * AJ + jt) * (AR / 4) + k;
                            f32x4 v = {x[it][jt][4 * k], x[it][jt][4 * k + 1], x[it][jt][4 * k + 2], x[it][jt][4 * k + 3]};
                            if (!first) {  // 1 KiB per wave-instruction
                                const f32x4 prev = ws[i * NTHREADS];  // (ordinary, L2-resident accesses: non-temporal ones measured -1 ... -2.5 %)
                                if (cmax) { v[0] = fmaxf(prev[0], v[0]); v[1] = fmaxf(prev[1], v[1]); v[2] = fmaxf(prev[2], v[2]); v[3] = fmaxf(prev[3], v[3]); }
                                else v = prev + v;
                            }
                            if (!last) ws[i * NTHREADS] = v;
                            else if (!cmax) v *= inv;
                            x[it][jt][4 * k] = v[0]; x[it][jt][4 * k + 1] = v[1]; x[it][jt][4 * k + 2] = v[2]; x[it][jt][4 * k + 3] = v[3];
                        }
                    }
            }
        }
#pragma unroll 1
        for (int b = COMBINE_LAYER; b < N_BLOCKS; ++b) block(x, b, false);
        if constexpr (TRAIN) {
            dump_rows(x, q.f_x5, tr_rows_pooled, tr_rows_left);
            put_mask(x, 10, tr_mask_pooled);
        }

        // lin_out(relu(x)): each wave contracts its own 64 features (the wave's accumulators are the B operand)
        probe_note(x, 10);
        if constexpr (M16) {
            // A = lin_out's 4 rows padded to 16 (row tile 0 of the two ring steps), B = the own block's two K-steps from the
            // accumulators as in stage_own16: the 4 outputs of point 16 jt + pl land in registers 0..3 of the lanes of group 0
            f32x4 o[NJ16];
#pragma unroll
            for (int jt = 0; jt < NJ16; ++jt) o[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            // Its fragments are the one place where the packed stream is not "two packed steps per K = 32 step": K-step m, group g
            // is row pl of packed fragment (step m, it = g & 1), lane half g >> 1 (rows 4..31 of those fragments are zero).  They are
            // fetched here rather than through the ring: a ring step is 4 KiB further on for every lane, lin_out's second K-step
            // is 2 KiB behind its first, and a per-lane offset cannot turn one stride into the other.  The ring's two steps at this
            // cursor (packed steps 324-327: lin_out's pieces in another order, and zero padding) are read and dropped, as the
            // 32x32x16 core drops its zero steps 2-3 there: 16 KiB per wave against the 1.3 MB a wave streams per tile.  The four
            // loads wait ~1 us per 176 us tile; the next tile's lin_in steps are requested first, so the ring fills meanwhile.
            const size_t pf = ring_pf16(R);
            refill16(R, 0, pf);
            refill16(R, 1, pf);
            ring_advance16(R, NS);
            const size_t out_off = (size_t)(RS_TOTAL_F - KS_OUT) * (IT * 1024) + (h & 1) * 1024 + (pl + 32 * (h >> 1)) * 16;
            h8 oh[2], ol[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                oh[m] = gload8<PH>(R.base_h + out_off + m * (IT * 1024));
                ol[m] = gload8<PH>(R.base_l + out_off + m * (IT * 1024));
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const h8 ah = oh[m], al = ol[m];
#pragma unroll
                for (int jt = 0; jt < NJ16; ++jt) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] = x[2 * m][jt][e]; v[4 + e] = x[2 * m + 1][jt][e]; }
                    h8 bh, bl;
                    split8<true, GUARD>(v, bh, bl, &amax);
                    o[jt] = mf16(ah, bh, o[jt]);
                    o[jt] = mf16(ah, bl, o[jt]);
                    o[jt] = mf16(al, bh, o[jt]);
                }
            }
            sat_note(10);
            if (h == 0) {
#pragma unroll
                for (int jt = 0; jt < NJ16; ++jt) *reinterpret_cast<f32x4 *>(smem + ST::LDS_OUT + (wv * MT + jt * 16 + pl) * 16) = o[jt];
            }
        } else {
            f32x16 o[JT];
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[jt][r] = 0.f;
            const size_t pf = (size_t)R.pf_rs * (IT * 1024);
#pragma unroll
            for (int qk = 0; qk < 2 * IT; ++qk) {
                const int xit = qk >> 1, rr = qk & 1;
                const h8 ah = R.h[qk / IT][qk % IT], al = R.l[qk / IT][qk % IT];
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = x[xit][jt][8 * rr + e];
                    h8 bh, bl;
                    split8<true, GUARD>(v, bh, bl, &amax);
                    o[jt] = mf(ah, bh, o[jt]);
                    o[jt] = mf(ah, bl, o[jt]);
                    o[jt] = mf(al, bh, o[jt]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    R.h[j][it] = gload8<PH>(R.base_h + pf + j * (IT * 1024) + it * 1024);
                    R.l[j][it] = gload8<PH>(R.base_l + pf + j * (IT * 1024) + it * 1024);
                }
            ring_advance(R, NS);
            sat_note(10);
            if (h == 0) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) {
                    f32x4 t = {o[jt][0], o[jt][1], o[jt][2], o[jt][3]};
                    *reinterpret_cast<f32x4 *>(smem + ST::LDS_OUT + (wv * MT + jt * 32 + pl) * 16) = t;
                }
            }
        }
        PNR_T(PH_LIN_OUT);
        __syncthreads();
        PNR_T(PH_BAR_OUT);
        // (SC: the partials are at scale c 2^t, undone in front of lin_out's bias; GUARD: bit 11 = a non-finite output)
        output_stage<MT, SC != 0, GUARD>(smem + ST::LDS_OUT, tid, tile, q.bout, q.out, q.P, sc_out, &sat_bits);
        PNR_T(PH_FINAL);
    }
    if constexpr (GUARD) {
        if (sat_bits && q.sat_flag) atomicOr(q.sat_flag, sat_bits);
    }
    if constexpr (PROBE) {
        if (sat_bits & (1u << 11)) probe_lds[11] = 0x3F800000u;  // (every writer stores the same word)
        __syncthreads();
        if (tid < PROBE_WORDS) {
            const uint32_t m = probe_lds[tid];
            const float v = tid < 11 ? __builtin_bit_cast(float, m) * sc_inv : __builtin_bit_cast(float, m);  // true units
            if (m) atomicMax(q.probe + tid, __builtin_bit_cast(uint32_t, v));
        }
    }
}

// The instantiation of eval_split_kernel for one launch.  form: 0 = plain, 1 = stream scale, 2 = range probe (at any scale).
// The scaled and probe forms exist as the guard-capable instantiation only (it reports when EvalParams::sat_flag is set); the
// training instantiation takes ray samples at form 0.  nullptr: no such instantiation.
using SplitKernel = void (*)(EvalParams);
template <bool RAYS, bool MV>
static SplitKernel split_kernel_of(bool train, bool guard, int form) {
    if (train) {
        if constexpr (RAYS)
            if (form == 0) return guard ? eval_split_kernel<true, MV, false, true, true> : eval_split_kernel<true, MV, false, true>;
        return nullptr;
    }
    switch (form) {
    case 0: return guard ? eval_split_kernel<RAYS, MV, false, false, true> : eval_split_kernel<RAYS, MV>;
    case 1: return eval_split_kernel<RAYS, MV, false, false, true, 1>;
    case 2: return eval_split_kernel<RAYS, MV, false, false, true, 2>;
    }
    return nullptr;
}
static SplitKernel split_kernel(bool rays, bool mv, bool train, bool guard, int form) {
    return mv ? (rays ? split_kernel_of<true, true>(train, guard, form) : split_kernel_of<false, true>(train, guard, form))
              : (rays ? split_kernel_of<true, false>(train, guard, form) : split_kernel_of<false, false>(train, guard, form));
}

int check_split_aux(const PnrSplitAux *aux, int precision, const char *entry) {
    if (!aux) return PNR_OK;
    char msg[256];
    if (aux->stream_scale_log2 < 0 || aux->stream_scale_log2 > STREAM_SCALE_MAX) {
        std::snprintf(msg, sizeof(msg), "%s: PnrSplitAux.stream_scale_log2 must be in [0, 30]", entry);
        return pnr_fail(PNR_E_INVALID, msg);
    }
    if (precision != PNR_PREC_F16X3 && (aux->stream_scale_log2 || aux->sat_flag || aux->range_probe)) {
        std::snprintf(msg, sizeof(msg), "%s: PnrSplitAux (stream_scale_log2, sat_flag, range_probe) belongs to PNR_PREC_F16X3 only", entry);
        return pnr_fail(PNR_E_INVALID, msg);
    }
    return PNR_OK;
}

// q: from ray_samples() / points() (pnr_entry.h: scene, sizes and limits checked); aux: checked by the entry (check_split_aux)
static int split_launch(const PnrScene *s, const void *packed, const void *tables, EvalParams &q, bool rays, const PnrSplitAux *aux,
                        hipStream_t st) {
    if (!packed || !tables || !q.out) return pnr_fail(PNR_E_INVALID, "pnr_eval_split: null argument");
    if (q.P == 0) return PNR_OK;
    set_packed(q, packed);
    q.tables = (const char *)tables;
    q.table_stride = grid_elems(*s);
    const bool mv = s->NS > 1;
    if (mv && !q.mv_ws) return pnr_fail(PNR_E_INVALID, "pnr_eval_split: a multi-view scene needs PnrScene.mv_workspace (pnr_mv_workspace_bytes())");
    const int ncu = device_cus();
    // tile: 64 points (the two full operand images fill the LDS; the 96-point K-half-staged form of round 3 measured 15 % slower,
    // profiles/r03_split_kernel_ab.txt, and was removed with the other experiment code in round 4)
    const int MT = SplitTileT<64>::MT, lds = SplitTileT<64>::LDS_TOTAL;
    const long long nt = (q.P + MT - 1) / MT;
    q.ntiles = (int)nt;
    const int grid = (int)(nt < ncu ? nt : ncu);
    // guard word, stream scale and probe words of this network: the caller's (PnrSplitAux).  The training forward (q.f_x5: the
    // same kernel + what the backward keeps) has no scaled form (its entry refuses a scale) and no probe form (the pointer is unused).
    const bool train = q.f_x5 != nullptr;
    q.sat_flag = aux ? aux->sat_flag : nullptr;
    q.probe = aux ? reinterpret_cast<unsigned int *>(aux->range_probe) : nullptr;
    const int form = q.probe && !train ? 2 : aux && aux->stream_scale_log2 ? 1 : 0;
    SplitKernel k = split_kernel(rays, mv, train, q.sat_flag != nullptr, form);
    if (!k) return pnr_fail(PNR_E_INVALID, "pnr_eval_split: the training instantiation takes ray samples at stream scale 0");
    const int lds_extra = form == 2 ? 64 : 0;  // the probe's 12 words behind the tile map
#ifdef PNR_VARIANT
    if (q.tim) {  // diagnostic instantiation (pnr_debug_phase_timing_split): single view, rays
        if (form) return pnr_fail(PNR_E_INVALID, "phase timing: unscaled blobs, no probe");
        if (mv || !rays) return pnr_fail(PNR_E_INVALID, "phase timing: single-view ray launches only");
        k = eval_split_kernel<true, false, true>;
    }
#endif
    static_assert(SplitTileT<64>::LDS_TOTAL + 64 <= 160 * 1024 && PROBE_WORDS * 4 <= 64, "room for the probe's words");
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds + lds_extra);
    if (e != hipSuccess) return pnr_check_hip(e, "hipFuncSetAttribute(eval_split_kernel)");
    {
        q.n_xcd = device_xcd_count();
        ProfileScope prof(st);  // HIP events around the launch on ITS stream when pnr_profile_enable(1) is active
        hipLaunchKernelGGL(k, dim3(grid), dim3(NTHREADS), lds + lds_extra, st, q);
    }
    return pnr_check_launch("eval_split_kernel");
}

}  // namespace pnr

extern "C" size_t pnr_packed_mlp_split_bytes(void) { return 2 * pnr::PACKED_BYTES; }

int pnr::eval_samples_split_src(const char *entry, const PnrScene *scene, const void *packed_split, const void *tables_f32,
                                const RaySrc &src, const float *z, int R, int rays_per_obj, int K, float *rgbsigma,
                                const PnrSplitAux *aux, hipStream_t stream) {
    pnr::EvalParams q = {};
    if (int rc = pnr::ray_samples(q, entry, scene, src, z, R, rays_per_obj, K, true, pnr::EVAL_LIMITS)) return rc;
    q.out = rgbsigma;
    return pnr::split_launch(scene, packed_split, tables_f32, q, true, aux, stream);
}

// training forward of the fp32-class path (pnr_f32.hip, pnr_eval_ray_samples_split_train): outputs + what the backward keeps
int pnr::eval_samples_split_train(const PnrScene *scene, const void *packed_split, const void *tables_f32, const EvalParams &samples,
                                  float *rgbsigma, void *const *img_a, void *const *img_n, float *x5, void *masks,
                                  const PnrSplitAux *aux, hipStream_t stream) {
    if (!img_a || !img_n || !x5 || !masks) return pnr_fail(PNR_E_INVALID, "pnr_eval_ray_samples_split_train: null argument");
    pnr::EvalParams q = samples;
    q.out = rgbsigma;
    for (int b = 0; b < 5; ++b) {
        if (!img_a[b] || !img_n[b]) return pnr_fail(PNR_E_INVALID, "pnr_eval_ray_samples_split_train: null operand buffer");
        q.s_a[b] = (char *)img_a[b]; q.s_n[b] = (char *)img_n[b];
    }
    q.f_x5 = x5;
    q.d_mask = (unsigned long long *)masks;
    return pnr::split_launch(scene, packed_split, tables_f32, q, true, aux, stream);
}

extern "C" int pnr_eval_ray_samples_split(const PnrScene *scene, const void *packed_split, const void *tables_f32,
                                          const float *rays, const float *z, int R, int rays_per_obj, int K, float *rgbsigma,
                                          const PnrSplitAux *aux, void *stream) {
    if (int rc = pnr::check_split_aux(aux, PNR_PREC_F16X3, "pnr_eval_ray_samples_split")) return rc;
    return pnr::eval_samples_split_src("pnr_eval_ray_samples_split", scene, packed_split, tables_f32, pnr::explicit_rays(rays), z, R,
                                       rays_per_obj, K, rgbsigma, aux, (hipStream_t)stream);
}

#ifdef PNR_VARIANT
// diagnostic hook of variant builds (tools/gpu_phase_timing_split.py): per-phase cycle totals of every wave of workgroup 0, one
// single-view launch
extern "C" int pnr_debug_phase_timing_split(const PnrScene *scene, const void *packed_split, const void *tables_f32, const float *rays,
                                            const float *z, int R, int rays_per_obj, int K, float *rgbsigma, unsigned long long *tim,
                                            void *stream) {
    if (!tim) return pnr_fail(PNR_E_INVALID, "pnr_debug_phase_timing_split: null argument");
    pnr::EvalParams q = {};
    if (int rc = pnr::ray_samples(q, "pnr_debug_phase_timing_split", scene, rays, z, R, rays_per_obj, K, false, pnr::EVAL_LIMITS)) return rc;
    q.out = rgbsigma; q.tim = tim;
    return pnr::split_launch(scene, packed_split, tables_f32, q, true, nullptr, (hipStream_t)stream);
}
#endif

extern "C" int pnr_eval_points_split(const PnrScene *scene, const void *packed_split, const void *tables_f32, const float *xyz,
                                     const float *viewdirs, int B, float *rgbsigma, const PnrSplitAux *aux, void *stream) {
    if (int rc = pnr::check_split_aux(aux, PNR_PREC_F16X3, "pnr_eval_points_split")) return rc;
    pnr::EvalParams q = {};
    if (int rc = pnr::points(q, "pnr_eval_points_split", scene, xyz, viewdirs, B, pnr::EVAL_LIMITS)) return rc;
    q.out = rgbsigma;
    return pnr::split_launch(scene, packed_split, tables_f32, q, false, aux, (hipStream_t)stream);
}
