// pnr_bwd_split.hip -- the data-gradient chain of the fp32-class training path (gfx950).
//
// The data-gradient chain of one ResnetFC at split-operand precision, behind the training forward of pnr_split.hip and fused like
// pnr_bwd.hip's bwd_kernel: same tile geometry as the forward (persistent 512-thread workgroup, 64-point tiles, wave w owns
// features 64w..64w+63), the gradient G of the residual stream resident in fp32 accumulators, a TRANSPOSED (head, tail) weight stream
//     lin_out^T | fc_1[4]^T fc_0[4]^T fc_1[3]^T fc_0[3]^T | per source view: fc_1[2]^T fc_0[2]^T ... fc_0[0]^T,
// gradient images as (head, tail) f16 pairs in LDS (pnr_split_ops.h), relu masks = the TRAIN forward's 1-bit words.  Every layer's
// output gradient dY leaves as (head | tail) 16-bit rows at the chain's power-of-two scale: the operands of the weight-gradient
// GEMMs (dw_split_kernel, pnr_bwd.hip); d z_lat and d(code) come out of the same launch as fp32 rows.
// (reference: torch autograd through src/model/resnetfc.py:132-184, resnetfc.py:55-62 per block.)
//   pack_weights_bwd_split_kernel   the transposed weight streams, from the raw parameters
//   bwd_split_kernel<MV>            the chain: all 15 transposed products of a network in one launch
// Host side of the training path: pnr_f32.hip (pnr_*_split_train).
#include <hip/hip_runtime.h>

#include "pnr_common.h"
#include "pnr_device.h"
#include "pnr_entry.h"
#include "pnr_internal.h"
#include "pnr_layout.h"
#include "pnr_split_ops.h"

namespace pnr {

// one thread = one lane's 8-element fragment slice of the head AND the tail stream (16-byte stores)
__global__ void pack_weights_bwd_split_kernel(PnrMlpWeights p, _Float16 *__restrict__ out_h, _Float16 *__restrict__ out_l) {
    const size_t idx8 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx8 >= (size_t)BSRS_TOTAL * IT * 64 * NW) return;
    const int lane = idx8 & 63;
    const int it = (idx8 >> 6) % IT;
    const size_t rest = idx8 / (64 * IT);
    const int rs = rest % BSRS_TOTAL;
    const int wv = rest / BSRS_TOTAL;
    int g = 0;
    while (g + 1 < NBGEMM && rs >= bgemm_offset(g + 1)) ++g;
    const int st = rs - bgemm_offset(g);
    const int i = lane & 31, h = lane >> 5;
    const int f_row = wv * SL + it * 32 + i;  // A-operand row = output row of the transposed GEMM = INPUT feature of the layer
    __attribute__((aligned(16))) _Float16 oh[8], ol[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = 0.f;
        if (g == BG_Z2 || g == BG_Z1 || g == BG_Z0) {
            // d z_lat[c] += sum_f dY_b[f] W_z[b][f][c]: rows = latent channel c (natural order, wave w owns 64w..64w+63),
            // K = hidden feature f in the storage order of the gradient image
            const int b = g == BG_Z2 ? 2 : (g == BG_Z1 ? 1 : 0);
            const int f_o = feat_of(st >> 1, st & 1, 8 * h + e);
            v = p.lin_z_w[b][f_o * C_LAT + f_row];
        } else if (g == BG_IN) {
            // d(code | viewdir)[k] = sum_f dY[f] W_in[f][k]: every wave holds the FULL 64 (42 real) output rows and contracts
            // only its own 64 hidden features = storage elements 64w + 16s + 8h + e (K-split, reduced across waves in LDS)
            const int k_row = it * 32 + i;
            const int f_o = feat_of(wv * IT + (st >> 1), st & 1, 8 * h + e);
            if (k_row < D_IN) v = p.lin_in_w[f_o * D_IN + k_row];
        } else if (g == BG_OUT) {
            const int k = st * 16 + h * 8 + e;  // natural order of the 4 network outputs, zero padded
            if (k < D_OUT) v = p.lin_out_w[k * D_HID + f_row];
        } else {
            const int b = 4 - (g - 1) / 2;       // BG_FC1_4, BG_FC0_4, BG_FC1_3, ... -> block index
            const float *w = ((g - 1) & 1) == 0 ? p.fc1_w[b] : p.fc0_w[b];
            const int f_o = feat_of(st >> 1, st & 1, 8 * h + e);  // K index = OUTPUT feature, storage order of the gradient image
            v = w[f_o * D_HID + f_row];
        }
        const _Float16 hh = (_Float16)v;
        oh[e] = hh;
        ol[e] = (_Float16)(v - (float)hh);
    }
    *reinterpret_cast<uint4 *>(out_h + idx8 * 8) = *reinterpret_cast<const uint4 *>(oh);
    *reinterpret_cast<uint4 *>(out_l + idx8 * 8) = *reinterpret_cast<const uint4 *>(ol);
}

struct BwdSplitParams {
    const char *wstream;                 // head blob; the tail blob follows at + BSPACKED_BYTES
    const unsigned long long *d_mask;    // relu bit masks of the forward, [layer][view][tile][thread]
    const float *g_out;                  // (P,4) dL/d(lin_out output), unscaled
    const float *scale_dev;              // device [s, 1/s]: the chain runs at s (pnr_grad_scale)
    long long P;
    int NS, ntiles;
    char *g_fc1[5], *g_fc0[5], *g_x0;    // dY at scale s as (head | tail) 16-bit rows in storage order (copies of the gradient images):
                                         // b < 3 (NS*P,512) [view][point], else (P,512); g_x0 (NS*P,512); tail array behind the head array
    float *d_zlat;                       // (NS*P, 512) fp32, natural channel order, UNSCALED: d(interpolated latent) = sum_b dY_b W_z[b]
    float *d_in;                         // (NS*P, 42) fp32, unscaled: d(positional code | view direction)   (nullable: not written)
    float *mv_ws;                        // several views: per-workgroup scratch for the pooled gradient every view starts from
};

template <bool MV>
__global__ void __launch_bounds__(NTHREADS, NW / 4) bwd_split_kernel(const BwdSplitParams q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef SplitTileT<64> ST;
    constexpr int JT = ST::JT, MT = ST::MT;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = lane & 31, h = lane >> 5;
    const int NS = MV ? q.NS : 1;
    const uint32_t a_rd0 = ST::A_HI + pl * ROW_ACT + h * 16;
    const uint32_t in_rd0 = ST::LDS_IN + pl * ROW_IN + h * 16;
    const uint32_t a_wr = pl * ROW_ACT + (wv * IT) * 64 + h * 32;
    f16_ovfl_mode<PH>();
    SplitRing R;
    R.base_h = q.wstream + (size_t)wv * (BSRS_TOTAL * IT * 1024) + lane * 16;
    R.base_l = R.base_h + BSPACKED_BYTES;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            R.h[j][it] = gload8<PH>(R.base_h + j * (IT * 1024) + it * 1024);
            R.l[j][it] = gload8<PH>(R.base_l + j * (IT * 1024) + it * 1024);
        }
    R.pf_rs = 4;
    R.pf_view = 0;
    const float scale = q.scale_dev[0], inv_scale = q.scale_dev[1];
    const size_t mask_layer = (size_t)NS * (size_t)q.ntiles * NTHREADS;

    long long rows_left = 0;
    // the gradient image just published (head, tail) -> its 16-bit row sets (operands of the weight-gradient GEMM), whole rows
    auto dump_pair = [&](char *head, long long rows, bool per_view) {
        const size_t total = (size_t)(per_view ? (long long)NS * q.P : q.P) * (D_HID * 2);
        dump_image<MT>(smem, ST::A_HI, head + (size_t)rows * (D_HID * 2), rows_left, wv, lane);
        dump_image<MT>(smem, ST::A_LO, head + total + (size_t)rows * (D_HID * 2), rows_left, wv, lane);
    };
    // the GEMM on the image just published, with the image's copy-out in front of it
    auto gemm_dump = [&](f32x16 (&a)[IT][JT], char *head, long long rows, bool per_view) {
        dump_pair(head, rows, per_view);
        gemm_split<JT, SplitAdvBwd>(a, smem, a_rd0, 32 * ROW_ACT, ST::A_LO - ST::A_HI, KS_BIG / 4, R, NS);
    };
    // reverse of one residual block (resnetfc.py:55-62):  given G = dL/d(x + fc_1(relu(fc_0(relu(x))))),
    //   dY(fc_1) = G ;  d net = (fc_1^T G) . [net > 0] = dY(fc_0) ;  G += (fc_0^T d net) . [x > 0]
    auto bwd_block = [&](f32x16 (&G)[IT][JT], int b, long long rows, size_t mask_off) {
        __syncthreads();  // every wave is done reading the gradient image (previous GEMM)
        write_split<ST, false>(G, smem, a_wr);
        __syncthreads();
        f32x16 t[IT][JT];
        const unsigned long long mk_n = (q.d_mask + (size_t)(2 * b + 1) * mask_layer)[mask_off];
        zero_acc(t);
        gemm_dump(t, q.g_fc1[b], rows, b < COMBINE_LAYER);
        apply_mask(t, mk_n);
        __syncthreads();
        write_split<ST, false>(t, smem, a_wr);
        __syncthreads();
        const unsigned long long mk_a = (q.d_mask + (size_t)(2 * b) * mask_layer)[mask_off];
        zero_acc(t);
        gemm_dump(t, q.g_fc0[b], rows, b < COMBINE_LAYER);
        masked_add(G, t, mk_a);
    };

    for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
        rows_left = q.P - (long long)tile * MT;
        const long long rows_pooled = (long long)tile * MT;
        const size_t mask_pooled = (size_t)tile * NTHREADS + tid;
        __syncthreads();  // previous tile: readers of the staging rows / gradient image are done
        {   // stage s * g_out as (head, tail) operand rows [point][64] (4 real values, zero padded)
            const int row = tid >> 3, chunk = tid & 7;
            const long long g = rows_pooled + row;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (chunk == 0 && g < q.P) {
                const f32x4 gv = *reinterpret_cast<const f32x4 *>(q.g_out + g * 4) * scale;
                v[0] = gv[0]; v[1] = gv[1]; v[2] = gv[2]; v[3] = gv[3];
            }
            h8 hi, lo;
            split8<false>(v, hi, lo);
            *reinterpret_cast<h8 *>(smem + ST::LDS_IN + row * ROW_IN + chunk * 16) = hi;
            *reinterpret_cast<h8 *>(smem + ST::LDS_IN + ST::IN_LO_DELTA + row * ROW_IN + chunk * 16) = lo;
        }
        __syncthreads();
        f32x16 G[IT][JT];
        {
            const unsigned long long mk = (q.d_mask + (size_t)10 * mask_layer)[mask_pooled];
            zero_acc(G);
            gemm_split<JT, SplitAdvBwd>(G, smem, in_rd0, 32 * ROW_IN, ST::IN_LO_DELTA, KS_IN / 4, R, NS);  // lin_out^T g_out
            apply_mask(G, mk);                                                                             // . [x5 > 0]
        }
#pragma unroll 1
        for (int b = N_BLOCKS - 1; b >= COMBINE_LAYER; --b) bwd_block(G, b, rows_pooled, mask_pooled);
        // backward of the view mean (util.py:461-466): every view starts from G / NS, parked in the per-workgroup scratch
        [[maybe_unused]] f32x4 *gws = MV ? reinterpret_cast<f32x4 *>(q.mv_ws) + (size_t)blockIdx.x * (IT * JT * 4 * NTHREADS) + tid : nullptr;
        if constexpr (MV) {
            const float inv = 1.f / (float)NS;
#pragma unroll
            for (int it = 0; it < IT; ++it)
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const f32x4 v = {G[it][jt][4 * k], G[it][jt][4 * k + 1], G[it][jt][4 * k + 2], G[it][jt][4 * k + 3]};
                        gws[((it * JT + jt) * 4 + k) * NTHREADS] = v * inv;
                    }
        }
#pragma unroll 1
        for (int view = 0; view < NS; ++view) {
            if constexpr (MV) {
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const f32x4 v = gws[((it * JT + jt) * 4 + k) * NTHREADS];
                            G[it][jt][4 * k] = v[0]; G[it][jt][4 * k + 1] = v[1]; G[it][jt][4 * k + 2] = v[2]; G[it][jt][4 * k + 3] = v[3];
                        }
            }
            const long long rows_view = (long long)view * q.P + rows_pooled;
            const size_t mask_view = mask_pooled + (size_t)view * (size_t)q.ntiles * NTHREADS;
#pragma unroll 1
            for (int b = COMBINE_LAYER - 1; b >= 0; --b) bwd_block(G, b, rows_view, mask_view);
            // ---- d z_lat = sum_b dY_b W_z[b] and d(code) = dY_0 W_in (resnetfc.py:147,175-180 backward): four more transposed-
            // stream GEMMs on gradient images this tile has just produced.  dY_2, dY_1 (= g_fc1[1], g_fc1[0]) come back from the
            // rows this workgroup copied out a moment ago (L2-resident); dY_0 = G is still in registers.
            f32x16 Z[IT][JT];
            zero_acc(Z);
#pragma unroll 1
            for (int b = COMBINE_LAYER - 1; b >= 1; --b) {
                __threadfence_block();
                __syncthreads();  // the image's readers are done; the rows this tile dumped are visible
                {
                    const char *src = q.g_fc1[b - 1] + (size_t)rows_view * (D_HID * 2);
                    const size_t total = (size_t)NS * (size_t)q.P * (D_HID * 2);
#pragma unroll
                    for (int u = 0; u < MT / NW; ++u) {
                        const int row = wv * (MT / NW) + u;
                        u32x4 vh = {0, 0, 0, 0}, vl = vh;
                        if (row < rows_left) {
                            vh = *reinterpret_cast<const u32x4 *>(src + (size_t)row * (D_HID * 2) + lane * 16);
                            vl = *reinterpret_cast<const u32x4 *>(src + total + (size_t)row * (D_HID * 2) + lane * 16);
                        }
                        *reinterpret_cast<u32x4 *>(smem + ST::A_HI + row * ROW_ACT + lane * 16) = vh;
                        *reinterpret_cast<u32x4 *>(smem + ST::A_LO + row * ROW_ACT + lane * 16) = vl;
                    }
                }
                __syncthreads();
                gemm_split<JT, SplitAdvBwd>(Z, smem, a_rd0, 32 * ROW_ACT, ST::A_LO - ST::A_HI, KS_BIG / 4, R, NS);  // lin_z[b]^T dY_b
            }
            __syncthreads();
            write_split<ST, false>(G, smem, a_wr);  // dY of lin_in and lin_z[0]
            __syncthreads();
            gemm_dump(Z, q.g_x0, rows_view, true);                                                                   // lin_z[0]^T dY_0
            {   // accumulator (channel 64 wv + 32 it + (r&3) + 8(r>>2) + 4h, point) -> fp32 rows, 16-byte pieces, out of the scaled domain
                float *dst = q.d_zlat + ((size_t)rows_view + pl) * C_LAT + (wv * IT) * 32 + 4 * h;
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) {
                    if (jt * 32 + pl >= rows_left) continue;
#pragma unroll
                    for (int it = 0; it < IT; ++it)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const f32x4 v = {Z[it][jt][4 * k], Z[it][jt][4 * k + 1], Z[it][jt][4 * k + 2], Z[it][jt][4 * k + 3]};
                            __builtin_nontemporal_store(v * inv_scale, reinterpret_cast<f32x4 *>(dst + (size_t)jt * 32 * C_LAT + it * 32 + 8 * k));
                        }
                }
            }
            // lin_in^T, K-split: this wave's 64 hidden features = bytes [128 wv, 128 wv + 128) of every image row
            zero_acc(Z);
            gemm_split<JT, SplitAdvBwd>(Z, smem, a_rd0 + wv * 128, 32 * ROW_ACT, ST::A_LO - ST::A_HI, KS_IN / 4, R, NS);
            __syncthreads();  // every wave is done with the images: their space takes the partials
            {
                // partial[w][point][k], 66-float rows: lanes of a half-wave write consecutive points -> distinct banks
                float *part = reinterpret_cast<float *>(smem) + (size_t)wv * (MT * 66);
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            part[(jt * 32 + pl) * 66 + it * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = Z[it][jt][r];
            }
            __syncthreads();
            if (q.d_in) {
                const int pnt = tid >> 3, k0 = (tid & 7) * 8;
                if (pnt < rows_left) {
#pragma unroll
                    for (int k = k0; k < k0 + 8; ++k) {
                        if (k >= D_IN) break;
                        float sum = 0.f;
#pragma unroll
                        for (int w = 0; w < NW; ++w) sum += reinterpret_cast<const float *>(smem)[(size_t)w * (MT * 66) + pnt * 66 + k];
                        q.d_in[((size_t)rows_view + pnt) * D_IN + k] = sum * inv_scale;
                    }
                }
            }
            __syncthreads();  // the partials are consumed before the next view / tile reuses the space
        }
    }
}

size_t bwd_split_packed_bytes() { return 2 * BSPACKED_BYTES; }

int pack_bwd_split(const PnrMlpWeights *w, void *packed, hipStream_t st) {
    if (!w || !packed) return pnr_fail(PNR_E_INVALID, "pack_bwd_split: null argument");
    const size_t n8 = (size_t)BSRS_TOTAL * IT * 64 * NW;
    hipLaunchKernelGGL(pack_weights_bwd_split_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, *w, (_Float16 *)packed,
                       (_Float16 *)((char *)packed + BSPACKED_BYTES));
    return pnr_check_launch("pack_weights_bwd_split_kernel");
}

int mlp_backward_split_chain(const void *packed_bwd_split, const unsigned long long *masks, const float *g_out, const float *scale_dev,
                             long long P, int NS, void *const *g_fc1, void *const *g_fc0, void *g_x0, float *d_zlat, float *d_in,
                             float *mv_ws, hipStream_t st) {
    if (!packed_bwd_split || !masks || !g_out || !scale_dev || !g_fc1 || !g_fc0 || !g_x0 || !d_zlat || P <= 0 || NS <= 0)
        return pnr_fail(PNR_E_INVALID, "mlp_backward_split_chain: bad argument");
    BwdSplitParams q = {};
    q.wstream = (const char *)packed_bwd_split; q.d_mask = masks; q.g_out = g_out; q.scale_dev = scale_dev; q.P = P; q.NS = NS;
    const long long nt = (P + 63) / 64;
    if (nt * NTHREADS * NS > 0xffffffffLL) return pnr_fail(PNR_E_INVALID, "mlp_backward_split_chain: too many points");
    q.ntiles = (int)nt;
    for (int b = 0; b < 5; ++b) {
        if (!g_fc1[b] || !g_fc0[b]) return pnr_fail(PNR_E_INVALID, "mlp_backward_split_chain: null gradient buffer");
        q.g_fc1[b] = (char *)g_fc1[b]; q.g_fc0[b] = (char *)g_fc0[b];
    }
    q.g_x0 = (char *)g_x0; q.d_zlat = d_zlat; q.d_in = d_in;
    const int cus = device_cus();
    const int grid = (int)(nt < cus ? nt : cus);
    const bool mv = NS > 1;
    if (mv && !mv_ws) return pnr_fail(PNR_E_INVALID, "mlp_backward_split_chain: NS > 1 needs the multi-view scratch");
    q.mv_ws = mv_ws;
    auto k = mv ? bwd_split_kernel<true> : bwd_split_kernel<false>;
    const int lds = SplitTileT<64>::LDS_TOTAL;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return pnr_check_hip(e, "hipFuncSetAttribute(bwd_split_kernel)");
    hipLaunchKernelGGL(k, dim3(grid), dim3(NTHREADS), lds, st, q);
    return pnr_check_launch("bwd_split_kernel");
}

}  // namespace pnr
