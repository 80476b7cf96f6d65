// pnr_bwd.hip -- backward of the hot path for training (BASELINE config 5), gfx950.
//
//   bwd_kernel            fused data-gradient chain of one ResnetFC: same tile geometry as the
//                         forward kernel (persistent 512-thread workgroup, 64-point tiles, wave w
//                         owns features 64w..64w+63, gradient of the residual stream resident in
//                         fp32 accumulators), driven by a TRANSPOSED weight stream
//                         (lin_out^T, fc_1[b]^T, fc_0[b]^T, b = 4..0, then lin_z[2..0]^T and lin_in^T).
//                         relu masks = the forward's 1-bit-per-element words; every layer's output
//                         gradient dY leaves as whole 16-bit rows copied out of the LDS image
//                         (operands of the weight-gradient GEMMs dW = dY^T X).
//   dw_kernel             dW = dY^T X for all linears of a network in one launch (MFMA from the dumps
//                         through transposing LDS reads), dw_reduce_kernel sums the row slices.
//   dw_split_wide_kernel  the same at split-operand (fp32-class) precision: (head | tail) f16 operand rows, three
//                         MFMAs per product -- the weight gradients of the fused fp32-class training path.
//   composite_bwd_kernel  backward of the alpha compositing (nerf.py:223-249), wavefront per ray: the suffix sums by a
//                         reverse scan of affine maps (no division, no difference of sums).
//                         also emits dL/dz through the deltas and depth = sum w z, and dL/dfar through the last delta.
//   position_bwd_kernel   dL/dz through the network inputs (positional code, projection, bilinear
//                         coordinates): the reference's position gradient through the n_fine_depth
//                         samples (nerf.py:292), for all points or for the depth samples only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "pnr_common.h"
#include "pnr_device.h"
#include "pnr_entry.h"
#include "pnr_internal.h"
#include "pnr_layout.h"

namespace pnr {

typedef Advance<BRS_HEAD_END, BRS_TOTAL, BRS_TOTAL> AdvanceBwd;

// ---------------------------------------------------------------- transposed weight stream
// one thread = one lane's 8-element fragment slice (16-byte store)
template <typename T>
__global__ void pack_weights_bwd_kernel(PnrMlpWeights p, T *__restrict__ out) {
    const size_t idx8 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx8 >= BWSTREAM_ELEMS_PER_WAVE / 8 * NW) return;
    const int lane = idx8 & 63;
    const int it = (idx8 >> 6) % IT;
    const size_t rest = idx8 / ((FRAG_ELEMS / 8) * IT);
    const int rs = rest % BRS_TOTAL;
    const int wv = rest / BRS_TOTAL;
    int g = 0;
    while (g + 1 < NBGEMM && rs >= bgemm_offset(g + 1)) ++g;
    const int s = rs - bgemm_offset(g);
    const int i = lane & 31, h = lane >> 5;
    // A-operand row = output row of the transposed GEMM = INPUT feature of the layer
    const int f_row = wv * SL + it * 32 + i;
    __attribute__((aligned(16))) T o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = 0.f;
        if (g == BG_Z2 || g == BG_Z1 || g == BG_Z0) {
            // d z_lat[c] += sum_f dY_b[f] W_z[b][f][c]: rows = latent channel c (natural order, wave w owns 64w..64w+63),
            // K = hidden feature f in the storage order of the gradient image
            const int b = g == BG_Z2 ? 2 : (g == BG_Z1 ? 1 : 0);
            const int f_o = feat_of(s >> 1, s & 1, 8 * h + e);
            v = p.lin_z_w[b][f_o * C_LAT + f_row];
        } else if (g == BG_IN) {
            // d(code | viewdir)[k] = sum_f dY[f] W_in[f][k]: every wave holds the FULL 64 (42 real) output rows and
            // contracts only its own 64 hidden features = storage elements 64w + 16s + 8h + e (K-split, reduced across
            // waves in LDS)
            const int k_row = it * 32 + i;
            const int f_o = feat_of(wv * IT + (s >> 1), s & 1, 8 * h + e);
            if (k_row < D_IN) v = p.lin_in_w[f_o * D_IN + k_row];
        } else if (g == BG_OUT) {
            const int k = s * 16 + h * 8 + e;  // natural order of the 4 network outputs, zero padded
            if (k < D_OUT) v = p.lin_out_w[k * D_HID + f_row];
        } else {
            const int b = 4 - (g - 1) / 2;       // BG_FC1_4, BG_FC0_4, BG_FC1_3, ... -> block index
            const bool fc1 = ((g - 1) & 1) == 0;
            const float *w = fc1 ? p.fc1_w[b] : p.fc0_w[b];
            // K index = OUTPUT feature of the layer, in the storage order of the gradient image
            const int f_o = feat_of(s >> 1, s & 1, 8 * h + e);
            v = w[f_o * D_HID + f_row];
        }
        o[e] = (T)v;
    }
    *reinterpret_cast<uint4 *>(out + idx8 * 8) = *reinterpret_cast<const uint4 *>(o);
}

// ---------------------------------------------------------------- fused data-gradient chain
struct BwdParams {
    const char *wstream;
    const unsigned long long *d_mask;    // relu bit masks of the forward (pnr_device.h: nonzero_bits8), [layer][view][tile][thread]
    const float *g_out;                  // (P,4) dL/d(lin_out output)
    float scale;
    const float *scale_dev;  // when set, the chain runs at *scale_dev instead (scale picked on the device)
    long long P;
    int NS, ntiles;
    char *g_fc1[5], *g_fc0[5], *g_x0;
    float *d_zlat;  // (NS*P, 512) fp32, natural channel order: d(interpolated latent)   (nullable: skip)
    float *d_in;    // (NS*P, 42)  fp32: d(positional code | view direction)             (nullable: skip)
    float *mv_ws;   // multi-view: per-workgroup scratch for the pooled gradient every view starts from ([slot][thread])
};

// reverse of one residual block (resnetfc.py:55-62):  given G = dL/d(x + fc_1(relu(fc_0(relu(x))))),
//   dY(fc_1) = G ;  d net = (fc_1^T G) . [net > 0] = dY(fc_0) ;  G += (fc_0^T d net) . [x > 0]
template <typename P>
__device__ __forceinline__ void bwd_block(f32x16 (&G)[IT][JT], char *smem, int b, Ring<P> &R, int NS, const BwdParams &q,
                                          size_t off, uint32_t a_rd0, uint32_t a_rd1, uint32_t a_wr,
                                          uint32_t mask_off, size_t mask_layer, long long rows_left, int wv, int lane) {
    // gradient dumps (operands of the weight-gradient GEMMs): copied out of the image behind the barrier, whole rows; rows beyond
    // the last point stay out through dump_image's rows_left (no per-lane validity is needed here)
    const size_t off_tile = off - (size_t)(((lane & 31) * D_HID + (wv * IT) * 32 + (lane >> 5) * 16) * 2);
    __syncthreads();  // every wave is done reading the gradient image (previous GEMM)
    write_act<P, false, false>(G, smem, a_wr);
    __syncthreads();
    dump_image<MT>(smem, LDS_A, q.g_fc1[b] + off_tile, rows_left, wv, lane);
    f32x16 t[IT][JT];
    // mask_off / mask_layer: this thread's word within a layer of q.d_mask / words per layer (layer 2b: x, 2b+1: net)
    const unsigned long long mk_n = (q.d_mask + (size_t)(2 * b + 1) * mask_layer)[mask_off];
    zero_acc(t);
    gemm<P, AdvanceBwd>(t, smem, a_rd0, a_rd1, KS_BIG / 4, R, NS);
    apply_mask(t, mk_n);
    __syncthreads();
    write_act<P, false, false>(t, smem, a_wr);
    __syncthreads();
    dump_image<MT>(smem, LDS_A, q.g_fc0[b] + off_tile, rows_left, wv, lane);
    const unsigned long long mk_a = (q.d_mask + (size_t)(2 * b) * mask_layer)[mask_off];
    zero_acc(t);
    gemm<P, AdvanceBwd>(t, smem, a_rd0, a_rd1, KS_BIG / 4, R, NS);
    masked_add(G, t, mk_a);
}

template <int PREC, bool MV>
__global__ void __launch_bounds__(NTHREADS, NW / 4) bwd_kernel(const BwdParams q) {
    typedef Prec<PREC> P;
    typedef typename P::T T;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = lane & 31, h = lane >> 5;
    const int NS = MV ? q.NS : 1;
    const uint32_t a_rd0 = LDS_A + pl * ROW_ACT + h * 16, a_rd1 = a_rd0 + 32 * ROW_ACT;
    const uint32_t in_rd0 = LDS_IN + pl * ROW_IN + h * 16, in_rd1 = in_rd0 + 32 * ROW_IN;
    const uint32_t a_wr = LDS_A + pl * ROW_ACT + (wv * IT) * 64 + h * 32;

    Ring<P> R;
    R.wave_base = q.wstream + (size_t)wv * (BRS_TOTAL * IT * 1024) + lane * 16;
    R.pf_view = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int it = 0; it < IT; ++it) R.r[j][it] = gload8<P>(R.wave_base + j * (IT * 1024) + it * 1024);
    R.pf_rs = 4;

    for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
        bool valid[JT];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) valid[jt] = (long long)tile * MT + jt * 32 + pl < q.P;
        const size_t off_pooled = (((size_t)tile * MT + pl) * D_HID + (wv * IT) * 32 + h * 16) * 2;

        __syncthreads();  // previous tile: readers of the staging rows / gradient image are done
        {   // stage scale * g_out as 16-bit operand rows [point][64] (4 real values, zero padded)
            const int row = tid >> 3, chunk = tid & 7;
            const long long g = (long long)tile * MT + row;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (chunk == 0 && g < q.P) v = *reinterpret_cast<const f32x4 *>(q.g_out + g * 4) * (q.scale_dev ? *q.scale_dev : q.scale);
            if (tid < MT * 8)
                *reinterpret_cast<typename P::T8 *>(smem + LDS_IN + row * ROW_IN + chunk * 16) =
                    pack8<P, false>(v[0], v[1], v[2], v[3], 0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        f32x16 G[IT][JT];
        const size_t mask_layer = (size_t)NS * (size_t)q.ntiles * NTHREADS;
        const long long rows_left = q.P - (long long)tile * MT;
        const uint32_t mask_pooled = (uint32_t)tile * NTHREADS + tid;  // 32 bits: NS * tiles * 512 < 2^32 (host check)
        {
            const unsigned long long mk = (q.d_mask + (size_t)10 * mask_layer)[mask_pooled];
            zero_acc(G);
            gemm<P, AdvanceBwd>(G, smem, in_rd0, in_rd1, KS_IN / 4, R, NS);  // lin_out^T g_out
            apply_mask(G, mk);                                                // . [x5 > 0]
        }
#pragma unroll 1
        for (int b = N_BLOCKS - 1; b >= COMBINE_LAYER; --b)
            bwd_block<P>(G, smem, b, R, NS, q, off_pooled, a_rd0, a_rd1, a_wr, mask_pooled, mask_layer, rows_left, wv, lane);
        // backward of the view mean (util.py:461-466): every view starts from G / NS.  That gradient is PARKED in a
        // per-workgroup scratch ([slot][thread]: every lane re-reads what it wrote, L2-resident) instead of 64 registers held
        // across the whole per-view loop -- the in-register form spilled 106 registers.
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
            const size_t off_view = off_pooled + (size_t)view * (size_t)q.P * (D_HID * 2);
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
#pragma unroll 1
            for (int b = COMBINE_LAYER - 1; b >= 0; --b)
                bwd_block<P>(G, smem, b, R, NS, q, off_view, a_rd0, a_rd1, a_wr,
                             mask_pooled + (uint32_t)view * (uint32_t)q.ntiles * NTHREADS, mask_layer, rows_left, wv, lane);
            // ---- d z_lat = sum_b dY_b W_z[b] and d(code) = dY_0 W_in (resnetfc.py:147,175-180 backward): four more
            // transposed-stream GEMMs on gradient images this tile has just produced.  dY_2, dY_1 (= g_fc1[1], g_fc1[0])
            // come back from their dumps (written by this workgroup a moment ago, L2-resident), dY_0 = G is in registers.
            const float inv_scale = 1.f / (q.scale_dev ? *q.scale_dev : q.scale);
            f32x16 Z[IT][JT];
            zero_acc(Z);
#pragma unroll 1
            for (int b = COMBINE_LAYER - 1; b >= 1; --b) {
                __threadfence_block();
                __syncthreads();  // the image's readers are done; the dump rows of this tile are visible
                {
                    const char *src = q.g_fc1[b - 1] + (size_t)view * (size_t)q.P * (D_HID * 2);
#pragma unroll
                    for (int u = 0; u < MT / NW; ++u) {
                        const int row = wv * (MT / NW) + u;
                        const long long g = (long long)tile * MT + row;
                        u32x4 v = {0, 0, 0, 0};
                        if (g < q.P) v = *reinterpret_cast<const u32x4 *>(src + (size_t)g * (D_HID * 2) + lane * 16);
                        *reinterpret_cast<u32x4 *>(smem + LDS_A + row * ROW_ACT + lane * 16) = v;
                    }
                }
                __syncthreads();
                gemm<P, AdvanceBwd>(Z, smem, a_rd0, a_rd1, KS_BIG / 4, R, NS);  // lin_z[b]^T dY_b
            }
            __syncthreads();
            write_act<P, false, false>(G, smem, a_wr);  // dY of lin_in and lin_z[0]
            __syncthreads();
            dump_image<MT>(smem, LDS_A, q.g_x0 + (size_t)view * (size_t)q.P * (D_HID * 2) + (size_t)tile * MT * (D_HID * 2), rows_left,
                           wv, lane);
            gemm<P, AdvanceBwd>(Z, smem, a_rd0, a_rd1, KS_BIG / 4, R, NS);      // lin_z[0]^T dY_0
            {   // accumulator (channel 32T + (r&3) + 8(r>>2) + 4h, point) -> fp32 rows, 16-byte pieces
                float *dst = q.d_zlat + ((size_t)view * (size_t)q.P + (size_t)tile * MT + pl) * C_LAT + (wv * IT) * 32 + 4 * h;
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt) {
                        if (!valid[jt]) continue;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            f32x4 v = {Z[it][jt][4 * k], Z[it][jt][4 * k + 1], Z[it][jt][4 * k + 2], Z[it][jt][4 * k + 3]};
                            __builtin_nontemporal_store(v * inv_scale, reinterpret_cast<f32x4 *>(dst + (size_t)jt * 32 * C_LAT + it * 32 + 8 * k));  // streamed past the L2 (dump_image)
                        }
                    }
            }
            // lin_in^T, K-split: this wave's 64 hidden features = bytes [128 wv, 128 wv + 128) of every image row
            zero_acc(Z);
            gemm<P, AdvanceBwd>(Z, smem, a_rd0 + wv * 128, a_rd1 + wv * 128, KS_IN / 4, R, NS);
            __syncthreads();  // every wave is done with the image: its space (and LDS_Z below it) takes the partials
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
                const long long g = (long long)tile * MT + pnt;
                if (g < q.P) {
#pragma unroll
                    for (int k = k0; k < k0 + 8; ++k) {
                        if (k >= D_IN) break;
                        float sum = 0.f;
#pragma unroll
                        for (int w = 0; w < NW; ++w) sum += reinterpret_cast<const float *>(smem)[(size_t)w * (MT * 66) + pnt * 66 + k];
                        q.d_in[((size_t)view * (size_t)q.P + (size_t)g) * D_IN + k] = sum * inv_scale;
                    }
                }
            }
            __syncthreads();  // the partials are consumed before the next view / tile reuses the space
        }
    }
}

// ---------------------------------------------------------------- weight-gradient GEMM
// dW[o][k] = sum_r dY[r][o] X[r][k]   over 16-bit row-major dumps (rows,512) / (rows,512), fp32 out.
// The reduction index r is the slow dimension of both operands.  Slabs of 32 rows are staged in LDS AS
// THEY LIE IN MEMORY (row-major, 16-byte global loads -> 16-byte LDS writes) and the MFMA fragments
// (8 consecutive rows of one column) come out of gfx950's transposing LDS read ds_read_b64_tr_b16:
// per 16-lane group a [4 rows][16 columns] block, lane c receives column c.  Row stride 576 B puts the
// 4 rows of a block and the two blocks of a 32-lane half on disjoint banks.
// Block = 8 waves = one 256x256 tile of dW (wave = 64x128 = 2x4 MFMA tiles: every operand element is
// fetched from L2 twice, not four times as with 128x128 tiles); the 1-D grid enumerates (tile, slice of the
// rows = split-K, job): all linears of a network go in ONE launch.  Every slice writes its own
// partial (part[job][z][512][512], bpart[job][z][512]) with plain stores and dw_reduce_kernel sums them in
// a fixed order -> bit-reproducible, no atomics.  bpart = bias gradient sum_r dY[r][o].
constexpr int DW_MAX_JOBS = 16;
struct DwJobs {
    const void *dY[DW_MAX_JOBS], *X[DW_MAX_JOBS];
    float *dW[DW_MAX_JOBS], *db[DW_MAX_JOBS];
    long long rows[DW_MAX_JOBS];
    short nx[DW_MAX_JOBS];   // columns of X (= its row stride): 512, or 64 for the lin_in operand
    short ncw[DW_MAX_JOBS];  // columns of dW written (= its row stride): 512, or 42 for lin_in
    unsigned char rows_st[DW_MAX_JOBS], cols_st[DW_MAX_JOBS];
    int nsplit;
};

template <typename T8, int LDB>
__device__ __forceinline__ T8 tr_frag(const char *smem_row_col) {
    // two transposing reads: rows +0..3 and +4..7 (row stride LDB bytes) of this lane's column
    typedef short s4 __attribute__((ext_vector_type(4)));
    typedef short s8 __attribute__((ext_vector_type(8)));
    typedef __attribute__((address_space(3))) s4 *lds_s4;
    const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(smem_row_col));
    const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(smem_row_col + 4 * LDB));
    const s8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(T8, v);
}

template <int PREC>
__global__ void __launch_bounds__(512)
dw_kernel(const DwJobs jobs, float *__restrict__ part, float *__restrict__ bpart) {
    typedef Prec<PREC> P;
    typedef typename P::T T;
    constexpr int SR = 32, LDB = 576;  // rows per slab, LDS row stride in bytes (256 columns + 64 B pad: 144 dwords = 16 mod 64)
    __shared__ __attribute__((aligned(16))) char sYb[2][SR * LDB];  // double-buffered: slab s+1 is written while s is multiplied
    __shared__ __attribute__((aligned(16))) char sXb[2][SR * LDB];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // XCD-aware placement.  The four 256x256 tiles of one (job, row slice) read the SAME dY / X rows; workgroups are dealt
    // to the 8 XCDs round-robin by linear id, so a (tile, slice, job) grid puts the four on four different L2s and every
    // operand byte crosses the fabric twice.  Here the linear id is re-read as (XCD, k): four consecutive k of one XCD
    // are the four tiles of a group, so the group's operands are fetched into ONE L2 once.
    const int lid = blockIdx.x, ngroups = gridDim.x >> 2, full = (ngroups >> 3) * 32;
    int grp, tile4;
    if (lid < full) { const int k = lid >> 3; grp = (k >> 2) * 8 + (lid & 7); tile4 = k & 3; }
    else { const int rem = lid - full; grp = (full >> 2) + (rem >> 2); tile4 = rem & 3; }  // last partial row of groups
    const int job = grp / jobs.nsplit, slice = grp - job * jobs.nsplit;
    const T *dY = reinterpret_cast<const T *>(jobs.dY[job]);
    const T *X = reinterpret_cast<const T *>(jobs.X[job]);
    const long long rows = jobs.rows[job];
    const int nx = jobs.nx[job];
    long long per = (rows + jobs.nsplit - 1) / jobs.nsplit;
    per = (per + SR - 1) / SR * SR;
    const int o0 = (tile4 >> 1) * 256, k0 = (tile4 & 1) * 256;
    if (k0 >= nx) return;  // narrow X (lin_in): only the first column tile exists
    const long long r_begin = (long long)slice * per;
    const long long r_end = r_begin + per < rows ? r_begin + per : rows;
    const int wo = (w >> 1) * 64, wk = (w & 1) * 128;  // wave tile: 64 (o) x 128 (k) = 2 x 4 MFMA tiles
    const int i = lane & 31, kh = lane >> 5;
    f32x16 acc[2][4];
    float bsum[2] = {0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // register-staged software pipeline: the global loads of slab s+1 are in flight while slab s is
    // being multiplied out of LDS.  slab = 32 rows x 32 chunks of 8 columns per operand; 2 chunks per thread
    u32x4 vy[2], vx[2];
    auto load_slab = [&](long long r0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int chunk = t + u * 512;  // consecutive lanes -> consecutive 16-byte chunks of a row
            const int srow = chunk >> 5, scol = (chunk & 31) * 8;
            vy[u] = u32x4{0, 0, 0, 0};
            vx[u] = u32x4{0, 0, 0, 0};
            if (r0 + srow < r_end) {
                vy[u] = *reinterpret_cast<const u32x4 *>(dY + (r0 + srow) * D_HID + o0 + scol);
                if (k0 + scol < nx) vx[u] = *reinterpret_cast<const u32x4 *>(X + (r0 + srow) * nx + k0 + scol);
            }
        }
    };
    // this lane's corner of the [4][16] transpose blocks: row 8kh + (c16>>2), column 16*((lane>>4)&1) + 4*(c16&3)
    const int c16 = lane & 15;
    const int frag_off = (8 * kh + (c16 >> 2)) * LDB + (16 * ((lane >> 4) & 1) + 4 * (c16 & 3)) * 2;
    auto store_slab = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int chunk = t + u * 512;
            const int srow = chunk >> 5, scol = (chunk & 31) * 8;
            *reinterpret_cast<u32x4 *>(sYb[buf] + srow * LDB + scol * 2) = vy[u];
            *reinterpret_cast<u32x4 *>(sXb[buf] + srow * LDB + scol * 2) = vx[u];
        }
    };
    if (r_begin < r_end) {
        load_slab(r_begin);
        store_slab(0);
    }
    __syncthreads();
    int cur = 0;
    for (long long r0 = r_begin; r0 < r_end; r0 += SR, cur ^= 1) {
        const bool more = r0 + SR < r_end;
        if (more) load_slab(r0 + SR);  // in flight under this slab's MFMAs
        const char *sY = sYb[cur], *sX = sXb[cur];
#pragma unroll
        for (int ks = 0; ks < SR / 16; ++ks) {
            typename P::T8 af[2], bf[4];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = tr_frag<typename P::T8, LDB>(sY + ks * 16 * LDB + (wo + a * 32) * 2 + frag_off);
#pragma unroll
            for (int b = 0; b < 4; ++b) bf[b] = tr_frag<typename P::T8, LDB>(sX + ks * 16 * LDB + (wk + b * 32) * 2 + frag_off);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = P::mfma(af[a], bf[b], acc[a][b]);
            if ((tile4 & 1) == 0 && (w & 1) == 0) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int e = 0; e < 8; ++e) bsum[a] += (float)af[a][e];
            }
        }
        if (more) store_slab(cur ^ 1);  // the other buffer: its readers passed the barrier of the previous slab
        __syncthreads();
    }
    // D layout: column j = lane&31 -> k, row (r&3)+8(r>>2)+4kh -> o
    float *pz = part + ((size_t)job * jobs.nsplit + slice) * (D_HID * D_HID);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int orow = o0 + wo + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                pz[(size_t)orow * D_HID + k0 + wk + b * 32 + i] = acc[a][b][r];
            }
    if ((tile4 & 1) == 0 && (w & 1) == 0) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            float v = bsum[a] + __shfl_xor(bsum[a], 32, 64);  // both row halves of every k-step
            if (kh == 0) bpart[((size_t)job * jobs.nsplit + slice) * D_HID + o0 + wo + a * 32 + i] = v;
        }
    }
}

// The same weight-gradient GEMM at split-operand (fp32-class) precision: both operands arrive as (head, tail) f16 row sets -- the
// activation images of the fused split forward and the gradient images of the fused split chain, copied out of LDS as they lie
// there; the tail array of an operand follows its head array -- and every fragment pair costs three MFMAs (head x head,
// head x tail, tail x head; fp32 accumulate), the arithmetic of PNR_PREC_F16X3.  Same placement, slice reduction and storage ->
// feature order mapping as dw_kernel; four operand slabs (dY / X, head / tail), double-buffered: 147 KiB of LDS.
// ONE wave per SIMD (round 6): 4 waves of 128 (o) x 128 (k) = 4 x 4 MFMA tiles, 256 accumulator registers per lane (the AGPR half
// of the 512-register file a 256-thread workgroup owns), 16 fragments per k-step for 48 MFMAs (the round-3..5 8-wave form: 12 for
// 24 -- a third less LDS traffic per MFMA), and room for TWO fragment sets: the fragments of k-step j + 1 are read while the MFMAs
// of k-step j issue, the slab barrier sits BETWEEN the two k-steps of a slab (every LDS read of a slab is issued before it, so the
// other buffer may be overwritten right behind it), and no k-step starts with an LDS burst of all waves behind a barrier.  What
// the 8-wave form did there (ISA): 24 transposing reads at the top of every k-step, waited for, then 24 MFMAs; after the barrier
// of every second k-step all 8 waves read at once -- 96 KiB through the 128 B/clk LDS pipe = 768 clocks against 1536 clocks of
// MFMAs per k-step and SIMD.  -12 % per launch, same partial sums bit for bit (profiles/r06_dw_split_notes.md).
__global__ void __launch_bounds__(256)
dw_split_wide_kernel(const DwJobs jobs, float *__restrict__ part, float *__restrict__ bpart) {
    typedef Prec<PNR_PREC_F16> P;
    typedef _Float16 T;
    constexpr int SR = 32, LDB = 576;
    extern __shared__ __attribute__((aligned(16))) char dws[];  // [buf][dY head, dY tail, X head, X tail][SR * LDB]
    constexpr int SLAB = SR * LDB;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int lid = blockIdx.x, ngroups = gridDim.x >> 2, full = (ngroups >> 3) * 32;
    int grp, tile4;
    if (lid < full) { const int k = lid >> 3; grp = (k >> 2) * 8 + (lid & 7); tile4 = k & 3; }
    else { const int rem = lid - full; grp = (full >> 2) + (rem >> 2); tile4 = rem & 3; }
    const int job = grp / jobs.nsplit, slice = grp - job * jobs.nsplit;
    const long long rows = jobs.rows[job];
    const int nx = jobs.nx[job];
    const T *dYh = reinterpret_cast<const T *>(jobs.dY[job]), *dYl = dYh + (size_t)rows * D_HID;
    const T *Xh = reinterpret_cast<const T *>(jobs.X[job]), *Xl = Xh + (size_t)rows * nx;
    long long per = (rows + jobs.nsplit - 1) / jobs.nsplit;
    per = (per + SR - 1) / SR * SR;
    const int o0 = (tile4 >> 1) * 256, k0 = (tile4 & 1) * 256;
    if (k0 >= nx) return;  // narrow X (lin_in): only the first column tile exists
    const long long r_begin = (long long)slice * per;
    const long long r_end = r_begin + per < rows ? r_begin + per : rows;
    const int wo = (w >> 1) * 128, wk = (w & 1) * 128;  // wave tile: 128 (o) x 128 (k) = 4 x 4 MFMA tiles
    const int i = lane & 31, kh = lane >> 5;
    f32x16 acc[4][4];
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // Staging: 4 x (dY head, dY tail, X head, X tail) 16-byte chunks per thread.  The pipelined loop takes FULL slabs only: its loads
    // are unconditional (uniform base per slab + 32-bit lane offset) and go to LDS as they arrive -- no exec-mask branches and no
    // selects, so the body is one basic block whose issue order is pinned, and nothing but the LDS stores of the NEXT k-step waits
    // for a load.  A narrow X (lin_in: 64 of the 256 columns exist) reads column 0 in place of the missing ones: those columns of
    // the partial products are never read (dw_reduce_kernel stops at the job's width).  A last partial slab of the slice (rows not
    // a multiple of 32) runs behind the loop with predicated loads.
    u32x4 vyh[4], vyl[4], vxh[4], vxl[4];
    unsigned offy[4], offx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int chunk = t + u * 256;  // consecutive lanes -> consecutive 16-byte chunks of a row
        const int srow = chunk >> 5, scol = (chunk & 31) * 8;
        offy[u] = (unsigned)(srow * D_HID + scol);
        offx[u] = (unsigned)(srow * nx + (k0 + scol < nx ? scol : 0));
    }
    const int lds_off = (t >> 5) * LDB + (t & 31) * 16;  // chunk u sits 8 rows further down
    const size_t tail_y = (size_t)rows * D_HID, tail_x = (size_t)rows * nx;
    auto load_slab = [&](long long r0) {
        const T *by = dYh + (size_t)r0 * D_HID + o0, *bx = Xh + (size_t)r0 * nx + k0;  // uniform
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            vyh[u] = *reinterpret_cast<const u32x4 *>(by + offy[u]);
            vyl[u] = *reinterpret_cast<const u32x4 *>(by + tail_y + offy[u]);
            vxh[u] = *reinterpret_cast<const u32x4 *>(bx + offx[u]);
            vxl[u] = *reinterpret_cast<const u32x4 *>(bx + tail_x + offx[u]);
        }
    };
    auto store_slab = [&](int buf) {
        char *base = dws + buf * (4 * SLAB) + lds_off;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            *reinterpret_cast<u32x4 *>(base + u * 8 * LDB) = vyh[u];
            *reinterpret_cast<u32x4 *>(base + SLAB + u * 8 * LDB) = vyl[u];
            *reinterpret_cast<u32x4 *>(base + 2 * SLAB + u * 8 * LDB) = vxh[u];
            *reinterpret_cast<u32x4 *>(base + 3 * SLAB + u * 8 * LDB) = vxl[u];
        }
    };
    const int c16 = lane & 15;
    const int frag_off = (8 * kh + (c16 >> 2)) * LDB + (16 * ((lane >> 4) & 1) + 4 * (c16 & 3)) * 2;
    struct Frags { P::T8 ah[4], al[4], bh[4], bl[4]; };
    auto read_frags = [&](Frags &f, int buf, int ks) {
        const char *sYh = dws + buf * (4 * SLAB) + ks * 16 * LDB + frag_off, *sYl = sYh + SLAB, *sXh = sYh + 2 * SLAB, *sXl = sYh + 3 * SLAB;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            f.ah[a] = tr_frag<P::T8, LDB>(sYh + (wo + a * 32) * 2);
            f.al[a] = tr_frag<P::T8, LDB>(sYl + (wo + a * 32) * 2);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            f.bh[b] = tr_frag<P::T8, LDB>(sXh + (wk + b * 32) * 2);
            f.bl[b] = tr_frag<P::T8, LDB>(sXl + (wk + b * 32) * 2);
        }
    };
    const bool sums = (tile4 & 1) == 0 && (w & 1) == 0;
    auto mfmas = [&](const Frags &f) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = P::mfma(f.ah[a], f.bh[b], acc[a][b]);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = P::mfma(f.ah[a], f.bl[b], acc[a][b]);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = P::mfma(f.al[a], f.bh[b], acc[a][b]);
        // column sums of dY (the bias gradient), formed in every wave -- a uniform branch would cut the pinned block in two -- and
        // written by the waves that own them: v_dot2_f32_f16 against (1, 1), fp32 accumulate, 8 VALU per fragment pair
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 ones = {(_Float16)1.f, (_Float16)1.f};
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                bsum[a] = __builtin_amdgcn_fdot2(h2{f.ah[a][e], f.ah[a][e + 1]}, ones, bsum[a], false);
                bsum[a] = __builtin_amdgcn_fdot2(h2{f.al[a][e], f.al[a][e + 1]}, ones, bsum[a], false);
            }
    };
    const int nrows = r_begin < r_end ? (int)(r_end - r_begin) : 0;
    const int nfull = nrows / SR;  // slabs of the pipelined loop
    if (nfull > 0) {
        Frags f0, f1;
        load_slab(r_begin);
        store_slab(0);
        __syncthreads();
        load_slab(r_begin + (long long)min(1, nfull - 1) * SR);
        read_frags(f0, 0, 0);
#pragma unroll 1
        for (int sl = 0; sl + 1 < nfull; ++sl) {
            const int cur = sl & 1;
            // k-step 0 of slab sl: its fragments were read under the previous k-step; read k-step 1's, then park slab sl + 1 (requested
            // a whole k-step ago) in the other buffer -- its last readers waited for their data in front of the previous barrier
            // k-step 0 of slab sl: its fragments were read under the previous k-step.  Read k-step 1's (32 slots), then park slab sl + 1 --
            // requested two k-steps ago -- in the other buffer (its last readers waited for their data in front of the previous barrier)
            // and request slab sl + 2 into every staging register right behind the LDS store that read it: 96 MFMA slots in flight
            // (requested behind the barrier instead -- 64 slots -- the launch was 2.5 % slower: profiles/r06_dw_split_notes.md)
            read_frags(f1, cur, 1);
            store_slab(cur ^ 1);
            load_slab(r_begin + (long long)min(sl + 2, nfull - 1) * SR);  // (the last iteration re-requests the last slab: no branch)
            mfmas(f0);
#pragma unroll
            for (int n = 0; n < 32; ++n) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 transposing read
                __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);  // 1 VALU (addresses, bias sums)
            }
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // 1 LDS store
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 global load into the register it read
                __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
            }
            __syncthreads();  // slab sl + 1 is visible; nobody reads buffer `cur` any more
            read_frags(f0, cur ^ 1, 0);
            mfmas(f1);
#pragma unroll
            for (int n = 0; n < 32; ++n) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
            }
        }
        // the last full slab
        read_frags(f1, (nfull - 1) & 1, 1);
        mfmas(f0);
        mfmas(f1);
    }
    if (nrows > nfull * SR) {  // the slice's last, partial slab (rows not a multiple of 32): predicated loads, no pipelining
        __syncthreads();
        const long long r0 = r_begin + (long long)nfull * SR;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int srow = (t + u * 256) >> 5;
            vyh[u] = vyl[u] = vxh[u] = vxl[u] = u32x4{0, 0, 0, 0};
            if (r0 + srow < r_end) {
                const T *by = dYh + (size_t)r0 * D_HID + o0, *bx = Xh + (size_t)r0 * nx + k0;
                vyh[u] = *reinterpret_cast<const u32x4 *>(by + offy[u]);
                vyl[u] = *reinterpret_cast<const u32x4 *>(by + tail_y + offy[u]);
                vxh[u] = *reinterpret_cast<const u32x4 *>(bx + offx[u]);
                vxl[u] = *reinterpret_cast<const u32x4 *>(bx + tail_x + offx[u]);
            }
        }
        store_slab(0);
        __syncthreads();
        Frags f;
        read_frags(f, 0, 0);
        mfmas(f);
        read_frags(f, 0, 1);
        mfmas(f);
    }
    float *pz = part + ((size_t)job * jobs.nsplit + slice) * (D_HID * D_HID);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int orow = o0 + wo + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                pz[(size_t)orow * D_HID + k0 + wk + b * 32 + i] = acc[a][b][r];
            }
    if (sums) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float v = bsum[a] + __shfl_xor(bsum[a], 32, 64);
            if (kh == 0) bpart[((size_t)job * jobs.nsplit + slice) * D_HID + o0 + wo + a * 32 + i] = v;
        }
    }
}

// dW = scale * sum_z part[job][z], db = scale * sum_z bpart[job][z]  (fixed summation order); blockIdx.y = job.
// rows_st / cols_st: the operand that indexes the rows (dY) / columns (X) of dW was dumped in storage order;
// the result is written in feature order (row e -> feature feat_of(e/32, (e%32)/16, e%16)).
__global__ void dw_reduce_kernel(const DwJobs jobs, const float *__restrict__ part, const float *__restrict__ bpart,
                                 float scale, const float *__restrict__ scale_dev) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int job = blockIdx.y, nz = jobs.nsplit;
    if (scale_dev) scale *= *scale_dev;
    const float *pj = part + (size_t)job * nz * (D_HID * D_HID);
    const float *bj = bpart + (size_t)job * nz * D_HID;
    const bool rows_st = jobs.rows_st[job], cols_st = jobs.cols_st[job];
    if (idx < D_HID * D_HID && (idx % D_HID) < ((jobs.nx[job] + 255) / 256) * 256) {
        float s = 0.f;
        for (int z = 0; z < nz; ++z) s += pj[(size_t)z * (D_HID * D_HID) + idx];
        int r = idx / D_HID, c = idx % D_HID;
        if (rows_st) r = feat_of(r >> 5, (r >> 4) & 1, r & 15);
        if (cols_st) c = feat_of(c >> 5, (c >> 4) & 1, c & 15);
        const int ncw = jobs.ncw[job];
        if (c < ncw) jobs.dW[job][r * ncw + c] = s * scale;
    }
    if (jobs.db[job] && idx < D_HID) {
        float s = 0.f;
        for (int z = 0; z < nz; ++z) s += bj[(size_t)z * D_HID + idx];
        jobs.db[job][rows_st ? feat_of(idx >> 5, (idx >> 4) & 1, idx & 15) : idx] = s * scale;
    }
}

// ---------------------------------------------------------------- compositing backward
// w_i = a_i T_i, T_i = prod_{j<i} tf_j, tf_j = 1 - a_j + 1e-10, a_i = 1 - exp(-delta_i relu(sigma_i))
// g_i = dL/dw_i = d_rgb.c_i + d_depth z_i + d_w_i - [white] sum(d_rgb)
// dL/da_i = T_i (g_i - S_i),  S_i = sum_{j>i} g_j a_j prod_{i<k<j} tf_k = g_{i+1} a_{i+1} + tf_{i+1} S_{i+1}
// (= g_i T_i - (sum_{j>i} g_j w_j) / tf_i, with the suffix summed directly: formed as total - prefix and divided by tf_i, its
// rounding is divided by a tiny tf_i on a nearly opaque sample and comes back times sigma_i exp(..) in dL/dz.)
// The 64-sample chunks are walked from the last to the first: per chunk a reverse wave scan of the maps S -> g_j a_j + tf_j S
// (wave_rscan_affine), S carried across chunks; T_i from the forward product scan, as composite_kernel forms it.
struct CompSample {
    float zi, delta, ex, alpha, tf;
    float4 cs;
    bool valid;
};

__device__ __forceinline__ CompSample composite_sample(const float *zr, const float4 *cr, int K, float far, int i) {
    CompSample s;
    s.valid = i < K;
    s.zi = 0.f; s.delta = 0.f; s.ex = 1.f; s.alpha = 0.f;
    s.cs = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s.valid) {
        s.zi = zr[i];
        s.delta = ((i + 1 < K) ? zr[i + 1] : far) - s.zi;
        s.cs = cr[i];
        s.ex = expf(-s.delta * fmaxf(s.cs.w, 0.f));
        s.alpha = 1.f - s.ex;
    }
    s.tf = s.valid ? (1.f - s.alpha + 1e-10f) : 1.f;
    return s;
}

// prod of tf over chunk c (every lane)
__device__ __forceinline__ float composite_chunk_product(const float *zr, const float4 *cr, int K, float far, int c, int lane) {
    return __shfl(wave_scan_mul(composite_sample(zr, cr, K, far, c * 64 + lane).tf, lane), 63, 64);
}

__global__ void __launch_bounds__(CW * 64)
composite_bwd_kernel(const float *__restrict__ rays, const float *__restrict__ z, const float4 *__restrict__ rgbs, int R,
                     int K, int white_bkgd, const float *__restrict__ d_rgb, const float *__restrict__ d_depth,
                     const float *__restrict__ d_w, float4 *__restrict__ d_rgbs, float *__restrict__ d_z, int preact,
                     float *__restrict__ d_far) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = blockIdx.x * CW + wv;
    if (r >= R) return;
    const float far = rays[(size_t)r * 8 + 7];
    const float3 drgb = make_float3(d_rgb[(size_t)r * 3], d_rgb[(size_t)r * 3 + 1], d_rgb[(size_t)r * 3 + 2]);
    const float ddepth = d_depth ? d_depth[r] : 0.f;
    const float gwhite = white_bkgd ? (drgb.x + drgb.y + drgb.z) : 0.f;  // rgb += 1 - sum w
    const float *zr = z + (size_t)r * K;
    const float4 *cr = rgbs + (size_t)r * K;
    const float *dwr = d_w ? d_w + (size_t)r * K : nullptr;
    float4 *dout = d_rgbs + (size_t)r * K;
    float *dzout = d_z ? d_z + (size_t)r * K : nullptr;
    const int nc = (K + 63) >> 6;

    // T at the head of chunk c, for c < 64 in lane c of `heads` (nothing to do for K <= 64); the chunks beyond 4096 samples
    // rebuild theirs from chunk 63's
    float heads = 1.f, carry = 1.f;
    for (int c = 1; c < nc && c < 64; ++c) {
        carry *= composite_chunk_product(zr, cr, K, far, c - 1, lane);
        if (lane == c) heads = carry;
    }

    float S_in = 0.f;  // S of the chunk's last sample
    float pend = 0.f;  // w d_depth - ddelta of the first sample of the chunk walked before: waits for ddelta of its left neighbour
    for (int c = nc - 1; c >= 0; --c) {
        const int c0 = c * 64, i = c0 + lane;
        carry = __shfl(heads, c < 64 ? c : 63, 64);
        for (int cc = 63; cc < c; ++cc) carry *= composite_chunk_product(zr, cr, K, far, cc, lane);
        const CompSample s = composite_sample(zr, cr, K, far, i);
        const float4 cs = s.cs;
        const float incl = wave_scan_mul(s.tf, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.f;
        const float T = carry * excl;
        const float w = s.alpha * T;
        float g = 0.f;
        if (s.valid) g = drgb.x * cs.x + drgb.y * cs.y + drgb.z * cs.z + ddepth * s.zi + (dwr ? dwr[i] : 0.f) - gwhite;
        float m = s.tf, b = g * s.alpha;  // past the end: (1, 0), the identity
        wave_rscan_affine(m, b, lane);
        const float mn = __shfl_down(m, 1, 64), bn = __shfl_down(b, 1, 64);
        const float S = lane == 63 ? S_in : bn + mn * S_in;
        S_in = __shfl(b + m * S_in, 0, 64);  // S of sample c0 - 1
        float ddelta = 0.f;
        if (s.valid) {
            const float dalpha = T * (g - S);
            const float dsigma = cs.w > 0.f ? dalpha * s.delta * s.ex : 0.f;
            float4 go = make_float4(w * drgb.x, w * drgb.y, w * drgb.z, dsigma);
            if (preact) {  // through rgb = sigmoid(.), sigma = relu(.) (models.py:260-263): relu' already applied
                go.x *= cs.x * (1.f - cs.x); go.y *= cs.y * (1.f - cs.y); go.z *= cs.z * (1.f - cs.z);
            }
            dout[i] = go;
            ddelta = dalpha * fmaxf(cs.w, 0.f) * s.ex;  // d alpha_i / d delta_i = relu(sigma) exp(-delta relu(sigma))
            if (d_far && i == K - 1) d_far[r] = ddelta;   // the last delta is far - z_{K-1} (nerf.py:181)
        }
        if (dzout) {
            // delta_i = z_{i+1} - z_i (last: far - z_i), depth = sum w z:
            //   dL/dz_i = w_i d_depth - ddelta_i + ddelta_{i-1}
            // the left neighbour of lane 0 is in the chunk walked next: its share is written from there (lane 63)
            const float up = __shfl_up(ddelta, 1, 64);
            const float own = w * ddepth - ddelta;
            if (s.valid && (lane > 0 || c0 == 0)) dzout[i] = lane > 0 ? own + up : own;
            if (lane == 63 && c0 + 64 < K) dzout[c0 + 64] = pend + ddelta;
            pend = __shfl(own, 0, 64);
        }
    }
}

// dL/dz through the network inputs; one wavefront per (view, point).
// ranks == nullptr: every point, the result is accumulated into d_z[point].
// ranks (R, Kfd): only the depth samples (the ones whose position carries gradient, nerf.py:157-160,292): wave =
// (view, ray, j), point = ray * K + ranks[ray][j]; the total dL/dz of that sample -- this network term plus the compositing
// term dz_comp -- goes through the clamp z = max(min(depth + n * std, far), near) into contrib[view][ray][j].
struct DepthSamples {
    const int *ranks;        // (R, Kfd) position of each depth sample in the sorted z, or null
    const float *n4;         // (R, Kfd) the normal draws
    const float *depth_c;    // (R) coarse depth
    const float *dz_comp;    // (R, K) compositing dL/dz (nullable)
    float *contrib;          // (NS, R, Kfd) out: what sample j of ray r sends to d_depth[r] through view v (summed by the caller
                             // in a fixed order: the result stays bit-reproducible)
    float depth_std;
    int Kfd;
};

__global__ void __launch_bounds__(CW * 64)
position_bwd_kernel(const EvalParams q, const float *__restrict__ d_in42, const float *__restrict__ d_zlat,
                    float *__restrict__ d_z, const DepthSamples ds) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long widx = (long long)blockIdx.x * CW + wv;
    int view, g, jd = 0;
    if (ds.ranks) {  // (view, ray, j)
        const long long per_view = (long long)(q.P / q.K) * ds.Kfd;
        if (widx >= per_view * q.NS) return;
        view = (int)(widx / per_view);
        const long long rj = widx - (long long)view * per_view;
        const int ray_i = (int)(rj / ds.Kfd);
        jd = (int)(rj - (long long)ray_i * ds.Kfd);
        g = ray_i * q.K + ds.ranks[(size_t)ray_i * ds.Kfd + jd];
    } else {         // view * P + point
        if (widx >= q.P * q.NS) return;
        view = (int)(widx / q.P);
        g = (int)(widx % q.P);
    }
    const long long idx = (long long)view * q.P + g;
    const SamplePoint sp = sample_point_fused(q, g, view);
    const PointGrad pg = point_grad(q, sp, view, idx, d_in42, d_zlat, lane);
    if (lane == 0) {
        const float g0 = pg.g0, g1 = pg.g1, g2 = pg.g2;
        const float *pose = sp.pose;
        // x_world gradient = R^T g ; dz = ray_dir . that
        const float wx = pose[0] * g0 + pose[4] * g1 + pose[8] * g2;
        const float wy = pose[1] * g0 + pose[5] * g1 + pose[9] * g2;
        const float wz = pose[2] * g0 + pose[6] * g1 + pose[10] * g2;
        float val = sp.dx * wx + sp.dy * wy + sp.dz * wz;
        if (!ds.ranks) {
            // a point on a source camera's plane or a non-finite upstream gradient: dropped, the rule of camera_record_kernel
            if (__builtin_isfinite(val)) atomicAdd(d_z + g, val);
        } else {
            if (view == 0 && ds.dz_comp) val += ds.dz_comp[g];
            const int r = sp.r;
            const float *ray = q.rays + (size_t)r * 8;
            const float zraw = ds.depth_c[r] + ds.n4[(size_t)r * ds.Kfd + jd] * ds.depth_std;
            const bool live = zraw < ray[7] && zraw > ray[6];  // inside the clamp: gradient passes (nerf.py:157-160)
            ds.contrib[widx] = (live && __builtin_isfinite(val)) ? val : 0.f;
        }
    }
}
#pragma clang fp contract(fast)

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_storage_perm(int32_t *perm512) {
    if (!perm512) return pnr_fail(PNR_E_INVALID, "pnr_storage_perm: null argument");
    for (int e = 0; e < D_HID; ++e) perm512[e] = feat_of(e / 32, (e % 32) / 16, e % 16);
    return PNR_OK;
}

extern "C" size_t pnr_packed_mlp_bwd_bytes(void) { return BPACKED_BYTES; }

extern "C" int pnr_pack_mlp_bwd(const PnrMlpWeights *w, int precision, void *packed_bwd, void *stream) {
    if (!w || !packed_bwd) return pnr_fail(PNR_E_INVALID, "pnr_pack_mlp_bwd: null argument");
    if (w->stream_scale_log2 != 0) return pnr_fail(PNR_E_INVALID, "pnr_pack_mlp_bwd: training at a stream scale (stream_scale_log2 != 0) is not supported");
    const size_t n = BWSTREAM_ELEMS_PER_WAVE / 8 * NW;  // one thread per 8 elements
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (precision == PNR_PREC_F16)
        hipLaunchKernelGGL(pack_weights_bwd_kernel<_Float16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *w, (_Float16 *)packed_bwd);
    else if (precision == PNR_PREC_BF16)
        hipLaunchKernelGGL(pack_weights_bwd_kernel<__bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *w, (__bf16 *)packed_bwd);
    else
        return pnr_fail(PNR_E_INVALID, "pnr_pack_mlp_bwd: unknown precision");
    return pnr_check_launch("pnr_pack_mlp_bwd");
}

// scales[0] = 2^(6 - ceil(log2 max|g|)) (1 if g == 0), scales[1] = 1 / scales[0]; NaN if g holds a non-finite value
__global__ void __launch_bounds__(1024) grad_scale_kernel(const float *__restrict__ g, long long n, float *__restrict__ scales) {
    __shared__ float red[1024];
    float m = 0.f;
    bool bad = false;
    // one block, but 8 independent 16-byte loads in flight per thread: a handful of memory round trips for the
    // (P,4) gradient instead of one per element (51 us -> a few us at config-5 sizes)
    const long long n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? n / 4 : 0;
    const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
    for (long long i0 = threadIdx.x; i0 < n4; i0 += 8 * 1024) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long i = i0 + (long long)u * 1024;
            v[u] = i < n4 ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = fabsf(v[u][e]);
                bad |= !(a <= 3.0e38f);
                m = fmaxf(m, a);
            }
    }
    for (long long i = n4 * 4 + threadIdx.x; i < n; i += 1024) {
        const float a = fabsf(g[i]);
        bad |= !(a <= 3.0e38f);
        m = fmaxf(m, a);
    }
    red[threadIdx.x] = bad ? __builtin_inff() : m;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float mx = red[0];
        float sc = 1.f;
        if (!(mx <= 3.0e38f)) sc = __builtin_nanf("");
        // exponent clamped to +-100: scale and 1/scale stay finite normal numbers for vanishing (denormal-range) or huge
        // gradients -- an unclamped 2^(6 - log2 mx) overflows to inf for mx < 2^-121 and poisons the step with 0 * inf
        else if (mx > 0.f) sc = exp2f(fminf(fmaxf(6.f - ceilf(log2f(mx)), -100.f), 100.f));
        scales[0] = sc;
        scales[1] = 1.f / sc;
    }
}

extern "C" size_t pnr_train_masks_bytes(long long P, int NS) {
    if (P <= 0 || NS <= 0) return 0;
    return (size_t)11 * (size_t)NS * (size_t)((P + MT - 1) / MT) * NTHREADS * sizeof(unsigned long long);
}

// Large gradients (the stand-alone linear operators scale a whole (rows, d_out) tensor: 33 M values take 1.5 ms in one workgroup):
// max |g| over many workgroups -- non-negative floats order like their bit patterns, a non-finite value enters as +inf -- into
// scales[0] (zeroed first), then one thread turns the maximum into [scale, 1 / scale] exactly as grad_scale_kernel does.
__global__ void __launch_bounds__(1024) grad_absmax_kernel(const float *__restrict__ g, long long n, unsigned int *__restrict__ out) {
    __shared__ float red[1024];
    float m = 0.f;
    bool bad = false;
    const long long n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? n / 4 : 0;
    const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
    const long long stride = (long long)gridDim.x * 8 * 1024;
    for (long long i0 = (long long)blockIdx.x * 8 * 1024 + threadIdx.x; i0 < n4; i0 += stride) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long i = i0 + (long long)u * 1024;
            v[u] = i < n4 ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = fabsf(v[u][e]);
                bad |= !(a <= 3.0e38f);
                m = fmaxf(m, a);
            }
    }
    if (blockIdx.x == 0)
        for (long long i = n4 * 4 + threadIdx.x; i < n; i += 1024) {
            const float a = fabsf(g[i]);
            bad |= !(a <= 3.0e38f);
            m = fmaxf(m, a);
        }
    red[threadIdx.x] = bad ? __builtin_inff() : m;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, __float_as_uint(red[0]));
}
__global__ void grad_scale_from_max_kernel(float *__restrict__ scales) {
    const float mx = __uint_as_float(reinterpret_cast<const unsigned int *>(scales)[0]);
    float sc = 1.f;
    if (!(mx <= 3.0e38f)) sc = __builtin_nanf("");
    else if (mx > 0.f) sc = exp2f(fminf(fmaxf(6.f - ceilf(log2f(mx)), -100.f), 100.f));
    scales[0] = sc;
    scales[1] = 1.f / sc;
}

extern "C" int pnr_grad_scale(const float *g, long long n, float *scales, void *stream) {
    if (!g || !scales || n <= 0) return pnr_fail(PNR_E_INVALID, "pnr_grad_scale: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (n <= (1LL << 20)) {  // the renderer's (P, 4) output gradient: one workgroup, one launch
        hipLaunchKernelGGL(grad_scale_kernel, dim3(1), dim3(1024), 0, st, g, n, scales);
        return pnr_check_launch("pnr_grad_scale");
    }
    const hipError_t e = hipMemsetAsync(scales, 0, 2 * sizeof(float), st);
    if (e != hipSuccess) return pnr_check_hip(e, "hipMemsetAsync(pnr_grad_scale)");
    const long long chunks = (n / 4 + 8 * 1024 - 1) / (8 * 1024);
    const unsigned blocks = (unsigned)(chunks < 1024 ? (chunks < 1 ? 1 : chunks) : 1024);
    hipLaunchKernelGGL(grad_absmax_kernel, dim3(blocks), dim3(1024), 0, st, g, n, reinterpret_cast<unsigned int *>(scales));
    hipLaunchKernelGGL(grad_scale_from_max_kernel, dim3(1), dim3(1), 0, st, scales);
    return pnr_check_launch("pnr_grad_scale");
}

extern "C" int pnr_mlp_backward(const void *packed_bwd, int precision, const PnrTrainDumps *fwd, const float *g_out,
                                float grad_scale, const float *grad_scale_dev, long long P, int NS,
                                const PnrBackwardDumps *out, void *stream) {
    if (!packed_bwd || !fwd || !g_out || !out || P <= 0 || NS <= 0 || (!grad_scale_dev && !(grad_scale > 0.f)))
        return pnr_fail(PNR_E_INVALID, "pnr_mlp_backward: bad argument");
    if (P > 0x7fffffc0LL || (P + MT - 1) / MT * NS * NTHREADS > 0xffffffffLL)
        return pnr_fail(PNR_E_INVALID, "pnr_mlp_backward: too many points");
    BwdParams q = {};
    q.wstream = (const char *)packed_bwd;
    q.g_out = g_out; q.scale = grad_scale; q.scale_dev = grad_scale_dev; q.P = P; q.NS = NS; q.ntiles = (int)((P + MT - 1) / MT);
    q.d_mask = (const unsigned long long *)fwd->d_mask; q.g_x0 = (char *)out->g_x0;
    q.d_zlat = out->d_zlat; q.d_in = out->d_in;
    // d_zlat is REQUIRED: the lin_z^T / lin_in^T GEMMs sit inside the per-view segment of the transposed weight stream, and
    // the prefetch ring only stays in step with that stream when they run (skipping them made every later view / tile
    // multiply by the wrong fragments)
    if (!q.d_zlat) return pnr_fail(PNR_E_INVALID, "pnr_mlp_backward: PnrBackwardDumps.d_zlat is required (d_in alone is optional)");
    if (!q.d_mask) return pnr_fail(PNR_E_INVALID, "pnr_mlp_backward: the forward dumps carry no relu bit masks (PnrTrainDumps.d_mask)");
    if (!q.g_x0) return pnr_fail(PNR_E_INVALID, "pnr_mlp_backward: null dump");
    for (int b = 0; b < 5; ++b) {
        q.g_fc1[b] = (char *)out->g_fc1[b]; q.g_fc0[b] = (char *)out->g_fc0[b];
        if (!q.g_fc1[b] || !q.g_fc0[b]) return pnr_fail(PNR_E_INVALID, "pnr_mlp_backward: null dump");
    }
    const bool mv = NS > 1;
    q.mv_ws = (float *)out->mv_workspace;
    if (mv && !q.mv_ws) return pnr_fail(PNR_E_INVALID, "pnr_mlp_backward: NS > 1 needs PnrBackwardDumps.mv_workspace (pnr_mv_workspace_bytes())");
    const int grid = q.ntiles < device_cus() ? q.ntiles : device_cus();
    void (*k)(const BwdParams);
    if (precision == PNR_PREC_F16) k = mv ? bwd_kernel<PNR_PREC_F16, true> : bwd_kernel<PNR_PREC_F16, false>;
    else if (precision == PNR_PREC_BF16) k = mv ? bwd_kernel<PNR_PREC_BF16, true> : bwd_kernel<PNR_PREC_BF16, false>;
    else return pnr_fail(PNR_E_INVALID, "pnr_mlp_backward: unknown precision");
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TOTAL);
    if (e != hipSuccess) return pnr_check_hip(e, "hipFuncSetAttribute(bwd_kernel)");
    hipLaunchKernelGGL(k, dim3(grid), dim3(NTHREADS), LDS_TOTAL, (hipStream_t)stream, q);
    return pnr_check_launch("bwd_kernel");
}

// lin_out (4 x 512): dW[o][k] = sum_r g[r][o] x5[r][k], db[o] = sum_r g[r][o]; g fp32 (P,4), x5 16-bit (P,512)
// in storage order.  Row slices -> partials -> fixed-order reduce (written in feature order).
constexpr int LO_BLOCKS = 256;
template <typename T>
__global__ void __launch_bounds__(256)
lin_out_grad_kernel(const float *__restrict__ g, const T *__restrict__ x5, long long P, float *__restrict__ part) {
    const int t = threadIdx.x;
    const long long per = (P + LO_BLOCKS - 1) / LO_BLOCKS;
    const long long r0 = (long long)blockIdx.x * per, r1 = r0 + per < P ? r0 + per : P;
    float acc[4][2] = {}, bs[4] = {};
#pragma unroll 8  // 8 rows of loads in flight: the loop is latency-bound otherwise (66 us -> ~10 us at config-5 sizes)
    for (long long r = r0; r < r1; ++r) {
        const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + r * 4);
        const uint32_t xw = *reinterpret_cast<const uint32_t *>(x5 + r * D_HID + 2 * t);
        const float xa = (float)__builtin_bit_cast(T, (uint16_t)(xw & 0xffffu)), xb = (float)__builtin_bit_cast(T, (uint16_t)(xw >> 16));
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            acc[o][0] += gv[o] * xa; acc[o][1] += gv[o] * xb;
            bs[o] += gv[o];
        }
    }
    float *pz = part + (size_t)blockIdx.x * (4 * D_HID + 4);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        pz[o * D_HID + 2 * t] = acc[o][0];
        pz[o * D_HID + 2 * t + 1] = acc[o][1];
    }
    if (t == 0) {
#pragma unroll
        for (int o = 0; o < 4; ++o) pz[4 * D_HID + o] = bs[o];
    }
}
__global__ void lin_out_reduce_kernel(const float *__restrict__ part, float *__restrict__ dW, float *__restrict__ db) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 4 * D_HID + 4) return;
    float s = 0.f;
    for (int z = 0; z < LO_BLOCKS; ++z) s += part[(size_t)z * (4 * D_HID + 4) + idx];
    if (idx < 4 * D_HID) {
        const int o = idx / D_HID, e = idx % D_HID;
        dW[o * D_HID + feat_of(e >> 5, (e >> 4) & 1, e & 15)] = s;
    } else if (db) {
        db[idx - 4 * D_HID] = s;
    }
}

extern "C" size_t pnr_lin_out_grad_workspace_bytes(void) { return (size_t)LO_BLOCKS * (4 * D_HID + 4) * sizeof(float); }

extern "C" int pnr_lin_out_grad(const float *g_out, const void *x5, long long P, int precision, float *dW, float *db,
                                void *workspace, void *stream) {
    if (!g_out || !x5 || !dW || !workspace || P <= 0) return pnr_fail(PNR_E_INVALID, "pnr_lin_out_grad: bad argument");
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)workspace;
    if (precision == PNR_PREC_F16)
        hipLaunchKernelGGL(lin_out_grad_kernel<_Float16>, dim3(LO_BLOCKS), dim3(256), 0, st, g_out, (const _Float16 *)x5, P, part);
    else if (precision == PNR_PREC_BF16)
        hipLaunchKernelGGL(lin_out_grad_kernel<__bf16>, dim3(LO_BLOCKS), dim3(256), 0, st, g_out, (const __bf16 *)x5, P, part);
    else
        return pnr_fail(PNR_E_INVALID, "pnr_lin_out_grad: unknown precision");
    hipLaunchKernelGGL(lin_out_reduce_kernel, dim3((4 * D_HID + 4 + 255) / 256), dim3(256), 0, st, part, dW, db);
    return pnr_check_launch("pnr_lin_out_grad");
}

constexpr int DW_MAX_SPLIT = 32;
static int dw_nsplit(int n_jobs, long long max_rows) {
    // 4 tiles x jobs x slices workgroups of 8 waves, one per CU at a time: pick the slice count whose workgroup total fills
    // whole rounds of the chip (14 jobs: 9 slices = 504 workgroups = 1.97 rounds; the former "at least 512" rule gave 10
    // slices = 560 = 2.19 rounds, i.e. a third round at 19 % occupancy); slices of at least 256 rows
    const int cus = device_cus();
    const int per = 4 * n_jobs;
    int best = 1;
    double best_eff = 0.0;
    for (int ns = 1; ns <= DW_MAX_SPLIT && (long long)per * ns <= 3LL * cus; ++ns) {
        const long long blocks = (long long)per * ns;
        const long long rounds = (blocks + cus - 1) / cus;
        const double eff = (double)blocks / (double)(rounds * cus);
        if (blocks >= cus && eff > best_eff + 1e-9) { best_eff = eff; best = ns; }
        else if (blocks < cus) best = ns;  // fewer workgroups than CUs: more slices is always better
    }
    const long long cap = (max_rows + 255) / 256;
    if (best > cap) best = (int)cap;
    return best < 1 ? 1 : best;
}

extern "C" size_t pnr_weight_grad_batched_workspace_bytes(int n_jobs, long long max_rows) {
    if (n_jobs < 1 || n_jobs > DW_MAX_JOBS || max_rows < 1) return 0;
    return (size_t)n_jobs * dw_nsplit(n_jobs, max_rows) * (D_HID * D_HID + D_HID) * sizeof(float);
}
extern "C" size_t pnr_weight_grad_workspace_bytes(void) { return (size_t)DW_MAX_SPLIT * (D_HID * D_HID + D_HID) * sizeof(float); }

extern "C" int pnr_weight_grad_batched(const PnrWeightGradJob *jobs, int n_jobs, int precision, float out_scale,
                                       const float *out_scale_dev, void *workspace, void *stream) {
    if (!jobs || !workspace || n_jobs < 1 || n_jobs > DW_MAX_JOBS)
        return pnr_fail(PNR_E_INVALID, "pnr_weight_grad_batched: 1..16 jobs and a workspace are required");
    DwJobs J = {};
    long long max_rows = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (!jobs[j].dY || !jobs[j].X || !jobs[j].dW || jobs[j].rows <= 0)
            return pnr_fail(PNR_E_INVALID, "pnr_weight_grad_batched: bad job");
        J.dY[j] = jobs[j].dY; J.X[j] = jobs[j].X; J.dW[j] = jobs[j].dW; J.db[j] = jobs[j].db; J.rows[j] = jobs[j].rows;
        J.rows_st[j] = jobs[j].rows_storage_order ? 1 : 0; J.cols_st[j] = jobs[j].cols_storage_order ? 1 : 0;
        const int nx = jobs[j].x_cols ? jobs[j].x_cols : D_HID, ncw = jobs[j].dw_cols ? jobs[j].dw_cols : nx;
        if (nx < 8 || nx > D_HID || nx % 8 != 0 || ncw < 1 || ncw > nx || (nx != D_HID && jobs[j].cols_storage_order))
            return pnr_fail(PNR_E_INVALID, "pnr_weight_grad_batched: x_cols must be a multiple of 8 in [8,512], dw_cols <= x_cols");
        J.nx[j] = (short)nx; J.ncw[j] = (short)ncw;
        if (jobs[j].rows > max_rows) max_rows = jobs[j].rows;
    }
    J.nsplit = dw_nsplit(n_jobs, max_rows);
    float *part = (float *)workspace;
    float *bpart = part + (size_t)n_jobs * J.nsplit * D_HID * D_HID;
    dim3 grid(4u * (unsigned)J.nsplit * (unsigned)n_jobs);  // (tile, slice, job) decoded XCD-aware in the kernel
    hipStream_t st = (hipStream_t)stream;
    if (precision == PNR_PREC_F16)
        hipLaunchKernelGGL(dw_kernel<PNR_PREC_F16>, grid, dim3(512), 0, st, J, part, bpart);
    else if (precision == PNR_PREC_BF16)
        hipLaunchKernelGGL(dw_kernel<PNR_PREC_BF16>, grid, dim3(512), 0, st, J, part, bpart);
    else if (precision == PNR_PREC_F16X3) {
        // split-operand form: dY / X are (head | tail) f16 row sets, the tail array behind the head array
        constexpr int lds = 2 * 4 * 32 * 576;
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dw_split_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return pnr_check_hip(e, "hipFuncSetAttribute(dw_split_wide_kernel)");
        hipLaunchKernelGGL(dw_split_wide_kernel, grid, dim3(256), lds, st, J, part, bpart);
    } else
        return pnr_fail(PNR_E_INVALID, "pnr_weight_grad_batched: unknown precision");
    hipLaunchKernelGGL(dw_reduce_kernel, dim3(D_HID * D_HID / 256, (unsigned)n_jobs), dim3(256), 0, st, J, part, bpart, out_scale, out_scale_dev);
    return pnr_check_launch("pnr_weight_grad_batched");
}

extern "C" int pnr_weight_grad(const void *dY, const void *X, long long rows, int precision, float out_scale,
                               int rows_storage_order, int cols_storage_order, float *dW, float *db, void *workspace,
                               void *stream) {
    if (!dY || !X || !dW || !workspace || rows <= 0) return pnr_fail(PNR_E_INVALID, "pnr_weight_grad: bad argument");
    PnrWeightGradJob job = {dY, X, rows, rows_storage_order, cols_storage_order, dW, db, 0, 0};
    return pnr_weight_grad_batched(&job, 1, precision, out_scale, nullptr, workspace, stream);
}

// pnr_composite_backward / pnr_composite_backward_far (d_far: dL/dfar through the last delta, or null)
static int composite_backward(const char *entry, const float *rays, const float *z, const float *rgbsigma, int R, int K, int white_bkgd,
                              const float *d_rgb, const float *d_depth, const float *d_weights, float *d_rgbsigma, float *d_z,
                              float *d_far, int pre_activation, void *stream) {
    if (R < 0 || K <= 0) return entry_fail(entry, "bad sizes");
    if (R == 0) return PNR_OK;
    if (!rays || !z || !rgbsigma || !d_rgb || !d_rgbsigma) return entry_fail(entry, "null argument");
    hipLaunchKernelGGL(composite_bwd_kernel, dim3((R + CW - 1) / CW), dim3(CW * 64), 0, (hipStream_t)stream, rays, z,
                       (const float4 *)rgbsigma, R, K, white_bkgd, d_rgb, d_depth, d_weights, (float4 *)d_rgbsigma, d_z,
                       pre_activation, d_far);
    return pnr_check_launch(entry);
}

extern "C" int pnr_composite_backward(const float *rays, const float *z, const float *rgbsigma, int R, int K, int white_bkgd,
                                      const float *d_rgb, const float *d_depth, const float *d_weights, float *d_rgbsigma,
                                      float *d_z, int pre_activation, void *stream) {
    return composite_backward("pnr_composite_backward", rays, z, rgbsigma, R, K, white_bkgd, d_rgb, d_depth, d_weights, d_rgbsigma, d_z,
                              nullptr, pre_activation, stream);
}

extern "C" int pnr_composite_backward_far(const float *rays, const float *z, const float *rgbsigma, int R, int K,
                                          int white_bkgd, const float *d_rgb, const float *d_depth, const float *d_weights,
                                          float *d_rgbsigma, float *d_z, float *d_far, int pre_activation, void *stream) {
    return composite_backward("pnr_composite_backward_far", rays, z, rgbsigma, R, K, white_bkgd, d_rgb, d_depth, d_weights, d_rgbsigma,
                              d_z, d_far, pre_activation, stream);
}

// position_bwd_kernel holds a point index in an int
extern "C" int pnr_position_backward(const PnrScene *s, const float *rays, const float *z, int R, int rays_per_obj, int K,
                                     const float *d_in42, const float *d_zlat, float *d_z, void *stream) {
    EvalParams q = {};
    if (int rc = ray_samples(q, "pnr_position_backward", s, rays, z, R, rays_per_obj, K, false, {0, INDEX_I32, 0})) return rc;
    if (!d_in42 || !d_zlat || !d_z) return pnr_fail(PNR_E_INVALID, "pnr_position_backward: bad argument");
    const long long n = q.P * q.NS;
    hipLaunchKernelGGL(position_bwd_kernel, dim3((unsigned)((n + CW - 1) / CW)), dim3(CW * 64), 0, (hipStream_t)stream, q,
                       d_in42, d_zlat, d_z, DepthSamples{});
    return pnr_check_launch("pnr_position_backward");
}

extern "C" int pnr_depth_sample_backward(const PnrScene *s, const float *rays, const float *z, int R, int rays_per_obj, int K,
                                         const int *ranks, const float *n4, int Kfd, const float *depth_c, float depth_std,
                                         const float *d_in42, const float *d_zlat, const float *dz_comp, float *contrib,
                                         void *stream) {
    EvalParams q = {};
    if (int rc = ray_samples(q, "pnr_depth_sample_backward", s, rays, z, R, rays_per_obj, K, false, {0, INDEX_I32, 0})) return rc;
    if (!ranks || !n4 || !depth_c || !d_in42 || !d_zlat || !contrib || Kfd <= 0 || Kfd > K)
        return pnr_fail(PNR_E_INVALID, "pnr_depth_sample_backward: bad argument");
    DepthSamples ds = {ranks, n4, depth_c, dz_comp, contrib, depth_std, Kfd};
    const long long n = (long long)R * Kfd * q.NS;
    hipLaunchKernelGGL(position_bwd_kernel, dim3((unsigned)((n + CW - 1) / CW)), dim3(CW * 64), 0, (hipStream_t)stream, q,
                       d_in42, d_zlat, nullptr, ds);
    return pnr_check_launch("pnr_depth_sample_backward");
}
