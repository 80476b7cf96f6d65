/*
 * pixelnerf_hip.h -- C ABI of libpixelnerf_hip.so: the MI355X (gfx950) native pixelNeRF
 * volume-rendering hot path.
 *
 * The reference (sxyu/pixel-nerf) has no FFI of its own: its seam is two Python classes,
 * NeRFRenderer (src/render/nerf.py:45-371) and PixelNeRFNet (src/model/models.py:14-316).
 * Every entry point below replaces a span of those classes; the span is cited per function
 * (paths relative to the reference repository root).  The Python host layer
 * (pixel-nerf_amd/render, pixel-nerf_amd/model) binds these through ctypes and presents the
 * reference's API on top; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP, current device) unless marked "host";
 *   - tensors are dense, row-major, fp32 unless stated;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     enqueued on it, nothing synchronises;
 *   - return value: 0 = ok, negative = PNR_E_* ; pnr_last_error() gives a message (host,
 *     thread-local);
 *   - memory is owned by the caller (torch tensors in the Python host); the library
 *     allocates nothing.
 */
#ifndef PIXELNERF_HIP_H
#define PIXELNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with hidden default visibility: what this header declares is all it exports */
#pragma GCC visibility push(default)

#define PNR_OK 0
#define PNR_E_INVALID (-1)   /* bad argument / unsupported shape          */
#define PNR_E_HIP (-2)       /* a HIP runtime call or kernel launch failed */

/* arithmetic of the 512-wide linear layers (operands of the MFMA; accumulation is fp32) */
#define PNR_PREC_F16 0       /* fp16 operands, v_mfma_f32_32x32x16_f16  */
#define PNR_PREC_BF16 1      /* bf16 operands, v_mfma_f32_32x32x16_bf16 */
#define PNR_PREC_F32 2       /* exact fp32 validation path (pnr_eval_*_f32 only), v_mfma_f32_32x32x2_f32 */
#define PNR_PREC_F16X3 3     /* fp32-class: every operand a (head, tail) pair of fp16, 3 f16 MFMAs per product,
                                fp32 tables (pnr_*_split entries; pnr_render_forward_folded accepts it) */

/* Encoded-scene state: exactly what PixelNeRFNet.encode() leaves in module buffers
 * (src/model/models.py:111-141, src/model/encoder.py:160-163), except that the feature grid
 * is channel-last so one bilinear corner is a contiguous 2 KiB row. */
typedef struct PnrScene {
    const float *latent_nhwc; /* (SB*NS, Hl, Wl, 512)  encoder.latent permuted NCHW->NHWC   */
    const float *poses;       /* (SB*NS, 3, 4) world->camera [R^T | -R^T t]  models.py:112-114 */
    const float *focal;       /* (n_focal, 2)  (fx, -fy)                     models.py:129-130 */
    const float *c;           /* (n_c, 2)      principal point               models.py:132-141 */
    int32_t SB;               /* objects                                                    */
    int32_t NS;               /* source views per object (row = obj*NS + view)              */
    int32_t Hl, Wl;           /* latent grid size                                           */
    int32_t n_focal, n_c;     /* 1 (broadcast) or SB (per object)            models.py:207-212 */
    float img_w, img_h;       /* net.image_shape = (W, H)                    models.py:116-117 */
    void *mv_workspace;       /* NS > 1: pnr_mv_workspace_bytes() bytes of device scratch, caller-owned: the view sum of
                                 every forward entry that takes this scene (eval, render, _split, _train); NS == 1: unused.
                                 Launches that share one scene must be ordered on one stream. */
} PnrScene;

/* One ResnetFC (src/model/resnetfc.py:66-130) at the only shape the reference ships:
 * d_in=42, d_latent=512, d_hidden=512, n_blocks=5, combine_layer=3, d_out=4, ReLU, average
 * (or max) pooling.  nn.Linear layout: weight (out, in) row-major, bias (out). */
typedef struct PnrMlpWeights {
    const float *lin_in_w, *lin_in_b;       /* (512,42), (512)  */
    const float *lin_z_w[3], *lin_z_b[3];   /* (512,512), (512) */
    const float *fc0_w[5], *fc0_b[5];       /* blocks[b].fc_0   */
    const float *fc1_w[5], *fc1_b[5];       /* blocks[b].fc_1   */
    const float *lin_out_w, *lin_out_b;     /* (4,512), (4)     */
    int32_t combine_max;                    /* pooling over the source views (util.combine_interleaved, util.py:461-471):
                                               0 = "average" (every shipped config), 1 = "max" (inference entries only) */
    int32_t stream_scale_log2;              /* ABI rev 11.  s in [0, 30], honoured by pnr_pack_mlp_split only: the PNR_PREC_F16X3
                                               inference kernels carry the hidden stream (x and the block-internal net of
                                               resnetfc.py:66-88, 147-184) at 2^-s of its value -- see "stream scale" below.
                                               0 = off.  Every other pack entry and every training entry refuses a non-zero
                                               value (PNR_E_INVALID); the exact fp32 inference entries ignore it. */
} PnrMlpWeights;

/* What a launch of ONE split-operand (PNR_PREC_F16X3) network takes beyond its blob and tables (ABI rev 12; host struct).  A NULL
 * pointer = every field zero = the plain launch.  The library keeps none of this between calls: a launch is a function of its
 * arguments.  See "fp16-range guard" and "stream scale and range probe" below. */
typedef struct PnrSplitAux {
    int32_t stream_scale_log2;  /* the s this network's blob was packed with (PnrMlpWeights.stream_scale_log2), in [0, 30] */
    unsigned int *sat_flag;     /* device, ONE 32-bit word, nullable: the fp16-range guard ORs this network's bits into it */
    float *range_probe;         /* device, 12 floats, nullable: the range probe's words of this network                    */
} PnrSplitAux;

const char *pnr_last_error(void);

/* Library / device facts (host out-params may be NULL). */
int pnr_version(int *major, int *minor);
/* ABI revision of THIS header: bumped whenever a struct layout or an entry point's argument list changes.  The
 * library returns the value it was compiled with; a binding must compare it with the header it was written against
 * before the first call (pixelnerf_amd/_lib.py does, and refuses a stale or foreign .so). */
#define PNR_ABI_VERSION 12
int pnr_abi_version(void);
int pnr_device_info(int *num_cus, int *lds_bytes_per_block);
/* Bytes of the multi-view scratch (PnrScene.mv_workspace, PnrBackwardDumps.mv_workspace) on the CURRENT device: one tile of
 * fp32 view-sum accumulators per workgroup, CUs x 96 x 512 x 4 (48 MiB on 256 CUs).  A multi-view call with a NULL
 * workspace fails with PNR_E_INVALID. */
size_t pnr_mv_workspace_bytes(void);

/* 64-bit content fingerprint of the 30 parameter tensors, computed and (optionally) compared on the device with no host
 * synchronisation: ws = pnr_params_checksum_ws_bytes() of device scratch, first 8 bytes zero (left so); sum_out (device,
 * nullable) receives it; with `expect`
 * (device) a differing value sets *mismatch_flag (device int) to 1.  Lets a caller that caches packed streams notice
 * parameter writes that bypass its cache key (the Python layer: `p.data.copy_()` bumps no tensor version). */
size_t pnr_params_checksum_ws_bytes(void);
int pnr_params_checksum(const PnrMlpWeights *w /*host*/, void *ws, unsigned long long *sum_out,
                        const unsigned long long *expect, int *mismatch_flag, void *stream);

/* ---- one-time weight repack ------------------------------------------------------------
 * Replaces nothing in the reference (it feeds nn.Linear weights to addmm directly,
 * resnetfc.py:147,175,55-62,183); needed because the fused kernel streams MFMA fragments.
 * Re-run whenever the parameters change.  `packed` must hold pnr_packed_mlp_bytes() bytes. */
size_t pnr_packed_mlp_bytes(void);
int pnr_pack_mlp(const PnrMlpWeights *w /*host struct of device ptrs*/, int precision,
                 void *packed, void *stream);

/* ---- folded inference form -------------------------------------------------------------------
 * lin_z[b] (resnetfc.py:175-180) acts on the bilinearly interpolated latent, and both are linear:
 * lin_z[b](sum_c w_c grid[c]) = sum_c w_c (W_z[b] grid[c] + b_z[b]) because the bilinear weights sum to 1.
 * pnr_fold_latent applies W_z[b] to every texel of the encoded grid once per scene and network (fp32 MFMA,
 * 3 tables of (SB*NS,Hl,Wl,512) 16-bit, pnr_folded_tables_bytes), pnr_pack_mlp_folded packs the stream
 * without the three lin_z GEMMs, and the *_folded entry points replace those GEMMs (22-28 % of the
 * per-point FLOPs) by one bilinear lookup per table.  Same results to the stated tolerance; inference
 * only.  Re-fold when the grid or the lin_z parameters change. */
size_t pnr_folded_tables_bytes(const PnrScene *scene /*host*/);
int pnr_fold_latent(const PnrScene *scene /*host*/, const PnrMlpWeights *w /*host*/, int precision,
                    void *tables, void *stream);
int pnr_pack_mlp_folded(const PnrMlpWeights *w /*host*/, int precision, void *packed /*pnr_packed_mlp_bytes()*/,
                        void *stream);
int pnr_eval_ray_samples_folded(const PnrScene *scene /*host*/, const void *packed_folded, const void *tables,
                                int precision, const float *rays, const float *z, int R, int rays_per_obj,
                                int K, float *rgbsigma, void *stream);
int pnr_eval_points_folded(const PnrScene *scene /*host*/, const void *packed_folded, const void *tables,
                           int precision, const float *xyz, const float *viewdirs, int B, float *rgbsigma,
                           void *stream);
int pnr_render_forward_folded(const PnrScene *scene /*host*/, const void *packed_coarse,
                              const void *tables_coarse, const void *packed_fine /*nullable*/,
                              const void *tables_fine, int precision, const float *rays, int R,
                              int rays_per_obj, int Kc, int Kf, int Kfd, float depth_std, int white_bkgd,
                              int lindisp, const float *u1, const float *u2, const float *u3,
                              const float *n4, float *rgb_c, float *depth_c, float *weights_c,
                              float *rgb_f, float *depth_f, float *weights_f, void *workspace,
                              const PnrSplitAux *aux_coarse /*host, nullable*/, const PnrSplitAux *aux_fine /*host, nullable*/,
                              void *stream);

/* ---- fp32-class accuracy on the f16 matrix cores (PNR_PREC_F16X3): same spans as the folded entries above
 * (src/model/models.py:146-266, src/model/resnetfc.py:132-184), any number of source views, inference.
 * w = wh + wl and x = xh + xl with f16 heads/tails, w x ~= wh xh + wh xl + wl xh accumulated in fp32 (error
 * 2^-22 per product instead of 2^-11); lin_z folded into fp32 per-texel tables.  Agrees with the reference's fp32
 * arithmetic to the bars of the exact-fp32 path (per-point |rgb| <= 2e-5) at several times the fp32-MFMA ceiling.
 * packed_split: pnr_packed_mlp_split_bytes() bytes from pnr_pack_mlp_split; tables_f32: pnr_folded_tables_f32_bytes()
 * bytes from pnr_fold_latent_f32 (layout of the 16-bit tables, 4 bytes per entry). */
size_t pnr_packed_mlp_split_bytes(void);
int pnr_pack_mlp_split(const PnrMlpWeights *w /*host*/, void *packed_split, void *stream);
size_t pnr_folded_tables_f32_bytes(const PnrScene *scene /*host*/);
int pnr_fold_latent_f32(const PnrScene *scene /*host*/, const PnrMlpWeights *w /*host*/, float *tables_f32,
                        unsigned int *sat_flag /*nullable: guard bit 12*/, void *stream);
/* The same tables for the texels ONE training pass reads (ABI rev 8).  A training step re-folds lin_z every pass -- the
 * weights moved -- and on a large grid most texels are not near any ray of the pass (DTU, 128 rays x 3 views: 37-43 k of
 * 90 k).  rays (R,8), z (R,K) = the pass's samples: every (view, point) is projected with the forward kernels' own code, its
 * four corner rows are marked, the marked rows are folded (same sums, same order: the bits of pnr_fold_latent_f32) and written
 * at their texels' places; all other rows of tables_f32 keep what they held -- hand in a buffer that was zero-initialised once
 * and use it only for a pnr_eval_ray_samples_split_train call on the SAME rays and z.  workspace:
 * pnr_fold_latent_f32_rows_workspace_bytes() bytes of device memory, 16-byte aligned, caller-owned (graph capture).
 * Takes grids of >= 8192 texels in total (smaller ones: pnr_fold_latent_f32 is one short launch). */
size_t pnr_fold_latent_f32_rows_workspace_bytes(const PnrScene *scene /*host*/);
int pnr_fold_latent_f32_rows(const PnrScene *scene /*host*/, const PnrMlpWeights *w /*host*/, const float *rays, const float *z,
                             int R, int rays_per_obj, int K, float *tables_f32, void *workspace, size_t workspace_bytes,
                             unsigned int *sat_flag /*nullable: guard bit 12*/, void *stream);
int pnr_eval_ray_samples_split(const PnrScene *scene /*host*/, const void *packed_split, const void *tables_f32,
                               const float *rays, const float *z, int R, int rays_per_obj, int K, float *rgbsigma,
                               const PnrSplitAux *aux /*host, nullable*/, void *stream);
int pnr_eval_points_split(const PnrScene *scene /*host*/, const void *packed_split, const void *tables_f32,
                          const float *xyz, const float *viewdirs, int B, float *rgbsigma,
                          const PnrSplitAux *aux /*host, nullable*/, void *stream);

/* encoder.latent NCHW -> NHWC (layout change for the lookup in src/model/encoder.py:80-109). */
int pnr_nchw_to_nhwc(const float *in, float *out, int N, int C, int H, int W, void *stream);

/* ---- ray sampling ------------------------------------------------------------------------
 * NeRFRenderer.sample_coarse, src/render/nerf.py:98-118.  rays (R,8), u1 (R,Kc) uniforms
 * (the reference's torch.rand_like at :111) -> z (R,Kc). */
int pnr_sample_coarse(const float *rays, const float *u1, int R, int Kc, int lindisp, float *z,
                      void *stream);

/* NeRFRenderer.sample_fine + sample_fine_depth + cat + sort, src/render/nerf.py:120-161 and
 * :285-295.  weights_c (R,Kc), depth_c (R), z_coarse (R,Kc); u2,u3 (R,Kimp) uniforms (:135,
 * :141), n4 (R,Kfd) normals (:158); Kimp = n_fine - n_fine_depth.  Either count may be 0
 * (the pointers are then ignored).  z_sorted (R, Kc+Kimp+Kfd) ascending.  depth_ranks (may be
 * NULL): (R,Kfd) position of every depth sample in z_sorted (training: the sort's permutation). */
int pnr_sample_fine(const float *rays, const float *weights_c, const float *depth_c,
                    const float *z_coarse, const float *u2, const float *u3, const float *n4,
                    int R, int Kc, int Kimp, int Kfd, float depth_std, int lindisp,
                    float *z_sorted, int32_t *depth_ranks, void *stream);

/* ---- the fused per-point network ---------------------------------------------------------
 * PixelNeRFNet.forward, src/model/models.py:146-266, including PositionalEncoding
 * (src/model/code.py:30-42), SpatialEncoder.index (src/model/encoder.py:80-109),
 * ResnetFC.forward (src/model/resnetfc.py:132-184), view mean pooling
 * (src/util/util.py:461-471) and the output activations (models.py:260-265).
 *
 * Variant A (renderer path; also fuses nerf.py:185,204 "points = o + z d, viewdirs = d"):
 *   rays (R,8), z (R,K) -> rgbsigma (R,K,4).  rays_per_obj = R / SB. */
int pnr_eval_ray_samples(const PnrScene *scene /*host*/, const void *packed, int precision,
                         const float *rays, const float *z, int R, int rays_per_obj, int K,
                         float *rgbsigma, void *stream);
/* Variant B (direct net(xyz, viewdirs) calls): xyz, viewdirs (SB,B,3) -> rgbsigma (SB,B,4). */
int pnr_eval_points(const PnrScene *scene /*host*/, const void *packed, int precision,
                    const float *xyz, const float *viewdirs, int B, float *rgbsigma,
                    void *stream);

/* ResnetFC.forward on explicit rows (src/model/resnetfc.py:132-184): zx (rows, 512 + 42) fp32 = [latent | code+viewdir]
 * per row, rows ordered [group][view][point] with combine_inner_dims = (NS, B) (mean over the NS views before block 3,
 * util.py:461-471; NS = 1: no pooling, B ignored beyond divisibility).  out (rows / NS, 4) is lin_out's RAW output
 * (no sigmoid / relu: those are PixelNeRFNet.forward's, models.py:260-265).  Unfused fp32 linears, same kernels as the
 * exact-fp32 path below; workspace = pnr_resnetfc_forward_f32_workspace_bytes(rows, NS). */
size_t pnr_resnetfc_forward_f32_workspace_bytes(long long rows, int NS);
int pnr_resnetfc_forward_f32(const PnrMlpWeights *w /*host*/, const float *zx, long long rows, int NS, int B, float *out,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ---- nn.Linear as a stand-alone operator pair ----------------------------------------------------
 * One `nn.Linear` of ResnetFC / ResnetBlockFC (src/model/resnetfc.py:53-62: fc_0, fc_1, shortcut; :147,175-183: lin_in, lin_z,
 * scale_z, lin_out) with the ReLU in front of it and the residual behind it folded in, for ANY rows / d_in / d_out: the
 * operator the host side composes ResnetFCs of NON-shipped shapes from (the shipped 42+512 -> 512 x 5 -> 4 shape runs in the
 * fused kernels above).
 *   Y (rows, d_out) = [Yin +] [relu](X (rows, d_in)) W^T + b      W (d_out, d_in) as nn.Linear stores it; b, Yin nullable;
 *                                                                 Yin may alias Y
 * precision PNR_PREC_F32: exact fp32 products (v_mfma_f32_32x32x2_f32); PNR_PREC_F16X3: fp32-class split operands on the f16
 * matrix cores (~6x faster, the arithmetic of the fused fp32-class kernels). */
int pnr_linear(const float *X, const float *W, const float *b /*nullable*/, const float *Yin /*nullable*/, float *Y, long long rows,
               int d_in, int d_out, int relu_in, int precision, void *stream);
/* its backward (what torch autograd derives for the lines above):
 *   dX (rows, d_in)  = (dY W) . [X > 0 if relu_in]      (nullable)
 *   dW (d_out, d_in) = dY^T [relu](X),  db (d_out) = sum_rows dY      (nullable; db only together with dW)
 * The reduction over the rows is split into fixed slices summed in a fixed order (bit-reproducible, no atomics):
 * workspace = pnr_linear_backward_workspace_bytes(d_in, d_out), needed when dW is requested.
 * PNR_PREC_F16X3 carries dY as fp16 (head, tail) pairs at a power-of-two scale: grad_scale = device [s, 1/s] from
 * pnr_grad_scale(dY) (required for that precision, ignored for PNR_PREC_F32). */
size_t pnr_linear_backward_workspace_bytes(int d_in, int d_out);
int pnr_linear_backward(const float *dY, const float *X, const float *W, long long rows, int d_in, int d_out, int relu_in,
                        float *dX /*nullable*/, float *dW /*nullable*/, float *db /*nullable*/, const float *grad_scale /*device [s,1/s]*/,
                        void *workspace, size_t workspace_bytes, int precision, void *stream);

/* ---- exact-fp32 evaluation (validation grade) --------------------------------------------------
 * Same contract as pnr_eval_ray_samples / pnr_eval_points (PixelNeRFNet.forward, models.py:161-265)
 * with every operand in fp32: unfused, one GEMM launch per nn.Linear on the fp32 MFMA, activations
 * in HBM.  Takes the raw nn.Linear tensors (no repack).  Results track the reference's fp32 path
 * to rounding level; throughput is ~1/20 of the 16-bit fused kernel.  The points are processed in
 * chunks sized by the workspace: pnr_eval_f32_workspace_bytes(NS, chunk_points) bytes hold one
 * chunk of chunk_points points (>= 64). */
size_t pnr_eval_f32_workspace_bytes(int NS, long long chunk_points);
int pnr_eval_ray_samples_f32(const PnrScene *scene /*host*/, const PnrMlpWeights *w /*host*/,
                             const float *rays, const float *z, int R, int rays_per_obj, int K,
                             float *rgbsigma, void *workspace, size_t workspace_bytes, void *stream);
int pnr_eval_points_f32(const PnrScene *scene /*host*/, const PnrMlpWeights *w /*host*/,
                        const float *xyz, const float *viewdirs, int B, float *rgbsigma,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- training (autograd) support -------------------------------------------------------------
 * The reference trains through this path with plain autograd (train/train.py:199-215): MSE on
 * coarse + fine rgb, gradients w.r.t. both ResnetFCs and encoder.latent.  Here:
 *   forward : pnr_eval_ray_samples_train = pnr_eval_ray_samples + 16-bit dumps of every linear
 *             layer's input operand (PnrTrainDumps);
 *   backward: pnr_composite_backward (d rgb/depth/weights -> d rgbsigma per point),
 *             pnr_mlp_backward (fused data-gradient chain with transposed weight streams: consumes
 *             d(pre-activation output), writes the per-layer output gradients dY as 16-bit rows),
 *             pnr_latent_scatter (d interpolated latent -> d feature grid, bilinear scatter-add);
 *             pnr_weight_grad_batched / pnr_lin_out_grad (dW = dY^T X, db = sum dY from those dumps),
 *             pnr_depth_sample_backward (the position gradient of the depth samples, nerf.py:292).
 * Array shapes: rows_v = NS*P for per-view layers (row = view*P + point), rows_p = P pooled;
 * 512-wide dims of activation dumps / gradients are in "storage order" (pnr_storage_perm). */
typedef struct PnrTrainDumps {
    void *d_in;     /* (rows_v, 64)  lin_in operand: code(39) | viewdir(3) | 0-pad, natural order */
    void *d_z;      /* (rows_v, 512) interpolated latent, natural channel order                  */
    void *d_a[5];   /* relu(x) in front of blocks[b].fc_0: b<3 (rows_v,512), b>=3 (rows_p,512)   */
    void *d_n[5];   /* relu(net) in front of blocks[b].fc_1, same shapes                         */
    void *d_x5;     /* (rows_p, 512) relu(x) in front of lin_out                                 */
    void *d_mask;   /* pnr_train_masks_bytes(P, NS) bytes: 1 bit per element of the 11 activation dumps ("was dumped non-zero"
                       = the relu derivative), 64-bit word per (layer, view, 64-point tile, kernel thread); what the
                       backward chain reads instead of the 1 KiB dump rows (which only the weight-gradient GEMMs read) */
} PnrTrainDumps;
size_t pnr_train_masks_bytes(long long P, int NS);

typedef struct PnrBackwardDumps {
    void *g_fc1[5]; /* dL/d(blocks[b].fc_1 output) = dL/d(residual stream after block b), shapes as d_n */
    void *g_fc0[5]; /* dL/d(blocks[b].fc_0 output), shapes as d_a                                */
    void *g_x0;     /* (rows_v, 512) dL/d(residual stream in front of block 0) = dY of lin_in, lin_z[0] */
    float *d_zlat;  /* (rows_v, 512) fp32, natural channel order: d(interpolated latent) = sum_b dY_b W_z[b]
                       (resnetfc.py:175-180 backward), unscaled; REQUIRED (pnr_mlp_backward rejects NULL)     */
    float *d_in;    /* (rows_v, 42) fp32: d(positional code | view direction) = dY W_in (resnetfc.py:147
                       backward), unscaled; NULL = not wanted                                            */
    void *mv_workspace; /* NS > 1: pnr_mv_workspace_bytes() bytes of device scratch (required); NS == 1: unused */
} PnrBackwardDumps;

int pnr_eval_ray_samples_train(const PnrScene *scene /*host*/, const void *packed, int precision,
                               const float *rays, const float *z, int R, int rays_per_obj, int K,
                               float *rgbsigma, const PnrTrainDumps *dumps /*host*/, void *stream);

/* feature index held at storage position e (0..511) of an activation dump row: perm[e]. host out. */
int pnr_storage_perm(int32_t *perm512 /*host*/);

/* transposed weight streams for the backward chain (fc_1^T, fc_0^T of every block, lin_out^T). */
size_t pnr_packed_mlp_bwd_bytes(void);
int pnr_pack_mlp_bwd(const PnrMlpWeights *w /*host struct of device ptrs*/, int precision,
                     void *packed_bwd, void *stream);

/* Backward of pnr_composite (src/render/nerf.py:178-182,223-249 under autograd).
 * d_depth / d_weights may be NULL.  d_rgbsigma (R,K,4) = dL/d(model output) after sigmoid/relu,
 * or, with pre_activation != 0, dL/d(lin_out output) (through rgb = sigmoid(.), sigma = relu(.),
 * src/model/models.py:260-263) -- the g_out that pnr_mlp_backward consumes;
 * d_z (R,K) (may be NULL) = dL/dz through the deltas and depth = sum w z. */
int pnr_composite_backward(const float *rays, const float *z, const float *rgbsigma, int R, int K,
                           int white_bkgd, const float *d_rgb, const float *d_depth,
                           const float *d_weights, float *d_rgbsigma, float *d_z,
                           int pre_activation, void *stream);

/* dL/dz of the sample positions through the network inputs (x = o + z d: positional code,
 * models.py:169-182 / code.py:37-41, and projection + bilinear lookup, models.py:206-215 /
 * encoder.py:96-109 with grid_sample's border-clip gradient).  d_in42 (rows_v,42) and d_zlat
 * (rows_v,512) fp32 are dL/d(lin_in operand) and dL/d(interpolated latent); d_z (R,K) is
 * accumulated (atomic adds; caller zero-initialises or passes the compositing d_z). */
int pnr_position_backward(const PnrScene *scene /*host*/, const float *rays, const float *z, int R,
                          int rays_per_obj, int K, const float *d_in42, const float *d_zlat,
                          float *d_z, void *stream);

/* The same gradient for the DEPTH samples only -- the only sample positions that carry gradient in the reference (the
 * importance samples are drawn from detached weights, nerf.py:288; z = clamp(depth_c + n4 * depth_std), nerf.py:157-160,292)
 * -- pushed through the sort and the clamp towards dL/d(coarse depth): for ray r, depth sample j at sorted position
 * ranks[r][j] and view v, contrib[v][r][j] = [near < depth_c[r] + n4[r][j] depth_std < far] * (network term of view v
 * [+ dz_comp[r][ranks[r][j]] for v = 0]); dL/d depth_c[r] = sum over (v, j) -- left to the caller so that the sum has a
 * fixed order.  dz_comp (R,K) = the compositing dL/dz of pnr_composite_backward (nullable); contrib (NS,R,Kfd) out. */
int pnr_depth_sample_backward(const PnrScene *scene /*host*/, const float *rays, const float *z, int R, int rays_per_obj,
                              int K, const int *ranks, const float *n4, int Kfd, const float *depth_c, float depth_std,
                              const float *d_in42, const float *d_zlat, const float *dz_comp, float *contrib, void *stream);

/* pnr_composite_backward plus d_far (R) (nullable) = dL/d(far) through the last delta far - z_{K-1} (nerf.py:181). */
int pnr_composite_backward_far(const float *rays, const float *z, const float *rgbsigma, int R, int K,
                               int white_bkgd, const float *d_rgb, const float *d_depth,
                               const float *d_weights, float *d_rgbsigma, float *d_z, float *d_far,
                               int pre_activation, void *stream);

/* Gradients with respect to the rays and the source cameras of one network pass (torch autograd through
 * src/render/nerf.py:98-249 and src/model/models.py:161-215): per (view, sample) the world-space gradient of the point
 * p = o + z d through the positional code of R_v p, the projection of R_v p + t_v and the bilinear lookup, and of the
 * view direction R_v d; summed in a fixed order (no atomics: bit-reproducible).
 *   d_rays (R,8): d origin, d direction, d near, d far.  dL/dz of a sample (network term over all views + dz_comp) goes
 *     to near / far through z = near (1-s) + far s (lindisp: 1/z linear in s; nerf.py:98-148); depth samples (ranks) only
 *     where their clamp is active (nerf.py:157-160) -- unclamped ones belong to pnr_depth_sample_backward.  d_far (R)
 *     of pnr_composite_backward_far is added to column 7.
 *   d_poses (SB*NS,3,4): d of the world->camera [R | t] in the scene; d_focal (n_focal,2), d_c (n_c,2): d of the scene's
 *     focal (fy negated as stored) and principal point, each summed over the rows it is broadcast to.
 * Nullable: dz_comp, d_far, ranks (with n4, depth_c, Kfd), d_rays, d_poses, d_focal, d_c.
 * workspace: pnr_camera_backward_workspace_bytes(R, K, rays_per_obj, NS) bytes. */
size_t pnr_camera_backward_workspace_bytes(int R, int K, int rays_per_obj, int NS);
/* The sampling part of that reduction alone, for renderers around an arbitrary model (points built by the caller):
 * dz (R,K) = dL/d(sample positions) -> d_rays (R,8) with columns 0..5 zero, near / far as above (z = near (1-s) + far s,
 * lindisp: 1/z linear in s, nerf.py:98-148; the depth samples at `ranks` only where their clamp is active,
 * nerf.py:157-160), plus d_far (R) (nullable).  A ray with near == far has every z equal to both, so s cannot be recovered
 * from z: each sample's dz goes half to near and half to far (d near + d far = sum dz, exact for both maps; the same in
 * pnr_camera_backward).  Nullable: ranks (with n4, depth_c, Kfd), d_far. */
int pnr_sample_bounds_backward(const float *rays, const float *z, const float *dz, int R, int K, int lindisp,
                               const int *ranks, const float *n4, int Kfd, const float *depth_c, float depth_std,
                               const float *d_far, float *d_rays, void *stream);
int pnr_camera_backward(const PnrScene *scene /*host*/, const float *rays, const float *z, int R, int rays_per_obj,
                        int K, int lindisp, const float *d_in42, const float *d_zlat, const float *dz_comp,
                        const float *d_far, const int *ranks, const float *n4, int Kfd, const float *depth_c,
                        float depth_std, float *d_rays, float *d_poses, float *d_focal, float *d_c,
                        void *workspace, void *stream);

/* Fused data-gradient chain of one ResnetFC (reverse of src/model/resnetfc.py:132-184).
 * g_out (P,4) = dL/d(lin_out output) (pre sigmoid/relu), grad_scale = power of two the chain is
 * run at (16-bit range management; every dump is scaled by it).  NS = views per object. */
int pnr_mlp_backward(const void *packed_bwd, int precision, const PnrTrainDumps *fwd /*host*/,
                     const float *g_out, float grad_scale, const float *grad_scale_dev /*nullable:
                     device scalar that overrides grad_scale (no host sync to pick it)*/,
                     long long P, int NS, const PnrBackwardDumps *out /*host*/, void *stream);

/* Picks that scale on the device: scales[0] = 2^e with e = 6 - ceil(log2 max|g|) (1 for g == 0), scales[1] =
 * 2^-e; both NaN when g holds a non-finite value (the gradients then come out NaN).  g: n floats, any 4-byte alignment.
 * e is clamped to [-100, 100]: both scales stay finite NORMAL powers of two for a vanishing (subnormal-range) or a huge
 * gradient (unclamped, 2^e overflows to inf for max|g| < 2^-121 and the step dies of 0 * inf); with the clamp a maximum below
 * 2^-94 is scaled to max|g| 2^100 < 2^6 and one above 2^106 to max|g| 2^-100 > 2^6, still exactly.  A subnormal max|g| counts
 * (it is not flushed to zero).  At a maximum that IS a power of two, 2^k, ceil(log2) = k: the scaled maximum is 2^6 itself;
 * otherwise it lies in (2^5, 2^6) (log2 is evaluated in fp32: a maximum a few last places above 2^k may still count as 2^k). */
int pnr_grad_scale(const float *g, long long n, float *scales /*device, 2 floats*/, void *stream);

/* Weight gradient of one 512x512 linear from the 16-bit dumps: dW (512,512) fp32 = out_scale *
 * dY^T X, db (512) fp32 = out_scale * column sums of dY (db may be NULL); dY, X (rows,512) 16-bit
 * row-major at `precision`.  Split over row slices with a fixed-order reduction (bit-reproducible);
 * workspace: pnr_weight_grad_workspace_bytes().  rows_storage_order / cols_storage_order: dY / X
 * columns are in storage order (pnr_storage_perm); dW and db are always written in feature order. */
size_t pnr_weight_grad_workspace_bytes(void);
int pnr_weight_grad(const void *dY, const void *X, long long rows, int precision, float out_scale,
                    int rows_storage_order, int cols_storage_order, float *dW, float *db,
                    void *workspace, void *stream);

/* The same for up to 16 linears in ONE launch pair (all 13 512x512 layers of a ResnetFC): fewer, fuller
 * launches and 4-8x fewer split slices to reduce.  jobs: host array.
 * workspace: pnr_weight_grad_batched_workspace_bytes(n_jobs, largest rows of the jobs).
 * precision PNR_PREC_F16X3: dY and X are (head | tail) f16 row sets (the tail array behind the head array), three MFMAs per
 * product -- the fused fp32-class training path. */
typedef struct PnrWeightGradJob {
    const void *dY, *X;          /* (rows,512) 16-bit row-major dumps                  */
    long long rows;
    int rows_storage_order, cols_storage_order;
    float *dW, *db;              /* (512,dw_cols), (512) fp32 outputs; db may be NULL */
    int x_cols;                  /* columns (= row stride) of X: 0 -> 512; 64 for the lin_in operand (natural order) */
    int dw_cols;                 /* columns (= row stride) of dW written: 0 -> x_cols; 42 for lin_in                 */
} PnrWeightGradJob;
size_t pnr_weight_grad_batched_workspace_bytes(int n_jobs, long long max_rows);
int pnr_weight_grad_batched(const PnrWeightGradJob *jobs /*host*/, int n_jobs, int precision,
                            float out_scale, const float *out_scale_dev /*nullable device scalar,
                            multiplies out_scale*/, void *workspace, void *stream);

/* lin_out (4 x 512): dW = g_out^T x5, db = column sums of g_out; g_out (P,4) fp32 = dL/d(lin_out output),
 * x5 (P,512) 16-bit dump (storage order); dW written in feature order.  Fixed-order reduction. */
size_t pnr_lin_out_grad_workspace_bytes(void);
int pnr_lin_out_grad(const float *g_out, const void *x5, long long P, int precision, float *dW,
                     float *db, void *workspace, void *stream);

/* d(encoder.latent) += bilinear scatter of d_zlat (rows_v,512) fp32 (natural channel order) to
 * d_latent_nhwc (SB*NS,Hl,Wl,512) fp32 (caller zero-initialises; accumulates).  Grids of up to 2274
 * texels per image (32 x 32 and the like) are accumulated in fp64 LDS slabs, one per (image, 16- / 8-channel slice),
 * fed per ray segment (consecutive samples in one grid cell); a slab reaches HBM with plain read-add-write when one
 * workgroup owns its (image, slice), and with one atomic per touched element otherwise -- never more than two workgroups
 * per pair (the slice width follows the image count), so onto a ZEROED buffer the result is bit-reproducible.  Larger grids
 * (64 x 64, DTU's 150 x 200) are cut into tiles of 32 x 32 texels: one owner workgroup per (image, tile, 16-channel slice)
 * takes the segments whose corners touch its tile from a binned list and writes the tile back with plain read-add-write
 * (every texel has one owner; fp64 sums, no HBM atomics).  Objects of 2^29 samples or more, grids of more than 8192 tiles
 * and PIXELNERF_SCATTER_TILED=0 take global fp32 atomics (order-dependent in the last bit).
 * workspace: pnr_latent_scatter_workspace_bytes() bytes of device memory, 16-byte aligned (projected positions, segment
 * lists, tile lists; 0 only on the global-atomic path, workspace may then be NULL), owned by the caller so that the call can
 * sit inside a HIP-graph capture (ABI rev 7; rev 6 kept a per-stream scratch inside the library).  (encoder.py:96-109 backward) */
size_t pnr_latent_scatter_workspace_bytes(const PnrScene *scene /*host*/, int R, int rays_per_obj, int K);
/* 1 when this call shape takes the tiled form (one owner workgroup per grid element, plain read-add-write): several calls may
 * then accumulate into ONE buffer order-independently (a training step's fine and coarse pass); 0: give every call its own
 * zeroed buffer and sum them for a bit-reproducible gradient (ABI rev 8) */
int pnr_latent_scatter_single_owner(const PnrScene *scene /*host*/, int R, int rays_per_obj, int K);
int pnr_latent_scatter(const PnrScene *scene /*host*/, const float *rays, const float *z, int R,
                       int rays_per_obj, int K, const float *d_zlat, float *d_latent_nhwc, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ---- alpha compositing -------------------------------------------------------------------
 * NeRFRenderer.composite after the model call, src/render/nerf.py:178-182 and :223-249.
 * rays (R,8), z (R,K), rgbsigma (R,K,4) -> weights (R,K) (may be NULL), rgb (R,3), depth (R). */
int pnr_composite(const float *rays, const float *z, const float *rgbsigma, int R, int K,
                  int white_bkgd, float *weights, float *rgb, float *depth, void *stream);

/* ---- whole renderer forward --------------------------------------------------------------
 * NeRFRenderer.forward, src/render/nerf.py:251-303 (inference; no autograd).
 * Noise pointers follow the reference's draw order (u1 :111, u2 :135, u3 :141, n4 :158).
 * packed_fine == NULL falls back to the coarse network (models.py:242); the fine pass then evaluates only the Kf
 * new samples and merges them with the coarse pass's outputs at the Kc shared positions (same network, same
 * points: bit-identical to evaluating all Kc+Kf).
 * Outputs: *_c (coarse), *_f (fine; ignored when Kf == 0); weights pointers may be NULL.
 * workspace: pnr_render_workspace_bytes(R,Kc,Kf) bytes of scratch. */
size_t pnr_render_workspace_bytes(int R, int Kc, int Kf);
int pnr_render_forward(const PnrScene *scene /*host*/, const void *packed_coarse,
                       const void *packed_fine, int precision, const float *rays, int R,
                       int rays_per_obj, int Kc, int Kf, int Kfd, float depth_std,
                       int white_bkgd, int lindisp, const float *u1, const float *u2,
                       const float *u3, const float *n4, float *rgb_c, float *depth_c,
                       float *weights_c, float *rgb_f, float *depth_f, float *weights_f,
                       void *workspace, void *stream);

/* ---- next-row helpers -----------------------------------------------
 * util.gen_rays / unproj_map, src/util/util.py:113-143,238-276 (ndc=False).
 * poses (NV,4,4) camera-to-world -> rays (NV,H,W,8). */
int pnr_gen_rays(const float *poses, int NV, int W, int H, float fx, float fy, float cx, float cy,
                 float z_near, float z_far, float *rays, void *stream);
/* Its backward (src/util/util.py:238-276 under torch autograd): d rays (NV,H,W,8) -> d camera-to-world [R | t]
 * (NV,3,4): d t = sum of d origin, d R = sum of d direction (x) unprojected pixel direction; fixed-order sum per pose.
 * The intrinsics are constants. */
int pnr_gen_rays_backward(const float *d_rays, int NV, int W, int H, float fx, float fy, float cx, float cy,
                          float *d_poses, void *stream);

/* ---- counter-based random draws (production mode; SURVEY.md 7 "hard parts", nerf.py:111,135,141,158) ------------
 * The reference draws its jitter / importance / depth-sample noise with four torch.rand launches per call.  The
 * seeded entries below draw inside the sampling kernels instead: Philox4x32-10, key = 64-bit seed, counter =
 * (global ray id, value index / 4, draw id), uniforms = 24 random bits in [0,1), normals by Box-Muller.  A value
 * depends only on (seed, global ray id, draw, index): an image does not change with chunking or with sharding
 * the rays across GPUs (ray_id_offset / ray_id_stride place a shard inside the whole ray set: id =
 * (r / rays_per_obj) * ray_id_stride + r % rays_per_obj + ray_id_offset; 0 / 0 = the call IS the whole set).
 * pnr_philox_noise writes the same draws out as the explicit tensors of pnr_render_forward (u1 (R,Kc), u2, u3
 * (R,Kimp), n4 (R,Kfd)); pnr_philox_raw is the bare block function on the host, for known-answer tests. */
int pnr_philox_noise(unsigned long long seed, long long ray_id_offset, int ray_id_stride, int rays_per_obj, int R,
                     int Kc, int Kimp, int Kfd, float *u1, float *u2, float *u3, float *n4, void *stream);
int pnr_philox_raw(const uint32_t *counter4 /*host*/, const uint32_t *key2 /*host*/, uint32_t *out4 /*host*/);
/* NeRFRenderer.forward (nerf.py:251-303) with in-kernel draws; tables_* NULL = unfolded streams. */
int pnr_render_forward_seeded(const PnrScene *scene /*host*/, const void *packed_coarse, const void *tables_coarse,
                              const void *packed_fine /*nullable*/, const void *tables_fine, int precision,
                              const float *rays, int R, int rays_per_obj, int Kc, int Kf, int Kfd, float depth_std,
                              int white_bkgd, int lindisp, unsigned long long seed, long long ray_id_offset,
                              int ray_id_stride, float *rgb_c, float *depth_c, float *weights_c, float *rgb_f,
                              float *depth_f, float *weights_f, void *workspace,
                              const PnrSplitAux *aux_coarse /*host, nullable*/, const PnrSplitAux *aux_fine /*host, nullable*/,
                              void *stream);

/* ---- next-row helpers (continued): render whole target views ----------
 * util.gen_rays + NeRFRenderer.forward in ONE call (what eval/eval.py:247-279 and eval/gen_video.py do per
 * object: build all rays of the target views on the host, copy, render): poses_c2w (NV,4,4) device, views
 * grouped per object (NV = SB * views_per_object).  The rays are NOT materialised: the sampling, network and
 * compositing kernels regenerate the ray of a pixel from (pose, intrinsics, pixel id) where they need it, in
 * gen_rays' operation order (bit-identical to pnr_gen_rays + pnr_render_forward).  tables_* NULL = unfolded
 * streams.  Noise: explicit tensors laid out as in pnr_render_forward with R = NV*H*W, or all four NULL ->
 * in-kernel draws from `seed` (ray id = pixel index in the (NV,H,W) order). */
size_t pnr_render_views_workspace_bytes(int NV, int W, int H, int Kc, int Kf);
int pnr_render_views(const PnrScene *scene /*host*/, const void *packed_coarse, const void *tables_coarse,
                     const void *packed_fine /*nullable*/, const void *tables_fine, int precision,
                     const float *poses_c2w, int NV, int W, int H, float fx, float fy, float cx, float cy,
                     float z_near, float z_far, int Kc, int Kf, int Kfd, float depth_std, int white_bkgd,
                     int lindisp, const float *u1, const float *u2, const float *u3, const float *n4,
                     unsigned long long seed, float *rgb_c, float *depth_c, float *weights_c, float *rgb_f,
                     float *depth_f, float *weights_f, void *workspace,
                     const PnrSplitAux *aux_coarse /*host, nullable*/, const PnrSplitAux *aux_fine /*host, nullable*/, void *stream);

/* ---- fp16-range guard of the fp32-class ("f16x3") kernels ---------------------------------------
 * The split-operand kernels carry every operand as an fp16 (head, tail) pair: values up to 65504 are
 * represented to ~2^-22, beyond that the head SATURATES (MODE.FP16_OVFL) and the result silently leaves
 * the reference's arithmetic class (src/model/resnetfc.py:132-184 computes in fp32, whatever the
 * magnitude).  Random-init networks stay four orders of magnitude below the limit; a checkpoint need not.
 * A launch whose PnrSplitAux.sat_flag is non-NULL runs the instantiation that follows the largest operand
 * head produced (one v_pk_maximum3_f16 per four values in the split epilogue, 1.15 % of the kernel; a head
 * of 65504 means a value >= 65488) and ORs into that ONE word:
 *   bit 2b    a value >= 65504 in relu(x) entering blocks[b].fc_0        (b = 0..4)
 *   bit 2b+1  a value >= 65504 in relu(net) entering blocks[b].fc_1
 *   bit 10    a value >= 65504 in the stream in front of lin_out
 *   bit 11    a non-finite network output
 *   bit 12    (pnr_fold_latent_f32 / _rows, through their own sat_flag argument) a feature-grid value or lin_z weight
 *             beyond the fp16 range
 * The word is per network: the render entries take one struct for the coarse and one for the fine network, and a
 * caller that wants the two apart passes two words (pixelnerf_amd: word 0 coarse, word 1 fine).  With packed_fine == NULL
 * (the merge path) both launches of the coarse network use aux_coarse.  The word is zeroed by the caller and read back by
 * the caller (asynchronously: pixelnerf_amd copies it to pinned memory and looks at it on the next call, like the
 * parameter check).  The guard never changes a result.  pnr_eval_ray_samples_split_train reports the same bits. */

/* ---- stream scale and range probe of the fp32-class ("f16x3") kernels ----------------------------
 * ReLU is positively homogeneous, so the hidden stream of a ResnetFC (src/model/resnetfc.py:147-184: x, and
 * net / dx inside every block, resnetfc.py:66-88) can be carried at c = 2^-s of its value and undone exactly in
 * front of lin_out's bias (resnetfc.py:183, src/model/models.py:258-265).  A network packed with
 * PnrMlpWeights.stream_scale_log2 = s > 0 (pnr_pack_mlp_split) must be LAUNCHED with PnrSplitAux.stream_scale_log2 = s:
 * that selects the scaled instantiation in every PNR_PREC_F16X3 inference entry (pnr_eval_points_split,
 * pnr_eval_ray_samples_split, pnr_render_forward_folded / _seeded, pnr_render_views; single- and multi-view, the merge
 * path of a NULL fine network included).  A blob is position-independent bytes -- it may be copied, moved to another
 * device or restored from a file -- and the library remembers nothing about it: the caller passes the s it packed with.
 * A launch at another s than the blob's computes with biases packed for the wrong scale, and nothing reports it.  All
 * four scale sites are fp32 and exact -- nothing that is stored as fp16 is shifted:
 *   x *= c          after lin_in + table 0 (lin_in's bias included)         resnetfc.py:147, 175-180 (b = 0)
 *   x += c * t      tables 1 and 2 (one FMA; the tables in memory are unscaled) resnetfc.py:175-180 (b = 1, 2)
 *   c * bias        blocks[b].fc_0 / fc_1 biases, at pack time               resnetfc.py:81-82
 *   sum * 2^(s-t)   the lin_out partial sum, BEFORE lin_out's bias           resnetfc.py:183
 * t: lin_out's weights are packed LIFTED by 2^t (the largest t in [0, 30] with max |W_out| 2^t <= 2^14; exact, in fp32, in
 * front of the head/tail split).  A network with a large hidden stream has a correspondingly small lin_out, whose fp16 tails
 * -- at 1e-6 even its heads -- are subnormal; the lift moves them up into the normal range.  The hidden weights are untouched.
 * A blob packed with s = 0 and launched with s = 0 (or a NULL struct) runs the unscaled instantiations: the bits of revision 10.
 * What a scale does NOT cure: guard bit 12 (grid values / lin_z weights themselves beyond 65504).
 * Every entry refuses an s outside [0, 30]; pnr_eval_ray_samples_split_train refuses s != 0 (no training at a stream scale);
 * the render entries refuse a struct with any field set at a precision other than PNR_PREC_F16X3 (all PNR_E_INVALID, before
 * any device work).
 *
 * A launch whose PnrSplitAux.range_probe is non-NULL runs a calibration instantiation (at any s) that follows the fp32 values
 * entering the (head, tail) split with v_max3_f32 and, at the end of each workgroup, does one atomic max per layer on the
 * bit pattern of the non-negative float.  range_probe: DEVICE array of 12 floats per network, zeroed by the caller:
 *   words 0..10  largest value that entered the operand image of layer l (the numbering of the guard's bits 0..10),
 *                in TRUE units (the kernel multiplies by 2^s)
 *   word 11      non-zero if a network output was NaN / inf (the guard's bit 11)
 * Downstream of a saturated layer the probe under-reports (the products used clamped heads): calibrate
 * iteratively.  A calibration tool, not a timed path.  The guard, when given its word too, keeps reporting.
 * pnr_eval_ray_samples_split_train has no probe form and ignores the pointer. */

/* ---- SpatialEncoder.index as a stand-alone operator ------------------------------------------
 * src/model/encoder.py:80-109 (SpatialEncoder.index): F.grid_sample(latent, uv[:, :, None], mode "bilinear",
 * padding_mode "border", align_corners=True)[..., 0] on the encoded grid -- latent_nhwc (NV,Hl,Wl,C) is the
 * channel-last copy (pnr_nchw_to_nhwc / pnr_pyramid_to_latent), uv (NV,N,2) the NORMALISED coordinates in
 * [-1,1] (x, y) the reference forms at encoder.py:96-99 (`uv * latent_scaling / image_size - 1`),
 * out (NV,C,N) as the reference returns it.  ATen's corner arithmetic in its operation order; a NaN
 * coordinate reads texel 0 (what the fused kernels do, pinned by the adv_plane golden).  The fused
 * network kernels do not call this: they gather the same rows themselves.
 * _backward: d_latent_nhwc (NV,Hl,Wl,C) is ACCUMULATED into (zero it first; fp32 atomics), d_uv (NV,N,2) is
 * written; either may be NULL.  Gradient through the border clip as ATen's clip_coordinates_set_grad
 * (zero outside the open interval (0, size-1)). */
int pnr_grid_index(const float *latent_nhwc, int NV, int Hl, int Wl, int C, const float *uv, long long N,
                   float *out, void *stream);
int pnr_grid_index_backward(const float *latent_nhwc, int NV, int Hl, int Wl, int C, const float *uv,
                            long long N, const float *g_out, float *d_latent_nhwc, float *d_uv, void *stream);

/* ---- PositionalEncoding as a stand-alone operator --------------------------------------------
 * src/model/code.py:30-42 (PositionalEncoding.forward): x (N, d_in) ->
 * out (N, d_out), d_out = d_in * (2 num_freqs + (include_input ? 1 : 0)):
 *   out[n] = [x[n]] ++ sin(phases2[j] + x[n][d] * freqs2[j]),  j = 0 .. 2 num_freqs - 1 outer, d inner,
 * freqs2 / phases2 = DEVICE arrays of 2 num_freqs floats: the module's `_freqs` / `_phases` buffers
 * (code.py:24-28: every frequency twice, phases 0 and pi/2), so a loaded checkpoint's buffers are
 * what is evaluated.  The sine argument is one fused multiply-add (ATen's addcmul).  The fused
 * kernels do not call this: they form the code of their own 3-vectors in registers.
 * _backward: g_x (N, d_in) = d/dx of sum(out * g_out)  (torch autograd of the same lines). */
int pnr_positional_encoding(const float *x, long long N, int d_in, int num_freqs, const float *freqs2,
                            const float *phases2, int include_input, float *out, void *stream);
int pnr_positional_encoding_backward(const float *x, const float *g_out, long long N, int d_in,
                                     int num_freqs, const float *freqs2, const float *phases2,
                                     int include_input, float *g_x, void *stream);

/* ---- next-row helpers: encoder output formatting --------------------
 * src/model/encoder.py:150-163: F.interpolate(bilinear, align_corners=True) of every ResNet stage
 * to stage 0's size + channel concat.  stages: HOST array of n_stages device pointers, stage s is
 * (NV, channels[s], heights[s], widths[s]) NCHW fp32; channels multiples of 64.  Writes the grid
 * channel-last (NV, H0, W0, sum channels) -- the layout PnrScene.latent_nhwc wants -- and, if
 * latent_nchw != NULL, the reference's NCHW `latent` tensor as well, in one pass. */
int pnr_pyramid_to_latent(const float *const *stages, const int *channels, const int *heights,
                          const int *widths, int n_stages, int NV, float *latent_nhwc,
                          float *latent_nchw, void *stream);

/* Backward of the above: src/model/encoder.py:150-163 under autograd (upsample_bilinear2d backward of
 * every stage + the cat's channel slicing).  d_latent is the gradient of the grid, channel-last
 * (NV, H0, W0, sum channels) -- the layout pnr_latent_scatter produces -- or, with d_latent_is_nchw != 0,
 * (NV, sum channels, H0, W0).  d_stages: HOST array of n_stages device pointers, d_stages[s] is
 * (NV, channels[s], heights[s], widths[s]) NCHW fp32; EVERY element is written (the caller does not zero
 * it, nothing is accumulated).  A texel gathers h * w * g over the output pixels whose forward read it,
 * with the forward's fp32 indices and weights, in a fixed order and without atomics: two calls give the
 * same bits.  Accepts exactly what pnr_pyramid_to_latent accepts (d_latent 16-byte aligned). */
int pnr_pyramid_to_latent_backward(const float *d_latent, int d_latent_is_nchw, float *const *d_stages,
                                   const int *channels, const int *heights, const int *widths,
                                   int n_stages, int NV, void *stream);

/* ---- the encoder's ResNet trunk for inference (added within ABI rev 12) ----------------------
 * src/model/encoder.py:111-164 over torchvision's BasicBlock trunk (resnet18 / resnet34), batch norm in eval mode folded
 * into a per-channel affine.  Everything is fp32 in and out, NCHW, contiguous.
 *
 * pnr_conv2d_affine: convolution + affine + optional residual + optional ReLU in one call,
 *   y[n,co,oy,ox] = act( (sum_{ci,ky,kx} x[n,ci, oy s + ky - p, ox s + kx - p] w[co,ci,ky,kx]) scale[co] + shift[co]
 *                        + res[n,co,oy,ox] )
 *   x (N,Cin,H,W); w (Cout,Cin,k,k) in torch's order; scale, shift (Cout); res (nullable) and y (N,Cout,Ho,Wo);
 *   Ho = (H + 2p - k) / s + 1 floored, likewise Wo; p = k / 2 (3, 1, 0 for k = 7, 3, 1); zeros lie outside the image;
 *   act = ReLU when relu != 0, else the identity.  (k, s) is one of (7,2), (3,1), (3,2), (1,2); Cin is 3 or a multiple of 64;
 *   Cout is a multiple of 64.  y must not overlap x, res or the workspace.
 *   THE BATCH-NORM FOLD is the caller's: scale = gamma / sqrt(var + eps), shift = beta - mean scale, formed in fp64 and
 *   rounded to fp32 once.
 *   ARITHMETIC: exact fp32 -- fp32 operands, one fused multiply-add per term, fp32 accumulation; acc scale + shift is one
 *   fused multiply-add, the residual one addition.  No 16-bit operands, no (head, tail) splits.
 *   DETERMINISM: no atomics.  The K = Cin k k terms of an output element are taken in ascending (ci, ky, kx).  The
 *   reduction is cut into S contiguous slices (S = 1 below K = 1152, else min(8, K / 576)) of ceil(K / S) terms rounded up
 *   to 64, and every slice into four equal quarters; a quarter is one chain started from zero, the quarters of a slice are
 *   added in ascending order, then the slices in ascending order in a second pass.  pnr_conv2d_affine_slices(Cin, k) = 4 S
 *   is the number of partial sums that meet in one element.  That order is a function of (Cin, k) alone: never of N, H, W,
 *   the tile an element falls in or the launch.  Hence two calls give equal bytes, and image n of a batch gets the bytes it
 *   gets when it is sent alone.
 *   workspace: pnr_conv2d_affine_workspace_bytes(...) bytes of device scratch, the caller's (0 for S = 1, then
 *   workspace may be NULL; else S x the output's size); the size entry answers 0 for a shape the entry refuses.
 * pnr_maxpool2d_3x3s2: nn.MaxPool2d(3, 2, 1).  x (N,C,H,W) -> y (N,C,Ho,Wo), Ho = (H - 1) / 2 + 1.  The padding never wins
 *   the maximum; the maximum is exact, so the output equals torch's bit for bit.
 * PNR_E_INVALID, before any HIP call: a null pointer (res excepted) or one that is not 4-byte aligned; N < 0 or another
 *   size <= 0; a (ksize, stride) outside the four pairs; channel counts outside the rule; N Ho Wo >= 2^31; a workspace
 *   that is too small.  N = 0 is a no-op. */
int pnr_conv2d_affine_slices(int Cin, int ksize);
size_t pnr_conv2d_affine_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride);
int pnr_conv2d_affine(const float *x, int N, int Cin, int H, int W, const float *w, const float *scale,
                      const float *shift, int Cout, int ksize, int stride, const float *res /*nullable*/, int relu,
                      float *y, void *workspace, size_t workspace_bytes, void *stream);
int pnr_maxpool2d_3x3s2(const float *x, int N, int C, int H, int W, float *y, void *stream);

/* One convolution of the trunk with its folded batch norm (host struct of device pointers). */
typedef struct PnrConvRecord {
    const float *w;       /* (cout, cin, ksize, ksize) */
    const float *scale;   /* (cout) gamma / sqrt(var + eps) */
    const float *shift;   /* (cout) beta - mean scale       */
    int32_t cin, cout, ksize, stride;
} PnrConvRecord;

/* The whole trunk as one host loop over the two entries above (SpatialEncoder._stages): the stem (7x7 / 2, ReLU) gives
 * level 0, BEFORE the pool; then, if use_first_pool, the max pool; then residual stage i = 1 .. n_levels - 1 of blocks[i-1]
 * BasicBlocks (64, 128, 256, 512 channels; stages 2.. halve the size in their first block) gives level i.  A block is
 * relu(affine2(conv2(relu(affine1(conv1(x))))) + idt), idt = x or the block's 1x1 / 2 downsample convolution with its affine.
 *   convs: HOST array of n_convs records in the order the layers run: the stem; then per block its downsample (first block
 *     of stages 2, 3, 4 only), conv1, conv2.  n_convs = 1 + sum over the stages run of (2 blocks + [stage > 1]).
 *   blocks: HOST array of 4 block counts, (3,4,6,3) for resnet34, (2,2,2,2) for resnet18 (each in [1, 64]; all four are
 *     checked, the first n_levels - 1 are run);  n_levels in [1, 5] (the encoder's num_layers);
 *   images (NV,3,H,W); levels: HOST array of n_levels device pointers, level i is (NV, C_i, h_i, w_i) with C = 64, 64, 128,
 *     256, 512 and (h_i, w_i) = pnr_encoder_level_shape(H, W, i, use_first_pool) (host arithmetic only; level in [0, 4]):
 *     exactly what pnr_pyramid_to_latent takes;
 *   workspace: pnr_encoder_trunk_workspace_bytes(...) bytes of device scratch, the caller's (0 for a shape refused).
 * The determinism rules of pnr_conv2d_affine hold for the whole: equal bytes from call to call, and per image whatever NV.
 * PNR_E_INVALID, before any HIP call: a null or misaligned pointer (records' included); H, W <= 0 or NV < 0; n_levels or a
 * block count out of range; n_convs or a record that does not describe the layer at its place; a workspace that is too
 * small.  NV = 0 is a no-op. */
int pnr_encoder_level_shape(int H, int W, int level, int use_first_pool, int *h /*host*/, int *w /*host*/);
size_t pnr_encoder_trunk_workspace_bytes(const int *blocks /*host*/, int n_levels, int use_first_pool, int NV, int H, int W);
int pnr_encoder_trunk_forward(const PnrConvRecord *convs /*host*/, int n_convs, const int *blocks /*host*/, int n_levels,
                              int use_first_pool, const float *images, int NV, int H, int W, float *const *levels /*host*/,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---- the encoder's ResNet trunk under training (added within ABI rev 12) ---------------------
 * The same trunk with batch norm in BATCH mode and a backward for every layer (trainer.py:180 net.train(), Adam over
 * net.parameters()).  fp32 in and out, NCHW, contiguous; exact fp32 arithmetic (sums of the batch norm in fp64); no atomics;
 * every output element is written; no host synchronisation and no device -> host copy, so a forward + backward can be captured
 * into a HIP graph.  Every reduction runs in an order fixed by the layer's shape alone: two calls give equal bytes.
 *
 * pnr_batchnorm2d_train_forward:  v (N,C,H,W) the raw convolution output, M = N H W values per channel, numbered
 *   m = (n H + y) W + x.
 *     mean = sum v / M, var = sum (v - mean)^2 / M (biased), both accumulated in fp64 (order below);
 *     save_mean = fp32(mean), save_invstd = fp32(1 / sqrt(var + eps));
 *     xhat = (v - save_mean) save_invstd;  y = act(fma(xhat, gamma, beta) + res);   res nullable, act = ReLU when relu != 0;
 *     running_mean <- (1 - momentum) running_mean + momentum mean, running_var likewise with the unbiased M / (M - 1) var
 *     (formed in fp64, rounded once), when the two pointers are not NULL -- nn.BatchNorm2d in training mode.
 *   frozen != 0 is the module in eval() with grad enabled: mean and var ARE running_mean and running_var (required), nothing
 *   is updated.  M < 2 in batch mode is refused, as torch refuses it.
 *   ORDER: the M values are cut into S contiguous slices (S = 1 below M = 8192, else min(64, M / 4096)) of ceil(M / S) values
 *   rounded up to 256.  Within a slice thread t of 256 adds m = begin + t, + 256, ... ascending into one fp64 sum from +0;
 *   the 256 sums are folded a[t] += a[t + s], s = 128, 64, .., 1; the slices are added in ascending order.  A function of M alone.
 * pnr_batchnorm2d_backward:  g_y the gradient of y; y (nullable) the forward's output, given when the layer had a ReLU:
 *   g = g_y where y > 0, else 0 (g = g_y without y).  d_res (nullable) receives g: the residual branch's gradient.
 *     d_beta = sum g, d_gamma = sum g xhat (fp64, the product formed in fp64, the forward's order), rounded to fp32;
 *     d_v = gamma save_invstd (g - mean(g) - xhat mean(g xhat)), the two means rounded to fp32 first;
 *     frozen: d_v = gamma save_invstd g.
 *   d_v and d_res must not overlap g_y, y or v.
 *   workspace (both): pnr_batchnorm2d_*_workspace_bytes(N, C, H, W) bytes, 8-byte aligned, required.
 * pnr_conv2d_backward_data:  d_x[n,ci,iy,ix] = sum_{co,ky,kx} d_y[n,co,oy,ox] w[co,ci,ky,kx] over the (oy, ox) with
 *   oy s - p + ky = iy, ox s - p + kx = ix: a gather.  The K = Cout k k terms are taken in ascending (co, ky, kx), terms that
 *   do not exist enter as zeros, and K is cut into slices and quarters exactly as pnr_conv2d_affine cuts Cin k k:
 *   pnr_conv2d_affine_slices(Cout, k) partial sums meet in one element.  d_x == NULL is a no-op (the stem's is wanted only
 *   when the image requires grad).  Shapes as pnr_conv2d_affine (the forward layer's N, Cin, H, W, Cout, ksize, stride).
 * pnr_conv2d_backward_weight:  d_w[co,ci,ky,kx] = sum_{n,oy,ox} d_y[n,co,oy,ox] x[n,ci, oy s - p + ky, ox s - p + kx], the
 *   P = N Ho Wo terms in ascending p = (n Ho + oy) Wo + ox.  P is cut into S slices, S = 1 (P < 1024), 8 (P < 16384), else 64,
 *   of ceil(P / S) terms rounded up to 64, every slice into four quarters; quarters and slices are added as in the forward.
 *   pnr_conv2d_backward_weight_slices(P) = 4 S.  A function of P alone.  N >= 1.
 * pnr_maxpool2d_3x3s2_backward:  x (N,C,H,W) the pool's input, g_y (N,C,Ho,Wo) -> d_x (N,C,H,W).  A gather: an input pixel
 *   adds the gradients of the <= 4 windows that hold it and whose FIRST maximum in (ky, kx) scan order it is (the forward's
 *   rule and torch's: it decides the ties at 0 behind a ReLU), in ascending (oy, ox).  Equals torch's CPU result bit for bit.
 *   Needs no workspace.
 * PNR_E_INVALID, before any HIP call, the message prefixed with the entry's name: a null or misaligned pointer (the nullable
 *   ones excepted), a bad size or (ksize, stride), channel counts outside pnr_conv2d_affine's rule, N H W or N Ho Wo >= 2^31,
 *   M < 2 in batch mode, a workspace that is too small.  N = 0 is a no-op (refused by pnr_conv2d_backward_weight). */
size_t pnr_batchnorm2d_train_forward_workspace_bytes(int N, int C, int H, int W);
size_t pnr_batchnorm2d_backward_workspace_bytes(int N, int C, int H, int W);
int pnr_batchnorm2d_train_forward(const float *v, int N, int C, int H, int W, const float *gamma, const float *beta,
                                  float *running_mean /*nullable*/, float *running_var /*nullable*/, double eps,
                                  double momentum, int frozen, const float *res /*nullable*/, int relu, float *y,
                                  float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes,
                                  void *stream);
int pnr_batchnorm2d_backward(const float *g_y, const float *y /*nullable*/, const float *v, const float *save_mean,
                             const float *save_invstd, const float *gamma, int N, int C, int H, int W, int frozen,
                             float *d_v, float *d_gamma, float *d_beta, float *d_res /*nullable*/, void *workspace,
                             size_t workspace_bytes, void *stream);
size_t pnr_conv2d_backward_data_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride);
int pnr_conv2d_backward_data(const float *d_y, const float *w, int N, int Cin, int H, int W, int Cout, int ksize,
                             int stride, float *d_x /*nullable*/, void *workspace, size_t workspace_bytes, void *stream);
int pnr_conv2d_backward_weight_slices(long long P);
size_t pnr_conv2d_backward_weight_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride);
int pnr_conv2d_backward_weight(const float *d_y, const float *x, int N, int Cin, int H, int W, int Cout, int ksize,
                               int stride, float *d_w, void *workspace, size_t workspace_bytes, void *stream);
int pnr_maxpool2d_3x3s2_backward(const float *x, const float *g_y, int N, int C, int H, int W, float *d_x, void *stream);

/* One convolution of the trunk with its batch norm, for training (host struct of device pointers). */
typedef struct PnrConvTrainRecord {
    const float *w;        /* (cout, cin, ksize, ksize) */
    const float *gamma;    /* (cout) */
    const float *beta;     /* (cout) */
    float *running_mean;   /* (cout); nullable together with running_var unless frozen */
    float *running_var;
    float *d_w;            /* backward only: where the three gradients go, every element written */
    float *d_gamma;
    float *d_beta;
    double eps, momentum;
    int32_t cin, cout, ksize, stride;
} PnrConvTrainRecord;

/* The whole trunk forward and backward as host loops over the entries above and pnr_conv2d_affine (scale 1, shift 0: the raw
 * convolution) / pnr_maxpool2d_3x3s2; arguments as pnr_encoder_trunk_forward, the records in the same order.  The library owns
 * no memory: `saved` (pnr_encoder_trunk_train_saved_bytes, 8-byte aligned) receives in the forward what the backward reads --
 * every raw convolution, every layer output that is not a level, the pooled stem, every (mean, invstd) -- and must reach the
 * backward unchanged together with images and levels.  workspace: pnr_encoder_trunk_train_workspace_bytes, 8-byte aligned,
 * serves both calls and carries nothing between them.  frozen as in pnr_batchnorm2d_train_forward, for every batch norm.
 * Backward: d_levels (HOST array of n_levels device pointers, all required) are the gradients of the levels; a level's own
 * gradient is added last, (d_conv1 + d_identity) + d_level; d_images (NV,3,H,W) is nullable.  The forward updates the running
 * statistics of every record that has them (batch mode); num_batches_tracked is the caller's.
 * The bytes are those of the per-layer entries chained by hand.  Refusals as pnr_encoder_trunk_forward, plus M < 2 for any
 * batch norm in batch mode.  NV = 0 is a no-op. */
size_t pnr_encoder_trunk_train_saved_bytes(const int *blocks /*host*/, int n_levels, int use_first_pool, int NV, int H, int W);
size_t pnr_encoder_trunk_train_workspace_bytes(const int *blocks /*host*/, int n_levels, int use_first_pool, int NV, int H, int W);
int pnr_encoder_trunk_train_forward(const PnrConvTrainRecord *convs /*host*/, int n_convs, const int *blocks /*host*/,
                                    int n_levels, int use_first_pool, int frozen, const float *images, int NV, int H, int W,
                                    float *const *levels /*host*/, void *saved, size_t saved_bytes, void *workspace,
                                    size_t workspace_bytes, void *stream);
int pnr_encoder_trunk_backward(const PnrConvTrainRecord *convs /*host*/, int n_convs, const int *blocks /*host*/,
                               int n_levels, int use_first_pool, int frozen, const float *images, int NV, int H, int W,
                               const float *const *levels /*host*/, const float *const *d_levels /*host*/, const void *saved,
                               size_t saved_bytes, float *d_images /*nullable*/, void *workspace, size_t workspace_bytes,
                               void *stream);

/* ---- next-row helpers: eval epilogue on device ----------------------
 * eval/eval.py:283-290,327-329 and util.psnr (src/util/util.py:474-481): rgb (n_views,pixels,3) ->
 * clamp to [0,1] [-> uint8 = trunc(x*255)]; depth -> (d - z_near)/(z_far - z_near); per-view sum
 * of squared errors against gt_rgb (same shape, [0,1]) in fp64 (PSNR_v = -10 log10(sse_v /
 * (3*pixels))).  Every output pointer may be NULL. */
int pnr_eval_epilogue(const float *rgb, const float *depth, int n_views, int pixels_per_view,
                      float z_near, float z_far, const float *gt_rgb, unsigned char *rgb_u8,
                      float *rgb_clamped, float *depth_norm, double *sq_err_sum, void *stream);

/* eval/eval.py:321-326 (the structural-similarity call between the clamp and the PSNR; also
 * eval/calc_metrics.py:186-191): per-view mean SSIM with a uniform win_size x win_size window,
 * the second number of the reference's `final psnr ... ssim ...` line, on device.
 * pred, gt: (n_views, H, W, channels) fp32, channel-interleaved (pnr_eval_epilogue's layout with
 * pixels = H*W).  Per channel, in fp64 throughout: over every window that lies fully inside the
 * image (NP = win_size^2 pixels) the window means ux, uy, uxx, uyy, uxy of x, y, x^2, y^2, x*y;
 *   vx = cn (uxx - ux^2), vy = cn (uyy - uy^2), vxy = cn (uxy - ux uy), cn = NP / (NP - 1);
 *   C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2;
 *   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2));
 * ssim[v] = mean of S over the (H-win_size+1)(W-win_size+1) windows and the channels.  (A filter
 * with reflected borders cropped by (win_size-1)/2 -- the usual formulation -- is the same number.)
 * Reduction in a fixed order, no floating-point atomics: every workgroup (one 16x16 tile of window
 * positions of one channel of one view) writes ONE fp64 partial into `workspace`, a second pass
 * adds a view's partials in an order that depends on (H, W, channels) only -- bit-identical from
 * run to run, and a view's value does not depend on how many views share the call.
 * win_size odd, in [3, 15], <= min(H, W); channels in [1, 4]; data_range > 0; workspace: device
 * memory of at least pnr_ssim_workspace_bytes (the caller's; the library allocates nothing);
 * ssim: device, (n_views) fp64.  n_views == 0 is a no-op. */
size_t pnr_ssim_workspace_bytes(int n_views, int H, int W, int channels);
int pnr_ssim(const float *pred, const float *gt, int n_views, int H, int W, int channels,
             int win_size, double data_range, void *workspace, size_t workspace_bytes,
             double *ssim, void *stream);

/* ---- next-row helpers: training-ray selection on device ---------------
 * train/train.py:143-182 with util.bbox_sample (src/util/util.py:220-235): for each of SB objects
 * pick B pixels among its NV views and emit their rays and ground-truth colours (image*0.5+0.5)
 * directly -- the reference builds all NV*H*W rays per object to index 128 of them.
 * poses (SB,NV,4,4) camera-to-world; images (SB,NV,3,H,W) in [-1,1]; focal (SB,2) = (fx,fy);
 * c (SB,2) or NULL (image centre).  Random draws are inputs, in the reference's order:
 *   bboxes != NULL: bboxes (SB,NV,4) float [x0,y0,x1,y1]; ids (SB,B) int64 = randint(0,NV);
 *                   ux, uy (SB,B) = rand;   x = long(ux*(x1+1-x0)+x0), y likewise;
 *   bboxes == NULL: ids (SB,B) int64 = randint(0,NV*H*W) flat pixel indices; ux, uy ignored.
 * Out: rays (SB,B,8), rgb_gt (SB,B,3). */
int pnr_sample_training_rays(const float *poses, const float *images, const float *focal,
                             const float *c, const float *bboxes, const long long *ids,
                             const float *ux, const float *uy, int SB, int NV, int W, int H, int B,
                             float z_near, float z_far, float *rays, float *rgb_gt, void *stream);

/* ---- exact-fp32 TRAINING path (validation grade; precision "f32" under autograd).  The unfused fp32 chain of
 * pnr_eval_ray_samples_f32 with every activation the backward needs kept in fp32, and its backward on fp32 MFMA:
 * the fp32 yardstick of the 16-bit training kernels (ResnetFC.forward / autograd through it, src/model/resnetfc.py:132-184;
 * train/train.py:199-215).  rows_v = NS * P ordered [view][point], rows_p = P. */
typedef struct PnrF32Saved {
    float *in42;    /* (rows_v, 64)  lin_in operand: positional code | rotated view direction | 0 pad   */
    float *zlat;    /* (rows_v, 512) interpolated latent (operand of lin_z[0..2])                      */
    float *xin[5];  /* residual stream entering blocks[b] (after + lin_z[b]): b < 3 (rows_v,512), else (rows_p,512) */
    float *net[5];  /* blocks[b].fc_0 output (pre-relu), same shapes                                   */
    float *x5;      /* (rows_p, 512) residual stream in front of lin_out                               */
    float *pool_in; /* (rows_v, 512) residual stream after block 2, in front of the view mean; NS == 1: unused, may be NULL */
} PnrF32Saved;
/* split_gemm = 0: every product on the exact fp32 MFMA (precision "f32": the yardstick).  split_gemm = 1: the same chain with
 * every product formed from (head, tail) fp16 operand pairs -- 3 f16 MFMAs, fp32 accumulate, the arithmetic of
 * PNR_PREC_F16X3 -- about 6x faster at fp32-class accuracy (precision "f16x3" under autograd). */
int pnr_eval_ray_samples_f32_train(const PnrScene *scene /*host*/, const PnrMlpWeights *w /*host*/, const float *rays,
                                   const float *z, int R, int rays_per_obj, int K, float *rgbsigma,
                                   const PnrF32Saved *saved /*host*/, int split_gemm, void *stream);
/* ---- fp32-class TRAINING, fused (the default of precision "f16x3" under autograd).  Forward: the inference kernel of
 * PNR_PREC_F16X3 (one launch per network pass, lin_z through the folded fp32 tables) in its training instantiation, which also
 * keeps what the backward needs -- every 512-wide linear's operand as the (head, tail) f16 images the kernel multiplies from,
 * copied out of LDS, and 1-bit relu masks.  Backward: one launch for all 15 transposed products of the network (lin_out^T,
 * ten fc^T, lin_z[2..0]^T, lin_in^T; gradient images copied out the same way), one batched split-operand weight-gradient
 * launch pair over those images (pnr_weight_grad_batched at PNR_PREC_F16X3) and lin_out's 4 x 512 gradient.  Same reference
 * lines and the same accuracy class as the GEMM-per-layer entries above (the tests hold both to the same gradient bars).
 * "(head | tail)": two f16 arrays of the stated shape, the tail array directly behind the head array.  Storage order:
 * pnr_storage_perm.  packed_split = pnr_pack_mlp_split stream, tables_f32 = pnr_fold_latent_f32 tables of the CURRENT
 * parameters and grid (re-pack / re-fold after every optimizer step / encode()). */
typedef struct PnrSplitSaved {
    void *in_op;   /* (rows_v, 64)  (head | tail), natural order: lin_in operand (code | view direction | 0 pad) */
    void *zlat;    /* (rows_v, 512) (head | tail), natural channel order: interpolated latent                     */
    void *a[5];    /* relu(x) entering blocks[b].fc_0, (head | tail) rows in storage order: b < 3 (rows_v,512), else (rows_p,512) */
    void *n[5];    /* relu(fc_0 output) entering blocks[b].fc_1, same shapes                                       */
    float *x5;     /* (rows_p, 512) fp32, natural order: residual stream in front of lin_out                       */
    void *masks;   /* pnr_train_masks_bytes(P, NS) bytes: 1-bit relu masks of the 11 activations                   */
} PnrSplitSaved;
int pnr_eval_ray_samples_split_train(const PnrScene *scene /*host*/, const void *packed_split, const void *tables_f32,
                                     const float *rays, const float *z, int R, int rays_per_obj, int K, float *rgbsigma,
                                     const PnrSplitSaved *saved /*host*/, const PnrSplitAux *aux /*host, nullable*/, void *stream);
/* grad_scale = device [s, 1/s] from pnr_grad_scale(g_out); outputs as pnr_mlp_backward_f32 (d_zlat required, d_in and grads
 * nullable: grads == NULL runs the data-gradient chain only, without the weight-gradient launches).  With NS > 1 the workspace
 * also holds the multi-view scratch. */
size_t pnr_mlp_backward_split_workspace_bytes(long long P, int NS);
int pnr_mlp_backward_split(const PnrMlpWeights *w /*host*/, const PnrSplitSaved *saved /*host*/, const float *g_out, long long P,
                           int NS, const PnrMlpWeights *grads /*host*/, float *d_zlat, float *d_in /*nullable*/,
                           const float *grad_scale, void *workspace, size_t workspace_bytes, void *stream);
/* All parameter gradients of one ResnetFC + d(interpolated latent) [+ d(lin_in operand)] from g_out (P,4) =
 * dL/d(lin_out output): `grads` holds device pointers of the 30 gradient tensors in PnrMlpWeights' layout (same shapes as
 * the parameters, overwritten) or NULL (data gradients only: pose refinement with a frozen network, src/model/models.py:161-215
 * differentiated with respect to the inputs alone -- no weight-gradient launch); d_zlat (rows_v,512), d_in (rows_v,42) or NULL. */
size_t pnr_mlp_backward_f32_workspace_bytes(long long P, int NS);
/* split_gemm = 1 additionally takes grad_scale = device [s, 1/s] from pnr_grad_scale(g_out): the gradient chain runs at the
 * power-of-two scale s (fp16 range of the operand heads), results are un-scaled exactly on their way out. */
int pnr_mlp_backward_f32(const PnrMlpWeights *w /*host*/, const PnrF32Saved *saved /*host*/, const float *g_out, long long P,
                         int NS, const PnrMlpWeights *grads /*host*/, float *d_zlat, float *d_in, int split_gemm,
                         const float *grad_scale, void *workspace, size_t workspace_bytes, void *stream);

/* The feature phase of the exact-fp32 path on its own -- PositionalEncoding.forward (src/model/code.py:30-42) on the
 * rotated point + the rotated view direction (src/model/models.py:161-196) and SpatialEncoder.index
 * (src/model/encoder.py:80-109) -- for B points per object: in42 (NS*SB*B, 64) = [code(39) | R d (3) | zero pad],
 * zlat (NS*SB*B, 512), rows ordered [view][object][point].  What lin_in / lin_z consume in pnr_eval_points_f32. */
int pnr_point_features_f32(const PnrScene *scene /*host*/, const float *xyz, const float *viewdirs, int B,
                           float *in42, float *zlat, void *stream);

/* ---- mesh extraction (src/util/recon.py; the grid of src/util/util.py:93-110) ----------------
 * src/util/recon.py:43,54 with src/util/util.py:93-110: rows first .. first+count of
 * util.gen_grid((c1x,c2x,nx), (c1y,c2y,ny), (c1z,c2z,nz), ij_indexing=True) -- x the slowest
 * axis -- with every coordinate np.linspace(lo, hi, n, dtype=float32)'s value (numpy's fp64
 * expression restated: i * ((hi-lo)/(n-1)) + lo, the last point = hi, cast to float32).
 * c1, c2 (doubles), reso: HOST arrays of 3.  xyz (count,3) device.  viewdirs (count,3) device or
 * NULL: the reference's "fake" direction -p/|p| (recon.py:54) in fp32.  Deviation: a point of
 * norm 0 gets (0,0,0), not the reference's 0/0 = NaN. */
int pnr_gen_grid_points(const double *c1 /*host*/, const double *c2 /*host*/, const int *reso /*host*/,
                        long long first, long long count, float *xyz, float *viewdirs /*nullable*/,
                        void *stream);

/* src/util/recon.py:68-78 (where the reference calls PyMCubes on the host): marching cubes on a
 * density grid, on device.  field (nx,ny,nz) fp32, C-contiguous (sigmas.view(*reso)).
 *   inside   : a corner is inside iff its value is finite and > iso (== iso is outside; a
 *              non-finite value is outside and counted in n_nonfinite).
 *   vertices : an indexed mesh, one vertex per grid edge whose ends differ, shared by the cells
 *              around the edge; ordered by owning grid point (the edge's lower end, linear index
 *              (i ny + j) nz + k), then axis x, y, z.  From the lower end a to the upper end b:
 *              t = (iso - f_a) / (f_b - f_a) in fp32, computed once per edge (no cracks from
 *              rounding); a non-finite end cannot be interpolated through: the vertex sits on the
 *              finite end (t = 0 or 1).  Index space: (i,j,k) + t e_axis; output: index * scale + c1
 *              (separately rounded fp32).
 *   triangles: cells in ascending linear order, within a cell the case table's order; winding
 *              such that (v1 - v0) x (v2 - v0) points from inside to outside.
 *   tables   : corner c = dx + 2 dy + 4 dz (bit c of the case index = inside); edge e = 4 axis + r
 *              joins the corner whose other two coordinates, in axis order, are (r & 1, r >> 1)
 *              with its neighbour along axis.  On every cube face the patch boundary depends on the
 *              face's four flags alone; on an ambiguous face each inside corner is cut off on its
 *              own.  pnr_marching_cubes_tables (host): edge_mask[256] (bit e: edge e carries a
 *              vertex), tri[256*16] (up to five triangles as edge ids, -1 terminated).
 * pnr_marching_cubes_count classifies, takes the exclusive prefix sums (a hand-written integer
 * scan: block sums, a scan of the block sums, the add -- no atomics, the same bytes every run)
 * into `workspace` (device, 8-byte aligned, pnr_marching_cubes_workspace_bytes; the caller's) and
 * leaves counts_dev = [n_vertices, n_triangles, n_nonfinite] (3 ints, device; the last two
 * saturate at INT_MAX).  The library does not synchronise: the caller reads the counts, allocates
 * vertices (n_vertices,3) fp32 and triangles (n_triangles,3) int32 and calls
 * pnr_marching_cubes_emit with the SAME field, sizes, iso and workspace.  c1, scale: HOST arrays
 * of 3 floats.  PNR_E_INVALID for n < 2 on any axis and for 3 nx ny nz >= 2^31 (edge ids are
 * int32); the workspace size of such a grid is 0. */
size_t pnr_marching_cubes_workspace_bytes(int nx, int ny, int nz);
int pnr_marching_cubes_count(const float *field, int nx, int ny, int nz, float iso, void *workspace,
                             int *counts_dev, void *stream);
int pnr_marching_cubes_emit(const float *field, int nx, int ny, int nz, float iso,
                            const float *c1 /*host*/, const float *scale /*host*/,
                            const void *workspace, float *vertices, int *triangles, void *stream);
int pnr_marching_cubes_tables(int *edge_mask /*host, 256*/, int *tri /*host, 256*16*/);

/* ---- finishing a mesh: floater removal and vertex normals (added within ABI rev 12: no struct or argument list changed; ---
 * nothing in the reference corresponds: src/util/recon.py:68-106 meshes whatever the grid holds, writes bare vertices) ---
 * pnr_grid_components: the connected components of the inside voxels of a density grid.  field (nx,ny,nz) fp32,
 * C-contiguous, x the slowest axis (sigmas.view(*reso)).
 *   inside  : a voxel is inside iff its value is finite and > threshold -- the mesher's rule above: == threshold and
 *             NaN / +-inf are outside.
 *   joined  : 6-connectivity, the grid edges.  pnr_marching_cubes_* puts a vertex exactly on the edges whose ends differ
 *             under this rule, so two voxels are in one component iff the mesher joins them without a surface between.
 *   labels  : (nx,ny,nz) int32.  -1 outside; inside, the SMALLEST linear index (i ny + j) nz + k among the voxels of the
 *             voxel's component.  That makes the answer unique: the same bytes on every run, whatever the scheduling.
 *   sizes   : nullable; int32, one entry per voxel, written in full: the component's voxel count at the entry of its
 *             smallest index, 0 everywhere else (integer atomic adds, which commute exactly).
 *   counts_dev : nullable; 2 ints, device: [n_inside, n_components].
 * A lock-free union-find over `labels` in three launches in stream order (init, union, flatten; the two invariants that
 * bound every loop are stated in csrc/pnr_meshfinish.hip); no workspace, no workgroup waits on another.
 * PNR_E_INVALID: n < 1 on an axis (so a grid always has a voxel), nx ny nz >= 2^31, a NaN threshold (+-inf are
 * ordinary: nothing / every finite value is inside), a null field / labels. */
int pnr_grid_components(const float *field, int nx, int ny, int nz, float threshold, int *labels,
                        int *sizes /*nullable*/, int *counts_dev /*nullable, 2 ints*/, void *stream);
/* pnr_grid_normals: the field's gradient at mesh vertices, as unit normals; one thread per vertex, no atomics: the same
 * bytes on every run.  vertices (V,3) in world coordinates, as pnr_marching_cubes_emit wrote them with the same c1 and
 * scale (HOST arrays of 3 floats); normals (V,3).
 *   index coordinates : p = (v - c1) / scale per axis, clamped to [0, n - 1]; the cell is floor(p), clamped to n - 2;
 *                       the position in the cell is t = p - cell.
 *   grid gradient     : per axis the central difference (f[i+1] - f[i-1]) / 2, at the border the one-sided difference
 *                       f[1] - f[0] / f[n-1] - f[n-2].
 *   at the vertex     : the trilinear blend of the cell's eight grid-point gradients, a + t (b - a) along x, then y, then
 *                       z; component a is then divided by scale[a] (world units: the grid may be anisotropic, and
 *                       recon.marching_cubes(align_to_grid=False) deliberately uses the reference's (c2 - c1) / reso).
 *   normal            : -g / |g| -- from inside (high sigma) to outside, the direction the mesher's winding gives
 *                       (v1 - v0) x (v2 - v0); (0,0,0) where g is zero or not finite.
 * Separately rounded fp32 operations (no contraction); the norm and the final quotient go through fp64.
 * PNR_E_INVALID: n < 2 on an axis, nx ny nz >= 2^31, a zero or non-finite scale, a non-finite c1, V < 0, a null
 * pointer with V > 0.  V = 0: no-op. */
int pnr_grid_normals(const float *field, int nx, int ny, int nz, const float *c1 /*host*/, const float *scale /*host*/,
                     const float *vertices, long long V, float *normals, void *stream);

/* ---- occupancy-grid ray culling (inference; nothing in the reference corresponds: it renders every ray) --------
 * A density grid of one encoded object -- sigma at the points of util.gen_grid (src/util/util.py:93-110), the grid
 * src/util/recon.py:43-66 evaluates -- becomes a bitfield of occupied CELLS; rays are classified against it and only
 * those that can hit something are rendered.  A ray that passes through empty cells alone composites to the value
 * src/render/nerf.py:178-182,223-249 yields when every sigma is zero: weights 0, depth 0, rgb 0 (1 on every channel
 * with white_bkgd, nerf.py:244-247) -- what the caller fills in for the rays these entries cull.
 *
 * Geometry.  A field (nx,ny,nz) has (nx-1)(ny-1)(nz-1) cells.  Cell (i,j,k) has linear index
 * (i (ny-1) + j)(nz-1) + k; its bit is bit (index & 31) of word (index >> 5).  Per axis it spans
 * [c1 + i h, c1 + (i+1) h] with h = (c2 - c1) / (n - 1): the TRUE spacing of util.gen_grid (util.py:93-110), where the
 * densities were sampled -- not the (c2 - c1) / reso of src/util/recon.py:74.  c1, c2: HOST arrays of 3 floats, c1 < c2.
 *
 * pnr_occupancy_bytes: 4 x the number of 32-bit words of the bitfield; 0 for an invalid grid (n < 2 on an axis, or
 * 2^31 cells and more). */
size_t pnr_occupancy_bytes(int nx, int ny, int nz);
/* field (nx,ny,nz) fp32, C-contiguous (the sigmas of recon.py:66 viewed as the grid) -> bits.
 *   raw-occupied : a cell any of whose 8 corners is > threshold or is not finite (== threshold is empty).  NaN / +-inf
 *                  count as OCCUPIED: culling must err towards rendering.  This is deliberately the opposite of the mesher
 *                  above, where a non-finite corner is outside (recon.py:68-78).
 *   occupied     : a cell with a raw-occupied cell within Chebyshev distance `dilate` (0..4).
 * Every word of `bits` is written in full by ONE thread (no atomics: two calls give the same bytes); the unused high bits
 * of the last word are zero.  n_occupied_dev (device int, nullable): the number of occupied cells = the popcount of the
 * result, summed in a fixed order by a second, single-workgroup launch that needs no scratch (so there is no workspace
 * argument; pnr_ssim's partial sums need one).  PNR_E_INVALID: n < 2 on an axis, 2^31 cells or more, dilate outside
 * [0, 4], a NaN threshold, a null field / bits. */
int pnr_occupancy_build(const float *field, int nx, int ny, int nz, float threshold, int dilate, uint32_t *bits,
                        int *n_occupied_dev /*nullable*/, void *stream);
/* rays (R,8) [origin, direction, near, far] (the rows of util.gen_rays, util.py:238-276) against the bitfield: for the
 * segment o + t d, t in [near, far], over the occupied cells it passes through,
 *   hit[r] = 1 iff there is one, and then t_bounds[r] = (max(near, t_enter - pad), min(far, t_exit + pad)) with t_enter
 *            the smallest entry parameter and t_exit the largest exit parameter over those cells (both within
 *            [near, far]: an origin inside an occupied cell gives t_enter = near);
 *   hit[r] = 0 and t_bounds[r] = (near, far) otherwise.
 * Conservative on what it cannot classify: a ray with a non-finite component, a zero direction or near >= far gets
 * hit = 1 and unchanged bounds.  Zero direction components, origins inside the box or on a cell plane are ordinary.
 * One thread per ray: the segment is clipped to the box, then a 3-D DDA (Amanatides & Woo) walks its cells -- all of
 * them, the last occupied one is needed too -- at most (nx-1)+(ny-1)+(nz-1) of them.  Planes and parameters are
 * separately rounded fp32 operations, t = ((c1 + i h) - o) / d, never accumulated.  pad >= 0, finite. */
int pnr_occupancy_clip_rays(const float *rays, long long R, const uint32_t *bits, int nx, int ny, int nz,
                            const float *c1 /*host*/, const float *c2 /*host*/, float pad, float *t_bounds /*(R,2)*/,
                            int32_t *hit /*(R)*/, void *stream);
/* pnr_philox_noise for an arbitrary list of rays (nerf.py:111,135,141,158): row r of u1 (R,Kc), u2, u3 (R,Kimp), n4 (R,Kfd)
 * holds exactly the values the seeded entries draw for GLOBAL ray id ray_ids[r] (device, R int64; ids may repeat, be
 * unordered and exceed 2^31) -- what the renderer feeds the explicit-noise entries with when it renders the rays that
 * survived culling, so that a kept pixel has the bits of the dense render. */
int pnr_philox_noise_ids(unsigned long long seed, const long long *ray_ids, int R, int Kc, int Kimp, int Kfd, float *u1,
                         float *u2, float *u3, float *n4, void *stream);

/* ---- per-sample skipping against the same bitfield (inference): the network runs on the samples in occupied cells only.
 * The staged entries (pnr_sample_coarse, pnr_eval_ray_samples*, pnr_composite, pnr_sample_fine) launch the kernels of the
 * one-call renderer and a sample's world point is o + z d in separately rounded operations, so the one-sample "ray"
 * (rays[r], z[r,k]) is the same point as sample k of ray r in the dense call.  mark -> compact ->
 * pnr_eval_ray_samples*(rays_c, z_c, R = M, K = 1) -> expand -> pnr_composite is the dense pass with rgb sigma = 0 at every
 * sample the grid calls empty: bit for bit where a point's output does not depend on its place in the launch (the 16-bit
 * kernel, the exact fp32 path).  The split-operand kernel's last places depend on whether the point's place in the launch is
 * even or odd: there a caller keeps whole pairs (2j, 2j+1) of the dense launch in the list and drops the partner's output.
 *
 * pnr_occupancy_mark_samples: rays (R,8), z (R,K) -> keep (R,K) bytes, one thread per sample (consecutive samples of a
 * ray in consecutive lanes), no atomics.  The point is P[a] = o[a] + z d[a]: one multiply and one add, each rounded (the
 * operations of the network kernels' own sample point).  keep = 1 iff c1[a] <= P[a] <= c2[a] on all three axes AND the
 * bit of the point's cell is set; the cell is clamp(floorf((P[a] - c1[a]) / h[a]), 0, n[a] - 2) per axis, with the h of
 * pnr_occupancy_clip_rays (the fp32 rounding of the fp64 quotient (c2 - c1) / (n - 1)) -- the cell that entry assigns to
 * a point; a point on the c2 face belongs to the last cell.  A point outside the box is EMPTY (keep = 0), as a ray that
 * misses the box is culled.  A sample whose z, or any origin or direction component of whose ray, is not finite gets
 * keep = 1: culling errs towards rendering.  near and far (columns 6, 7) are not read.  c1, c2: HOST arrays, c1 < c2.
 * PNR_E_INVALID: R < 0, K < 1, R K >= 2^31, a bad grid (as pnr_occupancy_clip_rays), a null pointer.  R = 0: no-op. */
int pnr_occupancy_mark_samples(const float *rays, const float *z, int R, int K, const uint32_t *bits, int nx, int ny,
                               int nz, const float *c1 /*host*/, const float *c2 /*host*/, uint8_t *keep /*(R,K)*/,
                               void *stream);
/* Stable compaction of the marked samples.  With g_0 < g_1 < ... < g_{M-1} the sample ids (r K + k) whose keep != 0:
 *   index[m] = g_m,  rays_c[m] = rays[g_m / K] (all 8 floats, near and far included),  z_c[m] = z[g_m],  *count_dev = M.
 * index, rays_c (.,8) and z_c need room for M rows (R K always suffices); rows >= M are NOT written.  Three ordinary
 * launches in stream order -- per-workgroup totals (wave ballot + popcount), an exclusive scan of the totals by ONE
 * workgroup, the scatter -- and no workgroup waits on another; no atomics, so two calls give the same bytes.  Ray rows
 * move as two 16-byte accesses: rays and rays_c must be 16-byte aligned.  workspace: caller-owned device memory of
 * pnr_compact_samples_workspace_bytes(R K) bytes (4 per workgroup of 256 samples; 0 for N <= 0 or N >= 2^31), overwritten.
 * PNR_E_INVALID: R < 0, K < 1, R K >= 2^31, a null or misaligned pointer, a workspace that is too small.
 * R = 0: no-op (nothing is written, *count_dev included). */
size_t pnr_compact_samples_workspace_bytes(long long N);
int pnr_compact_samples(const uint8_t *keep, const float *rays, const float *z, int R, int K, int32_t *index,
                        float *rays_c, float *z_c, int *count_dev, void *workspace, size_t workspace_bytes, void *stream);
/* The inverse placement: rgbsigma (N,4) = rgbsigma_c[m] at row index[m] (m < M), (0,0,0,0) at every other row.  EVERY
 * element of rgbsigma is written (a zero fill, then the scatter, in stream order).  index: M distinct rows in [0, N), as
 * pnr_compact_samples writes them (an entry outside [0, N) is skipped, never written through).  M = 0 is valid (index and
 * rgbsigma_c may then be null) and gives all zeros.  Rows move as 16-byte accesses: rgbsigma and rgbsigma_c must be
 * 16-byte aligned.  PNR_E_INVALID: M < 0, N < 0, M > N, N >= 2^31, a null or misaligned pointer.  N = 0: no-op. */
int pnr_expand_rgbsigma(const int32_t *index, const float *rgbsigma_c /*(M,4)*/, int M, long long N,
                        float *rgbsigma /*(N,4)*/, void *stream);

/* ---- early ray termination (inference): the network is not run behind the point where a ray has gone opaque.
 * A pass with K sorted samples per ray is cut into stages at sample indices 0 = b_0 < b_1 < ... < b_S = K.  A ray STOPS at
 * the first boundary b_s, s >= 1, at which the transmittance in front of sample b_s,
 *   T = prod_{j < b_s} (1 - alpha_j + 1e-10),  alpha_j = 1 - exp(-delta_j relu(sigma_j)),  delta_j = z_{j+1} - z_j
 *   (delta_{K-1} = far - z_{K-1}; src/render/nerf.py:178-182,228-235, every operation in fp32 as pnr_composite performs it),
 * is <= eps; the samples k >= b_s of a stopped ray get rgb sigma = 0.  Stage by stage a caller runs
 *   pnr_termination_mark(stage) -> pnr_compact_samples -> pnr_eval_ray_samples*(rays_c, z_c, R = M, K = 1) -> placement of the
 *   kept samples into the (R,K,4) buffer, which starts as zeros,
 * and after the last stage one pnr_composite.  The result is pnr_composite of the dense pass's outputs with rgb sigma = 0 at
 * every sample behind its ray's stop, bit for bit (with the pair rule of the split-operand kernel stated above): the weights in
 * front of the stop are the dense weights, behind it they are 0, and the transmittance that is left goes to the background.
 * On a ray with every delta >= 0 the weights behind the stop and the final transmittance of the dense pass sum to T at the
 * stop (up to the K 1e-10 terms), so with rgb in [0,1] every channel moves by at most eps -- towards the background -- and
 * the depth by at most eps far.  A ray whose last sample lies beyond `far` has a negative last delta, hence a negative alpha
 * and a factor above 1: the identity holds for it, the bound does not.
 *
 * pnr_termination_mark: rays (R,8) (only `far`, column 7, is read), z (R,K), rgbsigma (R,K,4): the outputs so far.
 *   t_front[r] (nullable) = T in front of sample k_begin: exactly the value pnr_composite forms for that sample from the same
 *                buffer (chunks of 64 samples, a product scan per chunk, the chunk totals carried), 1 for k_begin = 0.  Only
 *                the sigmas of the samples < k_begin are read; z[r, k_begin] gives the last delta, `far` when k_begin = K.
 *   keep[r,k]  = 1 iff k_begin <= k < k_end, and not (t_front[r] <= eps), and keep_in is null or keep_in[r,k] != 0
 *                (keep_in (R,K) bytes: e.g. pnr_occupancy_mark_samples' answer).  A NaN transmittance does not stop the ray:
 *                the rule errs towards rendering.  EVERY byte of keep is written, 0 outside the stage.
 * One wavefront per ray, no atomics (two calls give the same bytes), no scratch, no LDS.  Later stages of a ray that has
 * stopped see zeros behind the stop, whose factors are exactly 1; a caller that must not depend on the last place of that
 * product also ANDs its own record of the stopped rays into keep, as the renderer does.
 * PNR_E_INVALID, before any HIP call: R < 0, K < 1, R K >= 2^31, not 0 <= k_begin <= k_end <= K, eps NaN or outside (0, 1),
 * a null rays / z / rgbsigma / keep (with R > 0).  R = 0: no-op. */
int pnr_termination_mark(const float *rays, const float *z, const float *rgbsigma /*(R,K,4)*/, int R, int K, int k_begin,
                         int k_end, float eps, const uint8_t *keep_in /*(R,K), nullable*/, uint8_t *keep /*(R,K)*/,
                         float *t_front /*(R), nullable*/, void *stream);

/* ---- baked volumes (inference; added within ABI rev 12: no struct or argument list changed; nothing in the reference
 * corresponds).  The network of ONE encoded object is evaluated once on the points of its grid, for colour as well as density,
 * and any number of views is rendered from the grid alone, with no network behind a pixel.  The image is an approximation of
 * the network's render: trilinear in space, one view direction per grid point, equidistant samples (no importance sampling).
 *
 * Volume.  vol (nx,ny,nz,4) fp32, C-contiguous, 16-byte aligned: (r, g, b, sigma) at the points of
 *   pnr_gen_grid_points(c1, c2, reso) -- x the slowest axis -- i.e. the geometry of the occupancy entries above: cells of the
 *   TRUE spacing h = (c2 - c1) / (n - 1), h rounded once from fp64.  Every axis has at least 2 points, the grid fewer than 2^31
 *   cells; all index arithmetic is 64-bit.  The values are the network's outputs (rgb after the sigmoid, sigma after the relu):
 *   the kernel applies no activation.  c1, c2: HOST arrays of 3 floats, c1 < c2.
 * Samples of a ray (o, d, near, far).  step > 0, a length in the units of z:
 *   n = ceil((far - near) / step),  t_i = near + (i + 0.5) step for i < n,  p_i = o + t_i d  (the product and the sum rounded
 *   separately: ray_point of csrc/pnr_geom.h).  The samples are anchored at `near`, not at the box.  A sample with a coordinate
 *   outside [c1, c2] on any axis, or not finite, has sigma = 0.  Inside the box, per axis u = (p - c1) / h, the cell is
 *   clamp(floor(u), 0, n - 2) and the position in it f = clamp(u - cell, 0, 1): because of the clamp no input can make the kernel
 *   read outside the volume.  The 8 corners are one 16-byte load each; all four channels are blended as a + f (b - a), along z
 *   (the 4 corner pairs, at f_z), then along y (at f_y), then along x (at f_x); every operation is rounded on its own.
 *   A ray that cannot be sampled -- near >= far, a non-finite origin, direction, near or far, n > 2^20 -- gets the background
 *   (rgb 0, or 1 with white_bkgd; depth 0; alpha 0) and does no volume reads.
 * Compositing: src/render/nerf.py:178-182,223-249 with a constant delta, in fp32:
 *   alpha_i = 1 - exp(-step sigma_i),  T_i = prod_{j<i} (1 - alpha_j + 1e-10),  w_i = alpha_i T_i,
 *   rgb = sum w_i c_i  (with white_bkgd (sum + 1) - sum w_i on every channel),  depth = sum w_i t_i,  alpha = sum w_i.
 *   One wavefront per ray: lane l of chunk c takes sample 64 c + l; T is an inclusive product scan across the lanes times the
 *   carry of the earlier chunks (pnr_composite's scan); the four sums are per-lane accumulators, reduced once at the end in a
 *   fixed butterfly order.  A chunk none of whose samples is inside the box (and occupied, below) issues no loads; all its
 *   factors are exactly 1, so it leaves the carry and the sums as they are.
 * Skipping.  bits (nullable): pnr_occupancy_build's bitfield of a field with the same nx, ny, nz.  A sample whose cell's bit is
 *   off has sigma = 0; it enters the product as the factor 1, in its own place.  Built from vol's sigma (>= 0) at threshold 0
 *   with dilate 0 this is exact: the 8 corners of an empty cell are 0, the blend is 0, alpha is 0 and the factor is exactly 1,
 *   so the renders with and without bits are equal bit for bit.  At a threshold > 0 the image changes where the dropped haze
 *   was visible.
 * Termination.  terminate = eps in [0, 1), 0: off.  Once the transmittance carried out of a chunk of 64 samples is <= eps the
 *   ray stops; what was left goes to the background.  With rgb in [0, 1] every channel and alpha move by at most eps and the
 *   depth by at most eps far (the argument of pnr_termination_mark above; the deltas here are all positive).  eps = 0 gives the
 *   bits of the plain render; a NaN transmittance does not stop a ray.
 * No atomics, no LDS, no workspace: two calls give the same bytes.  Outputs: rgb (R,3), depth (R), alpha (R) fp32.
 * pnr_baked_render_rays: rays (R,8) [origin, direction, near, far].  pnr_baked_render_views: poses (NV,4,4) camera-to-world and
 *   the intrinsics of pnr_gen_rays; R = NV H W rays ordered (view, row, column), each regenerated in the kernel with
 *   pnr_gen_rays' operations -- the same kernel, the same bits as pnr_baked_render_rays on pnr_gen_rays' rows, and no ray array
 *   is written.
 * PNR_E_INVALID, before any HIP call: a bad grid (as pnr_occupancy_clip_rays), step not finite or <= 0, terminate NaN or outside
 *   [0, 1), R < 0 / NV < 0 / W <= 0 / H <= 0, more than 2^33 rays, and with R > 0 a null rays / poses / vol / rgb / depth /
 *   alpha, a vol that is not 16-byte aligned, any other pointer that is not 4-byte aligned.  R = 0: no-op. */
int pnr_baked_render_rays(const float *rays, long long R, const float *vol, const uint32_t *bits /*nullable*/, int nx, int ny,
                          int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd,
                          float terminate, float *rgb /*(R,3)*/, float *depth /*(R)*/, float *alpha /*(R)*/, void *stream);
int pnr_baked_render_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                           float z_near, float z_far, const float *vol, const uint32_t *bits /*nullable*/, int nx, int ny,
                           int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd,
                           float terminate, float *rgb /*(NV H W,3)*/, float *depth, float *alpha, void *stream);

/* View-dependent baked volumes (added within ABI rev 12 as well).  Every grid point keeps a low-order function of the VIEW
 * DIRECTION instead of one value: real spherical harmonics up to degree L in {0, 1, 2} on all four channels, evaluated in the
 * march for each ray's own direction.  An SH render of a ray equals the RGBA render, by the rules above, of the volume "this
 * object seen from direction d": that sentence is the specification; what follows says how that volume's corners are computed.
 * Still trilinear in space, still equidistant samples, still nothing outside the box; degree <= 2; fp32 storage here, fp16
 * storage through the half entries below (the same march on the widened values).
 * Layout.  B = (L+1)^2 basis functions.  coef (nx,ny,nz,B,4) fp32, C-contiguous, 16-byte aligned: float4 k of a grid point holds
 *   (r_k, g_k, b_k, sigma_k); 16 B bytes per point (64 at degree 1, 144 at degree 2).  The grid, c1, c2, the cells and the point
 *   order are those of the RGBA volume.
 * Basis, normalised so that Y_0 = 1 (the integral of Y_j Y_k over the sphere is 4 pi delta_jk).  From the ray's direction
 *   (x, y, z) = d / sqrt(dx dx + dy dy + dz dz), the sum taken left to right; the constants rounded to fp32 once:
 *     Y_1 = sqrt(3) y,  Y_2 = sqrt(3) z,  Y_3 = sqrt(3) x,
 *     Y_4 = sqrt(15) (x y),  Y_5 = sqrt(15) (y z),  Y_6 = (sqrt(5)/2) (3 (z z) - 1),  Y_7 = sqrt(15) (x z),
 *     Y_8 = (sqrt(15)/2) (x x - y y).
 *   A direction whose squared norm is 0 or not finite gets Y_k = 0 for k >= 1.  Y is a per-ray constant.
 * Corner value.  At corner p, v = coef[p][0] Y_0 + coef[p][1] Y_1 + ... in this order, every product and every sum rounded on its
 *   own.  Then, PER CORNER AND BEFORE THE BLEND, a channel of rgb below 0 becomes 0 and one above 1 becomes 1, a sigma below 0
 *   becomes 0; a value inside its range keeps its bits.  A corner is B contiguous 16-byte loads, a pair of corners along z 2 B.
 * Everything else -- the sample count and positions, the inside test, the blend along z, y, x, alpha_i, the product scan, depth
 *   and alpha, white_bkgd, the termination check every 64 samples, the ray that cannot be sampled -- is the RGBA march, unchanged.
 * Consequences.  A volume whose coefficients k >= 1 are all zero, with rgb in [0, 1] and sigma >= 0, renders the same BYTES as
 *   pnr_baked_render_rays on coef[..., 0, :]: v_0 1 + 0 Y_k is exact and the clamps change nothing.  Degree 0 is that case by
 *   construction.
 * Skipping.  bits as above, of a field that bounds sigma over all directions: |Y_k| <= m_k = (sqrt 3, sqrt 3, sqrt 3, sqrt(15)/2,
 *   sqrt(15)/2, sqrt 5, sqrt(15)/2, sqrt(15)/2), so sigma at a corner never exceeds s_0 + sum_k m_k |s_k| (plus the rounding of Y
 *   and of the sum: util.bake.BakedSHVolume takes a factor 1 + 2^-16 on the sum).  A cell whose 8 corners have a bound <= 0 has
 *   sigma exactly 0 at all of them for every direction: built at threshold 0 with dilate 0 the skipped render equals the
 *   unskipped one bit for bit.
 * PNR_E_INVALID: what the two entries above refuse (coef in the place of vol), and a degree outside {0, 1, 2}. */
int pnr_baked_sh_render_rays(const float *rays, long long R, const float *coef /*(nx,ny,nz,B,4)*/, int degree,
                             const uint32_t *bits /*nullable*/, int nx, int ny, int nz, const float *c1 /*host*/,
                             const float *c2 /*host*/, float step, int white_bkgd, float terminate, float *rgb /*(R,3)*/,
                             float *depth /*(R)*/, float *alpha /*(R)*/, void *stream);
int pnr_baked_sh_render_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                              float z_near, float z_far, const float *coef /*(nx,ny,nz,B,4)*/, int degree,
                              const uint32_t *bits /*nullable*/, int nx, int ny, int nz, const float *c1 /*host*/,
                              const float *c2 /*host*/, float step, int white_bkgd, float terminate,
                              float *rgb /*(NV H W,3)*/, float *depth, float *alpha, void *stream);

/* Sparse baked volumes (added within ABI rev 12 as well).  The dense forms above keep 16 B bytes for every grid point, although the
 * skipped march reads only the corners of occupied cells.  The sparse form keeps the rows of exactly those points, renders the same
 * BYTES as the dense march with the same bits, and can be baked without evaluating the network anywhere else.
 * The kept set -- one definition, used by every entry below.  Grid (nx,ny,nz), P = nx ny nz points, linear id p = (i ny + j) nz + k
 *   (the order of pnr_gen_grid_points); bits: pnr_occupancy_build's bitfield of the cells of the same grid.
 *     corner[p] = 1 iff at least one of the up to 8 cells that have p as a corner has its bit on;
 *     keep[p]   = corner[p] | corner[p ^ 1], where p ^ 1 exists (an odd P: the last point has no partner).
 *   The second line is the closure over the pairs (2j, 2j+1) of the dense launch -- the pair rule of the per-sample skipping above:
 *   a compacted network launch over the kept points, in ascending order, has every point at a place of its own parity, the one
 *   thing a point's last bits depend on with the split-operand kernel.  So baking the kept points alone gives the dense bake's
 *   rows bit for bit at every precision.  ids (M) int32: the kept ids, ascending; index (nx,ny,nz) int32: index[p] = the rank of p
 *   in ids if kept, else -1.  What is stored IS the pair-closed set.  What the march relies on: in a cell whose bit is on, the two
 *   corners of a pair along z (p, p + 1) are both kept and adjacent in id, so index[p + 1] == index[p] + 1.
 * pnr_sparse_points_mark: bits -> keep (P) bytes as defined above.  One thread per PAIR (2j, 2j+1): the closure needs no second
 *   pass; no atomics, EVERY byte is written, two calls give the same bytes.  The prefix sum that turns keep into index and ids is
 *   the caller's (ops.sparse_points: one cumsum and one host read of M).  PNR_E_INVALID: what pnr_occupancy_bytes calls an invalid
 *   grid (n < 2 on an axis, 2^31 cells or more), 2^31 points or more (ranks are int32), a null pointer.
 * pnr_gen_grid_points_at: row m of xyz (count,3) and of viewdirs (count,3, nullable) holds the bits of row ids[m] of
 *   pnr_gen_grid_points(c1, c2, reso, 0, P, ...), coordinates and fake view directions alike (one device function computes a row
 *   in both entries).  An id outside [0, P) gives a row of NaN.  PNR_E_INVALID: a null c1 / c2 / reso, reso < 1 on an axis, a
 *   non-finite c1 / c2, count < 0, and with count > 0 a null ids / xyz or a pointer that is not 4-byte aligned.  count = 0: no-op.
 * pnr_baked_sparse_render_rays / pnr_baked_sparse_render_views: the argument lists of the pnr_baked_sh_render_* pair with
 *   (rows, M, degree, index, bits) in the place of (coef, degree, bits).  degree = -1: rows (M,4) fp32, the (r, g, b, sigma) of the
 *   kept points (the RGBA march); degree 0, 1, 2: rows (M,B,4), their coefficients (the view-dependent march).  rows is 16-byte
 *   aligned; bits and index are mandatory: a sparse volume has nothing to march unskipped.
 *   Semantics: the dense march above, with ONE change in where a corner comes from.  For an active sample (inside the box, its
 *   cell's bit on) the four index values of the pair bases p000, p000 + sy, p000 + sx, p000 + sx + sy (p000 the cell's lowest
 *   corner, sy = nz, sx = ny nz) are loaded -- four independent 4-byte loads, issued together -- and the corners of a pair are
 *   rows r and r + 1 of `rows`.  Everything else is the dense march unchanged, operation for operation (it is the same function,
 *   instantiated on where a row lies): the B float4 loads of a corner, the SH evaluation and the clamps, the blend order, the
 *   number of corner pairs in flight, the compositing, terminate and white_bkgd.  With index and rows made from a dense volume and
 *   the same bits, the outputs are the bytes of pnr_baked_render_* / pnr_baked_sh_render_* with those bits.
 *   Safety -- the counterpart of "no input can make the kernel read outside the volume": an index value is always read inside
 *   index (the cell is clamped to the grid); a sample any of whose four pair rows is not in [0, M - 2] has sigma = 0 and reads NO
 *   row; it enters the product as the factor 1, like a skipped sample.  An index built by pnr_sparse_points_mark and a prefix sum
 *   never triggers it.  M = 0 (and M = 1): every ray gets the background; neither index nor rows is read, and with M = 0 index,
 *   bits and rows may be null.
 *   One wavefront per ray, no atomics, no LDS, no workspace: two calls give the same bytes.
 *   PNR_E_INVALID: what the dense entries refuse (rows in the place of vol / coef), and M < 0, a null index, bits or rows with
 *   R > 0 and M > 0, rows not 16-byte aligned, index not 4-byte aligned, a degree outside {-1, 0, 1, 2}.  R = 0: no-op. */
int pnr_sparse_points_mark(const uint32_t *bits, int nx, int ny, int nz, uint8_t *keep /*(P)*/, void *stream);
int pnr_gen_grid_points_at(const double *c1 /*host*/, const double *c2 /*host*/, const int *reso /*host*/,
                           const int32_t *ids /*(count)*/, long long count, float *xyz, float *viewdirs /*nullable*/,
                           void *stream);
int pnr_baked_sparse_render_rays(const float *rays, long long R, const float *rows /*(M,4) or (M,B,4)*/, long long M, int degree,
                                 const int32_t *index /*(nx,ny,nz)*/, const uint32_t *bits, int nx, int ny, int nz,
                                 const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd, float terminate,
                                 float *rgb /*(R,3)*/, float *depth /*(R)*/, float *alpha /*(R)*/, void *stream);
int pnr_baked_sparse_render_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                  float z_near, float z_far, const float *rows /*(M,4) or (M,B,4)*/, long long M, int degree,
                                  const int32_t *index /*(nx,ny,nz)*/, const uint32_t *bits, int nx, int ny, int nz,
                                  const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd,
                                  float terminate, float *rgb /*(NV H W,3)*/, float *depth, float *alpha, void *stream);

/* Half-precision baked volumes (added within ABI rev 12 as well): fp16 STORAGE, the fp32 march.  What a volume stores -- rgb in
 * [0, 1], a relu'd sigma, low-order SH coefficients of those -- is kept as IEEE binary16: a stored (r, g, b, sigma) is four fp16
 * numbers in 8 bytes, a grid point 8 B bytes (8 for RGBA, 32 at degree 1, 72 at degree 2), half of the forms above.
 * The contract, which needs no tolerance because fp16 -> fp32 is exact:
 *     marching a half volume gives the BYTES of the fp32 march of the same values widened to fp32
 *   -- pnr_baked_half_render_* gives the bytes of pnr_baked_render_* (degree -1) / pnr_baked_sh_render_* (degree 0, 1, 2), and
 *   pnr_baked_sparse_half_render_* those of pnr_baked_sparse_render_*, on the widened array with every other argument the same.
 *   Every stored number is loaded (one 8-byte load per (r, g, b, sigma)) and widened exactly, component by component; subnormals,
 *   -0 and 65504 keep their value.  EVERYTHING ELSE IS THOSE ENTRIES' TEXT, operation for operation (it is the same function,
 *   instantiated on what a stored number is): the left-to-right SH sum in fp32, the per-corner clamps, the blend order z, y, x, the
 *   compositing scan, terminate, white_bkgd, skipping, the ray that cannot be sampled, the sparse safety rule (a sample whose pair
 *   rows are not in [0, M - 2] reads no row), the number of corner pairs in flight.
 * degree = -1: vol (nx,ny,nz,4) / rows (M,4) fp16, the RGBA march.  degree 0, 1, 2: vol (nx,ny,nz,B,4) / rows (M,B,4) fp16, the
 *   view-dependent march.  vol / rows are C-contiguous and 16-byte aligned.  The sparse pair has the argument lists of
 *   pnr_baked_sparse_render_rays / _views with `const uint16_t *rows`.
 * What rounding to fp16 costs, per stored value (util.bake.to_half: round to nearest even, a finite value beyond +-65504 saturates
 *   at +-65504, so an infinity is never stored -- it would put inf - inf into the blend):
 *     a value v with |v| <= 65504 is off by at most max(2^-11 |v|, 2^-25);
 *     an SH corner value before the clamp by at most 2^-11 (|c_0| + sum_k |c_k| |Y_k|) (+ k 2^-25 for subnormal coefficients) plus
 *     the fp32 rounding of the sum that the fp32 form has as well;
 *     a sigma above 65504 is stored as 65504: at any usable step (step sigma > 88) that corner alone still gives alpha = 1, but
 *     the trilinear blend with its neighbours weighs 65504 where it weighed more, so samples next to it can come out less opaque.
 *   The skip grid of a half volume is built from the widened values, so skipping stays exact at threshold 0; a sigma below 2^-25
 *   rounds to 0 and may switch its cells off.  The effect on an image has no bound here; profiles/baked_notes.md has measurements.
 * PNR_E_INVALID, before any HIP call: what the fp32 counterparts refuse, a degree outside {-1, 0, 1, 2}, vol / rows not 16-byte
 *   aligned.  R = 0: no-op. */
int pnr_baked_half_render_rays(const float *rays, long long R, const uint16_t *vol /*(nx,ny,nz,4) or (nx,ny,nz,B,4) fp16*/,
                               int degree, const uint32_t *bits /*nullable*/, int nx, int ny, int nz, const float *c1 /*host*/,
                               const float *c2 /*host*/, float step, int white_bkgd, float terminate, float *rgb /*(R,3)*/,
                               float *depth /*(R)*/, float *alpha /*(R)*/, void *stream);
int pnr_baked_half_render_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                float z_near, float z_far, const uint16_t *vol /*(nx,ny,nz,4) or (nx,ny,nz,B,4) fp16*/,
                                int degree, const uint32_t *bits /*nullable*/, int nx, int ny, int nz, const float *c1 /*host*/,
                                const float *c2 /*host*/, float step, int white_bkgd, float terminate,
                                float *rgb /*(NV H W,3)*/, float *depth, float *alpha, void *stream);
int pnr_baked_sparse_half_render_rays(const float *rays, long long R, const uint16_t *rows /*(M,4) or (M,B,4) fp16*/, long long M,
                                      int degree, const int32_t *index /*(nx,ny,nz)*/, const uint32_t *bits, int nx, int ny,
                                      int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd,
                                      float terminate, float *rgb /*(R,3)*/, float *depth /*(R)*/, float *alpha /*(R)*/,
                                      void *stream);
int pnr_baked_sparse_half_render_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx,
                                       float cy, float z_near, float z_far, const uint16_t *rows /*(M,4) or (M,B,4) fp16*/,
                                       long long M, int degree, const int32_t *index /*(nx,ny,nz)*/, const uint32_t *bits,
                                       int nx, int ny, int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step,
                                       int white_bkgd, float terminate, float *rgb /*(NV H W,3)*/, float *depth, float *alpha,
                                       void *stream);

/* Gradients of the baked march with respect to the STORED VALUES (added within ABI rev 12 as well): what lets a caller fit a
 * volume to images -- distil the network's renders past the point-sample bake, or refine per scene -- instead of only baking it.
 * pnr_baked_backward_rays / pnr_baked_backward_views are the backward of every fp32 march above: `stored` is
 *     degree -1: the RGBA volume (nx,ny,nz,4);   degree 0, 1, 2: the coefficient volume (nx,ny,nz,B,4), B = (degree+1)^2;
 *     index == NULL: that dense array, and M is not looked at;
 *     index != NULL: the M kept rows (M,4) / (M,B,4) of pnr_baked_sparse_render_*, and bits are then mandatory.
 * d_rgb (R,3), d_depth (R), d_alpha (R): the upstream gradients dL/d rgb, dL/d depth, dL/d alpha of the march's three outputs;
 *   each may be NULL and is then read as zeros.  A ray whose upstream gradients are all exactly zero is not walked.
 * d_stored: fp32, the shape of `stored`.  The entry ADDS dL/d stored into it (fp32 atomicAdd on global memory, exact zeros are
 *   skipped): the caller zeroes it before the first call, and calls on several batches of rays accumulate.  Only elements that a
 *   sample of the march read are touched.
 * The samples are EXACTLY the forward's: the kernels call the same device functions for the inside-the-box test, the cell, the
 *   skip-bit test, the sparse row lookup and the blend (and count the samples with the same five lines), and with terminate > 0 the backward first walks the
 *   chunks in the forward's direction with the forward's operations and stops after the chunk the forward stopped after.
 *   With w_i = a_i T_i, T_i = prod_{j<i} (1 - a_j + 1e-10), a_i = 1 - exp(-step sigma_i):
 *     g_i = d_rgb . c_i + d_depth t_i + d_alpha - [white_bkgd] (d_rgb.r + d_rgb.g + d_rgb.b)
 *     dL/da_i = T_i (g_i - S_i),  S_i = g_{i+1} a_{i+1} + (1 - a_{i+1} + 1e-10) S_{i+1}  (S of the last sample: 0)
 *     dL/dsigma_i = dL/da_i step exp(-step sigma_i),   dL/dc_i = w_i d_rgb
 *   S is carried from the last chunk of 64 samples to the first by a reverse scan of these affine maps: it is never formed as a
 *   difference of sums and nothing is divided by 1 - a_j, so a sample with a_i = 1 in fp32 keeps the gradients on both sides of it
 *   finite and accurate.  Through the blend: corner (ix,iy,iz) of the sample's cell gets the product over the axes of f or 1 - f
 *   (the derivative of the nested a + f (b - a)).  Through a view-dependent corner: coefficient k gets that times Y_k (Y_0 = 1)
 *   times the derivative of the clamp, per channel, under torch.clamp's convention: 1 where the unclamped value lies in the closed
 *   range ([0,1] for rgb, >= 0 for sigma), 0 outside and for a NaN.  The RGBA form has no clamp and no relu, as its forward.
 * With bits, a sample in a cell whose bit is off contributes nothing and receives nothing: fitting against a skip grid freezes the
 *   empty cells, and cannot grow density in them.  Without bits such a sample reaches sigma like any other.
 * This is the one path of the baked family that is NOT bit-reproducible from run to run: the order in which the atomics of
 *   different samples arrive varies, so a sum can differ in its last bits.
 * These two entries give no gradient with respect to rays or poses (pnr_baked_ray_backward_* below do); none exists with respect
 *   to step or the geometry.  fp32 storage only: there is no fp16 entry (fit the fp32
 *   volume, round it afterwards).  No workspace.
 * PNR_E_INVALID, before any HIP call, in the order and with the words of the march entries: a degree outside {-1, 0, 1, 2}; bad
 *   sizes, a null or misaligned ray / pose array; M < 0 with an index; the grid and march settings; a null d_stored or stored, an
 *   index with M > 0 and no bits ("null argument"); stored not 16-byte aligned; index, bits, d_rgb, d_depth, d_alpha or d_stored not
 *   4-byte aligned.  R = 0 (NV = 0): no-op, PNR_OK. */
int pnr_baked_backward_rays(const float *rays, long long R, const float *stored, long long M, int degree,
                            const int32_t *index /*nullable: dense*/, const uint32_t *bits /*nullable when dense*/, int nx, int ny,
                            int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd, float terminate,
                            const float *d_rgb /*(R,3), nullable*/, const float *d_depth /*(R), nullable*/,
                            const float *d_alpha /*(R), nullable*/, float *d_stored /*fp32, the shape of stored; added into*/,
                            void *stream);
int pnr_baked_backward_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                             float z_near, float z_far, const float *stored, long long M, int degree,
                             const int32_t *index /*nullable: dense*/, const uint32_t *bits /*nullable when dense*/, int nx, int ny,
                             int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd, float terminate,
                             const float *d_rgb /*(NV H W,3), nullable*/, const float *d_depth /*nullable*/,
                             const float *d_alpha /*nullable*/, float *d_stored, void *stream);

/* Gradients of the baked march with respect to the RAYS (added within ABI rev 12 as well): what lets a caller register a camera
 * against a baked volume -- move a pose by gradient descent until the march matches an image.  (The sentence above, "no gradient
 * with respect to rays", stays true of pnr_baked_backward_*; these two entries are that gradient.)
 * pnr_baked_ray_backward_rays / pnr_baked_ray_backward_views are the backward of EVERY march above: `stored` is what
 *   pnr_baked_backward_* calls `stored` (degree -1: (nx,ny,nz,4); 0, 1, 2: (nx,ny,nz,B,4); index != NULL: the M kept rows, bits then
 *   mandatory), as fp32 (storage_half 0) or as fp16 (storage_half 1: four fp16 numbers per (r,g,b,sigma), widened exactly on load).
 *   The volume is not differentiated here, so a half volume is a legitimate target, and gives the BYTES of the call on the widened
 *   values.  d_rgb, d_depth, d_alpha: as pnr_baked_backward_*.
 * d_rays: (R,8) fp32, dL/d [ox,oy,oz,dx,dy,dz,near,far].  EVERY row is WRITTEN (not added into): a ray with no samples, a ray that
 *   misses the box and a ray whose upstream gradients are all exactly zero get a row of exact zeros; the caller zeroes nothing.
 *   The views form regenerates each ray from the camera as the march does and writes the gradient with respect to that regenerated
 *   ray, rows ordered (view, row, column): pnr_gen_rays_backward applied to it is the gradient with respect to the poses.
 * The samples are EXACTLY the forward's, found by the device functions of the forward and of pnr_baked_backward_*; g_i, S_i, T_i,
 *   w_i, dL/da_i, dL/dsigma_i and dL/dc_i are those of pnr_baked_backward_*, by the same walk and the same reverse scan.  Then,
 *   with the corner values v[ix][iy][iz] of the sample's cell (clamped, for a view-dependent volume) and (fx, fy, fz) its fractions:
 *     d val / d fz = the x,y-blend of (v[..][..][1] - v[..][..][0])
 *     d val / d fy = the x-blend of the z-blended (y1 - y0)
 *     d val / d fx = vy[1] - vy[0]
 *     d val / d p_a = (d val / d f_a) / h_a, times the derivative of f's clamp (torch.clamp's convention: 1 on the closed [0,1])
 *     dL/dp_i = sum_c dL/dval_{i,c} d val_c / d p,   dL/dval_i = (w_i d_rgb.r, w_i d_rgb.g, w_i d_rgb.b, dL/dsigma_i)
 *     dL/dt_i = dL/dp_i . d + d_depth w_i            (depth = sum w_i t_i, and t_i = near + (i + 1/2) step moves with near alone)
 *     d_o = sum_i dL/dp_i,   d_d = sum_i t_i dL/dp_i,   d_near = sum_i dL/dt_i,   d_far = 0
 *   A view-dependent volume (degree >= 1) adds the way through the basis: dL/dY_k = sum over samples and corners of (trilinear
 *   weight) x (the clamps' derivative, as pnr_baked_backward_* forms it) x coef[point][k] . dL/dval for k = 1..B-1, and
 *     d_d += (I - n n^T) / |d| . sum_k dL/dY_k grad Y_k(n),   n = d / |d|, with
 *     grad Y_1 = (0, s3, 0)   grad Y_2 = (0, 0, s3)   grad Y_3 = (s3, 0, 0)   grad Y_4 = s15 (y, x, 0)   grad Y_5 = s15 (0, z, y)
 *     grad Y_6 = (0, 0, 3 s5 z)   grad Y_7 = s15 (z, 0, x)   grad Y_8 = s15 (x, -y, 0)      (s3 = sqrt 3, s5 = sqrt 5, s15 = sqrt 15)
 *   A direction whose squared norm is 0 or not finite has Y_k = 0 for k >= 1 and gets no such term.
 * Treated as CONSTANTS: the number of samples n = ceil((far - near) / step) -- far enters through it alone, so d_far is exactly 0 --,
 *   the inside-the-box test, the skip bits, the sparse row lookup, the chunk the march stops after (terminate), the cell floor()
 *   names, and which side of each clamp a value lies on.  The march is piecewise smooth in the ray: the gradient is the exact
 *   derivative almost everywhere, and for a sample ON a cell plane the one-sided derivative of the cell the floor convention puts
 *   it in (a caller comparing against another precision must keep samples off the planes: the two may name different cells).
 * Arithmetic: the per-sample part (the point, the blend and its partials, dL/dval, dL/dp) is fp32, each operation rounded on its
 *   own.  What runs ALONG the ray is carried in fp64: alpha is a_i = -expm1f(-step sigma_i) in fp32 and the factor 1 - a_i + 1e-10
 *   a double, and the products T_i, the affine maps of S_i and the seven sums of the row are doubles, rounded to fp32 once at the
 *   end.  The forward's fp32 chain is not used for them: over thousands of samples expf's rounding of a number next to 1 and the
 *   rounding of every factor make T drift by 1e-6 .. 3e-5, which a sum whose terms cancel (d_o across a blob) does not average
 *   away (profiles/baked_notes.md, "Ray gradients and registration").  The alphas differ from the forward's by less than an ulp of
 *   1; where the forward STOPPED (terminate) is decided by its own fp32 factors, formed with its operations.
 * Everything a ray's samples contribute is summed inside the ray's own wavefront -- per lane over the chunks, then across the 64
 *   lanes in a fixed butterfly order -- and one lane writes the row: no atomics, no LDS, no workspace; two calls on equal inputs
 *   give equal bytes, and the sparse entry gives the bytes of the dense entry with the same bits.
 * PNR_E_INVALID, before any HIP call, in the order and with the words of pnr_baked_backward_*, d_rays in the place of d_stored
 *   ("null argument"; "bits, d_rgb, d_depth, d_alpha and d_rays must be 4-byte aligned"), and after the degree rule one more:
 *   "storage_half must be 0 or 1".  R = 0 (NV = 0): no-op, PNR_OK. */
int pnr_baked_ray_backward_rays(const float *rays, long long R, const void *stored, int storage_half, long long M, int degree,
                                const int32_t *index /*nullable: dense*/, const uint32_t *bits /*nullable when dense*/, int nx, int ny,
                                int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd, float terminate,
                                const float *d_rgb /*(R,3), nullable*/, const float *d_depth /*(R), nullable*/,
                                const float *d_alpha /*(R), nullable*/, float *d_rays /*(R,8), every row written*/, void *stream);
int pnr_baked_ray_backward_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                 float z_near, float z_far, const void *stored, int storage_half, long long M, int degree,
                                 const int32_t *index /*nullable: dense*/, const uint32_t *bits /*nullable when dense*/, int nx, int ny,
                                 int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, int white_bkgd, float terminate,
                                 const float *d_rgb /*(NV H W,3), nullable*/, const float *d_depth /*nullable*/,
                                 const float *d_alpha /*nullable*/, float *d_rays /*(NV H W,8), every row written*/, void *stream);

/* Visibility of a baked volume (added within ABI rev 12 as well): which stored rows a set of rays SEES -- per row the largest
 * compositing weight any sample gave it.  The pruning criterion of a fitted volume (a row no ray sees is not constrained by the
 * fit), and the picture of what a set of views determines.
 * pnr_baked_visibility_rays / pnr_baked_visibility_views take the argument list of pnr_baked_ray_backward_* without white_bkgd and
 *   without upstream gradients: `stored`, storage_half, M, degree, index, bits, the grid, c1 / c2, step, terminate, then vis.
 *   All 16 kinds are served (RGBA and degree 0, 1, 2; fp32 and fp16; dense and sparse); the pass only READS the volume.
 * vis: fp32, (nx,ny,nz) when index == NULL, (M) -- one number per kept row -- when sparse.  The CALLER zeroes it once; the entry
 *   max-accumulates into it, so calls on several batches or views accumulate.
 * The samples are EXACTLY the forward's (its sample count, points, cells, skip bits, row lookup, blend and alpha, its product scan
 *   and carry; with terminate > 0 the walk stops after the chunk the forward stops after), and w_i = a_i (carry x excl_i) is formed
 *   with the forward's own fp32 operations: the forward's weight bit for bit.  For an active sample that found its rows, corner
 *   c = (ix,iy,iz) of its cell proposes
 *     v = w_i * omega_c,   omega_c = ((ix ? fx : 1 - fx) * (iy ? fy : 1 - fy)) * (iz ? fz : 1 - fz)
 *   -- the corner weights of pnr_baked_backward_*, by its operations and in its order --, a proposal that is not > 0 is dropped
 *   (zeros, and anything that is not a number), and vis[row(c)] = max(vis[row(c)], v).
 * The maximum is taken by an unsigned-integer atomic max on the bit pattern of the float: every proposal is a positive finite
 *   float, on which the two orders agree.  Maximum is commutative and associative EXACTLY: unlike pnr_baked_backward_*, two calls
 *   on equal inputs give EQUAL BYTES, and so do any order of the rays and any split of them into accumulating calls; the sparse
 *   entry gives the dense entry's bytes (with the same bits) at the kept points; a half volume gives the bytes of its widened one.
 *   No scratch, no LDS, no workspace; one wavefront per ray.  vis must hold non-negative finite floats on entry (zeros, or the
 *   result of earlier calls).
 * Out of scope: scenes (pnr_baked_scene_* have no visibility).
 * PNR_E_INVALID, before any HIP call, in the order and with the words of pnr_baked_ray_backward_*, vis in the place of d_rays
 *   ("null argument"; "bits, d_rgb, d_depth, d_alpha and vis must be 4-byte aligned").  R = 0 (NV = 0): no-op, PNR_OK. */
int pnr_baked_visibility_rays(const float *rays, long long R, const void *stored, int storage_half, long long M, int degree,
                              const int32_t *index /*nullable: dense*/, const uint32_t *bits /*nullable when dense*/, int nx, int ny,
                              int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, float terminate,
                              float *vis /*(nx,ny,nz) or (M); zeroed by the caller, max-accumulated into*/, void *stream);
int pnr_baked_visibility_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                               float z_near, float z_far, const void *stored, int storage_half, long long M, int degree,
                               const int32_t *index /*nullable: dense*/, const uint32_t *bits /*nullable when dense*/, int nx, int ny,
                               int nz, const float *c1 /*host*/, const float *c2 /*host*/, float step, float terminate, float *vis,
                               void *stream);

/* Resampling a baked volume (added within ABI rev 12 as well): the stored values on ANOTHER point count over the SAME box -- what
 * lets a fitted volume go from a coarse grid to a fine one without another bake.
 * src: what pnr_baked_ray_backward_* call `stored` -- (nx,ny,nz,4) (degree -1) or (nx,ny,nz,B,4) (degree 0, 1, 2), fp32
 *   (storage_half 0) or fp16 (1), or with index != NULL the M kept rows and `index` (nx,ny,nz).  index == NULL: M is not looked at.
 * dst: always fp32.  ids_dst == NULL: dense, (nx',ny',nz'[,B],4), M_dst not looked at; otherwise the M_dst rows at the int32
 *   linear ids `ids_dst` of the destination grid -- an id outside that grid writes a row of zeros and reads nothing.
 * Per axis, for destination point i of n' over n source points, in 64-bit INTEGER arithmetic:
 *     num = i (n - 1),  q = num / (n' - 1),  rem = num % (n' - 1),  i0 = q,  i1 = min(q + 1, n - 1),  f = (float)rem / (float)(n' - 1)
 *   -- f is the one rounding.  The value is the nested blend of the march, along z, then y, then x, each 1-D blend
 *     f == 0 ? a : a + f (b - a)
 *   with the product, the difference and the sum rounded on their own and the f == 0 case a SELECT: a destination point that
 *   coincides with a source point copies its value, -0 included.  So resampling to the same point count is the identity, and a
 *   refinement n' - 1 = m (n - 1) keeps the old points, bit for bit, at stride m.  A view-dependent volume interpolates its
 *   COEFFICIENTS: no basis, no clamp.  A sparse source reads a corner that is not kept (index < 0 or a rank outside [0, M)) as
 *   zeros -- what the dense form of the volume holds there.
 * One thread per destination float4 (point, k), k fastest, then z.  No atomics; two calls on equal inputs give equal bytes.
 * Out of scope: autograd through the resampling, another box, fp16 destinations.
 * PNR_E_INVALID before any HIP call, in this order: a degree outside {-1, 0, 1, 2}; storage_half neither 0 nor 1; either grid with
 *   an axis < 2 points, or with 2^31 points or more; M < 0 with an index, M_dst < 0 with ids_dst; (no destination rows: no-op,
 *   PNR_OK;) a null dst, a null src with source rows; src or dst not 16-byte aligned (fp16 src: 8-byte); index or ids_dst not
 *   4-byte aligned. */
int pnr_baked_resample(const void *src, int storage_half, long long M, int degree, const int32_t *index /*nullable: dense*/, int nx,
                       int ny, int nz, float *dst, long long M_dst, const int32_t *ids_dst /*nullable: dense*/, int nx_dst, int ny_dst,
                       int nz_dst, void *stream);

/* Total-variation prior of a fitted volume (added within ABI rev 12 as well): the smoothness term a fit to few views needs, its
 * value and its gradient in one pass, with no atomics.  `stored` is what pnr_baked_backward_* calls `stored`: fp32 (nx,ny,nz,4)
 * (degree -1) or (nx,ny,nz,B,4) (degree 0, 1, 2; B = 1, 4, 9); with index != NULL the M kept rows (M,4) / (M,B,4), `index`
 * (nx,ny,nz) and `ids` (M) being those of pnr_sparse_points_mark's kept set (ops.sparse_points).  index == NULL: M is not looked at.
 * A point p holds E = 4 or 4 B elements; w: a HOST array of E floats, finite and >= 0, one weight per element of a row.
 *   d_a(p,c) = S[p + e_a, c] - S[p, c] for the axes a = x, y, z: raw differences, not divided by the spacing; 0 where p + e_a lies
 *     beyond the grid, and in the sparse form 0 where p + e_a is not kept (index < 0, or a rank that is not in [0, M)).
 *   n(p,c) = sqrt(d_x^2 + d_y^2 + d_z^2 + eps), eps finite and > 0
 *   value = (1/N) sum_p sum_c w_c n(p,c),   N = nx ny nz (dense) or M (sparse: the sum runs over the kept points)
 *   grad[p,c] += scale * d value / d S[p,c]
 *             = scale * (fp32(w_c / N) * (-(d_x + d_y + d_z)/n(p,c) + sum_a d_a(p - e_a, c)/n(p - e_a, c)))
 *     over the back neighbours p - e_a that exist (and are kept), in the order x, y, z.  The entry ADDS into the caller's buffer, as
 *     the march backward does.  scale: a DEVICE pointer to one float, NULL = 1 (an autograd backward hands its upstream gradient over
 *     without a host read).  A scale that is a power of two scales the added term exactly.
 * Arithmetic: the differences, squares, the sum ((d_x^2 + d_y^2) + d_z^2) + eps, sqrtf and the quotients are fp32, each rounded on
 *   its own.  The value is accumulated in fp64 (w_c n(p,c) as a product of doubles) and reduced in a fixed order: a thread over the
 *   float4s it owns, the lanes of a wave by a butterfly, the four waves of a block in order, and one last block over the block
 *   partials; sum / N is written as one fp64 (value64) and the same number rounded to fp32 (value32).
 * Guarantees: no atomics; two calls on equal inputs give equal bytes, value and gradient; the dense entry and the sparse entry with
 *   every point kept give equal bytes; the library allocates nothing.  workspace: pnr_baked_tv_workspace_bytes() bytes of device
 *   memory (16 KiB, whatever the volume), 8-byte aligned, needed only when a value is asked for; two calls in flight on different
 *   streams need one each.  Either half may be asked for alone (grad == NULL; value32 == value64 == NULL); with neither the call is
 *   a no-op.  M = 0: nothing is read, the value written is 0.  stored and grad must not overlap.
 * The kernel takes one float4 (point, basis k) per thread -- consecutive lanes read consecutive 16-byte words -- and the thread that
 *   owns S[p] recomputes the norms of its three back neighbours: a 13-point stencil, nothing stored in between.  Index arithmetic
 *   is 64-bit; an id outside the grid or a rank outside [0, M) is treated as "not kept": no input makes the kernel read outside
 *   stored, index or ids.
 * PNR_E_INVALID before any HIP call, in this order: a degree outside {-1, 0, 1, 2}; index without ids or ids without index; M < 0
 *   with an index; the grid (every axis >= 2 points, fewer than 2^31 cells; sparse: fewer than 2^31 points); eps not finite or <= 0;
 *   a null w; a weight that is negative or not finite; a value asked for without a workspace; a null stored with N > 0; stored or
 *   grad not 16-byte aligned; index, ids, scale or value32 not 4-byte aligned, value64 or workspace not 8-byte aligned. */
size_t pnr_baked_tv_workspace_bytes(void);
int pnr_baked_tv(const float *stored, long long M, int degree, const int32_t *index /*nullable: dense*/,
                 const int32_t *ids /*(M) int32, with index*/, int nx, int ny, int nz, const float *w /*host, E floats*/, float eps,
                 const float *scale /*device, nullable*/, float *value32 /*device, nullable*/, double *value64 /*device, nullable*/,
                 float *grad /*device, nullable, the shape of stored; added into*/, void *workspace, void *stream);

/* Scenes of several baked volumes (inference; added within ABI rev 12 as well: one struct and two entries, nothing existing
 * changes).  Every entry above renders ONE volume in ONE axis-aligned box.  A baked object lives in its own frame; these two
 * entries march up to PNR_BAKED_SCENE_MAX_OBJECTS posed volumes in one image.  Separate marches cannot be merged afterwards:
 * where boxes overlap, or one object stands in front of another, the transmittance of one attenuates the other sample by sample.
 * Objects.  `objects`: a HOST array of n_objects PnrBakedObject, 1 <= n_objects <= 8; every pointer inside is a device pointer.
 *   Per object: `stored` as pnr_baked_ray_backward_* take it (degree -1: (nx,ny,nz,4); 0, 1, 2: (nx,ny,nz,B,4); with index != NULL
 *   the M kept rows, bits then mandatory; storage_half 0: fp32, 1: fp16), its skip grid `bits`, its own grid (nx,ny,nz) and box
 *   (c1, c2) IN THE OBJECT'S FRAME, and pose = [R | t], row-major (3,4): object-to-world, x_world = R x_object + t, rigid.
 *   One kind per scene: all objects share degree, storage_half and whether index is set; grids, boxes and poses may differ.
 * The world ray.  n = ceil((far - near) / step) and t_i = near + (i + 0.5) step are those of the single-volume march, taken from
 *   the WORLD ray (o, d, near, far); a ray that cannot be sampled -- by that march's rule, applied to the world ray -- gets the
 *   background and reads nothing.
 * The ray in the frame of object j.  q = o - t_j, then for the axes a = x, y, z
 *     o'_a = (q_x R_xa + q_y R_ya) + q_z R_za,   d'_a = (d_x R_xa + d_y R_ya) + d_z R_za      (R_ra = pose[4 r + a])
 *   every product, difference and sum rounded on its own.  The pose is rigid, so t is shared: p'_i = o' + t_i d'.
 * The value of object j at sample i is exactly what the single-volume march computes for the ray (o', d', near, far): the inside
 *   test against the object's own box, its skip bit, its cell, its blend; for a coefficient volume the basis is evaluated on d'
 *   and the clamps are per corner.  A sample that is outside, skipped, or (sparse) finds no rows contributes nothing.
 * Mixing.  Over the objects that contribute to sample i, in list order:
 *     sigma = sum_j sigma_j  (summed left to right),   c = sum_j (sigma_j / sigma) c_j  when sigma > 0 (left to right), else 0
 *   -- the colour of a mixture of media weighted by density.  alpha_i = 1 - exp(-step sigma), the product scan, rgb, depth, alpha,
 *   white_bkgd and the termination check every 64 samples are the single-volume march's, applied to (c, sigma).  A chunk in which
 *   no object has a sample inside its box and occupied issues no loads and leaves the carry as it is.  Stored sigmas are taken to
 *   be >= 0, as a bake's are (a negative sum gives c = 0).
 * What the rules imply (tests/test_hip_baked_scene.py holds the kernel to each):
 *   (a) one object whose pose is exactly [I | 0] renders the BYTES of the matching single-volume entry: products with 0 and 1 and
 *       sums with 0 are exact for finite rays, x / x = 1; no special case in the code;
 *   (b) one object whose rotation has entries in {0, +1, -1} renders the bytes of the single-volume entry on the rays (o', d')
 *       formed by the same fp32 operations;
 *   (c) an object whose sigma is 0 at every sample of a ray leaves that ray's bytes as they are without it (x + 0, x / x, 0 c);
 *   (d) two objects commute;
 *   (e) the same volume listed twice at one pose renders the bytes of that volume with sigma doubled (sigma / (2 sigma) = 0.5,
 *       0.5 c + 0.5 c = c, and doubling commutes with the blend's roundings);
 *   (f) with every object's bits built at threshold 0 and dilate 0, skipping is exact;
 *   (g) no atomics, no LDS, no workspace: two calls give the same bytes;
 *   (h) pnr_baked_scene_render_views gives the bytes of pnr_baked_scene_render_rays on pnr_gen_rays' rows.
 * Kernel.  One wavefront per ray, lane l of chunk c takes sample 64 c + l; the objects are an inner loop.  The scene travels by
 *   value as a kernel argument (128 bytes per object) and the loop's index is wave-uniform, so an object's fields are scalar
 *   loads.  A lane to whose sample ONE object contributes keeps that value; a lane with several walks the objects a second time,
 *   because the weights need the finished sum -- the second walk repeats the first one's loads, in overlaps only.
 * Cost: per sample and object one transform and one inside test; the loads are those of the single marches.
 * PNR_E_INVALID, before any HIP call, in this order: n_objects outside [1, 8]; objects == NULL; per object "object j: reserved
 *   must be 0", then "object j: mixed kinds ..." (degree, storage_half or index-set differs from object 0); the rays / poses
 *   checks, step, terminate, and with R > 0 a null or misaligned rgb / depth / alpha, in the words of pnr_baked_render_*; then per
 *   object, under "entry: object j: ", everything pnr_baked_ray_backward_* refuse about a volume in their words (degree,
 *   storage_half, M < 0, the grid, c1 / c2, nulls, 16-byte alignment of stored, 4-byte alignment of index and bits, bits missing
 *   for sparse rows) and "pose must be finite and rigid": all 12 numbers finite, max |R^T R - I| <= 1e-4 and det R > 0, computed
 *   in fp64 -- far above what an fp32 rotation leaves, far below a visible shear.  R = 0 (NV = 0): no-op, PNR_OK.
 * Not here: gradients of any kind, mixed kinds, scale or shear, more than 8 objects, a step per object, a background layer. */
#define PNR_BAKED_SCENE_MAX_OBJECTS 8
typedef struct PnrBakedObject {      /* one posed volume; all pointers are device pointers */
    const void *stored;              /* dense (nx,ny,nz[,B],4) or the M kept rows; fp32 or fp16 */
    const uint32_t *bits;            /* skip grid of this object; nullable for dense, mandatory for sparse */
    const int32_t *index;            /* sparse only, else NULL */
    long long M;                     /* sparse only, else 0 */
    int nx, ny, nz, degree;          /* degree -1: RGBA, 0..2: coefficient volume */
    int storage_half, reserved;      /* 0 | 1; reserved must be 0 */
    float c1[3], c2[3];              /* the object's box, in the OBJECT's frame */
    float pose[12];                  /* object-to-world [R | t], row-major (3,4), rigid */
} PnrBakedObject;
int pnr_baked_scene_render_rays(const float *rays, long long R, const PnrBakedObject *objects /*host*/, int n_objects,
                                float step, int white_bkgd, float terminate, float *rgb /*(R,3)*/, float *depth /*(R)*/,
                                float *alpha /*(R)*/, void *stream);
int pnr_baked_scene_render_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                 float z_near, float z_far, const PnrBakedObject *objects /*host*/, int n_objects, float step,
                                 int white_bkgd, float terminate, float *rgb /*(NV H W,3)*/, float *depth, float *alpha,
                                 void *stream);

/* Gradients of the scene march (added within ABI rev 12 as well; "Not here: gradients of any kind" above stays true of the two
 * render entries -- these two are the gradient with respect to the world RAYS and to each object's POSE; the stored values of a
 * scene are differentiated by pnr_baked_scene_stored_backward_* below, not here).  What lets a caller find where an object stands: move its pose by gradient descent until the
 * scene matches its images, or refine a camera against a scene with an occluder in it.
 * pnr_baked_scene_backward_rays / _views are the backward of pnr_baked_scene_render_rays / _views for every kind those take:
 *   RGBA and degree 0, 1, 2, dense and sparse rows, fp32 and fp16 storage (the volumes are not differentiated, so a half volume is
 *   legitimate, as in pnr_baked_ray_backward_*).  objects, step, white_bkgd, terminate: the forward's.  d_rgb, d_depth, d_alpha:
 *   the upstream gradients of the march's outputs, each NULL = zeros.
 * Outputs, each WRITTEN (not added into):
 *   d_rays  (R,8)            dL/d [ox,oy,oz,dx,dy,dz,near,far] of the WORLD ray; column 7 is exactly 0.  The views form writes the
 *                            gradient with respect to the regenerated ray, rows ordered (view, row, column): pnr_gen_rays_backward
 *                            applied to it is the gradient with respect to the cameras.
 *   d_local (R,n_objects,6)  dL/d (o'_j, d'_j): the gradient with respect to the ray in the frame of object j.
 *   d_poses (n_objects,12)   nullable.  dL/d [R_j | t_j] as 12 FREE numbers, row-major (3,4) as PnrBakedObject::pose; the caller
 *                            projects onto the tangent of the rigid motions.
 * Samples: exactly the forward's.  The walk is pnr_baked_ray_backward_*'s: a first walk in the forward's direction finds the chunk
 *   the forward stopped after (by the forward's own fp32 factors) and the fp64 transmittance at the head of each chunk; then the
 *   chunks from last to first with the fp64 reverse affine scan; beyond 4096 samples the heads are rebuilt.  It is applied to the
 *   mixture (c_i, sigma_i) of the scene march, formed with the forward's operations in list order.
 * Along the ray: g_i, T_i, S_i, w_i, dL/da_i, dL/dsigma_i = dL/da_i step (1 - a_i) and dL/dc_i = w_i d_rgb are those of
 *   pnr_baked_ray_backward_*, computed on sigma_i = sum_j sigma_ij and c_i = sum_j (sigma_ij / sigma_i) c_ij.
 * Through the mixing, for every object j that contributes to sample i, where sigma_i > 0:
 *     dL/dc_ij = (sigma_ij / sigma_i) dL/dc_i,      dL/dsigma_ij = dL/dsigma_i + ((c_ij - c_i) . dL/dc_i) / sigma_i
 *   CONVENTION: where sigma_i is not > 0 the forward's colour is the constant 0, so there dL/dc_ij = 0 and dL/dsigma_ij =
 *   dL/dsigma_i.  Off the cell planes a blended sigma of exactly 0 (stored sigmas >= 0) has zero spatial slope, so nothing is lost.
 *   With one contributor sigma_ij / sigma_i is exactly 1 and c_ij - c_i exactly 0: no special case.
 * Through each object's blend, exactly as pnr_baked_ray_backward_* do in that object's frame on the object ray (o', d'): the
 *   partials of the blend, the clamp of the fractions, the division by that object's h, and for a coefficient volume dL/dY_k and
 *   its way through Y(d' / |d'|).  Per sample this gives dp'_ij (fp32), and per ray and object
 *     d_local[r][j] = (sum_i dp'_ij,  sum_i t_i dp'_ij + the basis term of object j)
 * World ray: dp_i = sum_j R_j dp'_ij in fp32, objects in list order, each component (R_a0 x + R_a1 y) + R_a2 z;
 *     dL/dt_i = sum_j dp'_ij . d'_j + d_depth w_i
 *     d_o = sum_i dp_i,   d_d = sum_i t_i dp_i + sum_j R_j basis_j,   d_near = sum_i dL/dt_i,   d_far = 0
 * Poses: with q = o - t_j as the forward forms it,
 *     dL/dR_j[r][a] = sum_rays (q_r d_local.o'_a + d_r d_local.d'_a),      dL/dt_j[r] = - sum_rays sum_a R_j[r][a] d_local.o'_a
 *   reduced by a second kernel that regenerates (o, d) from the same ray source (explicit rows or cameras).
 * Treated as CONSTANTS: everything pnr_baked_ray_backward_* list, per object -- the sample count, the inside tests, the skip bits,
 *   the row lookup, the stop chunk, the cells floor() names, the sides of the clamps -- and which objects contribute to a sample.
 * Arithmetic: the per-sample part is fp32, each operation rounded on its own; what runs along the ray (T_i, the maps of S_i) is
 *   fp64 as in pnr_baked_ray_backward_*.  The seven sums of the world row are per-lane doubles over the chunks, reduced by the
 *   butterfly of the ray's wavefront, in that entry's order.  dL/dt_i is formed per contributing object as that entry's fp32 chain
 *   ((d_depth w_i + x) + y) + z on dp'_ij . d'_j; the chains are added in fp64 and the cnt - 1 surplus d_depth w_i taken off, so
 *   one contributor gives that entry's number and two objects commute.  The six numbers of an object are summed per chunk across the lanes
 *   (fp64, the same butterfly) and added, chunk after chunk from the last to the first, into one fp64 accumulator per (object,
 *   number); the basis sums dL/dY_k are per-lane fp32 sums per object, reduced at the end as that entry reduces them.  The pose
 *   reduction is fp64 in a fixed order -- a thread over the rays it owns, the lanes by the butterfly, one last wave per object over
 *   the block partials -- and rounds to fp32 once; a ray whose d_local row of an object is all zeros is not added for it.
 * Guarantees: no atomics, no LDS, no memory allocated by the library; every row of d_rays and d_local is written; exact zeros
 *   (8 + 6 n_objects of them) for a ray with no samples or with all-zero upstream gradients; an object no ray meets gets 12 exact
 *   zeros in d_poses; two calls give equal bytes; the sparse form gives the dense form's bytes; fp16 storage gives the bytes of the
 *   call on the widened values; the views entry gives the rays entry's bytes on pnr_gen_rays' rows; ONE object whose pose is
 *   exactly [I | 0] gives pnr_baked_ray_backward_*'s bytes in d_rays (products with 0 and 1 and sums with 0 are exact).
 *   workspace: pnr_baked_scene_backward_workspace_bytes() bytes of device memory (384 KiB, whatever the scene), 8-byte aligned,
 *   needed only with d_poses; two calls in flight on different streams need one each.  Index arithmetic is 64-bit; no input makes a
 *   kernel read outside an object's stored, index or bits, or outside the workspace.
 * PNR_E_INVALID, before any HIP call: the refusals of pnr_baked_scene_render_*, in their order and words, through the same
 *   checking function, with d_rays / d_local in the place of rgb / depth / alpha ("null argument" with R > 0); the alignment
 *   sentence is "d_rgb, d_depth, d_alpha, d_rays, d_local and d_poses must be 4-byte aligned"; then one more: d_poses without a
 *   workspace, or with one that is not 8-byte aligned ("d_poses needs the workspace of
 *   pnr_baked_scene_backward_workspace_bytes(), 8-byte aligned"); per object the words are those of pnr_baked_ray_backward_*.
 *   R = 0 (NV = 0): nothing is marched, PNR_OK; d_poses, if given, is still WRITTEN, as zeros. */
size_t pnr_baked_scene_backward_workspace_bytes(void);
int pnr_baked_scene_backward_rays(const float *rays, long long R, const PnrBakedObject *objects /*host*/, int n_objects, float step,
                                  int white_bkgd, float terminate, const float *d_rgb /*(R,3), nullable*/,
                                  const float *d_depth /*(R), nullable*/, const float *d_alpha /*(R), nullable*/,
                                  float *d_rays /*(R,8), every row written*/, float *d_local /*(R,n_objects,6), every row written*/,
                                  float *d_poses /*(n_objects,12), nullable; written*/, void *workspace /*needed only with d_poses*/,
                                  void *stream);
int pnr_baked_scene_backward_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx, float cy,
                                   float z_near, float z_far, const PnrBakedObject *objects /*host*/, int n_objects, float step,
                                   int white_bkgd, float terminate, const float *d_rgb /*(NV H W,3), nullable*/,
                                   const float *d_depth /*nullable*/, const float *d_alpha /*nullable*/,
                                   float *d_rays /*(NV H W,8)*/, float *d_local /*(NV H W,n_objects,6)*/,
                                   float *d_poses /*(n_objects,12), nullable*/, void *workspace, void *stream);

/* Gradients of the scene march with respect to the STORED VALUES of its objects (added within ABI rev 12 as well: two entries,
 * PnrBakedObject unchanged): what lets a caller fit the contents of a scene to images of the scene.  Where objects overlap or
 * stand in front of one another the mixing makes every object's gradient depend on the others, so the single-volume backward of
 * each object alone is not this gradient.
 * pnr_baked_scene_stored_backward_rays / _views are the backward of pnr_baked_scene_render_rays / _views for fp32 storage: RGBA and
 *   degree 0, 1, 2, dense and sparse rows.  objects, step, white_bkgd, terminate: the forward's.  d_rgb, d_depth, d_alpha: the
 *   upstream gradients of the march's outputs, each NULL = zeros; a ray whose upstream gradients are all exactly zero is not walked.
 * d_stored: a HOST array of n_objects DEVICE pointers.  d_stored[j] is fp32 and has the shape of object j's `stored` (dense
 *   (nx,ny,nz,4) or (nx,ny,nz,B,4); sparse: the M kept rows).  The entry ADDS dL/d stored_j into it (fp32 atomicAdd on global
 *   memory, exact zeros are skipped): the caller zeroes it before the first call, and successive calls accumulate.  Only elements
 *   that a sample of the march read are touched.
 *   d_stored[j] == NULL: object j is FROZEN.  It still attenuates and mixes -- the mixture is formed over all objects --, receives
 *   nothing, and no atomic is issued for it: this is how one object is fitted in the presence of the others.
 *   Two entries may hold the same pointer (a volume listed twice): the buffer receives the sum of both listings' gradients.
 *   Every entry NULL: a no-op returning PNR_OK, after the checks.
 * Samples: exactly the scene forward's, found by its device functions.  The walk is pnr_baked_scene_backward_*'s: a first walk in
 *   the forward's direction finds the chunk the forward stopped after (by the forward's own fp32 factors) and the fp64
 *   transmittance at the head of each chunk; then the chunks from last to first with the fp64 reverse affine scan; beyond 4096
 *   samples the heads are rebuilt.  g_i, T_i, S_i, w_i, dL/da_i, dL/dsigma_i = dL/da_i step (1 - a_i) and dL/dc_i = w_i d_rgb are
 *   that entry's, on the mixture sigma_i = sum_j sigma_ij, c_i = sum_j (sigma_ij / sigma_i) c_ij; what runs along the ray is fp64
 *   (a_i = -expm1f(-step sigma_i) in fp32, the factor 1 - a_i + 1e-10 a double), rounded to fp32 once per sample; the rest is
 *   fp32, each operation rounded on its own.
 * Through the mixing, for every object j that contributes to sample i and is not frozen, where sigma_i > 0:
 *     dL/dc_ij = (sigma_ij / sigma_i) dL/dc_i,      dL/dsigma_ij = dL/dsigma_i + ((c_ij - c_i) . dL/dc_i) / sigma_i
 *   and where sigma_i is not > 0 (the forward's colour is the constant 0): dL/dc_ij = 0, dL/dsigma_ij = dL/dsigma_i -- the
 *   convention of pnr_baked_scene_backward_*.  Seen from the stored values it shows: g_i of such a sample has no d_rgb . c_i, so
 *   one object at [I | 0] gets pnr_baked_backward_*'s gradient EXCEPT from samples whose blended sigma is exactly 0 -- there that
 *   entry keeps the blended colour and its dL/dsigma_i is larger by T_i step (d_rgb . c_i).  The forward does not tell the two
 *   apart (w_i = 0).  With a skip grid, cells made of exactly empty points alone are not marched and the two agree.
 * Through the object's blend in ITS frame, exactly as pnr_baked_backward_* do: corner (ix,iy,iz) of the sample's cell gets the
 *   product over the axes of f or 1 - f; through a view-dependent corner, coefficient k gets that times Y_k (evaluated on d'_j)
 *   times the derivative of the clamps under torch.clamp's convention.  The RGBA form has no clamp.
 * With bits, a sample in a cell of object j whose bit is off contributes nothing and receives nothing, exactly as in
 *   pnr_baked_backward_*.
 * NOT bit-reproducible from run to run, like pnr_baked_backward_*: the order in which the atomics arrive varies.  No gradient
 *   with respect to rays or poses from these entries (pnr_baked_scene_backward_* give those).  No workspace, no LDS; the library
 *   allocates nothing.  Index arithmetic is 64-bit; only rows that the forward read are added into.
 * PNR_E_INVALID, before any HIP call, through the checking function of the other scene entries and in its order: n_objects,
 *   objects == NULL, "object j: reserved must be 0", "object j: mixed kinds ..."; then storage_half != 0 ("gradients exist for fp32
 *   volumes only; fit the volume in fp32 and call half() afterwards"); the rays / poses checks, step, terminate; with R > 0 a null
 *   d_stored array ("null argument (d_stored)"); "d_rgb, d_depth, d_alpha and every d_stored[j] must be 4-byte aligned"; then per
 *   object, under "entry: object j: ", the words of pnr_baked_backward_* and "pose must be finite and rigid".  R = 0 (NV = 0):
 *   no-op, PNR_OK, after these checks (d_stored may then be NULL). */
int pnr_baked_scene_stored_backward_rays(const float *rays, long long R, const PnrBakedObject *objects /*host*/, int n_objects,
                                         float step, int white_bkgd, float terminate, const float *d_rgb /*(R,3), nullable*/,
                                         const float *d_depth /*(R), nullable*/, const float *d_alpha /*(R), nullable*/,
                                         float *const *d_stored /*HOST array of n_objects device pointers; an entry may be NULL*/,
                                         void *stream);
int pnr_baked_scene_stored_backward_views(const float *poses /*(NV,4,4)*/, int NV, int W, int H, float fx, float fy, float cx,
                                          float cy, float z_near, float z_far, const PnrBakedObject *objects /*host*/,
                                          int n_objects, float step, int white_bkgd, float terminate,
                                          const float *d_rgb /*(NV H W,3), nullable*/, const float *d_depth /*nullable*/,
                                          const float *d_alpha /*nullable*/, float *const *d_stored /*HOST array, as above*/,
                                          void *stream);

/* Timing hook for bench.py: seconds spent in the fused network kernel launches issued on
 * `stream` since the last reset, measured with HIP events recorded around each launch on
 * that stream (call only after the stream has been synchronised). */
int pnr_profile_enable(int on);
int pnr_profile_read(double *mlp_kernel_ms, int *mlp_launches);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* PIXELNERF_HIP_H */
