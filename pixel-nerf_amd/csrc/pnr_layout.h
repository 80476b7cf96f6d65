// pnr_layout.h -- tile geometry and packed-weight layout shared by the repack kernel
// (pnr_pack.hip) and the fused network kernel (pnr_mlp.hip).  gfx950 only.
//
// Fused-kernel geometry:
//   workgroup = NW=8 waves (512 threads, 2 waves per SIMD), one workgroup per CU, persistent;
//   point tile = MT=64 sample points = JT=2 MFMA column tiles of 32 points;
//   wave w owns hidden features [64w, 64w+64) = IT=2 MFMA row tiles of 32 features;
//   every 512x512 linear is computed as  Y^T[feature][point] = W[feature][k] * X^T[k][point]
//   with v_mfma_f32_32x32x16_{f16,bf16}: A operand = weights (streamed from L2 straight into
//   VGPRs, pre-packed in fragment order), B operand = activations (LDS, or registers for
//   lin_out), C/D = fp32 accumulators that hold the residual stream.
//
// MFMA 32x32x16 fragment maps (lane l, h = l>>5):
//   A: row i = l&31, k = 8h+e (e=0..7)      B: col j = l&31, k = 8h+e
//   D: col j = l&31, row i = (r&3) + 8*(r>>2) + 4h  (r=0..15)
#pragma once
#include <stdint.h>

namespace pnr {

// Loads through a PnrMlpWeights pointer: the parameters are CALLER memory and may be views into a flat buffer at any 4-byte
// offset (torch's own allocations are 16-byte aligned, a `flat[1:]` view is not).  Every kernel that reads a parameter tensor with
// vector loads goes through these 4-byte-aligned types -- global_load_dwordx4 either way, without the compiler assuming more
// (one alignment contract for pack, fold, checksum, the fp32 GEMMs and the backward transposes).
typedef float f32x4_param __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned int u32x4_param __attribute__((ext_vector_type(4), aligned(4)));


constexpr int C_LAT = 512;   // latent channels (encoder.latent_size, encoder.py:68)
constexpr int D_HID = 512;   // d_hidden
constexpr int D_IN = 42;     // 39 positional code + 3 view direction (models.py:47-60)
constexpr int D_IN_PAD = 64; // padded K of lin_in
constexpr int D_OUT = 4;
constexpr int N_BLOCKS = 5;
constexpr int COMBINE_LAYER = 3;

#ifndef PNR_NW
#define PNR_NW 8
#endif
constexpr int NW = PNR_NW;        // waves per workgroup (8: 2 per SIMD, 16: 4 per SIMD)
constexpr int NTHREADS = NW * 64;
constexpr int SL = D_HID / NW;    // hidden features per wave (64)
constexpr int IT = SL / 32;       // feature tiles per wave (2)
constexpr int MT = 64;            // points per tile
constexpr int JT = MT / 32;       // point tiles (2)

// ---- per-wave weight stream, in "ring steps" (one ring step = IT fragments of 1 KiB) ----
constexpr int KS_IN = D_IN_PAD / 16;  // 4
constexpr int KS_BIG = D_HID / 16;    // 32
constexpr int KS_OUT = 4;             // lin_out: 4 real k-steps packed into ring steps 0,1 (x IT); 2,3 zero
// execution order of the GEMMs
enum Gemm {
    G_LIN_IN = 0, G_Z0, G_FC0_0, G_FC1_0, G_Z1, G_FC0_1, G_FC1_1, G_Z2, G_FC0_2, G_FC1_2,
    G_FC0_3, G_FC1_3, G_FC0_4, G_FC1_4, G_OUT, NGEMM
};
__host__ __device__ constexpr int gemm_ksteps(int g) {
    return g == G_LIN_IN ? KS_IN : (g == G_OUT ? KS_OUT : KS_BIG);
}
__host__ __device__ constexpr int gemm_offset(int g) {  // first ring step of GEMM g
    int o = 0;
    for (int i = 0; i < g; ++i) o += gemm_ksteps(i);
    return o;
}
constexpr int RS_VIEW_END = gemm_offset(G_FC0_3);  // 292: end of the per-view segment (blocks 0-2)
constexpr int RS_TOTAL = gemm_offset(NGEMM);       // 424
static_assert(RS_VIEW_END % 4 == 0 && RS_TOTAL % 4 == 0, "ring depth 4 needs aligned segments");

// "folded" inference stream: lin_z[b](z) is linear in the interpolated latent, so W_z[b] is applied to the feature
// grid once per scene (per-texel tables, pnr_fold_latent) and the three lin_z GEMMs leave the per-point stream.
__host__ __device__ constexpr bool gemm_is_linz(int g) { return g == G_Z0 || g == G_Z1 || g == G_Z2; }
__host__ __device__ constexpr int gemm_offset_fold(int g) {  // first ring step of GEMM g in the folded stream
    int o = 0;
    for (int i = 0; i < g; ++i) o += gemm_is_linz(i) ? 0 : gemm_ksteps(i);
    return o;
}
constexpr int RS_VIEW_END_F = gemm_offset_fold(G_FC0_3);  // 196
constexpr int RS_TOTAL_F = gemm_offset_fold(NGEMM);       // 328
static_assert(RS_VIEW_END_F % 4 == 0 && RS_TOTAL_F % 4 == 0, "ring depth 4 needs aligned segments");

constexpr int FRAG_ELEMS = 64 * 8;  // 64 lanes x 8 elements (1 KiB of 16-bit)
constexpr size_t WSTREAM_ELEMS_PER_WAVE = (size_t)RS_TOTAL * IT * FRAG_ELEMS;
constexpr size_t WSTREAM_BYTES = WSTREAM_ELEMS_PER_WAVE * NW * 2;  // 6,946,816 B

// ---- bias slots: one per accumulator (re)initialisation, already summed where two linears
// accumulate into the residual stream back to back ----
enum BiasSlot {
    B_IN_Z0 = 0,   // lin_in.bias + lin_z[0].bias
    B_FC0_0, B_FC1_0_Z1,  // blocks[0].fc_0 ; blocks[0].fc_1 + lin_z[1]
    B_FC0_1, B_FC1_1_Z2,
    B_FC0_2, B_FC1_2,
    B_FC0_3, B_FC1_3, B_FC0_4, B_FC1_4, NBIAS
};
constexpr int BIAS_FLOATS_PER_WAVE = IT * 2 * 16;  // [it][h][r]
constexpr size_t BIAS_OFFSET_BYTES = WSTREAM_BYTES;
constexpr size_t BIAS_BYTES = (size_t)NBIAS * NW * BIAS_FLOATS_PER_WAVE * 4;
constexpr size_t BOUT_OFFSET_BYTES = BIAS_OFFSET_BYTES + BIAS_BYTES;
constexpr size_t PACKED_BYTES = BOUT_OFFSET_BYTES + 32;  // lin_out bias (4 floats) | network flags word (+ pad)
constexpr int BOUT_FLAGS_INDEX = 4;  // 32-bit word behind lin_out's bias: bit 0 = combine_type "max" (util.py:467-468)
constexpr int BOUT_SCALE_INDEX = 5;  // next word: stream scale s (PnrMlpWeights.stream_scale_log2; split-operand blobs, else 0)
constexpr int BOUT_LIFT_INDEX = 6;   // s > 0: lin_out's weights are packed times 2^t (pnr_pack.hip, lin_out_lift), this is t; word 7: zero
constexpr int STREAM_SCALE_MAX = 30;

// hidden feature held by D-register r of half h in feature tile T (global tile index 0..15)
__host__ __device__ constexpr int feat_of(int T, int h, int r) {
    return 32 * T + (r & 3) + 8 * (r >> 2) + 4 * h;
}
// inverse: position of hidden feature f in "storage order" (element 32T + 16h + r of an activation row)
__host__ __device__ constexpr int slot_of(int f) {
    return (f & ~31) + 16 * ((f >> 2) & 1) + (f & 3) + 4 * ((f & 31) >> 3);
}

// ---- the 16x16x32 core of the split-operand INFERENCE kernel (pnr_split.hip, eval_split_kernel<.., TRAIN = false, ..>) ----
// v_mfma_f32_16x16x32_f16, lane (c = l & 15, g = l >> 4):  A: row c, the 8 K values of group g   B: col c, the same K group
//                                                          D: col c, rows 4 g + r (r = 0..3)
// A wave's 64 features are 4 row tiles t of 16, the 64 points of a tile 4 column tiles jt of 16.  The operand images, the tables
// and the bias table keep their storage order; what changes is which storage slot an accumulator register holds:
//   register r of tile (t, jt), lane (c, g)  =  wave-local storage slot slot16(t, g, r) of point 16 jt + c
// so that the 8 slots a lane owns in tiles 2m and 2m + 1 are the 8 consecutive slots 32 m + 8 g .. + 7: the lane's B fragment
// of K-step m (32 slots) of the wave's own block, as the MFMA wants it -- and 16 contiguous bytes of the image row.
constexpr int NT16 = SL / 16;            // feature tiles per wave (4)
constexpr int NJ16 = MT / 16;            // point tiles (4)
__host__ __device__ constexpr int slot16(int t, int g, int r) { return 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r; }
// MFMA row i = 4 g + r of tile t
__host__ __device__ constexpr int slot16_row(int t, int i) { return slot16(t, i >> 2, i & 3); }
// hidden feature in global storage slot s (the inverse of slot_of)
__host__ __device__ constexpr int feat_of_slot(int s) { return 32 * (s >> 5) + (s & 3) + 8 * ((s & 15) >> 2) + 4 * ((s >> 4) & 1); }
__host__ __device__ constexpr bool slot16_is_bijection() {
    bool seen[64] = {};
    for (int t = 0; t < 4; ++t)
        for (int g = 0; g < 4; ++g)
            for (int r = 0; r < 4; ++r) {
                const int s = slot16(t, g, r);
                if (s < 0 || s >= 64 || seen[s]) return false;
                seen[s] = true;
            }
    return true;
}
__host__ __device__ constexpr bool slot16_own_k() {  // K-step m, lane group g: registers 0..3 of tiles 2m, 2m+1 = slots 32m + 8g .. +7
    for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 4; ++g)
            for (int e = 0; e < 8; ++e)
                if (slot16(2 * m + (e >> 2), g, e & 3) != 32 * m + 8 * g + e) return false;
    return true;
}
__host__ __device__ constexpr bool feat_of_slot_inverts() {
    for (int f = 0; f < 512; ++f)
        if (feat_of_slot((f & ~31) + 16 * ((f >> 2) & 1) + (f & 3) + 4 * ((f & 31) >> 3)) != f) return false;
    return true;
}
static_assert(NW != 8 || (NT16 == 4 && NJ16 == 4), "16x16x32 core: 4 x 4 tiles per wave");
static_assert(slot16_is_bijection(), "slot16 must map (t, g, r) onto the wave's 64 storage slots one to one");
static_assert(slot16_own_k(), "K-step m of lane group g must be the slots 32 m + 8 g .. + 7");
static_assert(feat_of_slot_inverts(), "feat_of_slot is the inverse of slot_of");
// Its A fragments come out of the SAME packed (head, tail) streams the 32x32x16 core reads (pnr_pack.hip, OWNK; no second
// stream, no pack cost): a 16-byte piece of that stream is 8 K values of one weight row, which is what a lane of either shape
// holds, so the core only addresses the pieces differently.  One ring step of this core = one K = 32 step = two ring steps of
// the packed stream (IT fragments of 1 KiB each); lane (i, g) of row tile t takes
//   row         a16_row(t, i) of fragment `it` = t >> 1   (the packed rows are features in natural order, feat_of_slot(slot16_row))
//   K group g   from packed step 2 K + (g >> 1), lane half g & 1         (lin_in, and the blocks of the other waves: image order)
//               from packed step 2 K + (g & 1),  lane half g >> 1        (the wave's own block: the 32x32x16 core's register order)
// -- runs of four consecutive pieces (64 B), pairs of which share a 128-byte line.  lin_out's 4 rows sit in packed steps 0, 1.
constexpr int KS16_IN = D_IN_PAD / 32;   // 2
constexpr int KS16_BIG = D_HID / 32;     // 16: the wave's own block (2 steps) first, then the blocks of waves wv+1 .. wv+7
constexpr int KS16_OUT = KS_OUT / 2;     // 2
constexpr int RS16_VIEW_END = RS_VIEW_END_F / 2;  // 98
constexpr int RS16_TOTAL = RS_TOTAL_F / 2;        // 164
static_assert(RS16_VIEW_END == KS16_IN + 2 * COMBINE_LAYER * KS16_BIG && RS16_TOTAL == KS16_IN + 2 * N_BLOCKS * KS16_BIG + KS16_OUT,
              "one K = 32 step = two packed ring steps");
static_assert(RS16_VIEW_END % 2 == 0 && RS16_TOTAL % 2 == 0, "ring depth 2 needs aligned segments");
static_assert(NW != 8 || IT == 2, "the address maps below are for two packed fragments per ring step");
constexpr int RS16_BYTES = 2 * IT * 1024;  // one K = 32 step of one wave in one blob
// packed row (within its 32-row fragment t >> 1) of MFMA row i of row tile t
__host__ __device__ constexpr int a16_row(int t, int i) { return (i & 3) + 4 * (i >> 3) + 16 * ((i >> 2) & 1) + 8 * (t & 1); }
__host__ __device__ constexpr bool a16_row_is_the_feature() {
    for (int t = 0; t < 4; ++t)
        for (int i = 0; i < 16; ++i)
            if (feat_of_slot(slot16_row(t, i)) != 32 * (t >> 1) + a16_row(t, i)) return false;
    return true;
}
static_assert(a16_row_is_the_feature(), "a16_row must name the packed row that holds the feature of slot16_row");
// byte offset of lane (i, g)'s piece for row tile 0 inside a K = 32 step (row tile t: + (t >> 1) * 1024 + (t & 1) * 128)
__host__ __device__ constexpr int a16_lane_off(int i, int g, bool own) {
    return own ? (g & 1) * (IT * 1024) + (a16_row(0, i) + 32 * (g >> 1)) * 16 : (g >> 1) * (IT * 1024) + (a16_row(0, i) + 32 * (g & 1)) * 16;
}
// K-order check of the two maps against the packed stream's own definition (pnr_pack.hip, kind == 2): first storage slot of the 8
// K values of K-step j, lane half h -- own block: register order 32 (j >> 1) + 16 h + 8 (j & 1); other blocks: 16 j + 8 h
__host__ __device__ constexpr bool a16_k_order() {
    for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 4; ++g) {
            const int jo = 2 * m + (g & 1), ho = g >> 1, jg = 2 * m + (g >> 1), hg = g & 1;
            if (32 * (jo >> 1) + 16 * ho + 8 * (jo & 1) != 32 * m + 8 * g) return false;
            if (16 * jg + 8 * hg != 32 * m + 8 * g) return false;
        }
    return true;
}
static_assert(a16_k_order(), "K group g of K-step m must be the storage slots 32 m + 8 g .. + 7 in both maps");

// ---- backward chain: transposed weight stream, consumption order per tile ----
//   head (pooled, once): lin_out^T (4 ring steps, k-step 0 real) | fc_1[4]^T fc_0[4]^T fc_1[3]^T fc_0[3]^T
//   per source view    : fc_1[2]^T fc_0[2]^T fc_1[1]^T fc_0[1]^T fc_1[0]^T fc_0[0]^T
//                        | lin_z[2]^T lin_z[1]^T lin_z[0]^T  (d z_lat = sum_b dY_b W_z[b])
//                        | lin_in^T (4 ring steps: every wave contracts its own 64 hidden features, K-split)
enum BGemm { BG_OUT = 0, BG_FC1_4, BG_FC0_4, BG_FC1_3, BG_FC0_3, BG_FC1_2, BG_FC0_2, BG_FC1_1, BG_FC0_1, BG_FC1_0, BG_FC0_0,
             BG_Z2, BG_Z1, BG_Z0, BG_IN, NBGEMM };
__host__ __device__ constexpr int bgemm_offset(int g) { return g == 0 ? 0 : KS_IN + (g - 1) * KS_BIG; }
constexpr int BRS_HEAD_END = bgemm_offset(BG_FC1_2);  // 132
constexpr int BRS_TOTAL = bgemm_offset(BG_IN) + KS_IN;  // 424
static_assert(BRS_HEAD_END % 4 == 0 && BRS_TOTAL % 4 == 0, "ring depth 4 needs aligned segments");
constexpr size_t BWSTREAM_ELEMS_PER_WAVE = (size_t)BRS_TOTAL * IT * FRAG_ELEMS;
constexpr size_t BPACKED_BYTES = BWSTREAM_ELEMS_PER_WAVE * NW * 2;
constexpr int ROW_GOUT = 48;  // d(lin_out output) operand rows: 16 x 16-bit (4 real) + pad -> 3 slots/row

// ---- LDS map of the fused kernel (bytes), per point-tile size ----
constexpr int ROW_ACT = D_HID * 2 + 16;      // 1040 B per point row: 1024 B of 16-bit activations + one
                                             // 16-B slot of padding, so the 32 rows a ds_read_b128 touches
                                             // fall on distinct 16-B bank slots (65 slots/row, odd)
constexpr int ROW_IN = D_IN_PAD * 2 + 16;    // 144 B: 9 slots/row -> conflict-free b128 reads
// Tile<64>: two images -- Z (interpolated latent / table rows) and A (relu(x) / relu(net) operand) -- as the
//           unfolded, training and multi-view instantiations need (lin_z reads Z while A is live).
// Tile<96>: the folded single-view inference tile.  x + net for 96 points are 2 x 96 accumulator registers per
//           wave (the 256-register budget of 2 waves/SIMD allows no more), and ONE image: the table rows of
//           lin_z[b+1] are looked up into the activation image after fc_1[b] has finished reading it.  A weight
//           fragment fetched from L2 now feeds 3 MFMAs instead of 2: the L2->CU stream per point drops by a third.
template <int MT_> struct Tile {
    static_assert(MT_ == 64 || MT_ == 96, "supported point tiles");
    static constexpr int MT = MT_;            // points per tile
    static constexpr int JT = MT_ / 32;       // MFMA column tiles of 32 points
    static constexpr bool SINGLE_IMAGE = MT_ > 64;
    static constexpr int IN_LO_DELTA = 0;     // no split-operand image (pnr_split.hip has its own map)
    static constexpr int LDS_Z = 0;
    static constexpr int LDS_A = SINGLE_IMAGE ? 0 : MT_ * ROW_ACT;
    static constexpr int LDS_IN = LDS_A + MT_ * ROW_ACT;       // positional code + viewdir
    static constexpr int LDS_META = LDS_IN + MT_ * ROW_IN;     // per point: 4 corner offsets + 4 weights
    static constexpr int LDS_OUT = LDS_META + MT_ * 32;        // lin_out partials [NW][MT][4] floats
    // the 96-point tile has room for the network's bias table (11 slots x 512 fp32, accumulator order): the 20 accumulator
    // initialisations of a tile then read LDS instead of waiting for an L2 round trip in front of every GEMM
    static constexpr bool BIAS_IN_LDS = SINGLE_IMAGE;
    static constexpr int LDS_BIAS = LDS_OUT + NW * MT_ * 16;
    static constexpr int LDS_TOTAL = LDS_BIAS + (BIAS_IN_LDS ? 11 * NW * IT * 32 * 4 : 0);  // 152,576 B (64) / 151,552 B (96)
    static_assert(LDS_TOTAL <= 160 * 1024, "LDS budget");
};
// the 64-point map under its historical names (backward chain, training instantiation)
constexpr int LDS_Z = Tile<64>::LDS_Z;
constexpr int LDS_A = Tile<64>::LDS_A;
constexpr int LDS_IN = Tile<64>::LDS_IN;
constexpr int LDS_META = Tile<64>::LDS_META;
constexpr int LDS_OUT = Tile<64>::LDS_OUT;
constexpr int LDS_TOTAL = Tile<64>::LDS_TOTAL;

}  // namespace pnr
