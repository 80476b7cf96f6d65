// pnr_scatter_plan.h -- which form of the latent scatter (pnr_scatter.hip) a call takes, its geometry and the layout of the
// caller's workspace, decided in ONE place: the workspace-size entry, the ownership query and the launch all read the same
// ScatterPlan, so the kernels cannot be handed offsets the size entry did not count.  Host code and the kernels' constants.
#pragma once
#include <cstdlib>

#include "pnr_internal.h"  // device_cus
#include "pnr_layout.h"

namespace pnr {

constexpr int SCATTER_RUN = 16;             // latent_scatter_kernel: consecutive points per wavefront
constexpr int SLAB_MAX_BYTES = 160 * 1024;  // whole LDS
constexpr int OWNER_NT = 1024;
constexpr int SEG_NT = 1024;
constexpr int SEG_NSUB = 16;  // sub-ranges of an object's samples, one workgroup of scatter_segments_kernel each
constexpr int TILE_W = 32, TILE_TEXELS = TILE_W * TILE_W, TILE_CS = 16, TILE_ROW = TILE_CS + 1;
constexpr int TILE_LDS = TILE_TEXELS * TILE_ROW * 8;  // 139,264 B

struct TileGeom { int tx, ty, ntiles; };  // tiles per image row / column, per image

// slab: an fp64 slab per (image, cs-channel slice) in LDS; tiled: the same per 32 x 32-texel tile, one owner per grid element;
// atomic: global fp32 atomics (objects of 2^29+ samples, grids of > 8192 tiles, PIXELNERF_SCATTER_TILED=0 on a large grid)
enum ScatterForm { SCATTER_ATOMIC = 0, SCATTER_SLAB, SCATTER_TILED };

struct ScatterPlan {
    ScatterForm form;
    int images;       // SB * NS
    int cs, row;      // slab: channels per slice (16 / 8 / 4), fp64 slots per texel row (cs + 1, or 4 where the padding does not fit)
    int psplit;       // slab: workgroups that share an (image, slice) pair, 1 or 2
    int sub_len;      // slab, tiled: samples per sub-range of scatter_segments_kernel, a multiple of 64
    TileGeom tiles;   // tiled
    // byte offsets into the workspace.  slab, tiled: coords NS*P float2 | segs, SEG_NSUB x sub_len ints per image | nseg, SEG_NSUB
    // ints per image; tiled adds, 16-byte aligned, per (image, tile): tile_cnt | tile_off (+1) | cursor | entries, at most four per segment
    size_t coords, segs, nseg, tile_cnt, tile_off, cursor, entries;
    size_t bytes;     // the whole workspace (atomic: 0)
};

// channels per slab (16 / 8 / 4) and fp64 slots per texel row (padded by one when that fits the LDS; 64x64: unpadded); cs = 0: the
// grid does not fit.  Of the widths that fit, the widest one whose (image, slice) pairs fill the chip with at most TWO workgroups
// per pair is taken (4+ images of 32x32: 16 channels; 2 images: 8; 1 image: 4): wider slices read the gradient rows in longer
// pieces (profiles/r06_scatter_notes.md section 4), and at most two atomic adds per grid element keep the result independent of
// their order (onto a zeroed buffer two terms commute).
inline bool slab_row(int texels, int cs, int &row) {
    if ((size_t)texels * (cs + 1) * 8 <= SLAB_MAX_BYTES - 128) { row = cs + 1; return true; }
    if (cs == 4 && (size_t)texels * 4 * 8 <= SLAB_MAX_BYTES - 128) { row = 4; return true; }
    return false;
}
inline void scatter_slab_width(int texels, int images, int &cs, int &row) {
    cs = 0; row = 0;
    const int cus = device_cus();
    for (int c = 16; c >= 4; c >>= 1) {
        int r = 0;
        if (!slab_row(texels, c, r)) continue;
        if (!cs) { cs = c; row = r; }                                      // the widest that fits, unless a narrower one fills the chip
        if (2 * images * (C_LAT / c) >= cus) { cs = c; row = r; return; }  // ... with <= 2 workgroups per (image, slice)
    }
    if (cs) { int r = 0; if (slab_row(texels, 4, r)) { cs = 4; row = r; } }  // very few images: the most pairs there are
}
// Grids whose slab only fits 4 channels wide (2275 .. 5116 texels: the 64 x 64 grids of SRN-sized images) read the gradient rows in
// 16-byte pieces; cut into tiles they read 64-byte pieces like the small grids (4 x 64 x 64: 165 -> see profiles/r06_scatter_notes.md).
inline bool scatter_prefers_tiles(int cs, int texels) {
    int r = 0;
    return cs == 4 && !slab_row(texels, 8, r);  // (one or two small images also get cs == 4 -- for the pair count; they stay slabs)
}
// the tiled form needs 29-bit sample indices inside an object; beyond that (and with PIXELNERF_SCATTER_TILED=0) the global-atomic kernel runs
inline bool scatter_tiled_ok(long long pts, int ntiles) {
    if (ntiles > 8192) return false;  // (the binning histogram lives in LDS: 2 x 4 bytes per tile)
    static const bool off = [] { const char *e = getenv("PIXELNERF_SCATTER_TILED"); return e && e[0] == '0'; }();
    return !off && pts < (1LL << 29);
}

// sizes of a scatter call that a plan can be made for (the scene itself: scene_defect / check_scene, pnr_entry.h)
inline bool scatter_sizes_ok(const PnrScene &s, int R, int rays_per_obj, int K) {
    return R > 0 && K > 0 && rays_per_obj > 0 && (long long)rays_per_obj * s.SB == R;
}

// s: a checked scene (SB, NS > 0, Hl, Wl >= 2); R = SB * rays_per_obj > 0, K > 0
inline ScatterPlan scatter_plan(const PnrScene &s, int R, int rays_per_obj, int K) {
    ScatterPlan p = {};
    const int texels = s.Hl * s.Wl;
    const long long P = (long long)R * K, pts = (long long)rays_per_obj * K;  // points of the pass, of one object
    p.images = s.SB * s.NS;
    p.tiles.tx = (s.Wl + TILE_W - 1) / TILE_W; p.tiles.ty = (s.Hl + TILE_W - 1) / TILE_W; p.tiles.ntiles = p.tiles.tx * p.tiles.ty;
    scatter_slab_width(texels, p.images, p.cs, p.row);
    if (scatter_tiled_ok(pts, p.tiles.ntiles) && (p.cs == 0 || scatter_prefers_tiles(p.cs, texels))) p.form = SCATTER_TILED;
    else p.form = p.cs ? SCATTER_SLAB : SCATTER_ATOMIC;
    if (p.form != SCATTER_SLAB) p.cs = p.row = 0;
    if (p.form == SCATTER_ATOMIC) return p;
    p.sub_len = (int)(((pts + SEG_NSUB - 1) / SEG_NSUB + 63) / 64 * 64);
    p.coords = 0;
    p.segs = (size_t)s.NS * P * sizeof(float2);
    p.nseg = p.segs + (size_t)p.images * SEG_NSUB * p.sub_len * sizeof(int);
    p.bytes = p.nseg + (size_t)p.images * SEG_NSUB * sizeof(int);
    if (p.form == SCATTER_SLAB) {
        // the segments of an (image, slice) pair are split only when there are fewer pairs than compute units (and never below
        // ~one segment per thread: a segment is >= 1 sample), and in two at most (scatter_slab_width: two adds per grid element)
        const int owners = p.images * (C_LAT / p.cs);
        const long long rounds = (pts + 4LL * OWNER_NT - 1) / (4LL * OWNER_NT);
        p.psplit = (device_cus() + owners - 1) / owners;
        if (p.psplit > rounds) p.psplit = (int)rounds;
        if (p.psplit > 2) p.psplit = 2;
        if (p.psplit < 1) p.psplit = 1;
        return p;
    }
    const size_t it = (size_t)p.images * p.tiles.ntiles;
    p.tile_cnt = (p.bytes + 15) / 16 * 16;
    p.tile_off = p.tile_cnt + it * sizeof(int);
    p.cursor = p.tile_off + (it + 1) * sizeof(int);
    p.entries = p.cursor + it * sizeof(int);
    p.bytes = p.entries + 4 * (size_t)s.NS * P * sizeof(unsigned);
    return p;
}

}  // namespace pnr
