// pnr_scatter.hip -- latent scatter-add of the training backward: d(interpolated latent) -> d(feature grid), gfx950.
//
//   scatter_segments_kernel       projects every (view, point) once and cuts the rays into segments that share a grid cell
//   latent_scatter_owner_kernel   small grids: an fp64 slab in LDS per (image, channel slice), fed per ray segment
//   tile_bin_kernel, tile_scan_kernel, latent_scatter_tiled_kernel
//                                 large grids: the slab form on 32 x 32-texel tiles, one owner workgroup per tile
//   latent_scatter_kernel         global fp32 atomics, the fallback
// Which form runs, its geometry and the layout of the caller's workspace are decided once, by scatter_plan()
// (pnr_scatter_plan.h); the three pnr_latent_scatter* entries below only read the plan.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pnr_common.h"
#include "pnr_device.h"
#include "pnr_entry.h"
#include "pnr_internal.h"
#include "pnr_layout.h"
#include "pnr_scatter_plan.h"

namespace pnr {

// ---------------------------------------------------------------- latent scatter-add
// (global fp32 atomics: since round 6 only the fallback for objects of 2^29+ samples, grids of > 8192 tiles and PIXELNERF_SCATTER_TILED=0 --
// every other grid takes the LDS-slab forms further down.)  One wavefront per (view, run of SCATTER_RUN consecutive points); lane handles channels 8*lane..+7.
// Consecutive samples of a ray mostly fall into the same grid cell, so each of the 4 bilinear
// corners keeps a register accumulator that is flushed with atomics only when its texel changes
// (run-length merging: ~5x fewer atomics on the 32x32 sn64 grid).
#pragma clang fp contract(off)
__global__ void __launch_bounds__(CW * 64)
latent_scatter_kernel(const EvalParams q, const float *__restrict__ d_zlat, float *__restrict__ d_latent) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long runs_per_view = (q.P + SCATTER_RUN - 1) / SCATTER_RUN;
    const long long run = (long long)blockIdx.x * CW + wv;
    if (run >= runs_per_view * q.NS) return;
    const int view = (int)(run / runs_per_view);
    const long long g0 = (run % runs_per_view) * SCATTER_RUN;
    float acc[4][8];
    uint32_t cur[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[c][e] = 0.f;
    for (int j = 0; j < SCATTER_RUN; ++j) {
        const long long gl = g0 + j;
        if (gl >= q.P) break;
        const int g = (int)gl;
        const SamplePoint sp = sample_point(q, g, view);
        const Proj pr = project_point(q, sp.pose, sp.obj, view, sp.xr0, sp.xr1, sp.xr2, true);
        const float *src = d_zlat + ((size_t)view * q.P + g) * C_LAT + lane * 8;
        const f32x4 a = *reinterpret_cast<const f32x4 *>(src), b = *reinterpret_cast<const f32x4 *>(src + 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t off = __builtin_amdgcn_readfirstlane(pr.off[c]);  // identical in every lane
            if (off != cur[c]) {
                if (cur[c] != 0xffffffffu) {
                    float *dst = d_latent + cur[c] + lane * 8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if (acc[c][e] != 0.f) atomicAdd(dst + e, acc[c][e]);
                        acc[c][e] = 0.f;
                    }
                }
                cur[c] = off;
            }
            const float w = pr.w[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[c][e] += w * a[e];
                acc[c][4 + e] += w * b[e];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (cur[c] != 0xffffffffu) {
            float *dst = d_latent + cur[c] + lane * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (acc[c][e] != 0.f) atomicAdd(dst + e, acc[c][e]);
        }
}

// Small grids (the 32x32 / 64x64 grids of sn64 / SRN, anything whose (image, 4-channel) slab fits the LDS): dozens of samples
// hit every texel, so global atomics serialise on a few thousand addresses.  Instead a workgroup owns an (image, CS-channel
// slice) slab of the gradient grid in LDS (CS = 16 / 8 / 4 by what fits), walks the points of that image's object, and adds
// the slab to HBM once.  When there are at least as many (image, slice) pairs as compute units ONE workgroup walks all
// points and the slab goes out with plain read-add-write; otherwise TWO workgroups share the pair and meet in HBM with
// atomics (config 5 at CS = 16: 4 images x 32 slices x 2) -- never more (scatter_form picks the slice width by the image
// count): two adds onto a zeroed element commute, so the result does not depend on their order.
//
// What bounded the round-2..5 form of this kernel (thread = run of 8 consecutive samples x 8 channels, register accumulator
// per corner flushed when ITS texel changes; 64-bit fixed-point slab) -- tools/ubench/lds_atomic.hip + timing twins,
// profiles/r06_scatter_notes.md:
//   * the NUMBER of LDS atomic instructions, not their lanes: a 64-bit LDS atomic costs ~7.5 clocks of the CU's LDS pipe per
//     wave instruction whether 64 lanes or one are active.  Merging the adds of a run removed 70 % of the lane adds and not
//     one instruction -- some lane of the wave changes texel at every step, so every flush site executes;
//   * VALU: 64 slices each projected every point (~100 instructions), and every add converted fp32 -> int64 (17 instructions
//     in hipcc's expansion: 4350 of the kernel's 7700 static instructions);
//   * the L1: a lane read its 32 bytes of a 2 KiB gradient row as two dwordx4 -- 16 waves x 64 lines in flight against
//     256 lines of cache, each line fetched twice for a quarter of its bytes.
// Here the merge is done BEFORE lanes are assigned:
//   * scatter_segments_kernel projects every (view, point) ONCE -- the clamped grid position (ix, iy) of grid_coords
//     (pnr_geom.h), 8 bytes per point -- and cuts every ray into SEGMENTS: consecutive samples that share the cell (floor ix, floor iy),
//     i.e. all four corners, at most SEG_B of them; per image a sorted list of segment starts (ballot + scan compaction,
//     SEG_NSUB workgroups per image);
//   * latent_scatter_owner_kernel: lane = (segment, 4 channels); the CS / 4 lanes of a segment read adjacent 16-byte pieces of a
//     row in ONE load instruction.  A lane sums w_c * grad over its segment in fp32 registers and issues its 16 LDS adds once,
//     every lane of the wave active; segment bounds are requested two segments ahead, samples one segment ahead.
// The slab is fp64 and takes ds_add_f64 (39 clocks per wave instruction like ds_add_u64, 4.0 lanes/clk/CU with all 64 lanes on
// random banks; ds_add_f32 is executed one lane at a time for the whole CU: 192 clocks): no common scale, so no max pass over the
// gradients, no clamp, one conversion per add.  An fp32 value is exact in fp64 and a texel sums ~1e2-1e3 of them: the slab
// holds the sum to 2^-53, and its fp32 rounding can differ between two orders of the adds only on near-ties (the repeat
// runs of tools/gpu_scatter_bench.py agree bit for bit; not guaranteed).
// Same-box A/B, config 5 (4 x 32x32; 32 768 / 49 152 points), us per call: round-5 kernel 90 / 119, this one 48 / 59 (of which
// 5 are the segment pass); 4 x 64x64 grid: 400 -> 143-170.  What is left is the 16 ds_add_f64 per segment lane (~50 M lane adds
// per pass at 4 per clock and CU: ~25 us) and the chain list -> rows behind them.

#pragma clang fp contract(off)
// Workgroup (image = obj * NS + view, sub-range j of the object's samples: sub_len consecutive samples, a multiple of 64):
// coords[view * P + point] = (ix, iy); segs[(img * SEG_NSUB + j) * sub_len + k], k < nseg[img * SEG_NSUB + j] = first sample
// (index inside the object, ascending) of the k-th segment that starts in the sub-range.  A segment ends where the next one
// starts, or with its sub-range.
__global__ void __launch_bounds__(SEG_NT)
scatter_segments_kernel(const EvalParams q, float2 *__restrict__ coords, int *__restrict__ segs, int *__restrict__ nseg,
                        const int sub_len) {
    __shared__ int wave_total[SEG_NT / 64];
    __shared__ int carry;  // segments written by the previous rounds
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int img = blockIdx.x / SEG_NSUB, sub = blockIdx.x % SEG_NSUB, obj = img / q.NS, view = img % q.NS;
    const int pts = q.per_obj * q.K;  // < 2^31 (P is)
    const int s_begin = sub * sub_len, s_end = s_begin + sub_len < pts ? s_begin + sub_len : pts;
    const size_t row0 = (size_t)view * q.P + (size_t)obj * pts;
    int *list = segs + (size_t)blockIdx.x * sub_len;
    const float *pose = q.poses + (size_t)img * 12;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = s_begin; base < s_end; base += SEG_NT) {
        const int s = base + t;
        int cell = -1;
        if (s < s_end) {
            // the pose is the workgroup's (uniform), the rest is the forward's chain (pnr_geom.h)
            const RayPoint rp = ray_point(q, obj * pts + s);
            const float3 xr = rotate_point(pose, rp.X, rp.Y, rp.Z);
            float2 p = grid_coords(q, pose, obj, xr.x, xr.y, xr.z);
            if (!(p.x == p.x)) p.x = 0.f;  // NaN (point on the camera plane): as project_point
            if (!(p.y == p.y)) p.y = 0.f;
            coords[row0 + s] = p;
            cell = (int)floorf(p.y) * q.Wl + (int)floorf(p.x);
        }
        // segment start: first sample of a ray, a cell that differs from the previous sample's, or every SEG_B-th sample (a
        // segment is ONE trip of the owner kernel's loads: a ray that leaves the image clamps to one border cell for dozens of
        // samples, and the wave that held such a lane waited for 16 dependent trips -- 100 k of the kernel's 130 k cycles)
        const int prev = __shfl_up(cell, 1, 64);
        const bool head = s < s_end && (s % SEG_B == 0 || s % q.K == 0 || cell != prev);
        const unsigned long long m = __ballot(head);
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) wave_total[wv] = __popcll(m);
        __syncthreads();
        int off = carry, total = 0;
#pragma unroll
        for (int w = 0; w < SEG_NT / 64; ++w) {
            const int c = wave_total[w];
            if (w < wv) off += c;
            total += c;
        }
        if (head) list[off + before] = s;
        __syncthreads();
        if (t == 0) carry += total;
    }
    __syncthreads();
    if (t == 0) nseg[blockIdx.x] = carry;
}

template <int CS>
__global__ void __launch_bounds__(OWNER_NT)
latent_scatter_owner_kernel(const EvalParams q, const float *__restrict__ d_zlat, const float2 *__restrict__ coords,
                            const int *__restrict__ segs, const int *__restrict__ nseg, const int sub_len,
                            float *__restrict__ d_latent, const int psplit, const int row) {
    extern __shared__ double dslab[];  // [Hl*Wl][row]
    constexpr int LPS = CS / 4;        // lanes per segment (4 channels = one 16-byte load per sample and lane)
    constexpr int GRP = 32 / CS;       // slices that share a 128-byte line of a d_zlat / d_latent row
    const int t = threadIdx.x;
    const int texels = q.Hl * q.Wl, nslices = C_LAT / CS;
    int grp, sub;
    xcd_group_slot(blockIdx.x, gridDim.x / GRP, GRP, grp, sub);
    const int cs = (grp % (nslices / GRP)) * GRP + sub;
    const int pslice = (grp / (nslices / GRP)) % psplit;
    const int img = grp / ((nslices / GRP) * psplit);  // img = obj * NS + view
    const int obj = img / q.NS, view = img % q.NS;
    for (int i = t; i < texels * row; i += OWNER_NT) dslab[i] = 0.0;
    const long long pts = (long long)q.per_obj * q.K;  // points of this object
    const size_t row0 = (size_t)view * q.P + (size_t)obj * pts;  // first row of this (view, object) in d_zlat / coords
    const float *grad = d_zlat + row0 * C_LAT + cs * CS;
    const float2 *xy = coords + row0;
    // this image's segment lists: SEG_NSUB sub-ranges, read as one list through the running sums of their counts
    const int *list = segs + (size_t)img * SEG_NSUB * sub_len;
    __shared__ int pre[SEG_NSUB + 1];
    if (t == 0) {
        int run = 0;
        for (int j = 0; j < SEG_NSUB; ++j) { pre[j] = run; run += nseg[img * SEG_NSUB + j]; }
        pre[SEG_NSUB] = run;
    }
    __syncthreads();
    const int n = pre[SEG_NSUB];
    const int per = (n + psplit - 1) / psplit;
    const int i_begin = pslice * per, i_end = i_begin + per < n ? i_begin + per : n;
    const int Wl = q.Wl, Hl = q.Hl;
    __syncthreads();  // slab zeroed
    // lane = (segment, 4-channel part of the slice): the LPS lanes of a segment read LPS * 16 contiguous bytes of a gradient row
    // with ONE load instruction (a lane that read its 32 bytes as two dwordx4 fetched the line twice: 16 waves x 64 lines in
    // flight against the 256 lines of the L1)
    const int part = t % LPS;
    // segment i -> [s0, s1): sub-range j with pre[j] <= i < pre[j + 1] (binary search over the SEG_NSUB = 16 running sums in LDS)
    auto seg_bounds = [&](int i, int &s0, int &s1) {
        int j = 0;
#pragma unroll
        for (int step = SEG_NSUB / 2; step > 0; step >>= 1) j += i >= pre[j + step] ? step : 0;
        const int k = i - pre[j];
        const int *lj = list + (size_t)j * sub_len;
        const int sub_end = (j + 1) * sub_len < (int)pts ? (j + 1) * sub_len : (int)pts;
        s0 = lj[k];
        s1 = i + 1 < pre[j + 1] ? lj[k + 1] : sub_end;
    };
    // a segment is at most SEG_B samples: all its loads are issued before the first use
    auto load_batch = [&](int sb, int s1, float2 (&pos)[SEG_B], f32x4 (&v)[SEG_B]) {
#pragma unroll
        for (int b = 0; b < SEG_B; ++b) {
            pos[b] = make_float2(0.f, 0.f);
            v[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (sb + b < s1) {
                pos[b] = xy[sb + b];
                v[b] = reinterpret_cast<const f32x4 *>(grad + (size_t)(sb + b) * C_LAT)[part];
            }
        }
    };
    // Two-deep software pipeline over this lane's segments: a segment's bounds come out of the list (one round trip), its
    // samples out of the gradient rows (a second one that depends on the first) -- taken one after the other, ~8 segments
    // per lane were a chain of 16 loaded round trips (~2 us each at this access pattern).  The bounds are requested two
    // segments ahead and the first batch one segment ahead.
    constexpr int STRIDE = OWNER_NT / LPS;
    int i = i_begin + t / LPS;
    int s0 = 0, s1 = 0, s0n = 0, s1n = 0;
    float2 pos[SEG_B];
    f32x4 v[SEG_B];
    if (i < i_end) { seg_bounds(i, s0, s1); load_batch(s0, s1, pos, v); }
    if (i + STRIDE < i_end) seg_bounds(i + STRIDE, s0n, s1n);
    for (; i < i_end; i += STRIDE) {
        int s0nn = 0, s1nn = 0;
        if (i + 2 * STRIDE < i_end) seg_bounds(i + 2 * STRIDE, s0nn, s1nn);
        float2 posn[SEG_B];
        f32x4 vn[SEG_B];
        if (i + STRIDE < i_end) load_batch(s0n, s1n, posn, vn);
        f32x4 acc[4];
        const Corners k = segment_corner_sums(pos, v, Wl, Hl, acc);  // s1 - s0 <= SEG_B: scatter_segments_kernel cuts there
        const int x0 = k.x0, y0 = k.y0, x1 = k.x1(), y1 = k.y1();
        const int tex[4] = {y0 * Wl + x0, y0 * Wl + x1, y1 * Wl + x0, y1 * Wl + x1};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double *dst = dslab + tex[c] * row + part * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(dst + e, (double)acc[c][e]);  // ds_add_f64, no return
        }
        s0 = s0n; s1 = s1n; s0n = s0nn; s1n = s1nn;
#pragma unroll
        for (int b = 0; b < SEG_B; ++b) { pos[b] = posn[b]; v[b] = vn[b]; }
    }
    __syncthreads();
    float *out = d_latent + (size_t)img * texels * C_LAT + cs * CS;
    for (int i = t; i < texels * CS; i += OWNER_NT) {
        const double sv = dslab[(i / CS) * row + (i % CS)];
        if (sv != 0.0) {
            float *dst = out + (size_t)(i / CS) * C_LAT + (i % CS);
            if (psplit == 1) *dst += (float)sv;  // this workgroup is the only writer of the (image, slice) in this launch
            else atomicAdd(dst, (float)sv);
        }
    }
}

// ---- LARGE grids (DTU: 150 x 200 texels per image; anything whose (image, 4-channel) slab does not fit the LDS).  Rounds 2-5 sent
// them through global fp32 atomics (latent_scatter_kernel above): 25 M atomics per call of a 1-object x 3-view DTU training step,
// 965 us -- the largest kernel of that step -- and order-dependent.  Round 6: the slab form with the image cut into TILES of
// 32 x 32 texels.  A workgroup owns (image, tile, 16-channel slice): its slab is the tile (139 KiB of fp64), it takes the ray
// segments that touch the tile -- a segment's four corners can straddle up to four tiles, so it is listed in each -- adds only the
// corners that lie INSIDE the tile, and writes the tile back with plain read-add-write: every texel has one owner.
//   scatter_segments_kernel  (as above)           coords, segment starts per image
//   tile_bin_kernel<COUNT>                         per (image, tile): how many segments touch it
//   tile_scan_kernel                               running sums -> list offsets
//   tile_bin_kernel<FILL>                          segment (start | length - 1 << 29) into the lists of the tiles it touches (one atomic per entry:
//                                                  the order inside a list is not fixed -- the fp64 slab sum does not depend on it beyond 2^-53)
//   latent_scatter_tiled_kernel                    lane = (list entry, 4 channels): one trip of <= SEG_B samples, 16 predicated ds_add_f64
__device__ __forceinline__ void tiles_of_cell(int x0, int y0, int Wl, int Hl, int tx, int (&tiles)[4], int &n) {
    const int x1 = min(x0 + 1, Wl - 1), y1 = min(y0 + 1, Hl - 1);
    const int ax = x0 / TILE_W, bx = x1 / TILE_W, ay = y0 / TILE_W, by = y1 / TILE_W;
    n = 0;
    tiles[n++] = ay * tx + ax;
    if (bx != ax) tiles[n++] = ay * tx + bx;
    if (by != ay) {
        tiles[n++] = by * tx + ax;
        if (bx != ax) tiles[n++] = by * tx + bx;
    }
}

// Workgroup = 256 slots of the segment list of one (image, sub-range): every touched tile is first counted in an LDS histogram
// (ranks from the returning LDS atomic), then ONE global atomic per (workgroup, tile) -- the counters are a hundred addresses, and
// one global atomic per list entry serialised on them (2 x 66 us for the 36 k segments of a DTU step; 2 x ~5 us this way).
template <bool FILL>
__global__ void __launch_bounds__(256)
tile_bin_kernel(const EvalParams q, const float2 *__restrict__ coords, const int *__restrict__ segs, const int *__restrict__ nseg,
                const int sub_len, const TileGeom tg, int *__restrict__ tile_cnt, const int *__restrict__ tile_off,
                int *__restrict__ cursor, unsigned *__restrict__ entries) {
    extern __shared__ int hist[];  // [ntiles] counts, [ntiles] bases (FILL)
    const int t = threadIdx.x, k = blockIdx.x * 256 + t, lj = blockIdx.y;
    const int n_list = nseg[lj];
    if (blockIdx.x * 256 >= n_list) return;  // uniform
    for (int i = t; i < tg.ntiles; i += 256) hist[i] = 0;
    __syncthreads();
    const int img = lj / SEG_NSUB, j = lj % SEG_NSUB, obj = img / q.NS, view = img % q.NS;
    const int pts = q.per_obj * q.K;
    int tiles[4], rank[4], n = 0;
    unsigned entry = 0;
    if (k < n_list) {
        const int *list = segs + (size_t)lj * sub_len;
        const int s0 = list[k];
        const int sub_end = (j + 1) * sub_len < pts ? (j + 1) * sub_len : pts;
        const int s1 = k + 1 < n_list ? list[k + 1] : sub_end;
        const float2 p0 = coords[(size_t)view * q.P + (size_t)obj * pts + s0];
        tiles_of_cell((int)floorf(p0.x), (int)floorf(p0.y), q.Wl, q.Hl, tg.tx, tiles, n);
        entry = (unsigned)s0 | ((unsigned)(s1 - s0 - 1) << 29);
        for (int c = 0; c < n; ++c) rank[c] = atomicAdd(hist + tiles[c], 1);
    }
    __syncthreads();
    for (int i = t; i < tg.ntiles; i += 256) {
        const int c = hist[i];
        if (c) {
            if (!FILL) atomicAdd(tile_cnt + img * tg.ntiles + i, c);
            else hist[tg.ntiles + i] = atomicAdd(cursor + img * tg.ntiles + i, c);
        }
    }
    if (FILL) {
        __syncthreads();
        for (int c = 0; c < n; ++c) entries[tile_off[img * tg.ntiles + tiles[c]] + hist[tg.ntiles + tiles[c]] + rank[c]] = entry;
    }
}

// tile_off[i] = sum of tile_cnt[0 .. i) over all (image, tile) pairs, one workgroup; clears the FILL pass's cursors
__global__ void __launch_bounds__(1024) tile_scan_kernel(const int *__restrict__ tile_cnt, int n, int *__restrict__ tile_off, int *__restrict__ cursor) {
    __shared__ int part[1024];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int v = base + t < n ? tile_cnt[base + t] : 0;
        part[t] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan (n is a few hundred: one round)
            const int add = t >= o ? part[t - o] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        if (base + t < n) { tile_off[base + t] = carry + part[t] - v; cursor[base + t] = 0; }
        __syncthreads();
        if (t == 1023) carry += part[1023];
        __syncthreads();
    }
    if (t == 0) tile_off[n] = carry;
}

#pragma clang fp contract(off)
__global__ void __launch_bounds__(OWNER_NT)
latent_scatter_tiled_kernel(const EvalParams q, const float *__restrict__ d_zlat, const float2 *__restrict__ coords,
                            const unsigned *__restrict__ entries, const int *__restrict__ tile_off, const TileGeom tg,
                            float *__restrict__ d_latent) {
    extern __shared__ double dslab[];  // [32 x 32 texels][TILE_ROW]
    constexpr int LPS = TILE_CS / 4, NSL = C_LAT / TILE_CS, GRP = 32 / TILE_CS;
    const int t = threadIdx.x;
    int grp, sub;
    xcd_group_slot(blockIdx.x, gridDim.x / GRP, GRP, grp, sub);
    const int cs = (grp % (NSL / GRP)) * GRP + sub;
    const int it = grp / (NSL / GRP);  // (image, tile)
    const int img = it / tg.ntiles, tile = it % tg.ntiles;
    const int obj = img / q.NS, view = img % q.NS;
    const int tx0 = (tile % tg.tx) * TILE_W, ty0 = (tile / tg.tx) * TILE_W;
    const int e_begin = tile_off[it], e_end = tile_off[it + 1];
    if (e_begin == e_end) return;  // no ray crosses this tile: nothing to add (uniform over the workgroup)
    for (int i = t; i < TILE_TEXELS * TILE_ROW; i += OWNER_NT) dslab[i] = 0.0;
    const long long pts = (long long)q.per_obj * q.K;
    const size_t row0 = (size_t)view * q.P + (size_t)obj * pts;
    const float *grad = d_zlat + row0 * C_LAT + cs * TILE_CS;
    const float2 *xy = coords + row0;
    const int Wl = q.Wl, Hl = q.Hl;
    const int part = t % LPS;
    __syncthreads();
    for (int i = e_begin + t / LPS; i < e_end; i += OWNER_NT / LPS) {
        const unsigned en = entries[i];
        const int s0 = (int)(en & 0x1fffffffu), len = (int)(en >> 29) + 1;
        float2 pos[SEG_B];
        f32x4 v[SEG_B];
#pragma unroll
        for (int b = 0; b < SEG_B; ++b) {
            pos[b] = make_float2(0.f, 0.f);
            v[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (b < len) {
                pos[b] = xy[s0 + b];
                v[b] = reinterpret_cast<const f32x4 *>(grad + (size_t)(s0 + b) * C_LAT)[part];
            }
        }
        f32x4 acc[4];
        const Corners k = segment_corner_sums(pos, v, Wl, Hl, acc);
        const int x0 = k.x0, y0 = k.y0, x1 = k.x1(), y1 = k.y1();
        const int cx[4] = {x0, x1, x0, x1}, cy[4] = {y0, y0, y1, y1};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int lx = cx[c] - tx0, ly = cy[c] - ty0;
            if ((unsigned)lx < (unsigned)TILE_W && (unsigned)ly < (unsigned)TILE_W) {  // this tile owns the corner's texel
                double *dst = dslab + (ly * TILE_W + lx) * TILE_ROW + part * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) atomicAdd(dst + e, (double)acc[c][e]);  // ds_add_f64, no return
            }
        }
    }
    __syncthreads();
    // write-back: read-add-write of the touched elements, this workgroup being their only writer.  Done element by element -- LDS read,
    // branch, global load, add, store -- every touched element of a thread was a round trip of its own (a quarter of a tile's texels are
    // touched: ~4 dependent trips per thread); here all 16 loads of a thread are issued first (an untouched element reads a valid
    // dummy), then the touched ones are added and stored: one trip
    float *out = d_latent + (size_t)img * Hl * Wl * C_LAT + cs * TILE_CS;
    constexpr int WB = TILE_TEXELS * TILE_CS / OWNER_NT;  // 16 elements per thread
    static_assert(TILE_TEXELS * TILE_CS % OWNER_NT == 0, "write-back tiling");
    float add[WB], old[WB];
    float *dst[WB];
#pragma unroll
    for (int j = 0; j < WB; ++j) {
        const int i = t + j * OWNER_NT;
        const int tex = i / TILE_CS, ch = i % TILE_CS;
        const int x = tx0 + tex % TILE_W, y = ty0 + tex / TILE_W;
        const double sv = dslab[tex * TILE_ROW + ch];
        const bool touched = sv != 0.0 && x < Wl && y < Hl;
        add[j] = (float)sv;
        dst[j] = touched ? out + (size_t)(y * Wl + x) * C_LAT + ch : nullptr;
        old[j] = *(touched ? dst[j] : out);  // (`out` itself is always a valid address of the image)
    }
#pragma unroll
    for (int j = 0; j < WB; ++j)
        if (dst[j]) *dst[j] = old[j] + add[j];
}
#pragma clang fp contract(fast)

}  // namespace pnr

using namespace pnr;

extern "C" size_t pnr_latent_scatter_workspace_bytes(const PnrScene *s, int R, int rays_per_obj, int K) {
    if (scene_defect(s) || !scatter_sizes_ok(*s, R, rays_per_obj, K)) return 0;
    return scatter_plan(*s, R, rays_per_obj, K).bytes;
}

// 1: every element of the grid gradient is written by ONE workgroup with plain read-add-write (the tiled form): successive calls may
// accumulate into one buffer and the result still does not depend on any execution order; 0: the two-workgroups-per-pair / global-atomic
// forms, which are order-free only onto a zeroed buffer
extern "C" int pnr_latent_scatter_single_owner(const PnrScene *s, int R, int rays_per_obj, int K) {
    if (scene_defect(s) || !scatter_sizes_ok(*s, R, rays_per_obj, K)) return 0;
    return scatter_plan(*s, R, rays_per_obj, K).form == SCATTER_TILED ? 1 : 0;
}

// the scatter kernels hold a sample index in an int; latent_scatter_kernel (the global-atomic form) also takes project_point's 32-bit
// element offsets into the grid
extern "C" int pnr_latent_scatter(const PnrScene *s, const float *rays, const float *z, int R, int rays_per_obj, int K,
                                  const float *d_zlat, float *d_latent_nhwc, void *workspace, size_t workspace_bytes, void *stream) {
    EvalParams q = {};
    if (int rc = ray_samples(q, "pnr_latent_scatter", s, rays, z, R, rays_per_obj, K, false, {0, INDEX_I32, 0})) return rc;
    if (!d_zlat || !d_latent_nhwc) return pnr_fail(PNR_E_INVALID, "pnr_latent_scatter: bad argument");
    const ScatterPlan p = scatter_plan(*s, R, rays_per_obj, K);
    hipStream_t st = (hipStream_t)stream;
    if (p.form == SCATTER_ATOMIC) {
        if (int rc = check_limits(*s, q.P, {GRID_U32, 0, 0}, "pnr_latent_scatter")) return rc;
        const long long n = ((q.P + SCATTER_RUN - 1) / SCATTER_RUN) * q.NS;  // wavefronts
        hipLaunchKernelGGL(latent_scatter_kernel, dim3((unsigned)((n + CW - 1) / CW)), dim3(CW * 64), 0, st, q, d_zlat, d_latent_nhwc);
        return pnr_check_launch("pnr_latent_scatter");
    }
    if (!workspace || workspace_bytes < p.bytes || ((uintptr_t)workspace & 15) != 0)
        return pnr_fail(PNR_E_INVALID, "pnr_latent_scatter: workspace missing, misaligned (16 bytes) or smaller than "
                                       "pnr_latent_scatter_workspace_bytes()");
    char *scratch = reinterpret_cast<char *>(workspace);
    float2 *coords = reinterpret_cast<float2 *>(scratch + p.coords);
    int *segs = reinterpret_cast<int *>(scratch + p.segs), *nseg = reinterpret_cast<int *>(scratch + p.nseg);
    if (p.form == SCATTER_SLAB) {
        // one workgroup per (image, slice) takes all of the image's segments; p.psplit = 2 share them when there are fewer pairs than CUs
        const int owners = p.images * (C_LAT / p.cs);
        const size_t lds = (size_t)q.Hl * q.Wl * p.row * 8;
        auto k = p.cs == 16 ? latent_scatter_owner_kernel<16> : (p.cs == 8 ? latent_scatter_owner_kernel<8> : latent_scatter_owner_kernel<4>);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           SLAB_MAX_BYTES - 128);
        if (e != hipSuccess) return pnr_check_hip(e, "hipFuncSetAttribute(latent_scatter_owner_kernel)");
        hipLaunchKernelGGL(scatter_segments_kernel, dim3((unsigned)(p.images * SEG_NSUB)), dim3(SEG_NT), 0, st, q, coords, segs, nseg, p.sub_len);
        hipLaunchKernelGGL(k, dim3((unsigned)(owners * p.psplit)), dim3(OWNER_NT), lds, st, q, d_zlat, coords, segs, nseg, p.sub_len,
                           d_latent_nhwc, p.psplit, p.row);
        return pnr_check_launch("pnr_latent_scatter");
    }
    // large grid: 32 x 32-texel tiles, one owner workgroup per (image, tile, 16-channel slice) (latent_scatter_tiled_kernel)
    const TileGeom tg = p.tiles;
    const int IT = p.images * tg.ntiles;
    int *tile_cnt = reinterpret_cast<int *>(scratch + p.tile_cnt), *tile_off = reinterpret_cast<int *>(scratch + p.tile_off);
    int *cursor = reinterpret_cast<int *>(scratch + p.cursor);
    unsigned *entries = reinterpret_cast<unsigned *>(scratch + p.entries);
    hipError_t e = hipMemsetAsync(tile_cnt, 0, (size_t)IT * sizeof(int), st);
    if (e != hipSuccess) return pnr_check_hip(e, "hipMemsetAsync(tile counts)");
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(latent_scatter_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TILE_LDS);
    if (e != hipSuccess) return pnr_check_hip(e, "hipFuncSetAttribute(latent_scatter_tiled_kernel)");
    hipLaunchKernelGGL(scatter_segments_kernel, dim3((unsigned)(p.images * SEG_NSUB)), dim3(SEG_NT), 0, st, q, coords, segs, nseg, p.sub_len);
    const dim3 bgrid((unsigned)((p.sub_len + 255) / 256), (unsigned)(p.images * SEG_NSUB));
    const size_t bin_lds = 2 * (size_t)tg.ntiles * sizeof(int);
    hipLaunchKernelGGL(tile_bin_kernel<false>, bgrid, dim3(256), bin_lds, st, q, coords, segs, nseg, p.sub_len, tg, tile_cnt, tile_off, cursor, entries);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, st, tile_cnt, IT, tile_off, cursor);
    hipLaunchKernelGGL(tile_bin_kernel<true>, bgrid, dim3(256), bin_lds, st, q, coords, segs, nseg, p.sub_len, tg, tile_cnt, tile_off, cursor, entries);
    hipLaunchKernelGGL(latent_scatter_tiled_kernel, dim3((unsigned)(IT * (C_LAT / TILE_CS))), dim3(OWNER_NT), TILE_LDS, st, q, d_zlat, coords,
                       entries, tile_off, tg, d_latent_nhwc);
    return pnr_check_launch("pnr_latent_scatter");
}
