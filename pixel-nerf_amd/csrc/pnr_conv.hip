// pnr_conv.hip -- the ResNet trunk of the image encoder for inference (src/model/encoder.py:111-164 over torchvision's BasicBlock
// trunk): convolution + per-channel affine (+ residual) (+ ReLU) in one launch, the 3x3 / stride-2 max pool, and the host loop
// that runs a whole trunk through the two.  Exact fp32 (fused multiply-adds, fp32 accumulation), no atomics.
//
// DETERMINISM.  An output element's K = Cin k k terms are taken in ascending k = (ci k + ky) k + kx.  The reduction is cut into
// conv_slices(K) contiguous slices of conv_slice_len(K) terms (a multiple of 64), one workgroup each, and every slice into
// four quarters, one wave each (both cuts are functions of K alone).  A quarter is ONE fused-multiply-add chain started from +0;
// the quarters of a slice are added in ascending order through the LDS, ((q0 + q1) + q2) + q3, and the slices in ascending order
// in a second pass, ((s0 + s1) + s2) + ...  Nothing of that depends on the batch, the image size, the tile an element falls in
// or the launch: tiles decide only WHICH elements a workgroup computes.  Terms that fall on the zero padding, and the k beyond a
// quarter's end that fill its last staged chunk, enter as 0 * w or 0 * 0.
//
// WHY QUARTERS.  A 64 x 64 tile with one chain per element keeps a wave on 16 K dependent-issue multiply-adds: 24 us for K = 576
// whatever the image, and the late stages have a handful of tiles.  A 32 x 32 tile whose four waves share the reduction is a
// quarter of that per wave and four times the workgroups.
#include <cstdio>

#include "pnr_conv.h"  // the tile and slice constants, the shape rules: shared with the training entries (pnr_conv_bwd.hip)

namespace pnr {

struct ConvParams {
    const float *x, *w, *scale, *shift, *res;
    float *y, *part;       // part: n_slices planes of the output's size (n_slices > 1), else unused
    int N, Cin, H, W, Cout, Ho, Wo, stride, pad, K, n_slices, slice_len, relu;
    int P;                 // N Ho Wo
    long long total;       // N Cout Ho Wo
};

// y = act(acc * scale + shift + res): the product and the shift in one fused multiply-add, then the residual, then the ReLU
__device__ inline float conv_finish(float acc, float sc, float sh, const float *res, size_t idx, int relu) {
    float v = __fmaf_rn(acc, sc, sh);
    if (res) v += res[idx];
    if (relu) v = v < 0.f ? 0.f : v;  // a NaN stays a NaN, as torch's relu
    return v;
}

// 256 threads = 4 waves: a 32 x 32 tile of (output channel, output pixel); wave q owns quarter q of the slice's reduction and
// computes the whole tile over it, 4 x 4 per lane; blockIdx = (pixel tile, channel tile, slice)
template <int KS>
__global__ __launch_bounds__(256) void conv_affine_kernel(ConvParams q) {
    __shared__ __attribute__((aligned(16))) float As[CV_WAVES][CV_BK][CV_LD];
    __shared__ __attribute__((aligned(16))) float Bs[CV_WAVES][CV_BK][CV_LD];
    __shared__ float Red[CV_WAVES][CV_BM][CV_BN + 1];
    const int t = threadIdx.x, wave = t >> 6, l = t & 63, tx = l & 7, ty = l >> 3;
    const int p0 = blockIdx.x * CV_BN, co0 = blockIdx.y * CV_BM;
    const int quarter = q.slice_len / CV_WAVES;  // a multiple of CV_BK: every wave runs the same number of chunks
    const int slice_end = min((int)(blockIdx.z + 1) * q.slice_len, q.K);
    const int k_begin = blockIdx.z * q.slice_len + wave * quarter;
    const int k_end = min(k_begin + quarter, slice_end);
    const int HoWo = q.Ho * q.Wo;

    // operand B: this lane always stages the same pixel (l % 32), rows kk = l / 32 + 2 i of its wave's chunk
    const int pl = l & 31, kb = l >> 5;
    const int p = p0 + pl;
    const bool p_ok = p < q.P;
    int iy0 = 0, ix0 = 0;
    const float *xn = q.x;
    if (p_ok) {
        const int n = p / HoWo, rem = p - n * HoWo, oy = rem / q.Wo, ox = rem - oy * q.Wo;
        iy0 = oy * q.stride - q.pad; ix0 = ox * q.stride - q.pad;
        xn = q.x + (size_t)n * q.Cin * q.H * q.W;
    }
    // operand A: w (Cout, K) row-major; rows c = l / 16 + 4 i of the tile, column kk = l % 16 of the chunk
    const int ak = l & 15, ac = l >> 4;
    const float *wrow = q.w + (size_t)(co0 + ac) * q.K;

    float ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + ak;
            ra[i] = k < k_end ? wrow[(size_t)i * 4 * q.K + k] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + kb + 2 * i;
            float v = 0.f;
            if (p_ok && k < k_end) {
                const int ci = k / (KS * KS), r = k - ci * (KS * KS), ky = r / KS, kx = r - ky * KS;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < q.H && ix >= 0 && ix < q.W) v = xn[((size_t)ci * q.H + iy) * q.W + ix];
            }
            rb[i] = v;
        }
    };

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    fetch(k_begin);  // (a quarter beyond the slice's end stages zeros: k_end <= k_begin)
    for (int c = 0; c < quarter; c += CV_BK) {  // the same trip count in every wave: the barriers below are workgroup-wide
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            As[wave][ak][ac + 4 * i] = ra[i];
            Bs[wave][kb + 2 * i][pl] = rb[i];
        }
        __syncthreads();
        if (c + CV_BK < quarter) fetch(k_begin + c + CV_BK);  // the next chunk's loads fly under this chunk's arithmetic
#pragma unroll
        for (int kk = 0; kk < CV_BK; ++kk) {
            const float4 a = *reinterpret_cast<const float4 *>(&As[wave][kk][ty * 4]);
            const float4 b = *reinterpret_cast<const float4 *>(&Bs[wave][kk][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __fmaf_rn(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }

    // the four quarters meet in the LDS and are added in ascending order
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Red[wave][ty * 4 + i][tx * 4 + j] = acc[i][j];
    __syncthreads();
#pragma unroll
    for (int e = t; e < CV_BM * CV_BN; e += 256) {
        const int cl = e >> 5, pe = e & 31, pj = p0 + pe;
        if (pj >= q.P) continue;
        const float sum = ((Red[0][cl][pe] + Red[1][cl][pe]) + Red[2][cl][pe]) + Red[3][cl][pe];
        const int n = pj / HoWo, rem = pj - n * HoWo, co = co0 + cl;
        const size_t idx = ((size_t)n * q.Cout + co) * HoWo + rem;
        if (q.n_slices > 1)
            q.part[(size_t)blockIdx.z * q.total + idx] = sum;
        else
            q.y[idx] = conv_finish(sum, q.scale[co], q.shift[co], q.res, idx, q.relu);
    }
}

// the fixed-order second pass of a sliced reduction: ((s0 + s1) + s2) + ..., then the same epilogue
__global__ __launch_bounds__(256) void conv_reduce_kernel(ConvParams q) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)q.total) return;
    float acc = q.part[idx];
    for (int z = 1; z < q.n_slices; ++z) acc += q.part[(size_t)z * q.total + idx];
    const int co = (int)((idx / ((size_t)q.Ho * q.Wo)) % q.Cout);
    q.y[idx] = conv_finish(acc, q.scale[co], q.shift[co], q.res, idx, q.relu);
}

// nn.MaxPool2d(3, 2, 1): the padding never wins (a window always holds an image pixel); a NaN in the window is the result
__global__ __launch_bounds__(256) void maxpool_3x3s2_kernel(const float *x, float *y, int H, int W, int Ho, int Wo, long long total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)total) return;
    const int ox = (int)(idx % Wo), oy = (int)((idx / Wo) % Ho);
    const size_t plane = idx / ((size_t)Wo * Ho);
    const float *xp = x + plane * H * W;
    float m = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - 1 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const float v = xp[(size_t)iy * W + ix];
            m = (v > m || v != v) ? v : m;
        }
    }
    y[idx] = m;
}

// ------------------------------------------------------------------------------------------------ host
// what is wrong with a layer's shape (nullptr: nothing)
const char *conv_shape_defect(int N, int Cin, int H, int W, int Cout, int ksize, int stride) {
    if (N < 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return "bad sizes (N >= 0; Cin, H, W, Cout > 0)";
    if (!((ksize == 7 && stride == 2) || (ksize == 3 && stride == 1) || (ksize == 3 && stride == 2) || (ksize == 1 && stride == 2)))
        return "(ksize, stride) must be one of (7,2), (3,1), (3,2), (1,2)";
    if (!(Cin == 3 || Cin % 64 == 0)) return "Cin must be 3 or a multiple of 64";
    if (Cout % 64 != 0) return "Cout must be a multiple of 64";
    const long long Ho = conv_out(H, ksize, stride), Wo = conv_out(W, ksize, stride);
    if (Ho <= 0 || Wo <= 0) return "the image is smaller than the kernel allows (no output pixel)";
    if ((long long)Cin * ksize * ksize > 0x7fffffffLL / 2) return "Cin k k must stay below 2^30";
    if ((long long)N * Ho * Wo > 0x7fffffe0LL) return "N Ho Wo must stay below 2^31";
    if ((long long)N * Cout * Ho * Wo > (1LL << 40)) return "the output must stay below 2^40 elements";
    return nullptr;
}

size_t conv_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride) {
    const int n_sl = conv_slices((long long)Cin * ksize * ksize);
    if (n_sl == 1) return 0;
    return (size_t)n_sl * N * Cout * conv_out(H, ksize, stride) * conv_out(W, ksize, stride) * sizeof(float);
}

// every check of one layer; no HIP call
static int conv_check(const char *entry, const float *x, int N, int Cin, int H, int W, const float *w, const float *scale,
                      const float *shift, int Cout, int ksize, int stride, const float *res, const float *y, const void *workspace,
                      size_t workspace_bytes) {
    if (const char *d = conv_shape_defect(N, Cin, H, W, Cout, ksize, stride)) return conv_fail(entry, d);
    if (!x || !w || !scale || !shift || !y) return conv_fail(entry, "null argument (x, w, scale, shift, y)");
    if (misaligned(x) || misaligned(w) || misaligned(scale) || misaligned(shift) || misaligned(y) || misaligned(res) ||
        misaligned(workspace))
        return conv_fail(entry, "misaligned pointer (every array is fp32: 4-byte aligned)");
    const size_t need = conv_workspace_bytes(N, Cin, H, W, Cout, ksize, stride);
    if (need > 0 && (!workspace || workspace_bytes < need)) return conv_fail(entry, "workspace too small (pnr_conv2d_affine_workspace_bytes)");
    return PNR_OK;
}

// launches of one checked layer
void conv_launch(const float *x, int N, int Cin, int H, int W, const float *w, const float *scale, const float *shift, int Cout,
                 int ksize, int stride, const float *res, int relu, float *y, void *workspace, hipStream_t stream) {
    ConvParams q = {};
    q.x = x; q.w = w; q.scale = scale; q.shift = shift; q.res = res; q.y = y; q.part = (float *)workspace;
    q.N = N; q.Cin = Cin; q.H = H; q.W = W; q.Cout = Cout; q.stride = stride; q.pad = conv_pad(ksize);
    q.Ho = conv_out(H, ksize, stride); q.Wo = conv_out(W, ksize, stride);
    q.K = Cin * ksize * ksize; q.n_slices = conv_slices(q.K); q.slice_len = conv_slice_len(q.K); q.relu = relu != 0;
    q.P = N * q.Ho * q.Wo; q.total = (long long)q.P * Cout;
    const dim3 grid((q.P + CV_BN - 1) / CV_BN, Cout / CV_BM, q.n_slices);
    auto k = ksize == 7 ? conv_affine_kernel<7> : (ksize == 3 ? conv_affine_kernel<3> : conv_affine_kernel<1>);
    hipLaunchKernelGGL(k, grid, dim3(256), 0, stream, q);
    if (q.n_slices > 1)
        hipLaunchKernelGGL(conv_reduce_kernel, dim3((unsigned)((q.total + 255) / 256)), dim3(256), 0, stream, q);
}

static const char *pool_defect(const float *x, int N, int C, int H, int W, const float *y) {
    if (N < 0 || C <= 0 || H <= 0 || W <= 0) return "bad sizes (N >= 0; C, H, W > 0)";
    if ((long long)N * C * conv_out(H, 3, 2) * conv_out(W, 3, 2) > (1LL << 38)) return "the output must stay below 2^38 elements";
    if (!x || !y) return "null argument (x, y)";
    if (misaligned(x) || misaligned(y)) return "misaligned pointer (every array is fp32: 4-byte aligned)";
    return nullptr;
}

void pool_launch(const float *x, int N, int C, int H, int W, float *y, hipStream_t stream) {
    const int Ho = conv_out(H, 3, 2), Wo = conv_out(W, 3, 2);
    const long long total = (long long)N * C * Ho * Wo;
    hipLaunchKernelGGL(maxpool_3x3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, y, H, W, Ho, Wo, total);
}

// ---- the whole trunk: one walk that either sizes the scratch (run == false) or launches

struct TrunkShape {
    int h[5], w[5];      // level sizes
    int hp, wp;          // after the first pool (== level 0's without it)
    size_t act;          // bytes of one activation buffer: the largest stage output
    size_t pool;         // bytes of the pooled stem (0 without the pool or with one level)
    size_t conv_ws;      // bytes of the largest sliced reduction
    int n_convs;
};

static const char *trunk_defect(const int *blocks, int n_levels, int use_first_pool, int NV, int H, int W, TrunkShape &t) {
    if (!blocks) return "null argument (blocks)";
    if (n_levels < 1 || n_levels > 5) return "n_levels must be in [1, 5]";
    for (int i = 0; i < 4; ++i)
        if (blocks[i] < 1 || blocks[i] > 64) return "every block count must be in [1, 64]";
    if (NV < 0 || H <= 0 || W <= 0) return "bad sizes (NV >= 0; H, W > 0)";
    t = {};
    t.h[0] = conv_out(H, 7, 2); t.w[0] = conv_out(W, 7, 2);
    const bool pool = use_first_pool && n_levels > 1;
    t.hp = pool ? conv_out(t.h[0], 3, 2) : t.h[0]; t.wp = pool ? conv_out(t.w[0], 3, 2) : t.w[0];
    if (const char *d = conv_shape_defect(NV, 3, H, W, 64, 7, 2)) return d;
    t.pool = pool ? align_up((size_t)NV * 64 * t.hp * t.wp * sizeof(float)) : 0;
    t.n_convs = 1;
    int h = t.hp, w = t.wp;
    for (int st = 0; st + 1 < n_levels; ++st) {
        const int C = 64 << st, s = st == 0 ? 1 : 2, cin = st == 0 ? 64 : C / 2;
        if (const char *d = conv_shape_defect(NV, cin, h, w, C, 3, s)) return d;
        size_t ws = conv_workspace_bytes(NV, cin, h, w, C, 3, s);
        h = conv_out(h, 3, s); w = conv_out(w, 3, s);
        t.h[st + 1] = h; t.w[st + 1] = w;
        const size_t ws2 = conv_workspace_bytes(NV, C, h, w, C, 3, 1);
        ws = ws > ws2 ? ws : ws2;
        t.conv_ws = t.conv_ws > ws ? t.conv_ws : align_up(ws);
        const size_t act = align_up((size_t)NV * C * h * w * sizeof(float));
        t.act = t.act > act ? t.act : act;
        t.n_convs += 2 * blocks[st] + (st > 0);
    }
    return nullptr;
}

inline size_t trunk_bytes(const TrunkShape &t) { return t.pool + 4 * t.act + t.conv_ws; }

}  // namespace pnr

extern "C" int pnr_conv2d_affine_slices(int Cin, int ksize) {
    if (Cin <= 0 || ksize <= 0 || (long long)Cin * ksize * ksize > 0x7fffffffLL / 2) return 0;
    return pnr::CV_WAVES * pnr::conv_slices((long long)Cin * ksize * ksize);  // quarters per slice x slices
}

extern "C" size_t pnr_conv2d_affine_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride) {
    if (pnr::conv_shape_defect(N, Cin, H, W, Cout, ksize, stride)) return 0;
    return pnr::conv_workspace_bytes(N, Cin, H, W, Cout, ksize, stride);
}

extern "C" int pnr_conv2d_affine(const float *x, int N, int Cin, int H, int W, const float *w, const float *scale, const float *shift,
                                 int Cout, int ksize, int stride, const float *res, int relu, float *y, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    if (int rc = pnr::conv_check("pnr_conv2d_affine", x, N, Cin, H, W, w, scale, shift, Cout, ksize, stride, res, y, workspace,
                                 workspace_bytes))
        return rc;
    if (N == 0) return PNR_OK;
    pnr::conv_launch(x, N, Cin, H, W, w, scale, shift, Cout, ksize, stride, res, relu, y, workspace, (hipStream_t)stream);
    return pnr_check_launch("pnr_conv2d_affine");
}

extern "C" int pnr_maxpool2d_3x3s2(const float *x, int N, int C, int H, int W, float *y, void *stream) {
    if (const char *d = pnr::pool_defect(x, N, C, H, W, y)) return pnr::conv_fail("pnr_maxpool2d_3x3s2", d);
    if (N == 0) return PNR_OK;
    pnr::pool_launch(x, N, C, H, W, y, (hipStream_t)stream);
    return pnr_check_launch("pnr_maxpool2d_3x3s2");
}

extern "C" int pnr_encoder_level_shape(int H, int W, int level, int use_first_pool, int *h, int *w) {
    if (H <= 0 || W <= 0) return pnr::conv_fail("pnr_encoder_level_shape", "bad sizes (H, W > 0)");
    if (level < 0 || level > 4) return pnr::conv_fail("pnr_encoder_level_shape", "level must be in [0, 4]");
    int hh = pnr::conv_out(H, 7, 2), ww = pnr::conv_out(W, 7, 2);
    if (level >= 1 && use_first_pool) { hh = pnr::conv_out(hh, 3, 2); ww = pnr::conv_out(ww, 3, 2); }
    for (int l = 2; l <= level; ++l) { hh = pnr::conv_out(hh, 3, 2); ww = pnr::conv_out(ww, 3, 2); }
    if (h) *h = hh;
    if (w) *w = ww;
    return PNR_OK;
}

extern "C" size_t pnr_encoder_trunk_workspace_bytes(const int *blocks, int n_levels, int use_first_pool, int NV, int H, int W) {
    pnr::TrunkShape t;
    if (pnr::trunk_defect(blocks, n_levels, use_first_pool, NV, H, W, t)) return 0;
    return pnr::trunk_bytes(t);
}

extern "C" int pnr_encoder_trunk_forward(const PnrConvRecord *convs, int n_convs, const int *blocks, int n_levels, int use_first_pool,
                                         const float *images, int NV, int H, int W, float *const *levels, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    static const char *const entry = "pnr_encoder_trunk_forward";
    pnr::TrunkShape t;
    if (const char *d = pnr::trunk_defect(blocks, n_levels, use_first_pool, NV, H, W, t)) return pnr::conv_fail(entry, d);
    if (!convs || !images || !levels) return pnr::conv_fail(entry, "null argument (convs, images, levels)");
    if (n_convs != t.n_convs) {
        char msg[128];
        std::snprintf(msg, sizeof(msg), "n_convs is %d, this trunk has %d convolutions", n_convs, t.n_convs);
        return pnr::conv_fail(entry, msg);
    }
    if (pnr::misaligned(images)) return pnr::conv_fail(entry, "misaligned pointer (images)");
    for (int l = 0; l < n_levels; ++l)
        if (!levels[l] || pnr::misaligned(levels[l])) return pnr::conv_fail(entry, "null or misaligned level pointer");
    // every record against the layer the trunk has at its place, in the order the layers run: stem; per block its downsample
    // (the first block of stages 2..4), conv1, conv2
    {
        int r = 0;
        auto expect = [&](int cin, int cout, int k, int s) -> int {
            const PnrConvRecord &c = convs[r];
            char msg[160];
            if (c.cin != cin || c.cout != cout || c.ksize != k || c.stride != s) {
                std::snprintf(msg, sizeof(msg), "conv record %d is (cin %d, cout %d, ksize %d, stride %d), the trunk runs (%d, %d, %d, %d) there",
                              r, c.cin, c.cout, c.ksize, c.stride, cin, cout, k, s);
                return pnr::conv_fail(entry, msg);
            }
            if (!c.w || !c.scale || !c.shift || pnr::misaligned(c.w) || pnr::misaligned(c.scale) || pnr::misaligned(c.shift)) {
                std::snprintf(msg, sizeof(msg), "conv record %d: null or misaligned w / scale / shift", r);
                return pnr::conv_fail(entry, msg);
            }
            ++r;
            return PNR_OK;
        };
        if (int rc = expect(3, 64, 7, 2)) return rc;
        for (int st = 0; st + 1 < n_levels; ++st) {
            const int C = 64 << st, s = st == 0 ? 1 : 2, cin = st == 0 ? 64 : C / 2;
            for (int b = 0; b < blocks[st]; ++b) {
                if (b == 0 && st > 0)
                    if (int rc = expect(cin, C, 1, 2)) return rc;
                if (int rc = expect(b == 0 ? cin : C, C, 3, b == 0 ? s : 1)) return rc;
                if (int rc = expect(C, C, 3, 1)) return rc;
            }
        }
    }
    const size_t need = pnr::trunk_bytes(t);
    if (need > 0 && (!workspace || workspace_bytes < need || ((size_t)workspace & 3) != 0))
        return pnr::conv_fail(entry, "workspace too small (pnr_encoder_trunk_workspace_bytes)");
    if (NV == 0) return PNR_OK;

    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)workspace;
    float *pool = (float *)base;
    float *T = (float *)(base + t.pool), *D = (float *)(base + t.pool + t.act);
    float *B[2] = {(float *)(base + t.pool + 2 * t.act), (float *)(base + t.pool + 3 * t.act)};
    void *cws = base + t.pool + 4 * t.act;
    int r = 0;
    auto conv = [&](const float *x, int cin, int h, int w, const float *res, int relu, float *y) {
        const PnrConvRecord &c = convs[r++];
        pnr::conv_launch(x, NV, cin, h, w, c.w, c.scale, c.shift, c.cout, c.ksize, c.stride, res, relu, y, cws, s);
    };
    conv(images, 3, H, W, nullptr, 1, levels[0]);
    const float *cur = levels[0];
    int h = t.h[0], w = t.w[0];
    for (int st = 0; st + 1 < n_levels; ++st) {
        const int C = 64 << st, cin = st == 0 ? 64 : C / 2;
        if (st == 0 && use_first_pool) {
            pnr::pool_launch(cur, NV, 64, h, w, pool, s);
            cur = pool; h = t.hp; w = t.wp;
        }
        for (int b = 0; b < blocks[st]; ++b) {
            const int ci = b == 0 ? cin : C, ho = b == 0 ? t.h[st + 1] : h, wo = b == 0 ? t.w[st + 1] : w;
            const float *idt = cur;
            if (b == 0 && st > 0) { conv(cur, ci, h, w, nullptr, 0, D); idt = D; }
            conv(cur, ci, h, w, nullptr, 1, T);
            float *out = b == blocks[st] - 1 ? levels[st + 1] : B[b & 1];
            conv(T, C, ho, wo, idt, 1, out);
            cur = out; h = ho; w = wo;
        }
    }
    return pnr_check_launch(entry);
}
