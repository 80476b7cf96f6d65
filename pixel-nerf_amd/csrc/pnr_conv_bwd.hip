// pnr_conv_bwd.hip -- the encoder's ResNet trunk under training: batch norm with batch statistics (forward and backward), the
// two gradients of a convolution, the backward of the 3x3 / stride-2 max pool, and the host loops that run a whole trunk forward
// (saving what the backward needs in the caller's buffer) and backward.  The raw convolution of the training forward is
// pnr_conv.hip's conv_affine_kernel with scale 1 and shift 0 (acc * 1 + 0 is acc).  Exact fp32 operands and results, no atomics,
// every output element written, no host synchronisation: a forward + backward can be captured into a HIP graph.
//
// DETERMINISM.  Every reduction runs in an order fixed by the layer's shape alone.
//   batch norm     A channel's M = N H W values are numbered m = (n H + y) W + x and cut into bn_slices(M) contiguous slices of
//                  bn_slice_len(M) values (a multiple of 256; both functions of M alone), one workgroup each.  Thread t of 256
//                  adds the values m = begin + t, begin + t + 256, ... of its slice in ascending order into one fp64 sum started
//                  from +0; the 256 sums are folded in the LDS, a[t] += a[t + s] for s = 128, 64, ..., 1; the slices are added
//                  in ascending order, ((s0 + s1) + s2) + ...  The mean is taken first, the variance is the mean of the fp64
//                  (v - mean)^2 in the same order.  The two sums of the backward (g and g xhat, the product formed in fp64) use
//                  the same order.
//   conv gradients Both are GEMMs run by conv_bwd_kernel, which has conv_affine_kernel's structure: a 32 x 32 output tile per
//                  workgroup, the reduction cut into slices, a slice into four quarters (one wave each), a quarter ONE chain of
//                  fused multiply-adds started from +0 in ascending order, the quarters added ((q0 + q1) + q2) + q3, the slices
//                  in ascending order in a second pass.  Terms that do not exist enter as zeros.
//                    data:   d_x[n,ci,iy,ix], reduction over k = (co k + ky) k + kx ascending, K = Cout k k terms, cut by
//                            conv_slices(K) / conv_slice_len(K) exactly as the forward cuts Cin k k.
//                    weight: d_w[co,ci,ky,kx], reduction over p = (n Ho + oy) Wo + ox ascending, P = N Ho Wo terms, cut into
//                            wgrad_slices(P) = 1 (P < 1024), 8 (P < 16384) or 64 slices of ceil(P / slices) rounded up to 64.
//   max pool       An input pixel adds the gradients of the <= 4 windows whose first maximum it is, in ascending (oy, ox).
// Tiles decide only WHICH elements a workgroup computes, never the order of a sum.
#include <cstdio>
#include <vector>

#include "pnr_conv.h"

namespace pnr {

// ================================================================================================ batch norm
constexpr long long BN_SLICE = 4096;   // a channel of >= 2 BN_SLICE values is cut into slices of about that length ...
constexpr int BN_MAX_SLICES = 64;      // ... at most this many

inline int bn_slices(long long M) { return M >= 2 * BN_SLICE ? (int)(M / BN_SLICE < BN_MAX_SLICES ? M / BN_SLICE : BN_MAX_SLICES) : 1; }
inline long long bn_slice_len(long long M) {
    const int n = bn_slices(M);
    const long long per = (M + n - 1) / n;
    return (per + 255) / 256 * 256;
}

struct BnParams {
    const float *v, *gamma, *beta, *res, *gy, *y_in, *mean_in, *invstd_in;
    float *y, *mean, *invstd, *running_mean, *running_var, *d_v, *d_gamma, *d_beta, *d_res;
    double *part;   // 2 C n_slices partial sums ...
    float *coef;    // ... and behind them 2 C fp32 means of the backward
    double eps, momentum;
    int C, HW, relu, frozen, n_slices;
    unsigned M, slice_len;
    long long total;
};

// the fixed fold of 256 fp64 sums (see DETERMINISM); every thread gets the result
__device__ inline double bn_fold(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__device__ inline double bn_slices_sum(const double *part, int n) {
    double s = part[0];
    for (int z = 1; z < n; ++z) s += part[z];
    return s;
}

// blockIdx = (slice, channel).  PASS 0: the slice's sum of v.  PASS 1: its sum of (v - mean)^2, mean from pass 0's partial sums
template <int PASS>
__global__ __launch_bounds__(256) void bn_stat_kernel(BnParams q) {
    __shared__ double sh[256];
    const int c = blockIdx.y, z = blockIdx.x;
    const unsigned begin = (unsigned)z * q.slice_len;
    const unsigned end = begin + q.slice_len < q.M ? begin + q.slice_len : q.M;
    double mean = 0.0;
    if (PASS == 1) mean = bn_slices_sum(q.part + (size_t)c * q.n_slices, q.n_slices) / (double)q.M;
    double acc = 0.0;
    for (unsigned m = begin + threadIdx.x; m < end; m += 256) {
        const unsigned n = m / (unsigned)q.HW, hw = m - n * (unsigned)q.HW;
        const double val = (double)q.v[((size_t)n * q.C + c) * q.HW + hw];
        if (PASS == 0) {
            acc += val;
        } else {
            const double d = val - mean;
            acc += d * d;
        }
    }
    const double sum = bn_fold(acc, sh);
    if (threadIdx.x == 0) q.part[(size_t)(PASS * q.C + c) * q.n_slices + z] = sum;
}

// one thread per channel: mean, invstd, the running statistics
__global__ __launch_bounds__(256) void bn_finalize_kernel(BnParams q) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= q.C) return;
    double mean, var;
    if (q.frozen) {
        mean = (double)q.running_mean[c];
        var = (double)q.running_var[c];
    } else {
        mean = bn_slices_sum(q.part + (size_t)c * q.n_slices, q.n_slices) / (double)q.M;
        var = bn_slices_sum(q.part + (size_t)(q.C + c) * q.n_slices, q.n_slices) / (double)q.M;
        if (q.running_mean) {
            const double m = q.momentum;
            q.running_mean[c] = (float)((1.0 - m) * (double)q.running_mean[c] + m * mean);
            q.running_var[c] = (float)((1.0 - m) * (double)q.running_var[c] + m * (var * (double)q.M / ((double)q.M - 1.0)));
        }
    }
    q.mean[c] = (float)mean;
    q.invstd[c] = (float)(1.0 / sqrt(var + q.eps));
}

__device__ inline float bn_xhat(float v, float mean, float invstd) { return __fmul_rn(__fsub_rn(v, mean), invstd); }

// y = act(fma(xhat, gamma, beta) + res)
__global__ __launch_bounds__(256) void bn_apply_kernel(BnParams q) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)q.total) return;
    const int c = (int)((idx / (size_t)q.HW) % q.C);
    float val = __fmaf_rn(bn_xhat(q.v[idx], q.mean[c], q.invstd[c]), q.gamma[c], q.beta[c]);
    if (q.res) val += q.res[idx];
    if (q.relu) val = val < 0.f ? 0.f : val;
    q.y[idx] = val;
}

// the gradient behind the ReLU mask (y > 0; y_in == NULL: no ReLU)
__device__ inline float bn_masked(const BnParams &q, size_t idx) {
    const float g = q.gy[idx];
    return (q.y_in && !(q.y_in[idx] > 0.f)) ? 0.f : g;
}

// blockIdx = (slice, channel): the slice's sums of g and g xhat; writes the masked gradient for the residual branch
__global__ __launch_bounds__(256) void bn_bwd_sum_kernel(BnParams q) {
    __shared__ double sh[256];
    const int c = blockIdx.y, z = blockIdx.x;
    const unsigned begin = (unsigned)z * q.slice_len;
    const unsigned end = begin + q.slice_len < q.M ? begin + q.slice_len : q.M;
    const float mean = q.mean_in[c], invstd = q.invstd_in[c];
    double sg = 0.0, sgx = 0.0;
    for (unsigned m = begin + threadIdx.x; m < end; m += 256) {
        const unsigned n = m / (unsigned)q.HW, hw = m - n * (unsigned)q.HW;
        const size_t idx = ((size_t)n * q.C + c) * q.HW + hw;
        const float g = bn_masked(q, idx);
        if (q.d_res) q.d_res[idx] = g;
        sg += (double)g;
        sgx += (double)g * (double)bn_xhat(q.v[idx], mean, invstd);
    }
    const double a = bn_fold(sg, sh), b = bn_fold(sgx, sh);
    if (threadIdx.x == 0) {
        q.part[(size_t)c * q.n_slices + z] = a;
        q.part[(size_t)(q.C + c) * q.n_slices + z] = b;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(BnParams q) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= q.C) return;
    const double sg = bn_slices_sum(q.part + (size_t)c * q.n_slices, q.n_slices);
    const double sgx = bn_slices_sum(q.part + (size_t)(q.C + c) * q.n_slices, q.n_slices);
    q.d_beta[c] = (float)sg;
    q.d_gamma[c] = (float)sgx;
    q.coef[c] = (float)(sg / (double)q.M);
    q.coef[q.C + c] = (float)(sgx / (double)q.M);
}

// d_v = gamma invstd (g - mean(g) - xhat mean(g xhat)); frozen: gamma invstd g
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnParams q) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)q.total) return;
    const int c = (int)((idx / (size_t)q.HW) % q.C);
    const float invstd = q.invstd_in[c];
    float t = bn_masked(q, idx);
    if (!q.frozen) {
        t = __fsub_rn(t, q.coef[c]);
        t = __fmaf_rn(-bn_xhat(q.v[idx], q.mean_in[c], invstd), q.coef[q.C + c], t);
    }
    q.d_v[idx] = __fmul_rn(__fmul_rn(q.gamma[c], invstd), t);
}

static size_t bn_workspace_bytes(int C, long long M) { return align_up((size_t)2 * C * bn_slices(M) * sizeof(double) + (size_t)2 * C * sizeof(float)); }

static const char *bn_defect(int N, int C, int H, int W, int frozen) {
    if (N < 0 || C <= 0 || H <= 0 || W <= 0) return "bad sizes (N >= 0; C, H, W > 0)";
    const long long M = (long long)N * H * W;
    if (M > 0x7fffffffLL) return "N H W must stay below 2^31";
    if (M * C > (1LL << 40)) return "the map must stay below 2^40 elements";
    if (N > 0 && !frozen && M < 2) return "batch statistics need more than one value per channel (N H W >= 2), as torch's batch norm in training mode";
    return nullptr;
}

static void bn_fill(BnParams &q, int N, int C, int H, int W, void *workspace) {
    q.C = C; q.HW = H * W; q.M = (unsigned)((long long)N * H * W); q.total = (long long)q.M * C;
    q.n_slices = bn_slices(q.M); q.slice_len = (unsigned)bn_slice_len(q.M);
    q.part = (double *)workspace;
    q.coef = (float *)(q.part + (size_t)2 * C * q.n_slices);
}

static void bn_forward_launch(BnParams q, hipStream_t s) {
    if (!q.frozen) {
        hipLaunchKernelGGL(bn_stat_kernel<0>, dim3(q.n_slices, q.C), dim3(256), 0, s, q);
        hipLaunchKernelGGL(bn_stat_kernel<1>, dim3(q.n_slices, q.C), dim3(256), 0, s, q);
    }
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((q.C + 255) / 256), dim3(256), 0, s, q);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((q.total + 255) / 256)), dim3(256), 0, s, q);
}

static void bn_backward_launch(BnParams q, hipStream_t s) {
    hipLaunchKernelGGL(bn_bwd_sum_kernel, dim3(q.n_slices, q.C), dim3(256), 0, s, q);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((q.C + 255) / 256), dim3(256), 0, s, q);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((q.total + 255) / 256)), dim3(256), 0, s, q);
}

// ================================================================================================ convolution gradients
constexpr long long WG_CUT_LO = 1024, WG_CUT_HI = 16384;
inline int wgrad_slices(long long P) { return P < WG_CUT_LO ? 1 : (P < WG_CUT_HI ? 8 : 64); }
inline int wgrad_slice_len(long long P) {
    const int n = wgrad_slices(P);
    const long long per = (P + n - 1) / n;
    return (int)((per + 63) / 64 * 64);
}

struct BwdParams {
    const float *dy, *src;  // src: the weights (data gradient) or the layer's input (weight gradient)
    float *out, *part;
    int N, Cin, H, W, Cout, Ho, Wo, stride, pad;
    int rows, cols, K, n_slices, slice_len;
    long long total;
};

// MODE 0, data gradient:   rows = ci, columns = input pixels (n, iy, ix), reduction k = (co, ky, kx)
// MODE 1, weight gradient: rows = co, columns = (ci, ky, kx),             reduction p = (n, oy, ox)
// 256 threads = 4 waves, wave q owns quarter q of the slice; blockIdx = (column tile, row tile, slice)
template <int KS, int MODE>
__global__ __launch_bounds__(256) void conv_bwd_kernel(BwdParams q) {
    __shared__ __attribute__((aligned(16))) float As[CV_WAVES][CV_BK][CV_LD];
    __shared__ __attribute__((aligned(16))) float Bs[CV_WAVES][CV_BK][CV_LD];
    __shared__ float Red[CV_WAVES][CV_BM][CV_BN + 1];
    constexpr int KK = KS * KS;
    const int t = threadIdx.x, wave = t >> 6, l = t & 63, ltx = l & 7, lty = l >> 3;
    const int c0 = blockIdx.x * CV_BN, r0 = blockIdx.y * CV_BM;
    const int quarter = q.slice_len / CV_WAVES;
    const long long s_end = (long long)(blockIdx.z + 1) * q.slice_len;
    const int slice_end = s_end < q.K ? (int)s_end : q.K;
    const long long kb0 = (long long)blockIdx.z * q.slice_len + (long long)wave * quarter;
    const int k_begin = kb0 < q.K ? (int)kb0 : q.K;
    const int k_end = min(k_begin + quarter, slice_end);
    const int HW = q.H * q.W, HoWo = q.Ho * q.Wo;

    // operand B: this lane always stages the same column (l % 32), rows kk = l / 32 + 2 i of its wave's chunk
    const int pl = l & 31, kb = l >> 5;
    const int col = c0 + pl;
    const bool col_ok = col < q.cols;
    int cn = 0, cy = 0, cx = 0;  // data: (n, iy + pad, ix + pad); weight: (ci, ky - pad, kx - pad)
    if (col_ok) {
        if (MODE == 0) {
            cn = col / HW;
            const int rem = col - cn * HW;
            cy = rem / q.W; cx = rem - cy * q.W;
            cy += q.pad; cx += q.pad;
        } else {
            cn = col / KK;
            const int r = col - cn * KK;
            cy = r / KS; cx = r - cy * KS;
            cy -= q.pad; cx -= q.pad;
        }
    }
    // operand A: rows r = l / 16 + 4 i of the tile, column kk = l % 16 of the chunk
    const int ak = l & 15, ac = l >> 4;

    float ra[8], rb[8];
    auto fetch = [&](int k0) {
        {
            const int k = k0 + ak;
            const bool k_ok = k < k_end;
            size_t base = 0, step = 0;
            if (k_ok) {
                if (MODE == 0) {  // w[co, row, ky, kx]
                    const int co = k / KK, r = k - co * KK;
                    base = (size_t)co * q.Cin * KK + r; step = KK;
                } else {          // dy[n, row, oy, ox]
                    const int n = k / HoWo, rem = k - n * HoWo;
                    base = (size_t)n * q.Cout * HoWo + rem; step = HoWo;
                }
            }
            const float *a = MODE == 0 ? q.src : q.dy;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = r0 + ac + 4 * i;
                ra[i] = (k_ok && row < q.rows) ? a[base + (size_t)row * step] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + kb + 2 * i;
            float v = 0.f;
            if (col_ok && k < k_end) {
                if (MODE == 0) {
                    const int co = k / KK, r = k - co * KK, ky = r / KS, kx = r - ky * KS;
                    const int ty = cy - ky, tx = cx - kx;  // oy s, ox s
                    if (ty >= 0 && tx >= 0 && (q.stride == 1 || ((ty & 1) == 0 && (tx & 1) == 0))) {
                        const int oy = q.stride == 1 ? ty : ty >> 1, ox = q.stride == 1 ? tx : tx >> 1;
                        if (oy < q.Ho && ox < q.Wo) v = q.dy[(((size_t)cn * q.Cout + co) * q.Ho + oy) * q.Wo + ox];
                    }
                } else {
                    const int n = k / HoWo, rem = k - n * HoWo, oy = rem / q.Wo, ox = rem - oy * q.Wo;
                    const int iy = oy * q.stride + cy, ix = ox * q.stride + cx;
                    if (iy >= 0 && iy < q.H && ix >= 0 && ix < q.W) v = q.src[(((size_t)n * q.Cin + cn) * q.H + iy) * q.W + ix];
                }
            }
            rb[i] = v;
        }
    };

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    fetch(k_begin);
    for (int c = 0; c < quarter; c += CV_BK) {  // the same trip count in every wave: the barriers below are workgroup-wide
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            As[wave][ak][ac + 4 * i] = ra[i];
            Bs[wave][kb + 2 * i][pl] = rb[i];
        }
        __syncthreads();
        if (c + CV_BK < quarter) fetch(k_begin + c + CV_BK);
#pragma unroll
        for (int kk = 0; kk < CV_BK; ++kk) {
            const float4 a = *reinterpret_cast<const float4 *>(&As[wave][kk][lty * 4]);
            const float4 b = *reinterpret_cast<const float4 *>(&Bs[wave][kk][ltx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __fmaf_rn(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Red[wave][lty * 4 + i][ltx * 4 + j] = acc[i][j];
    __syncthreads();
    for (int e = t; e < CV_BM * CV_BN; e += 256) {
        const int rl = e >> 5, ce = e & 31, row = r0 + rl, cj = c0 + ce;
        if (row >= q.rows || cj >= q.cols) continue;
        const float sum = ((Red[0][rl][ce] + Red[1][rl][ce]) + Red[2][rl][ce]) + Red[3][rl][ce];
        size_t idx;
        if (MODE == 0) {
            const int n = cj / HW, rem = cj - n * HW;
            idx = ((size_t)n * q.Cin + row) * HW + rem;
        } else {
            idx = (size_t)row * q.cols + cj;
        }
        if (q.n_slices > 1)
            q.part[(size_t)blockIdx.z * q.total + idx] = sum;
        else
            q.out[idx] = sum;
    }
}

// the fixed-order second pass of a sliced reduction: ((s0 + s1) + s2) + ...
__global__ __launch_bounds__(256) void conv_bwd_reduce_kernel(BwdParams q) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)q.total) return;
    float acc = q.part[idx];
    for (int z = 1; z < q.n_slices; ++z) acc += q.part[(size_t)z * q.total + idx];
    q.out[idx] = acc;
}

static const char *bwd_shape_defect(int N, int Cin, int H, int W, int Cout, int ksize, int stride) {
    if (const char *d = conv_shape_defect(N, Cin, H, W, Cout, ksize, stride)) return d;
    if ((long long)N * H * W > 0x7fffffe0LL) return "N H W must stay below 2^31";
    if ((long long)Cout * ksize * ksize > 0x7fffffffLL / 2) return "Cout k k must stay below 2^30";
    if ((long long)N * conv_out(H, ksize, stride) * conv_out(W, ksize, stride) > 0x7fff0000LL) return "N Ho Wo must stay below 2^31 - 2^16";
    if ((long long)N * Cin * H * W > (1LL << 40)) return "the input must stay below 2^40 elements";
    return nullptr;
}

static size_t dgrad_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize) {
    const int n_sl = conv_slices((long long)Cout * ksize * ksize);
    return n_sl == 1 ? 0 : (size_t)n_sl * N * Cin * H * W * sizeof(float);
}

static size_t wgrad_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride) {
    const int n_sl = wgrad_slices((long long)N * conv_out(H, ksize, stride) * conv_out(W, ksize, stride));
    return n_sl == 1 ? 0 : (size_t)n_sl * Cout * Cin * ksize * ksize * sizeof(float);
}

static BwdParams bwd_params(const float *dy, const float *src, int N, int Cin, int H, int W, int Cout, int ksize, int stride, float *out,
                            void *workspace) {
    BwdParams q = {};
    q.dy = dy; q.src = src; q.out = out; q.part = (float *)workspace;
    q.N = N; q.Cin = Cin; q.H = H; q.W = W; q.Cout = Cout; q.stride = stride; q.pad = conv_pad(ksize);
    q.Ho = conv_out(H, ksize, stride); q.Wo = conv_out(W, ksize, stride);
    return q;
}

template <int MODE>
static void bwd_launch(BwdParams q, int ksize, hipStream_t s) {
    const dim3 grid((q.cols + CV_BN - 1) / CV_BN, (q.rows + CV_BM - 1) / CV_BM, q.n_slices);
    auto k = ksize == 7 ? conv_bwd_kernel<7, MODE> : (ksize == 3 ? conv_bwd_kernel<3, MODE> : conv_bwd_kernel<1, MODE>);
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, q);
    if (q.n_slices > 1) hipLaunchKernelGGL(conv_bwd_reduce_kernel, dim3((unsigned)((q.total + 255) / 256)), dim3(256), 0, s, q);
}

static void dgrad_launch(const float *dy, const float *w, int N, int Cin, int H, int W, int Cout, int ksize, int stride, float *dx,
                         void *workspace, hipStream_t s) {
    BwdParams q = bwd_params(dy, w, N, Cin, H, W, Cout, ksize, stride, dx, workspace);
    q.rows = Cin; q.cols = N * H * W; q.K = Cout * ksize * ksize;
    q.n_slices = conv_slices(q.K); q.slice_len = conv_slice_len(q.K); q.total = (long long)q.cols * Cin;
    bwd_launch<0>(q, ksize, s);
}

static void wgrad_launch(const float *dy, const float *x, int N, int Cin, int H, int W, int Cout, int ksize, int stride, float *dw,
                         void *workspace, hipStream_t s) {
    BwdParams q = bwd_params(dy, x, N, Cin, H, W, Cout, ksize, stride, dw, workspace);
    q.rows = Cout; q.cols = Cin * ksize * ksize; q.K = N * q.Ho * q.Wo;
    q.n_slices = wgrad_slices(q.K); q.slice_len = wgrad_slice_len(q.K); q.total = (long long)q.cols * Cout;
    bwd_launch<1>(q, ksize, s);
}

// ================================================================================================ max pool backward, helpers
// an input pixel looks at the <= 2 x 2 windows that hold it (rows iy / 2 .. (iy + 1) / 2) and takes the gradient of each window
// whose FIRST maximum in (ky, kx) scan order it is -- maxpool_3x3s2_kernel's rule, NaN handling included
__global__ __launch_bounds__(256) void maxpool_3x3s2_bwd_kernel(const float *x, const float *g, float *dx, int H, int W, int Ho, int Wo,
                                                               long long total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)total) return;
    const int ix = (int)(idx % W), iy = (int)((idx / W) % H);
    const size_t plane = idx / ((size_t)W * H);
    const float *xp = x + plane * H * W;
    const float *gp = g + plane * Ho * Wo;
    float acc = 0.f;
    for (int oy = iy / 2; oy <= (iy + 1) / 2; ++oy) {
        if (oy >= Ho) continue;
        for (int ox = ix / 2; ox <= (ix + 1) / 2; ++ox) {
            if (ox >= Wo) continue;
            float m = -INFINITY;
            int ay = -1, ax = -1;
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = oy * 2 - 1 + ky;
                if (yy < 0 || yy >= H) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = ox * 2 - 1 + kx;
                    if (xx < 0 || xx >= W) continue;
                    const float v = xp[(size_t)yy * W + xx];
                    if (v > m || v != v) { m = v; ay = yy; ax = xx; }
                }
            }
            if (ay == iy && ax == ix) acc += gp[(size_t)oy * Wo + ox];
        }
    }
    dx[idx] = acc;
}

static void pool_bwd_launch(const float *x, const float *g, int N, int C, int H, int W, float *dx, hipStream_t s) {
    const int Ho = conv_out(H, 3, 2), Wo = conv_out(W, 3, 2);
    const long long total = (long long)N * C * H * W;
    hipLaunchKernelGGL(maxpool_3x3s2_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, g, dx, H, W, Ho, Wo, total);
}

__global__ __launch_bounds__(256) void add_kernel(const float *a, const float *b, float *out, long long total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < (size_t)total) out[idx] = a[idx] + b[idx];
}

static void add_launch(const float *a, const float *b, float *out, long long total, hipStream_t s) {
    hipLaunchKernelGGL(add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, b, out, total);
}

constexpr int UNIT_LEN = 512;  // the widest layer of the trunk
// ones[UNIT_LEN] then zeros[UNIT_LEN]: the (scale, shift) with which conv_affine_kernel is the raw convolution
__global__ __launch_bounds__(256) void unit_affine_kernel(float *u) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * UNIT_LEN) u[i] = i < UNIT_LEN ? 1.f : 0.f;
}

// ================================================================================================ the whole trunk
struct TrainLayer {
    int cin, h, w, cout, k, s, ho, wo;
    int level;            // >= 0: the layer's output is that pyramid level (the caller's), else it lies in `saved`
    size_t v_off, y_off, stat_off;  // in `saved`: the raw convolution, the layer's output, (mean, invstd)
    size_t out_bytes;
};

struct TrainPlan {
    std::vector<TrainLayer> L;
    int h0, w0, hp, wp;
    bool pool;
    size_t pool_off, saved_bytes;
    size_t act, conv_ws, bn_ws;   // backward scratch: one activation-sized buffer, the largest sliced reduction, the batch-norm sums
};

inline size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

static const char *train_plan(const int *blocks, int n_levels, int use_first_pool, int frozen, int NV, int H, int W, TrainPlan &t) {
    if (!blocks) return "null argument (blocks)";
    if (n_levels < 1 || n_levels > 5) return "n_levels must be in [1, 5]";
    for (int i = 0; i < 4; ++i)
        if (blocks[i] < 1 || blocks[i] > 64) return "every block count must be in [1, 64]";
    if (NV < 0 || H <= 0 || W <= 0) return "bad sizes (NV >= 0; H, W > 0)";
    t = {};
    size_t cursor = 0;
    const char *defect = nullptr;
    auto add = [&](int cin, int h, int w, int cout, int k, int s, int level) {
        if (defect) return;
        if ((defect = bwd_shape_defect(NV, cin, h, w, cout, k, s))) return;
        TrainLayer l = {};
        l.cin = cin; l.h = h; l.w = w; l.cout = cout; l.k = k; l.s = s; l.ho = conv_out(h, k, s); l.wo = conv_out(w, k, s); l.level = level;
        if ((defect = bn_defect(NV, cout, l.ho, l.wo, frozen))) return;
        l.out_bytes = align_up((size_t)NV * cout * l.ho * l.wo * sizeof(float));
        l.v_off = cursor; cursor += l.out_bytes;
        if (level < 0) { l.y_off = cursor; cursor += l.out_bytes; }
        l.stat_off = cursor; cursor += align_up((size_t)2 * cout * sizeof(float));
        t.act = max_sz(t.act, l.out_bytes);
        if (cin != 3) t.act = max_sz(t.act, align_up((size_t)NV * cin * h * w * sizeof(float)));
        t.conv_ws = max_sz(t.conv_ws, align_up(conv_workspace_bytes(NV, cin, h, w, cout, k, s)));
        t.conv_ws = max_sz(t.conv_ws, align_up(dgrad_workspace_bytes(NV, cin, h, w, cout, k)));
        t.conv_ws = max_sz(t.conv_ws, align_up(wgrad_workspace_bytes(NV, cin, h, w, cout, k, s)));
        t.bn_ws = max_sz(t.bn_ws, bn_workspace_bytes(cout, (long long)NV * l.ho * l.wo));
        t.L.push_back(l);
    };
    add(3, H, W, 64, 7, 2, 0);
    if (defect) return defect;
    t.h0 = t.L[0].ho; t.w0 = t.L[0].wo;
    t.pool = use_first_pool && n_levels > 1;
    t.hp = t.pool ? conv_out(t.h0, 3, 2) : t.h0; t.wp = t.pool ? conv_out(t.w0, 3, 2) : t.w0;
    if (t.pool) { t.pool_off = cursor; cursor += align_up((size_t)NV * 64 * t.hp * t.wp * sizeof(float)); }
    int h = t.hp, w = t.wp;
    for (int st = 0; st + 1 < n_levels; ++st) {
        const int C = 64 << st, s = st == 0 ? 1 : 2, cin = st == 0 ? 64 : C / 2;
        for (int b = 0; b < blocks[st]; ++b) {
            const int ci = b == 0 ? cin : C, sb = b == 0 ? s : 1;
            if (b == 0 && st > 0) add(ci, h, w, C, 1, 2, -1);
            add(ci, h, w, C, 3, sb, -1);
            h = conv_out(h, 3, sb); w = conv_out(w, 3, sb);
            add(C, h, w, C, 3, 1, b == blocks[st] - 1 ? st + 1 : -1);
            if (defect) return defect;
        }
    }
    t.saved_bytes = cursor;
    return nullptr;
}

constexpr int TRAIN_GRAD_BUFFERS = 6;
inline size_t train_unit_bytes() { return align_up((size_t)2 * UNIT_LEN * sizeof(float)); }
inline size_t train_workspace_bytes(const TrainPlan &t) { return train_unit_bytes() + t.conv_ws + t.bn_ws + TRAIN_GRAD_BUFFERS * t.act; }

// the checks the two whole-trunk entries share; no HIP call
static int train_check(const char *entry, const PnrConvTrainRecord *convs, int n_convs, const int *blocks, int n_levels, int use_first_pool,
                       int frozen, const float *images, int NV, int H, int W, const float *const *levels, const float *const *d_levels,
                       bool backward, const void *saved, size_t saved_bytes, const void *workspace, size_t workspace_bytes, TrainPlan &t) {
    if (const char *d = train_plan(blocks, n_levels, use_first_pool, frozen, NV, H, W, t)) return conv_fail(entry, d);
    if (!convs || !images || !levels || (backward && !d_levels)) return conv_fail(entry, backward ? "null argument (convs, images, levels, d_levels)" : "null argument (convs, images, levels)");
    if (n_convs != (int)t.L.size()) {
        char msg[128];
        std::snprintf(msg, sizeof(msg), "n_convs is %d, this trunk has %d convolutions", n_convs, (int)t.L.size());
        return conv_fail(entry, msg);
    }
    if (misaligned(images)) return conv_fail(entry, "misaligned pointer (images)");
    for (int l = 0; l < n_levels; ++l) {
        if (!levels[l] || misaligned(levels[l])) return conv_fail(entry, "null or misaligned level pointer");
        if (backward && (!d_levels[l] || misaligned(d_levels[l]))) return conv_fail(entry, "null or misaligned d_levels pointer");
    }
    for (int r = 0; r < n_convs; ++r) {
        const PnrConvTrainRecord &c = convs[r];
        const TrainLayer &l = t.L[r];
        char msg[200];
        if (c.cin != l.cin || c.cout != l.cout || c.ksize != l.k || c.stride != l.s) {
            std::snprintf(msg, sizeof(msg), "conv record %d is (cin %d, cout %d, ksize %d, stride %d), the trunk runs (%d, %d, %d, %d) there", r,
                          c.cin, c.cout, c.ksize, c.stride, l.cin, l.cout, l.k, l.s);
            return conv_fail(entry, msg);
        }
        if (!c.w || !c.gamma || !c.beta || misaligned(c.w) || misaligned(c.gamma) || misaligned(c.beta)) {
            std::snprintf(msg, sizeof(msg), "conv record %d: null or misaligned w / gamma / beta", r);
            return conv_fail(entry, msg);
        }
        if (misaligned(c.running_mean) || misaligned(c.running_var) || (!c.running_mean != !c.running_var) || (frozen && !c.running_mean)) {
            std::snprintf(msg, sizeof(msg), "conv record %d: running_mean / running_var misaligned, only one of them given, or missing in the frozen form", r);
            return conv_fail(entry, msg);
        }
        if (!backward && !frozen && c.running_mean && !(c.momentum >= 0.0 && c.momentum <= 1.0)) {
            std::snprintf(msg, sizeof(msg), "conv record %d: momentum must be in [0, 1]", r);
            return conv_fail(entry, msg);
        }
        if (!(c.eps >= 0.0)) {
            std::snprintf(msg, sizeof(msg), "conv record %d: eps must be >= 0", r);
            return conv_fail(entry, msg);
        }
        if (backward && (!c.d_w || !c.d_gamma || !c.d_beta || misaligned(c.d_w) || misaligned(c.d_gamma) || misaligned(c.d_beta))) {
            std::snprintf(msg, sizeof(msg), "conv record %d: null or misaligned d_w / d_gamma / d_beta", r);
            return conv_fail(entry, msg);
        }
    }
    if (t.saved_bytes > 0 && (!saved || saved_bytes < t.saved_bytes || ((size_t)saved & 7) != 0))
        return conv_fail(entry, "saved buffer too small or misaligned (pnr_encoder_trunk_train_saved_bytes, 8-byte aligned)");
    if (!workspace || workspace_bytes < train_workspace_bytes(t) || ((size_t)workspace & 7) != 0)
        return conv_fail(entry, "workspace too small or misaligned (pnr_encoder_trunk_train_workspace_bytes, 8-byte aligned)");
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

// ================================================================================================ per-layer entries
extern "C" size_t pnr_batchnorm2d_train_forward_workspace_bytes(int N, int C, int H, int W) {
    if (bn_defect(N, C, H, W, 1)) return 0;
    return bn_workspace_bytes(C, (long long)N * H * W);
}

extern "C" size_t pnr_batchnorm2d_backward_workspace_bytes(int N, int C, int H, int W) {
    return pnr_batchnorm2d_train_forward_workspace_bytes(N, C, H, W);
}

extern "C" int pnr_batchnorm2d_train_forward(const float *v, int N, int C, int H, int W, const float *gamma, const float *beta,
                                             float *running_mean, float *running_var, double eps, double momentum, int frozen,
                                             const float *res, int relu, float *y, float *save_mean, float *save_invstd, void *workspace,
                                             size_t workspace_bytes, void *stream) {
    static const char *const entry = "pnr_batchnorm2d_train_forward";
    if (const char *d = bn_defect(N, C, H, W, frozen)) return conv_fail(entry, d);
    if (!v || !gamma || !beta || !y || !save_mean || !save_invstd) return conv_fail(entry, "null argument (v, gamma, beta, y, save_mean, save_invstd)");
    if (!running_mean != !running_var) return conv_fail(entry, "running_mean and running_var come together or not at all");
    if (frozen && !running_mean) return conv_fail(entry, "the frozen form reads running_mean and running_var: null argument");
    if (misaligned(v) || misaligned(gamma) || misaligned(beta) || misaligned(y) || misaligned(save_mean) || misaligned(save_invstd) ||
        misaligned(running_mean) || misaligned(running_var) || misaligned(res))
        return conv_fail(entry, "misaligned pointer (every array is fp32: 4-byte aligned)");
    if (!(eps >= 0.0)) return conv_fail(entry, "eps must be >= 0");
    if (!frozen && running_mean && !(momentum >= 0.0 && momentum <= 1.0)) return conv_fail(entry, "momentum must be in [0, 1]");
    if (!workspace || ((size_t)workspace & 7) != 0 || workspace_bytes < bn_workspace_bytes(C, (long long)N * H * W))
        return conv_fail(entry, "workspace too small or misaligned (pnr_batchnorm2d_train_forward_workspace_bytes, 8-byte aligned)");
    if (N == 0) return PNR_OK;
    BnParams q = {};
    q.v = v; q.gamma = gamma; q.beta = beta; q.res = res; q.y = y; q.mean = save_mean; q.invstd = save_invstd;
    q.running_mean = running_mean; q.running_var = running_var; q.eps = eps; q.momentum = momentum; q.relu = relu != 0; q.frozen = frozen != 0;
    bn_fill(q, N, C, H, W, workspace);
    bn_forward_launch(q, (hipStream_t)stream);
    return pnr_check_launch(entry);
}

extern "C" int pnr_batchnorm2d_backward(const float *g_y, const float *y, const float *v, const float *save_mean, const float *save_invstd,
                                        const float *gamma, int N, int C, int H, int W, int frozen, float *d_v, float *d_gamma,
                                        float *d_beta, float *d_res, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *const entry = "pnr_batchnorm2d_backward";
    if (const char *d = bn_defect(N, C, H, W, frozen)) return conv_fail(entry, d);
    if (!g_y || !v || !save_mean || !save_invstd || !gamma || !d_v || !d_gamma || !d_beta)
        return conv_fail(entry, "null argument (g_y, v, save_mean, save_invstd, gamma, d_v, d_gamma, d_beta)");
    if (misaligned(g_y) || misaligned(y) || misaligned(v) || misaligned(save_mean) || misaligned(save_invstd) || misaligned(gamma) ||
        misaligned(d_v) || misaligned(d_gamma) || misaligned(d_beta) || misaligned(d_res))
        return conv_fail(entry, "misaligned pointer (every array is fp32: 4-byte aligned)");
    if (!workspace || ((size_t)workspace & 7) != 0 || workspace_bytes < bn_workspace_bytes(C, (long long)N * H * W))
        return conv_fail(entry, "workspace too small or misaligned (pnr_batchnorm2d_backward_workspace_bytes, 8-byte aligned)");
    if (N == 0) return PNR_OK;
    BnParams q = {};
    q.gy = g_y; q.y_in = y; q.v = v; q.mean_in = save_mean; q.invstd_in = save_invstd; q.gamma = gamma; q.frozen = frozen != 0;
    q.d_v = d_v; q.d_gamma = d_gamma; q.d_beta = d_beta; q.d_res = d_res;
    bn_fill(q, N, C, H, W, workspace);
    bn_backward_launch(q, (hipStream_t)stream);
    return pnr_check_launch(entry);
}

extern "C" size_t pnr_conv2d_backward_data_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride) {
    if (bwd_shape_defect(N, Cin, H, W, Cout, ksize, stride)) return 0;
    return dgrad_workspace_bytes(N, Cin, H, W, Cout, ksize);
}

extern "C" int pnr_conv2d_backward_data(const float *d_y, const float *w, int N, int Cin, int H, int W, int Cout, int ksize, int stride,
                                        float *d_x, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *const entry = "pnr_conv2d_backward_data";
    if (const char *d = bwd_shape_defect(N, Cin, H, W, Cout, ksize, stride)) return conv_fail(entry, d);
    if (!d_y || !w) return conv_fail(entry, "null argument (d_y, w)");
    if (misaligned(d_y) || misaligned(w) || misaligned(d_x) || misaligned(workspace))
        return conv_fail(entry, "misaligned pointer (every array is fp32: 4-byte aligned)");
    const size_t need = dgrad_workspace_bytes(N, Cin, H, W, Cout, ksize);
    if (d_x && need > 0 && (!workspace || workspace_bytes < need))
        return conv_fail(entry, "workspace too small (pnr_conv2d_backward_data_workspace_bytes)");
    if (N == 0 || !d_x) return PNR_OK;
    dgrad_launch(d_y, w, N, Cin, H, W, Cout, ksize, stride, d_x, workspace, (hipStream_t)stream);
    return pnr_check_launch(entry);
}

extern "C" int pnr_conv2d_backward_weight_slices(long long P) { return P <= 0 ? 0 : CV_WAVES * wgrad_slices(P); }

extern "C" size_t pnr_conv2d_backward_weight_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride) {
    if (bwd_shape_defect(N, Cin, H, W, Cout, ksize, stride)) return 0;
    return wgrad_workspace_bytes(N, Cin, H, W, Cout, ksize, stride);
}

extern "C" int pnr_conv2d_backward_weight(const float *d_y, const float *x, int N, int Cin, int H, int W, int Cout, int ksize, int stride,
                                          float *d_w, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *const entry = "pnr_conv2d_backward_weight";
    if (const char *d = bwd_shape_defect(N, Cin, H, W, Cout, ksize, stride)) return conv_fail(entry, d);
    if (N == 0) return conv_fail(entry, "an empty batch has no weight gradient (N >= 1)");
    if (!d_y || !x || !d_w) return conv_fail(entry, "null argument (d_y, x, d_w)");
    if (misaligned(d_y) || misaligned(x) || misaligned(d_w) || misaligned(workspace))
        return conv_fail(entry, "misaligned pointer (every array is fp32: 4-byte aligned)");
    const size_t need = wgrad_workspace_bytes(N, Cin, H, W, Cout, ksize, stride);
    if (need > 0 && (!workspace || workspace_bytes < need)) return conv_fail(entry, "workspace too small (pnr_conv2d_backward_weight_workspace_bytes)");
    wgrad_launch(d_y, x, N, Cin, H, W, Cout, ksize, stride, d_w, workspace, (hipStream_t)stream);
    return pnr_check_launch(entry);
}

extern "C" int pnr_maxpool2d_3x3s2_backward(const float *x, const float *g_y, int N, int C, int H, int W, float *d_x, void *stream) {
    static const char *const entry = "pnr_maxpool2d_3x3s2_backward";
    if (N < 0 || C <= 0 || H <= 0 || W <= 0) return conv_fail(entry, "bad sizes (N >= 0; C, H, W > 0)");
    if ((long long)N * C * H * W > (1LL << 40)) return conv_fail(entry, "the input must stay below 2^40 elements");
    if (!x || !g_y || !d_x) return conv_fail(entry, "null argument (x, g_y, d_x)");
    if (misaligned(x) || misaligned(g_y) || misaligned(d_x)) return conv_fail(entry, "misaligned pointer (every array is fp32: 4-byte aligned)");
    if (N == 0) return PNR_OK;
    pool_bwd_launch(x, g_y, N, C, H, W, d_x, (hipStream_t)stream);
    return pnr_check_launch(entry);
}

// ================================================================================================ whole-trunk entries
extern "C" size_t pnr_encoder_trunk_train_saved_bytes(const int *blocks, int n_levels, int use_first_pool, int NV, int H, int W) {
    TrainPlan t;
    if (train_plan(blocks, n_levels, use_first_pool, 1, NV, H, W, t)) return 0;
    return t.saved_bytes;
}

extern "C" size_t pnr_encoder_trunk_train_workspace_bytes(const int *blocks, int n_levels, int use_first_pool, int NV, int H, int W) {
    TrainPlan t;
    if (train_plan(blocks, n_levels, use_first_pool, 1, NV, H, W, t)) return 0;
    return train_workspace_bytes(t);
}

extern "C" int pnr_encoder_trunk_train_forward(const PnrConvTrainRecord *convs, int n_convs, const int *blocks, int n_levels,
                                               int use_first_pool, int frozen, const float *images, int NV, int H, int W,
                                               float *const *levels, void *saved, size_t saved_bytes, void *workspace,
                                               size_t workspace_bytes, void *stream) {
    static const char *const entry = "pnr_encoder_trunk_train_forward";
    TrainPlan t;
    if (int rc = train_check(entry, convs, n_convs, blocks, n_levels, use_first_pool, frozen, images, NV, H, W, levels, nullptr, false, saved,
                             saved_bytes, workspace, workspace_bytes, t))
        return rc;
    if (NV == 0) return PNR_OK;
    hipStream_t s = (hipStream_t)stream;
    char *sv = (char *)saved, *ws = (char *)workspace;
    float *unit = (float *)ws;
    void *cws = ws + train_unit_bytes();
    void *bws = ws + train_unit_bytes() + t.conv_ws;
    hipLaunchKernelGGL(unit_affine_kernel, dim3((2 * UNIT_LEN + 255) / 256), dim3(256), 0, s, unit);
    int r = 0;
    // one layer: raw convolution -> saved; batch norm (+ residual) (+ ReLU) -> the layer's output
    auto layer = [&](const float *x, const float *res, int relu) -> float * {
        const TrainLayer &l = t.L[r];
        const PnrConvTrainRecord &c = convs[r];
        ++r;
        float *v = (float *)(sv + l.v_off);
        float *y = l.level >= 0 ? levels[l.level] : (float *)(sv + l.y_off);
        conv_launch(x, NV, l.cin, l.h, l.w, c.w, unit, unit + UNIT_LEN, l.cout, l.k, l.s, nullptr, 0, v, cws, s);
        BnParams q = {};
        q.v = v; q.gamma = c.gamma; q.beta = c.beta; q.res = res; q.y = y;
        q.mean = (float *)(sv + l.stat_off); q.invstd = q.mean + l.cout;
        q.running_mean = c.running_mean; q.running_var = c.running_var; q.eps = c.eps; q.momentum = c.momentum; q.relu = relu; q.frozen = frozen != 0;
        bn_fill(q, NV, l.cout, l.ho, l.wo, bws);
        bn_forward_launch(q, s);
        return y;
    };
    const float *cur = layer(images, nullptr, 1);
    for (int st = 0; st + 1 < n_levels; ++st) {
        if (st == 0 && t.pool) {
            float *pool = (float *)(sv + t.pool_off);
            pool_launch(cur, NV, 64, t.h0, t.w0, pool, s);
            cur = pool;
        }
        for (int b = 0; b < blocks[st]; ++b) {
            const float *idt = cur;
            if (b == 0 && st > 0) idt = layer(cur, nullptr, 0);
            const float *mid = layer(cur, nullptr, 1);
            cur = layer(mid, idt, 1);
        }
    }
    return pnr_check_launch(entry);
}

extern "C" int pnr_encoder_trunk_backward(const PnrConvTrainRecord *convs, int n_convs, const int *blocks, int n_levels, int use_first_pool,
                                          int frozen, const float *images, int NV, int H, int W, const float *const *levels,
                                          const float *const *d_levels, const void *saved, size_t saved_bytes, float *d_images,
                                          void *workspace, size_t workspace_bytes, void *stream) {
    static const char *const entry = "pnr_encoder_trunk_backward";
    TrainPlan t;
    if (int rc = train_check(entry, convs, n_convs, blocks, n_levels, use_first_pool, frozen, images, NV, H, W, levels, d_levels, true, saved,
                             saved_bytes, workspace, workspace_bytes, t))
        return rc;
    if (misaligned(d_images)) return conv_fail(entry, "misaligned pointer (d_images)");
    if (NV == 0) return PNR_OK;
    hipStream_t s = (hipStream_t)stream;
    const char *sv = (const char *)saved;
    char *ws = (char *)workspace;
    void *cws = ws + train_unit_bytes();
    void *bws = ws + train_unit_bytes() + t.conv_ws;
    char *gb = ws + train_unit_bytes() + t.conv_ws + t.bn_ws;
    float *GA = (float *)gb, *GM = (float *)(gb + t.act), *DV = (float *)(gb + 2 * t.act), *DY = (float *)(gb + 3 * t.act),
          *DC = (float *)(gb + 4 * t.act), *DD = (float *)(gb + 5 * t.act);

    auto out_of = [&](int r) -> const float * { return t.L[r].level >= 0 ? levels[t.L[r].level] : (const float *)(sv + t.L[r].y_off); };
    auto elems_in = [&](int r) { return (long long)NV * t.L[r].cin * t.L[r].h * t.L[r].w; };
    // batch norm backward of layer r: g_y -> DV (and the masked gradient -> d_res), d_gamma, d_beta
    auto bn_bwd = [&](int r, const float *g_y, bool relu, float *d_res) {
        const TrainLayer &l = t.L[r];
        const PnrConvTrainRecord &c = convs[r];
        BnParams q = {};
        q.gy = g_y; q.y_in = relu ? out_of(r) : nullptr; q.v = (const float *)(sv + l.v_off);
        q.mean_in = (const float *)(sv + l.stat_off); q.invstd_in = q.mean_in + l.cout; q.gamma = c.gamma; q.frozen = frozen != 0;
        q.d_v = DV; q.d_gamma = c.d_gamma; q.d_beta = c.d_beta; q.d_res = d_res;
        bn_fill(q, NV, l.cout, l.ho, l.wo, bws);
        bn_backward_launch(q, s);
    };
    // convolution backward of layer r from DV: d_w, and the input's gradient -> dx (NULL: not wanted)
    auto conv_bwd = [&](int r, const float *x, float *dx) {
        const TrainLayer &l = t.L[r];
        wgrad_launch(DV, x, NV, l.cin, l.h, l.w, l.cout, l.k, l.s, convs[r].d_w, cws, s);
        if (dx) dgrad_launch(DV, convs[r].w, NV, l.cin, l.h, l.w, l.cout, l.k, l.s, dx, cws, s);
    };

    // the layers of every block, in the order the forward ran them
    struct Block { int down, c1, c2, st, b; };
    std::vector<Block> blk;
    {
        int r = 1;
        for (int st = 0; st + 1 < n_levels; ++st)
            for (int b = 0; b < blocks[st]; ++b) {
                Block k = {};
                k.down = (b == 0 && st > 0) ? r++ : -1;
                k.c1 = r++; k.c2 = r++; k.st = st; k.b = b;
                blk.push_back(k);
            }
    }
    const float *pooled = t.pool ? (const float *)(sv + t.pool_off) : levels[0];
    const float *g = d_levels[n_levels - 1];  // the gradient of the current block's output
    for (int i = (int)blk.size() - 1; i >= 0; --i) {
        const Block &k = blk[i];
        const float *cur = i == 0 ? pooled : (blk[i - 1].st == k.st ? out_of(blk[i - 1].c2) : levels[k.st]);  // the block's input
        bn_bwd(k.c2, g, true, GM);
        conv_bwd(k.c2, out_of(k.c1), DY);
        bn_bwd(k.c1, DY, true, nullptr);
        conv_bwd(k.c1, cur, DC);
        const long long n_in = elems_in(k.c1);
        if (k.down >= 0) {
            bn_bwd(k.down, GM, false, nullptr);
            conv_bwd(k.down, cur, DD);
            add_launch(DC, DD, GA, n_in, s);
        } else {
            add_launch(DC, GM, GA, n_in, s);
        }
        g = GA;
        if (k.b == 0) {  // the block's input is a pyramid level (behind the pool for stage 1): its own gradient joins
            if (k.st == 0 && t.pool) {
                pool_bwd_launch(levels[0], GA, NV, 64, t.h0, t.w0, DC, s);
                add_launch(DC, d_levels[0], GA, (long long)NV * 64 * t.h0 * t.w0, s);
            } else {
                add_launch(GA, d_levels[k.st], GA, n_in, s);
            }
        }
    }
    bn_bwd(0, g, true, nullptr);
    conv_bwd(0, images, d_images);
    return pnr_check_launch(entry);
}
