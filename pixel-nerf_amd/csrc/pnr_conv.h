// pnr_conv.h -- what the encoder trunk's forward (pnr_conv.hip) and its training entries (pnr_conv_bwd.hip) share: the tile and
// slice constants of the convolution kernels, the cut of a reduction into slices, the host-side shape rules, and the launches of
// the forward convolution and the max pool, which the training forward reuses unchanged.  Host code only.
#pragma once
#include <cstdio>

#include "pnr_common.h"

namespace pnr {

constexpr int CV_BM = 32;   // output rows (channels) per workgroup
constexpr int CV_BN = 32;   // output columns (pixels of the whole batch, flattened: n, oy, ox) per workgroup
constexpr int CV_BK = 16;   // reduction terms a wave stages per chunk
constexpr int CV_LD = 36;   // LDS row stride in floats: 16-byte aligned rows, 4 floats of padding
constexpr int CV_WAVES = 4; // quarters of a slice = waves of a workgroup
constexpr int CV_SLICE = 576;  // a reduction of >= 2 CV_SLICE terms is cut into slices of about that length ...
constexpr int CV_MAX_SLICES = 8;  // ... at most this many

inline int conv_slices(long long K) { return K >= 2 * CV_SLICE ? (int)(K / CV_SLICE < CV_MAX_SLICES ? K / CV_SLICE : CV_MAX_SLICES) : 1; }
inline int conv_slice_len(long long K) {
    const int n = conv_slices(K);
    const long long per = (K + n - 1) / n;
    return (int)((per + 63) / 64 * 64);  // a quarter is a whole number of chunks
}

inline int conv_fail(const char *entry, const char *what) {
    char msg[256];
    std::snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return pnr_fail(PNR_E_INVALID, msg);
}

inline int conv_pad(int ksize) { return ksize / 2; }
inline int conv_out(int n, int ksize, int stride) { return (n + 2 * conv_pad(ksize) - ksize) / stride + 1; }
inline bool misaligned(const void *p) { return ((size_t)p & 3) != 0; }

constexpr size_t TRUNK_ALIGN = 256;
inline size_t align_up(size_t b) { return (b + TRUNK_ALIGN - 1) / TRUNK_ALIGN * TRUNK_ALIGN; }

// pnr_conv.hip
const char *conv_shape_defect(int N, int Cin, int H, int W, int Cout, int ksize, int stride);  // nullptr: nothing wrong
size_t conv_workspace_bytes(int N, int Cin, int H, int W, int Cout, int ksize, int stride);
void conv_launch(const float *x, int N, int Cin, int H, int W, const float *w, const float *scale, const float *shift, int Cout,
                 int ksize, int stride, const float *res, int relu, float *y, void *workspace, hipStream_t stream);
void pool_launch(const float *x, int N, int C, int H, int W, float *y, hipStream_t stream);

}  // namespace pnr
