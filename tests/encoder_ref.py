"""
fp64 restatement of the encoder trunk's layers (pixel-nerf_amd/csrc/pnr_conv.hip) and the DERIVED per-element bound of one layer,
in the manner of tests/gemm_ref.py, whose gamma, U, FTZ, product and input families it uses.  A helper, not a test:
tests/test_encoder_ref_host.py proves what is claimed here (no GPU), tests/test_hip_encoder_trunk.py holds the kernels to it,
profiles/encoder_notes.md has the measured figures.

LAYER.   y[n,co,oy,ox] = act((sum_{ci,ky,kx} x[n,ci, oy s + ky - p, ox s + kx - p] w[co,ci,ky,kx]) scale[co] + shift[co] + res)
with zeros outside the image, written reduction-last as gemm_ref.product(A, B):  A (N Ho Wo, K) the gathered patches
(im2col), B (Cout, K) the weights, K = Cin k k in (ci, ky, kx) order.

BOUND.   With S = sum |x| |w|, acc the sum, a = acc scale, value = a + shift + res and n_sl the slices the kernel adds up
(pnr_conv2d_affine_slices):

    bound = (gamma(K + n_sl) + U) S |scale| + 3 U (|value| + |a| + |shift| + |res|) + (K + n_sl) FTZ max(|scale|, 1) [S > 0]

    accumulation   K products and n_sl partial sums in any order, each addition one rounding of relative size <= U: gamma(K + n_sl) S.
    products       fp32 x fp32 is not exact in fp32: + U S (a fused multiply-add spends that rounding in the addition; it is
                   granted anyway, the arithmetic class allows either).
    epilogue       three operations (scale, shift, residual), each one rounding of a number no larger than
                   |value| + |a| + |shift| + |res|.
    subnormal      a sum below 2^-126 may be flushed: (K + n_sl) FTZ, scaled; not where S = 0 -- a sum of zeros is zero, and the
                   output is then exactly shift + res.
ReLU is 1-Lipschitz: |relu(u) - relu(v)| <= |u - v|, so the bound of the value before the ReLU holds behind it.
Nothing here is fitted to the kernel.
"""
import copy

import numpy as np
import torch

from gemm_ref import FTZ, U, cancelling, exact_ints, gamma, product, ranged  # noqa: F401 (the tests take the families from here)

CHANNELS = (64, 64, 128, 256, 512)


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def im2col(x, k, s, p):
    """x (N,Cin,H,W) -> (N Ho Wo, Cin k k) float64 patches, zeros outside the image, columns in (ci, ky, kx) order"""
    x = np.asarray(x, np.float64)
    N, C, H, W = x.shape
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    xp = np.zeros((N, C, H + 2 * p + s, W + 2 * p + s))
    xp[:, :, p:p + H, p:p + W] = x
    cols = np.empty((N, Ho, Wo, C, k, k))
    for ky in range(k):
        for kx in range(k):
            cols[:, :, :, :, ky, kx] = xp[:, :, ky:ky + s * Ho:s, kx:kx + s * Wo:s][:, :, :Ho, :Wo].transpose(0, 2, 3, 1)
    return cols.reshape(N * Ho * Wo, C * k * k)


def _nchw(flat, N, Ho, Wo):
    """(N Ho Wo, Cout) -> (N, Cout, Ho, Wo)"""
    return flat.reshape(N, Ho, Wo, -1).transpose(0, 3, 1, 2)


def conv_affine(x, w, scale, shift, res, relu, k, s, p, mut=None):
    """The layer in float64.  -> (y (N,Cout,Ho,Wo), A, B): A, B the im2col operands of gemm_ref.product.
    `mut` restates it WRONGLY for tests/test_encoder_ref_host.py: "flip" (kernel flipped), "pad" (pad off by one),
    "phase" (stride phase off by one), "transpose" (channels of w transposed; Cin == Cout only)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, _, H, W = x.shape
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    if mut == "flip":
        w = w[:, :, ::-1, ::-1]
    if mut == "transpose":
        w = w.transpose(1, 0, 2, 3)
    if mut == "pad":       # samples x one pixel further down-right: pad p - 1, cropped / extended to the same output size
        xs = np.zeros_like(x); xs[:, :, :-1, :-1] = x[:, :, 1:, 1:]; x = xs
    if mut == "phase":     # starts the strided walk one input pixel late along x
        xs = np.zeros_like(x); xs[:, :, :, :-1] = x[:, :, :, 1:]; x = xs
    A = im2col(x, k, s, p)
    B = w.reshape(w.shape[0], -1)
    v = _nchw((A @ B.T) * np.asarray(scale, np.float64)[None, :] + np.asarray(shift, np.float64)[None, :], N, Ho, Wo)
    if res is not None:
        v = v + np.asarray(res, np.float64)
    return (np.maximum(v, 0.0) if relu else v), A, B


def layer_bound(A, B, scale, shift, res, n_sl, N, Ho, Wo):
    """-> (value BEFORE the ReLU, bound, S), each (N,Cout,Ho,Wo) float64: the module docstring's formula"""
    ref = product(A, B)
    K = A.shape[1]
    sc, sh = np.asarray(scale, np.float64)[None, :], np.asarray(shift, np.float64)[None, :]
    a = ref.value * sc
    r = np.zeros_like(a) if res is None else np.asarray(res, np.float64).transpose(0, 2, 3, 1).reshape(a.shape)
    value = a + sh + r
    bound = ((gamma(K + n_sl) + U) * ref.S * np.abs(sc) + 3 * U * (np.abs(value) + np.abs(a) + np.abs(sh) + np.abs(r))
             + (K + n_sl) * FTZ * np.maximum(np.abs(sc), 1.0) * (ref.S > 0))
    return _nchw(value, N, Ho, Wo), _nchw(bound, N, Ho, Wo), _nchw(ref.S, N, Ho, Wo)


def maxpool(x):
    """nn.MaxPool2d(3, 2, 1): the padding is -inf, it never wins"""
    x = np.asarray(x)
    N, C, H, W = x.shape
    Ho, Wo = out_size(H, 3, 2, 1), out_size(W, 3, 2, 1)
    xp = np.full((N, C, H + 4, W + 4), -np.inf, x.dtype)
    xp[:, :, 1:1 + H, 1:1 + W] = x
    out = np.full((N, C, Ho, Wo), -np.inf, x.dtype)
    for ky in range(3):
        for kx in range(3):
            out = np.maximum(out, xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][:, :, :Ho, :Wo])
    return out


def level_shape(H, W, level, use_first_pool):
    """(h, w) of pyramid level `level`: stem 7x7/2 pad 3; the pool (3x3/2 pad 1) in front of stage 1; stages 2.. halve (3x3/2 pad 1)"""
    h, w = out_size(H, 7, 2, 3), out_size(W, 7, 2, 3)
    if level >= 1 and use_first_pool:
        h, w = out_size(h, 3, 2, 1), out_size(w, 3, 2, 1)
    for _ in range(2, level + 1):
        h, w = out_size(h, 3, 2, 1), out_size(w, 3, 2, 1)
    return h, w


def trunk_levels(module, images, dtype=torch.float64):
    """the module's `_stages` (its torch trunk, eval mode) on the CPU in `dtype`: the pyramid levels as a list of tensors"""
    m = copy.deepcopy(module).cpu().to(dtype).eval()
    m.trunk = "torch"
    with torch.no_grad():
        return m._stages(images.detach().cpu().to(dtype))


def fold_bn(bn):
    """(scale, shift) of an eval-mode batch norm, formed in fp64 and rounded to fp32 once, as the header tells a C caller"""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.double() * scale
    return scale.float(), shift.float()


def randomise_bn(module, seed):
    """gamma and var in [0.5, 1.5], beta and mean ~ 0.1 N(0,1): an affine that matters"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.running_var.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(0.1 * torch.randn(m.weight.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.weight.shape, generator=g))
    return module
