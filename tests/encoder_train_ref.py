"""
fp64 restatements of the training entries of the encoder trunk (pixel-nerf_amd/csrc/pnr_conv_bwd.hip) and the DERIVED bounds the
GPU tests hold them to, in the manner of tests/encoder_ref.py, whose families, gamma, U and FTZ it uses.  A helper, not a test:
tests/test_encoder_train_ref_host.py proves what is claimed here against torch's fp64 CPU autograd (no GPU),
tests/test_hip_encoder_train.py holds the kernels to it, profiles/encoder_notes.md has the measured figures.

BATCH NORM.   mean = sum v / M, var = sum (v - mean)^2 / M over the M = N H W values of a channel; invstd = 1 / sqrt(var + eps);
xhat = (v - mean) invstd; y = act(xhat gamma + beta + res); running <- (1 - m) running + m (mean | var M / (M - 1)).
Backward: g = g_y [y > 0]; d_beta = sum g; d_gamma = sum g xhat; d_v = gamma invstd (g - mean(g) - xhat mean(g xhat));
frozen (running statistics): d_v = gamma invstd g.
CONVOLUTION.  d_x[n,ci,iy,ix] = sum_{co,ky,kx} d_y[n,co,oy,ox] w[co,ci,ky,kx] over oy s - p + ky = iy, ox s - p + kx = ix;
d_w[co,ci,ky,kx] = sum_{n,oy,ox} d_y[n,co,oy,ox] x[n,ci, oy s - p + ky, ox s - p + kx].
MAX POOL.     d_x[pixel] = sum of g over the windows whose FIRST maximum in (ky, kx) scan order the pixel is.

BOUND of a convolution gradient, per element, with S = sum |d_y| |other operand|, R the reduction length and n_sl the partial sums
that meet (pnr_conv2d_affine_slices(Cout, k) for the data gradient, pnr_conv2d_backward_weight_slices(P) for the weight gradient):

    bound = (gamma(R + n_sl) + U) S + R FTZ

(encoder_ref.layer_bound without an epilogue: R products and n_sl partial sums in any order, each addition one rounding; the
product's own rounding; a flushed subnormal per term.)  The pool backward adds at most 4 terms: 3 additions, 3 U sum |g|.
Nothing here is fitted to a kernel.
"""
import copy

import numpy as np
import torch

from encoder_ref import FTZ, U, gamma, im2col, out_size, randomise_bn  # noqa: F401


# ------------------------------------------------------------------------------------------------ batch norm
def bn_forward(v, gamma_, beta, running_mean, running_var, eps=1e-5, momentum=0.1, frozen=False, res=None, relu=False, mut=None):
    """-> dict(y, mean, invstd, running_mean, running_var) in float64.  mut "unbiased": the variances swapped (the unbiased one
    normalises, the biased one goes to running_var)."""
    v = np.asarray(v, np.float64)
    N, C, H, W = v.shape
    M = N * H * W
    rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    if frozen:
        mean, var = rm, rv
    else:
        mean = v.mean(axis=(0, 2, 3))
        var = ((v - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
        biased, unbiased = var, var * M / (M - 1)
        if mut == "unbiased":
            biased, unbiased = unbiased, biased
        var = biased
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * unbiased
    invstd = 1.0 / np.sqrt(var + eps)
    b = lambda a: np.asarray(a, np.float64)[None, :, None, None]
    y = (v - b(mean)) * b(invstd) * b(gamma_) + b(beta)
    if res is not None:
        y = y + np.asarray(res, np.float64)
    if relu:
        y = np.maximum(y, 0.0)
    return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv)


def bn_backward(g_y, y, v, mean, invstd, gamma_, frozen=False, mut=None):
    """-> dict(d_v, d_gamma, d_beta, g); y None: no ReLU.  mut "no_mean_terms": the batch form without its two mean terms."""
    g = np.asarray(g_y, np.float64)
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.0)
    v = np.asarray(v, np.float64)
    b = lambda a: np.asarray(a, np.float64)[None, :, None, None]
    xhat = (v - b(mean)) * b(invstd)
    d_beta, d_gamma = g.sum(axis=(0, 2, 3)), (g * xhat).sum(axis=(0, 2, 3))
    M = v.shape[0] * v.shape[2] * v.shape[3]
    if frozen or mut == "no_mean_terms":
        d_v = b(gamma_) * b(invstd) * g
    else:
        d_v = b(gamma_) * b(invstd) * (g - b(d_beta / M) - xhat * b(d_gamma / M))
    return dict(d_v=d_v, d_gamma=d_gamma, d_beta=d_beta, g=g)


# ------------------------------------------------------------------------------------------------ convolution gradients
def conv_backward_data(d_y, w, x_shape, k, s, p, mut=None):
    """-> d_x (N,Cin,H,W) float64.  mut: "flip" (kernel flipped), "transpose" (channels of w transposed; Cin == Cout),
    "phase" (the strided walk starts one input pixel late along x)."""
    d_y, w = np.asarray(d_y, np.float64), np.asarray(w, np.float64)
    N, Cin, H, W = x_shape
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    if mut == "flip":
        w = w[:, :, ::-1, ::-1]
    if mut == "transpose":
        w = w.transpose(1, 0, 2, 3)
    off = 1 if mut == "phase" else 0
    xp = np.zeros((N, Cin, H + 2 * p + s + 1, W + 2 * p + s + 1))
    for ky in range(k):
        for kx in range(k):
            xp[:, :, ky:ky + s * Ho:s, kx + off:kx + off + s * Wo:s][:, :, :Ho, :Wo] += np.einsum("nohw,oc->nchw", d_y, w[:, :, ky, kx])
    return xp[:, :, p:p + H, p:p + W]


def conv_backward_weight(d_y, x, k, s, p, mut=None):
    """-> d_w (Cout,Cin,k,k) float64.  mut: "flip", "transpose" (Cin == Cout), "phase" (x sampled one pixel late along x)."""
    d_y, x = np.asarray(d_y, np.float64), np.asarray(x, np.float64)
    if mut == "phase":
        xs = np.zeros_like(x); xs[:, :, :, :-1] = x[:, :, :, 1:]; x = xs
    cols = im2col(x, k, s, p)                                         # (P, Cin k k)
    flat = d_y.transpose(0, 2, 3, 1).reshape(-1, d_y.shape[1])        # (P, Cout)
    d_w = (flat.T @ cols).reshape(d_y.shape[1], x.shape[1], k, k)
    if mut == "flip":
        d_w = d_w[:, :, ::-1, ::-1]
    if mut == "transpose":
        d_w = d_w.transpose(1, 0, 2, 3)
    return np.ascontiguousarray(d_w)


def grad_bound(S, R, n_sl):
    """the module docstring's bound of a convolution gradient from S = the same gradient of the operands' magnitudes"""
    return (gamma(R + n_sl) + U) * S + R * FTZ


# ------------------------------------------------------------------------------------------------ max pool
def maxpool_backward(x, g, mut=None):
    """nn.MaxPool2d(3, 2, 1) backward in the dtype of g: the gradient of a window goes to its FIRST maximum in (ky, kx) scan
    order (mut "last": to its last); the windows are added in ascending (oy, ox)"""
    x, g = np.asarray(x), np.asarray(g)
    N, C, H, W = x.shape
    Ho, Wo = out_size(H, 3, 2, 1), out_size(W, 3, 2, 1)
    xp = np.full((N, C, H + 4, W + 4), -np.inf, x.dtype)
    xp[:, :, 1:1 + H, 1:1 + W] = x
    win = np.stack([xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][:, :, :Ho, :Wo] for ky in range(3) for kx in range(3)], axis=-1)
    arg = 8 - np.argmax(win[..., ::-1], axis=-1) if mut == "last" else np.argmax(win, axis=-1)
    oy, ox = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    iy, ix = 2 * oy - 1 + arg // 3, 2 * ox - 1 + arg % 3              # (N,C,Ho,Wo) positions in the image
    plane = np.arange(N * C).reshape(N, C, 1, 1)
    d_x = np.zeros(N * C * H * W, g.dtype)
    np.add.at(d_x, ((plane * H + iy) * W + ix).reshape(-1), g.reshape(-1))
    return d_x.reshape(N, C, H, W)


# ------------------------------------------------------------------------------------------------ the whole trunk
# (backbone, num_layers, use_first_pool, image shape, frozen): every batch norm sees M >= 8 values (with M = 2 the gradient is
# ill-conditioned: torch-fp32 is itself off by 1e-2 relative there and such a shape tests nothing)
TRUNK_CASES = [
    ("resnet18", 4, True, (2, 3, 32, 40), False),
    ("resnet18", 4, True, (3, 3, 37, 50), False),
    ("resnet18", 4, False, (2, 3, 32, 40), False),
    ("resnet34", 4, True, (2, 3, 24, 32), False),
    ("resnet34", 5, True, (2, 3, 40, 48), False),
    ("resnet18", 4, True, (2, 3, 32, 40), True),
]
TRUNK_IDS = [f"{b}_L{n}_pool{int(p)}_{'x'.join(map(str, s))}{'_frozen' if f else ''}" for b, n, p, s, f in TRUNK_CASES]
TRUNK_SEED = 0


def make_encoder(backbone, num_layers, use_first_pool, seed=TRUNK_SEED):
    from pixelnerf_amd.model.encoder import SpatialEncoder
    torch.manual_seed(seed)
    enc = SpatialEncoder(backbone, pretrained=False, num_layers=num_layers, use_first_pool=use_first_pool)
    return randomise_bn(enc, seed + 1)


def trunk_image(shape, seed=TRUNK_SEED):
    return torch.rand(shape, generator=torch.Generator().manual_seed(11 + seed)) * 2 - 1


def level_cotangents(levels, seed=TRUNK_SEED):
    """fixed random G_i of the loss sum_i <level_i, G_i>"""
    g = torch.Generator().manual_seed(100 + seed)
    return [torch.randn(tuple(t.shape), generator=g) for t in levels]


def trunk_autograd(module, image, frozen, dtype=torch.float64, cotangents=None):
    """the module's torch trunk on the CPU in `dtype`, training mode (frozen: eval mode, grad enabled), loss sum <level, G>
    -> (levels, grads {name: tensor} with "image" and every conv / BN parameter of the layers that ran, buffers {name: tensor}
    after the forward, cotangents)"""
    m = copy.deepcopy(module).cpu().to(dtype)
    m.trunk = "torch"
    m.train(not frozen)
    x = image.detach().cpu().to(dtype).requires_grad_(True)
    levels = m._stages(x)
    G = cotangents if cotangents is not None else level_cotangents(levels)
    sum((t * g.to(dtype)).sum() for t, g in zip(levels, G)).backward()
    grads = {"image": x.grad}
    for name, p in m.model.named_parameters():
        if p.grad is not None:
            grads[name] = p.grad
    buffers = {name: b.detach().clone() for name, b in m.model.named_buffers()}
    return [t.detach() for t in levels], grads, buffers, G


def rel_err(a, ref):
    """max |a - ref| / max |ref| of one tensor"""
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))
