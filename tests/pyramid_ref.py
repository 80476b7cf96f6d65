"""Reference and error bound for the backward of the encoder output formatting (pnr_pyramid_to_latent_backward).

The reference restates the operator: per axis the interpolation matrix of F.interpolate(bilinear, align_corners=True) is
built with the forward's fp32 expressions (src = scale * dst, scale = (in-1)/(out-1) or 0, i0 = min((int)src, in-1),
i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1), its entries rounded to fp32, and applied to the gradient in fp64:
d_stage = My^T . g . Mx per channel.

The bound is the worst case of an n-term fp32 sum of three-factor products (h * w * g), in any order:
|hip - ref| <= (n + 4) * 2^-24 * A elementwise, A = the same product applied to |g|, n = the largest number of non-zero
weights feeding one texel of the stage (product of the per-axis maxima, read off the same matrices).
"""
import numpy as np
import torch

U = 2.0 ** -24


def axis_matrix(n_in, n_out):
    """(n_out, n_in) float64 array holding the fp32 weights the forward applies along one axis"""
    f = np.float32
    scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0.0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (f(1.0) - l1).astype(np.float32)
    m = np.zeros((n_out, n_in), dtype=np.float32)
    rows = np.arange(n_out)
    np.add.at(m, (rows, i0), l0)  # i0 == i1 (last source index): the entry is fl32(l0 + l1)
    np.add.at(m, (rows, i1), l1)
    return m.astype(np.float64)


def reference(g_nchw, shapes):
    """g_nchw (NV, sum C, H0, W0) tensor, shapes [(C,H,W)] -> ([d_stage float64 (NV,C,H,W)], [bound float64])"""
    g = g_nchw.detach().cpu().double()
    H0, W0 = shapes[0][1:]
    refs, bounds = [], []
    c = 0
    for C, H, W in shapes:
        my, mx = axis_matrix(H, H0), axis_matrix(W, W0)
        n = int((my != 0).sum(0).max()) * int((mx != 0).sum(0).max())
        ty, tx = torch.from_numpy(my), torch.from_numpy(mx)
        gs = g[:, c:c + C]
        refs.append(torch.einsum("yi,ncyx,xj->ncij", ty, gs, tx))
        a = torch.einsum("yi,ncyx,xj->ncij", ty.abs(), gs.abs(), tx.abs())
        bounds.append((n + 4) * U * a)
        c += C
    return refs, bounds


def torch_backward(g_nchw, shapes, device="cpu"):
    """torch's own fp32 autograd of interpolate + cat (the reference's operator) -> [d_stage fp32]"""
    import torch.nn.functional as F
    NV = g_nchw.shape[0]
    levels = [torch.zeros((NV, C, H, W), dtype=torch.float32, device=device, requires_grad=True) for C, H, W in shapes]
    size = levels[0].shape[-2:]
    lat = torch.cat([F.interpolate(t, size, mode="bilinear", align_corners=True) for t in levels], dim=1)
    lat.backward(g_nchw.to(device))
    return [t.grad for t in levels]


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf)"""
    err = (got.detach().cpu().double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())
