"""Test helper (not a test): what composite_bwd_kernel (pnr_bwd.hip, ops.composite_backward) computes, restated in plain fp32
torch with sequential sums and products in place of the wave scans -- plus the seeded inputs, the fp64 / fp32 autograd yardsticks
and the bar that tests/test_composite_bwd_host.py and tests/test_hip_stage_sweep_backward.py share.

    delta_i = z_{i+1} - z_i (last: far - z_i),  ex_i = exp(-delta_i relu(sigma_i)),  a_i = 1 - ex_i,  tf_i = 1 - a_i + 1e-10
    T_i = prod_{j<i} tf_j,  w_i = a_i T_i
    g_i = dL/dw_i = d_rgb . c_i + d_depth z_i + d_w_i - [white] sum(d_rgb)
    S_i = g_{i+1} a_{i+1} + tf_{i+1} S_{i+1}  (S_{K-1} = 0):  the suffix sum_{j>i} g_j w_j / (T_i tf_i), summed directly
    dL/da_i = T_i (g_i - S_i)
    dL/dsigma_i = [sigma_i > 0] dL/da_i delta_i ex_i,   dL/drgb_i = w_i d_rgb   (pre_activation: times c (1 - c))
    dL/ddelta_i = dL/da_i relu(sigma_i) ex_i,  dL/dz_i = w_i d_depth - dL/ddelta_i + dL/ddelta_{i-1},  dL/dfar = dL/ddelta_{K-1}

`old_form=True` keeps the formula the kernel used before: dL/da_i = g_i T_i - (total - sum_{j<=i} g_j w_j) / tf_i, a full-ray sum
minus an inclusive prefix, divided by tf_i.  On a nearly opaque sample the rounding of that difference is divided by a tiny tf_i and
survives in dL/dz; tests/test_composite_bwd_host.py keeps the case where it misses the bar.
"""
import numpy as np
import torch

from oracle import pnr_oracle as O

# (R, K, near, far): R not a multiple of the 4 waves per block, K on both sides of the 64-lane chunk, several chunks with carry,
# K = 1 (the only delta is far - z), near == far
CASES = [
    (1, 1, 1.2, 4.0),
    (7, 3, 0.1, 5.0),
    (33, 17, 0.8, 1.8),
    (9, 63, 1.2, 4.0),
    (64, 64, 1.2, 4.0),
    (9, 65, 1.2, 4.0),
    (129, 31, 0.5, 50.0),
    (5, 129, 1.2, 4.0),
    (3, 400, 1.2, 4.0),
    (300, 8, 2.0, 2.0),
]
CASE_IDS = [f"R{c[0]}_K{c[1]}" for c in CASES]
FAMILIES = ("hostile", "shell")

BAR_FLOOR, BAR_CAP, BAR_FACTOR = 2e-6, 2e-5, 10.0


def composite_backward_ref(rays, z, rgbsigma, white_bkgd, d_rgb, d_depth=None, d_weights=None, pre_activation=False,
                           old_form=False):
    """fp32 in, fp32 out: (d_rgbsigma (R,K,4), d_z (R,K), d_far (R,)).  rgbsigma holds the values AFTER the output activations
    (sigmoid / relu) also with pre_activation=True, as the kernel receives them."""
    f32 = torch.float32
    rays, z, rgbsigma, d_rgb = (t.to(f32) for t in (rays, z, rgbsigma, d_rgb))
    R, K = z.shape
    far = rays[:, 7]
    c, sigma = rgbsigma[..., :3], rgbsigma[..., 3]
    relu = torch.clamp_min(sigma, 0.0)
    delta = torch.cat([z[:, 1:], far[:, None]], 1) - z
    ex = torch.exp(-delta * relu)
    a = 1.0 - ex
    tf = 1.0 - a + 1e-10
    T = torch.ones((R, K), dtype=f32)
    for i in range(1, K):
        T[:, i] = T[:, i - 1] * tf[:, i - 1]
    w = a * T
    g = (c * d_rgb[:, None, :]).sum(-1)
    if d_depth is not None:
        g = g + d_depth.to(f32)[:, None] * z
    if d_weights is not None:
        g = g + d_weights.to(f32)
    if white_bkgd:
        g = g - d_rgb.sum(-1, keepdim=True)
    if old_form:
        gw = g * w
        pre = torch.zeros((R, K), dtype=f32)
        run = torch.zeros(R, dtype=f32)
        for i in range(K):
            run = run + gw[:, i]
            pre[:, i] = run
        dalpha = g * T - (run[:, None] - pre) / tf
    else:
        S = torch.zeros((R, K), dtype=f32)
        for i in range(K - 2, -1, -1):
            S[:, i] = g[:, i + 1] * a[:, i + 1] + tf[:, i + 1] * S[:, i + 1]
        dalpha = T * (g - S)
    dsigma = torch.where(sigma > 0, dalpha * delta * ex, torch.zeros_like(dalpha))
    drgb = w[..., None] * d_rgb[:, None, :]
    if pre_activation:
        drgb = drgb * (c * (1.0 - c))
    ddelta = dalpha * relu * ex
    dz = -ddelta
    dz[:, 1:] += ddelta[:, :-1]
    if d_depth is not None:
        dz = w * d_depth.to(f32)[:, None] + dz
    return torch.cat([drgb, dsigma[..., None]], -1), dz, ddelta[:, -1].clone()


def rand_rays(rs, R, near, far):
    o = rs.uniform(-2, 2, (R, 3))
    d = rs.randn(R, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    nf = np.stack([np.full(R, near), np.full(R, far)], 1)
    return torch.from_numpy(np.concatenate([o, d, nf], 1).astype(np.float32))


def hostile_sigma(rs, R, K):
    """the forward sweep's densities: lognormal(0, 3), 30 % zeros, 10 % negated, ray 1 transparent, ray 2 opaque"""
    sig = rs.lognormal(0.0, 3.0, (R, K)).astype(np.float32)
    sig[rs.uniform(size=sig.shape) < 0.3] = 0.0
    sig[rs.uniform(size=sig.shape) < 0.1] *= -1.0
    if R > 2:
        sig[1] = 0.0
        sig[2] = 1e6
    return sig


def make_inputs(case, family, pre_activation=False):
    """Seeded fp32 inputs of one case, drawn as tests/test_hip_stage_sweep.py draws its own (RandomState(R * 1000 + K): rays, u1,
    colours, densities), then the upstream gradients.  pre_activation: `raw` holds the network outputs in front of sigmoid / relu
    (rgb ~ N(0, 2^2), hostile sigma) and `rgbsigma` their activations in fp32."""
    R, K, near, far = case
    rs = np.random.RandomState(R * 1000 + K)
    rays = rand_rays(rs, R, near, far)
    u1 = torch.from_numpy(rs.uniform(0, 1, (R, K)).astype(np.float32))
    z = O.sample_coarse(rays, u1, K, False)
    rgbs = torch.from_numpy(rs.uniform(-0.5, 1.5, (R, K, 4)).astype(np.float32))
    sig = hostile_sigma(rs, R, K)
    if family == "shell":  # three consecutive samples of sigma 50..300 at a random place, nothing elsewhere
        n = min(3, K)
        start = rs.randint(0, K - n + 1, size=R)
        shell = rs.uniform(50.0, 300.0, (R, n)).astype(np.float32)
        sig = np.zeros((R, K), dtype=np.float32)
        for r in range(R):
            sig[r, start[r]:start[r] + n] = shell[r]
    elif family == "haze":  # one absorbing sample per 64-sample chunk, alpha ~ 0.05 each: the transmittance steps down chunk by chunk
        sig = np.zeros((R, K), dtype=np.float32)
        n = len(range(32, K, 64))
        sig[:, 32::64] = (rs.uniform(0.5, 1.5, (R, n)) * 0.05 * K / max(far - near, 1e-3)).astype(np.float32)
    elif family != "hostile":
        raise ValueError(family)
    rgbs[..., 3] = torch.from_numpy(sig)
    raw = None
    if pre_activation:
        raw = rgbs.clone()
        raw[..., :3] = torch.from_numpy((2.0 * rs.randn(R, K, 3)).astype(np.float32))
        rgbs = torch.cat([torch.sigmoid(raw[..., :3]), torch.relu(raw[..., 3:])], -1)
    gen = torch.Generator().manual_seed(9)  # as test_composite_backward_matches_autograd seeds its own
    d_rgb, d_depth, d_w = torch.randn((R, 3), generator=gen), torch.randn((R,), generator=gen), torch.randn((R, K), generator=gen)
    return {"rays": rays, "z": z, "rgbsigma": rgbs, "raw": raw, "d_rgb": d_rgb, "d_depth": d_depth, "d_w": d_w}


def autograd_ref(inp, white_bkgd, dtype, pre_activation=False):
    """torch autograd through O.composite_from_rgbsigma at `dtype` (fp64: the reference; fp32: the yardstick of the bar).
    -> (d_rgbsigma, d_z, d_far); pre_activation: d_rgbsigma is with respect to `raw`, through sigmoid / relu at `dtype`."""
    rays = inp["rays"].detach().clone().to(dtype).requires_grad_(True)
    z = inp["z"].detach().clone().to(dtype).requires_grad_(True)
    if pre_activation:
        leaf = inp["raw"].detach().clone().to(dtype).requires_grad_(True)
        out = torch.cat([torch.sigmoid(leaf[..., :3]), torch.relu(leaf[..., 3:])], -1)
    else:
        leaf = inp["rgbsigma"].detach().clone().to(dtype).requires_grad_(True)
        out = leaf
    w, rgb, depth = O.composite_from_rgbsigma(rays, z, out, white_bkgd)
    loss = (rgb * inp["d_rgb"].to(dtype)).sum() + (depth * inp["d_depth"].to(dtype)).sum() + (w * inp["d_w"].to(dtype)).sum()
    d_out, d_z, d_rays = torch.autograd.grad(loss, (leaf, z, rays))
    return d_out, d_z, d_rays[:, 7].clone()


def errors(got, ref64):
    """per output tensor max|got - ref| / max|ref|; d_far over max(max|d_far ref|, max|d_z ref|): it is the last sample's delta
    gradient, ~1e-40 on opaque rays, where a purely relative figure means nothing"""
    den = [float(r.abs().max()) for r in ref64]
    den[2] = max(den[2], den[1])
    return [float((g.double() - r).abs().max()) / d if d > 0 else float((g.double() - r).abs().max())
            for g, r, d in zip(got, ref64, den)]


def bar_from(err32):
    """10 x the error of torch's fp32 autograd on the same inputs, floor 2e-6, cap 2e-5 (the stage's bar in test_hip_backward.py)"""
    return min(max(BAR_FACTOR * err32, BAR_FLOOR), BAR_CAP)


# ------------------------------------------------------------------------------------------------ sampling maps
# (shared by tests/test_hip_stage_sweep_backward.py and tests/position_ref.py)
def coarse_map_ref(rays, u1, dz, K, lindisp, dtype):
    r = rays.detach().clone().to(dtype).requires_grad_(True)
    z = O.sample_coarse(r, u1.to(dtype), K, lindisp)
    (d_rays,) = torch.autograd.grad((z * dz.to(dtype)).sum(), r)
    return z.detach(), d_rays


def fine_map_ref(rays, u1, weights, u2, u3, n4, depth_c, dz, Kc, Kfd, lindisp, dtype, perm=None):
    """the merged fine set (nerf.py:285-295) at `dtype` and d(sum dz z_all)/d rays; depth_c is a constant here: the depth samples
    reach near / far only where clamped, the semantics of _SampleFineFunction"""
    r = rays.detach().clone().to(dtype).requires_grad_(True)
    parts = [O.sample_coarse(r, u1.to(dtype), Kc, lindisp), O.sample_fine(r, weights.to(dtype), u2.to(dtype), u3.to(dtype), Kc, lindisp)]
    if Kfd:
        parts.append(O.sample_fine_depth(r, depth_c.to(dtype), n4.to(dtype), 0.01))
    z_cat = torch.cat(parts, -1)
    if perm is None:
        perm = torch.argsort(z_cat.detach(), dim=-1, stable=True)
    z_all = torch.gather(z_cat, 1, perm)
    (d_rays,) = torch.autograd.grad((z_all * dz.to(dtype)).sum(), r)
    return z_all.detach(), perm, d_rays
