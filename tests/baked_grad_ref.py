"""Test helper (not a test): the baked-volume ray march (include/pixelnerf_hip.h, "baked volumes") restated in plain torch at any
dtype, DIFFERENTIABLE with respect to the stored values, and the cases, error and bar that tests/test_baked_backward_host.py and
tests/test_hip_baked_backward.py share.  No GPU, no package import.

march() covers the RGBA and the spherical-harmonic form, the `occupied` mask of a skip grid, `terminate` and the white background,
for all rays at once (padded to the longest).  Its forward is baked_ref.render_ref / baked_sh_ref.render_ref (the host test holds
it to them in fp64); its gradients are torch autograd's.  The inputs proper -- rays, stored, c1, c2, step -- are rounded to fp32
first and then carried in `dtype`, as there.

Error and bar are those of tests/position_ref.py: error = max|got - ref64| / max|ref64|, bar = 10 x the error of torch's fp32
autograd through the same restatement on the same inputs, floor 2e-6, cap 2e-4.
"""
import collections
import functools

import numpy as np
import torch

import baked_ref as B
import baked_sh_ref as S
import position_ref as P
import sparse_baked_ref as SP

error, bar_from, BAR_CAP = P.error, P.bar_from, P.BAR_CAP
RESO, C1, C2 = B.RESO, B.C1, B.C2
MAX_SAMPLES = B.MAX_SAMPLES


def _fp32(x, dtype):
    """x rounded to fp32, then carried in `dtype`; always a fresh tensor"""
    return torch.tensor(np.array(x, np.float32)).to(dtype)


def sh_basis(d, degree, dtype):
    """baked_sh_ref.sh_basis in torch: d (R,3) at `dtype` -> (R,B); the constants are rounded to fp32 once"""
    c1, c2, c20, c22 = (float(np.float32(v)) for v in (np.sqrt(3.0), np.sqrt(15.0), np.sqrt(5.0) / 2.0, np.sqrt(15.0) / 2.0))
    n2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    s = n2.sqrt()
    x, y, z = d[:, 0] / s, d[:, 1] / s, d[:, 2] / s
    cols = [torch.ones_like(x), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c20 * (3.0 * (z * z) - 1.0), c2 * (x * z),
            c22 * (x * x - y * y)]
    Y = torch.stack(cols[:(degree + 1) ** 2], dim=1)
    bad = ~(torch.isfinite(n2) & (n2 != 0))
    Y[:, 1:] = torch.where(bad[:, None], torch.zeros_like(Y[:, 1:]), Y[:, 1:])
    return Y


def march(rays, stored, c1, c2, step, degree=None, white_bkgd=False, occupied=None, terminate=0.0, dtype=torch.float64, info=None):
    """rays (R,8) array; stored a torch tensor at `dtype` holding fp32-representable values, (nx,ny,nz,4) (degree None) or
    (nx,ny,nz,B,4) (degree 0, 1, 2), through which autograd runs; occupied None or (nx-1,ny-1,nz-1) bool; terminate eps in [0,1).
    -> rgb (R,3), depth (R,), alpha (R,) at `dtype`.
    info: a dict that receives `boundaries` -- per ray the transmittance after every full chunk of 64 samples the march walked --,
    `face_margin` -- the smallest distance of a sample of any ray to a face of the box, in units of the box edge -- and `n`."""
    rays = _fp32(rays, dtype)
    c1t, c2t = _fp32(c1, dtype), _fp32(c2, dtype)
    reso = tuple(stored.shape[:3])
    h = torch.as_tensor(B.cell_size(c1, c2, reso, np.float64)).to(dtype)
    stepv, eps = float(np.float32(step)), float(np.float32(terminate))
    R = rays.shape[0]
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    ok = torch.isfinite(rays).all(dim=1) & (near < far)
    count = torch.ceil((far - near) / torch.tensor(stepv, dtype=dtype))
    n = torch.where(ok & (count <= MAX_SAMPLES), count, torch.zeros_like(count)).long()
    nmax = int(n.max()) if R else 0
    i = torch.arange(nmax, dtype=dtype)
    exists = torch.arange(nmax)[None, :] < n[:, None]                                  # (R,nmax)
    t = near[:, None] + (i[None, :] + 0.5) * stepv
    p = o[:, None, :] + t[:, :, None] * d[:, None, :]                                  # (R,nmax,3)
    inside = ((p >= c1t) & (p <= c2t)).all(dim=2)
    u = (p - c1t) / h
    top = torch.tensor([r - 2 for r in reso], dtype=dtype)
    cell = torch.minimum(torch.maximum(torch.floor(u), torch.zeros_like(u)), top.expand_as(u))
    cell = torch.where(torch.isnan(cell), torch.zeros_like(cell), cell)
    f = torch.clamp(u - cell, 0.0, 1.0)
    f = torch.where(torch.isnan(f), torch.zeros_like(f), f)
    idx = cell.long()
    active = exists & inside
    if occupied is not None:
        active = active & torch.as_tensor(np.asarray(occupied, bool))[idx[..., 0], idx[..., 1], idx[..., 2]]
    if info is not None:
        gap = torch.minimum((p - c1t).abs(), (p - c2t).abs()) / (c2t - c1t)
        info["face_margin"] = float(gap[exists].min()) if bool(exists.any()) else float("inf")
        info["n"] = n.tolist()

    # the eight corner values of every sample: (R,nmax,2,2,2,4)
    Y = sh_basis(d, degree, dtype) if degree is not None else None
    corners = []
    for ix in (0, 1):
        for iy in (0, 1):
            for iz in (0, 1):
                v = stored[idx[..., 0] + ix, idx[..., 1] + iy, idx[..., 2] + iz]       # (R,nmax,4) or (R,nmax,B,4)
                if degree is not None:
                    acc = v[:, :, 0, :] * Y[:, None, 0, None]
                    for k in range(1, Y.shape[1]):
                        acc = acc + v[:, :, k, :] * Y[:, None, k, None]
                    v = torch.cat((torch.clamp(acc[..., :3], 0.0, 1.0), torch.clamp(acc[..., 3:], min=0.0)), dim=-1)
                corners.append(v)
    v = torch.stack(corners, dim=2).reshape(R, nmax, 2, 2, 2, 4)
    fx, fy, fz = f[..., 0, None], f[..., 1, None], f[..., 2, None]
    vz = v[:, :, :, :, 0] + fz[:, :, None, None] * (v[:, :, :, :, 1] - v[:, :, :, :, 0])   # along z, then y, then x
    vy = vz[:, :, :, 0] + fy[:, :, None] * (vz[:, :, :, 1] - vz[:, :, :, 0])
    val = vy[:, :, 0] + fx * (vy[:, :, 1] - vy[:, :, 0])
    val = torch.where(active[..., None], val, torch.zeros_like(val))

    a = 1.0 - torch.exp(-(stepv * val[..., 3]))
    tfac = torch.where(exists, 1.0 - a + torch.tensor(1e-10, dtype=dtype), torch.ones_like(a))
    incl = torch.cumprod(tfac, dim=1)
    T = torch.cat((torch.ones((R, 1), dtype=dtype), incl[:, :-1]), dim=1) if nmax else incl
    walked = exists
    full = incl[:, 63::64].detach()                                                    # T after every full chunk
    if eps > 0 and full.shape[1]:
        chunk_exists = (64 * (torch.arange(full.shape[1]) + 1))[None, :] <= n[:, None]
        stop = (full <= eps) & chunk_exists
        first = torch.where(stop.any(dim=1), stop.float().argmax(dim=1), torch.full((R,), full.shape[1]))
        walked = exists & (torch.arange(nmax)[None, :] < 64 * (first[:, None] + 1))
    if info is not None:
        bounds = []
        for r in range(R):
            k = int(walked[r].sum()) // 64
            bounds.append(full[r, :k].tolist())
        info["boundaries"] = bounds
    w = torch.where(walked, a * T, torch.zeros_like(a))
    rgb = (w[..., None] * val[..., :3]).sum(dim=1)
    depth = (w * t).sum(dim=1)
    alpha = w.sum(dim=1)
    if white_bkgd:
        rgb = rgb + 1.0 - alpha[:, None]
    return rgb, depth, alpha


def gradient(rays, stored, c1, c2, step, d_rgb=None, d_depth=None, d_alpha=None, dtype=torch.float64, **kw):
    """dL/d stored at `dtype` for L = sum rgb . d_rgb + sum depth d_depth + sum alpha d_alpha (each None: absent), by autograd"""
    leaf = _fp32(stored, dtype).requires_grad_(True)
    rgb, depth, alpha = march(rays, leaf, c1, c2, step, dtype=dtype, **kw)
    L = rgb.sum() * 0.0
    if d_rgb is not None:
        L = L + (rgb * _fp32(d_rgb, dtype)).sum()
    if d_depth is not None:
        L = L + (depth * _fp32(d_depth, dtype)).sum()
    if d_alpha is not None:
        L = L + (alpha * _fp32(d_alpha, dtype)).sum()
    (g,) = torch.autograd.grad(L, leaf, allow_unused=True)
    return torch.zeros_like(leaf) if g is None else g


# ---------------------------------------------------------------- the cases of tests/test_hip_baked_backward.py (checked on the host too)
# (near = 1.2 for the rays that start outside; far = near + (n - 0.5) step: n samples, fp32 and fp64 agree on the ceil)
SETTINGS = {"n40": (40, 0.1), "n64": (64, 0.05), "n150": (150, 0.03), "n4500": (4500, 0.0005)}
NEAR = 1.2


def case_rays(setting, which=None):
    """baked_ref.common_rays (26 hits, 4 misses, 2 origins inside, 3 axis-parallel, 1 in a cell plane, 1 with near >= far) with the
    near / far of `setting`; which: a list of rows to keep"""
    n, step = SETTINGS[setting]
    rays = B.common_rays("n133").copy()
    span = np.float32((n - 0.5) * step)
    outside = rays[:, 6] == np.float32(B.SETTINGS["n133"][0])
    inside = rays[:, 6] == 0
    rays[outside, 6], rays[outside, 7] = np.float32(NEAR), np.float32(NEAR) + span
    rays[inside, 7] = span
    assert int(outside.sum()) + int(inside.sum()) == 36 and rays[36, 6] > rays[36, 7]
    return rays if which is None else np.ascontiguousarray(rays[list(which)])


MISSING = (26, 27, 28, 29, 36)   # the rows of case_rays that give exact zeros: four miss the box, one has near >= far


def rgba_volume(sigma_scale=1.0, opaque=False):
    """baked_ref.common_volume with sigma scaled; opaque: sigma = 1e4 at the 2x2x2 points [4:6, 3:5, 3:5] in the middle of the box --
    a sample that blends any of them with weight >= 0.06 has alpha = 1 in fp32 at step 0.03"""
    vol = B.common_volume().copy()
    vol[..., 3] = vol[..., 3] * np.float32(sigma_scale)
    if opaque:
        vol[4:6, 3:5, 3:5, 3] = np.float32(1e4)
    return vol


SH_MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def sh_coef(degree, setting="n150"):
    """baked_sh_ref.common_coef(degree) with the DC part moved so that every channel is clamped on both sides at some corners for
    some rays at EVERY degree (rgb DC 1.4 c - 0.2 in [-0.2, 1.2]; sigma DC s - 3 where s > 0), then nudged, point by point, until
    no unclamped corner value of any ray of case_rays(setting) lies within SH_MARGIN of a clamp edge -- except the points whose
    sigma coefficients are all exactly zero (the empty layers): those sit ON the edge in every precision, where the clamp's
    derivative is 1 by torch.clamp's convention and by the kernel's.  Treat as read-only."""
    coef = S.common_coef(degree).copy()
    coef[..., 0, :3] = coef[..., 0, :3] * np.float32(1.4) - np.float32(0.2)
    live = coef[..., 0, 3] > 0
    coef[..., 0, 3] = np.where(live, coef[..., 0, 3] - np.float32(3.0), np.float32(0.0))
    Y = S.sh_basis(case_rays(setting)[:, 3:6], degree, np.float64)                     # (R,B)
    for _ in range(64):
        v = np.einsum("xyzbc,rb->rxyzc", coef.astype(np.float64), Y)
        close = np.minimum(np.abs(v), np.abs(v - 1.0)) < 2 * SH_MARGIN
        close[..., 3] = (np.abs(v[..., 3]) < 2 * SH_MARGIN) & live[None]
        bad = close.any(axis=0)                                                        # (nx,ny,nz,4)
        if not bad.any():
            break
        coef[..., 0, :] = np.where(bad, coef[..., 0, :] + np.float32(7 * SH_MARGIN), coef[..., 0, :])
    else:
        raise AssertionError("sh_coef: could not clear the clamp edges")
    coef.setflags(write=False)
    return coef


def sh_clamp_census(coef, rays, degree):
    """-> (the smallest distance of an unclamped corner value to a clamp edge over all rays, points and channels, the points on
    the edge by construction left out; per channel the number of (ray, point) values below the range; the same above it)"""
    Y = S.sh_basis(rays[:, 3:6], degree, np.float64)
    v = np.einsum("xyzbc,rb->rxyzc", coef.astype(np.float64), Y)
    empty = (coef[..., :, 3] == 0).all(axis=-1)
    gap = np.minimum(np.abs(v), np.abs(v - 1.0))
    gap[..., 3] = np.where(empty[None], np.inf, np.abs(v[..., 3]))
    below = [(v[..., c] < 0).sum() for c in range(4)]
    above = [(v[..., c] > 1).sum() for c in range(3)]
    return float(gap.min()), below, above


# name, setting, kind (None: RGBA; 0, 1, 2: degree), rows of case_rays or None, upstream gradients present (r, d, a), white, the
# threshold of the skip grid (None: no bits), terminate, sigma scale, opaque block
Case = collections.namedtuple("Case", "name setting kind rows up white thr terminate scale opaque")
ALL = (True, True, True)
# rows of case_rays("n4500") that still cross density beyond sample 4096 (sigma scaled by 0.15: T there is 0.1 .. 0.9) and keep
# every sample 1e-5 box edges off the faces
LONG = (11, 14, 22, 32, 33, 34)
# rows of case_rays("n150") whose fp64 transmittance at every boundary of 64 samples is <= eps / 2 or >= 2 eps at eps = 1e-2
# (tests/test_baked_backward_host.py holds them to that): 14 / 13 of them stop early
TERM_RGBA = (0, 1, 2, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36)
TERM_SH2 = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 35, 36)
CASES = [
    Case("rgba_n40", "n40", None, None, ALL, False, None, 0.0, 1.0, False),
    Case("rgba_n64_white", "n64", None, None, ALL, True, None, 0.0, 1.0, False),
    Case("rgba_n150", "n150", None, None, ALL, False, None, 0.0, 1.0, False),
    Case("rgba_n150_rgb_white", "n150", None, None, (True, False, False), True, None, 0.0, 1.0, False),
    Case("rgba_n150_depth", "n150", None, None, (False, True, False), False, None, 0.0, 1.0, False),
    Case("rgba_n150_alpha_white", "n150", None, None, (False, False, True), True, None, 0.0, 1.0, False),
    Case("rgba_n4500_thin", "n4500", None, LONG, ALL, False, None, 0.0, 0.15, False),   # 71 chunks: 7 beyond the heads in lanes
    Case("rgba_n150_opaque", "n150", None, None, ALL, False, None, 0.0, 0.05, True),
    Case("rgba_n150_bits0", "n150", None, None, ALL, True, 0.0, 0.0, 1.0, False),
    Case("rgba_n150_bits10", "n150", None, None, ALL, False, 10.0, 0.0, 1.0, False),
    Case("rgba_n150_terminate", "n150", None, TERM_RGBA, ALL, True, None, 1e-2, 1.0, False),
    Case("rgba_n150_bits10_terminate", "n150", None, TERM_RGBA, ALL, False, 10.0, 1e-2, 1.0, False),
    Case("sh0_n150", "n150", 0, None, ALL, False, None, 0.0, 1.0, False),
    Case("sh1_n150_white", "n150", 1, None, ALL, True, None, 0.0, 1.0, False),
    Case("sh2_n150", "n150", 2, None, ALL, False, None, 0.0, 1.0, False),
    Case("sh2_n150_bits10_terminate", "n150", 2, TERM_SH2, ALL, True, 10.0, 1e-2, 1.0, False),
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> dict of the fp32 inputs of one case (numpy; shared: treat as read-only): rays, stored, step, occupied (cells, or None),
    d_rgb / d_depth / d_alpha (None where the case has none), and the keyword arguments march() takes"""
    n, step = SETTINGS[case.setting]
    rays = case_rays(case.setting, case.rows)
    if case.kind is None:
        stored = rgba_volume(case.scale, case.opaque)
        sigma = stored[..., 3]
    else:
        stored = np.array(sh_coef(case.kind, case.setting))
        sigma = S.common_coef(0)[..., 0, 3]   # the skip grid of the case: the cells of the UNMOVED DC sigma (any grid will do)
    occupied = None if case.thr is None else SP.occupied_cells(sigma, case.thr)
    rs = np.random.RandomState(4242 + CASES.index(case))
    R = rays.shape[0]
    d_rgb = rs.standard_normal((R, 3)).astype(np.float32) if case.up[0] else None
    d_depth = rs.standard_normal((R,)).astype(np.float32) if case.up[1] else None
    d_alpha = rs.standard_normal((R,)).astype(np.float32) if case.up[2] else None
    kw = dict(degree=case.kind, white_bkgd=case.white, occupied=occupied, terminate=case.terminate)
    return dict(rays=rays, stored=stored, step=step, occupied=occupied, d_rgb=d_rgb, d_depth=d_depth, d_alpha=d_alpha, kw=kw)


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (inputs, the fp64 gradient, torch's fp32 gradient) of one case, computed once (treat as read-only)"""
    inp = inputs(case)
    args = (inp["rays"], inp["stored"], C1, C2, inp["step"], inp["d_rgb"], inp["d_depth"], inp["d_alpha"])
    return inp, gradient(*args, dtype=torch.float64, **inp["kw"]), gradient(*args, dtype=torch.float32, **inp["kw"])


# ---------------------------------------------------------------- the fitting loop of util.bake.fit, restated on the host
FIT_RESO, FIT_C1, FIT_C2 = (12, 12, 12), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
FIT_STEP, FIT_N = 2.0 / 11.0, 20
FIT = dict(steps=40, lr=2e-2, batch=128, seed=3)
FIT_RAY_SEED = 5   # (every sample of every ray at least 3e-5 box edges off the faces)


@functools.lru_cache(maxsize=None)
def fit_scene(degree):
    """-> (known stored, perturbed start, rays (512,8)) as fp32 arrays (treat as read-only): a smooth blob on a 12^3 grid -- RGBA
    (degree None) or degree-1 coefficients whose DC part is that blob --, a start with sigma scaled by 0.5 .. 1.5 and rgb moved by
    up to 0.2, and 512 rays from four cameras at distance 3 towards points of the inner box, 20 samples one cell apart"""
    rs = np.random.RandomState(11 if degree is None else 12)
    ax = [np.linspace(lo, hi, n) for lo, hi, n in zip(FIT_C1, FIT_C2, FIT_RESO)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    known = np.empty(FIT_RESO + (4,), np.float32)
    known[..., 0] = 0.5 + 0.35 * np.sin(2.0 * X + 0.3)
    known[..., 1] = 0.5 + 0.35 * np.cos(1.7 * Y - 0.2)
    known[..., 2] = 0.5 + 0.35 * np.sin(2.3 * Z + X)
    known[..., 3] = 12.0 * np.exp(-(X * X + 1.4 * Y * Y + 0.8 * Z * Z) / 0.35)
    start = known.copy()
    start[..., :3] = np.clip(known[..., :3] + rs.uniform(-0.2, 0.2, FIT_RESO + (3,)), 0.0, 1.0)
    start[..., 3] = known[..., 3] * rs.uniform(0.5, 1.5, FIT_RESO)
    if degree is not None:
        nb = (degree + 1) ** 2
        def lift(dc, seed):
            r = np.random.RandomState(seed)
            coef = np.zeros(FIT_RESO + (nb, 4), np.float32)
            coef[..., 0, :] = dc
            coef[..., 1:, :3] = r.uniform(-0.1, 0.1, FIT_RESO + (nb - 1, 3))
            coef[..., 1:, 3] = r.uniform(-1.0, 1.0, FIT_RESO + (nb - 1,))
            return coef
        known, start = lift(known, 21), lift(start, 22)
    cams = np.array([(3.0, 0.3, 0.2), (-0.5, 2.8, 1.0), (0.4, -1.0, 2.9), (-2.0, -2.0, -1.0)])
    rows, rs = [], np.random.RandomState(FIT_RAY_SEED)
    for k in range(512):
        cam = cams[k % 4]
        target = rs.uniform(-0.6, 0.6, 3)
        d = (target - cam) / np.linalg.norm(target - cam)
        near = np.linalg.norm(cam) - 1.8
        rows.append(np.concatenate((cam, d, [near, near + (FIT_N - 0.5) * FIT_STEP])))
    out = (np.ascontiguousarray(known, np.float32), np.ascontiguousarray(start, np.float32), np.asarray(rows, np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def fit_ref(degree, dtype, steps, lr, batch, seed):
    """util.bake.fit through the restatement at `dtype` on the CPU: the target is the restatement's render of the known volume, the
    batches are fit's (a CPU torch.Generator with fit's seed and draws), the optimiser torch.optim.Adam with fit's settings, the
    projection of an RGBA volume fit's.  -> the batch losses, floats"""
    known, start, rays = fit_scene(degree)
    with torch.no_grad():
        target = march(rays, _fp32(known, dtype), FIT_C1, FIT_C2, FIT_STEP, degree=degree, dtype=dtype)[0]
    stored = _fp32(start, dtype).requires_grad_(True)
    optimiser = torch.optim.Adam([stored], lr=lr)
    gen = torch.Generator().manual_seed(seed)
    losses = []
    for _ in range(steps):
        ids = torch.randint(0, rays.shape[0], (min(batch, rays.shape[0]),), generator=gen)
        rgb = march(rays[ids.numpy()], stored, FIT_C1, FIT_C2, FIT_STEP, degree=degree, dtype=dtype)[0]
        loss = ((rgb - target[ids]) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        loss.backward()
        optimiser.step()
        if degree is None:
            with torch.no_grad():
                stored[..., :3].clamp_(0.0, 1.0)
                stored[..., 3].clamp_(min=0.0)
        losses.append(float(loss.detach()))
    return losses


# ---------------------------------------------------------------- contention: 2048 copies of one ray
COPIES = 2048


@functools.lru_cache(maxsize=None)
def contention():
    """row 0 of the case rgba_n40, COPIES times over -> (the inputs of the case with the copies in place of its rays, the fp64
    gradient of the single ray, the fp64 and the torch-fp32 gradient of the copies), computed once (treat as read-only)"""
    case = BY_NAME["rgba_n40"]
    inp = inputs(case)
    one = {k: inp[k][:1] for k in ("rays", "d_rgb", "d_depth", "d_alpha")}
    many = {k: np.repeat(v, COPIES, axis=0) for k, v in one.items()}
    grad = lambda d, dtype: gradient(d["rays"], inp["stored"], C1, C2, inp["step"], d["d_rgb"], d["d_depth"], d["d_alpha"], dtype=dtype,
                                     **inp["kw"])
    return dict(inp, **many), grad(one, torch.float64), grad(many, torch.float64), grad(many, torch.float32)
