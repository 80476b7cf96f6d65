"""Test helper (not a test): the visibility of a baked volume (include/pixelnerf_hip.h, "Visibility of a baked volume") restated in
plain torch at any dtype, and the cases that tests/test_baked_visibility_host.py and tests/test_hip_baked_visibility.py share.  No
GPU, no package import.

visibility() walks the samples of baked_grad_ref.march -- the same lines for the sample count, the points, the cells, the fractions,
the blend, alpha and the transmittance, the same stop after a chunk -- and keeps, per grid point, the largest w_i x omega_c; the
host test holds sum_i w_i of this walk to march()'s alpha, so the weights ARE march()'s.  A sparse volume is the dense one with the
cells of its grid as `occupied`, read at the kept ids (every corner of an occupied cell is kept).

Error and bar: those of baked_grad_ref (max|got - ref64| / max|ref64|; 10 x the error of the fp32 restatement, floor 2e-6, cap 2e-4).
"""
import collections
import functools

import numpy as np
import torch

import baked_grad_ref as G
import baked_ref as B
import sparse_baked_ref as SP

error, bar_from = G.error, G.bar_from
RESO, C1, C2 = G.RESO, G.C1, G.C2


def weights(rays, stored, c1, c2, step, degree=None, occupied=None, terminate=0.0, dtype=torch.float64):
    """baked_grad_ref.march's samples: -> dict(w (R,nmax) the compositing weights, 0 where the walk did not go; idx (R,nmax,3) the
    cells; f (R,nmax,3) the fractions; active (R,nmax); walked (R,nmax); n (R,))"""
    rays = G._fp32(rays, dtype)
    stored = stored if isinstance(stored, torch.Tensor) else G._fp32(stored, dtype)
    c1t, c2t = G._fp32(c1, dtype), G._fp32(c2, dtype)
    reso = tuple(stored.shape[:3])
    h = torch.as_tensor(B.cell_size(c1, c2, reso, np.float64)).to(dtype)
    stepv, eps = float(np.float32(step)), float(np.float32(terminate))
    R = rays.shape[0]
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    ok = torch.isfinite(rays).all(dim=1) & (near < far)
    count = torch.ceil((far - near) / torch.tensor(stepv, dtype=dtype))
    n = torch.where(ok & (count <= G.MAX_SAMPLES), count, torch.zeros_like(count)).long()
    nmax = int(n.max()) if R else 0
    i = torch.arange(nmax, dtype=dtype)
    exists = torch.arange(nmax)[None, :] < n[:, None]
    t = near[:, None] + (i[None, :] + 0.5) * stepv
    p = o[:, None, :] + t[:, :, None] * d[:, None, :]
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
    Y = G.sh_basis(d, degree, dtype) if degree is not None else None
    corners = []
    for ix in (0, 1):
        for iy in (0, 1):
            for iz in (0, 1):
                v = stored[idx[..., 0] + ix, idx[..., 1] + iy, idx[..., 2] + iz]
                if degree is not None:
                    acc = v[:, :, 0, :] * Y[:, None, 0, None]
                    for k in range(1, Y.shape[1]):
                        acc = acc + v[:, :, k, :] * Y[:, None, k, None]
                    v = torch.cat((torch.clamp(acc[..., :3], 0.0, 1.0), torch.clamp(acc[..., 3:], min=0.0)), dim=-1)
                corners.append(v[..., 3])
    s = torch.stack(corners, dim=2).reshape(R, nmax, 2, 2, 2)
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    sz = s[..., 0] + fz[:, :, None, None] * (s[..., 1] - s[..., 0])
    sy = sz[..., 0] + fy[:, :, None] * (sz[..., 1] - sz[..., 0])
    sigma = sy[..., 0] + fx * (sy[..., 1] - sy[..., 0])
    sigma = torch.where(active, sigma, torch.zeros_like(sigma))
    a = 1.0 - torch.exp(-(stepv * sigma))
    tfac = torch.where(exists, 1.0 - a + torch.tensor(1e-10, dtype=dtype), torch.ones_like(a))
    incl = torch.cumprod(tfac, dim=1)
    T = torch.cat((torch.ones((R, 1), dtype=dtype), incl[:, :-1]), dim=1) if nmax else incl
    walked = exists
    full = incl[:, 63::64]
    if eps > 0 and full.shape[1]:
        chunk_exists = (64 * (torch.arange(full.shape[1]) + 1))[None, :] <= n[:, None]
        stop = (full <= eps) & chunk_exists
        first = torch.where(stop.any(dim=1), stop.float().argmax(dim=1), torch.full((R,), full.shape[1]))
        walked = exists & (torch.arange(nmax)[None, :] < 64 * (first[:, None] + 1))
    w = torch.where(walked, a * T, torch.zeros_like(a))
    return dict(w=w, idx=idx, f=f, active=active, walked=walked, n=n, full=full)


def visibility(rays, stored, c1, c2, step, degree=None, occupied=None, terminate=0.0, dtype=torch.float64, out=None, info=None):
    """-> vis (nx,ny,nz) at `dtype`: max over the walked active samples i and the corners c of their cells of w_i x omega_c,
    omega_c = ((x part) (y part)) (z part), proposals that are not > 0 dropped; `out`: a field to max-accumulate into.
    info: a dict that receives w_max (the largest weight), touched (nx,ny,nz) bool: a corner of the cell of a walked active sample,
    chunks (R,) the number of 64-sample chunks with a weight > 0, stopped (R,) bool: the walk ended before the last chunk"""
    stored = stored if isinstance(stored, torch.Tensor) else G._fp32(stored, dtype)
    reso = tuple(stored.shape[:3])
    s = weights(rays, stored, c1, c2, step, degree, occupied, terminate, dtype)
    w, idx, f = s["w"], s["idx"], s["f"]
    live = s["active"] & s["walked"]
    vis = torch.zeros(reso, dtype=dtype) if out is None else out
    flat = vis.view(-1)
    touched = torch.zeros(reso, dtype=torch.bool)
    for ix in (0, 1):
        for iy in (0, 1):
            for iz in (0, 1):
                om = ((f[..., 0] if ix else 1.0 - f[..., 0]) * (f[..., 1] if iy else 1.0 - f[..., 1])) * (f[..., 2] if iz else 1.0 - f[..., 2])
                v = w * om
                take = live & (v > 0)
                point = ((idx[..., 0] + ix) * reso[1] + idx[..., 1] + iy) * reso[2] + idx[..., 2] + iz
                flat.scatter_reduce_(0, point[take], v[take], reduce="amax", include_self=True)
                touched.view(-1)[point[live]] = True
    if info is not None:
        R, nmax = w.shape
        pad = (-nmax) % 64
        wp = torch.cat((w, torch.zeros((R, pad), dtype=dtype)), dim=1).view(R, -1, 64) if nmax else w.view(R, 0, 64)
        info["w_max"] = float(w.max()) if w.numel() else 0.0
        info["touched"] = touched
        info["chunks"] = (wp > 0).any(dim=2).sum(dim=1)
        info["stopped"] = (s["walked"].sum(dim=1) < s["n"])
        info["alpha"] = w.sum(dim=1)
        info["n"] = s["n"]
    return vis


# ---------------------------------------------------------------- the cases (checked on the host, run on the GPU)
# The 37 rays of baked_grad_ref.case_rays("n150") and their reflections through the origin (the box is seen from six sides: 74 rays),
# step 0.03.  Without terminate every third ray is cut to 60 samples (fewer than 64) that start where the ray has reached the box;
# the others keep 150 (three chunks: the carry crosses two chunk boundaries).  With terminate every ray keeps 150 samples, and only
# the rays stay whose fp64 transmittance at every chunk boundary is a factor 2 off eps: both precisions stop after the same chunk.
STEP = 0.03
Case = collections.namedtuple("Case", "name kind scale thr terminate")
CASES = [
    Case("rgba", None, 0.15, None, 0.0),
    Case("rgba_bits", None, 0.15, 0.5, 0.0),
    Case("rgba_terminate", None, 1.0, None, 1e-2),
    Case("sh0", 0, 1.0, None, 0.0),
    Case("sh1_bits", 1, 1.0, 10.0, 0.0),
    Case("sh2", 2, 1.0, None, 0.0),
    Case("sh2_bits_terminate", 2, 1.0, 10.0, 1e-2),
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
SPARSE_CASES = ["rgba_bits", "sh1_bits", "sh2_bits_terminate"]


def all_rays():
    base = G.case_rays("n150")
    mirrored = base.copy()
    mirrored[:, :6] = -mirrored[:, :6]
    return np.concatenate((base, mirrored))


def _volume(case):
    if case.kind is None:
        stored = G.rgba_volume(case.scale)
        return stored, stored[..., 3]
    return np.array(G.sh_coef(case.kind, "n150")), G.S.common_coef(0)[..., 0, 3]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> dict (numpy fp32, read-only): rays, stored, occupied (cells or None), kw for visibility()"""
    stored, sigma = _volume(case)
    occupied = None if case.thr is None else SP.occupied_cells(sigma, case.thr)
    rays = all_rays()
    if case.terminate:
        full = weights(rays, stored, C1, C2, STEP, case.kind, occupied, 0.0, torch.float64)["full"]
        clear = ((full <= case.terminate / 2) | (full >= case.terminate * 2)).all(dim=1).numpy()
        rays = np.ascontiguousarray(rays[clear])
    else:
        short = (np.arange(rays.shape[0]) % 3 == 1) & (rays[:, 6] < rays[:, 7])
        rays[short & (rays[:, 6] > 0), 6] += np.float32(0.9)
        rays[short, 7] = rays[short, 6] + np.float32(59.5 * STEP)
    rays.setflags(write=False)
    kw = dict(degree=case.kind, occupied=occupied, terminate=case.terminate)
    return dict(rays=rays, stored=stored, occupied=occupied, kw=kw)


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (inputs, fp64 visibility, fp32 visibility, info of the fp64 walk), computed once (read-only)"""
    inp = inputs(case)
    info = {}
    v64 = visibility(inp["rays"], inp["stored"], C1, C2, STEP, dtype=torch.float64, info=info, **inp["kw"])
    v32 = visibility(inp["rays"], inp["stored"], C1, C2, STEP, dtype=torch.float32, **inp["kw"])
    return inp, v64, v32, info


def contention_rays(case, copies=64):
    """row 0 of the case's rays, `copies` times over"""
    return np.repeat(inputs(case)["rays"][:1], copies, axis=0)
