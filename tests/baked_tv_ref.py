"""Test helper (not a test): the total-variation prior of a baked volume (include/pixelnerf_hip.h, "Total-variation prior") restated
in plain torch at any dtype, its gradient by autograd, and the cases, error and bar that tests/test_baked_tv_host.py and
tests/test_hip_baked_tv.py share.  No GPU, no package import.

tv() is the definition: raw forward differences, 0 beyond the grid and -- with a `kept` mask, the sparse form -- 0 where either end
is not kept; n = sqrt(d_x^2 + d_y^2 + d_z^2 + eps); value = (1/N) sum_p sum_c w_c n(p,c) with N the number of grid points, or of
kept points.  The inputs proper -- stored, weights, eps -- are rounded to fp32 first and then carried in `dtype`.

Error and bar are those of tests/position_ref.py: error = max|got - ref64| / max|ref64|, bar = 10 x the error of torch's fp32
autograd through the same restatement on the same inputs, floor 2e-6, cap 2e-4.
"""
import collections
import functools

import numpy as np
import torch

import baked_grad_ref as G
import position_ref as P
import sparse_baked_ref as SP

error, bar_from, BAR_CAP = P.error, P.bar_from, P.BAR_CAP
EPS = 1e-8


def _fp32(x, dtype):
    """x rounded to fp32, then carried in `dtype`; always a fresh tensor"""
    return torch.tensor(np.array(x, np.float32)).to(dtype)


def tv(stored, weights, eps=EPS, kept=None):
    """stored: a torch tensor (nx,ny,nz,4) or (nx,ny,nz,B,4) at any dtype, through which autograd runs; weights: E = 4 or 4 B numbers;
    kept: None (the dense form) or (nx,ny,nz) bool, the sparse form: the dropped points count for nothing and a difference that
    touches one is 0.  -> the value, a 0-dim tensor at stored's dtype"""
    dtype = stored.dtype
    S = stored.reshape(tuple(stored.shape[:3]) + (-1,))
    w = _fp32(weights, dtype)
    e = float(np.float32(eps))
    assert w.shape == (S.shape[3],)
    on = None if kept is None else torch.as_tensor(np.asarray(kept, bool))
    diffs = []
    for axis in range(3):
        n = S.shape[axis]
        d = S.narrow(axis, 1, n - 1) - S.narrow(axis, 0, n - 1)
        if on is not None:
            both = on.narrow(axis, 1, n - 1) & on.narrow(axis, 0, n - 1)
            d = torch.where(both[..., None], d, torch.zeros_like(d))
        pad = list(S.shape)
        pad[axis] = 1
        diffs.append(torch.cat((d, torch.zeros(pad, dtype=dtype)), dim=axis))   # no neighbour beyond the grid
    dx, dy, dz = diffs
    norm = torch.sqrt(dx * dx + dy * dy + dz * dz + e)
    if on is None:
        return (norm * w).sum() / float(S.shape[0] * S.shape[1] * S.shape[2])
    return (torch.where(on[..., None], norm, torch.zeros_like(norm)) * w).sum() / float(int(on.sum()))


def value_and_gradient(stored, weights, eps=EPS, kept=None, dtype=torch.float64):
    """-> (value, d value / d stored) at `dtype`, the gradient by autograd, the shape of stored"""
    leaf = _fp32(stored, dtype).requires_grad_(True)
    value = tv(leaf, weights, eps, kept)
    (g,) = torch.autograd.grad(value, leaf)
    return value.detach(), g


# ---------------------------------------------------------------- weights
def weights(kind, degree):
    """E numbers for a row of a volume of `degree` (None: RGBA): "ones"; "rgb" / "sigma": that part of the RGBA or DC row alone, the
    higher basis rows taking the DC weights (what TrainableBaked.tv's sh=None means); "distinct": a different number per element"""
    nb = 1 if degree is None else (degree + 1) ** 2
    if kind == "ones":
        return [1.0] * (4 * nb)
    if kind == "rgb":
        return [1.0, 1.0, 1.0, 0.0] * nb
    if kind == "sigma":
        return [0.0, 0.0, 0.0, 1.0] * nb
    assert kind == "distinct"
    return [0.25 + 0.125 * ((5 * e) % 11) for e in range(4 * nb)]


# ---------------------------------------------------------------- the cases
RAMP_SLOPE = 0.375          # exact in fp32, as is every multiple of it on the grid
BLOCK = (slice(3, 6), slice(2, 5), slice(2, 5))   # the constant 3x3x3 block of the (9,8,7) grid; its centre:
BLOCK_CENTRE = (4, 3, 3)

# name, grid, degree (None: RGBA), weights kind, data ("noise": seeded random values plus a smooth part; "block": the same with a
# constant 3x3x3 block; "ramp": a linear ramp along x), sparse (None: dense; "third": the kept set of a random cell mask with about a
# third of the cells on; "all": every cell on)
Case = collections.namedtuple("Case", "name reso degree weights data sparse")
CASES = [
    Case("rgba_987_ones", (9, 8, 7), None, "ones", "noise", None),       # 504 points: two blocks
    Case("sh0_987_rgb", (9, 8, 7), 0, "rgb", "noise", None),
    Case("sh1_987_sigma", (9, 8, 7), 1, "sigma", "noise", None),         # 2016 float4s
    Case("sh2_987_distinct", (9, 8, 7), 2, "distinct", "noise", None),   # 4536 float4s: 18 blocks
    Case("rgba_222_distinct", (2, 2, 2), None, "distinct", "noise", None),   # every point on the border, every axis of length 2
    Case("sh1_222_ones", (2, 2, 2), 1, "ones", "noise", None),
    Case("rgba_253_ones", (2, 5, 3), None, "ones", "noise", None),
    Case("sh2_253_distinct", (2, 5, 3), 2, "distinct", "noise", None),
    Case("rgba_987_block", (9, 8, 7), None, "ones", "block", None),
    Case("sh1_987_block", (9, 8, 7), 1, "distinct", "block", None),
    Case("rgba_654_ramp", (6, 5, 4), None, "distinct", "ramp", None),
    Case("rgba_987_third", (9, 8, 7), None, "distinct", "noise", "third"),
    Case("sh2_987_third", (9, 8, 7), 2, "ones", "noise", "third"),
    Case("rgba_987_all", (9, 8, 7), None, "ones", "noise", "all"),
    Case("sh1_987_all", (9, 8, 7), 1, "sigma", "noise", "all"),
    Case("rgba_253_all", (2, 5, 3), None, "distinct", "noise", "all"),
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
DENSE_OF = {"rgba_987_all": "rgba_987_ones", "sh1_987_all": "sh1_987_sigma"}   # a sparse case with every cell on -> its dense twin


def volume(reso, degree, data, seed):
    tail = (4,) if degree is None else ((degree + 1) ** 2, 4)
    rs = np.random.RandomState(seed)
    ax = [np.linspace(-1.0, 1.0, n) for n in reso]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    if data == "ramp":
        vol = np.zeros(reso + tail, np.float32)
        vol += (RAMP_SLOPE * np.arange(reso[0], dtype=np.float32)).reshape((-1, 1, 1) + (1,) * len(tail))
        return vol
    smooth = 0.5 + 0.4 * np.sin(2.0 * X + 0.3) * np.cos(1.7 * Y - 0.2) + 0.3 * Z
    vol = (0.3 * rs.standard_normal(reso + tail) + smooth.reshape(reso + (1,) * len(tail))).astype(np.float32)
    vol[..., 3] = vol[..., 3] * np.float32(4.0)            # sigma on a larger scale than rgb, as in a baked volume
    if data == "block":
        vol[BLOCK] = vol[BLOCK_CENTRE]
    return vol


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> dict of the fp32 inputs of one case (numpy; shared: treat as read-only): stored (the dense array), weights, and for a sparse
    case cells, index (nx,ny,nz) int32, ids (M,) int32, kept (nx,ny,nz) bool and rows = stored at ids"""
    seed = 100 + CASES.index(case)
    if case.sparse == "all" and case.name in DENSE_OF:
        seed = 100 + CASES.index(BY_NAME[DENSE_OF[case.name]])     # the values of the dense twin
    stored = volume(case.reso, case.degree, case.data, seed)
    out = dict(stored=stored, weights=weights(case.weights, case.degree), kept=None)
    if case.sparse is not None:
        shape = tuple(n - 1 for n in case.reso)
        cells = np.ones(shape, bool) if case.sparse == "all" else np.random.RandomState(seed + 50).uniform(size=shape) < 1.0 / 3.0
        index, ids = SP.sparse_points(cells)
        tail = stored.shape[3:]
        out.update(cells=cells, index=index, ids=ids, kept=index >= 0, rows=np.ascontiguousarray(stored.reshape((-1,) + tail)[ids]))
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (inputs, value64, gradient64, value32, gradient32) of one case, computed once (treat as read-only); the gradients of a sparse
    case are those of its rows, (M,4) or (M,B,4)"""
    inp = inputs(case)
    out = [inp]
    for dtype in (torch.float64, torch.float32):
        value, g = value_and_gradient(inp["stored"], inp["weights"], EPS, inp["kept"], dtype)
        if case.sparse is not None:
            g = g.reshape((-1,) + tuple(g.shape[3:]))[torch.from_numpy(inp["ids"].astype(np.int64))]
        out += [value, g]
    return tuple(out)


# ---------------------------------------------------------------- util.bake.fit with the prior, restated on the host
# The prior of the fit test weighs rgb alone: the start of baked_grad_ref.fit_scene moves every rgb by up to 0.2, point by point,
# and 40 steps of Adam at lr 2e-2 can move a value by 0.8, so the prior can flatten that noise within the loop; the sigma noise
# (up to 6 at the blob's peak) is beyond what 40 such steps can move.  eps = 1e-2 rounds the kink of |d| over a radius of 0.1: the
# loop then stays a smooth function of its roundings, and the fp32 and fp64 runs stay together (their spread sets the margin).
FIT_TV = dict(tv_rgb=0.1, tv_sigma=0.0, tv_sh=None, tv_eps=1e-2)


def fit_weights(degree, tv_rgb, tv_sigma, tv_sh):
    nb = 1 if degree is None else (degree + 1) ** 2
    dc = [tv_rgb, tv_rgb, tv_rgb, tv_sigma]
    return dc + (dc if tv_sh is None else [tv_sh] * 4) * (nb - 1)


def fit_ref(degree, dtype, steps, lr, batch, seed, tv_rgb=0.0, tv_sigma=0.0, tv_sh=None, tv_eps=EPS):
    """baked_grad_ref.fit_ref with util.bake.fit's prior: the step's loss is mse + tv(stored) when any weight is > 0
    -> (the mse of every batch as floats, the fitted values as an fp32 array)"""
    known, start, rays = G.fit_scene(degree)
    w = fit_weights(degree, tv_rgb, tv_sigma, tv_sh)
    use_prior = any(x > 0 for x in w)
    with torch.no_grad():
        target = G.march(rays, _fp32(known, dtype), G.FIT_C1, G.FIT_C2, G.FIT_STEP, degree=degree, dtype=dtype)[0]
    stored = _fp32(start, dtype).requires_grad_(True)
    optimiser = torch.optim.Adam([stored], lr=lr)
    gen = torch.Generator().manual_seed(seed)
    losses = []
    for _ in range(steps):
        ids = torch.randint(0, rays.shape[0], (min(batch, rays.shape[0]),), generator=gen)
        rgb = G.march(rays[ids.numpy()], stored, G.FIT_C1, G.FIT_C2, G.FIT_STEP, degree=degree, dtype=dtype)[0]
        loss = ((rgb - target[ids]) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        (loss + tv(stored, w, tv_eps) if use_prior else loss).backward()
        optimiser.step()
        if degree is None:
            with torch.no_grad():
                stored[..., :3].clamp_(0.0, 1.0)
                stored[..., 3].clamp_(min=0.0)
        losses.append(float(loss.detach()))
    return losses, stored.detach().float().numpy()


def tv_of(values, degree, tv_rgb, tv_sigma, tv_sh, tv_eps):
    """the fp64 total variation of an fp32 array under the prior's weights"""
    with torch.no_grad():
        return float(tv(_fp32(values, torch.float64), fit_weights(degree, tv_rgb, tv_sigma, tv_sh), tv_eps))
