"""Test helper (not a test): the scene march of tests/baked_scene_grad_ref.py restated with every object's STORED tensor as an
autograd leaf, the references and the fitting loop that tests/test_baked_scene_fit_host.py and tests/test_hip_baked_scene_fit.py
share.  No GPU, no package import.

baked_scene_grad_ref._object_value rebuilds `stored` from numpy, so autograd cannot reach it; `_object_value` here is that function
with the tensor handed in, and `march` is that module's march around it.  Everything else -- the object rays, the cases, the
kept-rows rule, the upstream gradients (exactly 0 on the rows the rule drops or that stop near the threshold), error and bar --
comes from the existing helpers.  The host test holds this march to baked_scene_grad_ref.march under torch.equal, its gradient with
one object at the identity to baked_grad_ref.gradient, and its gradients to central differences in fp64.
"""
import functools

import numpy as np
import torch

import baked_grad_ref as G
import baked_ray_grad_ref as RG
import baked_ref as B
import baked_scene_grad_ref as R
import baked_scene_ref as SC

error, bar_from = G.error, G.bar_from
_fp32 = R._fp32


def _object_value(oray, t, exists, ob, stored, dtype):
    """baked_scene_grad_ref._object_value with the stored tensor (at `dtype`, fp32-representable values) handed in"""
    degree, occupied = ob["degree"], ob["occupied"]
    c1t, c2t = _fp32(ob["c1"], dtype), _fp32(ob["c2"], dtype)
    reso = tuple(stored.shape[:3])
    h = torch.as_tensor(B.cell_size(ob["c1"], ob["c2"], reso, np.float64)).to(dtype)
    R_, nmax = t.shape
    o, d = oray[:, 0:3], oray[:, 3:6]
    p = o[:, None, :] + t[:, :, None] * d[:, None, :]
    inside = ((p >= c1t) & (p <= c2t)).all(dim=2)
    u = (p - c1t) / h
    top = torch.tensor([r - 2 for r in reso], dtype=dtype)
    with torch.no_grad():
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
                corners.append(v)
    v = torch.stack(corners, dim=2).reshape(R_, nmax, 2, 2, 2, 4)
    fx, fy, fz = f[..., 0, None], f[..., 1, None], f[..., 2, None]
    vz = v[:, :, :, :, 0] + fz[:, :, None, None] * (v[:, :, :, :, 1] - v[:, :, :, :, 0])
    vy = vz[:, :, :, 0] + fy[:, :, None] * (vz[:, :, :, 1] - vz[:, :, :, 0])
    val = vy[:, :, 0] + fx * (vy[:, :, 1] - vy[:, :, 0])
    return torch.where(active[..., None], val, torch.zeros_like(val)), active


def march(rays, poses, stored, objects, step, white_bkgd=False, terminate=0.0):
    """baked_scene_grad_ref.march with `stored`: a list of one tensor per object at the dtype of rays and poses, through which
    autograd runs (the objects' own "stored" is not looked at).  -> rgb (R,3), depth (R,), alpha (R,)"""
    dtype = rays.dtype
    stepv, eps = float(np.float32(step)), float(np.float32(terminate))
    R_ = rays.shape[0]
    near, far = rays[:, 6], rays[:, 7]
    with torch.no_grad():
        ok = torch.isfinite(rays).all(dim=1) & (near < far)
        count = torch.ceil((far - near) / torch.tensor(stepv, dtype=dtype))
        n = torch.where(ok & (count <= G.MAX_SAMPLES), count, torch.zeros_like(count)).long()
    nmax = int(n.max()) if R_ else 0
    i = torch.arange(nmax, dtype=dtype)
    exists = torch.arange(nmax)[None, :] < n[:, None]
    t = near[:, None] + (i[None, :] + 0.5) * stepv
    vals = [_object_value(R.object_rays(rays, poses[j]), t, exists, ob, stored[j], dtype)[0] for j, ob in enumerate(objects)]
    sigma = vals[0][..., 3]
    for val in vals[1:]:
        sigma = sigma + val[..., 3]
    positive = sigma > 0
    safe = torch.where(positive, sigma, torch.ones_like(sigma))
    colour = torch.zeros_like(vals[0][..., :3])
    for val in vals:
        colour = colour + (val[..., 3] / safe)[..., None] * val[..., :3]
    colour = torch.where(positive[..., None], colour, torch.zeros_like(colour))

    a = 1.0 - torch.exp(-(stepv * sigma))
    tfac = torch.where(exists, 1.0 - a + torch.tensor(1e-10, dtype=dtype), torch.ones_like(a))
    incl = torch.cumprod(tfac, dim=1)
    T = torch.cat((torch.ones((R_, 1), dtype=dtype), incl[:, :-1]), dim=1) if nmax else incl
    walked = exists
    full = incl[:, 63::64].detach()
    chunk_exists = (64 * (torch.arange(full.shape[1]) + 1))[None, :] <= n[:, None]
    if eps > 0 and full.shape[1]:
        stop = (full <= eps) & chunk_exists
        first = torch.where(stop.any(dim=1), stop.float().argmax(dim=1), torch.full((R_,), full.shape[1]))
        walked = exists & (torch.arange(nmax)[None, :] < 64 * (first[:, None] + 1))
    w = torch.where(walked, a * T, torch.zeros_like(a))
    rgb = (w[..., None] * colour).sum(dim=1)
    depth = (w * t).sum(dim=1)
    alpha = w.sum(dim=1)
    if white_bkgd:
        rgb = rgb + 1.0 - alpha[:, None]
    return rgb, depth, alpha


def leaves(objects, dtype, share=False):
    """one autograd leaf per object, from its "stored"; share: objects whose "stored" is the SAME array get ONE leaf (a volume
    listed twice) -> the list of leaves, one entry per object"""
    made, out = {}, []
    for ob in objects:
        key = id(ob["stored"]) if share else len(out)
        if key not in made:
            made[key] = _fp32(ob["stored"], dtype).requires_grad_(True)
        out.append(made[key])
    return out


def gradients(rays, objects, step, d_rgb=None, d_depth=None, d_alpha=None, dtype=torch.float64, poses=None, share=False, **kw):
    """-> the list of dL/d stored_j at `dtype`, one per object, by autograd for L = the sum of baked_ray_grad_ref.loss_per_ray;
    share: a volume listed twice is one leaf and its gradient (the sum of both listings') stands at both positions"""
    stored = leaves(objects, dtype, share)
    pose_t = _fp32(R.stack_poses(objects) if poses is None else poses, dtype)
    L = RG.loss_per_ray(march(_fp32(rays, dtype), pose_t, stored, objects, step, **kw), d_rgb, d_depth, d_alpha, dtype).sum()
    unique = list({id(s): s for s in stored}.values())
    got = torch.autograd.grad(L, unique, allow_unused=True)
    by_id = {id(s): (torch.zeros_like(s) if g is None else g) for s, g in zip(unique, got)}
    return [by_id[id(s)] for s in stored]


def _with_stored_refs(ref):
    out = dict(ref)
    args = (ref["rays"], ref["objects"], ref["step"])
    out["ref64"] = gradients(*args, dtype=torch.float64, **ref["ups"], **ref["kw"])
    out["ref32"] = gradients(*args, dtype=torch.float32, **ref["ups"], **ref["kw"])
    for j, g in enumerate(out["ref64"]):
        assert bool(g.any()), f"object {j} gets no gradient"
    return out


@functools.lru_cache(maxsize=None)
def reference(degree, name, setting):
    """baked_scene_grad_ref.reference(degree, name, setting) -- rays, objects, step, held, ups (exactly 0 off `held`), kw; its own
    assertions on dropped and met rays hold -- with ref64 / ref32 replaced by the lists of d_stored_j by autograd at fp64 / fp32;
    every object has a non-zero element in ref64.  Computed once; treat as read-only."""
    return _with_stored_refs(R.reference(degree, name, setting))


@functools.lru_cache(maxsize=None)
def long_reference():
    """baked_scene_grad_ref.long_reference() (n4500, 71 chunks, 4 held rays) with the stored gradients"""
    return _with_stored_refs(R.long_reference())


@functools.lru_cache(maxsize=None)
def identity_reference(degree):
    """ONE object at the identity: object A of the parity cases with its skip grid at threshold 10, baked_grad_ref.case_rays(
    "n150"), white background -> the dict of `reference` plus `single64`, baked_grad_ref.gradient on the same inputs.  The two
    agree to round-off as long as no sample that contributes blends a sigma of EXACTLY 0: there the scene's colour is the
    constant 0 (the convention of the mixing) where the single march keeps the blended colour, and the derivative with respect
    to sigma differs by T step (d_rgb . c).  A has empty points (sigma exactly 0); the skip grid keeps the cells made of them
    out of both marches."""
    objects = R.with_bits([SC.obj(SC.stored_pair(degree)[0], degree=degree)], 10.0)
    ref = _with_stored_refs(R._reference(G.case_rays("n150"), objects, G.SETTINGS["n150"][1], 0.0, True, 2024))
    ref["single64"] = G.gradient(ref["rays"], objects[0]["stored"], G.C1, G.C2, ref["step"], dtype=torch.float64, degree=degree,
                                 occupied=objects[0]["occupied"], **ref["ups"], **ref["kw"])
    return ref


def hold(what, got, ref64, ref32):
    """print HIP error, torch-fp32 error and bar of ONE object's gradient, then hold `got` to the bar -> the bar"""
    got = got.detach().cpu().reshape(ref64.shape)
    err, err32 = error(got, ref64), error(ref32.double(), ref64)
    bar = bar_from(err32)
    print(f"{what}: HIP error {err:.3e}, torch-fp32 error {err32:.3e}, bar {bar:.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert err <= bar, (what, err, bar)
    return bar


# ---------------------------------------------------------------- the fitting loop of util.bake.fit_scene, restated on the host
FIT = dict(steps=40, lr=2e-2, batch=128, seed=3)
# the second object: baked_scene_grad_ref.POSE_OVERLAP's rotation, its translation scaled by 0.6 so that the object stays in view of
# baked_grad_ref.fit_scene's rays (they aim at the inner box [-0.6, 0.6]^3); both boxes are [-1, 1]^3 and overlap
FIT_POSES = np.stack((R.IDENTITY, np.concatenate((R.POSE_OVERLAP[:, :3], R.POSE_OVERLAP[:, 3:] * np.float32(0.6)), axis=1))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fit_scene():
    """-> (known (2,12,12,12,4), start (2,12,12,12,4), rays (512,8)) fp32 arrays (treat as read-only): object 0 is
    baked_grad_ref.fit_scene's RGBA blob and its perturbed start; object 1 the same with the colour channels rolled by one and the
    grid mirrored along x, so that the two differ where they overlap"""
    known, start, rays = G.fit_scene(None)
    second = lambda v: np.ascontiguousarray(np.concatenate((np.roll(v[..., :3], 1, axis=-1), v[..., 3:]), axis=-1)[::-1])
    out = (np.stack((known, second(known))), np.stack((start, second(start))), rays)
    for a in out:
        a.setflags(write=False)
    return out


def fit_objects(stored):
    return [SC.obj(stored[j], FIT_POSES[j], G.FIT_C1, G.FIT_C2) for j in range(2)]


@functools.lru_cache(maxsize=None)
def fit_ref(dtype, steps, lr, batch, seed):
    """util.bake.fit_scene through the restatement at `dtype` on the CPU: the target is the restatement's render of the known pair,
    the batches, the optimiser and the projection are fit_scene's (baked_grad_ref.fit_ref's, on two leaves) -> the batch losses"""
    known, start, rays = fit_scene()
    objects = fit_objects(known)
    poses, rays_t = _fp32(FIT_POSES, dtype), _fp32(rays, dtype)
    with torch.no_grad():
        target = march(rays_t, poses, [_fp32(k, dtype) for k in known], objects, G.FIT_STEP)[0]
    stored = [_fp32(s, dtype).requires_grad_(True) for s in start]
    optimiser = torch.optim.Adam(stored, lr=lr)
    gen = torch.Generator().manual_seed(seed)
    losses = []
    for _ in range(steps):
        ids = torch.randint(0, rays.shape[0], (min(batch, rays.shape[0]),), generator=gen)
        rgb = march(rays_t[ids], poses, stored, objects, G.FIT_STEP)[0]
        loss = ((rgb - target[ids]) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        loss.backward()
        optimiser.step()
        with torch.no_grad():
            for s in stored:
                s[..., :3].clamp_(0.0, 1.0)
                s[..., 3].clamp_(min=0.0)
        losses.append(float(loss.detach()))
    return losses
