"""Test helper (not a test): the scene march of tests/baked_scene_ref.py restated in torch with the WORLD RAYS and the OBJECT POSES
(N,3,4) as autograd leaves, the cases, the kept-rows rule and the placing loop that tests/test_baked_scene_grad_host.py and
tests/test_hip_baked_scene_grad.py share.  No GPU, no package import.

It composes baked_scene_ref.object_rays' operations (the ray in an object's frame), baked_ray_grad_ref.march's per-object value (the
point, the inside test, the cell, the blend, for a coefficient volume the basis on the ROTATED direction and the clamps per corner)
and the mixing of the header ("Gradients of the scene march"): sigma = sum_j sigma_j, c = sum_j (sigma_j / sigma) c_j where
sigma > 0 and the constant 0 elsewhere (torch.where: the branch not taken sends nothing back).  The gradient with respect to the ray
in an object's frame (d_local) is read off the intermediate tensor.

Kept-rows rule: a ray is kept if baked_ray_grad_ref.kept_rows keeps its object ray in EVERY object's frame and grid; upstream
gradients are exactly 0 on the other rays, so that d_poses sums kept rays only.  Error and bar are the project's
(baked_grad_ref.error, bar_from), applied to d_rays, d_local and d_poses separately.
"""
import functools

import numpy as np
import torch

import baked_grad_ref as G
import baked_ray_grad_ref as RG
import baked_ref as B
import baked_scene_ref as SC
import sparse_baked_ref as SP

error, bar_from, hold = RG.error, RG.bar_from, RG.hold
MAX_DROPPED = RG.MAX_DROPPED
MIN_MET = 4   # kept rays that meet each object of each case


def _fp32(x, dtype):
    return torch.tensor(np.array(x, np.float32)).to(dtype)


def pose_of(w, t):
    """axis-angle w and translation t -> (3,4) fp32 object-to-world: Rodrigues in fp64, rounded to fp32 once"""
    rot = RG.rodrigues(torch.tensor(w, dtype=torch.float64)).numpy()
    return np.concatenate((rot, np.asarray(t, np.float64).reshape(3, 1)), axis=1).astype(np.float32)


# generic poses (no entry in {0, +-1}): the object rays sit on cell planes no more often than chance puts them there
POSE_OVERLAP = pose_of((0.3, -0.5, 0.8), (0.25, -0.5, 0.125))
POSE_DISJOINT = pose_of((-0.2, 0.4, 1.1), (-1.9375, 0.0, 0.0))
# (the third object stood at t = (0, 0.3, -0.9): with the skip grid at threshold 10 only 3 kept rays met it at degree 2, below
# MIN_MET; moved towards the centre -- the object, not the cap -- 6 do, and no further ray is dropped)
POSE_THIRD = pose_of((0.1, 0.2, -0.3), (0.0, 0.2, -0.5))
POSE_SMALL = pose_of((0.7, 0.1, 0.4), (0.9, 0.2, 0.1))
IDENTITY = SC.IDENTITY


def cases(degree):
    """the scenes of the parity tests, baked_scene_ref.cases' volumes at generic poses: name -> list of baked_scene_ref.obj"""
    a, b = SC.stored_pair(degree)
    return {
        "overlap": [SC.obj(a, degree=degree), SC.obj(b, POSE_OVERLAP, degree=degree)],
        "disjoint": [SC.obj(a, degree=degree), SC.obj(b, POSE_DISJOINT, degree=degree)],
        "three": [SC.obj(a, degree=degree), SC.obj(SC.small_volume(degree=degree), POSE_SMALL, SC.SMALL_C1, SC.SMALL_C2, degree=degree),
                  SC.obj(b, POSE_THIRD, degree=degree)],
    }


def sigma_of(ob):
    """the density that decides an object's skip grid: sigma, or its DC coefficient"""
    return ob["stored"][..., 3] if ob["degree"] is None else ob["stored"][..., 0, 3]


def with_bits(objects, threshold):
    """the objects with `occupied` set to the cells of pnr_occupancy_build at `threshold`, dilate 0"""
    return [dict(ob, occupied=SP.occupied_cells(sigma_of(ob), threshold)) for ob in objects]


def object_rays(rays, pose):
    """baked_scene_ref.object_rays in torch: rays (R,8) and pose (3,4) at one dtype, autograd through both -> (R,8)"""
    rot, t = pose[:, :3], pose[:, 3]
    q, d = rays[:, 0:3] - t[None, :], rays[:, 3:6]
    cols = [(q[:, 0] * rot[0, a] + q[:, 1] * rot[1, a]) + q[:, 2] * rot[2, a] for a in range(3)]
    cols += [(d[:, 0] * rot[0, a] + d[:, 1] * rot[1, a]) + d[:, 2] * rot[2, a] for a in range(3)]
    return torch.cat((torch.stack(cols, dim=1), rays[:, 6:8]), dim=1)


def _object_value(oray, t, exists, ob, dtype):
    """the (r,g,b,sigma) of one object at the depths t (R,nmax) of its object rays: baked_ray_grad_ref.march's per-sample part
    -> (val (R,nmax,4), zeros where the object does not contribute; active (R,nmax))"""
    stored = _fp32(ob["stored"], dtype)
    degree, occupied = ob["degree"], ob["occupied"]
    c1t, c2t = _fp32(ob["c1"], dtype), _fp32(ob["c2"], dtype)
    reso = tuple(stored.shape[:3])
    h = torch.as_tensor(B.cell_size(ob["c1"], ob["c2"], reso, np.float64)).to(dtype)
    R, nmax = t.shape
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
    v = torch.stack(corners, dim=2).reshape(R, nmax, 2, 2, 2, 4)
    fx, fy, fz = f[..., 0, None], f[..., 1, None], f[..., 2, None]
    vz = v[:, :, :, :, 0] + fz[:, :, None, None] * (v[:, :, :, :, 1] - v[:, :, :, :, 0])
    vy = vz[:, :, :, 0] + fy[:, :, None] * (vz[:, :, :, 1] - vz[:, :, :, 0])
    val = vy[:, :, 0] + fx * (vy[:, :, 1] - vy[:, :, 0])
    return torch.where(active[..., None], val, torch.zeros_like(val)), active


def march(rays, poses, objects, step, white_bkgd=False, terminate=0.0, info=None):
    """rays (R,8) and poses (N,3,4): torch tensors at one dtype holding fp32-representable values, autograd through both; objects a
    list of baked_scene_ref.obj whose own "pose" is NOT looked at.  -> rgb (R,3), depth (R,), alpha (R,).
    info: a dict that receives `orays` (the N object-ray tensors, with retain_grad), `met` (R,N) bool: the object contributes to a
    sample of the ray, and `boundaries` (R, chunks): the transmittance after every full chunk (inf where the chunk does not exist)"""
    dtype = rays.dtype
    stepv, eps = float(np.float32(step)), float(np.float32(terminate))
    R = rays.shape[0]
    near, far = rays[:, 6], rays[:, 7]
    with torch.no_grad():
        ok = torch.isfinite(rays).all(dim=1) & (near < far)
        count = torch.ceil((far - near) / torch.tensor(stepv, dtype=dtype))
        n = torch.where(ok & (count <= G.MAX_SAMPLES), count, torch.zeros_like(count)).long()
    nmax = int(n.max()) if R else 0
    i = torch.arange(nmax, dtype=dtype)
    exists = torch.arange(nmax)[None, :] < n[:, None]
    t = near[:, None] + (i[None, :] + 0.5) * stepv
    orays, vals, met = [], [], []
    for j, ob in enumerate(objects):
        oray = object_rays(rays, poses[j])
        if oray.requires_grad:
            oray.retain_grad()
        val, active = _object_value(oray, t, exists, ob, dtype)
        orays.append(oray)
        vals.append(val)
        met.append(active.any(dim=1))
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
    T = torch.cat((torch.ones((R, 1), dtype=dtype), incl[:, :-1]), dim=1) if nmax else incl
    walked = exists
    full = incl[:, 63::64].detach()
    chunk_exists = (64 * (torch.arange(full.shape[1]) + 1))[None, :] <= n[:, None]
    if eps > 0 and full.shape[1]:
        stop = (full <= eps) & chunk_exists
        first = torch.where(stop.any(dim=1), stop.float().argmax(dim=1), torch.full((R,), full.shape[1]))
        walked = exists & (torch.arange(nmax)[None, :] < 64 * (first[:, None] + 1))
    if info is not None:
        info.update(orays=orays, met=torch.stack(met, dim=1), boundaries=torch.where(chunk_exists, full, torch.full_like(full, float("inf"))))
    w = torch.where(walked, a * T, torch.zeros_like(a))
    rgb = (w[..., None] * colour).sum(dim=1)
    depth = (w * t).sum(dim=1)
    alpha = w.sum(dim=1)
    if white_bkgd:
        rgb = rgb + 1.0 - alpha[:, None]
    return rgb, depth, alpha


def stack_poses(objects):
    return np.stack([np.asarray(ob["pose"], np.float32)[:3] for ob in objects])


def gradients(rays, objects, step, d_rgb=None, d_depth=None, d_alpha=None, dtype=torch.float64, poses=None, **kw):
    """-> (d_rays (R,8), d_local (R,N,6), d_poses (N,3,4)) at `dtype` by autograd for L = the sum of baked_ray_grad_ref.loss_per_ray"""
    ray_leaf = _fp32(rays, dtype).requires_grad_(True)
    pose_leaf = _fp32(stack_poses(objects) if poses is None else poses, dtype).requires_grad_(True)
    info = {}
    L = RG.loss_per_ray(march(ray_leaf, pose_leaf, objects, step, info=info, **kw), d_rgb, d_depth, d_alpha, dtype).sum()
    L.backward()
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    d_local = torch.stack([zero(o.grad, o)[:, :6] for o in info["orays"]], dim=1)
    return zero(ray_leaf.grad, ray_leaf), d_local, zero(pose_leaf.grad, pose_leaf)


def kept_rows(rays, objects, step):
    """the rule: a ray is kept if baked_ray_grad_ref.kept_rows keeps its object ray in every object's frame and grid -> (R,) bool"""
    kept = torch.ones((len(rays),), dtype=torch.bool)
    for ob in objects:
        moved = SC.object_rays(rays, ob["pose"], np.float32)
        kept &= RG.kept_rows(moved, ob["c1"], ob["c2"], ob["stored"].shape[:3], step)
    return kept


# setting name -> (the setting of baked_grad_ref.case_rays, the threshold of the skip grids or None, terminate, white background)
SETTINGS = {"n150": ("n150", None, 0.0, False), "n150_bits10_terminate": ("n150", 10.0, 1e-2, False), "n40_white": ("n40", None, 0.0, True)}
LONG_SCALE = 0.15   # sigma of the long-ray case (baked_grad_ref.LONG rows at n4500)


def off_the_stop(rays, objects, step, eps):
    """-> (R,) bool: the fp64 transmittance at every boundary of 64 samples is <= eps / 2 or >= 2 eps, as baked_grad_ref.TERM_* were
    chosen: fp32 and fp64 stop after the same chunk"""
    info = {}
    with torch.no_grad():
        march(_fp32(rays, torch.float64), _fp32(stack_poses(objects), torch.float64), objects, step, info=info)
    b = info["boundaries"]
    return ((b <= eps / 2) | (b >= 2 * eps)).all(dim=1)


def _reference(rays, objects, step, terminate, white, seed):
    kept = kept_rows(rays, objects, step)
    held = kept & off_the_stop(rays, objects, step, terminate) if terminate > 0 else kept
    rs = np.random.RandomState(seed)
    R = rays.shape[0]
    keep = held.numpy()[:, None].astype(np.float32)
    ups = dict(d_rgb=rs.standard_normal((R, 3)).astype(np.float32) * keep, d_depth=rs.standard_normal((R,)).astype(np.float32) * keep[:, 0],
               d_alpha=rs.standard_normal((R,)).astype(np.float32) * keep[:, 0])
    kw = dict(white_bkgd=white, terminate=terminate)
    info = {}
    with torch.no_grad():
        march(_fp32(rays, torch.float64), _fp32(stack_poses(objects), torch.float64), objects, step, info=info, **kw)
    met = info["met"] & held[:, None]
    return dict(rays=rays, objects=objects, step=step, kept=kept, held=held, met=met, ups=ups, kw=kw,
                ref64=gradients(rays, objects, step, dtype=torch.float64, **ups, **kw),
                ref32=gradients(rays, objects, step, dtype=torch.float32, **ups, **kw))


@functools.lru_cache(maxsize=None)
def reference(degree, name, setting):
    """-> dict of one parity case (computed once; treat as read-only): rays, objects (with their skip cells), step, kept (the rule),
    held (kept, and off the stop where the case terminates: the rows whose upstream gradients are not zero), met (R,N), ups (d_rgb,
    d_depth, d_alpha: exactly 0 off `held`), kw, and ref64 / ref32 = (d_rays, d_local, d_poses) by autograd at fp64 / fp32"""
    ray_setting, thr, terminate, white = SETTINGS[setting]
    objects = cases(degree)[name]
    if thr is not None:
        objects = with_bits(objects, thr)
    rays = G.case_rays(ray_setting)
    seed = 777 + 31 * sorted(SETTINGS).index(setting) + 7 * ["overlap", "disjoint", "three"].index(name) + (0 if degree is None else 3)
    ref = _reference(rays, objects, G.SETTINGS[ray_setting][1], terminate, white, seed)
    dropped = int((~ref["kept"]).sum())
    assert dropped <= MAX_DROPPED, (degree, name, setting, dropped)
    assert int(ref["met"].sum(dim=0).min()) >= MIN_MET, (degree, name, setting, ref["met"].sum(dim=0).tolist())
    return ref


@functools.lru_cache(maxsize=None)
def long_reference():
    """the long-ray case: RGBA, n4500, sigma scaled by 0.15, baked_grad_ref.LONG rows; A at the identity, B at the overlap pose.
    With 4500 samples in two frames the rule drops 2 of the 6 rows (in B's frame); the 4 held ones still cross density beyond
    sample 4096 in A, two of them in B as well"""
    a, b = (v.copy() for v in SC.stored_pair(None))
    a[..., 3] *= np.float32(LONG_SCALE)
    b[..., 3] *= np.float32(LONG_SCALE)
    objects = [SC.obj(a), SC.obj(b, POSE_OVERLAP)]
    ref = _reference(G.case_rays("n4500", G.LONG), objects, G.SETTINGS["n4500"][1], 0.0, False, 4321)
    assert int(ref["kept"].sum()) == 4, ref["kept"].tolist()
    return ref


# ---------------------------------------------------------------- the tangent of the rigid motions
def moved_poses(poses0, w, v):
    """util.bake.moved_poses on (N,3,4): P = [R(w) R0 | t0 + v]"""
    return torch.cat((RG.rodrigues(w) @ poses0[:, :, :3], (poses0[:, :, 3] + v)[:, :, None]), dim=2)


def project(d_poses, poses0):
    """the 12-number gradient (N,3,4) at P = poses0 -> its projection (d_w (N,3), d_v (N,3)) onto (w, v) at 0 through moved_poses"""
    w = torch.zeros((poses0.shape[0], 3), dtype=poses0.dtype, requires_grad=True)
    v = torch.zeros((poses0.shape[0], 3), dtype=poses0.dtype, requires_grad=True)
    (moved_poses(poses0, w, v) * d_poses).sum().backward()
    return w.grad, v.grad


# ---------------------------------------------------------------- placing: util.bake.place on the host
REG = RG.REG
PLACE = dict(c1=(-0.6, -0.6, -0.6), c2=(0.6, 0.6, 0.6), steps=120, lr=1e-2, start_deg=8.0, start_shift=0.1,
             true_w=(0.25, -0.4, 0.6), true_t=(0.55, -0.45, 0.6), start_axis=(0.4, -0.3, 0.86), shift_dir=(0.6, 0.0, -0.8))
PLACE_BLOBS = (((0.2, 0.15, -0.2), 0.16, (0.95, 0.85, 0.1)), ((-0.25, -0.1, 0.2), 0.14, (0.1, 0.85, 0.9)))


@functools.lru_cache(maxsize=None)
def place_scene():
    """-> (stored of object 0: baked_ray_grad_ref.reg_scene's blobs on [-1,1]^3, fixed at the identity; stored of object 1: two
    blobs on [-0.6,0.6]^3, both (16,16,16,4) fp32; the true poses (2,3,4); the start poses (2,3,4): object 1 turned by 8 degrees about
    its own origin and shifted by 0.1; the cameras (3,4,4)) as numpy arrays (treat as read-only)"""
    first, cams, _ = RG.reg_scene(None)
    ax = [np.linspace(lo, hi, n) for lo, hi, n in zip(PLACE["c1"], PLACE["c2"], REG["reso"])]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    sigma, colour = np.zeros(REG["reso"]), np.zeros(REG["reso"] + (3,))
    for centre, width, rgb in PLACE_BLOBS:
        g = np.exp(-((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) / (2.0 * width * width))
        sigma += 16.0 * g
        colour += g[..., None] * np.asarray(rgb)
    colour = colour / np.maximum(colour.sum(axis=-1, keepdims=True) / 1.6, 1e-6)
    second = np.concatenate((np.clip(colour, 0.0, 1.0), sigma[..., None]), axis=-1).astype(np.float32)
    true = np.stack((IDENTITY, pose_of(PLACE["true_w"], PLACE["true_t"])))
    w = np.asarray(PLACE["start_axis"]) / np.linalg.norm(PLACE["start_axis"]) * np.deg2rad(PLACE["start_deg"])
    shift = np.asarray(PLACE["shift_dir"]) / np.linalg.norm(PLACE["shift_dir"]) * PLACE["start_shift"]
    moved = moved_poses(torch.from_numpy(true[1:]).double(), torch.from_numpy(w)[None], torch.from_numpy(shift)[None]).float().numpy()
    start = np.concatenate((true[:1], moved))
    out = (first, np.ascontiguousarray(second), true, np.ascontiguousarray(start), cams)
    for a in out:
        a.setflags(write=False)
    return out


def place_objects():
    first, second, _, _, _ = place_scene()
    return [SC.obj(first, c1=REG["c1"], c2=REG["c2"]), SC.obj(second, c1=PLACE["c1"], c2=PLACE["c2"])]


def place_errors(poses, true):
    """-> (rotation error in degrees, translation error) of object 1: poses and true (2,3,4) tensors"""
    rot, shift = RG.pose_errors(poses[1:], true[1:])
    return float(rot[0]), float(shift[0])


@functools.lru_cache(maxsize=None)
def place_ref(dtype=torch.float32):
    """util.bake.place(objects=[1]) through the restatement at `dtype` on the CPU: the target is the restatement's render of the true
    poses (white background), Adam with place's settings on (w, v) of object 1 from zero -> (poses (2,3,4), losses), computed once"""
    _, _, true, start, cams = place_scene()
    objects, r = place_objects(), REG
    rays = RG.gen_rays(_fp32(cams, dtype), r["W"], r["H"], r["focal"], r["z_near"], r["z_far"]).reshape(-1, 8)
    render = lambda poses: march(rays, poses, objects, r["step"], white_bkgd=True)[0]
    with torch.no_grad():
        target = render(_fp32(true, dtype))
    poses0 = _fp32(start, dtype)
    w = torch.zeros((1, 3), dtype=dtype, requires_grad=True)
    v = torch.zeros((1, 3), dtype=dtype, requires_grad=True)
    optimiser = torch.optim.Adam([w, v], lr=PLACE["lr"])
    current = lambda: torch.cat((poses0[:1], moved_poses(poses0[1:], w, v)), dim=0)
    losses = []
    for _ in range(PLACE["steps"]):
        loss = ((render(current()) - target) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        loss.backward()
        optimiser.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        return current(), losses
