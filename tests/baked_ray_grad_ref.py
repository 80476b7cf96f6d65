"""Test helper (not a test): the baked-volume ray march of tests/baked_grad_ref.py restated with the RAYS (and, for the joint cases,
the stored values) as autograd leaves, the rule that says which rays of its cases a ray-gradient parity test may hold, util.gen_rays
in torch for the pose chain, and the registration loop of util.bake.register on the host.  What tests/test_baked_ray_grad_host.py
and tests/test_hip_baked_ray_grad.py share.  No GPU, no package import.

The march is only PIECEWISE smooth in the ray: the cell of a sample is floor(u), and a sample on a cell plane gets the one-sided
derivative of the cell its precision names -- fp32 may put u at 2.9999998 where fp64 has 3.  Neither is wrong, and the two differ
by the jump of the slope across the plane (5e-2 .. 2e-1 of the largest entry on the in-plane ray of baked_grad_ref.case_rays).  A
parity case therefore keeps a ray only if every sample of it that lies within NEAR_BOX of the box is at least PLANE_MARGIN cells
off every cell plane and every box face (`kept_rows`); fp32 rounding of u on this grid is below 2e-6 cells.

Error and bar are those of tests/position_ref.py, as in baked_grad_ref: error = max|got - ref64| / max|ref64| over the kept rows,
bar = 10 x the error of torch's fp32 autograd through the same restatement, floor 2e-6, cap 2e-4.
"""
import functools

import numpy as np
import torch

import baked_grad_ref as G
import baked_ref as B

error, bar_from, BAR_CAP = G.error, G.bar_from, G.BAR_CAP
RESO, C1, C2 = G.RESO, G.C1, G.C2
PLANE_MARGIN = 1e-5   # cells
NEAR_BOX = 1e-3       # world units: samples farther outside the box than this are outside it in every precision
MAX_DROPPED = 3       # of the 37 rays of a case
MIN_NONZERO = 27      # kept rays of a full case whose gradient row is not all zeros


def _fp32(x, dtype):
    return torch.tensor(np.array(x, np.float32)).to(dtype)


def march(rays, stored, c1, c2, step, degree=None, white_bkgd=False, occupied=None, terminate=0.0, info=None):
    """baked_grad_ref.march with `rays` a torch tensor (R,8) through which autograd runs, as `stored` is; both hold fp32-representable
    values at the dtype of `rays`.  -> rgb (R,3), depth (R,), alpha (R,).  info: a dict that receives n (R,), idx (R,nmax,3), active
    (R,nmax), u (R,nmax,3) and exists (R,nmax), detached."""
    dtype = rays.dtype
    c1t, c2t = _fp32(c1, dtype), _fp32(c2, dtype)
    reso = tuple(stored.shape[:3])
    h = torch.as_tensor(B.cell_size(c1, c2, reso, np.float64)).to(dtype)
    stepv, eps = float(np.float32(step)), float(np.float32(terminate))
    R = rays.shape[0]
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    with torch.no_grad():
        ok = torch.isfinite(rays).all(dim=1) & (near < far)
        count = torch.ceil((far - near) / torch.tensor(stepv, dtype=dtype))
        n = torch.where(ok & (count <= G.MAX_SAMPLES), count, torch.zeros_like(count)).long()
    nmax = int(n.max()) if R else 0
    i = torch.arange(nmax, dtype=dtype)
    exists = torch.arange(nmax)[None, :] < n[:, None]                                  # (R,nmax)
    t = near[:, None] + (i[None, :] + 0.5) * stepv
    p = o[:, None, :] + t[:, :, None] * d[:, None, :]                                  # (R,nmax,3)
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
    if info is not None:
        info.update(n=n, idx=idx, active=active, u=u.detach(), exists=exists, p=p.detach())

    Y = G.sh_basis(d, degree, dtype) if degree is not None else None
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
    w = torch.where(walked, a * T, torch.zeros_like(a))
    rgb = (w[..., None] * val[..., :3]).sum(dim=1)
    depth = (w * t).sum(dim=1)
    alpha = w.sum(dim=1)
    if white_bkgd:
        rgb = rgb + 1.0 - alpha[:, None]
    return rgb, depth, alpha


def loss_per_ray(out, d_rgb, d_depth, d_alpha, dtype):
    """(R,): rgb . d_rgb + depth d_depth + alpha d_alpha of each ray (each None: absent)"""
    rgb, depth, alpha = out
    L = rgb.sum(dim=1) * 0.0
    if d_rgb is not None:
        L = L + (rgb * _fp32(d_rgb, dtype)).sum(dim=1)
    if d_depth is not None:
        L = L + depth * _fp32(d_depth, dtype)
    if d_alpha is not None:
        L = L + alpha * _fp32(d_alpha, dtype)
    return L


def gradients(rays, stored, c1, c2, step, d_rgb=None, d_depth=None, d_alpha=None, dtype=torch.float64, want_stored=False, info=None, **kw):
    """-> d_rays (R,8) at `dtype` by autograd (and d_stored with want_stored) for L = the sum of loss_per_ray"""
    ray_leaf = _fp32(rays, dtype).requires_grad_(True)
    stored_leaf = _fp32(stored, dtype).requires_grad_(want_stored)
    L = loss_per_ray(march(ray_leaf, stored_leaf, c1, c2, step, info=info, **kw), d_rgb, d_depth, d_alpha, dtype).sum()
    leaves = (ray_leaf, stored_leaf) if want_stored else (ray_leaf,)
    grads = torch.autograd.grad(L, leaves, allow_unused=True)
    grads = tuple(torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves))
    return grads if want_stored else grads[0]


def kept_rows(rays, c1=C1, c2=C2, reso=RESO, step=None):
    """The rule: -> (R,) bool, True for a ray every one of whose samples within NEAR_BOX of the box lies at least PLANE_MARGIN cells
    from every cell plane and every box face (the faces are the planes u = 0 and u = n - 1).  fp64 from the fp32 inputs."""
    info = {}
    dummy = torch.zeros(tuple(reso) + (4,), dtype=torch.float64)
    march(_fp32(rays, torch.float64), dummy, c1, c2, step, info=info)
    p, u, exists = info["p"], info["u"], info["exists"]
    lo, hi = _fp32(c1, torch.float64), _fp32(c2, torch.float64)
    near_box = ((p >= lo - NEAR_BOX) & (p <= hi + NEAR_BOX)).all(dim=2) & exists
    off_plane = (u - torch.round(u)).abs().min(dim=2).values                           # cells, to the nearest plane of any axis
    bad = near_box & (off_plane < PLANE_MARGIN)
    return ~bad.any(dim=1)


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (inputs of baked_grad_ref, kept (R,) bool, the fp64 d_rays, torch's fp32 d_rays) of one case of baked_grad_ref.CASES,
    computed once (treat as read-only).  The gradients hold every row; compare on `kept`."""
    inp = G.inputs(case)
    kept = kept_rows(inp["rays"], step=inp["step"])
    args = (inp["rays"], inp["stored"], C1, C2, inp["step"], inp["d_rgb"], inp["d_depth"], inp["d_alpha"])
    return inp, kept, gradients(*args, dtype=torch.float64, **inp["kw"]), gradients(*args, dtype=torch.float32, **inp["kw"])


def hold(what, got, ref64, ref32, kept=None):
    """print HIP error, torch-fp32 error and bar on the kept rows, then hold `got` to the bar -> the bar"""
    if kept is not None:
        got, ref64, ref32 = got[kept], ref64[kept], ref32[kept]
    err, err32 = error(got.cpu(), ref64), error(ref32.double(), ref64)
    bar = bar_from(err32)
    print(f"{what}: HIP error {err:.3e}, torch-fp32 error {err32:.3e}, bar {bar:.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert err <= bar, (what, err, bar)
    return bar


# ---------------------------------------------------------------- util.gen_rays in torch, for the pose chain
def gen_rays(poses, W, H, focal, z_near, z_far, c=None):
    """poses (NV,4,4) at any dtype, through which autograd runs -> rays (NV,H,W,8), the operations of the kernels' load_ray"""
    dtype = poses.dtype
    fx = fy = float(np.float32(focal))
    cx, cy = (W * 0.5, H * 0.5) if c is None else (float(np.float32(c[0])), float(np.float32(c[1])))
    X = (torch.arange(W, dtype=dtype) - cx) / fx
    Y = (torch.arange(H, dtype=dtype) - cy) / fy
    d = torch.stack((X[None, :].expand(H, W), -Y[:, None].expand(H, W), -torch.ones((H, W), dtype=dtype)), dim=-1)
    d = d / (d * d).sum(dim=-1, keepdim=True).sqrt()
    NV = poses.shape[0]
    dirs = (poses[:, None, None, :3, :3] * d[None, :, :, None, :]).sum(dim=-1)          # (NV,H,W,3)
    origins = poses[:, None, None, :3, 3].expand(NV, H, W, 3)
    nf = torch.tensor([float(np.float32(z_near)), float(np.float32(z_far))], dtype=dtype).expand(NV, H, W, 2)
    return torch.cat((origins, dirs, nf), dim=-1)


# the views of tests/test_hip_baked_backward.py: 2 views of 5 x 4 pixels through the dense part of the common volume, n = 150
VIEWS = dict(W=5, H=4, focal=14.0, z_near=1.2, z_far=1.2 + 149.5 * 0.03, step=0.03)
VIEW_ANGLES = ((35.0, -20.0, 3.0), (190.0, -35.0, 3.2))


def pose_gradients(poses, stored, d_rgb, d_depth, d_alpha, dtype, **kw):
    """-> (d_poses (NV,4,4), d_rays (NV*H*W,8)) at `dtype` of L through gen_rays and the march, by autograd"""
    leaf = _fp32(poses, dtype).requires_grad_(True)
    v = VIEWS
    rays = gen_rays(leaf, v["W"], v["H"], v["focal"], v["z_near"], v["z_far"]).reshape(-1, 8)
    rays.retain_grad()
    L = loss_per_ray(march(rays, _fp32(stored, dtype), C1, C2, v["step"], **kw), d_rgb, d_depth, d_alpha, dtype).sum()
    L.backward()
    return leaf.grad, rays.grad


# ---------------------------------------------------------------- registration: util.bake.register on the host
REG = dict(reso=(16, 16, 16), c1=(-1.0, -1.0, -1.0), c2=(1.0, 1.0, 1.0), W=12, H=12, focal=14.0, z_near=1.5, z_far=3.9, step=0.05,
           radius=2.7, steps=120, lr=1e-2, start_deg=5.0, start_shift=0.12)
REG_CAMERAS = ((30.0, -25.0), (150.0, -40.0), (265.0, -15.0))   # (theta, phi) of testdata.synthetic.pose_spherical
# the starting error of each camera: the axis of its 5-degree rotation and the direction of its 0.12 shift
REG_AXES = ((0.3, 0.8, -0.52), (-0.6, 0.2, 0.77), (0.5, -0.7, 0.5))
REG_SHIFTS = ((0.6, -0.64, 0.48), (-0.36, 0.8, 0.48), (0.0, 0.6, -0.8))
# centre, width and colour of the three Gaussian blobs
REG_BLOBS = (((0.55, 0.2, -0.4), 0.22, (0.9, 0.2, 0.1)), ((-0.5, 0.45, 0.45), 0.2, (0.1, 0.8, 0.2)), ((-0.1, -0.6, -0.05), 0.21, (0.15, 0.25, 0.95)))


def rodrigues(w):
    """util.bake.rodrigues, restated"""
    t2 = (w * w).sum(dim=-1)
    small = t2 < 1e-6
    safe = torch.where(small, torch.ones_like(t2), t2)
    t = safe.sqrt()
    A = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, t.sin() / t)
    Bc = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, (1.0 - t.cos()) / safe)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    o = torch.zeros_like(x)
    K = torch.stack((torch.stack((o, -z, y), dim=-1), torch.stack((z, o, -x), dim=-1), torch.stack((-y, x, o), dim=-1)), dim=-2)
    return torch.eye(3, dtype=w.dtype).expand(K.shape) + A[..., None, None] * K + Bc[..., None, None] * (K @ K)


def moved_poses(poses0, w, v):
    top = torch.cat((rodrigues(w) @ poses0[:, :3, :3], (poses0[:, :3, 3] + v)[:, :, None]), dim=2)
    return torch.cat((top, poses0[:, 3:, :]), dim=1)


@functools.lru_cache(maxsize=None)
def reg_scene(degree=None):
    """-> (stored fp32 (16,16,16,4) or (16,16,16,4,4) at degree 1, true poses (3,4,4), start poses (3,4,4)) as numpy arrays (treat as
    read-only): three coloured Gaussian blobs on [-1,1]^3 -- at degree 1 the DC part is those blobs and the linear part tints each
    side --, three cameras at radius 2.7 looking at the origin, and starts 5 degrees and 0.12 off them"""
    from testdata import synthetic
    ax = [np.linspace(lo, hi, n) for lo, hi, n in zip(REG["c1"], REG["c2"], REG["reso"])]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    sigma, colour = np.zeros(REG["reso"]), np.zeros(REG["reso"] + (3,))
    for centre, width, rgb in REG_BLOBS:
        g = np.exp(-((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) / (2.0 * width * width))
        sigma += 14.0 * g
        colour += g[..., None] * np.asarray(rgb)
    colour = colour / np.maximum(colour.sum(axis=-1, keepdims=True) / 1.2, 1e-6)
    vol = np.concatenate((np.clip(colour, 0.0, 1.0), sigma[..., None]), axis=-1).astype(np.float32)
    if degree is not None:
        assert degree == 1
        coef = np.zeros(REG["reso"] + (4, 4), np.float32)
        coef[..., 0, :] = vol
        coef[..., 1, :3] = 0.08 * vol[..., :3]            # Y_1 = sqrt 3 y, Y_2 = sqrt 3 z, Y_3 = sqrt 3 x
        coef[..., 2, :3] = -0.06 * vol[..., :3]
        coef[..., 3, :3] = 0.05 * vol[..., :3]
        coef[..., 1:, 3] = 0.04 * vol[..., 3:4] * np.array([1.0, -1.0, 0.5])
        vol = coef
    true = np.stack([synthetic.pose_spherical(th, ph, REG["radius"]).numpy() for th, ph in REG_CAMERAS]).astype(np.float32)
    w = np.stack([np.asarray(a) / np.linalg.norm(a) * np.deg2rad(REG["start_deg"]) for a in REG_AXES])
    shift = np.stack([np.asarray(s) / np.linalg.norm(s) * REG["start_shift"] for s in REG_SHIFTS])
    start = moved_poses(torch.from_numpy(true).double(), torch.from_numpy(w), torch.from_numpy(shift)).float().numpy()
    out = (np.ascontiguousarray(vol), true, np.ascontiguousarray(start))
    for a in out:
        a.setflags(write=False)
    return out


def pose_errors(poses, true):
    """-> (rotation error in degrees (NV,), translation error (NV,)) of poses against true, both (NV,4,4) tensors"""
    poses, true = poses.double().cpu(), true.double().cpu()
    rel = poses[:, :3, :3] @ true[:, :3, :3].transpose(1, 2)
    cos = ((rel[:, 0, 0] + rel[:, 1, 1] + rel[:, 2, 2]) - 1.0) / 2.0
    return torch.rad2deg(torch.acos(cos.clamp(-1.0, 1.0))), (poses[:, :3, 3] - true[:, :3, 3]).norm(dim=1)


@functools.lru_cache(maxsize=None)
def register_ref(dtype=torch.float32, degree=None):
    """util.bake.register through the restatement at `dtype` on the CPU: the target is the restatement's render of the true poses,
    the optimiser torch.optim.Adam with register's settings on (w, v) from zero -> (poses (3,4,4), losses), computed once"""
    stored, true, start = reg_scene(degree)
    r = REG
    stored_t = _fp32(stored, dtype)
    render = lambda poses: march(gen_rays(poses, r["W"], r["H"], r["focal"], r["z_near"], r["z_far"]).reshape(-1, 8), stored_t, r["c1"],
                                 r["c2"], r["step"], degree=degree, white_bkgd=True)[0]
    with torch.no_grad():
        target = render(_fp32(true, dtype))
    poses0 = _fp32(start, dtype)
    w = torch.zeros((3, 3), dtype=dtype, requires_grad=True)
    v = torch.zeros((3, 3), dtype=dtype, requires_grad=True)
    optimiser = torch.optim.Adam([w, v], lr=r["lr"])
    losses = []
    for _ in range(r["steps"]):
        loss = ((render(moved_poses(poses0, w, v)) - target) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        loss.backward()
        optimiser.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        return moved_poses(poses0, w, v), losses
