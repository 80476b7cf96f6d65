"""
Baked volume of one encoded object: the network evaluated ONCE on the points of a grid, for colour as well as density, and any number
of views ray-marched from the grid alone (pnr_baked_render_rays / pnr_baked_render_views, include/pixelnerf_hip.h "baked volumes").
The reference has no counterpart: every pixel it renders pays for 64 + 128 evaluations of the network.  For previews, orbit videos
(eval/gen_video.py's use), picking cameras and sanity checks during training.

The image is an APPROXIMATION of the network's render: trilinear in space, one view direction per grid point, equidistant samples
(no importance sampling).  It is separate from NeRFRenderer: nothing there changes.  After a weight update, bake again (from_model).
BakedSHVolume lifts the one-direction limit: it keeps real spherical harmonics up to degree 2 of all four channels at every grid
point (n_dirs network passes to bake, 4 or 9 times the memory) and the march evaluates them for each ray's own direction
(pnr_baked_sh_render_rays / pnr_baked_sh_render_views); the other limits stay.
SparseBakedVolume keeps only the rows of the grid points that the occupied cells of an OccupancyGrid read, renders the bytes of the
dense march with the same bits (pnr_baked_sparse_render_rays / pnr_baked_sparse_render_views) and is baked without touching the
other points: less to bake and to store, not a faster march (profiles/baked_notes.md).
All three store fp32 or fp16 (`half()`, `from_model(dtype=torch.float16)`, `to_half`): fp16 is storage only, the march is fp32 on the
widened values, and a half volume renders the BYTES of its `float()` (pnr_baked_half_render_* / pnr_baked_sparse_half_render_*).
BakedScene places up to 8 volumes of one kind in one world by rigid poses and marches them together (pnr_baked_scene_render_*).

The grid is the one util.recon.marching_cubes and util.occupancy.OccupancyGrid use (points of ops.gen_grid_points, cells of the TRUE
spacing (c2 - c1) / (reso - 1)); the skip grid of a volume is an OccupancyGrid of its sigma channel with dilate 0.
"""
import warnings

import torch

from .dotmap import DotMap
from .occupancy import OccupancyGrid, _check_geometry


HALF_MAX = 65504.0  # the largest finite fp16 number


def to_half(t):
    """How a baked volume is rounded to fp16 storage: t, a floating-point tensor on any device (CPU too), -> torch.float16, every
    value rounded to nearest even; a finite value beyond +-65504 SATURATES at +-65504, so nothing is ever stored as infinity (a
    stored infinity would put inf - inf into the trilinear blend), and a `warnings.warn` names how many did.  A NaN or an infinity
    in `t` raises ValueError.  A value v with |v| <= 65504 moves by at most max(2^-11 |v|, 2^-25).  An fp16 tensor is returned
    as it is."""
    if not isinstance(t, torch.Tensor) or not t.is_floating_point():
        raise TypeError("to_half: expected a floating-point torch.Tensor")
    t = t.detach()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("to_half: the tensor holds a non-finite value")
    if t.dtype == torch.float16:
        return t
    saturated = int((t.abs() > HALF_MAX).sum())
    if saturated:
        warnings.warn(f"to_half: {saturated} value{'s' if saturated != 1 else ''} beyond +-65504 saturated at +-65504")
    return t.clamp(-HALF_MAX, HALF_MAX).to(torch.float16)


def _storage_dtype(what, dtype):
    if dtype not in (torch.float32, torch.float16):
        raise ValueError(f"{what}: dtype must be torch.float32 or torch.float16, got {dtype}")
    return dtype


def _bake(what, net, c1, c2, reso, dtype, coarse, eval_batch_size, sparse=False, occupancy=None, degree=None, n_dirs=32,
          viewdirs="origin"):
    """The bake loop of the three from_model methods.  Points: every grid point in ascending order (ops.gen_grid_points), or with
    `sparse` the kept points of `occupancy` alone (ops.sparse_points, ops.gen_grid_points_at).  Mode: degree None -- all four output
    columns of ONE pass with `viewdirs` -- or degree 0, 1, 2 -- n_dirs passes projected onto the basis in fp32, the product then the
    sum, in the order of m.  Even chunks, eval mode with the train flag restored, `to_half` at the end for dtype=torch.float16.
    -> (stored (P or M,4) or (P or M,B,4), (reso, c1, c2) as checked, (index, ids) or None)"""
    from .. import ops
    _storage_dtype(what, dtype)
    if int(getattr(net, "num_objs", 1) or 1) > 1:
        raise ValueError(f"{what}: the network encoded {int(net.num_objs)} objects; encode one object")
    reso, c1, c2, _ = _check_geometry(reso, c1, c2, 0)
    if sparse:
        _same_grid(what, occupancy, reso, c1, c2)
    use_viewdirs = bool(getattr(net, "use_viewdirs", False))
    origin, const_dir, dirs, P = True, None, None, None
    if degree is None:
        origin = isinstance(viewdirs, str)
        if origin and viewdirs != "origin":
            raise ValueError(f"{what}: viewdirs must be 'origin' or a 3-vector, got {viewdirs!r}")
    else:
        degree = int(degree)
        P = BakedSHVolume.projection(n_dirs, degree)  # (the degree and n_dirs checks)
        if not use_viewdirs and degree > 0:
            warnings.warn(f"{what}: the network takes no view directions; baking at degree 0")
            degree = 0
    device = next(net.parameters()).device
    if sparse and occupancy.bits.device != device:
        raise ValueError(f"{what}: the occupancy grid lives on {occupancy.bits.device}, the network on {device}")
    if degree is None:
        if not origin:
            const_dir = torch.as_tensor(viewdirs, dtype=torch.float32).flatten()
            if const_dir.numel() != 3 or not bool(torch.isfinite(const_dir).all()) or float(const_dir.norm()) == 0.0:
                raise ValueError(f"{what}: a constant view direction must be a finite non-zero 3-vector")
            const_dir = (const_dir / const_dir.norm()).to(device)
        if use_viewdirs and origin:
            warnings.warn("Running marching cubes with fake view dirs (pointing to origin), output may be invalid")
    elif use_viewdirs:
        dirs, P = BakedSHVolume.directions(n_dirs).to(device), P.float().to(device)
    else:
        P = torch.ones((1, 1), device=device)  # one pass: its output is the DC part
    nb = None if degree is None else (degree + 1) ** 2
    if coarse is None:
        coarse = getattr(net, "mlp_fine", None) is None
    chunk = max(2, int(eval_batch_size) // 2 * 2)
    kept = ops.sparse_points(occupancy.bits, reso) if sparse else None
    total = reso[0] * reso[1] * reso[2] if kept is None else kept[1].shape[0]
    is_train = bool(getattr(net, "training", False))
    if hasattr(net, "eval"):
        net.eval()
    try:
        with torch.no_grad():
            if degree is None:
                stored = torch.empty((total, 4), dtype=torch.float32, device=device)
            else:
                stored = torch.zeros((total, nb, 4), dtype=torch.float32, device=device)
            for first in range(0, total, chunk):
                count = min(chunk, total - first)
                fake_dirs = degree is None and use_viewdirs and origin
                if kept is None:
                    pnts, vd = ops.gen_grid_points(c1, c2, reso, first, count, device=device, viewdirs=fake_dirs)
                else:
                    pnts, vd = ops.gen_grid_points_at(c1, c2, reso, kept[1][first:first + count], viewdirs=fake_dirs)
                if degree is None:
                    if use_viewdirs and not origin:
                        vd = const_dir.expand(count, 3).contiguous()
                    out = net(pnts[None], coarse=bool(coarse), viewdirs=vd[None] if use_viewdirs else None)
                    stored[first:first + count] = out.reshape(count, -1)[:, :4]
                    continue
                part = stored[first:first + count]
                for m in range(P.shape[1]):
                    vd = dirs[m].expand(count, 3).contiguous()[None] if use_viewdirs else None
                    out = net(pnts[None], coarse=bool(coarse), viewdirs=vd).reshape(count, -1)[:, :4]
                    part += out[:, None, :] * P[:nb, m][None, :, None]  # the product, then the sum: two roundings, in the order of m
    finally:
        if is_train:
            net.train()
    if dtype == torch.float16:
        stored = to_half(stored)
    return stored, (reso, c1, c2), kept


def _tv_weights(what, degree, rgb, sigma, sh):
    """the per-element weights of ops.baked_tv: (rgb, rgb, rgb, sigma) for the RGBA row or the DC basis row, and `sh` -- one number
    for every channel, None = the DC weights -- for the basis rows k >= 1"""
    import math
    rgb, sigma = float(rgb), float(sigma)
    dc = [rgb, rgb, rgb, sigma]
    higher = dc if sh is None else [float(sh)] * 4
    weights = dc + higher * (0 if degree is None else (int(degree) + 1) ** 2 - 1)
    if not all(math.isfinite(w) and w >= 0.0 for w in weights):
        raise ValueError(f"{what}: the weights rgb, sigma and sh must be finite and >= 0, got {rgb}, {sigma}, {sh}")
    return weights


def _flat_rays(what, rays):
    """rays (...,8), checked -> (the rays as (R,8) fp32, the leading shape the outputs take back)"""
    if not isinstance(rays, torch.Tensor) or rays.dim() < 1 or rays.shape[-1] != 8:
        raise ValueError(f"{what}: rays must be (...,8)")
    return rays.reshape(-1, 8).float(), tuple(rays.shape[:-1])


def _ray_result(rgb, depth, alpha, lead):
    return DotMap(rgb=rgb.reshape(*lead, 3), depth=depth.reshape(lead), alpha=alpha.reshape(lead))


def _camera_args(what, poses_c2w, W, H, focal, c, gt_rgb):
    """the camera of a render_views call, checked -> (W, H, focal, c) as the ops functions take them"""
    if not isinstance(poses_c2w, torch.Tensor) or poses_c2w.dim() != 3 or tuple(poses_c2w.shape[1:]) != (4, 4):
        raise ValueError(f"{what}: poses_c2w must be (NVt,4,4)")
    W, H, NVt = int(W), int(H), poses_c2w.shape[0]
    if torch.is_tensor(focal):
        focal = focal.flatten().tolist()
        focal = focal[0] if len(focal) == 1 else (focal[0], focal[1])
    if torch.is_tensor(c):
        c = c.flatten().tolist()
    if gt_rgb is not None and tuple(gt_rgb.shape) != (NVt, H, W, 3):
        raise ValueError(f"{what}: gt_rgb must be (NVt,H,W,3) = {(NVt, H, W, 3)}, got {tuple(gt_rgb.shape)}")
    return W, H, focal, c


def _views_result(rgb, depth, alpha, NVt, W, H, z_near, z_far, gt_rgb, want_u8):
    """the outputs of a march over NVt views through NeRFRenderer.render_views' epilogue (ops.eval_epilogue) -> the DotMap of
    render_views"""
    from .. import ops
    gt = None if gt_rgb is None else gt_rgb.reshape(NVt, H * W, 3).float()
    ep = ops.eval_epilogue(rgb.reshape(NVt, H * W, 3), depth.reshape(NVt, H * W), z_near, z_far, gt_rgb=gt, want_u8=want_u8,
                           image_shape=(H, W) if gt is not None else None)
    ret = DotMap(rgb=rgb.reshape(NVt, H, W, 3), depth=depth.reshape(NVt, H, W), alpha=alpha.reshape(NVt, H, W),
                 depth_norm=ep["depth_norm"].reshape(NVt, H, W))
    if want_u8:
        ret.rgb_u8 = ep["rgb_u8"].reshape(NVt, H, W, 3)
    if gt is not None:
        ret.psnr, ret.ssim = ep["psnr"], ep["ssim"]
    return ret


def _check_field(what, name, field, shape, nullable=False):
    """a visibility field (or the `out` of one): a contiguous fp32 tensor of `shape`; checked before any device work"""
    if field is None and nullable:
        return
    if not isinstance(field, torch.Tensor) or field.dtype != torch.float32 or tuple(field.shape) != tuple(shape) \
            or not field.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous float32 tensor of shape {tuple(shape)}, got "
                         f"{(tuple(field.shape), field.dtype) if isinstance(field, torch.Tensor) else type(field).__name__}")


def _resample_reso(what, reso):
    """an int or three ints, each >= 2 -> (nx, ny, nz)"""
    import numbers
    reso = (reso,) * 3 if isinstance(reso, numbers.Integral) and not isinstance(reso, bool) else reso
    try:
        reso = tuple(reso)
    except TypeError:
        raise ValueError(f"{what}: reso must be an int or three ints, got {reso!r}") from None
    if len(reso) != 3 or not all(isinstance(r, numbers.Integral) and not isinstance(r, bool) for r in reso):
        raise ValueError(f"{what}: reso must be an int or three ints, got {reso!r}")
    reso = tuple(int(r) for r in reso)
    if any(r < 2 for r in reso) or reso[0] * reso[1] * reso[2] >= 2 ** 31:
        raise ValueError(f"{what}: every axis needs at least 2 grid points and the grid fewer than 2^31, got reso {reso}")
    return reso


def _sparse_refinement(what, reso, new):
    """the integer factors m_a with n'_a - 1 == m_a (n_a - 1), or ValueError: a sparse volume keeps whole cells, and only an integer
    refinement maps every new cell into ONE old cell"""
    if any((b - 1) % (a - 1) for a, b in zip(reso, new)):
        raise ValueError(f"{what}: a sparse volume takes integer refinements only (n' - 1 == m (n - 1) on every axis), got {tuple(reso)} -> "
                         f"{tuple(new)}; resample the dense volume and prune again")
    return tuple((b - 1) // (a - 1) for a, b in zip(reso, new))


def _cells_of(bits, reso):
    """the bitfield of ops.occupancy_build as a (nx-1,ny-1,nz-1) bool tensor"""
    shape = tuple(r - 1 for r in reso)
    shifts = torch.arange(32, device=bits.device)
    flat = ((bits.long()[:, None] >> shifts) & 1).bool().flatten()
    return flat[:shape[0] * shape[1] * shape[2]].view(shape)


def _bits_of(cells):
    """a bool tensor of cells as the bitfield of ops.occupancy_build: cell index i is bit (i & 31) of int32 word (i >> 5)"""
    flat = cells.flatten()
    words = (flat.numel() + 31) // 32
    padded = torch.zeros((words * 32,), dtype=torch.int64, device=flat.device)
    padded[:flat.numel()] = flat
    value = (padded.view(words, 32) << torch.arange(32, device=flat.device)).sum(dim=1)
    return torch.where(value >= 2 ** 31, value - 2 ** 32, value).to(torch.int32)


def _count_bits(bits):
    """the number of bits set, as the 0-d int32 device tensor an OccupancyGrid carries"""
    table = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int32, device=bits.device)
    return table[bits.contiguous().view(torch.uint8).long()].sum().to(torch.int32)


def _check_stages(what, stages):
    """stages of fit_coarse_to_fine: a non-empty sequence of (reso | None, steps) -> [(reso (nx,ny,nz) | None, steps)]"""
    import numbers
    try:
        stages = list(stages)
    except TypeError:
        raise ValueError(f"{what}: stages must be a sequence of (reso | None, steps)") from None
    if not stages:
        raise ValueError(f"{what}: stages must hold at least one (reso | None, steps)")
    out = []
    for k, stage in enumerate(stages):
        if not isinstance(stage, (tuple, list)) or len(stage) != 2:
            raise ValueError(f"{what}: stage {k} must be (reso | None, steps), got {stage!r}")
        reso, steps = stage
        if not isinstance(steps, numbers.Integral) or isinstance(steps, bool) or steps < 0:
            raise ValueError(f"{what}: stage {k}: steps must be an int >= 0, got {steps!r}")
        out.append((None if reso is None else _resample_reso(f"{what}: stage {k}", reso), int(steps)))
    return out


class _Baked:
    """what BakedVolume, BakedSHVolume and SparseBakedVolume share: the march through `self.occupancy` on the grid (reso, c1, c2) and
    the storage methods.  A subclass names the tensor it stores (`_stored_name`: the attribute, and the key of its state) and has a
    `degree` when its march is the view-dependent one.
    Storage is fp32 or fp16 (`dtype`); the march is fp32 either way: a half volume renders the BYTES its `float()` renders
    (include/pixelnerf_hip.h, "Half-precision baked volumes")."""

    _stored_name = None  # "vol", "coef" or "rows"
    degree = None        # None: the RGBA march

    def _stored(self):
        return getattr(self, self._stored_name)

    def _around(self, stored):
        """this volume around another stored tensor"""
        return type(self)(stored, self.c1, self.c2, self.skip_threshold)

    def half(self):
        """this volume with `to_half` of its stored tensor (a sparse volume shares index, ids and occupancy); a half volume is
        returned as it is"""
        return self if self.dtype == torch.float16 else self._around(to_half(self._stored()))

    def float(self):
        """this volume widened to fp32 (exact; a sparse volume shares index, ids and occupancy); an fp32 volume is returned as it is"""
        return self if self.dtype == torch.float32 else self._around(self._stored().float())

    def trainable(self):
        """-> TrainableBaked: an nn.Module whose one nn.Parameter is a copy of this volume's fp32 stored tensor; `forward(rays, ...)`
        and `forward_views(...)` render with gradients attached, `.volume()` gives the fitted volume back (`fit` is the loop around
        it).  An fp16 volume is refused: fit in fp32 and call `half()` afterwards."""
        return TrainableBaked(self)

    def tv(self, rgb=1.0, sigma=1.0, sh=None, eps=1e-8):
        """the total variation of the stored values as a float (ops.baked_tv's fp32 value, under no_grad): what
        `trainable().tv(...)` returns with gradients attached; the weights are explained there.  An fp16 volume is refused."""
        from .. import ops
        name = type(self).__name__
        if self.dtype != torch.float32:
            raise TypeError(f"{name}.tv: {_FP32_ONLY}")
        with torch.no_grad():
            value32, _ = ops.baked_tv(self._stored(), self.degree, self.reso, _tv_weights(f"{name}.tv", self.degree, rgb, sigma, sh),
                                      eps=eps, index=self._index, ids=self._ids)
        return float(value32)

    def state_dict(self):
        """the stored tensor under its name (a degree follows from its shape), the geometry and the skip threshold; the skip grid is
        rebuilt on load"""
        return {self._stored_name: self._stored(), "c1": torch.tensor(self.c1, dtype=torch.float64),
                "c2": torch.tensor(self.c2, dtype=torch.float64), "skip_threshold": torch.tensor(self.skip_threshold, dtype=torch.float64)}

    @classmethod
    def from_state_dict(cls, state, device=None):
        """:param device where to put the volume; None: where the stored tensor lives"""
        stored = state[cls._stored_name] if device is None else state[cls._stored_name].to(device)
        return cls(stored, state["c1"].tolist(), state["c2"].tolist(), float(state["skip_threshold"]))

    _index = _ids = None  # what the ops functions take as index and ids: a SparseBakedVolume's, None for a dense volume

    def _march(self, source, step, bits, white_bkgd, terminate):
        """source: (rays (R,8),), or the camera (poses, W, H, focal, c, z_near, z_far); ops.baked_march picks the function from the
        stored dtype, the degree and whether the volume is sparse"""
        from .. import ops
        return ops.baked_march(source, self._stored(), self.degree, self.reso, self.c1, self.c2, step, bits=bits, index=self._index,
                               white_bkgd=white_bkgd, terminate=terminate)

    @property
    def dtype(self):
        return self._stored().dtype

    @property
    def nbytes(self):
        """the bytes of the stored values"""
        return self._stored().numel() * self._stored().element_size()

    @property
    def cell_size(self):
        return tuple((hi - lo) / (n - 1) for lo, hi, n in zip(self.c1, self.c2, self.reso))

    def _march_args(self, step, terminate, skip):
        step = min(self.cell_size) if step is None else float(step)
        return step, (0.0 if terminate is None else float(terminate)), (self.occupancy.bits if skip else None)

    def render(self, rays, step=None, white_bkgd=False, terminate=None, skip=True):
        """rays (...,8) on the volume's device -> DotMap(rgb (...,3), depth (...), alpha (...)); ops.baked_render /
        ops.baked_sh_render.
        :param step the sample distance in the units of z; None: the smallest cell edge
        :param terminate eps in [0, 1): a ray stops once its transmittance, checked every 64 samples, is <= eps (every channel and
        alpha move by at most eps, depth by at most eps far); None / 0: off
        :param skip march against the skip grid (exact at skip_threshold 0)"""
        flat, lead = _flat_rays(f"{type(self).__name__}.render", rays)
        step, terminate, bits = self._march_args(step, terminate, skip)
        with torch.no_grad():
            return _ray_result(*self._march((flat,), step, bits, white_bkgd, terminate), lead)

    def render_views(self, poses_c2w, W, H, focal, z_near, z_far, c=None, gt_rgb=None, want_u8=False, step=None, white_bkgd=False,
                     terminate=None, skip=True):
        """Every pixel of the target views from their cameras, with NeRFRenderer.render_views' epilogue on the device: poses_c2w
        (NVt,4,4) camera-to-world, focal a scalar or (fx, fy), c (cx, cy) or None = the image centre; step, terminate, skip as
        render.  The rays are regenerated in the kernel: the same bits as render(util.gen_rays(...)), no ray array.
        :return DotMap: rgb (NVt,H,W,3), depth and alpha (NVt,H,W), unclamped; depth_norm = (depth - z_near) / (z_far - z_near);
        rgb_u8 with want_u8; with gt_rgb (NVt,H,W,3) in [0,1] psnr and ssim (NVt,) float64 of clamp(rgb, 0, 1)"""
        W, H, focal, c = _camera_args(f"{type(self).__name__}.render_views", poses_c2w, W, H, focal, c, gt_rgb)
        step, terminate, bits = self._march_args(step, terminate, skip)
        with torch.no_grad():
            rgb, depth, alpha = self._march((poses_c2w.float(), W, H, focal, c, z_near, z_far), step, bits, white_bkgd, terminate)
            return _views_result(rgb, depth, alpha, poses_c2w.shape[0], W, H, z_near, z_far, gt_rgb, want_u8)

    def _march_diff(self, source, step, bits, white_bkgd, terminate):
        from .. import autograd
        return autograd.baked_march_rays_autograd(self._stored(), source, self.degree, self.reso, self.c1, self.c2, step, bits=bits,
                                                  index=self._index, white_bkgd=white_bkgd, terminate=terminate)

    def render_diff(self, rays, step=None, white_bkgd=False, terminate=None, skip=True):
        """`render` with autograd to the RAYS: rays (...,8) -> DotMap(rgb (...,3), depth (...), alpha (...)), the bytes `render` gives,
        and a backward that hands dL/d rays to whatever made them (pnr_baked_ray_backward_rays: no atomics, the same bytes on every
        call; include/pixelnerf_hip.h, "Gradients of the baked march with respect to the RAYS").  The volume itself gets no gradient
        (`trainable()` is for that) and may be fp16.  step, terminate, skip: as render."""
        flat, lead = _flat_rays(f"{type(self).__name__}.render_diff", rays)
        step, terminate, bits = self._march_args(step, terminate, skip)
        return _ray_result(*self._march_diff((flat,), step, bits, white_bkgd, terminate), lead)

    def render_views_diff(self, poses_c2w, W, H, focal, z_near, z_far, c=None, step=None, white_bkgd=False, terminate=None, skip=True):
        """`render_views` without its epilogue and with autograd to the POSES: poses_c2w (NVt,4,4) -> DotMap(rgb (NVt,H,W,3), depth
        and alpha (NVt,H,W)), the bytes `render_views` gives; the backward is pnr_baked_ray_backward_views followed by
        ops.gen_rays_backward (the intrinsics are constants).  What `register` descends on."""
        W, H, focal, c = _camera_args(f"{type(self).__name__}.render_views_diff", poses_c2w, W, H, focal, c, None)
        NVt = poses_c2w.shape[0]
        step, terminate, bits = self._march_args(step, terminate, skip)
        rgb, depth, alpha = self._march_diff((poses_c2w.float(), W, H, focal, c, z_near, z_far), step, bits, white_bkgd, terminate)
        return DotMap(rgb=rgb.reshape(NVt, H, W, 3), depth=depth.reshape(NVt, H, W), alpha=alpha.reshape(NVt, H, W))

    # ---- coarse to fine: what the rays see, pruning by it, and the volume on another grid

    def _vis_shape(self):
        return (self._stored().shape[0],) if self._stored_name == "rows" else tuple(self.reso)

    def _visibility(self, what, source, step, terminate, skip, out):
        from .. import ops
        _check_field(what, "out", out, self._vis_shape(), nullable=True)
        step, terminate, bits = self._march_args(step, terminate, skip)
        kw = dict(bits=bits, index=self._index, terminate=terminate, out=out)
        with torch.no_grad():
            if len(source) == 1:
                return ops.baked_visibility(source[0], self._stored(), self.degree, self.reso, self.c1, self.c2, step, **kw)
            poses, W, H, focal, c, z_near, z_far = source
            return ops.baked_visibility_views(poses, W, H, focal, c, z_near, z_far, self._stored(), self.degree, self.reso, self.c1,
                                              self.c2, step, **kw)

    def visibility(self, rays, step=None, terminate=None, skip=True, out=None):
        """Which stored values the rays SEE (ops.baked_visibility): rays (...,8) -> fp32 (nx,ny,nz) for a dense volume, (M,) -- one
        number per kept row -- for a sparse one: the largest compositing weight x trilinear corner weight any sample of any ray gave
        the point, with exactly the samples and weights of `render(rays, step, terminate=, skip=)`.  0: no ray constrains the point.
        :param out a field of that shape from an earlier call: the result is max-accumulated into it and returned (batches, views)
        The same bytes on every call, whatever the order of the rays and however they are split into calls."""
        name = f"{type(self).__name__}.visibility"
        return self._visibility(name, (_flat_rays(name, rays)[0].detach(),), step, terminate, skip, out)

    def visibility_views(self, poses_c2w, W, H, focal, z_near, z_far, c=None, step=None, terminate=None, skip=True, out=None):
        """`visibility` over every pixel of the views (ops.baked_visibility_views): the rays are regenerated in the kernel -- the bytes
        of visibility(util.gen_rays(...)), no ray array.  poses_c2w, W, H, focal, z_near, z_far, c: as render_views."""
        name = f"{type(self).__name__}.visibility_views"
        W, H, focal, c = _camera_args(name, poses_c2w, W, H, focal, c, None)
        return self._visibility(name, (poses_c2w.detach().float(), W, H, focal, c, z_near, z_far), step, terminate, skip, out)

    def resample(self, reso):
        """This volume on another point count over the SAME box (ops.baked_resample): reso an int or (nx,ny,nz).  Trilinear in the
        stored values (a view-dependent volume: in its coefficients), exact index arithmetic: the same reso gives the same values,
        a refinement n' - 1 = m (n - 1) keeps every old point bit for bit.  -> a new volume of this class: a dense one with this
        skip_threshold and its skip grid rebuilt from the new sigma; a half one is the fp32 result through `to_half` (the one
        rounding path); a SparseBakedVolume takes integer refinements only (ValueError otherwise, before any device work): a cell
        of the new occupancy grid is occupied iff its parent cell was, and the dense tensor is never formed.  No autograd."""
        from .. import ops
        name = f"{type(self).__name__}.resample"
        reso = _resample_reso(name, reso)
        half = self.dtype == torch.float16
        if self._stored_name != "rows":
            out = ops.baked_resample(self._stored(), self.degree, self.reso, reso)
            return self._around(to_half(out) if half else out)
        m = _sparse_refinement(name, self.reso, reso)
        old = self.occupancy
        cells = _cells_of(old.bits, old.reso)
        for axis in range(3):
            cells = cells.repeat_interleave(m[axis], dim=axis)
        occupancy = OccupancyGrid(_bits_of(cells), reso, self.c1, self.c2, old.threshold, old.dilate,
                                  (old.n_occupied * (m[0] * m[1] * m[2])).to(torch.int32))
        index, ids = ops.sparse_points(occupancy.bits, reso)
        rows = ops.baked_resample(self.rows, self.degree, self.reso, reso, index=self.index, ids_dst=ids)
        return SparseBakedVolume(to_half(rows) if half else rows, occupancy, index=index, ids=ids)

    def prune(self, visibility, threshold, dilate=1):
        """Keep what the rays see: `visibility` the field of `visibility(...)` on this volume -- (nx,ny,nz), or (M,) of a sparse one --,
        -> the SparseBakedVolume of the cells within `dilate` cells of a cell with a corner whose visibility is > threshold
        (OccupancyGrid.from_density of the field), ANDed with this volume's own occupancy bits: pruning never adds a cell.  The
        result renders the bytes of this volume's `render(skip=True)` on every ray whose samples all lie in kept cells."""
        from .. import ops
        name = f"{type(self).__name__}.prune"
        _check_field(name, "visibility", visibility, self._vis_shape())
        sparse = self._stored_name == "rows"
        field = visibility.detach()
        if sparse:
            dense = torch.zeros((self.reso[0] * self.reso[1] * self.reso[2],), dtype=torch.float32, device=field.device)
            dense.index_copy_(0, self.ids.long(), field)
            field = dense.view(*self.reso)
        seen = OccupancyGrid.from_density(field.contiguous(), self.c1, self.c2, threshold, dilate=dilate)
        bits = (seen.bits & self.occupancy.bits).contiguous()
        occupancy = OccupancyGrid(bits, self.reso, self.c1, self.c2, threshold, dilate, _count_bits(bits))
        if not sparse:
            return self.sparse(occupancy)
        index, ids = ops.sparse_points(bits, self.reso)  # a subset of this volume's kept points: fewer cells, the same closure
        ranks = self.index.view(-1).index_select(0, ids.long())
        return SparseBakedVolume(self.rows.index_select(0, ranks.long()), occupancy, index=index, ids=ids)


class BakedVolume(_Baked):
    """vol: (nx,ny,nz,4) fp32 or fp16 on the device, (r, g, b, sigma) at the points of ops.gen_grid_points(c1, c2, reso) -- the network's
    outputs (rgb after the sigmoid, sigma after the relu); reso, c1, c2: the grid; skip_threshold and occupancy: the
    OccupancyGrid (dilate 0) of vol[..., 3] that `render(skip=True)` marches against -- at threshold 0 the skipped render equals the
    unskipped one bit for bit, above 0 the image changes where the dropped haze was visible (OccupancyGrid's contract).
    An fp16 volume (`half()`, `from_model(dtype=torch.float16)`, or a caller's fp16 tensor) renders the bytes of its `float()`; its
    skip grid is built from the widened sigma, so skipping stays exact (a sigma below 2^-25 has rounded to 0)."""

    _stored_name = "vol"

    def __init__(self, vol, c1, c2, skip_threshold=0.0, keep_largest=None, min_voxels=None):
        from .. import _lib
        if not isinstance(vol, torch.Tensor) or vol.dim() != 4 or vol.shape[3] != 4 or vol.dtype not in (torch.float32, torch.float16):
            raise ValueError("BakedVolume: vol must be a (nx,ny,nz,4) float32 or float16 tensor")
        reso, c1, c2, _ = _check_geometry(vol.shape[:3], c1, c2, 0)  # (before any device work)
        skip_threshold = float(skip_threshold)
        if skip_threshold != skip_threshold:
            raise ValueError("BakedVolume: skip_threshold is NaN")
        if not vol.is_cuda:
            raise _lib.PixelNerfHipError(f"BakedVolume: vol must live on a HIP device (got {vol.device}); pixelnerf_amd has no CPU path")
        vol = vol.detach().contiguous()
        if not bool(torch.isfinite(vol).all()):
            raise ValueError("BakedVolume: the volume holds a non-finite value")
        self.vol, self.reso, self.c1, self.c2, self.skip_threshold = vol, reso, c1, c2, skip_threshold
        self.occupancy = OccupancyGrid.from_density(vol[..., 3].float().contiguous(), c1, c2, skip_threshold, dilate=0,
                                                    keep_largest=keep_largest, min_voxels=min_voxels)

    @classmethod
    def from_tensor(cls, vol, c1, c2, skip_threshold=0.0):
        """wrap a caller-made volume: vol (nx,ny,nz,4) fp32 or fp16 HIP tensor spanning [c1, c2]"""
        return cls(vol, c1, c2, skip_threshold)

    @classmethod
    def from_model(cls, net, c1, c2, reso, coarse=None, viewdirs="origin", eval_batch_size=100000, skip_threshold=0.0,
                   keep_largest=None, min_voxels=None, dtype=torch.float32):
        """Bake ONE encoded object (checked as util.recon.density_grid checks it): every chunk of grid points goes through
        `net(xyz (1,N,3), coarse=, viewdirs=)` under torch.no_grad() in eval mode (the train / eval flag is restored) and all four
        output columns are written into the volume.
        :param coarse which network; None: the fine one when there is one
        :param viewdirs "origin": the reference's fake direction -p/|p| (src/util/recon.py:54), with density_grid's warning; or a
        3-vector: ONE constant direction, normalised -- what one bakes for a fixed camera side.  Ignored by a network that takes no
        view directions.
        :param eval_batch_size the chunk length, rounded DOWN to an even number (at least 2), so the volume does not depend on it
        (util.recon.vertex_colors has the reason)
        :param skip_threshold, keep_largest, min_voxels the skip grid: OccupancyGrid.from_density(vol[..., 3], c1, c2,
        skip_threshold, dilate=0, keep_largest=, min_voxels=)
        :param dtype torch.float32, or torch.float16: the bake is the fp32 one and `to_half` is applied to its result
        A non-finite value in the volume raises ValueError."""
        vol, (reso, c1, c2), _ = _bake("BakedVolume.from_model", net, c1, c2, reso, dtype, coarse, eval_batch_size, viewdirs=viewdirs)
        return cls(vol.view(*reso, 4), c1, c2, skip_threshold, keep_largest=keep_largest, min_voxels=min_voxels)

    def sparse(self, occupancy=None):
        """The SparseBakedVolume of this volume: the rows of the grid points that the occupied cells of `occupancy` read (None: the
        volume's own skip grid; or an OccupancyGrid of the same reso, c1, c2) and nothing else.  It renders the bytes of this volume's
        march with those bits: with None, `sparse().render(...)` equals `render(..., skip=True)` bit for bit at any skip_threshold."""
        return _sparse_of(self, self.vol.view(-1, 4), occupancy, "BakedVolume.sparse")


# ---------------------------------------------------------------- view-dependent volumes: real spherical harmonics up to degree 2

# max |Y_k| on the sphere, k = 1..8 (the basis of sh_basis)
_SH_MAX = (3.0 ** 0.5, 3.0 ** 0.5, 3.0 ** 0.5, 15.0 ** 0.5 / 2, 15.0 ** 0.5 / 2, 5.0 ** 0.5, 15.0 ** 0.5 / 2, 15.0 ** 0.5 / 2)


def _degree_of(n_basis, what):
    if n_basis not in (1, 4, 9):
        raise ValueError(f"{what}: a coefficient volume holds 1, 4 or 9 basis functions (degree 0, 1, 2), got {n_basis}")
    return {1: 0, 4: 1, 9: 2}[n_basis]


def sh_basis(dirs, degree, dtype=torch.float32):
    """The basis of include/pixelnerf_hip.h ("baked volumes"), with the kernel's operations in `dtype` on the host: dirs (...,3)
    (any length; normalised here as the kernel does) -> Y (...,(degree+1)^2), Y_0 = 1.  The four constants are rounded to fp32
    once, whatever `dtype`; a direction whose squared norm is 0 or not finite gets Y_k = 0 for k >= 1."""
    degree = int(degree)
    if degree not in (0, 1, 2):
        raise ValueError(f"sh_basis: degree must be 0, 1 or 2, got {degree}")
    d = torch.as_tensor(dirs, dtype=torch.float32).cpu().to(dtype)
    if d.dim() < 1 or d.shape[-1] != 3:
        raise ValueError("sh_basis: dirs must be (...,3)")
    c1, c2, c20, c22 = (float(torch.tensor(v, dtype=torch.float64).float()) for v in (3.0 ** 0.5, 15.0 ** 0.5, 5.0 ** 0.5 / 2, 15.0 ** 0.5 / 2))
    n2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    s = n2.sqrt()
    x, y, z = d[..., 0] / s, d[..., 1] / s, d[..., 2] / s
    cols = [torch.ones_like(x), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c20 * (3.0 * (z * z) - 1.0), c2 * (x * z),
            c22 * (x * x - y * y)]
    Y = torch.stack(cols[:(degree + 1) ** 2], dim=-1)
    bad = ~(torch.isfinite(n2) & (n2 != 0))
    Y[..., 1:] = torch.where(bad[..., None], torch.zeros_like(Y[..., 1:]), Y[..., 1:])
    return Y


class BakedSHVolume(_Baked):
    """A baked volume that keeps the dependence on the view direction: coef (nx,ny,nz,B,4) fp32 or fp16 on the device, B = (degree+1)^2 real
    spherical-harmonic coefficients (degree 0, 1 or 2) of (r, g, b, sigma) at the points of ops.gen_grid_points(c1, c2, reso).  The
    march evaluates every corner for the RAY's direction, clamps it (rgb to [0,1], sigma to >= 0) and then blends: a ray renders as
    BakedVolume would render the volume "this object seen from direction d" (`at_direction`).  Still trilinear in space, still
    equidistant samples, still nothing outside the box; degree <= 2.  Storage is fp32 or fp16: a half volume renders the bytes of
    its `float()`, a stored coefficient c being off by at most max(2^-11 |c|, 2^-25).
    Memory: 16 B bytes per grid point in fp32 -- 64 / 144 bytes at degree 1 / 2, 302 MB at 128^3 and degree 2 (BakedVolume: 16 bytes,
    34 MB) --, half of that in fp16.
    The skip grid is an OccupancyGrid (dilate 0) of an upper bound of sigma over all directions, s_0 + (1 + 2^-16) sum_k m_k |s_k|
    with m_k = max |Y_k|: at skip_threshold 0 a skipped cell has sigma exactly 0 at its eight corners for every direction, so
    `render(skip=True)` equals `render(skip=False)` bit for bit."""

    _stored_name = "coef"

    def __init__(self, coef, c1, c2, skip_threshold=0.0, keep_largest=None, min_voxels=None):
        from .. import _lib
        if not isinstance(coef, torch.Tensor) or coef.dim() != 5 or coef.shape[4] != 4 \
                or coef.dtype not in (torch.float32, torch.float16):
            raise ValueError("BakedSHVolume: coef must be a (nx,ny,nz,B,4) float32 or float16 tensor")
        degree = _degree_of(coef.shape[3], "BakedSHVolume")
        reso, c1, c2, _ = _check_geometry(coef.shape[:3], c1, c2, 0)  # (before any device work)
        skip_threshold = float(skip_threshold)
        if skip_threshold != skip_threshold:
            raise ValueError("BakedSHVolume: skip_threshold is NaN")
        if not coef.is_cuda:
            raise _lib.PixelNerfHipError(f"BakedSHVolume: coef must live on a HIP device (got {coef.device}); pixelnerf_amd has no CPU path")
        coef = coef.detach().contiguous()
        if not bool(torch.isfinite(coef).all()):
            raise ValueError("BakedSHVolume: the volume holds a non-finite value")
        self.coef, self.degree, self.reso, self.c1, self.c2, self.skip_threshold = coef, degree, reso, c1, c2, skip_threshold
        self.occupancy = OccupancyGrid.from_density(self.sigma_bound(), c1, c2, skip_threshold, dilate=0, keep_largest=keep_largest,
                                                    min_voxels=min_voxels)

    def sigma_bound(self):
        """(nx,ny,nz) fp32: s_0 + (1 + 2^-16) sum_{k>=1} m_k |s_k|, in fp64 from the stored coefficients (fp16 ones widened: the
        values the kernel sees) and rounded UP to fp32 -- no direction gives the kernel a larger sigma at the point (the slack covers
        the fp32 rounding of Y and of the sum)"""
        s = self.coef[..., 3].float().double()
        bound = s[..., 0]
        if s.shape[-1] > 1:
            m = torch.tensor(_SH_MAX[:s.shape[-1] - 1], dtype=torch.float64, device=s.device)
            bound = bound + (1.0 + 2.0 ** -16) * (s[..., 1:].abs() * m).sum(dim=-1)
        b32 = bound.float()
        up = torch.nextafter(b32, torch.full_like(b32, float("inf")))
        return torch.where(b32.double() < bound, up, b32).contiguous()

    @staticmethod
    def directions(n_dirs):
        """(n_dirs,3) fp32 on the host: the spherical Fibonacci set z_m = 1 - (2m+1)/M, phi_m = m pi (3 - sqrt 5), built in fp64 and
        rounded to fp32 -- the directions from_model shows the network, as they are"""
        import math
        n_dirs = int(n_dirs)
        if n_dirs < 1:
            raise ValueError(f"BakedSHVolume.directions: n_dirs must be positive, got {n_dirs}")
        m = torch.arange(n_dirs, dtype=torch.float64)
        z = 1.0 - (2.0 * m + 1.0) / n_dirs
        phi = m * (math.pi * (3.0 - math.sqrt(5.0)))
        rho = (1.0 - z * z).clamp_min(0.0).sqrt()
        return torch.stack((rho * phi.cos(), rho * phi.sin(), z), dim=1).float()

    @staticmethod
    def projection(n_dirs, degree):
        """(B, n_dirs) fp64: pinv of the basis matrix of directions(n_dirs), built in fp64 from the fp32 directions; from_model
        applies it rounded to fp32.  n_dirs < 2 B raises ValueError (the set must over-determine the fit: the condition number of
        the basis matrix is 1.05 at 32 and 1.16 at 18 directions for degree 2)."""
        degree = int(degree)
        if degree not in (0, 1, 2):
            raise ValueError(f"BakedSHVolume: degree must be 0, 1 or 2, got {degree}")
        if int(n_dirs) < 2 * (degree + 1) ** 2:
            raise ValueError(f"BakedSHVolume: degree {degree} needs n_dirs >= {2 * (degree + 1) ** 2}, got {n_dirs}")
        return torch.linalg.pinv(sh_basis(BakedSHVolume.directions(n_dirs), degree, torch.float64))

    @classmethod
    def from_tensor(cls, coef, c1, c2, skip_threshold=0.0):
        """wrap a caller-made volume: coef (nx,ny,nz,B,4) fp32 or fp16 HIP tensor spanning [c1, c2], B in {1, 4, 9}"""
        return cls(coef, c1, c2, skip_threshold)

    @classmethod
    def from_model(cls, net, c1, c2, reso, degree=2, n_dirs=32, coarse=None, eval_batch_size=100000, skip_threshold=0.0,
                   keep_largest=None, min_voxels=None, dtype=torch.float32):
        """Bake ONE encoded object with its dependence on the view direction: the network is evaluated on every grid point once per
        direction u_m of `directions(n_dirs)` and all four output columns are projected, in linear space (the clamps happen at render
        time), onto the basis: coef[:, k, :] = sum_m P[k, m] net(points, viewdirs = u_m)[:, :4] with P = fp32(projection(n_dirs,
        degree)), accumulated in fp32 in the fixed order m = 0..M-1 -- the volume does not depend on eval_batch_size (rounded DOWN to
        an even number, as BakedVolume.from_model) and is the same from run to run.  n_dirs network passes: n_dirs times
        BakedVolume.from_model's time.  The checks, the eval / train flag and `coarse` are BakedVolume.from_model's.
        A network that takes no view directions is baked at degree 0, whatever was asked, with a warning.
        Memory: 64 / 144 bytes per point at degree 1 / 2 (302 MB at 128^3, degree 2); half of it with dtype=torch.float16, which
        bakes and accumulates in fp32 exactly as above and then applies `to_half` (the fp32 tensor exists during the bake)."""
        coef, (reso, c1, c2), _ = _bake("BakedSHVolume.from_model", net, c1, c2, reso, dtype, coarse, eval_batch_size, degree=int(degree),
                                        n_dirs=n_dirs)
        return cls(coef.view(*reso, *coef.shape[1:]), c1, c2, skip_threshold, keep_largest=keep_largest, min_voxels=min_voxels)

    def at_direction(self, d):
        """The RGBA volume "this object seen from direction d" (a 3-vector of any length): per grid point coef_0 Y_0 + coef_1 Y_1
        + ... in this order in fp32, then rgb clamped to [0,1] and sigma to >= 0 -- the kernel's corner value.  What one bakes for a
        fixed camera side; a ray of direction d renders through it as it does through this volume.  A half volume gives the fp32
        BakedVolume of `float().at_direction(d)`."""
        if self.coef.dtype == torch.float16:
            return self.float().at_direction(d)
        d = torch.as_tensor(d, dtype=torch.float32).flatten()
        if d.numel() != 3:
            raise ValueError("BakedSHVolume.at_direction: d must be a 3-vector")
        Y = sh_basis(d, self.degree, torch.float32).tolist()
        with torch.no_grad():
            v = self.coef[..., 0, :] * Y[0]
            for k in range(1, len(Y)):
                v = v + self.coef[..., k, :] * Y[k]
            zero, one = torch.zeros_like(v), torch.ones_like(v)
            v = torch.where(v < 0, zero, v)
            v[..., :3] = torch.where(v[..., :3] > 1, one[..., :3], v[..., :3])
        return BakedVolume(v, self.c1, self.c2, self.skip_threshold)

    def sparse(self, occupancy=None):
        """BakedVolume.sparse for the coefficient volume: the kept points' (B,4) coefficients; `sparse().render(...)` equals
        `render(..., skip=True)` bit for bit"""
        return _sparse_of(self, self.coef.view(-1, *self.coef.shape[3:]), occupancy, "BakedSHVolume.sparse")


# ---------------------------------------------------------------- sparse volumes: only the rows that occupied cells read

def _same_grid(what, occupancy, reso, c1, c2):
    if not isinstance(occupancy, OccupancyGrid):
        raise ValueError(f"{what}: occupancy must be an OccupancyGrid, got {type(occupancy).__name__}")
    if (tuple(occupancy.reso), tuple(occupancy.c1), tuple(occupancy.c2)) != (tuple(reso), tuple(c1), tuple(c2)):
        raise ValueError(f"{what}: the occupancy grid spans {occupancy.reso} points over {occupancy.c1} .. {occupancy.c2}, the volume "
                         f"{tuple(reso)} over {tuple(c1)} .. {tuple(c2)}")


def _sparse_of(dense, per_point, occupancy, what):
    """BakedVolume.sparse / BakedSHVolume.sparse: the kept rows of the dense tensor `per_point` (P, ...)"""
    occupancy = dense.occupancy if occupancy is None else occupancy
    _same_grid(what, occupancy, dense.reso, dense.c1, dense.c2)
    if occupancy.bits.device != per_point.device:
        raise ValueError(f"{what}: the occupancy grid lives on {occupancy.bits.device}, the volume on {per_point.device}")
    from .. import ops
    index, ids = ops.sparse_points(occupancy.bits, dense.reso)
    return SparseBakedVolume(per_point.index_select(0, ids.long()), occupancy, index=index, ids=ids)


class SparseBakedVolume(_Baked):
    """A baked volume that keeps only what its occupancy grid lets the march read.  rows: (M,4) (degree None: the RGBA march) or
    (M,B,4) (degree 0, 1, 2: the view-dependent march), fp32 or fp16, on the device, the rows of the dense volume at the kept points; ids (M,)
    int32: their linear ids (i ny + j) nz + k, ascending; index (nx,ny,nz) int32: the rank of a kept point, -1 elsewhere; occupancy:
    the OccupancyGrid whose cells decide (reso, c1, c2 are its geometry).  Kept: the corners of the occupied cells, closed over the
    pairs (2j, 2j+1) of the linear ids (include/pixelnerf_hip.h, "baked volumes", the sparse paragraph).
    `render` / `render_views` give the bytes of the dense volume's march with `occupancy.bits`; `from_model` bakes the kept points
    alone and gives the dense bake's rows bit for bit.  Memory: `nbytes` = rows + 4 bytes per grid point (index) + the bitfield."""

    _stored_name = "rows"

    def __init__(self, rows, occupancy, index=None, ids=None):
        from .. import _lib, ops
        if not isinstance(rows, torch.Tensor) or rows.dim() not in (2, 3) or rows.shape[-1] != 4 \
                or rows.dtype not in (torch.float32, torch.float16):
            raise ValueError("SparseBakedVolume: rows must be a (M,4) or (M,B,4) float32 or float16 tensor")
        degree = _degree_of(rows.shape[1], "SparseBakedVolume") if rows.dim() == 3 else None
        if not isinstance(occupancy, OccupancyGrid):
            raise ValueError(f"SparseBakedVolume: occupancy must be an OccupancyGrid, got {type(occupancy).__name__}")
        if not rows.is_cuda:
            raise _lib.PixelNerfHipError(f"SparseBakedVolume: rows must live on a HIP device (got {rows.device}); pixelnerf_amd has no CPU path")
        if occupancy.bits.device != rows.device:
            raise ValueError(f"SparseBakedVolume: the occupancy grid lives on {occupancy.bits.device}, the rows on {rows.device}")
        if index is None or ids is None:
            index, ids = ops.sparse_points(occupancy.bits, occupancy.reso)
        if ids.shape[0] != rows.shape[0]:
            raise ValueError(f"SparseBakedVolume: the occupancy grid keeps {ids.shape[0]} points, rows holds {rows.shape[0]}")
        rows = rows.detach().contiguous()
        if not bool(torch.isfinite(rows).all()):
            raise ValueError("SparseBakedVolume: the volume holds a non-finite value")
        self.rows, self.degree, self.index, self.ids, self.occupancy = rows, degree, index, ids, occupancy
        self.reso, self.c1, self.c2 = occupancy.reso, occupancy.c1, occupancy.c2

    _index = property(lambda self: self.index)
    _ids = property(lambda self: self.ids)

    @property
    def n_rows(self):
        return self.rows.shape[0]

    @property
    def nbytes(self):
        return self.rows.numel() * self.rows.element_size() + 4 * (self.index.numel() + self.occupancy.bits.numel())

    def _around(self, rows):
        return type(self)(rows, self.occupancy, index=self.index, ids=self.ids)

    @classmethod
    def from_model(cls, net, c1, c2, reso, occupancy, degree=None, n_dirs=32, viewdirs="origin", coarse=None, eval_batch_size=100000,
                   dtype=torch.float32):
        """The sparse bake: BakedVolume.from_model's loop (degree None; `viewdirs` as there) or BakedSHVolume.from_model's (degree
        0, 1, 2 with `n_dirs` directions; `viewdirs` is not used) -- the same checks, the same fixed projection order, even chunks, the
        train / eval flag restored -- over the kept points of `occupancy` in ascending order (ops.gen_grid_points_at supplies them): the
        network sees M points per pass, not nx ny nz.
        `rows` equals the dense from_model tensor at `ids` bit for bit, at every precision and whatever eval_batch_size: the kept set is
        closed over the pairs (2j, 2j+1) of the dense launch and a chunk has an even length, so every kept point stands at a place of
        its own parity (profiles/occupancy_notes.md).  With occupancy = OccupancyGrid.from_model(net, c1, c2, reso, threshold,
        dilate=1) the result is the dense bake with nothing in the cells the grid calls empty.  A non-finite output raises ValueError.
        dtype=torch.float16: the fp32 bake, then `to_half` on the rows."""
        rows, _, (index, ids) = _bake("SparseBakedVolume.from_model", net, c1, c2, reso, dtype, coarse, eval_batch_size, sparse=True,
                                      occupancy=occupancy, degree=degree, n_dirs=n_dirs, viewdirs=viewdirs)
        return cls(rows, occupancy, index=index, ids=ids)

    def _march_args(self, step, terminate, skip):
        if not skip:
            raise ValueError("SparseBakedVolume: skip=False is not available (a sparse volume holds nothing to march unskipped)")
        return super()._march_args(step, terminate, True)

    def to_dense(self):
        """(nx,ny,nz,4) or (nx,ny,nz,B,4): the rows at their grid points, zeros at the dropped ones -- marched with `occupancy.bits` it
        renders the bytes of this volume; the dtype is the rows'"""
        total = self.reso[0] * self.reso[1] * self.reso[2]
        dense = torch.zeros((total, *self.rows.shape[1:]), dtype=self.rows.dtype, device=self.rows.device)
        dense.index_copy_(0, self.ids.long(), self.rows)
        return dense.view(*self.reso, *self.rows.shape[1:])

    def state_dict(self):
        """the rows (the degree follows from their shape), the bitfield and the geometry; index and ids are rebuilt on load and are the
        same bytes.  The threshold and the dilation the grid was built with are not part of the state."""
        return {"rows": self.rows, "bits": self.occupancy.bits, "reso": torch.tensor(self.reso, dtype=torch.int64),
                "c1": torch.tensor(self.c1, dtype=torch.float64), "c2": torch.tensor(self.c2, dtype=torch.float64)}

    @classmethod
    def from_state_dict(cls, state, device=None):
        """:param device where to put the volume; None: where state["rows"] lives.  The loaded grid reports threshold NaN and dilate 0
        (neither is recorded); its n_occupied is counted from the bits."""
        rows = state["rows"] if device is None else state["rows"].to(device)
        bits = state["bits"].to(rows.device).contiguous()
        table = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int32, device=rows.device)
        n_occupied = table[bits.view(torch.uint8).long()].sum().to(torch.int32)
        occupancy = OccupancyGrid(bits, state["reso"].tolist(), state["c1"].tolist(), state["c2"].tolist(), float("nan"), 0, n_occupied)
        return cls(rows, occupancy)


# ---------------------------------------------------------------- scenes: several posed volumes in one image

def _kind_of(v):
    return type(v).__name__, v.degree, v.dtype, v._stored_name == "rows"


class BakedScene:
    """1 to 8 baked volumes of ONE kind, each placed in the world by a rigid pose, marched together (ops.baked_scene_render;
    include/pixelnerf_hip.h, "Scenes of several baked volumes").  Each object keeps its own frame, grid and box; along a world ray the
    objects are sampled at the same depths, each as its own `render` samples the ray in its frame, and mixed per sample (sigma = the
    sum, colour weighted by sigma) before compositing -- so overlapping volumes, and one in front of another, attenuate each other as
    separate renders cannot.  One volume at the identity pose renders the bytes of its own `render`.
    volumes: a list of BakedVolume, BakedSHVolume or SparseBakedVolume of one class, degree, dtype and layout on one device; poses:
    (N,4,4) or (N,3,4) object-to-world, rigid (what `register` recovers, inverted, is such a pose); kept as given, on the host, fp32.
    `render` and `render_views` are inference: they run under torch.no_grad().  `render_diff` and `render_views_diff` give the same
    bytes with autograd to the world rays or the cameras and to the object poses (include/pixelnerf_hip.h, "Gradients of the scene
    march"); `place` descends on the poses of chosen objects.  `trainable()` gives the stored values of chosen objects their
    gradient through the same march (include/pixelnerf_hip.h, "Gradients of the scene march with respect to the STORED VALUES"), and
    `fit_scene` descends on them.  Nothing is copied: the scene refers to its volumes."""

    def __init__(self, volumes, poses):
        from .. import _lib
        if not isinstance(volumes, (list, tuple)) or not 1 <= len(volumes) <= _lib.BAKED_SCENE_MAX_OBJECTS:
            raise ValueError(f"BakedScene: volumes must be a list of 1 to {_lib.BAKED_SCENE_MAX_OBJECTS} baked volumes, got "
                             f"{len(volumes) if isinstance(volumes, (list, tuple)) else type(volumes).__name__}")
        for j, v in enumerate(volumes):
            if not isinstance(v, _Baked):
                raise ValueError(f"BakedScene: volume {j} is a {type(v).__name__}, not a baked volume")
            if _kind_of(v) != _kind_of(volumes[0]):
                raise ValueError(f"BakedScene: volumes 0 and {j} differ in kind -- (class, degree, dtype, sparse) {_kind_of(volumes[0])} against "
                                 f"{_kind_of(v)} -- and one scene holds one kind; convert with .float() / .half() (dtype), .sparse(occ) / "
                                 ".to_dense() (layout), sh.at_direction(d) (a coefficient volume as an RGBA one)")
            if v._stored().device != volumes[0]._stored().device:
                raise ValueError(f"BakedScene: volume {j} lives on {v._stored().device}, volume 0 on {volumes[0]._stored().device}")
        poses = torch.as_tensor(poses).detach().to("cpu", torch.float32)
        if poses.dim() != 3 or tuple(poses.shape[1:]) not in ((4, 4), (3, 4)) or poses.shape[0] != len(volumes):
            raise ValueError(f"BakedScene: poses must be ({len(volumes)},4,4) or ({len(volumes)},3,4) object-to-world, got {tuple(poses.shape)}")
        from .. import ops
        for j, pose in enumerate(poses):
            ops._baked_pose(f"BakedScene: object {j}", pose)  # (finite and rigid: refused here, not at the first render)
        self.volumes, self.poses = list(volumes), poses

    def __len__(self):
        return len(self.volumes)

    def with_pose(self, j, pose):
        """this scene with object j at another pose (3,4) or (4,4); the volumes are shared"""
        j = int(j)
        if not 0 <= j < len(self):
            raise IndexError(f"BakedScene.with_pose: no object {j} in a scene of {len(self)}")
        pose = torch.as_tensor(pose).detach().to("cpu", torch.float32)
        if tuple(pose.shape) not in ((3, 4), (4, 4)):
            raise ValueError(f"BakedScene.with_pose: pose must be (3,4) or (4,4), got {tuple(pose.shape)}")
        poses = self.poses.clone()
        poses[j, :3] = pose[:3]
        return BakedScene(self.volumes, poses)

    def _objects(self, skip):
        """the list ops.baked_scene_render takes"""
        objects = []
        for v, pose in zip(self.volumes, self.poses):
            bits = v.occupancy.bits if skip or v._index is not None else None
            objects.append((v._stored(), v.degree, v.reso, v.c1, v.c2, pose, bits, v._index))
        return objects

    def _march_args(self, step, terminate):
        step = min(min(v.cell_size) for v in self.volumes) if step is None else float(step)
        return step, (0.0 if terminate is None else float(terminate))

    def render(self, rays, step=None, white_bkgd=False, terminate=None, skip=True):
        """world rays (...,8) on the scene's device -> DotMap(rgb (...,3), depth (...), alpha (...)); ops.baked_scene_render.
        :param step the sample distance in the units of z; None: the smallest cell edge over all objects
        :param terminate as BakedVolume.render: checked every 64 samples on the transmittance of the mixture
        :param skip march every dense volume against its skip grid (exact at skip_threshold 0); sparse volumes always do"""
        from .. import ops
        flat, lead = _flat_rays("BakedScene.render", rays)
        step, terminate = self._march_args(step, terminate)
        with torch.no_grad():
            return _ray_result(*ops.baked_scene_render(flat, self._objects(skip), step, white_bkgd=white_bkgd, terminate=terminate), lead)

    def render_views(self, poses_c2w, W, H, focal, z_near, z_far, c=None, gt_rgb=None, want_u8=False, step=None, white_bkgd=False,
                     terminate=None, skip=True):
        """Every pixel of the target views from their cameras, as BakedVolume.render_views: poses_c2w (NVt,4,4) camera-to-WORLD; the
        rays are regenerated in the kernel (the same bits as render(util.gen_rays(...))), and the outputs go through the same
        epilogue.  :return DotMap: rgb (NVt,H,W,3), depth, alpha, depth_norm (NVt,H,W); rgb_u8 with want_u8; psnr, ssim with gt_rgb"""
        from .. import ops
        W, H, focal, c = _camera_args("BakedScene.render_views", poses_c2w, W, H, focal, c, gt_rgb)
        step, terminate = self._march_args(step, terminate)
        with torch.no_grad():
            rgb, depth, alpha = ops.baked_scene_render_views(poses_c2w.float(), W, H, focal, c, z_near, z_far, self._objects(skip), step,
                                                             white_bkgd=white_bkgd, terminate=terminate)
            return _views_result(rgb, depth, alpha, poses_c2w.shape[0], W, H, z_near, z_far, gt_rgb, want_u8)

    def trainable(self, objects=None):
        """-> TrainableScene: an nn.Module whose nn.ParameterList holds copies of the fp32 stored tensors of the chosen objects
        (indices; None: all), the others referenced and frozen; `forward(rays, ...)` and `forward_views(...)` render with gradients
        attached, `.scene()` gives the fitted scene back (`fit_scene` is the loop around it).  An fp16 scene is refused."""
        return TrainableScene(self, objects)

    def _obj_poses(self, what, poses):
        """the object poses of a differentiable call: self.poses, or the tensor (N,3,4) / (N,4,4) that replaces them -> (N,3,4)"""
        if poses is None:
            return self.poses[:, :3]
        if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or tuple(poses.shape[1:]) not in ((3, 4), (4, 4)) \
                or poses.shape[0] != len(self) or not poses.is_floating_point():
            raise ValueError(f"BakedScene.{what}: the object poses must be a float tensor ({len(self)},3,4) or ({len(self)},4,4) "
                             f"object-to-world, got {tuple(poses.shape) if isinstance(poses, torch.Tensor) else type(poses).__name__}")
        return poses[:, :3]

    def _march_diff(self, source, obj_poses, step, white_bkgd, terminate, skip):
        from .. import autograd
        volumes = [ob[:5] + ob[6:] for ob in self._objects(skip)]
        return autograd.baked_scene_march_autograd(source, volumes, obj_poses, step, white_bkgd=white_bkgd, terminate=terminate)

    def render_diff(self, rays, poses=None, step=None, white_bkgd=False, terminate=None, skip=True):
        """`render` with autograd: world rays (...,8) -> DotMap(rgb (...,3), depth (...), alpha (...)), the bytes `render` gives, and a
        backward (one pnr_baked_scene_backward_rays call: no atomics, the same bytes on every call) that hands dL/d rays to whatever
        made them and, when `poses` requires grad, dL/d poses to it.
        :param poses None: the scene's own poses (constants); else a tensor (N,3,4) or (N,4,4), object-to-world, that REPLACES them
        for this call -- it must be rigid, as the scene's are; the gradient is that of 12 free numbers per object, and a caller that
        builds the poses from rigid parameters (`moved_poses`) gets its projection from autograd.  The poses are kernel arguments by
        value: they are read to the host once per call.  step, terminate, skip: as render."""
        flat, lead = _flat_rays("BakedScene.render_diff", rays)
        obj_poses = self._obj_poses("render_diff", poses)
        step, terminate = self._march_args(step, terminate)
        return _ray_result(*self._march_diff((flat,), obj_poses, step, white_bkgd, terminate, skip), lead)

    def render_views_diff(self, poses_c2w, W, H, focal, z_near, z_far, c=None, obj_poses=None, step=None, white_bkgd=False, terminate=None,
                          skip=True):
        """`render_views` without its epilogue and with autograd: poses_c2w (NVt,4,4) -> DotMap(rgb (NVt,H,W,3), depth and alpha
        (NVt,H,W)), the bytes `render_views` gives; the backward is pnr_baked_scene_backward_views, followed by ops.gen_rays_backward
        for the cameras (the intrinsics are constants).  obj_poses: as `poses` of render_diff.  What `place` descends on."""
        W, H, focal, c = _camera_args("BakedScene.render_views_diff", poses_c2w, W, H, focal, c, None)
        obj_poses = self._obj_poses("render_views_diff", obj_poses)
        NVt = poses_c2w.shape[0]
        step, terminate = self._march_args(step, terminate)
        rgb, depth, alpha = self._march_diff((poses_c2w.float(), W, H, focal, c, z_near, z_far), obj_poses, step, white_bkgd, terminate, skip)
        return DotMap(rgb=rgb.reshape(NVt, H, W, 3), depth=depth.reshape(NVt, H, W), alpha=alpha.reshape(NVt, H, W))


# ---------------------------------------------------------------- fitting: gradients with respect to the stored values

_FP32_ONLY = "gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards"


class TrainableBaked(torch.nn.Module):
    """`volume.trainable()`: the fp32 stored tensor of a BakedVolume, BakedSHVolume or SparseBakedVolume as this module's one
    nn.Parameter (`stored`, a copy: the volume itself never changes), marched by the inference entries with gradients attached
    (autograd.baked_march_autograd: forward = the bytes of `volume.render`, backward = pnr_baked_backward_*).  Gradients reach the
    stored values only -- rays and poses that require grad are refused unless `forward(ray_grad=True)` / `forward_views(
    pose_grad=True)` asks for theirs too (pnr_baked_ray_backward_*) -- and those of the stored values are not bit-reproducible from
    run to run (fp32 atomics).  An fp16 volume is refused: fit in fp32 and call `half()` afterwards.
    `skip=True` marches against the skip grid of the volume `trainable()` was called on, as it was then: the cells it calls empty
    receive no gradient and stay as they are -- fitting with skip=True FREEZES the empty cells; with skip=False (the default) every
    cell a ray crosses can change.  A sparse volume holds nothing else, so it always marches against its grid.
    `tv(...)` is the smoothness prior a fit to few views needs: the total variation of `stored`, differentiable, with no atomics."""

    def __init__(self, volume):
        super().__init__()
        if not isinstance(volume, _Baked):
            raise TypeError(f"TrainableBaked: expected a baked volume, got {type(volume).__name__}")
        if volume.dtype != torch.float32:
            raise TypeError(f"{type(volume).__name__}.trainable: {_FP32_ONLY}")
        self._source = volume
        self.stored = torch.nn.Parameter(volume._stored().clone())

    def _march(self, source, step, white_bkgd, terminate, skip, source_grad=False):
        from .. import autograd
        v = self._source
        step, terminate, bits = _Baked._march_args(v, step, terminate, skip or v._index is not None)
        march = autograd.baked_march_rays_autograd if source_grad else autograd.baked_march_autograd
        return march(self.stored, source, v.degree, v.reso, v.c1, v.c2, step, bits=bits, index=v._index, white_bkgd=white_bkgd,
                     terminate=terminate)

    def forward(self, rays, step=None, white_bkgd=False, terminate=None, skip=False, ray_grad=False):
        """rays (...,8) -> DotMap(rgb (...,3), depth (...), alpha (...)) as `render`, differentiable with respect to `stored`.
        ray_grad=True: differentiable with respect to the rays as well (pnr_baked_ray_backward_rays); the default refuses rays that
        require grad."""
        flat, lead = _flat_rays("TrainableBaked.forward", rays)
        return _ray_result(*self._march((flat,), step, white_bkgd, terminate, skip, source_grad=bool(ray_grad)), lead)

    def forward_views(self, poses_c2w, W, H, focal, z_near, z_far, c=None, step=None, white_bkgd=False, terminate=None, skip=False,
                      pose_grad=False):
        """every pixel of the views, the rays regenerated in the kernel (as `render_views`, without its epilogue)
        -> DotMap(rgb (NVt,H,W,3), depth (NVt,H,W), alpha (NVt,H,W)), differentiable with respect to `stored`.  pose_grad=True:
        differentiable with respect to the poses as well (pnr_baked_ray_backward_views, then ops.gen_rays_backward); the default
        refuses poses that require grad."""
        W, H, focal, c = _camera_args("TrainableBaked.forward_views", poses_c2w, W, H, focal, c, None)
        NVt = poses_c2w.shape[0]
        rgb, depth, alpha = self._march((poses_c2w.float(), W, H, focal, c, z_near, z_far), step, white_bkgd, terminate, skip,
                                        source_grad=bool(pose_grad))
        return DotMap(rgb=rgb.reshape(NVt, H, W, 3), depth=depth.reshape(NVt, H, W), alpha=alpha.reshape(NVt, H, W))

    def tv(self, rgb=1.0, sigma=1.0, sh=None, eps=1e-8):
        """The total-variation prior of the stored values (include/pixelnerf_hip.h, "Total-variation prior"): a 0-dim fp32 tensor,
        differentiable with respect to `stored` (autograd.baked_tv_autograd; no atomics: value and gradient are bit-reproducible).
        (1/N) sum over points and elements of weight x sqrt(d_x^2 + d_y^2 + d_z^2 + eps), the d raw differences to the next grid
        point; N the number of grid points (a sparse volume: of kept points, and a difference to a dropped point is 0).
        :param rgb weighs channels 0..2 of the RGBA row or of the DC basis row
        :param sigma weighs channel 3 of the same row
        :param sh weighs every channel of the basis rows k >= 1; None: the DC weights"""
        from .. import autograd
        v = self._source
        return autograd.baked_tv_autograd(self.stored, v.degree, v.reso, _tv_weights("TrainableBaked.tv", v.degree, rgb, sigma, sh), eps=eps,
                                          index=v._index, ids=v._ids)

    def volume(self):
        """a fresh volume of the current values: checked as its constructor checks (a non-finite value raises ValueError) and with
        its skip grid rebuilt from them (a sparse volume keeps its occupancy grid, index and ids: its kept set does not grow)"""
        return self._source._around(self.stored.detach().clone())


def fit(volume, rays, target_rgb, steps=200, lr=1e-2, batch=4096, seed=0, step=None, white_bkgd=False, terminate=None, skip=False,
        tv_rgb=0.0, tv_sigma=0.0, tv_sh=None, tv_eps=1e-8):
    """Fit a baked volume to colours: Adam on `volume.trainable()` over `steps` batches of `batch` rays drawn with replacement from
    rays (...,8) by a CPU torch.Generator seeded with `seed`, loss = mean((rgb - target_rgb)^2) over the batch.  After every step
    an RGBA volume (BakedVolume, RGBA rows) is projected back onto what it stores: rgb into [0,1], sigma >= 0; a coefficient volume
    is left alone (its clamps are part of the march).  step, white_bkgd, terminate, skip: as TrainableBaked.forward (skip=True
    freezes the cells the volume's skip grid calls empty).
    tv_rgb, tv_sigma, tv_sh, tv_eps: the total-variation prior, `TrainableBaked.tv`'s rgb, sigma, sh and eps: when any weight is > 0
    the step's loss is mse + module.tv(...) (`losses` keeps reporting the mse alone); with all of them 0 -- the default -- no TV call
    is made.
    -> (the fitted volume -- a new one, `volume` is unchanged --, losses: the `steps` batch losses as floats, read once at the end)"""
    flat, _ = _flat_rays("fit", rays)
    if not isinstance(target_rgb, torch.Tensor) or tuple(target_rgb.shape) != tuple(rays.shape[:-1]) + (3,):
        raise ValueError(f"fit: target_rgb must be {tuple(rays.shape[:-1]) + (3,)}, got "
                         f"{tuple(target_rgb.shape) if isinstance(target_rgb, torch.Tensor) else type(target_rgb).__name__}")
    steps, batch = int(steps), int(batch)
    if steps < 0 or batch < 1:
        raise ValueError(f"fit: steps must be >= 0 and batch >= 1, got {steps}, {batch}")
    module = volume.trainable()
    prior = dict(rgb=tv_rgb, sigma=tv_sigma, sh=tv_sh, eps=tv_eps)
    use_prior = any(w > 0 for w in _tv_weights("fit", volume.degree, tv_rgb, tv_sigma, tv_sh))
    rays, target = flat.detach(), target_rgb.detach().reshape(-1, 3).float()
    R = rays.shape[0]
    if R == 0:
        raise ValueError("fit: no rays")
    optimiser = torch.optim.Adam(module.parameters(), lr=float(lr))
    gen = torch.Generator().manual_seed(int(seed))
    losses = []
    for _ in range(steps):
        ids = torch.randint(0, R, (min(batch, R),), generator=gen).to(rays.device)
        out = module(rays[ids], step=step, white_bkgd=white_bkgd, terminate=terminate, skip=skip)
        loss = ((out.rgb - target[ids]) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        (loss + module.tv(**prior) if use_prior else loss).backward()
        optimiser.step()
        if volume.degree is None:
            with torch.no_grad():
                module.stored[..., :3].clamp_(0.0, 1.0)
                module.stored[..., 3].clamp_(min=0.0)
        losses.append(loss.detach())
    return module.volume(), (torch.stack(losses).tolist() if losses else [])


_VISIBILITY_BATCH = 1 << 18  # rays per visibility call of fit_coarse_to_fine (the result does not depend on it)


def fit_coarse_to_fine(volume, rays, target_rgb, stages, prune=None, **fit_kwargs):
    """`fit` over a sequence of grids: stages = [(reso | None, steps), ...], reso an int, (nx,ny,nz) or None = stay.  Per stage k the
    volume is resampled (`volume.resample(reso)`) when the reso differs from its own, then fitted: fit(volume, rays, target_rgb,
    steps=steps, seed=seed + k, **fit_kwargs) -- every other argument of `fit` goes through, `seed` (default 0) is the first stage's.
    prune = dict(threshold=, dilate=1): after every stage the visibility of ALL rays (in batches, with the stage's step, terminate
    and skip) is taken and the volume pruned by it (`volume.prune`): the next stages fit a SparseBakedVolume, with skip=True, and
    refine by integer factors only.  Everything is checked before any device work.
    -> (the volume of the last stage, [the losses of each stage])"""
    what = "fit_coarse_to_fine"
    if not isinstance(volume, _Baked):
        raise TypeError(f"{what}: expected a baked volume, got {type(volume).__name__}")
    stages = _check_stages(what, stages)
    if prune is not None:
        if not isinstance(prune, dict) or "threshold" not in prune or set(prune) - {"threshold", "dilate"}:
            raise ValueError(f"{what}: prune must be None or dict(threshold=, dilate=1), got {prune!r}")
        prune = dict(threshold=float(prune["threshold"]), dilate=int(prune.get("dilate", 1)))
        if prune["threshold"] != prune["threshold"] or not 0 <= prune["dilate"] <= 4:
            raise ValueError(f"{what}: prune needs a threshold that is a number and a dilate in [0, 4], got {prune!r}")
    if "steps" in fit_kwargs:
        raise ValueError(f"{what}: the steps belong to the stages")
    flat = _flat_rays(what, rays)[0].detach()
    seed = int(fit_kwargs.pop("seed", 0))
    reso, sparse = tuple(volume.reso), volume._stored_name == "rows"
    for k, (new, _) in enumerate(stages):  # the chain of grids, walked on the host first
        if new is not None and new != reso:
            if sparse:
                _sparse_refinement(f"{what}: stage {k}", reso, new)
            reso = new
        sparse = sparse or prune is not None
    all_losses = []
    for k, (new, steps) in enumerate(stages):
        if new is not None and new != tuple(volume.reso):
            volume = volume.resample(new)
        kw = dict(fit_kwargs)
        if volume._stored_name == "rows":
            kw["skip"] = True
        volume, losses = fit(volume, rays, target_rgb, steps=steps, seed=seed + k, **kw)
        all_losses.append(losses)
        if prune is not None:
            vis = None
            for first in range(0, flat.shape[0], _VISIBILITY_BATCH):
                vis = volume.visibility(flat[first:first + _VISIBILITY_BATCH], step=kw.get("step"), terminate=kw.get("terminate"),
                                        skip=bool(kw.get("skip", False)), out=vis)
            volume = volume.prune(vis, prune["threshold"], prune["dilate"])
    return volume, all_losses


# ---------------------------------------------------------------- fitting a scene: stored-value gradients through the mixture

class TrainableScene(torch.nn.Module):
    """`scene.trainable(objects)`: the fp32 stored tensors of the chosen objects of a BakedScene (None: all) as this module's
    nn.ParameterList `stored` (copies: the scene and its volumes never change), marched TOGETHER by the inference entries with
    gradients attached (autograd.baked_scene_fit_autograd: forward = the bytes of `scene.render`, backward =
    pnr_baked_scene_stored_backward_*).  Where objects overlap or stand in front of one another every object's gradient depends on
    the others: fitting each volume alone against images of the scene gives another, wrong, answer.  The objects that are not
    chosen are referenced and FROZEN: they mix and attenuate and receive nothing.  A volume listed twice in the scene is ONE
    parameter and gets the sum of both listings' gradients (chosen when either listing is).  The gradients of the stored values are
    not bit-reproducible from run to run (fp32 atomics).  An fp16 scene is refused: fit in fp32 and call `half()` afterwards.
    `poses` / `obj_poses` that require grad get the gradient of `render_diff` (pnr_baked_scene_backward_*) in the same backward.
    `skip=True` marches every dense volume against the skip grid it had when `trainable()` was called: the cells it calls empty are
    frozen, as in TrainableBaked.  Sparse volumes always march against their grid.
    Where the mixture's density is exactly 0 its colour is the constant 0 (the header's convention): the density gradient of such a
    sample has no colour term, which TrainableBaked's has -- one object at the identity pose gets TrainableBaked's gradient except
    from those samples."""

    def __init__(self, scene, objects=None):
        super().__init__()
        if not isinstance(scene, BakedScene):
            raise TypeError(f"TrainableScene: expected a BakedScene, got {type(scene).__name__}")
        if scene.volumes[0].dtype != torch.float32:
            raise TypeError(f"BakedScene.trainable: {_FP32_ONLY}")
        N = len(scene)
        chosen = list(range(N)) if objects is None else [int(j) for j in objects]
        if not chosen or len(set(chosen)) != len(chosen) or not all(0 <= j < N for j in chosen):
            raise ValueError(f"BakedScene.trainable: objects must be distinct indices into a scene of {N} (None: all), got {objects}")
        self._source = scene
        self.slots, params, owner = [None] * N, [], {}  # slots[j]: the parameter object j marches, None: frozen
        for j, v in enumerate(scene.volumes):
            twin = next((k for k in range(N) if scene.volumes[k] is v and k in chosen), None)
            if twin is None:
                continue
            if id(v) not in owner:
                owner[id(v)] = len(params)
                params.append(torch.nn.Parameter(v._stored().clone()))
            self.slots[j] = owner[id(v)]
        self.stored = torch.nn.ParameterList(params)

    def _tensors(self):
        return [v._stored() if slot is None else self.stored[slot] for v, slot in zip(self._source.volumes, self.slots)]

    def _march(self, source, obj_poses, step, white_bkgd, terminate, skip):
        from .. import autograd
        scene = self._source
        step, terminate = scene._march_args(step, terminate)
        meta = [ob[1:5] + ob[6:] for ob in scene._objects(skip)]
        return autograd.baked_scene_fit_autograd(source, self._tensors(), meta, obj_poses, step, white_bkgd=white_bkgd, terminate=terminate)

    def forward(self, rays, poses=None, step=None, white_bkgd=False, terminate=None, skip=False):
        """world rays (...,8) -> DotMap(rgb (...,3), depth (...), alpha (...)) as `BakedScene.render`, differentiable with respect to
        the parameters; rays, and `poses` (None: the scene's own; else (N,3,4) or (N,4,4) object-to-world, as render_diff takes
        them), get their gradient when they require it."""
        flat, lead = _flat_rays("TrainableScene.forward", rays)
        obj_poses = self._source._obj_poses("trainable().forward", poses)
        return _ray_result(*self._march((flat,), obj_poses, step, white_bkgd, terminate, skip), lead)

    def forward_views(self, poses_c2w, W, H, focal, z_near, z_far, c=None, obj_poses=None, step=None, white_bkgd=False, terminate=None,
                      skip=False):
        """every pixel of the views, the rays regenerated in the kernel (as `BakedScene.render_views`, without its epilogue)
        -> DotMap(rgb (NVt,H,W,3), depth (NVt,H,W), alpha (NVt,H,W)), differentiable with respect to the parameters; poses_c2w and
        obj_poses get their gradient when they require it."""
        W, H, focal, c = _camera_args("TrainableScene.forward_views", poses_c2w, W, H, focal, c, None)
        obj_poses = self._source._obj_poses("trainable().forward_views", obj_poses)
        NVt = poses_c2w.shape[0]
        rgb, depth, alpha = self._march((poses_c2w.float(), W, H, focal, c, z_near, z_far), obj_poses, step, white_bkgd, terminate, skip)
        return DotMap(rgb=rgb.reshape(NVt, H, W, 3), depth=depth.reshape(NVt, H, W), alpha=alpha.reshape(NVt, H, W))

    def tv(self, rgb=1.0, sigma=1.0, sh=None, eps=1e-8):
        """the sum of the total-variation priors of the trainable objects (TrainableBaked.tv of each, a volume listed twice counted
        once): a 0-dim fp32 tensor, differentiable with respect to the parameters, no atomics"""
        from .. import autograd
        total, seen = None, set()
        for v, slot in zip(self._source.volumes, self.slots):
            if slot is None or slot in seen:
                continue
            seen.add(slot)
            term = autograd.baked_tv_autograd(self.stored[slot], v.degree, v.reso, _tv_weights("TrainableScene.tv", v.degree, rgb, sigma, sh),
                                              eps=eps, index=v._index, ids=v._ids)
            total = term if total is None else total + term
        return total

    def scene(self):
        """a fresh BakedScene of the current values: every trainable volume rebuilt as TrainableBaked.volume rebuilds it (checked,
        its skip grid rebuilt; a volume listed twice rebuilt once), the frozen ones shared, the poses kept"""
        rebuilt = {}
        volumes = []
        for v, slot in zip(self._source.volumes, self.slots):
            if slot is None:
                volumes.append(v)
                continue
            if slot not in rebuilt:
                rebuilt[slot] = v._around(self.stored[slot].detach().clone())
            volumes.append(rebuilt[slot])
        return BakedScene(volumes, self._source.poses.clone())


def fit_scene(scene, rays, target_rgb, objects=None, steps=200, lr=1e-2, batch=4096, seed=0, step=None, white_bkgd=False, terminate=None,
              skip=False, tv_rgb=0.0, tv_sigma=0.0, tv_sh=None, tv_eps=1e-8):
    """Fit the contents of a scene to colours of the scene: `fit`'s loop on `scene.trainable(objects)` -- Adam over `steps` batches of
    `batch` world rays drawn with replacement from rays (...,8) by a CPU torch.Generator seeded with `seed`, loss = mean((rgb -
    target_rgb)^2) over the batch; after every step RGBA volumes are projected back onto what they store (rgb into [0,1], sigma >=
    0), coefficient volumes are left alone.  objects: the indices of the objects that are fitted (None: all); the others are frozen
    and still mix and attenuate.  The poses stay where they are (`place` moves them; TrainableScene hands their gradient through for
    whoever wants a joint descent).  step, white_bkgd, terminate, skip: as TrainableScene.forward.  tv_*: the total-variation prior
    summed over the fitted objects, as in `fit` (`losses` reports the mse alone; all 0: no TV call).
    A step costs one scene march and one pnr_baked_scene_stored_backward_rays call; no network.
    -> (the fitted scene -- a new one, `scene` and its volumes are unchanged --, losses: the `steps` batch losses as floats)"""
    if not isinstance(scene, BakedScene):
        raise TypeError(f"fit_scene: expected a BakedScene, got {type(scene).__name__}")
    flat, _ = _flat_rays("fit_scene", rays)
    if not isinstance(target_rgb, torch.Tensor) or tuple(target_rgb.shape) != tuple(rays.shape[:-1]) + (3,):
        raise ValueError(f"fit_scene: target_rgb must be {tuple(rays.shape[:-1]) + (3,)}, got "
                         f"{tuple(target_rgb.shape) if isinstance(target_rgb, torch.Tensor) else type(target_rgb).__name__}")
    steps, batch = int(steps), int(batch)
    if steps < 0 or batch < 1:
        raise ValueError(f"fit_scene: steps must be >= 0 and batch >= 1, got {steps}, {batch}")
    module = scene.trainable(objects)
    degree = scene.volumes[0].degree
    prior = dict(rgb=tv_rgb, sigma=tv_sigma, sh=tv_sh, eps=tv_eps)
    use_prior = any(w > 0 for w in _tv_weights("fit_scene", degree, tv_rgb, tv_sigma, tv_sh))
    rays, target = flat.detach(), target_rgb.detach().reshape(-1, 3).float()
    R = rays.shape[0]
    if R == 0:
        raise ValueError("fit_scene: no rays")
    optimiser = torch.optim.Adam(module.parameters(), lr=float(lr))
    gen = torch.Generator().manual_seed(int(seed))
    losses = []
    for _ in range(steps):
        ids = torch.randint(0, R, (min(batch, R),), generator=gen).to(rays.device)
        out = module(rays[ids], step=step, white_bkgd=white_bkgd, terminate=terminate, skip=skip)
        loss = ((out.rgb - target[ids]) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        (loss + module.tv(**prior) if use_prior else loss).backward()
        optimiser.step()
        if degree is None:
            with torch.no_grad():
                for p in module.stored:
                    p[..., :3].clamp_(0.0, 1.0)
                    p[..., 3].clamp_(min=0.0)
        losses.append(loss.detach())
    return module.scene(), (torch.stack(losses).tolist() if losses else [])


# ---------------------------------------------------------------- registration: gradients with respect to the poses

def rodrigues(w):
    """Axis-angle vectors w (...,3) -> rotation matrices (...,3,3): R = I + A K + B K^2 with K the cross-product matrix of w,
    A = sin(t) / t, B = (1 - cos(t)) / t^2, t = |w|.  Below t^2 = 1e-6 the two are their series (1 - t^2/6 + t^4/120 and
    1/2 - t^2/24 + t^4/720; the terms left out are below 1e-21), so value and derivative are finite at w = 0 -- where R = I and
    dR/dw_a is the generator of axis a -- and nothing is divided by t."""
    if not isinstance(w, torch.Tensor) or w.dim() < 1 or w.shape[-1] != 3:
        raise ValueError("rodrigues: w must be (...,3)")
    t2 = (w * w).sum(dim=-1)
    small = t2 < 1e-6
    safe = torch.where(small, torch.ones_like(t2), t2)  # (the branch not taken still gets finite derivatives)
    t = safe.sqrt()
    A = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, t.sin() / t)
    B = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, (1.0 - t.cos()) / safe)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    o = torch.zeros_like(x)
    K = torch.stack((torch.stack((o, -z, y), dim=-1), torch.stack((z, o, -x), dim=-1), torch.stack((-y, x, o), dim=-1)), dim=-2)
    eye = torch.eye(3, dtype=w.dtype, device=w.device).expand(K.shape)
    return eye + A[..., None, None] * K + B[..., None, None] * (K @ K)


def moved_poses(poses0, w, v):
    """the poses `register` descends on: P = [R(w) R0 | t0 + v] over the bottom row of poses0; poses0 (NV,4,4), w and v (NV,3)"""
    top = torch.cat((rodrigues(w) @ poses0[:, :3, :3], (poses0[:, :3, 3] + v)[:, :, None]), dim=2)
    return torch.cat((top, poses0[:, 3:, :]), dim=1)


def register(volume, target_rgb, poses0, W, H, focal, z_near, z_far, c=None, steps=200, lr=1e-2, step=None, white_bkgd=False,
             terminate=None, skip=True):
    """Register cameras against a baked volume (iNeRF-style): Adam on a 6-DoF update per view, P = [R(w) R0 | t0 + v] with w an
    axis-angle vector through `rodrigues` and v a translation, both starting at 0, loss = mean((rgb - target_rgb)^2) over all pixels
    of all views, rgb = volume.render_views_diff(P, ...).rgb.  volume: any baked volume, fp32 or fp16 (it is not changed);
    target_rgb (NV,H,W,3); poses0 (NV,4,4) camera-to-world, the starting poses; W, H, focal, z_near, z_far, c: the camera, as
    render_views takes it; step, white_bkgd, terminate, skip: as render.
    A step costs one march and one ray-gradient launch, no network.  The loss is only piecewise smooth in the pose and the descent is
    local: it converges from a start inside the basin of the true pose (profiles/baked_notes.md, "Ray gradients and registration").
    -> (poses (NV,4,4), losses: the `steps` losses as floats, read once at the end)"""
    if not isinstance(volume, _Baked):
        raise TypeError(f"register: expected a baked volume, got {type(volume).__name__}")
    if not isinstance(poses0, torch.Tensor) or poses0.dim() != 3 or tuple(poses0.shape[1:]) != (4, 4):
        raise ValueError("register: poses0 must be (NV,4,4)")
    W, H, NV, steps = int(W), int(H), poses0.shape[0], int(steps)
    if not isinstance(target_rgb, torch.Tensor) or tuple(target_rgb.shape) != (NV, H, W, 3):
        raise ValueError(f"register: target_rgb must be (NV,H,W,3) = {(NV, H, W, 3)}, got "
                         f"{tuple(target_rgb.shape) if isinstance(target_rgb, torch.Tensor) else type(target_rgb).__name__}")
    if steps < 0:
        raise ValueError(f"register: steps must be >= 0, got {steps}")
    poses0, target = poses0.detach().float(), target_rgb.detach().float()
    w = torch.zeros((NV, 3), dtype=torch.float32, device=poses0.device, requires_grad=True)
    v = torch.zeros((NV, 3), dtype=torch.float32, device=poses0.device, requires_grad=True)
    optimiser = torch.optim.Adam([w, v], lr=float(lr))
    losses = []
    for _ in range(steps):
        out = volume.render_views_diff(moved_poses(poses0, w, v), W, H, focal, z_near, z_far, c=c, step=step, white_bkgd=white_bkgd,
                                       terminate=terminate, skip=skip)
        loss = ((out.rgb - target) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        loss.backward()
        optimiser.step()
        losses.append(loss.detach())
    with torch.no_grad():
        poses = moved_poses(poses0, w, v)
    return poses, (torch.stack(losses).tolist() if losses else [])


# ---------------------------------------------------------------- placing: gradients with respect to the objects' poses

def place(scene, target_rgb, cam_poses, W, H, focal, z_near, z_far, c=None, objects=None, steps=200, lr=1e-2, step=None,
          white_bkgd=False, terminate=None, skip=True):
    """Place objects of a scene against images: Adam on a 6-DoF update per moved object, P_j = [R(w_j) R0_j | t0_j + v_j] with w an
    axis-angle vector through `rodrigues` and v a translation, both starting at 0 (`moved_poses`: the object turns about its own
    origin), loss = mean((rgb - target_rgb)^2) over all pixels of all views, rgb = scene.render_views_diff(cam_poses, ...,
    obj_poses=P).rgb.  scene: a BakedScene of any kind, fp32 or fp16 (it is not changed); target_rgb (NV,H,W,3); cam_poses (NV,4,4)
    camera-to-world, fixed; W, H, focal, z_near, z_far, c: the camera, as render_views takes it; objects: the indices of the
    objects that move (None: all) -- the others keep their poses bit for bit; step, white_bkgd, terminate, skip: as render.
    A step costs one scene march, one pnr_baked_scene_backward_views call and one host read of the poses; no network.  The loss is
    only piecewise smooth in a pose and the descent is local: it converges from a start inside the basin of the true pose
    (profiles/baked_notes.md, "Scene gradients and placing objects").
    -> (a BakedScene with the new poses -- the volumes are shared --, losses: the `steps` losses as floats, read once at the end)"""
    if not isinstance(scene, BakedScene):
        raise TypeError(f"place: expected a BakedScene, got {type(scene).__name__}")
    if not isinstance(cam_poses, torch.Tensor) or cam_poses.dim() != 3 or tuple(cam_poses.shape[1:]) != (4, 4):
        raise ValueError("place: cam_poses must be (NV,4,4)")
    W, H, NV, steps, N = int(W), int(H), cam_poses.shape[0], int(steps), len(scene)
    if not isinstance(target_rgb, torch.Tensor) or tuple(target_rgb.shape) != (NV, H, W, 3):
        raise ValueError(f"place: target_rgb must be (NV,H,W,3) = {(NV, H, W, 3)}, got "
                         f"{tuple(target_rgb.shape) if isinstance(target_rgb, torch.Tensor) else type(target_rgb).__name__}")
    if steps < 0:
        raise ValueError(f"place: steps must be >= 0, got {steps}")
    moved = list(range(N)) if objects is None else [int(j) for j in objects]
    if not moved or len(set(moved)) != len(moved) or not all(0 <= j < N for j in moved):
        raise ValueError(f"place: objects must be distinct indices into a scene of {N} (None: all), got {objects}")
    cam_poses, target = cam_poses.detach().float(), target_rgb.detach().float()
    poses0 = scene.poses[:, :3].clone()  # (N,3,4) on the host, where the kernels take them from
    w = torch.zeros((len(moved), 3), dtype=torch.float32, requires_grad=True)
    v = torch.zeros((len(moved), 3), dtype=torch.float32, requires_grad=True)

    def current():
        poses = poses0.clone()
        poses[moved] = moved_poses(poses0[moved], w, v)
        return poses

    optimiser = torch.optim.Adam([w, v], lr=float(lr))
    losses = []
    for _ in range(steps):
        out = scene.render_views_diff(cam_poses, W, H, focal, z_near, z_far, c=c, obj_poses=current(), step=step, white_bkgd=white_bkgd,
                                      terminate=terminate, skip=skip)
        loss = ((out.rgb - target) ** 2).mean()
        optimiser.zero_grad(set_to_none=True)
        loss.backward()
        optimiser.step()
        losses.append(loss.detach())
    with torch.no_grad():
        poses = scene.poses.clone()
        poses[:, :3] = current()
    return BakedScene(scene.volumes, poses), (torch.stack(losses).tolist() if losses else [])
