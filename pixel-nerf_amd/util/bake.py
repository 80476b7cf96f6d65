"""
Baked volume of one encoded object: the network evaluated ONCE on the points of a grid, for colour as well as density, and any number
of views ray-marched from the grid alone (pnr_baked_render_rays / pnr_baked_render_views, include/pixelnerf_hip.h "baked volumes").
The reference has no counterpart: every pixel it renders pays for 64 + 128 evaluations of the network.  For previews, orbit videos
(eval/gen_video.py's use), picking cameras and sanity checks during training.

The image is an APPROXIMATION of the network's render: trilinear in space, one view direction per grid point, equidistant samples
(no importance sampling).  It is separate from NeRFRenderer: nothing there changes.  After a weight update, bake again (from_model).

The grid is the one util.recon.marching_cubes and util.occupancy.OccupancyGrid use (points of ops.gen_grid_points, cells of the TRUE
spacing (c2 - c1) / (reso - 1)); the skip grid of a volume is an OccupancyGrid of its sigma channel with dilate 0.
"""
import warnings

import torch

from .dotmap import DotMap
from .occupancy import OccupancyGrid, _check_geometry


class BakedVolume:
    """vol: (nx,ny,nz,4) fp32 on the device, (r, g, b, sigma) at the points of ops.gen_grid_points(c1, c2, reso) -- the network's
    outputs (rgb after the sigmoid, sigma after the relu); reso, c1, c2: the grid; skip_threshold and occupancy: the
    OccupancyGrid (dilate 0) of vol[..., 3] that `render(skip=True)` marches against -- at threshold 0 the skipped render equals the
    unskipped one bit for bit, above 0 the image changes where the dropped haze was visible (OccupancyGrid's contract)."""

    def __init__(self, vol, c1, c2, skip_threshold=0.0, keep_largest=None, min_voxels=None):
        from .. import _lib
        if not isinstance(vol, torch.Tensor) or vol.dim() != 4 or vol.shape[3] != 4 or vol.dtype != torch.float32:
            raise ValueError("BakedVolume: vol must be a (nx,ny,nz,4) float32 tensor")
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
        self.occupancy = OccupancyGrid.from_density(vol[..., 3].contiguous(), c1, c2, skip_threshold, dilate=0, keep_largest=keep_largest,
                                                    min_voxels=min_voxels)

    @classmethod
    def from_tensor(cls, vol, c1, c2, skip_threshold=0.0):
        """wrap a caller-made volume: vol (nx,ny,nz,4) fp32 HIP tensor spanning [c1, c2]"""
        return cls(vol, c1, c2, skip_threshold)

    @classmethod
    def from_model(cls, net, c1, c2, reso, coarse=None, viewdirs="origin", eval_batch_size=100000, skip_threshold=0.0,
                   keep_largest=None, min_voxels=None):
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
        A non-finite value in the volume raises ValueError."""
        from .. import ops
        what = "BakedVolume.from_model"
        if int(getattr(net, "num_objs", 1) or 1) > 1:
            raise ValueError(f"{what}: the network encoded {int(net.num_objs)} objects; encode one object")
        reso, c1, c2, _ = _check_geometry(reso, c1, c2, 0)
        use_viewdirs = bool(getattr(net, "use_viewdirs", False))
        origin = isinstance(viewdirs, str)
        if origin and viewdirs != "origin":
            raise ValueError(f"{what}: viewdirs must be 'origin' or a 3-vector, got {viewdirs!r}")
        device = next(net.parameters()).device
        const_dir = None
        if not origin:
            const_dir = torch.as_tensor(viewdirs, dtype=torch.float32).flatten()
            if const_dir.numel() != 3 or not bool(torch.isfinite(const_dir).all()) or float(const_dir.norm()) == 0.0:
                raise ValueError(f"{what}: a constant view direction must be a finite non-zero 3-vector")
            const_dir = (const_dir / const_dir.norm()).to(device)
        if use_viewdirs and origin:
            warnings.warn("Running marching cubes with fake view dirs (pointing to origin), output may be invalid")
        if coarse is None:
            coarse = getattr(net, "mlp_fine", None) is None
        chunk = max(2, int(eval_batch_size) // 2 * 2)
        total = reso[0] * reso[1] * reso[2]
        is_train = bool(getattr(net, "training", False))
        if hasattr(net, "eval"):
            net.eval()
        try:
            with torch.no_grad():
                vol = torch.empty((total, 4), dtype=torch.float32, device=device)
                for first in range(0, total, chunk):
                    count = min(chunk, total - first)
                    pnts, vd = ops.gen_grid_points(c1, c2, reso, first, count, device=device, viewdirs=use_viewdirs and origin)
                    if use_viewdirs and not origin:
                        vd = const_dir.expand(count, 3).contiguous()
                    out = net(pnts[None], coarse=bool(coarse), viewdirs=vd[None] if use_viewdirs else None)
                    vol[first:first + count] = out.reshape(count, -1)[:, :4]
        finally:
            if is_train:
                net.train()
        return cls(vol.view(*reso, 4), c1, c2, skip_threshold, keep_largest=keep_largest, min_voxels=min_voxels)

    @property
    def cell_size(self):
        return tuple((hi - lo) / (n - 1) for lo, hi, n in zip(self.c1, self.c2, self.reso))

    def _march_args(self, step, terminate, skip):
        step = min(self.cell_size) if step is None else float(step)
        return step, (0.0 if terminate is None else float(terminate)), (self.occupancy.bits if skip else None)

    def render(self, rays, step=None, white_bkgd=False, terminate=None, skip=True):
        """rays (...,8) on the volume's device -> DotMap(rgb (...,3), depth (...), alpha (...)); ops.baked_render.
        :param step the sample distance in the units of z; None: the smallest cell edge
        :param terminate eps in [0, 1): a ray stops once its transmittance, checked every 64 samples, is <= eps (every channel and
        alpha move by at most eps, depth by at most eps far); None / 0: off
        :param skip march against the skip grid (exact at skip_threshold 0)"""
        from .. import ops
        if not isinstance(rays, torch.Tensor) or rays.dim() < 1 or rays.shape[-1] != 8:
            raise ValueError("BakedVolume.render: rays must be (...,8)")
        lead = tuple(rays.shape[:-1])
        step, terminate, bits = self._march_args(step, terminate, skip)
        with torch.no_grad():
            rgb, depth, alpha = ops.baked_render(rays.reshape(-1, 8).float(), self.vol, self.reso, self.c1, self.c2, step, bits=bits,
                                                 white_bkgd=white_bkgd, terminate=terminate)
        return DotMap(rgb=rgb.reshape(*lead, 3), depth=depth.reshape(lead), alpha=alpha.reshape(lead))

    def render_views(self, poses_c2w, W, H, focal, z_near, z_far, c=None, gt_rgb=None, want_u8=False, step=None, white_bkgd=False,
                     terminate=None, skip=True):
        """Every pixel of the target views from their cameras, with NeRFRenderer.render_views' epilogue on the device: poses_c2w
        (NVt,4,4) camera-to-world, focal a scalar or (fx, fy), c (cx, cy) or None = the image centre; step, terminate, skip as
        render.  The rays are regenerated in the kernel: the same bits as render(util.gen_rays(...)), no ray array.
        :return DotMap: rgb (NVt,H,W,3), depth and alpha (NVt,H,W), unclamped; depth_norm = (depth - z_near) / (z_far - z_near);
        rgb_u8 with want_u8; with gt_rgb (NVt,H,W,3) in [0,1] psnr and ssim (NVt,) float64 of clamp(rgb, 0, 1)"""
        from .. import ops
        if not isinstance(poses_c2w, torch.Tensor) or poses_c2w.dim() != 3 or tuple(poses_c2w.shape[1:]) != (4, 4):
            raise ValueError("BakedVolume.render_views: poses_c2w must be (NVt,4,4)")
        W, H, NVt = int(W), int(H), poses_c2w.shape[0]
        if torch.is_tensor(focal):
            focal = focal.flatten().tolist()
            focal = focal[0] if len(focal) == 1 else (focal[0], focal[1])
        if torch.is_tensor(c):
            c = c.flatten().tolist()
        if gt_rgb is not None and tuple(gt_rgb.shape) != (NVt, H, W, 3):
            raise ValueError(f"BakedVolume.render_views: gt_rgb must be (NVt,H,W,3) = {(NVt, H, W, 3)}, got {tuple(gt_rgb.shape)}")
        step, terminate, bits = self._march_args(step, terminate, skip)
        with torch.no_grad():
            rgb, depth, alpha = ops.baked_render_views(poses_c2w.float(), W, H, focal, c, z_near, z_far, self.vol, self.reso, self.c1,
                                                       self.c2, step, bits=bits, white_bkgd=white_bkgd, terminate=terminate)
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

    def state_dict(self):
        """the volume, the geometry and the skip threshold; the skip grid is rebuilt on load"""
        return {"vol": self.vol, "c1": torch.tensor(self.c1, dtype=torch.float64), "c2": torch.tensor(self.c2, dtype=torch.float64),
                "skip_threshold": torch.tensor(self.skip_threshold, dtype=torch.float64)}

    @classmethod
    def from_state_dict(cls, state, device=None):
        """:param device where to put the volume; None: where state["vol"] lives"""
        vol = state["vol"] if device is None else state["vol"].to(device)
        return cls(vol, state["c1"].tolist(), state["c2"].tolist(), float(state["skip_threshold"]))
