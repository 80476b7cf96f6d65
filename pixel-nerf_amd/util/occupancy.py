"""
Occupancy grid of one encoded object: which cells of a density grid hold anything, as a bitfield on the device, and the rays
of a render classified against it (pnr_occupancy_build / pnr_occupancy_clip_rays, include/pixelnerf_hip.h).  The reference has no
counterpart: it evaluates 64 + 128 network samples on every ray, also on those that look through empty space.  Hand an
OccupancyGrid to `NeRFRenderer.forward(..., occupancy=)` / `render_views(..., occupancy=)` and only the rays that pass through an
occupied cell are rendered; the others get what the compositing yields for sigma == 0 (src/render/nerf.py:223-249).

The grid is the one util.recon.marching_cubes evaluates (src/util/recon.py:43-66; points of util.gen_grid, src/util/util.py:93-110),
with cells of the TRUE spacing (c2 - c1) / (reso - 1).
"""
import torch


class OccupancyGrid:
    """bits: (ceil(cells / 32),) int32 words on the device (cell (i,j,k) = bit (index & 31) of word (index >> 5), index =
    (i (ny-1) + j)(nz-1) + k); reso: grid POINTS per axis (cells: reso - 1); c1, c2: corners of the grid; threshold, dilate: what
    the bits were built with; n_occupied: 0-d int32 device tensor (`occupied_fraction` reads it: one host synchronisation);
    info: None, or util.recon.remove_floaters' dict when the grid was built with keep_largest / min_voxels."""

    def __init__(self, bits, reso, c1, c2, threshold, dilate, n_occupied):
        reso, c1, c2, words = _check_geometry(reso, c1, c2, dilate)
        if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or tuple(bits.shape) != (words,):
            raise ValueError(f"OccupancyGrid: bits must be the ({words},) int32 tensor of ops.occupancy_build for reso {reso}")
        self.bits, self.reso, self.c1, self.c2 = bits, reso, c1, c2
        self.threshold, self.dilate, self.n_occupied = float(threshold), int(dilate), n_occupied
        self.info = None

    @classmethod
    def from_density(cls, field, c1, c2, threshold, dilate=1, keep_largest=None, min_voxels=None):
        """field (nx,ny,nz) fp32 HIP tensor: sigma at the points of ops.gen_grid_points(c1, c2, (nx,ny,nz)).  A cell is occupied
        iff a cell with a corner > threshold (or a non-finite corner) lies within Chebyshev distance `dilate`.
        keep_largest / min_voxels (both None: off) ask for "the object only": the connected components of the grid POINTS
        > threshold are taken BEFORE dilation (util.recon.remove_floaters: a component is kept iff it has at least min_voxels
        points AND is among the keep_largest biggest), the points of a dropped component are set to `threshold`, then the build
        above runs; `info` carries remove_floaters' counts.  Non-finite points are outside for the labelling and are left
        untouched: the build still counts them as occupied, culling keeps erring towards rendering.  This CHANGES THE IMAGE
        wherever the dropped haze was visible -- that is the point of asking for it; without the two arguments a culled render
        stays exact where kept."""
        from .. import ops
        from . import recon
        if not isinstance(field, torch.Tensor) or field.dim() != 3:
            raise ValueError("OccupancyGrid.from_density: field must be a (nx,ny,nz) tensor")
        _check_geometry(field.shape, c1, c2, dilate)  # (before any device work)
        field, info = recon.remove_floaters(field, threshold, keep_largest=keep_largest, min_voxels=min_voxels)
        bits, count = ops.occupancy_build(field, threshold, dilate)
        grid = cls(bits, field.shape, c1, c2, threshold, dilate, count)
        grid.info = info
        return grid

    @classmethod
    def from_model(cls, net, c1, c2, reso, threshold, dilate=1, eval_batch_size=100000, keep_largest=None, min_voxels=None):
        """The grid of an encoded object from its networks: the field is the element-wise MAXIMUM of the coarse and the fine
        network's sigma (the coarse pass decides where the fine samples go, the fine pass decides the pixel; the coarse network's
        alone when net.mlp_fine is None), evaluated exactly as util.recon.marching_cubes evaluates its field (recon.density_grid:
        fake view directions with their warning, (1,N,3) calls, ONE encoded object, train / eval flag restored).
        threshold: a sigma, e.g. the reference's iso-level 50 (src/util/recon.py:17) or a fraction of it.
        keep_largest / min_voxels: as from_density (drops the haze's components; changes the image where it was visible)."""
        from . import recon
        passes = (True, False) if getattr(net, "mlp_fine", None) is not None else (True,)
        sigmas, reso = recon.density_grid(net, c1, c2, reso, coarse=passes, eval_batch_size=eval_batch_size,
                                          what="OccupancyGrid.from_model")
        return cls.from_density(sigmas.view(*reso), c1, c2, threshold, dilate, keep_largest=keep_largest, min_voxels=min_voxels)

    def clip_rays(self, rays, pad=0.0):
        """rays (...,8) on the grid's device -> (t_bounds (...,2) fp32, hit (...) int32); ops.occupancy_clip_rays"""
        from .. import ops
        if not isinstance(rays, torch.Tensor) or rays.dim() < 1 or rays.shape[-1] != 8:
            raise ValueError("OccupancyGrid.clip_rays: rays must be (...,8)")
        lead = tuple(rays.shape[:-1])
        t_bounds, hit = ops.occupancy_clip_rays(rays.reshape(-1, 8).float(), self.bits, self.reso, self.c1, self.c2, pad)
        return t_bounds.reshape(*lead, 2), hit.reshape(lead)

    def mark_samples(self, rays, z):
        """rays (R,8), z (R,K) on the grid's device -> keep (R,K) uint8: 1 iff the sample o + z d lies in an occupied cell of the
        grid (outside the box: 0; not classifiable: 1); ops.occupancy_mark_samples"""
        from .. import ops
        return ops.occupancy_mark_samples(rays, z, self.bits, self.reso, self.c1, self.c2)

    @property
    def n_cells(self):
        return (self.reso[0] - 1) * (self.reso[1] - 1) * (self.reso[2] - 1)

    @property
    def occupied_fraction(self):
        return float(int(self.n_occupied)) / self.n_cells


def _check_geometry(reso, c1, c2, dilate):
    """-> (reso, c1, c2 as tuples, number of 32-bit words of the bitfield); ValueError for what the C entries refuse"""
    reso = tuple(int(r) for r in reso)
    c1, c2 = tuple(float(v) for v in c1), tuple(float(v) for v in c2)
    if len(reso) != 3 or len(c1) != 3 or len(c2) != 3:
        raise ValueError("OccupancyGrid: c1, c2, reso must have 3 entries each")
    if any(r < 2 for r in reso):
        raise ValueError(f"OccupancyGrid: every axis needs at least 2 grid points, got reso {reso}")
    if not all(lo < hi for lo, hi in zip(c1, c2)):
        raise ValueError(f"OccupancyGrid: c1 must be below c2 on every axis, got {c1} .. {c2}")
    if not 0 <= int(dilate) <= 4:
        raise ValueError(f"OccupancyGrid: dilate must be in [0, 4], got {dilate}")
    cells = (reso[0] - 1) * (reso[1] - 1) * (reso[2] - 1)
    if cells >= 2 ** 31:
        raise ValueError(f"OccupancyGrid: the grid must have fewer than 2^31 cells, got reso {reso}")
    return reso, c1, c2, (cells + 31) // 32
