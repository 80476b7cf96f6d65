"""
torch.Tensor front-end of the baked volumes (include/pixelnerf_hip.h, "baked volumes" and the sections after it): the marches, the
scenes of several posed volumes, their gradients, visibility, resampling and the total-variation prior.  Every public name here is
re-exported by ops.py: `ops.baked_render` is `ops_baked.baked_render`.  Nothing in this module has a CPU or eager-PyTorch fallback.
"""
import ctypes
import math

import torch

from . import _lib
from ._ops_common import _check_grid_args, _f32, _float3_pair, _image_size, _intrinsics, _p, _stream


def _baked_march_args(what, reso, c1, c2, step, terminate):
    """the geometry and the march settings every baked render shares, checked before any device work -> ((nx, ny, nz), step, terminate)"""
    lib = _lib.load()
    if len(reso) != 3 or len(c1) != 3 or len(c2) != 3:
        raise ValueError(f"{what}: c1, c2, reso must have 3 entries each")
    nx, ny, nz = (int(r) for r in reso)
    if lib.pnr_occupancy_bytes(nx, ny, nz) == 0:
        raise ValueError(f"{what}: a grid needs at least 2 points per axis and fewer than 2^31 cells, got {(nx, ny, nz)}")
    if not all(math.isfinite(float(a)) and math.isfinite(float(b)) and float(a) < float(b) for a, b in zip(c1, c2)):
        raise ValueError(f"{what}: c1 must be below c2 on every axis, both finite, got {tuple(c1)} .. {tuple(c2)}")
    step, terminate = float(step), float(terminate)
    if not (math.isfinite(step) and step > 0.0):
        raise ValueError(f"{what}: step must be finite and > 0, got {step}")
    if not 0.0 <= terminate < 1.0:
        raise ValueError(f"{what}: terminate must lie in [0, 1), got {terminate}")
    return (nx, ny, nz), step, terminate


def _stored_tail(what, degree, name="stored", dtype=None):
    """degree None / -1 (RGBA; not for a "coef"), 0, 1 or 2, checked -> (degree as the library takes it, the shape of a row).
    `name` and `dtype` (_baked_volume's) only word the refusal"""
    rgba = name != "coef"
    degree = -1 if degree is None and rgba else int(degree)
    if degree not in (0, 1, 2) and (degree != -1 or not rgba):
        allowed = f"None / -1 (RGBA{' rows' if dtype == torch.float32 and name == 'rows' else ''}), 0, 1 or 2" if rgba else "0, 1 or 2"
        raise ValueError(f"{what}: degree must be {allowed}, got {degree}")
    return degree, ((4,) if degree < 0 else ((degree + 1) ** 2, 4))


def _check_index(what, index, dims, dev):
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or tuple(index.shape) != dims or index.device != dev:
        raise ValueError(f"{what}: index must be the {dims} int32 tensor of sparse_points on {dev}")


def _is_buffer(t, shape, dev=None):
    """a contiguous fp32 tensor of `shape` (on `dev`, when given) that does not require grad: what a kernel may accumulate into"""
    return isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape) and (dev is None or t.device == dev) \
        and t.is_contiguous() and not t.requires_grad


def _check_added_into(what, name, buf, shape, dev):
    if not _is_buffer(buf, shape, dev):
        raise ValueError(f"{what}: {name} must be a contiguous float32 tensor of shape {tuple(shape)} on {dev} that does not require "
                         "grad (it is added into)")


def _baked_volume(what, stored, degree, reso, c1, c2, step, bits, terminate, *, dtype=None, name=None, index=None, sparse=False):
    """The stored tensor of any baked march, its geometry and the march settings, checked before any device work.  `name` is what
    the caller's signature calls the tensor, and with `dtype` it says what the tensor may be: "vol" in fp32 is baked_render's RGBA
    volume (nx,ny,nz,4), which takes no degree; "coef" (nx,ny,nz,B,4) at degree 0, 1, 2; an fp16 "vol" or "rows" at degree None /
    -1 (RGBA: no B axis) or 0, 1, 2; `sparse`: (M,...) kept rows, with `index` (nx,ny,nz) int32 and bits both mandatory.  Without a
    `name` -- the entries that take `stored` in either dtype and either layout -- the tensor is "rows", sparse, when there is an index
    and "stored" otherwise, in the dtype it has.
    -> the checked volume every launcher takes, a plain tuple that each unpacks ONCE, in this order (a named tuple costs a call
    0.6 us more, profiles/baked_notes.md): what, name, stored (contiguous), degree (-1 for RGBA; None: the entry takes none), dims,
    c1, c2, step, terminate, bits, index (None: not sparse)"""
    if name is None:
        sparse = index is not None
        name = "rows" if sparse else "stored"
        dtype = torch.float16 if isinstance(stored, torch.Tensor) and stored.dtype == torch.float16 else torch.float32
    takes_degree = not (name == "vol" and dtype == torch.float32)
    tail = (4,)
    if takes_degree:
        degree, tail = _stored_tail(what, degree, name, dtype)
        lead = 1 if sparse else 3
        if not isinstance(stored, torch.Tensor) or stored.dim() != lead + len(tail) or tuple(stored.shape[lead:]) != tail:
            raise ValueError(f"{what}: {name} must be ({'M' if sparse else 'nx,ny,nz'},{','.join(str(s) for s in tail)}) at degree {degree}"
                             f", got {tuple(stored.shape) if isinstance(stored, torch.Tensor) else type(stored).__name__}")
        if name == "coef" and (len(reso) != 3 or tuple(int(r) for r in reso) != tuple(stored.shape[:3])):
            raise ValueError(f"{what}: coef spans {tuple(stored.shape[:3])} points, reso says {tuple(reso)}")
    dims, step, terminate = _baked_march_args(what, reso, c1, c2, step, terminate)
    if sparse and (bits is None or index is None):
        raise ValueError(f"{what}: index and bits are mandatory (a sparse volume has nothing to march unskipped)")
    stored = _f32(stored, name, ((None,) if sparse else dims) + tail, dtype)
    if stored.numel() and stored.data_ptr() % 16:
        raise ValueError(f"{what}: {name} must be 16-byte aligned")
    if bits is not None:
        _check_grid_args(what, bits, dims, c1, c2, stored.device)
    if sparse:
        _check_index(what, index, dims, stored.device)
    return what, name, stored, (degree if takes_degree else None), dims, c1, c2, step, terminate, bits, (index if sparse else None)


def _lives(name, stored, camera):
    """how a refusal names a march's volume and where it lives, in the words of the caller's signature"""
    if camera is not None and stored.dtype == torch.float16:
        return "the volume lives"
    return f"{name} {'live' if name == 'rows' else 'lives'}"


def _ray_source(what, subject, volume_dev, rays=None, camera=None, detach=False, convert_first=False):
    """The head of a baked entry's argument list: `rays` (R,8), or `camera` = (poses (NV,4,4), W, H, focal, c, z_near, z_far), which
    must live on `volume_dev`.  subject: the words of the refusal for what lives there ("the volumes live"), or a function that
    gives them (they are wanted only then).  detach: the entry differentiates the source itself, so the gradient goes to what the
    caller holds.  convert_first: the scenes' order -- focal, c, z_near, z_far become numbers before the devices are compared.
    -> (args, R, device, the contiguous rays / poses: keep it alive over the call)"""
    given = rays if camera is None else camera[0]
    if detach and isinstance(given, torch.Tensor):
        given = given.detach()
    if camera is None:
        source = _f32(given, "rays", (None, 8))
        R = source.shape[0]
        args = [_p(source), R]
    else:
        _, W, H, focal, c, z_near, z_far = camera
        source = _f32(given, "poses", (None, 4, 4))
        R = source.shape[0] * H * W
        args = [_p(source), source.shape[0], W, H, *_intrinsics(focal, c, W, H), float(z_near), float(z_far)] if convert_first else None
    dev = source.device
    if volume_dev != dev:
        raise ValueError(f"{what}: {subject if isinstance(subject, str) else subject()} on {volume_dev}, "
                         f"the {'rays' if camera is None else 'poses'} on {dev}")
    if args is None:
        args = [_p(source), source.shape[0], W, H, *_intrinsics(focal, c, W, H), float(z_near), float(z_far)]
    return args, R, dev, source


def _upstream(what, d_rgb, d_depth, d_alpha, R, dev, where):
    """the upstream gradients of a march's outputs, each None (zeros) or fp32 of the output's shape, detached, on `dev` -- `where`
    names what lives there in the caller's words -> [d_rgb, d_depth, d_alpha]"""
    grads = []
    for g, name, shape in ((d_rgb, "d_rgb", (R, 3)), (d_depth, "d_depth", (R,)), (d_alpha, "d_alpha", (R,))):
        g = None if g is None else _f32(g.detach() if isinstance(g, torch.Tensor) else g, name, shape)
        if g is not None and g.device != dev:
            raise ValueError(f"{what}: {name} lives on {g.device}, {where} on {dev}")
        grads.append(g)
    return grads


def _volume_args(v, half=None):
    """the volume part of a backward or visibility entry's argument list: stored, [half], M, degree, index, bits, dims, c1, c2"""
    _, _, stored, degree, dims, c1, c2, _, _, bits, index = v
    lo, hi = _float3_pair(c1, c2)
    return [_p(stored) if stored.numel() else None, *(() if half is None else (int(half),)), stored.shape[0] if index is not None else 0,
            degree, None if index is None else _p(index.contiguous()), None if bits is None else _p(bits.contiguous()), *dims, lo, hi]


def _baked_launch(entry, v, white_bkgd, rays=None, camera=None):
    """March the checked volume `v` (_baked_volume) through the library entry `entry`, along `rays` (R,8) or over the pixels of
    `camera` = (poses (NV,4,4), W, H, focal, c, z_near, z_far) -> (rgb (R,3), depth (R,), alpha (R,)) fp32, R = NV H W for a camera"""
    lib = _lib.load()
    what, name, stored, degree, dims, c1, c2, step, terminate, bits, index = v
    args, R, dev, source = _ray_source(what, lambda: _lives(name, stored, camera), stored.device, rays, camera)  # (source: kept alive)
    rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((R,), dtype=torch.float32, device=dev)
    alpha = torch.empty((R,), dtype=torch.float32, device=dev)
    lo, hi = _float3_pair(c1, c2)
    if index is None:
        args.append(_p(stored))
    else:
        M = stored.shape[0]
        args += (_p(stored) if M else None, M)
    if degree is not None:
        args.append(degree)
    if index is not None:
        args.append(_p(index.contiguous()))
    args += (None if bits is None else _p(bits.contiguous()), *dims, lo, hi, step, int(bool(white_bkgd)), terminate,
             _p(rgb), _p(depth), _p(alpha))
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    return rgb, depth, alpha


def baked_render(rays, vol, reso, c1, c2, step, bits=None, white_bkgd=False, terminate=0.0):
    """Rays through a baked RGBA volume (pnr_baked_render_rays; the contract is in include/pixelnerf_hip.h, "baked volumes"): rays
    (R,8), vol (nx,ny,nz,4) fp32 HIP tensors -- (r, g, b, sigma) at the points of gen_grid_points(c1, c2, reso) --, step > 0 the sample
    distance in the units of z, bits None or occupancy_build's bitfield of the same grid (a sample in a cell whose bit is off has
    sigma = 0), terminate eps in [0, 1) (0: off).  -> (rgb (R,3), depth (R,), alpha (R,)) fp32.  No network, no host synchronisation,
    the same bytes on every call."""
    v = _baked_volume("baked_render", vol, None, reso, c1, c2, step, bits, terminate, dtype=torch.float32, name="vol")
    return _baked_launch("pnr_baked_render_rays", v, white_bkgd, rays=rays)


def baked_render_views(poses, width, height, focal, c, z_near, z_far, vol, reso, c1, c2, step, bits=None, white_bkgd=False,
                       terminate=0.0):
    """baked_render over every pixel of the views of gen_rays(poses, width, height, focal, z_near, z_far, c) (pnr_baked_render_views):
    poses (NV,4,4) camera-to-world, focal a scalar or (fx, fy), c (cx, cy) or None = the image centre.  The rays are regenerated
    in the kernel -- the same bits as baked_render(gen_rays(...)), and no ray array is written.
    -> (rgb (NV*H*W,3), depth (NV*H*W,), alpha (NV*H*W,)) fp32, rays ordered (view, row, column)."""
    W, H = _image_size("baked_render_views", width, height)
    v = _baked_volume("baked_render_views", vol, None, reso, c1, c2, step, bits, terminate, dtype=torch.float32, name="vol")
    return _baked_launch("pnr_baked_render_views", v, white_bkgd, camera=(poses, W, H, focal, c, z_near, z_far))


def baked_sh_render(rays, coef, degree, reso, c1, c2, step, bits=None, white_bkgd=False, terminate=0.0):
    """baked_render through a view-dependent volume (pnr_baked_sh_render_rays; include/pixelnerf_hip.h, "baked volumes"): coef
    (nx,ny,nz,B,4) fp32 HIP tensor, B = (degree+1)^2 real spherical-harmonic coefficients of (r, g, b, sigma) per grid point, degree
    0, 1 or 2; every corner is evaluated for the ray's own direction and clamped before the blend.  Everything else as baked_render.
    -> (rgb (R,3), depth (R,), alpha (R,)) fp32."""
    v = _baked_volume("baked_sh_render", coef, degree, reso, c1, c2, step, bits, terminate, dtype=torch.float32, name="coef")
    return _baked_launch("pnr_baked_sh_render_rays", v, white_bkgd, rays=rays)


def baked_sh_render_views(poses, width, height, focal, c, z_near, z_far, coef, degree, reso, c1, c2, step, bits=None, white_bkgd=False,
                          terminate=0.0):
    """baked_render_views through a view-dependent volume (pnr_baked_sh_render_views): the same bits as
    baked_sh_render(gen_rays(...)), no ray array.  -> (rgb (NV*H*W,3), depth (NV*H*W,), alpha (NV*H*W,)) fp32."""
    W, H = _image_size("baked_sh_render_views", width, height)
    v = _baked_volume("baked_sh_render_views", coef, degree, reso, c1, c2, step, bits, terminate, dtype=torch.float32, name="coef")
    return _baked_launch("pnr_baked_sh_render_views", v, white_bkgd, camera=(poses, W, H, focal, c, z_near, z_far))


def sparse_points(bits, reso):
    """The kept set of a sparse baked volume (pnr_sparse_points_mark; the definition is in include/pixelnerf_hip.h, "baked volumes"):
    bits from occupancy_build of a field with `reso` = (nx,ny,nz) points -> (index (nx,ny,nz) int32 -- the rank of a kept point
    among the kept ones, -1 elsewhere --, ids (M,) int32 -- the kept linear ids (i ny + j) nz + k, ascending).  Kept: the corners of
    the occupied cells, closed over the pairs (2j, 2j+1) of the linear ids.  The mark is the kernel's; the prefix sum behind index
    and ids is torch's, and sizing ids costs one host read of M (as compact_samples)."""
    lib = _lib.load()
    if not isinstance(bits, torch.Tensor):
        raise TypeError("bits: expected a torch.Tensor")
    if not bits.is_cuda:
        raise _lib.PixelNerfHipError(f"bits: tensor must live on a HIP device (got {bits.device}); pixelnerf_amd has no CPU path")
    if len(reso) != 3:
        raise ValueError("sparse_points: reso must have 3 entries")
    dev = bits.device
    nx, ny, nz = _check_grid_args("sparse_points", bits, reso, (0.0,) * 3, (1.0,) * 3, dev)
    total = nx * ny * nz
    if total >= 2 ** 31:
        raise ValueError(f"sparse_points: a grid needs fewer than 2^31 points, got {(nx, ny, nz)}")
    keep = torch.empty((total,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pnr_sparse_points_mark(_p(bits.contiguous()), nx, ny, nz, _p(keep), _stream()), "pnr_sparse_points_mark")
    rank = torch.cumsum(keep, dim=0, dtype=torch.int32)  # inclusive: the rank of a kept point is rank - 1
    index = torch.where(keep != 0, rank - 1, torch.full_like(rank, -1))
    M = int(rank[-1])  # the host synchronisation
    ids = torch.nonzero(keep, as_tuple=False).flatten().to(torch.int32) if M else torch.empty((0,), dtype=torch.int32, device=dev)
    return index.view(nx, ny, nz), ids


def gen_grid_points_at(c1, c2, reso, ids, viewdirs=True):
    """gen_grid_points for a LIST of grid points (pnr_gen_grid_points_at): ids (M,) int32 HIP tensor of linear ids (i ny + j) nz + k
    -> (xyz (M,3), viewdirs (M,3) | None) on the ids' device; row m holds the bits of row ids[m] of gen_grid_points(c1, c2, reso),
    an id outside the grid a row of NaN."""
    lib = _lib.load()
    if not isinstance(ids, torch.Tensor):
        raise TypeError("ids: expected a torch.Tensor")
    if not ids.is_cuda:
        raise _lib.PixelNerfHipError(f"ids: tensor must live on a HIP device (got {ids.device}); pixelnerf_amd has no CPU path")
    if ids.dtype != torch.int32 or ids.dim() != 1:
        raise TypeError(f"ids: expected a 1-d int32 tensor, got {ids.dtype} {tuple(ids.shape)}")
    if len(c1) != 3 or len(c2) != 3 or len(reso) != 3:
        raise ValueError("gen_grid_points_at: c1, c2, reso must have 3 entries each")
    ids, dev = ids.contiguous(), ids.device
    xyz = torch.empty((ids.shape[0], 3), dtype=torch.float32, device=dev)
    vd = torch.empty_like(xyz) if viewdirs else None
    lo, hi = (ctypes.c_double * 3)(*[float(v) for v in c1]), (ctypes.c_double * 3)(*[float(v) for v in c2])
    with torch.cuda.device(dev):
        _lib.check(lib.pnr_gen_grid_points_at(lo, hi, (ctypes.c_int * 3)(*[int(r) for r in reso]), _p(ids), ids.shape[0], _p(xyz), _p(vd),
                                              _stream()), "pnr_gen_grid_points_at")
    return xyz, vd


def baked_sparse_render(rays, rows, degree, index, bits, reso, c1, c2, step, white_bkgd=False, terminate=0.0):
    """Rays through a sparse baked volume (pnr_baked_sparse_render_rays; include/pixelnerf_hip.h, "baked volumes"): rows (M,4)
    (degree None: RGBA) or (M,B,4) (degree 0, 1, 2) fp32 HIP tensor -- the rows of the dense volume at the kept points --, index and
    bits as sparse_points took and returned them.  The bytes of baked_render / baked_sh_render on the dense volume with the same
    bits; an index value that names no pair of rows drops its sample (sigma = 0) instead of reading.
    -> (rgb (R,3), depth (R,), alpha (R,)) fp32."""
    v = _baked_volume("baked_sparse_render", rows, degree, reso, c1, c2, step, bits, terminate, dtype=torch.float32,
                      name="rows", index=index, sparse=True)
    return _baked_launch("pnr_baked_sparse_render_rays", v, white_bkgd, rays=rays)


def baked_sparse_render_views(poses, width, height, focal, c, z_near, z_far, rows, degree, index, bits, reso, c1, c2, step,
                              white_bkgd=False, terminate=0.0):
    """baked_render_views through a sparse baked volume (pnr_baked_sparse_render_views): the same bits as
    baked_sparse_render(gen_rays(...)), no ray array.  -> (rgb (NV*H*W,3), depth (NV*H*W,), alpha (NV*H*W,)) fp32."""
    W, H = _image_size("baked_sparse_render_views", width, height)
    v = _baked_volume("baked_sparse_render_views", rows, degree, reso, c1, c2, step, bits, terminate, dtype=torch.float32,
                      name="rows", index=index, sparse=True)
    return _baked_launch("pnr_baked_sparse_render_views", v, white_bkgd, camera=(poses, W, H, focal, c, z_near, z_far))


# ---- half-precision baked volumes: fp16 storage, the fp32 march on the widened values (include/pixelnerf_hip.h, "Half-precision
# baked volumes").  degree None / -1: the RGBA march; 0, 1, 2: the view-dependent one

def baked_half_render(rays, vol, degree, reso, c1, c2, step, bits=None, white_bkgd=False, terminate=0.0):
    """baked_render (degree None / -1: vol (nx,ny,nz,4)) or baked_sh_render (degree 0, 1, 2: vol (nx,ny,nz,B,4)) through an fp16 HIP
    tensor (pnr_baked_half_render_rays): the bytes of that function on vol.float(), every other argument the same.
    -> (rgb (R,3), depth (R,), alpha (R,)) fp32."""
    v = _baked_volume("baked_half_render", vol, degree, reso, c1, c2, step, bits, terminate, dtype=torch.float16, name="vol")
    return _baked_launch("pnr_baked_half_render_rays", v, white_bkgd, rays=rays)


def baked_half_render_views(poses, width, height, focal, c, z_near, z_far, vol, degree, reso, c1, c2, step, bits=None, white_bkgd=False,
                            terminate=0.0):
    """baked_render_views / baked_sh_render_views through an fp16 volume (pnr_baked_half_render_views): the same bits as
    baked_half_render(gen_rays(...)), no ray array.  -> (rgb (NV*H*W,3), depth (NV*H*W,), alpha (NV*H*W,)) fp32."""
    W, H = _image_size("baked_half_render_views", width, height)
    v = _baked_volume("baked_half_render_views", vol, degree, reso, c1, c2, step, bits, terminate, dtype=torch.float16, name="vol")
    return _baked_launch("pnr_baked_half_render_views", v, white_bkgd, camera=(poses, W, H, focal, c, z_near, z_far))


def baked_sparse_half_render(rays, rows, degree, index, bits, reso, c1, c2, step, white_bkgd=False, terminate=0.0):
    """baked_sparse_render through fp16 rows (pnr_baked_sparse_half_render_rays): rows (M,4) (degree None / -1) or (M,B,4) fp16 HIP
    tensor; the bytes of baked_sparse_render on rows.float().  -> (rgb (R,3), depth (R,), alpha (R,)) fp32."""
    v = _baked_volume("baked_sparse_half_render", rows, degree, reso, c1, c2, step, bits, terminate, dtype=torch.float16,
                      name="rows", index=index, sparse=True)
    return _baked_launch("pnr_baked_sparse_half_render_rays", v, white_bkgd, rays=rays)


def baked_sparse_half_render_views(poses, width, height, focal, c, z_near, z_far, rows, degree, index, bits, reso, c1, c2, step,
                                   white_bkgd=False, terminate=0.0):
    """baked_sparse_render_views through fp16 rows (pnr_baked_sparse_half_render_views): the same bits as
    baked_sparse_half_render(gen_rays(...)), no ray array.  -> (rgb (NV*H*W,3), depth (NV*H*W,), alpha (NV*H*W,)) fp32."""
    W, H = _image_size("baked_sparse_half_render_views", width, height)
    v = _baked_volume("baked_sparse_half_render_views", rows, degree, reso, c1, c2, step, bits, terminate, dtype=torch.float16,
                      name="rows", index=index, sparse=True)
    return _baked_launch("pnr_baked_sparse_half_render_views", v, white_bkgd, camera=(poses, W, H, focal, c, z_near, z_far))


def baked_march(source, stored, degree, reso, c1, c2, step, bits=None, index=None, white_bkgd=False, terminate=0.0):
    """The inference march of ANY stored tensor: which of the ten functions above marches follows from the dtype (fp32 / fp16), the
    degree (None / -1: RGBA) and the index (given: the kept rows of a sparse volume), and that function is called, so the checks
    and refusals are its own.  source: (rays (R,8),), or the camera (poses (NV,4,4), W, H, focal, c, z_near, z_far).
    -> (rgb (R,3), depth (R,), alpha (R,)) fp32.  The ten named functions stay the documented forms; this is what autograd and
    util.bake call."""
    views = len(source) != 1
    tail = dict(white_bkgd=white_bkgd, terminate=terminate)
    half = isinstance(stored, torch.Tensor) and stored.dtype == torch.float16
    if index is not None:
        march = (baked_sparse_half_render, baked_sparse_half_render_views) if half else (baked_sparse_render, baked_sparse_render_views)
        return march[views](*source, stored, degree, index, bits, reso, c1, c2, step, **tail)
    if half:
        return (baked_half_render, baked_half_render_views)[views](*source, stored, degree, reso, c1, c2, step, bits=bits, **tail)
    if degree is None or degree < 0:
        return (baked_render, baked_render_views)[views](*source, stored, reso, c1, c2, step, bits=bits, **tail)
    return (baked_sh_render, baked_sh_render_views)[views](*source, stored, degree, reso, c1, c2, step, bits=bits, **tail)


# ---- scenes of several posed baked volumes (include/pixelnerf_hip.h, "Scenes of several baked volumes")

def _baked_pose(what, pose):
    """an object-to-world pose, (3,4) or (4,4), as 12 host floats [R | t] row-major; finite and rigid by the library's rule (fp64 on
    the fp32 numbers: max |R^T R - I| <= 1e-4, det R > 0)"""
    p = torch.as_tensor(pose).detach().to("cpu", torch.float32)
    if tuple(p.shape) not in ((3, 4), (4, 4)):
        raise ValueError(f"{what}: pose must be (3,4) or (4,4) object-to-world, got {tuple(p.shape)}")
    m = p[:3].double()
    if not all(math.isfinite(v) for v in m.flatten().tolist()):
        raise ValueError(f"{what}: pose is not finite")
    rot = m[:, :3]
    if float((rot.T @ rot - torch.eye(3, dtype=torch.float64)).abs().max()) > 1e-4 or not float(torch.linalg.det(rot)) > 0.0:
        raise ValueError(f"{what}: pose is not rigid (max |R^T R - I| <= 1e-4 and det R > 0; no scale, shear or reflection)")
    return p[:3].flatten().tolist()


def _baked_scene(what, objects, step, terminate):
    """the objects of a scene march, checked before any device work -> (the PnrBakedObject array, device, what to keep alive)"""
    if not isinstance(objects, (list, tuple)) or not 1 <= len(objects) <= _lib.BAKED_SCENE_MAX_OBJECTS:
        raise ValueError(f"{what}: objects must be a list of 1 to {_lib.BAKED_SCENE_MAX_OBJECTS} posed volumes, got "
                         f"{len(objects) if isinstance(objects, (list, tuple)) else type(objects).__name__}")
    arr = (_lib.PnrBakedObject * len(objects))()
    keep, kind0, dev, parsed = [], None, None, []
    for j, ob in enumerate(objects):  # what needs no device, for every object first
        if not isinstance(ob, (list, tuple)) or not 6 <= len(ob) <= 8:
            raise ValueError(f"{what}: object {j} must be (stored, degree, reso, c1, c2, pose[, bits[, index]])")
        stored, degree, reso, c1, c2, pose = ob[:6]
        bits = ob[6] if len(ob) > 6 else None
        index = ob[7] if len(ob) > 7 else None
        sparse = index is not None
        if not isinstance(stored, torch.Tensor) or stored.dtype not in (torch.float32, torch.float16):
            raise TypeError(f"{what}: object {j}: stored must be a float32 or float16 torch.Tensor")
        pose12 = _baked_pose(f"{what}: object {j}", pose)
        kind = (-1 if degree is None else int(degree), stored.dtype, sparse)
        if kind0 is None:
            kind0, dev = kind, stored.device
        elif kind != kind0:
            raise ValueError(f"{what}: objects 0 and {j} differ in kind -- (degree, dtype, sparse) {kind0} against {kind} -- and one "
                             "scene holds one kind")
        if stored.device != dev:
            raise ValueError(f"{what}: object {j} lives on {stored.device}, object 0 on {dev}")
        parsed.append((stored, degree, reso, c1, c2, pose12, bits, index, sparse))
    for j, (stored, degree, reso, c1, c2, pose12, bits, index, sparse) in enumerate(parsed):
        _, _, stored, degree, dims, c1, c2, _, _, bits, index = _baked_volume(
            f"{what}: object {j}", stored, degree, reso, c1, c2, step, bits, terminate, dtype=stored.dtype,
            name="rows" if sparse else "stored", index=index, sparse=sparse)
        o = arr[j]
        bits = None if bits is None else bits.contiguous()
        index = None if index is None else index.contiguous()
        keep += [stored, bits, index]
        o.stored = stored.data_ptr() if stored.numel() else None
        o.bits = None if bits is None else bits.data_ptr()
        o.index = None if index is None else index.data_ptr()
        o.M = stored.shape[0] if sparse else 0
        o.nx, o.ny, o.nz = dims
        o.degree, o.storage_half, o.reserved = degree, int(stored.dtype == torch.float16), 0
        o.c1[:], o.c2[:] = [float(x) for x in c1], [float(x) for x in c2]
        o.pose[:] = pose12
    return arr, dev, keep


def _baked_scene_launch(what, entry, objects, step, white_bkgd, terminate, rays=None, camera=None):
    lib = _lib.load()
    arr, dev, keep = _baked_scene(what, objects, step, terminate)
    args, R, dev, source = _ray_source(what, "the volumes live", dev, rays, camera, convert_first=True)  # (source: kept alive over the call)
    rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((R,), dtype=torch.float32, device=dev)
    alpha = torch.empty((R,), dtype=torch.float32, device=dev)
    args += (arr, len(arr), float(step), int(bool(white_bkgd)), float(terminate), _p(rgb), _p(depth), _p(alpha))
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    del keep
    return rgb, depth, alpha


def baked_scene_render(rays, objects, step, white_bkgd=False, terminate=0.0):
    """Rays through a SCENE of 1 to 8 posed baked volumes of one kind (pnr_baked_scene_render_rays; the contract is in
    include/pixelnerf_hip.h, "Scenes of several baked volumes"): rays (R,8) in the world frame; objects a list of
    (stored, degree, reso, c1, c2, pose, bits=None, index=None) -- stored fp32 or fp16, (nx,ny,nz,4) (degree None / -1) or
    (nx,ny,nz,B,4) (degree 0, 1, 2), or with `index` the kept rows (M,4) / (M,B,4) (bits are then mandatory); reso, c1, c2 the object's
    grid and box in its OWN frame; pose (3,4) or (4,4) object-to-world, rigid, read on the host.  All objects share degree, dtype and
    layout.  The samples are the world ray's; each object is sampled as its own march samples the ray in its frame, and the values at a
    sample are mixed (sigma = the sum, colour weighted by sigma) before alpha and the product scan: volumes that overlap or stand in
    front of each other attenuate each other sample by sample.  One object at the identity renders baked_render's bytes.
    -> (rgb (R,3), depth (R,), alpha (R,)) fp32.  No autograd here: baked_scene_backward is its gradient with respect to the rays
    and the poses, autograd.baked_scene_march_autograd ties the two together."""
    return _baked_scene_launch("baked_scene_render", "pnr_baked_scene_render_rays", objects, step, white_bkgd, terminate, rays=rays)


def baked_scene_render_views(poses, width, height, focal, c, z_near, z_far, objects, step, white_bkgd=False, terminate=0.0):
    """baked_scene_render over every pixel of the views of gen_rays(poses, width, height, focal, z_near, z_far, c)
    (pnr_baked_scene_render_views): poses (NV,4,4) camera-to-world; the rays are regenerated in the kernel -- the same bits as
    baked_scene_render(gen_rays(...)), no ray array.  -> (rgb (NV*H*W,3), depth (NV*H*W,), alpha (NV*H*W,)) fp32."""
    W, H = _image_size("baked_scene_render_views", width, height)
    return _baked_scene_launch("baked_scene_render_views", "pnr_baked_scene_render_views", objects, step, white_bkgd, terminate,
                               camera=(poses, W, H, focal, c, z_near, z_far))


# ---- gradients of the scene march with respect to the world rays and the objects' poses (include/pixelnerf_hip.h, "Gradients of
# the scene march")

def _baked_scene_backward(what, entry, objects, step, white_bkgd, terminate, d_rgb, d_depth, d_alpha, want_poses, rays=None, camera=None):
    """baked_scene_render's checks before any device work, then pnr_baked_scene_backward_rays / _views
    -> (d_rays (R,8), d_local (R,N,6), d_poses (N,12) or None), every row written by the kernels"""
    lib = _lib.load()
    arr, dev, keep = _baked_scene(what, objects, step, terminate)
    args, R, dev, source = _ray_source(what, "the volumes live", dev, rays, camera, detach=True, convert_first=True)  # (source: kept alive over the call)
    grads = _upstream(what, d_rgb, d_depth, d_alpha, R, dev, "the volumes")
    N = len(arr)
    d_rays = torch.empty((R, 8), dtype=torch.float32, device=dev)
    d_local = torch.empty((R, N, 6), dtype=torch.float32, device=dev)
    d_poses = workspace = None
    if want_poses:
        d_poses = torch.empty((N, 12), dtype=torch.float32, device=dev)
        workspace = torch.empty((int(lib.pnr_baked_scene_backward_workspace_bytes()) // 8,), dtype=torch.float64, device=dev)
    args += (arr, N, float(step), int(bool(white_bkgd)), float(terminate), _p(grads[0]), _p(grads[1]), _p(grads[2]),
             _p(d_rays) if R else None, _p(d_local) if R else None, _p(d_poses), _p(workspace))
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    del keep
    return d_rays, d_local, d_poses


def baked_scene_backward(rays, objects, step, d_rgb=None, d_depth=None, d_alpha=None, white_bkgd=False, terminate=0.0, want_poses=True):
    """The gradient of baked_scene_render with respect to the world RAYS and the objects' POSES (pnr_baked_scene_backward_rays;
    the contract is in include/pixelnerf_hip.h, "Gradients of the scene march"): rays (R,8) and objects as baked_scene_render takes
    them, every kind it takes (the volumes are not differentiated: fp16 is legitimate); d_rgb (R,3), d_depth (R,), d_alpha (R,) the
    upstream gradients of its outputs, None = zeros.
    -> (d_rays (R,8) = dL/d [origin, direction, near, far] of the world ray, column 7 exactly 0;
        d_local (R,N,6) = dL/d (o', d') of the ray in each object's frame;
        d_poses (N,12) = dL/d [R | t] of each object as 12 free numbers, row-major (3,4) -- None with want_poses=False).
    Every row is written by the kernels (exact zeros for a ray without samples or without upstream gradient, 12 exact zeros for an
    object no ray meets).  The samples are exactly the forward's; the sample count, the inside tests, the skip bits, the stop chunk,
    the cells, the clamps' sides and which objects contribute to a sample are constants.  No atomics: the same bytes on every call.
    One object at the identity gives baked_ray_backward's bytes in d_rays."""
    return _baked_scene_backward("baked_scene_backward", "pnr_baked_scene_backward_rays", objects, step, white_bkgd, terminate, d_rgb,
                                 d_depth, d_alpha, want_poses, rays=rays)


def baked_scene_backward_views(poses, width, height, focal, c, z_near, z_far, objects, step, d_rgb=None, d_depth=None, d_alpha=None,
                               white_bkgd=False, terminate=0.0, want_poses=True):
    """baked_scene_backward over every pixel of the views of gen_rays(poses, width, height, focal, z_near, z_far, c)
    (pnr_baked_scene_backward_views): the rays are regenerated in the kernels, d_rgb (NV*H*W,3), d_depth and d_alpha (NV*H*W,)
    ordered (view, row, column).  -> (d_rays (NV,H,W,8), d_local (NV*H*W,N,6), d_poses (N,12) or None): the bytes of
    baked_scene_backward(gen_rays(...)); gen_rays_backward of d_rays is the gradient with respect to the cameras."""
    W, H = _image_size("baked_scene_backward_views", width, height)
    d_rays, d_local, d_poses = _baked_scene_backward("baked_scene_backward_views", "pnr_baked_scene_backward_views", objects, step,
                                                     white_bkgd, terminate, d_rgb, d_depth, d_alpha, want_poses,
                                                     camera=(poses, W, H, focal, c, z_near, z_far))
    return d_rays.reshape(-1, H, W, 8), d_local, d_poses


# ---- gradients of the scene march with respect to every object's stored values (include/pixelnerf_hip.h, "Gradients of the scene
# march with respect to the STORED VALUES")

def _baked_scene_stored_backward(what, entry, objects, step, white_bkgd, terminate, d_rgb, d_depth, d_alpha, want, out, rays=None,
                                 camera=None):
    """baked_scene_render's checks and _baked_backward's before any device work, then pnr_baked_scene_stored_backward_rays / _views
    INTO the buffers -> a list with one buffer per object, None where want is False; objects whose `stored` is the same tensor
    share one buffer"""
    lib = _lib.load()
    if isinstance(objects, (list, tuple)):
        for j, ob in enumerate(objects):
            if isinstance(ob, (list, tuple)) and len(ob) and isinstance(ob[0], torch.Tensor) and ob[0].dtype == torch.float16:
                raise TypeError(f"{what}: object {j}: gradients exist for fp32 volumes only; fit the volume in fp32 and call half() "
                                "afterwards")
    source = rays if camera is None else camera[0]
    if isinstance(source, torch.Tensor) and source.requires_grad:
        raise ValueError(f"{what}: no gradient is given with respect to {'rays' if camera is None else 'poses'}; detach them "
                         "(baked_scene_backward gives that gradient)")
    arr, dev, keep = _baked_scene(what, objects, step, terminate)
    N = len(arr)
    args, R, dev, source = _ray_source(what, "the volumes live", dev, rays, camera, convert_first=True)  # (source: kept alive over the call)
    grads = _upstream(what, d_rgb, d_depth, d_alpha, R, dev, "the volumes")
    want = [True] * N if want is None else [bool(w) for w in want]
    if len(want) != N:
        raise ValueError(f"{what}: want must hold one bool per object ({N}), got {len(want)}")
    if out is not None and (not isinstance(out, (list, tuple)) or len(out) != N):
        raise ValueError(f"{what}: out must be a list of one buffer (or None) per object ({N})")
    stored = [keep[3 * j] for j in range(N)]  # (_baked_scene's contiguous tensors)
    bufs, shared = [None] * N, {}
    for j in range(N):
        if not want[j]:
            continue
        key = id(objects[j][0])  # the SAME tensor listed twice: one buffer, the sum of both listings
        given = None if out is None else out[j]
        if key in shared:
            if given is not None and given is not shared[key]:
                raise ValueError(f"{what}: object {j} shares its stored tensor with an earlier object; out[{j}] must be that object's buffer")
            bufs[j] = shared[key]
            continue
        if given is None:
            given = torch.zeros(stored[j].shape, dtype=torch.float32, device=dev)
        else:
            _check_added_into(what, f"out[{j}]", given, stored[j].shape, dev)
        bufs[j] = shared[key] = given
    ptrs = (ctypes.c_void_p * N)(*[None if b is None or not b.numel() else b.data_ptr() for b in bufs])
    args += (arr, N, float(step), int(bool(white_bkgd)), float(terminate), _p(grads[0]), _p(grads[1]), _p(grads[2]), ptrs)
    if R and any(p for p in ptrs):
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    del keep
    return bufs


def baked_scene_stored_backward(rays, objects, step, d_rgb=None, d_depth=None, d_alpha=None, white_bkgd=False, terminate=0.0, want=None,
                                out=None):
    """The gradient of baked_scene_render with respect to every object's STORED VALUES (pnr_baked_scene_stored_backward_rays; the
    contract is in include/pixelnerf_hip.h, "Gradients of the scene march with respect to the STORED VALUES"): rays (R,8) and
    objects as baked_scene_render takes them, fp32 only; d_rgb (R,3), d_depth (R,), d_alpha (R,) the upstream gradients of its
    outputs, None = zeros.
    :param want one bool per object (None: all).  False FREEZES the object: it still mixes and attenuates, gets no gradient, and its
    position in the result is None -- one object fitted in the presence of the others
    :param out a list of buffers the gradients are ADDED into (the caller zeroes them before the first batch), None entries or
    None: fresh zeroed ones
    -> a list of dL/d stored_j, fp32, each the shape of its object's stored.  Objects whose `stored` is the SAME tensor share one
    buffer, returned at each of their positions, holding the sum of their listings' gradients.  Where objects overlap, or one
    stands in front of another, this is not what baked_render_backward gives for each object alone.  The samples are exactly the
    forward's; with bits the cells whose bit is off receive nothing.  Not bit-reproducible from run to run (fp32 atomics).  No
    gradient with respect to rays or poses: baked_scene_backward gives those."""
    return _baked_scene_stored_backward("baked_scene_stored_backward", "pnr_baked_scene_stored_backward_rays", objects, step, white_bkgd,
                                        terminate, d_rgb, d_depth, d_alpha, want, out, rays=rays)


def baked_scene_stored_backward_views(poses, width, height, focal, c, z_near, z_far, objects, step, d_rgb=None, d_depth=None,
                                      d_alpha=None, white_bkgd=False, terminate=0.0, want=None, out=None):
    """baked_scene_stored_backward over every pixel of the views of gen_rays(poses, width, height, focal, z_near, z_far, c)
    (pnr_baked_scene_stored_backward_views): the rays are regenerated in the kernel, d_rgb (NV*H*W,3), d_depth and d_alpha
    (NV*H*W,) ordered (view, row, column) as baked_scene_render_views returns its outputs.  -> the list of dL/d stored_j."""
    W, H = _image_size("baked_scene_stored_backward_views", width, height)
    return _baked_scene_stored_backward("baked_scene_stored_backward_views", "pnr_baked_scene_stored_backward_views", objects, step,
                                        white_bkgd, terminate, d_rgb, d_depth, d_alpha, want, out,
                                        camera=(poses, W, H, focal, c, z_near, z_far))


# ---- gradients of the baked march with respect to the stored values (include/pixelnerf_hip.h, "Gradients of the baked march")

def _baked_backward(what, entry, stored, degree, reso, c1, c2, step, bits, index, white_bkgd, terminate, d_rgb, d_depth, d_alpha, out,
                    rays=None, camera=None):
    """checks before any device work, then pnr_baked_backward_rays / _views INTO `out` (None: a fresh zeroed buffer) -> out"""
    lib = _lib.load()
    if isinstance(stored, torch.Tensor) and stored.dtype == torch.float16:
        raise TypeError(f"{what}: gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards")
    source = rays if camera is None else camera[0]
    if isinstance(source, torch.Tensor) and source.requires_grad:
        raise ValueError(f"{what}: no gradient is given with respect to {'rays' if camera is None else 'poses'}; detach them")
    v = _baked_volume(what, stored, degree, reso, c1, c2, step, bits, terminate, index=index)
    _, name, stored, _, _, _, _, step, terminate, _, _ = v
    args, R, dev, source = _ray_source(what, lambda: _lives(name, stored, camera), stored.device, rays, camera)  # (source: kept alive)
    grads = _upstream(what, d_rgb, d_depth, d_alpha, R, dev, f"the {'rays' if camera is None else 'poses'}")
    if out is None:
        out = torch.zeros(stored.shape, dtype=torch.float32, device=dev)
    else:
        _check_added_into(what, "out", out, stored.shape, dev)
    args += (*_volume_args(v), step, int(bool(white_bkgd)), terminate, _p(grads[0]), _p(grads[1]), _p(grads[2]),
             _p(out) if out.numel() else None)
    if R and out.numel():
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    return out


def baked_render_backward(rays, stored, degree, reso, c1, c2, step, d_rgb=None, d_depth=None, d_alpha=None, bits=None, index=None,
                          white_bkgd=False, terminate=0.0, out=None):
    """The gradient of baked_render / baked_sh_render / baked_sparse_render with respect to the stored values
    (pnr_baked_backward_rays): stored fp32 (nx,ny,nz,4) (degree None / -1) or (nx,ny,nz,B,4) (degree 0, 1, 2), or with `index` the
    kept rows (M,4) / (M,B,4) (bits are then mandatory); d_rgb (R,3), d_depth (R,), d_alpha (R,) the upstream gradients of the
    march's outputs, None = zeros.  -> dL/d stored, fp32, the shape of stored.  `out`: a buffer the gradient is ADDED into (the
    caller zeroes it before the first batch); None: a fresh one.  The samples are exactly the forward's with the same rays, bits,
    step and terminate; with bits the cells whose bit is off receive nothing.  Not bit-reproducible from run to run (fp32 atomics).
    No gradient with respect to rays, step or the geometry: rays that require grad are refused.  An fp16 volume is refused."""
    return _baked_backward("baked_render_backward", "pnr_baked_backward_rays", stored, degree, reso, c1, c2, step, bits, index, white_bkgd,
                           terminate, d_rgb, d_depth, d_alpha, out, rays=rays)


def baked_render_views_backward(poses, width, height, focal, c, z_near, z_far, stored, degree, reso, c1, c2, step, d_rgb=None,
                                d_depth=None, d_alpha=None, bits=None, index=None, white_bkgd=False, terminate=0.0, out=None):
    """baked_render_backward over every pixel of the views of gen_rays(poses, width, height, focal, z_near, z_far, c)
    (pnr_baked_backward_views): the rays are regenerated in the kernel, d_rgb (NV*H*W,3), d_depth and d_alpha (NV*H*W,) ordered
    (view, row, column) as baked_render_views returns its outputs.  -> dL/d stored."""
    W, H = _image_size("baked_render_views_backward", width, height)
    return _baked_backward("baked_render_views_backward", "pnr_baked_backward_views", stored, degree, reso, c1, c2, step, bits, index,
                           white_bkgd, terminate, d_rgb, d_depth, d_alpha, out, camera=(poses, W, H, focal, c, z_near, z_far))


# ---- gradients of the baked march with respect to the rays (include/pixelnerf_hip.h, "Gradients of the baked march with respect to
# the RAYS")

def _baked_ray_backward(what, entry, stored, degree, reso, c1, c2, step, bits, index, white_bkgd, terminate, d_rgb, d_depth, d_alpha,
                        rays=None, camera=None):
    """checks before any device work, then pnr_baked_ray_backward_rays / _views -> d_rays (R,8), every row written by the kernel"""
    lib = _lib.load()
    v = _baked_volume(what, stored, degree, reso, c1, c2, step, bits, terminate, index=index)
    _, name, stored, _, dims, _, _, step, terminate, _, index = v
    args, R, dev, source = _ray_source(what, lambda: _lives(name, stored, camera), stored.device, rays, camera, detach=True)  # (kept alive)
    grads = _upstream(what, d_rgb, d_depth, d_alpha, R, dev, f"the {'rays' if camera is None else 'poses'}")
    out = torch.empty((R, 8), dtype=torch.float32, device=dev)
    args += (*_volume_args(v, stored.dtype == torch.float16), step, int(bool(white_bkgd)), terminate, _p(grads[0]), _p(grads[1]),
             _p(grads[2]), _p(out) if R else None)
    if R:
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    return out


def baked_ray_backward(rays, stored, degree, reso, c1, c2, step, d_rgb=None, d_depth=None, d_alpha=None, bits=None, index=None,
                       white_bkgd=False, terminate=0.0):
    """The gradient of any baked march with respect to its RAYS (pnr_baked_ray_backward_rays): rays (R,8); stored fp32 or fp16,
    (nx,ny,nz,4) (degree None / -1) or (nx,ny,nz,B,4) (degree 0, 1, 2), or with `index` the kept rows (M,4) / (M,B,4) (bits are then
    mandatory); d_rgb (R,3), d_depth (R,), d_alpha (R,) the upstream gradients of the march's outputs, None = zeros.
    -> d_rays (R,8) fp32 = dL/d [origin, direction, near, far]; column 7 is exactly 0 (far only sets the sample count).  Every row is
    written by the kernel: rays without samples or without upstream gradient get exact zeros.  The samples are exactly the
    forward's; the sample count, the inside test, the skip bits, the stop chunk, the cells and the clamps' regions are constants, so
    the gradient is the exact derivative almost everywhere and one-sided on a cell plane.  No atomics: the same bytes on every call;
    an fp16 volume gives the bytes of its float()."""
    return _baked_ray_backward("baked_ray_backward", "pnr_baked_ray_backward_rays", stored, degree, reso, c1, c2, step, bits, index,
                               white_bkgd, terminate, d_rgb, d_depth, d_alpha, rays=rays)


def baked_ray_backward_views(poses, width, height, focal, c, z_near, z_far, stored, degree, reso, c1, c2, step, d_rgb=None, d_depth=None,
                             d_alpha=None, bits=None, index=None, white_bkgd=False, terminate=0.0):
    """baked_ray_backward over every pixel of the views of gen_rays(poses, width, height, focal, z_near, z_far, c)
    (pnr_baked_ray_backward_views): the rays are regenerated in the kernel, d_rgb (NV*H*W,3), d_depth and d_alpha (NV*H*W,) ordered
    (view, row, column).  -> (NV,H,W,8): the gradient with respect to the regenerated rays, the bytes of
    baked_ray_backward(gen_rays(...)); gen_rays_backward of it is the gradient with respect to the poses."""
    W, H = _image_size("baked_ray_backward_views", width, height)
    out = _baked_ray_backward("baked_ray_backward_views", "pnr_baked_ray_backward_views", stored, degree, reso, c1, c2, step, bits, index,
                              white_bkgd, terminate, d_rgb, d_depth, d_alpha, camera=(poses, W, H, focal, c, z_near, z_far))
    return out.reshape(-1, H, W, 8)


# ---- what the rays of a march see, and a volume on another grid (include/pixelnerf_hip.h, "Visibility of a baked volume",
# "Resampling a baked volume")

def _baked_visibility(what, entry, stored, degree, reso, c1, c2, step, bits, index, terminate, out, rays=None, camera=None):
    """checks before any device work, then pnr_baked_visibility_rays / _views INTO `out` (None: a fresh zeroed field) -> out"""
    lib = _lib.load()
    # the shape of the field, from the arguments alone: a wrong `out` is refused before anything else looks at a device
    if out is not None and isinstance(stored, torch.Tensor) and len(reso) == 3:
        shape = (stored.shape[0],) if index is not None else tuple(int(r) for r in reso)
        if not _is_buffer(out, shape):
            raise ValueError(f"{what}: out must be a contiguous float32 tensor of shape {shape} that does not require grad (it is "
                             "max-accumulated into)")
    v = _baked_volume(what, stored, degree, reso, c1, c2, step, bits, terminate, index=index)
    _, name, stored, _, dims, _, _, step, terminate, _, index = v
    args, R, dev, source = _ray_source(what, lambda: _lives(name, stored, camera), stored.device, rays, camera, detach=True)  # (kept alive)
    if out is None:
        out = torch.zeros((stored.shape[0],) if index is not None else dims, dtype=torch.float32, device=dev)
    elif out.device != dev:
        raise ValueError(f"{what}: out lives on {out.device}, the {'rays' if camera is None else 'poses'} on {dev}")
    args += (*_volume_args(v, stored.dtype == torch.float16), step, terminate, _p(out))
    if R and out.numel():
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    return out


def baked_visibility(rays, stored, degree, reso, c1, c2, step, bits=None, index=None, terminate=0.0, out=None):
    """Which stored rows the rays of a march SEE (pnr_baked_visibility_rays): per row the largest w_i x (trilinear corner weight) over
    every sample of every ray, w_i the forward's compositing weight bit for bit.  rays (R,8); stored fp32 or fp16, (nx,ny,nz,4)
    (degree None / -1) or (nx,ny,nz,B,4) (degree 0, 1, 2), or with `index` the kept rows (M,4) / (M,B,4) (bits are then mandatory).
    -> vis fp32, (nx,ny,nz) for a dense volume, (M,) for a sparse one.  `out`: a field the result is MAX-accumulated into (zeroed
    by the caller before the first batch); None: a fresh one.  The samples are exactly the forward's with the same rays, bits, step
    and terminate.  An integer atomic max: the same bytes on every call, for any order of the rays and any split into batches."""
    return _baked_visibility("baked_visibility", "pnr_baked_visibility_rays", stored, degree, reso, c1, c2, step, bits, index, terminate,
                             out, rays=rays)


def baked_visibility_views(poses, width, height, focal, c, z_near, z_far, stored, degree, reso, c1, c2, step, bits=None, index=None,
                           terminate=0.0, out=None):
    """baked_visibility over every pixel of the views of gen_rays(poses, width, height, focal, z_near, z_far, c)
    (pnr_baked_visibility_views): the rays are regenerated in the kernel -- the bytes of baked_visibility(gen_rays(...))."""
    W, H = _image_size("baked_visibility_views", width, height)
    return _baked_visibility("baked_visibility_views", "pnr_baked_visibility_views", stored, degree, reso, c1, c2, step, bits, index,
                             terminate, out, camera=(poses, W, H, focal, c, z_near, z_far))


def baked_resample(stored, degree, reso, reso_dst, index=None, ids_dst=None):
    """The stored values of a baked volume on another point count over the SAME box (pnr_baked_resample): stored fp32 or fp16,
    (nx,ny,nz,4) (degree None / -1) or (nx,ny,nz,B,4) (degree 0, 1, 2) with reso = (nx,ny,nz), or with `index` (nx,ny,nz) int32 the
    kept rows (M,4) / (M,B,4) (a corner that is not kept reads as zeros).  reso_dst: the new point counts.
    -> fp32, dense (nx',ny',nz'[,B],4), or with ids_dst (M',) int32 -- linear ids of the NEW grid -- the rows (M'[,B],4) at those
    points (an id outside the grid: a row of zeros).  Integer index arithmetic and a select at fraction 0: the same reso is the
    identity, a refinement n' - 1 = m (n - 1) keeps the old points bit for bit.  A view-dependent volume interpolates its
    coefficients.  No atomics: the same bytes on every call.  No autograd."""
    what = "baked_resample"
    lib = _lib.load()
    degree, tail = _stored_tail(what, degree)
    if len(reso) != 3 or len(reso_dst) != 3:
        raise ValueError(f"{what}: reso and reso_dst must have 3 entries each")
    dims, dims_dst = tuple(int(r) for r in reso), tuple(int(r) for r in reso_dst)
    for d in (dims, dims_dst):
        if any(n < 2 for n in d) or d[0] * d[1] * d[2] >= 2 ** 31:
            raise ValueError(f"{what}: a grid needs at least 2 points per axis and fewer than 2^31 points, got {d}")
    sparse = index is not None
    lead = (None,) if sparse else dims
    if not isinstance(stored, torch.Tensor) or stored.dtype not in (torch.float32, torch.float16):
        raise TypeError(f"{what}: stored must be a float32 or float16 tensor")
    if stored.dim() != len(lead) + len(tail) or tuple(stored.shape[len(lead):]) != tail or (not sparse and tuple(stored.shape[:3]) != dims):
        raise ValueError(f"{what}: stored must be ({'M' if sparse else ','.join(str(d) for d in dims)},{','.join(str(s) for s in tail)}) at "
                         f"degree {degree}, got {tuple(stored.shape)}")
    half = stored.dtype == torch.float16
    stored = _f32(stored.detach(), "stored", lead + tail, stored.dtype)
    dev = stored.device
    if stored.numel() and stored.data_ptr() % (8 if half else 16):
        raise ValueError(f"{what}: stored must be {8 if half else 16}-byte aligned")
    if sparse:
        _check_index(what, index, dims, dev)
    if ids_dst is not None and (not isinstance(ids_dst, torch.Tensor) or ids_dst.dtype != torch.int32 or ids_dst.dim() != 1
                                or ids_dst.device != dev):
        raise ValueError(f"{what}: ids_dst must be a 1-d int32 tensor on {dev}")
    M = stored.shape[0] if sparse else 0
    M_dst = ids_dst.shape[0] if ids_dst is not None else 0
    out = torch.empty(((M_dst,) if ids_dst is not None else dims_dst) + tail, dtype=torch.float32, device=dev)
    if out.numel():
        ids_dst = None if ids_dst is None else ids_dst.contiguous()
        with torch.cuda.device(dev):
            _lib.check(lib.pnr_baked_resample(_p(stored) if stored.numel() else None, int(half), M, degree,
                                              _p(index.contiguous()) if sparse else None, *dims, _p(out), M_dst, _p(ids_dst), *dims_dst,
                                              _stream()), "pnr_baked_resample")
    return out


# ---- the total-variation prior of a fitted volume (include/pixelnerf_hip.h, "Total-variation prior")

def baked_tv(stored, degree, reso, weights, eps=1e-8, index=None, ids=None, want_value=True, grad_out=None, scale=None):
    """Total variation of the stored values of a baked volume and its gradient (pnr_baked_tv): stored fp32 (nx,ny,nz,4) (degree None
    / -1) or (nx,ny,nz,B,4) (degree 0, 1, 2), or with `index` (nx,ny,nz) int32 and `ids` (M,) int32 (sparse_points) the kept rows
    (M,4) / (M,B,4); weights: E = 4 or 4 B floats, finite and >= 0, one per element of a row.
    value = (1/N) sum_p sum_c w_c sqrt(d_x^2 + d_y^2 + d_z^2 + eps) over the raw forward differences (0 beyond the grid and, sparse,
    where either end is not kept), N = nx ny nz or M.
    -> (value32, value64): 0-dim fp32 and fp64 tensors on the device, or (None, None) with want_value=False.
    grad_out: a contiguous fp32 tensor of stored's shape that scale * d value / d stored is ADDED into (None: no gradient is
    computed); scale: None (1), a number, or a one-element fp32 tensor on the device, which is read by the kernel -- no host read.
    No atomics: the same bytes on every call.  An fp16 volume and a non-contiguous `stored` are refused."""
    what = "baked_tv"
    lib = _lib.load()
    if isinstance(stored, torch.Tensor) and stored.dtype == torch.float16:
        raise TypeError(f"{what}: gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards")
    degree, tail = _stored_tail(what, degree)
    if len(reso) != 3:
        raise ValueError(f"{what}: reso must have 3 entries")
    dims = tuple(int(r) for r in reso)
    if lib.pnr_occupancy_bytes(*dims) == 0:
        raise ValueError(f"{what}: a grid needs at least 2 points per axis and fewer than 2^31 cells, got {dims}")
    if (index is None) != (ids is None):
        raise ValueError(f"{what}: index and ids go together (both for the kept rows of a sparse volume, neither for a dense one)")
    sparse = index is not None
    lead = (None,) if sparse else dims
    if not isinstance(stored, torch.Tensor) or stored.dim() != len(lead) + len(tail) or tuple(stored.shape[len(lead):]) != tail \
            or (not sparse and tuple(stored.shape[:3]) != dims):
        raise ValueError(f"{what}: stored must be ({'M' if sparse else ','.join(str(d) for d in dims)},{','.join(str(s) for s in tail)}) at "
                         f"degree {degree}, got {tuple(stored.shape) if isinstance(stored, torch.Tensor) else type(stored).__name__}")
    if not stored.is_contiguous():
        raise ValueError(f"{what}: stored must be contiguous (the kernel walks it as rows of float4; call .contiguous() on a copy you keep)")
    E = math.prod(tail)
    w = [float(x) for x in (weights.flatten().tolist() if isinstance(weights, torch.Tensor) else weights)]
    if len(w) != E or not all(math.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError(f"{what}: weights must be {E} finite numbers >= 0 (one per element of a row), got {w}")
    eps = float(eps)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError(f"{what}: eps must be finite and > 0, got {eps}")
    stored = _f32(stored.detach(), "stored", lead + tail)
    dev = stored.device
    if stored.numel() and stored.data_ptr() % 16:
        raise ValueError(f"{what}: stored must be 16-byte aligned")
    M = stored.shape[0] if sparse else 0
    if sparse:
        _check_index(what, index, dims, dev)
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or tuple(ids.shape) != (M,) or ids.device != dev:
            raise ValueError(f"{what}: ids must be the ({M},) int32 tensor of sparse_points on {dev}")
        index = index.contiguous()
        ids = ids.contiguous() if M else torch.zeros((1,), dtype=torch.int32, device=dev)  # (no rows: a pointer that is not null)
    if grad_out is not None:
        _check_added_into(what, "grad_out", grad_out, stored.shape, dev)
    if scale is not None and not isinstance(scale, torch.Tensor):
        scale = torch.full((1,), float(scale), dtype=torch.float32, device=dev)
    if scale is not None:
        if scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != dev:
            raise ValueError(f"{what}: scale must be one float32 number on {dev}")
        scale = scale.detach().contiguous()
    value32 = torch.empty((), dtype=torch.float32, device=dev) if want_value else None
    value64 = torch.empty((), dtype=torch.float64, device=dev) if want_value else None
    workspace = torch.empty((lib.pnr_baked_tv_workspace_bytes() // 8,), dtype=torch.float64, device=dev) if want_value else None
    if want_value or grad_out is not None:
        some = stored.numel() > 0
        with torch.cuda.device(dev):
            _lib.check(lib.pnr_baked_tv(_p(stored) if some else None, M, degree, _p(index) if sparse else None, _p(ids) if sparse else None,
                                        dims[0], dims[1], dims[2], (ctypes.c_float * E)(*w), eps, _p(scale), _p(value32), _p(value64),
                                        _p(grad_out) if grad_out is not None and some else None, _p(workspace), _stream()), "pnr_baked_tv")
    return value32, value64
