"""
What ops.py and ops_baked.py both stand on: the current stream, pointers, the tensor check and the small argument rules that more
than one front-end uses.  Imports nothing of the package but _lib, so either module can be imported first.
"""
import ctypes

import torch

from . import _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _f32(t, name, shape=None, dtype=torch.float32):
    """a contiguous HIP tensor of `dtype` (fp32 unless said: a baked volume may be stored in fp16) and of `shape` (None: any size)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise _lib.PixelNerfHipError(f"{name}: tensor must live on a HIP device (got {t.device}); "
                                     "pixelnerf_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if shape is not None:
        if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    return t.contiguous()


def _intrinsics(focal, c, width, height):
    """focal a scalar or (fx, fy), c (cx, cy) or None = the image centre -> fx, fy, cx, cy as the library takes them"""
    fx, fy = (float(focal), float(focal)) if not hasattr(focal, "__len__") else (float(focal[0]), float(focal[-1]))
    cx, cy = (width * 0.5, height * 0.5) if c is None else (float(c[0]), float(c[1]))
    return fx, fy, cx, cy


def _image_size(what, width, height):
    W, H = int(width), int(height)
    if W <= 0 or H <= 0:
        raise ValueError(f"{what}: the image must have at least one pixel, got {W} x {H}")
    return W, H


def _check_grid_args(what, bits, reso, c1, c2, device):
    """-> (nx, ny, nz) of an occupancy bitfield checked against its geometry (occupancy_clip_rays / occupancy_mark_samples)"""
    lib = _lib.load()
    if len(reso) != 3 or len(c1) != 3 or len(c2) != 3:
        raise ValueError(f"{what}: c1, c2, reso must have 3 entries each")
    nx, ny, nz = (int(r) for r in reso)
    nbytes = lib.pnr_occupancy_bytes(nx, ny, nz)
    if nbytes == 0:
        raise ValueError(f"{what}: a grid needs at least 2 points per axis and fewer than 2^31 cells, got {(nx, ny, nz)}")
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or bits.dim() != 1 or bits.numel() != nbytes // 4:
        raise ValueError(f"{what}: bits must be the ({nbytes // 4},) int32 tensor of occupancy_build for reso {(nx, ny, nz)}")
    if bits.device != device:
        raise ValueError(f"{what}: bits live on {bits.device}, the rays on {device}")
    return nx, ny, nz


def _float3_pair(a, b):
    """two 3-vectors (box corners; origin and scale) as the C arrays the library takes"""
    return (ctypes.c_float * 3)(*[float(v) for v in a]), (ctypes.c_float * 3)(*[float(v) for v in b])
