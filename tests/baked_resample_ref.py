"""Test helper (not a test): pnr_baked_resample (include/pixelnerf_hip.h, "Resampling a baked volume") restated in plain torch, and the
volumes that tests/test_baked_resample_host.py and tests/test_hip_baked_resample.py share.  No GPU, no package import.

resample() at fp32 performs the entry's operations: the integer cell and remainder per axis, f = fp32(rem) / fp32(n' - 1), and the
blend f == 0 ? a : a + f (b - a) along z, then y, then x, each operation rounded on its own.  At fp64 f is rem / (n' - 1) in fp64 --
the fraction the entry rounds ONCE -- and the blends are fp64: the reference the fp32 result is held against.
"""
import functools

import numpy as np
import torch

GRIDS = ((5, 6, 7), (6, 5, 9))   # an odd point count, unequal axes
KINDS = (None, 0, 1, 2)          # RGBA, degree 0, 1, 2


def axis_map(n_src, n_dst):
    """-> (i0, i1, rem) int64 arrays over the n_dst points of an axis, den = n_dst - 1"""
    num = np.arange(n_dst, dtype=np.int64) * (n_src - 1)
    q, rem = num // (n_dst - 1), num % (n_dst - 1)
    return q, np.minimum(q + 1, n_src - 1), rem


def resample(stored, reso_dst, dtype=torch.float64, kept=None):
    """stored (nx,ny,nz,4) or (nx,ny,nz,B,4), numpy fp32 / fp16 or a torch tensor; kept None or (nx,ny,nz) bool: a point that is not
    kept reads as zeros -> the (reso_dst,...) tensor at `dtype`"""
    v = stored if isinstance(stored, torch.Tensor) else torch.tensor(np.asarray(stored).astype(np.float32))
    v = v.to(dtype)
    if kept is not None:
        mask = torch.as_tensor(np.asarray(kept, bool)).reshape(tuple(v.shape[:3]) + (1,) * (v.dim() - 3))
        v = torch.where(mask, v, torch.zeros_like(v))
    for axis in (2, 1, 0):
        n_src, n_dst = v.shape[axis], int(reso_dst[axis])
        i0, i1, rem = axis_map(n_src, n_dst)
        if dtype == torch.float32:
            f = torch.tensor(rem.astype(np.float32) / np.float32(n_dst - 1))
        else:
            f = torch.tensor(rem.astype(np.float64) / float(n_dst - 1)).to(dtype)
        shape = [1] * v.dim()
        shape[axis] = n_dst
        f = f.reshape(shape)
        a, b = v.index_select(axis, torch.from_numpy(i0)), v.index_select(axis, torch.from_numpy(i1))
        v = torch.where(f == 0, a, a + f * (b - a))
    return v


@functools.lru_cache(maxsize=None)
def volume(reso, kind, half=False):
    """seeded stored values (numpy, read-only) on `reso`: rgb-like numbers in [-0.5, 1.5], sigma-like in [0, 30] with zeros, a few
    exact -0 and (fp32) numbers that fp16 cannot hold; half: rounded to fp16"""
    rs = np.random.RandomState(1000 + 17 * GRIDS.index(tuple(reso)) + (0 if kind is None else kind + 1))
    tail = (4,) if kind is None else ((kind + 1) ** 2, 4)
    v = rs.uniform(-0.5, 1.5, tuple(reso) + tail).astype(np.float32)
    v[..., 3] = np.where(rs.uniform(size=v[..., 3].shape) < 0.4, 0.0, rs.uniform(0.0, 30.0, v[..., 3].shape)).astype(np.float32)
    flat = v.reshape(-1)
    flat[rs.choice(flat.size, 12, replace=False)] = np.float32(-0.0)
    if half:
        v = v.astype(np.float16)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def cells(reso):
    """a seeded third of the cells of `reso` (bool (nx-1,ny-1,nz-1), read-only): the occupancy of the sparse cases"""
    rs = np.random.RandomState(77 + GRIDS.index(tuple(reso)))
    c = rs.uniform(size=tuple(r - 1 for r in reso)) < 0.35
    c.setflags(write=False)
    return c


def refined(reso, m):
    return tuple(m * (r - 1) + 1 for r in reso)


def ulp32(x):
    """the spacing of fp32 at |x|"""
    return float(np.spacing(np.float32(abs(x))))
