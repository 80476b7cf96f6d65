"""CPU tests of the baked-volume feature: the numpy restatement (tests/baked_ref.py) against closed forms, the inputs of the GPU
parity test (tests/test_hip_baked.py) against the conditions its bar rests on, and the header / binding / wrapper layer, whose
argument checks all come before any device work."""
import ctypes
import math
import re
import os

import numpy as np
import pytest
import torch

import baked_ref as B
from pixelnerf_amd import _lib


# ---------------------------------------------------------------- the reference against closed forms

def _block_field(s):
    """9^3 points over [0,8]^3 (h = 1): (r,g,b,sigma) = (0.25, 0.5, 0.75, s) on the points 3..5 of every axis, sigma 0 elsewhere"""
    vol = np.zeros((9, 9, 9, 4), np.float32)
    vol[..., :3] = (0.25, 0.5, 0.75)
    vol[3:6, 3:6, 3:6, 3] = s
    return vol, (0.0, 0.0, 0.0), (8.0, 8.0, 8.0)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_reference_block_closed_form(axis):
    s, step = 0.046875, 0.25                          # (both exact in fp32, as the volume stores them)
    vol, c1, c2 = _block_field(s)
    o, d = np.full(3, 4.0), np.zeros(3)
    o[axis], d[axis] = -1.0, 1.0                       # through the block's middle; near = 1 is the box face, far = 9 the other
    rays = np.concatenate((o, d, [1.0, 9.0]))[None].astype(np.float32)
    # samples at 0.125 + 0.25 k along the axis.  Cells [3,4] and [4,5] lie wholly in the block: 8 samples at sigma = s.  The
    # boundary cells [2,3] and [5,6] ramp linearly: 4 samples each at the fractions 1/8, 3/8, 5/8, 7/8 (and mirrored), sum 2.
    L = step * 8 + step * (0.125 + 0.375 + 0.625 + 0.875) * 2
    assert L == 3.0
    want = 1.0 - math.exp(-s * L)
    for white in (False, True):
        rgb, depth, alpha = B.render_ref(rays, vol, c1, c2, step, white_bkgd=white)
        assert abs(alpha[0] - want) <= 1e-9, (alpha[0], want)
        bg = 1.0 if white else 0.0
        assert np.allclose(rgb[0], np.array([0.25, 0.5, 0.75]) * want + bg * (1.0 - want), atol=1e-9, rtol=0)
        assert 4.9 * want < depth[0] < 5.0 * want      # the field is symmetric about t = 5; the attenuation inside pulls forward
    cells = np.zeros((8, 8, 8), bool)
    cells[2:6, 2:6, 2:6] = True                        # the cells with a corner > 0: skipping them changes nothing
    assert B.gaps(B.render_ref(rays, vol, c1, c2, step), B.render_ref(rays, vol, c1, c2, step, occupied=cells)) == (0.0, 0.0, 0.0)
    none = B.render_ref(rays, vol, c1, c2, step, occupied=np.zeros((8, 8, 8), bool), white_bkgd=True)
    assert (none[0] == 1.0).all() and none[1][0] == 0.0 and none[2][0] == 0.0


def test_reference_background_exactly():
    vol, c1, c2 = _block_field(3.0)
    miss = np.array([[-1.0, 20.0, 4.0, 1.0, 0.0, 0.0, 1.0, 9.0],        # past the box
                     [4.0, 4.0, 4.0, 1.0, 0.0, 0.0, 2.0, 1.0],           # near >= far
                     [4.0, 4.0, np.nan, 1.0, 0.0, 0.0, 1.0, 9.0],        # not finite
                     [-1.0, 4.0, 4.0, 1.0, 0.0, 0.0, 1.0, 1e9]], np.float32)  # more than 2^20 samples
    for dtype in (np.float64, np.float32):
        for white in (False, True):
            rgb, depth, alpha = B.render_ref(miss, vol, c1, c2, 0.25, white_bkgd=white, dtype=dtype)
            assert rgb.dtype == dtype and (rgb == (1.0 if white else 0.0)).all() and (depth == 0).all() and (alpha == 0).all()
            hit = np.array([[-1.0, 4.0, 4.0, 1.0, 0.0, 0.0, 1.0, 9.0]], np.float32)
            rgb, depth, alpha = B.render_ref(hit, np.zeros_like(vol), c1, c2, 0.25, white_bkgd=white, dtype=dtype)  # zero field
            assert (rgb == (1.0 if white else 0.0)).all() and (depth == 0).all() and (alpha == 0).all()


def test_reference_termination_bound():
    vol, c1, c2 = _block_field(8.0)                                   # T behind the block = exp(-24)
    rays = np.array([[-1.0, 4.0, 4.0, 1.0, 0.0, 0.0, 1.0, 9.0]], np.float32)
    plain = B.render_ref(rays, vol, c1, c2, 0.0625)                   # 128 samples; after the first 64 T = exp(-12)
    assert B.gaps(plain, B.render_ref(rays, vol, c1, c2, 0.0625, terminate=0.0)) == (0.0, 0.0, 0.0)
    d = B.gaps(plain, B.render_ref(rays, vol, c1, c2, 0.0625, terminate=0.5))
    assert d[0] <= 0.5 and d[2] <= 0.5 and d[1] <= 0.5 * 9.0


@pytest.mark.parametrize("setting", sorted(B.SETTINGS))
def test_gpu_parity_inputs_carry_their_bar(setting):
    """what tests/test_hip_baked.py's parity bar rests on: on its own inputs the fp32 restatement differs from the fp64 one, by
    less than 1e-4, on every output; the sample counts are the intended ones in both precisions; the rays are the intended mix"""
    vol, rays = B.common_volume(), B.common_rays(setting)
    near, far, step = B.SETTINGS[setting]
    for dtype in (np.float32, np.float64):
        r = rays.astype(dtype)
        n = np.ceil((r[0, 7] - r[0, 6]) / dtype(np.float32(step)))
        assert int(n) == B.N_SAMPLES[setting]
    assert (vol[..., 3] >= 0).all() and vol[..., 3].max() > 25 and (vol[2:5, 2:5, 2:5, 3] == 0).all()
    for white in (False, True):
        r64 = B.render_ref(rays, vol, B.C1, B.C2, step, white_bkgd=white)
        r32 = B.render_ref(rays, vol, B.C1, B.C2, step, white_bkgd=white, dtype=np.float32)
        g = B.gaps(r32, r64)
        print(f"{setting} white={white}: fp32 - fp64 gap rgb {g[0]:.3e} depth {g[1]:.3e} alpha {g[2]:.3e}")
        assert all(0.0 < x < 1e-4 for x in g), g
        alpha = r64[2]
        assert (alpha[:26] > 0.5).sum() >= 20                         # the hitting rays: most of them meet something dense
        assert (alpha[26:30] == 0).all() and alpha[36] == 0           # the misses and the near >= far ray: background
        assert (alpha[30:36] > 0).all()                               # origin inside, axis-parallel, in a cell plane
        assert (r64[0][36] == (1.0 if white else 0.0)).all()


# ---------------------------------------------------------------- header, binding, wrappers

def test_header_declares_and_binding_binds(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("pnr_baked_render_rays", "pnr_baked_render_views"):
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert name in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.pnr_abi_version() == 12
    assert len(_lib.PROTOTYPES["pnr_baked_render_rays"][1]) == 16 and len(_lib.PROTOTYPES["pnr_baked_render_views"][1]) == 24
    assert "pnr_baked.hip" in _lib.SOURCES


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    lo, hi = _f3(-1, -1, -1), _f3(1, 1, 1)
    P = 64  # a non-null, 16-byte aligned stand-in for a device pointer: every call below must fail before it is touched

    def rays(R=4, rays_p=P, vol=P, bits=None, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P, depth=P, alpha=P):
        return lib.pnr_baked_render_rays(rays_p, R, vol, bits, n[0], n[1], n[2], c1, c2, step, 0, term, rgb, depth, alpha, None)

    def views(poses=P, NV=1, W=4, H=4, vol=P, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P):
        return lib.pnr_baked_render_views(poses, NV, W, H, 10.0, 10.0, 2.0, 2.0, 0.5, 3.0, vol, None, n[0], n[1], n[2], c1, c2, step, 0,
                                          term, rgb, P, P, None)

    for call in (rays, views):
        assert call(n=(1, 4, 4)) == -1 and b"at least 2 grid points" in lib.pnr_last_error()
        assert call(n=(2049, 2049, 2049)) == -1 and b"2^31" in lib.pnr_last_error()
        assert call(c1=hi, c2=lo) == -1 and b"c1 < c2" in lib.pnr_last_error()
        assert call(c1=None) == -1
        assert call(c2=_f3(1, float("nan"), 1)) == -1
        for step in (0.0, -0.1, float("inf"), float("nan")):
            assert call(step=step) == -1 and b"step" in lib.pnr_last_error()
        for term in (-0.01, 1.0, 1.5, float("nan")):
            assert call(term=term) == -1 and b"terminate" in lib.pnr_last_error()
        assert call(vol=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(rgb=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(vol=P + 8) == -1 and b"16-byte" in lib.pnr_last_error()
        assert call(rgb=P + 2) == -1 and b"4-byte" in lib.pnr_last_error()
    assert rays(R=-1) == -1 and rays(rays_p=None) == -1 and rays(rays_p=P + 1) == -1
    assert rays(depth=None) == -1 and rays(alpha=None) == -1 and rays(bits=P + 2) == -1
    assert rays(R=2 ** 34) == -1 and b"launch limit" in lib.pnr_last_error()
    assert views(NV=-1) == -1 and views(W=0) == -1 and views(H=-3) == -1 and views(poses=None) == -1
    assert rays(R=0, rays_p=None, vol=None, rgb=None, depth=None, alpha=None) == 0      # no rays: a no-op
    assert views(NV=0, poses=None, vol=None, rgb=None) == 0


def test_wrappers_refuse_before_any_device_work():
    from pixelnerf_amd import ops
    from pixelnerf_amd.util import bake                                # imports without a GPU
    from pixelnerf_amd.util.bake import BakedVolume
    vol, rays, poses = torch.zeros(4, 5, 6, 4), torch.zeros(3, 8), torch.eye(4)[None]
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    assert bake.BakedVolume is BakedVolume
    # CPU tensors: there is no CPU path
    with pytest.raises(_lib.PixelNerfHipError):
        BakedVolume.from_tensor(vol, lo, hi)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_render(rays, vol, (4, 5, 6), lo, hi, 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, vol, (4, 5, 6), lo, hi, 0.1)
    bv = BakedVolume.__new__(BakedVolume)                              # a volume object without its device parts
    bv.vol, bv.reso, bv.c1, bv.c2, bv.skip_threshold = vol, (4, 5, 6), lo, hi, 0.0
    with pytest.raises(_lib.PixelNerfHipError):
        bv.render(rays, skip=False)
    with pytest.raises(_lib.PixelNerfHipError):
        bv.render_views(poses, 4, 4, 10.0, 0.5, 3.0, skip=False)
    assert bv.cell_size == (2 / 3, 2 / 4, 2 / 5)
    # argument errors
    bad = [dict(reso=(4, 5)), dict(reso=(1, 5, 6)), dict(c1=hi, c2=lo), dict(c1=(0, 0)), dict(c2=(1.0, float("inf"), 1.0)),
           dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(step=float("inf")),
           dict(terminate=-0.1), dict(terminate=1.0), dict(terminate=float("nan"))]
    for kw in bad:
        a = dict(reso=(4, 5, 6), c1=lo, c2=hi, step=0.1, terminate=0.0)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.baked_render(rays, vol, a["reso"], a["c1"], a["c2"], a["step"], terminate=a["terminate"])
        with pytest.raises(ValueError):
            ops.baked_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, vol, a["reso"], a["c1"], a["c2"], a["step"], terminate=a["terminate"])
    with pytest.raises(ValueError):
        ops.baked_render_views(poses, 0, 4, 10.0, None, 0.5, 3.0, vol, (4, 5, 6), lo, hi, 0.1)
    for v, a, b in ((torch.zeros(4, 5, 6), lo, hi), (torch.zeros(4, 5, 6, 3), lo, hi), (vol.double(), lo, hi), (torch.zeros(1, 5, 6, 4), lo, hi),
                    (vol, hi, lo), (vol, lo, (1.0, 1.0))):
        with pytest.raises(ValueError):
            BakedVolume.from_tensor(v, a, b)
    with pytest.raises(ValueError):
        BakedVolume.from_tensor(vol, lo, hi, skip_threshold=float("nan"))
    with pytest.raises(ValueError):
        bv.render(torch.zeros(3, 7))
    with pytest.raises(ValueError):
        bv.render_views(torch.eye(4), 4, 4, 10.0, 0.5, 3.0)
    with pytest.raises(ValueError):
        bv.render_views(poses, 4, 4, 10.0, 0.5, 3.0, gt_rgb=torch.zeros(1, 4, 5, 3))

    class TwoObjects(torch.nn.Module):
        num_objs = 2

    with pytest.raises(ValueError, match="encode one object"):
        BakedVolume.from_model(TwoObjects(), lo, hi, (4, 5, 6))
    with pytest.raises(ValueError):
        BakedVolume.from_model(torch.nn.Linear(3, 4), lo, hi, (4, 5, 6), viewdirs="normal")
    with pytest.raises(ValueError):
        BakedVolume.from_model(torch.nn.Linear(3, 4), lo, hi, (4, 5, 6), viewdirs=(0.0, 0.0, 0.0))
