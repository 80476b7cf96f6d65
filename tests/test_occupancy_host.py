"""Host tests (no GPU) of the occupancy-grid ray culling: the new C entries are declared, exported, bound and refuse bad arguments
before any HIP call; util.occupancy.OccupancyGrid validates what it is given; the numpy restatement of tests/occ_ref.py agrees with
hand-computed cases; and the one-sided bracket the GPU test holds the device to is not vacuous on the rays it uses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import occ_ref as R
from pixelnerf_amd import _lib

ENTRIES = ("pnr_occupancy_bytes", "pnr_occupancy_build", "pnr_occupancy_clip_rays", "pnr_philox_noise_ids")


def test_header_declares_the_entries_and_the_abi_revision_stays_12(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    _lib.build_library()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and re.search(name + r"\s*\(", code), name
        assert hasattr(lib, name), name
    assert lib.pnr_abi_version() == 12
    assert "pnr_occupancy.hip" in _lib.SOURCES
    from pixelnerf_amd import ops
    for name in ("occupancy_build", "occupancy_clip_rays", "philox_noise_ids"):
        assert callable(getattr(ops, name))


def test_entries_refuse_bad_arguments_on_the_host():
    """PNR_E_INVALID (-1) before any HIP call; the addresses are dummies, never dereferenced"""
    _lib.build_library()
    lib = _lib.load()
    assert lib.pnr_occupancy_bytes(2, 2, 2) == 4 and lib.pnr_occupancy_bytes(5, 6, 7) == 16 and lib.pnr_occupancy_bytes(3, 4, 35) == 28
    assert lib.pnr_occupancy_bytes(128, 128, 128) == (127 ** 3 + 31) // 32 * 4                     # 250 KiB: it lives in L2
    assert lib.pnr_occupancy_bytes(1292, 1292, 1292) == 0 and 1291 ** 3 >= 2 ** 31 > 1290 ** 3       # 2^31 cells and more
    assert lib.pnr_occupancy_bytes(1291, 1291, 1291) == (1290 ** 3 + 31) // 32 * 4
    for n in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, -2, 4)):
        assert lib.pnr_occupancy_bytes(*n) == 0
    build = lambda field=64, n=(4, 4, 4), thr=0.5, dilate=1, bits=64, count=None: lib.pnr_occupancy_build(  # noqa: E731
        field, n[0], n[1], n[2], thr, dilate, bits, count, None)
    for n in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        assert build(n=n) == -1 and b"at least 2" in lib.pnr_last_error(), n
    assert build(n=(1292, 1292, 1292)) == -1 and b"2^31" in lib.pnr_last_error()
    for d in (-1, 5):
        assert build(dilate=d) == -1 and b"dilate" in lib.pnr_last_error()
    assert build(thr=float("nan")) == -1 and b"threshold" in lib.pnr_last_error()
    assert build(field=None) == -1 and b"field" in lib.pnr_last_error()
    assert build(bits=None) == -1 and b"bits" in lib.pnr_last_error()
    lo, hi = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    clip = lambda rays=64, R=8, bits=64, n=(4, 4, 4), c1=lo, c2=hi, pad=0.0, tb=64, hit=64: lib.pnr_occupancy_clip_rays(  # noqa: E731
        rays, R, bits, n[0], n[1], n[2], c1, c2, pad, tb, hit, None)
    assert clip(n=(4, 1, 4)) == -1 and b"at least 2" in lib.pnr_last_error()
    assert clip(R=-1) == -1
    assert clip(c1=None) == -1 and clip(c2=None) == -1 and b"c1 / c2" in lib.pnr_last_error()
    assert clip(c2=(ctypes.c_float * 3)(1, -1, 1)) == -1 and b"c1 < c2" in lib.pnr_last_error()
    assert clip(c1=(ctypes.c_float * 3)(float("nan"), -1, -1)) == -1
    for pad in (-0.1, float("nan"), float("inf")):
        assert clip(pad=pad) == -1 and b"pad" in lib.pnr_last_error()
    assert clip(rays=None) == -1 and clip(bits=None) == -1 and clip(tb=None) == -1 and clip(hit=None) == -1
    assert clip(R=0, rays=None, tb=None, hit=None) == 0                                             # no rays: a no-op
    ids = lambda seed=1, ray_ids=64, R=4, Kc=8, Kimp=5, Kfd=3, u=64: lib.pnr_philox_noise_ids(  # noqa: E731
        seed, ray_ids, R, Kc, Kimp, Kfd, u, u, u, u, None)
    assert ids(R=-1) == -1 and ids(Kc=-1) == -1 and b"bad sizes" in lib.pnr_last_error()
    assert ids(u=None) == -1 and b"null output" in lib.pnr_last_error()
    assert ids(ray_ids=None) == -1 and b"ray_ids" in lib.pnr_last_error()
    assert ids(R=0, ray_ids=None, u=None) == 0 and ids(Kc=0, Kimp=0, Kfd=0, ray_ids=None, u=None) == 0   # nothing to draw


def test_operators_and_the_grid_validate_their_arguments():
    from pixelnerf_amd import ops
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    with pytest.raises(_lib.PixelNerfHipError):
        ops.occupancy_build(torch.zeros(4, 4, 4), 0.5)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.occupancy_clip_rays(torch.zeros(2, 8), torch.zeros(1, dtype=torch.int32), (4, 4, 4), (-1,) * 3, (1,) * 3)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.philox_noise_ids(torch.zeros(4, dtype=torch.int64), 8, 8, 3, 1)
    with pytest.raises(TypeError):
        ops.philox_noise_ids([1, 2, 3], 8, 8, 3, 1)
    bits = torch.zeros(1, dtype=torch.int32)                       # 27 cells of a 4^3 grid: one word
    occ = OccupancyGrid(bits, (4, 4, 4), (-1, -1, -1), (1, 1, 1), 0.5, 1, torch.tensor(0, dtype=torch.int32))
    assert occ.reso == (4, 4, 4) and occ.n_cells == 27 and occ.occupied_fraction == 0.0 and occ.dilate == 1 and occ.threshold == 0.5
    for bad in (dict(reso=(4, 1, 4)), dict(reso=(4, 4)), dict(c2=(1, -1, 1)), dict(c1=(0, 0)), dict(dilate=5), dict(dilate=-1),
                dict(bits=torch.zeros(2, dtype=torch.int32)), dict(bits=torch.zeros(1, dtype=torch.int64)), dict(bits=[0]),
                dict(reso=(1292, 1292, 1292))):
        kw = dict(bits=bits, reso=(4, 4, 4), c1=(-1, -1, -1), c2=(1, 1, 1), threshold=0.5, dilate=1, n_occupied=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            OccupancyGrid(**kw)
    with pytest.raises(ValueError):
        OccupancyGrid.from_density(torch.zeros(4, 4), (-1,) * 3, (1,) * 3, 0.5)
    with pytest.raises(ValueError, match="dilate"):
        OccupancyGrid.from_density(torch.zeros(4, 4, 4), (-1,) * 3, (1,) * 3, 0.5, dilate=7)       # before any device work
    with pytest.raises(_lib.PixelNerfHipError):
        OccupancyGrid.from_density(torch.zeros(4, 4, 4), (-1,) * 3, (1,) * 3, 0.5)                  # a host tensor: no CPU path
    with pytest.raises(ValueError, match=r"\(\.\.\.,8\)"):
        occ.clip_rays(torch.zeros(3, 7))

    class Two(torch.nn.Module):
        num_objs = 2

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    with pytest.raises(ValueError, match="2 objects"):
        OccupancyGrid.from_model(Two(), (-1,) * 3, (1,) * 3, (4, 4, 4), 0.5)


def test_renderer_refuses_what_culling_cannot_do():
    """the refusals come before any device work: more than one object, a call that needs gradients"""
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    occ = OccupancyGrid(torch.zeros(1, dtype=torch.int32), (4, 4, 4), (-1, -1, -1), (1, 1, 1), 0.5, 1, None)
    rend = NeRFRenderer(n_coarse=8, n_fine=0).eval()

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, xyz, coarse=True, viewdirs=None):
            return xyz.new_zeros(*xyz.shape[:2], 4)

    with pytest.raises(ValueError, match="ONE object"):
        rend(Model(), torch.zeros(2, 5, 8), occupancy=occ)
    with pytest.raises(NotImplementedError, match="inference"):
        rend(Model(), torch.zeros(1, 5, 8), occupancy=occ)          # grad mode on, a parameter requires grad
    two = Model()
    two.num_objs = 2
    with torch.no_grad(), pytest.raises(ValueError, match="ONE object"):
        rend(two, torch.zeros(1, 5, 8), occupancy=occ)
    with pytest.raises(ValueError, match="ONE object"):
        rend.render_views(Model(), torch.eye(4).expand(2, 3, 4, 4), 4, 4, 5.0, 1.0, 3.0, occupancy=occ)


def test_build_ref_against_hand_computed_cases():
    f = np.zeros((2, 2, 2), np.float32)
    assert not R.build_ref(f, 0.0).any()                                            # == threshold is empty
    f[1, 0, 1] = np.float32(1e-30)
    assert R.build_ref(f, 0.0).all() and R.pack_bits(R.build_ref(f, 0.0)).tolist() == [1]
    for special in (np.nan, np.inf, -np.inf):                                       # non-finite: occupied
        g = np.full((2, 2, 2), -5.0, np.float32)
        g[0, 1, 0] = special
        assert R.build_ref(g, 0.0).all(), special
    f = np.zeros((3, 3, 3), np.float32)
    f[0, 0, 0] = 1.0                                                                # a corner point: cell (0,0,0) only
    assert R.pack_bits(R.build_ref(f, 0.5)).tolist() == [0x01]
    assert R.pack_bits(R.build_ref(f, 0.5, 1)).tolist() == [0xFF]                   # Chebyshev 1 in a 2x2x2 block of cells: all
    assert not R.build_ref(f, 1.0).any()
    f[:] = 0.0
    f[2, 2, 2] = 1.0                                                                # the opposite corner: cell (1,1,1), index 7
    assert R.pack_bits(R.build_ref(f, 0.5)).tolist() == [0x80]
    f[:] = 0.0
    f[1, 1, 1] = 1.0                                                                # the centre point touches all 8 cells
    assert R.pack_bits(R.build_ref(f, 0.5)).tolist() == [0xFF]
    f[:] = 0.0
    f[0, 1, 2] = 1.0                                                                # cells (0,0,1), (0,1,1): indices 1 and 3
    assert R.pack_bits(R.build_ref(f, 0.5)).tolist() == [0x0A]
    f = np.zeros((2, 2, 6), np.float32)                                             # a row of 5 cells: dilation along k only
    f[0, 0, 0] = 1.0
    assert [R.pack_bits(R.build_ref(f, 0.5, d)).tolist() for d in (0, 1, 2, 4)] == [[0b00001], [0b00011], [0b00111], [0b11111]]
    occ, rest = R.unpack_bits(np.array([0x0A], np.uint32), (2, 2, 2))
    assert occ[0, 0, 1] and occ[0, 1, 1] and occ.sum() == 2 and not rest.any()


def test_clip_ref_against_hand_computed_cases():
    one = np.ones((1, 1, 1), bool)                                                  # 2x2x2 points over [-1,1]^3: one cell, h = 2
    ray = lambda o, d, near=0.5, far=4.5: np.array([[*o, *d, near, far]], np.float64)  # noqa: E731
    c1, c2 = (-1, -1, -1), (1, 1, 1)
    hit, te, tx = R.clip_ref(ray((0, 0, -3), (0, 0, 1)), one, c1, c2)
    assert hit[0] and te[0] == 2.0 and tx[0] == 4.0
    hit, te, tx = R.clip_ref(ray((0, 0, -3), (0, 0, 1)), one, c1, c2, pad=0.75)
    assert hit[0] and te[0] == 1.25 and tx[0] == 4.5                                # the exit is clamped to far
    hit, te, tx = R.clip_ref(ray((0, 0, -3), (0, 0, 1)), one, c1, c2, inflate=0.25)  # grown by 0.25 h = 0.5 per side
    assert hit[0] and te[0] == 1.5 and tx[0] == 4.5
    hit, te, tx = R.clip_ref(ray((0, 0, -3), (0, 0, 1)), one, c1, c2, inflate=-0.25)
    assert hit[0] and te[0] == 2.5 and tx[0] == 3.5
    assert not R.clip_ref(ray((1.2, 0, -3), (0, 0, 1)), one, c1, c2)[0][0]          # passes beside the cell ...
    assert R.clip_ref(ray((1.2, 0, -3), (0, 0, 1)), one, c1, c2, inflate=0.25)[0][0]  # ... but inside the grown one
    assert R.clip_ref(ray((1.0, 0, -3), (0, 0, 1)), one, c1, c2)[0][0]              # in the face plane: closed intervals
    assert not R.clip_ref(ray((1.0, 0, -3), (0, 0, 1)), one, c1, c2, inflate=-R.DELTA)[0][0]
    hit, te, tx = R.clip_ref(ray((0, 0, 0), (0, 0, 2), near=0.0), one, c1, c2)      # origin inside: t_enter = near; d not unit
    assert hit[0] and te[0] == 0.0 and tx[0] == 0.5
    hit, te, tx = R.clip_ref(ray((0, 0, -3), (0, 0, 1), near=2.5, far=3.0), one, c1, c2)
    assert hit[0] and te[0] == 2.5 and tx[0] == 3.0                                 # near / far cut the cell
    hit, te, tx = R.clip_ref(ray((0, 0, -3), (0, 0, 1), near=0.5, far=1.5), one, c1, c2)
    assert not hit[0] and te[0] == 0.5 and tx[0] == 1.5                             # the segment ends in front of it
    two = np.zeros((2, 2, 2), bool)                                                 # 3x3x3 points: cells of size 1
    two[0, 0, 0] = two[1, 1, 1] = True
    hit, te, tx = R.clip_ref(np.concatenate([ray((-0.5, -0.5, -3), (0, 0, 1)), ray((0.5, 0.5, -3), (0, 0, 1)),
                                             ray((-0.5, 0.5, -3), (0, 0, 1)), ray((-3, -3, -3), (1, 1, 1), far=9.0)]), two, c1, c2)
    assert hit.tolist() == [True, True, False, True]
    assert te[:2].tolist() == [2.0, 3.0] and tx[:2].tolist() == [3.0, 4.0]
    assert te[3] == 2.0 and tx[3] == 4.0                                            # the diagonal: first cell in, last cell out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_bracket_is_not_vacuous(seed):
    """on the 4096 rays of the GPU test the cells grown and shrunk by DELTA * h disagree on at most 1 % of the rays, and both
    classes -- hit and missed -- hold at least a quarter of them (seed 0 is the GPU test's)"""
    occ = R.random_cells(seed)
    assert 0.05 <= occ.mean() <= 0.15
    ambiguous, hit = R.vacuity(R.sphere_rays(seed), occ)
    print(f"seed {seed}: {occ.mean():.3f} of the cells occupied, {100 * ambiguous:.3f} % of the rays ambiguous, {100 * hit:.1f} % hit")
    assert ambiguous <= 0.01 and 0.25 <= hit <= 0.75
