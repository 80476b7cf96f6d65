"""Host tests (no GPU) of the per-sample skipping (skip_empty): the three C entries are declared, exported, bound and refuse bad
arguments before any HIP call; the ABI revision stays 12 and a library without the entries is reported as stale; the numpy
restatement of tests/skip_ref.py agrees with hand-computed cases, and the sphere case the GPU test compares on is neither
vacuous nor hollowed out by exclusions; skip_empty without a grid is refused before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import skip_ref as S
from pixelnerf_amd import _lib

ENTRIES = ("pnr_occupancy_mark_samples", "pnr_compact_samples_workspace_bytes", "pnr_compact_samples", "pnr_expand_rgbsigma")


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
    from pixelnerf_amd import ops
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    for name in ("occupancy_mark_samples", "compact_samples", "expand_rgbsigma"):
        assert callable(getattr(ops, name))
    assert callable(OccupancyGrid.mark_samples)


def test_a_library_without_the_entries_is_reported_as_stale(monkeypatch):
    """the entries were added within revision 12: a revision-12 library built before them must give the usual rebuild message"""
    _lib.build_library()
    real = ctypes.CDLL(_lib.LIB_PATH)

    class Old:
        def __getattr__(self, name):
            if name in ENTRIES[1:]:
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_lib.PixelNerfHipError, match=r"pnr_compact_samples.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_entries_refuse_bad_arguments_on_the_host():
    """PNR_E_INVALID (-1) before any HIP call; the addresses are dummies, never dereferenced"""
    _lib.build_library()
    lib = _lib.load()
    lo, hi = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    mark = lambda rays=64, z=64, R=8, K=4, bits=64, n=(4, 4, 4), c1=lo, c2=hi, keep=64: lib.pnr_occupancy_mark_samples(  # noqa: E731
        rays, z, R, K, bits, n[0], n[1], n[2], c1, c2, keep, None)
    assert mark(n=(4, 1, 4)) == -1 and b"at least 2" in lib.pnr_last_error()
    assert mark(R=-1) == -1 and mark(K=0) == -1 and b"sizes" in lib.pnr_last_error()
    assert mark(R=1 << 16, K=1 << 15) == -1 and b"2^31" in lib.pnr_last_error()
    assert mark(c1=None) == -1 and mark(c2=None) == -1 and b"c1 / c2" in lib.pnr_last_error()
    assert mark(c2=(ctypes.c_float * 3)(1, -1, 1)) == -1 and b"c1 < c2" in lib.pnr_last_error()
    for name in ("rays", "z", "bits", "keep"):
        assert mark(**{name: None}) == -1 and b"null" in lib.pnr_last_error(), name
    assert mark(R=0, rays=None, z=None, keep=None) == 0                                             # R = 0: a no-op

    wsb = lib.pnr_compact_samples_workspace_bytes
    assert wsb(1) == 4 and wsb(256) == 4 and wsb(257) == 8 and wsb(1024 * 67) == 4 * 268
    assert wsb(0) == 0 and wsb(-5) == 0 and wsb(2 ** 31) == 0 and wsb(2 ** 31 - 1) == 4 * 2 ** 23
    comp = lambda keep=64, rays=64, z=64, R=8, K=4, index=64, rays_c=64, z_c=64, count=64, ws=64, nbytes=4: lib.pnr_compact_samples(  # noqa: E731
        keep, rays, z, R, K, index, rays_c, z_c, count, ws, nbytes, None)
    assert comp(R=-1) == -1 and comp(K=0) == -1
    assert comp(R=1 << 16, K=1 << 15) == -1 and b"2^31" in lib.pnr_last_error()
    for name in ("keep", "rays", "z", "index", "rays_c", "z_c", "count", "ws"):
        assert comp(**{name: None}) == -1 and b"null" in lib.pnr_last_error(), name
    assert comp(rays=68) == -1 and comp(rays_c=72) == -1 and b"16-byte" in lib.pnr_last_error()
    assert comp(R=100, K=4, nbytes=4) == -1 and b"workspace" in lib.pnr_last_error()               # 400 samples need 8 bytes
    assert comp(R=0, keep=None, rays=None, ws=None) == 0

    exp = lambda index=64, part=64, M=2, N=8, out=64: lib.pnr_expand_rgbsigma(index, part, M, N, out, None)  # noqa: E731
    assert exp(M=-1) == -1 and exp(N=-1) == -1 and exp(M=9) == -1 and b"sizes" in lib.pnr_last_error()
    assert exp(N=2 ** 31) == -1 and b"2^31" in lib.pnr_last_error()
    assert exp(out=None) == -1 and exp(index=None) == -1 and exp(part=None) == -1 and b"null" in lib.pnr_last_error()
    assert exp(out=68) == -1 and exp(part=72) == -1 and b"16-byte" in lib.pnr_last_error()
    assert exp(M=0, N=0, out=None) == 0


def test_restatement_on_hand_made_samples():
    rays, z, occ, want = S.hand_case()
    assert z.shape[1] == 1
    assert S.mark_ref(rays, z, occ, S.C1, S.C2).reshape(-1).tolist() == want.tolist()
    # compaction and expansion
    keep = np.array([[0, 1, 0], [2, 0, 255]], dtype=np.uint8)
    r2 = np.arange(16, dtype=np.float32).reshape(2, 8)
    z2 = np.array([[1, 2, 3], [4, 5, 6]], dtype=np.float32)
    index, rays_c, z_c, M = S.compact_ref(keep, r2, z2)
    assert M == 3 and index.tolist() == [1, 3, 5] and z_c.tolist() == [2.0, 4.0, 6.0]
    assert np.array_equal(rays_c, r2[[0, 1, 1]])
    part = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    full = S.expand_ref(index, part, 6)
    assert np.array_equal(full[[1, 3, 5]], part) and not full[[0, 2, 4]].any()
    assert not S.expand_ref(index[:0], part[:0], 6).any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sphere_case_is_neither_vacuous_nor_hollow(seed):
    """what keeps the GPU comparison on this case meaningful: 15-30 % of the samples are kept (both classes are populated, and
    some rays keep nothing at all), and at most 0.5 % of them are excluded as ambiguous"""
    rays, z, occ = S.sphere_case(seed)
    assert rays.shape == (256, 8) and z.shape == (256, 32) and occ.shape == (16, 16, 16)
    assert (z[:, 0] >= 0.8).all() and (z[:, -1] <= 3.2).all() and (np.diff(z, axis=1) > 0).all()
    keep = S.mark_ref(rays, z, occ, S.C1, S.C2)
    amb = S.ambiguous(rays, z, occ.shape, S.C1, S.C2)
    none = float((keep.sum(axis=1) == 0).mean())
    print(f"sphere case seed {seed}: kept {keep.mean():.4f}, rays that keep nothing {none:.3f}, ambiguous {100 * amb.mean():.3f} %")
    assert 0.15 <= keep.mean() <= 0.30
    assert amb.mean() <= 0.005
    assert 0.0 < none < 0.5
    # a sample that is kept lies in the box; the fp64 point of an unambiguous kept sample lies in an occupied cell
    P = rays[:, None, :3].astype(np.float64) + z[:, :, None].astype(np.float64) * rays[:, None, 3:6].astype(np.float64)
    sel = (keep == 1) & ~amb
    cell = np.floor((P[sel] + 1.0) / 0.125).astype(int)
    assert (np.abs(P[sel]) <= 1.0).all() and occ[cell[:, 0], cell[:, 1], cell[:, 2]].all()


def test_skip_empty_without_a_grid_is_refused_before_any_device_work():
    import torch
    from pixelnerf_amd.render import NeRFRenderer
    rend = NeRFRenderer(n_coarse=4, n_fine=0)

    def model(*a, **k):
        raise AssertionError("the model must not be called")

    rays = torch.zeros((1, 3, 8))                                                                   # CPU tensors: nothing can launch
    with pytest.raises(ValueError, match="occupancy"):
        rend(model, rays, skip_empty=True)
    with pytest.raises(ValueError, match="occupancy"):
        rend.render_views(model, torch.eye(4)[None], 4, 4, 10.0, 1.0, 2.0, skip_empty=True)
    par = rend.bind_parallel(model, None, simple_output=True)
    with pytest.raises(ValueError, match="occupancy"):
        par(rays, skip_empty=True)
    with pytest.raises(ValueError, match="occupancy"):
        par.render_views(torch.eye(4)[None], 4, 4, 10.0, 1.0, 2.0, skip_empty=True)
    assert rend.last_skip_stats is None
