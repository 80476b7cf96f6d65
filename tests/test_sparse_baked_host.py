"""CPU tests of the sparse baked volumes: the numpy restatement of the kept set (tests/sparse_baked_ref.py) on the shared volume and on
the edge grids, and the header / binding / wrapper layer of the new entries, whose argument checks all come before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baked_ref as B
import sparse_baked_ref as SP
from pixelnerf_amd import _lib


def _occupied_cell_ids(cells):
    return [tuple(int(v) for v in c) for c in np.argwhere(cells)]


# ---------------------------------------------------------------- the restatement

def test_kept_set_of_the_shared_volume():
    sigma = B.common_volume()[..., 3]
    cells = SP.occupied_cells(sigma, 0.0)
    corner, keep = SP.corner_points(cells), SP.kept_points(cells)
    index, ids = SP.sparse_points(cells)
    assert cells.shape == (8, 7, 6) and int(cells.sum()) == 84
    assert int(corner.sum()) == 165 and int(keep.sum()) == 198 == ids.size and keep.size == 504
    assert B.RESO[2] % 2 == 1                                             # nz odd: pairs straddle rows
    assert (keep | ~corner).all()                                         # the closure only adds
    flat = keep.reshape(-1)
    assert (flat[0::2] == flat[1::2]).all()                               # P even: whole pairs
    assert np.array_equal(ids, np.sort(ids)) and ids.dtype == np.int32 and index.dtype == np.int32
    assert np.array_equal(index.reshape(-1)[ids], np.arange(198)) and int((index < 0).sum()) == 504 - 198
    sy, sx = B.RESO[2], B.RESO[1] * B.RESO[2]
    lin = index.reshape(-1)
    for i, j, k in _occupied_cell_ids(cells):
        p000 = (i * B.RESO[1] + j) * B.RESO[2] + k
        for base in (p000, p000 + sy, p000 + sx, p000 + sx + sy):        # every corner kept, every z-pair at consecutive ranks
            assert lin[base] >= 0 and lin[base + 1] == lin[base] + 1, (i, j, k, base)
    # a higher threshold keeps fewer cells and still a proper subset of the points
    cells10 = SP.occupied_cells(sigma, 10.0)
    assert 0 < cells10.sum() < 84 and 0 < SP.sparse_points(cells10)[1].size <= 198


def test_edge_grids():
    g = SP.grids()
    index, ids = SP.sparse_points(g["empty"])
    assert ids.size == 0 and (index == -1).all() and index.shape == (5, 4, 3)
    index, ids = SP.sparse_points(g["full"])
    assert np.array_equal(ids, np.arange(60)) and np.array_equal(index.reshape(-1), np.arange(60))
    index, ids = SP.sparse_points(g["2x2x2"])
    assert np.array_equal(ids, np.arange(8)) and index.shape == (2, 2, 2)
    cells = g["3x3x3 last"]
    corner = SP.corner_points(cells)
    index, ids = SP.sparse_points(cells)
    want_corner = sorted((i * 3 + j) * 3 + k for i in (1, 2) for j in (1, 2) for k in (1, 2))
    assert np.flatnonzero(corner.reshape(-1)).tolist() == want_corner == [13, 14, 16, 17, 22, 23, 25, 26]
    # 27 points: 26 has no partner; 13 brings 12, 16 brings ... 17 is 16's partner, 22/23 and 25/24 likewise
    assert ids.tolist() == [12, 13, 14, 15, 16, 17, 22, 23, 24, 25, 26]
    lin = index.reshape(-1)
    for base in (13, 16, 22, 25):                                         # the four z-pairs of the one occupied cell
        assert lin[base + 1] == lin[base] + 1
    for cells in g.values():                                              # the bit packing helpers are inverses
        reso = tuple(n + 1 for n in cells.shape)
        assert np.array_equal(SP.cells_from_bits(SP.bits_from_cells(cells), reso), cells)


# ---------------------------------------------------------------- header, binding, entries

NEW = {"pnr_sparse_points_mark": 6, "pnr_gen_grid_points_at": 8, "pnr_baked_sparse_render_rays": 19, "pnr_baked_sparse_render_views": 27}


def test_header_declares_and_binding_binds(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name, n_args in NEW.items():
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)", code)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(lib, name)
    # the argument lists of the pnr_baked_sh_render_* pair with (rows, M, degree, index, bits) for (coef, degree, bits)
    assert len(_lib.PROTOTYPES["pnr_baked_sparse_render_rays"][1]) == len(_lib.PROTOTYPES["pnr_baked_sh_render_rays"][1]) + 2
    assert len(_lib.PROTOTYPES["pnr_baked_sparse_render_views"][1]) == len(_lib.PROTOTYPES["pnr_baked_sh_render_views"][1]) + 2
    assert "Sparse baked volumes" in src and "keep[p]   = corner[p] | corner[p ^ 1]" in src


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def _d3(*v):
    return (ctypes.c_double * 3)(*v)


def test_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    lo, hi = _f3(-1, -1, -1), _f3(1, 1, 1)
    P = 64  # a non-null, 16-byte aligned stand-in for a device pointer: every call below must fail before it is touched

    def rays(R=4, rays_p=P, rows=P, M=10, degree=2, index=P, bits=P, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P, depth=P, alpha=P):
        return lib.pnr_baked_sparse_render_rays(rays_p, R, rows, M, degree, index, bits, n[0], n[1], n[2], c1, c2, step, 0, term, rgb,
                                                depth, alpha, None)

    def views(poses=P, NV=1, W=4, H=4, rows=P, M=10, degree=2, index=P, bits=P, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P,
              depth=P, alpha=P):
        return lib.pnr_baked_sparse_render_views(poses, NV, W, H, 10.0, 10.0, 2.0, 2.0, 0.5, 3.0, rows, M, degree, index, bits, n[0], n[1],
                                                 n[2], c1, c2, step, 0, term, rgb, depth, alpha, None)

    for call in (rays, views):
        for degree in (3, -2, 9):
            assert call(degree=degree) == -1 and b"degree" in lib.pnr_last_error()
        assert call(M=-1) == -1 and b"bad sizes (M)" in lib.pnr_last_error()
        for degree in (-1, 0, 1, 2):
            assert call(rows=P + 8, degree=degree) == -1 and b"16-byte" in lib.pnr_last_error()
            assert call(rows=None, degree=degree) == -1 and b"null" in lib.pnr_last_error()
            assert call(index=None, degree=degree) == -1 and b"null" in lib.pnr_last_error()
            assert call(bits=None, degree=degree) == -1 and b"null" in lib.pnr_last_error()
        assert call(index=P + 2) == -1 and b"4-byte" in lib.pnr_last_error()
        assert call(bits=P + 2) == -1 and b"4-byte" in lib.pnr_last_error()
        assert call(rgb=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(depth=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(alpha=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(rgb=P + 2) == -1 and b"4-byte" in lib.pnr_last_error()
        assert call(n=(1, 4, 4)) == -1 and b"at least 2 grid points" in lib.pnr_last_error()
        assert call(c1=hi, c2=lo) == -1 and b"c1 < c2" in lib.pnr_last_error()
        for step in (0.0, -0.1, float("inf"), float("nan")):
            assert call(step=step) == -1 and b"step" in lib.pnr_last_error()
        for term in (-0.01, 1.0, float("nan")):
            assert call(term=term) == -1 and b"terminate" in lib.pnr_last_error()
    assert rays(R=-1) == -1 and rays(rays_p=None) == -1 and rays(rays_p=P + 1) == -1
    assert rays(R=2 ** 34) == -1 and b"launch limit" in lib.pnr_last_error()
    assert views(NV=-1) == -1 and views(W=0) == -1 and views(H=-3) == -1 and views(poses=None) == -1
    for degree in (-1, 0, 1, 2):                                          # no rays: a no-op, whatever M
        for M in (0, 10):
            assert rays(R=0, rays_p=None, rows=None, M=M, degree=degree, index=None, bits=None, rgb=None, depth=None, alpha=None) == 0
            assert views(NV=0, poses=None, rows=None, M=M, degree=degree, index=None, bits=None, rgb=None, depth=None, alpha=None) == 0
    assert rays(R=0, degree=3) == -1 and views(NV=0, degree=-2) == -1 and rays(R=0, M=-1) == -1   # refused even then

    # pnr_sparse_points_mark: what pnr_occupancy_bytes calls an invalid grid, and a null pointer
    for n in ((1, 4, 4), (4, 1, 4), (4, 4, 0), (2, 2 ** 16, 2 ** 16)):
        assert lib.pnr_occupancy_bytes(*n) == 0
        assert lib.pnr_sparse_points_mark(P, n[0], n[1], n[2], P, None) == -1
    assert lib.pnr_sparse_points_mark(None, 4, 4, 4, P, None) == -1 and b"null" in lib.pnr_last_error()
    assert lib.pnr_sparse_points_mark(P, 4, 4, 4, None, None) == -1 and b"null" in lib.pnr_last_error()
    assert lib.pnr_sparse_points_mark(P + 2, 4, 4, 4, P, None) == -1 and b"4-byte" in lib.pnr_last_error()

    # pnr_gen_grid_points_at
    dlo, dhi, reso = _d3(-1, -1, -1), _d3(1, 1, 1), (ctypes.c_int * 3)(4, 5, 6)
    at = lib.pnr_gen_grid_points_at
    assert at(None, dhi, reso, P, 3, P, None, None) == -1 and at(dlo, None, reso, P, 3, P, None, None) == -1
    assert at(dlo, dhi, None, P, 3, P, None, None) == -1 and b"null" in lib.pnr_last_error()
    assert at(dlo, dhi, (ctypes.c_int * 3)(4, 0, 6), P, 3, P, None, None) == -1 and b"reso" in lib.pnr_last_error()
    assert at(dlo, _d3(1, float("inf"), 1), reso, P, 3, P, None, None) == -1 and b"finite" in lib.pnr_last_error()
    assert at(dlo, dhi, reso, P, -1, P, None, None) == -1 and b"count" in lib.pnr_last_error()
    assert at(dlo, dhi, reso, None, 3, P, None, None) == -1 and b"null" in lib.pnr_last_error()
    assert at(dlo, dhi, reso, P, 3, None, None, None) == -1 and b"null" in lib.pnr_last_error()
    assert at(dlo, dhi, reso, P + 2, 3, P, None, None) == -1 and b"4-byte" in lib.pnr_last_error()
    assert at(dlo, dhi, reso, None, 0, None, None, None) == 0            # no points: a no-op


def test_wrappers_refuse_before_any_device_work():
    from pixelnerf_amd import ops
    from pixelnerf_amd.util import bake
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    lo, hi, reso = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (4, 5, 6)
    words = (3 * 4 * 5 + 31) // 32
    bits, index = torch.zeros(words, dtype=torch.int32), torch.zeros(reso, dtype=torch.int32)
    rows, rays, poses = torch.zeros(10, 4), torch.zeros(3, 8), torch.eye(4)[None]
    # CPU tensors: there is no CPU path
    with pytest.raises(_lib.PixelNerfHipError):
        ops.sparse_points(bits, reso)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.gen_grid_points_at(lo, hi, reso, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_sparse_render(rays, rows, None, index, bits, reso, lo, hi, 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_sparse_render(rays, torch.zeros(10, 9, 4), 2, index, bits, reso, lo, hi, 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_sparse_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, rows, None, index, bits, reso, lo, hi, 0.1)
    occ = OccupancyGrid(bits, reso, lo, hi, 0.0, 0, None)
    with pytest.raises(_lib.PixelNerfHipError):
        bake.SparseBakedVolume(rows, occ)
    # shapes and degrees
    for r, degree in ((rows, 0), (rows, 2), (torch.zeros(10, 9, 4), None), (torch.zeros(10, 4, 4), 2), (torch.zeros(10, 3), None),
                      (rows, 3), (rows, -2)):
        with pytest.raises(ValueError):
            ops.baked_sparse_render(rays, r, degree, index, bits, reso, lo, hi, 0.1)
    for kw in (dict(index=None), dict(bits=None), dict(step=0.0), dict(step=float("nan")), dict(terminate=1.0), dict(reso=(4, 5)),
               dict(c1=hi, c2=lo)):
        a = dict(index=index, bits=bits, reso=reso, c1=lo, c2=hi, step=0.1, terminate=0.0)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.baked_sparse_render(rays, rows, None, a["index"], a["bits"], a["reso"], a["c1"], a["c2"], a["step"], terminate=a["terminate"])
    with pytest.raises(ValueError):
        ops.baked_sparse_render_views(poses, 0, 4, 10.0, None, 0.5, 3.0, rows, None, index, bits, reso, lo, hi, 0.1)
    with pytest.raises(TypeError):
        ops.gen_grid_points_at(lo, hi, reso, [1, 2, 3])
    for bad in (torch.zeros(10, 5), torch.zeros(10, 5, 4), torch.zeros(10, 4, dtype=torch.float64), "rows"):
        with pytest.raises(ValueError):
            bake.SparseBakedVolume(bad, occ)
    with pytest.raises(ValueError):
        bake.SparseBakedVolume(rows, "grid")
    sp = bake.SparseBakedVolume.__new__(bake.SparseBakedVolume)           # a volume object without its device parts
    sp.rows, sp.degree, sp.index, sp.occupancy, sp.reso, sp.c1, sp.c2 = rows, None, index, occ, reso, lo, hi
    assert sp.n_rows == 10 and sp.nbytes == 4 * (40 + 120 + words) and sp.cell_size == (2 / 3, 2 / 4, 2 / 5)
    with pytest.raises(ValueError, match="skip=False"):
        sp.render(rays, skip=False)
    with pytest.raises(ValueError, match="skip=False"):
        sp.render_views(poses, 4, 4, 10.0, 0.5, 3.0, skip=False)
    with pytest.raises(_lib.PixelNerfHipError):
        sp.render(rays)

    class TwoObjects(torch.nn.Module):
        num_objs = 2

    with pytest.raises(ValueError, match="encode one object"):
        bake.SparseBakedVolume.from_model(TwoObjects(), lo, hi, reso, occ)
    with pytest.raises(ValueError, match="OccupancyGrid"):
        bake.SparseBakedVolume.from_model(torch.nn.Linear(3, 4), lo, hi, reso, None)
    with pytest.raises(ValueError, match="spans"):
        bake.SparseBakedVolume.from_model(torch.nn.Linear(3, 4), lo, hi, (4, 5, 7), occ)
    assert hasattr(bake.BakedVolume, "sparse") and hasattr(bake.BakedSHVolume, "sparse")
