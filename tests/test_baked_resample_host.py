"""CPU tests of pnr_baked_resample: the restatement of tests/baked_resample_ref.py against the properties the entry promises (the
identity, old points kept under refinement, the march of a refined volume), the entry of the ABI and every refusal, word for word
and in order, the Python layer's refusals, and the input conditions of tests/test_hip_baked_resample.py.  No call reaches a launch."""
import os
import re

import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_resample_ref as RS

from pixelnerf_amd import _lib

ENTRY = "pnr_baked_resample"
NON_INTEGER = (((5, 6, 7), (7, 4, 10)), ((6, 5, 9), (9, 7, 4)))   # 7 -> 10 and 9 -> 4 among them


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---------------------------------------------------------------- 1. the restatement's own properties
@pytest.mark.parametrize("reso", RS.GRIDS)
@pytest.mark.parametrize("kind", RS.KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_same_reso_is_the_identity(reso, kind, dtype):
    v = RS.volume(reso, kind)
    assert (v == 0).any() and np.signbit(v[v == 0]).any()                       # the volume holds -0
    out = RS.resample(v, reso, dtype)
    assert torch.equal(_bits(out), _bits(torch.tensor(v).to(dtype)))


@pytest.mark.parametrize("reso", RS.GRIDS)
@pytest.mark.parametrize("m", [2, 3])
def test_refinement_keeps_the_old_points_at_stride(reso, m):
    for kind in RS.KINDS:
        v = RS.volume(reso, kind)
        out = RS.resample(v, RS.refined(reso, m), torch.float32)
        assert tuple(out.shape[:3]) == RS.refined(reso, m)
        assert torch.equal(_bits(out[::m, ::m, ::m].contiguous()), _bits(torch.tensor(v)))


def test_fp64_march_of_a_volume_refined_by_2_is_the_march_of_the_original():
    """the trilinear interpolant of a trilinear function is that function: the refined volume describes the same field, and the
    samples are the same points"""
    vol, rays = G.rgba_volume(0.15), G.case_rays("n150")
    fine = RS.resample(vol, RS.refined(G.RESO, 2), torch.float64)
    a = G.march(rays, G._fp32(vol, torch.float64), G.C1, G.C2, 0.03)
    b = G.march(rays, fine, G.C1, G.C2, 0.03)
    for x, y in zip(a, b):
        assert float(x.abs().max()) > 0 and float((x - y).abs().max()) <= 1e-12


def test_sparse_source_reads_dropped_corners_as_zeros():
    import sparse_baked_ref as SP
    reso = RS.GRIDS[0]
    kept = SP.kept_points(RS.cells(reso))
    assert 0 < kept.sum() < kept.size
    v = RS.volume(reso, 1)
    dense = np.where(kept[..., None, None], v, np.float32(0))
    assert torch.equal(RS.resample(v, RS.refined(reso, 2), torch.float32, kept=kept), RS.resample(dense, RS.refined(reso, 2), torch.float32))


# ---------------------------------------------------------------- 2. the entry and its refusals
def test_entry_is_declared_bound_and_exported_within_abi_12(repo_root):
    header = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert "#define PNR_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    decl = re.search(ENTRY + r"\s*\(([^;]*)\)\s*;", code)
    assert decl and len(decl.group(1).split(",")) == 15 == len(_lib.PROTOTYPES[ENTRY][1])
    assert hasattr(lib, ENTRY) and "pnr_baked_resample.hip" in _lib.SOURCES


P = 64  # a non-null, 16-byte aligned stand-in for a device pointer
GOOD = dict(src=P, half=0, M=10, degree=2, index=None, n=(4, 4, 4), dst=P, M_dst=5, ids_dst=None, n_dst=(7, 7, 7))


def _call(lib, **defect):
    a = dict(GOOD)
    a.update(defect)
    rc = lib.pnr_baked_resample(a["src"], a["half"], a["M"], a["degree"], a["index"], *a["n"], a["dst"], a["M_dst"], a["ids_dst"], *a["n_dst"],
                                None)
    return rc, (lib.pnr_last_error().decode() if rc != 0 else "")


def test_every_refusal_of_the_entry():
    """each call carries one defect (or a pair that pins the order) and stand-in pointers that are never touched"""
    lib = _lib.load()
    degree, storage = "degree must be -1 (RGBA), 0, 1 or 2", "storage_half must be 0 or 1"
    axis, points = "every axis needs at least 2 grid points", "the grid must have fewer than 2^31 points"
    aligned4 = "index and ids_dst must be 4-byte aligned"
    expect = [
        (dict(degree=3), degree), (dict(degree=-2), degree),
        (dict(half=2), storage), (dict(half=-1), storage),
        (dict(n=(1, 4, 4)), axis), (dict(n_dst=(4, 4, 1)), axis),
        (dict(n=(2 ** 11, 2 ** 10, 2 ** 10)), points), (dict(n_dst=(2, 2 ** 15, 2 ** 15)), points),
        (dict(n=(2 ** 30, 2 ** 30, 2 ** 30)), points),
        (dict(M=-1, index=P), "bad sizes (M)"), (dict(M_dst=-1, ids_dst=P), "bad sizes (M)"),
        (dict(dst=None), "null argument"), (dict(src=None), "null argument"), (dict(src=None, index=P), "null argument"),
        (dict(src=P + 8), "src must be 16-byte aligned"), (dict(src=P + 4, half=1), "src must be 8-byte aligned"),
        (dict(dst=P + 8), "dst must be 16-byte aligned"),
        (dict(index=P + 2), aligned4), (dict(ids_dst=P + 1), aligned4),
        # two defects: the earlier check speaks
        (dict(degree=3, half=2), degree),
        (dict(half=2, n=(1, 4, 4)), storage),
        (dict(n=(1, 4, 4), n_dst=(2 ** 11, 2 ** 10, 2 ** 10)), axis),
        (dict(n=(2 ** 11, 2 ** 10, 2 ** 10), M=-1, index=P), points),
        (dict(M=-1, index=P, dst=None), "bad sizes (M)"),
        (dict(dst=None, src=P + 8), "null argument"),
        (dict(src=P + 8, index=P + 2), "src must be 16-byte aligned"),
        (dict(dst=P + 8, ids_dst=P + 2), "dst must be 16-byte aligned"),
    ]
    for defect, words in expect:
        assert _call(lib, **defect) == (-1, f"{ENTRY}: {words}"), (defect, _call(lib, **defect))
    # a dense call looks at neither M; an fp16 source needs 8 bytes only (refused for the last check: all others passed); no
    # destination rows: a no-op that looks at no pointer; a sparse source without rows needs no src
    assert _call(lib, M=-1, M_dst=-1, dst=P + 8) == (-1, f"{ENTRY}: dst must be 16-byte aligned")
    assert _call(lib, src=P + 8, half=1, index=P + 2) == (-1, f"{ENTRY}: {aligned4}")
    assert _call(lib, M_dst=0, ids_dst=P, src=None, dst=None) == (0, "")
    assert _call(lib, M=0, src=None, index=P, ids_dst=P + 2) == (-1, f"{ENTRY}: {aligned4}")


def test_python_layer_refuses_before_any_device_work():
    from pixelnerf_amd import ops
    from pixelnerf_amd.util import bake
    vol = torch.zeros(4, 4, 4, 4)
    with pytest.raises(ValueError, match=r"degree must be None / -1 \(RGBA\), 0, 1 or 2, got 3"):
        ops.baked_resample(vol, 3, (4, 4, 4), (7, 7, 7))
    with pytest.raises(ValueError, match="at least 2 points per axis and fewer than 2\\^31 points"):
        ops.baked_resample(vol, None, (4, 4, 4), (7, 1, 7))
    with pytest.raises(ValueError, match=r"stored must be \(4,4,4,4,4\) at degree 1"):
        ops.baked_resample(vol, 1, (4, 4, 4), (7, 7, 7))
    with pytest.raises(TypeError, match="float32 or float16"):
        ops.baked_resample(vol.double(), None, (4, 4, 4), (7, 7, 7))
    with pytest.raises(_lib.PixelNerfHipError, match="no CPU path"):
        ops.baked_resample(vol, None, (4, 4, 4), (7, 7, 7))
    # reso: an int or three ints
    assert bake._resample_reso("x", 9) == (9, 9, 9) and bake._resample_reso("x", (5, 6, np.int64(7))) == (5, 6, 7)
    for bad in (1, 2.5, (4, 4), (4, 4, 1), "9", (4, 4.0, 4), True, None):
        with pytest.raises(ValueError, match="x: "):
            bake._resample_reso("x", bad)
    # a sparse volume: integer refinements only, found on the host
    assert bake._sparse_refinement("x", (5, 6, 7), (9, 16, 7)) == (2, 3, 1)
    for new in ((10, 11, 13), (5, 6, 8), (3, 6, 7)):
        with pytest.raises(ValueError, match="a sparse volume takes integer refinements only"):
            bake._sparse_refinement("x", (5, 6, 7), new)
    sparse = object.__new__(bake.SparseBakedVolume)   # (no device: the refusal comes before anything looks at the rows)
    sparse.reso, sparse.rows = (5, 6, 7), torch.zeros(3, 4)
    with pytest.raises(ValueError, match=r"SparseBakedVolume.resample: a sparse volume takes integer refinements only"):
        sparse.resample((7, 11, 13))
    for cls in (bake.BakedVolume, bake.BakedSHVolume, bake.SparseBakedVolume):
        assert callable(cls.resample) and callable(cls.prune)
    # the bitfield helpers of the sparse refinement agree with the kernel's layout (sparse_baked_ref restates it)
    import sparse_baked_ref as SP
    cells = RS.cells(RS.GRIDS[1])
    bits = bake._bits_of(torch.from_numpy(np.array(cells)))
    assert bits.dtype == torch.int32 and np.array_equal(bits.numpy().view(np.uint32), SP.bits_from_cells(cells).view(np.uint32))
    assert np.array_equal(bake._cells_of(bits, RS.GRIDS[1]).numpy(), cells) and int(bake._count_bits(bits)) == int(cells.sum())


# ---------------------------------------------------------------- 3. the input conditions of the GPU tests
@pytest.mark.parametrize("reso,new", NON_INTEGER)
def test_fp32_restatement_is_within_4_ulp_of_the_fp64_one(reso, new):
    """the bar of the GPU test, met by the fp32 restatement: |fp32 - fp64| <= 4 ulp of the largest stored magnitude"""
    worst = 0.0
    for kind in RS.KINDS:
        v = RS.volume(reso, kind)
        r64, r32 = RS.resample(v, new, torch.float64), RS.resample(v, new, torch.float32)
        ulp = RS.ulp32(np.abs(v).max())
        worst = max(worst, float((r32.double() - r64).abs().max()) / ulp)
        assert not torch.equal(r32.double(), r64)                                  # the fractions are not all dyadic
    print(f"{reso} -> {new}: {worst:.2f} ulp")
    assert worst <= 4.0
