"""CPU tests of the half-precision baked volumes: util.bake.to_half against numpy's own conversion, the per-value error bound, the
preconditions of the shared fixture (tests/baked_half_ref.py), and the header / binding / entry layer of the four new entries, whose
argument checks all come before any device work."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import baked_half_ref as HR
from pixelnerf_amd import _lib
from pixelnerf_amd.util import bake


def _bits(t):
    return t.view(torch.int16).numpy()


# ---------------------------------------------------------------- to_half

def test_to_half_equals_numpy_bit_for_bit():
    x = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25,        # ties: to even, both ways; half the
                  2.0 ** -24 + 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),  # smallest subnormal; subnormal ties
                  65519.9, 65520.0, 1e6, -1e6, 65504.0, -65504.0, 65503.9, -0.0, 0.0, 6e-8, -3e-6, 0.1, 0.333, 30.0, 2.0 ** -14,
                  np.nextafter(np.float32(2.0 ** -14), np.float32(0))], np.float32)
    want = np.clip(x, -65504, 65504).astype(np.float16)
    with pytest.warns(UserWarning) as rec:
        got = bake.to_half(torch.from_numpy(x))
    assert got.dtype == torch.float16 and got.device.type == "cpu"
    assert np.array_equal(_bits(got), want.view(np.int16))
    assert np.array_equal(want.view(np.int16), HR.half_round(x).view(np.int16))
    assert np.signbit(got.numpy()[13]) and got.numpy()[13] == 0                     # -0.0 stays -0.0
    n_sat = int((np.abs(x) > 65504).sum())
    assert n_sat == 4                                                              # 65519.9, 65520, +-1e6
    messages = [str(w.message) for w in rec if "to_half" in str(w.message)]
    assert len(messages) == 1 and re.search(rf"\b{n_sat} values\b", messages[0])
    assert torch.isfinite(got).all() and float(got.abs().max()) == 65504.0
    # nothing beyond 65504: no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        quiet = bake.to_half(torch.tensor([0.5, -65504.0, 65504.0]))
        again = bake.to_half(quiet)
    assert torch.equal(quiet, torch.tensor([0.5, -65504.0, 65504.0], dtype=torch.float16))
    assert again is quiet or torch.equal(again, quiet)                             # the identity on a half tensor
    with pytest.warns(UserWarning, match=r"\b1 value\b"):
        bake.to_half(torch.tensor([65504.01]))
    # a seeded vector over the whole range, fp64 input too
    rs = np.random.RandomState(5)
    big = (rs.standard_normal(4096) * np.exp(rs.uniform(-20, 11, 4096))).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(_bits(bake.to_half(torch.from_numpy(big))), HR.half_round(big).view(np.int16))


def test_to_half_refuses_non_finite_values():
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="non-finite"):
            bake.to_half(torch.tensor([0.0, bad, 1.0]))
    with pytest.raises(ValueError, match="non-finite"):
        bake.to_half(torch.tensor([float("inf")], dtype=torch.float16))
    with pytest.raises(TypeError):
        bake.to_half(torch.tensor([1, 2]))
    with pytest.raises(TypeError):
        bake.to_half([1.0])


@pytest.mark.parametrize("kind", HR.KINDS, ids=HR.KIND_IDS)
def test_per_value_bound_and_preconditions_on_the_fixture(kind):
    a = HR.fixture(kind)
    with pytest.warns(UserWarning, match=r"\b1 value\b"):                          # the sigma of 1e6
        h = bake.to_half(torch.from_numpy(a))
    assert np.array_equal(_bits(h), HR.half_round(a).view(np.int16))
    wide = h.float().numpy().astype(np.float64)
    inside = np.abs(a) <= 65504
    assert int((~inside).sum()) == 1 and (np.abs(wide[~inside]) == 65504).all()
    err = np.abs(wide - a.astype(np.float64))
    assert (err[inside] <= HR.value_bound(a[inside])).all()
    assert float((err[inside] / HR.value_bound(a[inside])).max()) > 0.9             # (the bound is not slack)
    subnormal, exact_max, saturated, changed, differ = HR.check_preconditions(kind)
    print(f"{kind}: {subnormal} fp16 subnormals, {exact_max} at 65504, {saturated} saturated, {changed:.3f} of the values changed, "
          f"{differ} rays of the fp64 restatement differ")
    assert saturated == 1 and exact_max == 1 and subnormal >= 4
    # the volume for the skip test: its tiny sigmas are positive in fp32 and 0 in fp16
    t = HR.tiny_sigma(kind)
    block = t[2:5, 2:5, 2:5, 3] if kind == "rgba" else t[2:5, 2:5, 2:5, 0, 3]
    assert (block > 0).all() and (block < 2.0 ** -25).all() and (HR.half_round(block) == 0).all()


# ---------------------------------------------------------------- header, binding, entries

NEW = {"pnr_baked_half_render_rays": 17, "pnr_baked_half_render_views": 25, "pnr_baked_sparse_half_render_rays": 19,
       "pnr_baked_sparse_half_render_views": 27}


def test_header_declares_and_binding_binds(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name, n_args in NEW.items():
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)", code)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert "const uint16_t *" in decl.group(1)
        assert hasattr(lib, name)
    # the argument lists of the fp32 counterparts
    assert _lib.PROTOTYPES["pnr_baked_half_render_rays"][1] == _lib.PROTOTYPES["pnr_baked_sh_render_rays"][1]
    assert _lib.PROTOTYPES["pnr_baked_half_render_views"][1] == _lib.PROTOTYPES["pnr_baked_sh_render_views"][1]
    assert _lib.PROTOTYPES["pnr_baked_sparse_half_render_rays"][1] == _lib.PROTOTYPES["pnr_baked_sparse_render_rays"][1]
    assert _lib.PROTOTYPES["pnr_baked_sparse_half_render_views"][1] == _lib.PROTOTYPES["pnr_baked_sparse_render_views"][1]
    assert "gives the BYTES of the fp32 march of the same values widened to fp32" in src


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    lo, hi = _f3(-1, -1, -1), _f3(1, 1, 1)
    P = 64  # a non-null, 16-byte aligned stand-in for a device pointer: every call below must fail before it is touched

    def rays(R=4, rays_p=P, vol=P, degree=2, bits=P, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P, depth=P, alpha=P):
        return lib.pnr_baked_half_render_rays(rays_p, R, vol, degree, bits, n[0], n[1], n[2], c1, c2, step, 0, term, rgb, depth, alpha, None)

    def views(poses=P, NV=1, W=4, H=4, vol=P, degree=2, bits=P, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P, depth=P, alpha=P):
        return lib.pnr_baked_half_render_views(poses, NV, W, H, 10.0, 10.0, 2.0, 2.0, 0.5, 3.0, vol, degree, bits, n[0], n[1], n[2], c1, c2,
                                               step, 0, term, rgb, depth, alpha, None)

    def srays(R=4, rays_p=P, vol=P, M=10, degree=2, index=P, bits=P, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P, depth=P, alpha=P):
        return lib.pnr_baked_sparse_half_render_rays(rays_p, R, vol, M, degree, index, bits, n[0], n[1], n[2], c1, c2, step, 0, term, rgb,
                                                     depth, alpha, None)

    def sviews(poses=P, NV=1, W=4, H=4, vol=P, M=10, degree=2, index=P, bits=P, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P,
               depth=P, alpha=P):
        return lib.pnr_baked_sparse_half_render_views(poses, NV, W, H, 10.0, 10.0, 2.0, 2.0, 0.5, 3.0, vol, M, degree, index, bits, n[0],
                                                      n[1], n[2], c1, c2, step, 0, term, rgb, depth, alpha, None)

    for call in (rays, views, srays, sviews):
        for degree in (-2, 3, 9):
            assert call(degree=degree) == -1 and b"degree" in lib.pnr_last_error()
        for degree in (-1, 0, 1, 2):
            assert call(vol=P + 8, degree=degree) == -1 and b"16-byte" in lib.pnr_last_error()     # a pointer off by 8 bytes
            assert call(vol=None, degree=degree) == -1 and b"null" in lib.pnr_last_error()
        assert call(rgb=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(depth=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(alpha=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(rgb=P + 2) == -1 and b"4-byte" in lib.pnr_last_error()
        assert call(bits=P + 2) == -1 and b"4-byte" in lib.pnr_last_error()
        assert call(n=(1, 4, 4)) == -1 and b"at least 2 grid points" in lib.pnr_last_error()
        assert call(c1=hi, c2=lo) == -1 and b"c1 < c2" in lib.pnr_last_error()
        for step in (0.0, -0.1, float("inf"), float("nan")):
            assert call(step=step) == -1 and b"step" in lib.pnr_last_error()
        for term in (-0.01, 1.0, float("nan")):
            assert call(term=term) == -1 and b"terminate" in lib.pnr_last_error()
    for call in (srays, sviews):
        assert call(M=-1) == -1 and b"bad sizes (M)" in lib.pnr_last_error()
        assert call(index=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(bits=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(index=P + 2) == -1 and b"4-byte" in lib.pnr_last_error()
    for call in (rays, srays):
        assert call(R=-1) == -1 and call(rays_p=None) == -1 and b"null" in lib.pnr_last_error()
        assert call(rays_p=P + 1) == -1 and b"4-byte" in lib.pnr_last_error()
        assert call(R=2 ** 34) == -1 and b"launch limit" in lib.pnr_last_error()
    for call in (views, sviews):
        assert call(NV=-1) == -1 and call(W=0) == -1 and call(H=-3) == -1 and call(poses=None) == -1
    for degree in (-1, 0, 1, 2):                                           # no rays: a no-op
        assert rays(R=0, rays_p=None, vol=None, degree=degree, bits=None, rgb=None, depth=None, alpha=None) == 0
        assert views(NV=0, poses=None, vol=None, degree=degree, bits=None, rgb=None, depth=None, alpha=None) == 0
        for M in (0, 10):
            assert srays(R=0, rays_p=None, vol=None, M=M, degree=degree, index=None, bits=None, rgb=None, depth=None, alpha=None) == 0
            assert sviews(NV=0, poses=None, vol=None, M=M, degree=degree, index=None, bits=None, rgb=None, depth=None, alpha=None) == 0
    assert rays(R=0, degree=3) == -1 and views(NV=0, degree=-2) == -1 and srays(R=0, M=-1) == -1 and sviews(NV=0, degree=3) == -1


def test_wrappers_and_classes_refuse_before_any_device_work():
    from pixelnerf_amd import ops
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    lo, hi, reso = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (4, 5, 6)
    words = (3 * 4 * 5 + 31) // 32
    bits, index = torch.zeros(words, dtype=torch.int32), torch.zeros(reso, dtype=torch.int32)
    rays, poses = torch.zeros(3, 8), torch.eye(4)[None]
    vol16, coef16, rows16 = torch.zeros(reso + (4,), dtype=torch.float16), torch.zeros(reso + (9, 4), dtype=torch.float16), \
        torch.zeros(10, 4, dtype=torch.float16)
    # CPU tensors: there is no CPU path
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_half_render(rays, vol16, None, reso, lo, hi, 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_half_render(rays, coef16, 2, reso, lo, hi, 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_half_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, vol16, -1, reso, lo, hi, 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_sparse_half_render(rays, rows16, None, index, bits, reso, lo, hi, 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_sparse_half_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, rows16, None, index, bits, reso, lo, hi, 0.1)
    for vol, degree in ((vol16, 3), (vol16, -2), (vol16, 0), (coef16, None), (coef16, 1)):
        with pytest.raises(ValueError):
            ops.baked_half_render(rays, vol, degree, reso, lo, hi, 0.1)
    for kw in (dict(step=0.0), dict(step=float("nan")), dict(terminate=1.0), dict(reso=(4, 5)), dict(c1=hi, c2=lo)):
        a = dict(reso=reso, c1=lo, c2=hi, step=0.1, terminate=0.0)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.baked_half_render(rays, vol16, None, a["reso"], a["c1"], a["c2"], a["step"], terminate=a["terminate"])
        with pytest.raises(ValueError):
            ops.baked_sparse_half_render(rays, rows16, None, index, bits, a["reso"], a["c1"], a["c2"], a["step"], terminate=a["terminate"])
    for r, degree in ((rows16, 0), (rows16, 2), (torch.zeros(10, 9, 4, dtype=torch.float16), None), (rows16, 3)):
        with pytest.raises(ValueError):
            ops.baked_sparse_half_render(rays, r, degree, index, bits, reso, lo, hi, 0.1)
    with pytest.raises(ValueError):
        ops.baked_sparse_half_render(rays, rows16, None, None, bits, reso, lo, hi, 0.1)
    with pytest.raises(ValueError):
        ops.baked_half_render_views(poses, 0, 4, 10.0, None, 0.5, 3.0, vol16, -1, reso, lo, hi, 0.1)
    # the classes: fp16 and fp32 are storage types, nothing else is; a CPU tensor is refused after the shape and dtype checks
    occ = OccupancyGrid(bits, reso, lo, hi, 0.0, 0, None)
    for cls, good, bad in ((bake.BakedVolume, vol16, vol16.double()), (bake.BakedSHVolume, coef16, coef16.to(torch.bfloat16))):
        with pytest.raises(_lib.PixelNerfHipError):
            cls(good, lo, hi)
        with pytest.raises(ValueError):
            cls(bad, lo, hi)
    with pytest.raises(_lib.PixelNerfHipError):
        bake.SparseBakedVolume(rows16, occ)
    with pytest.raises(ValueError):
        bake.SparseBakedVolume(rows16.double(), occ)
    sp = bake.SparseBakedVolume.__new__(bake.SparseBakedVolume)           # a volume object without its device parts
    sp.rows, sp.degree, sp.index, sp.occupancy, sp.reso, sp.c1, sp.c2 = rows16, None, index, occ, reso, lo, hi
    assert sp.dtype == torch.float16 and sp.nbytes == 2 * 40 + 4 * (120 + words)
    assert sp.half() is sp
    with pytest.raises(_lib.PixelNerfHipError):
        sp.render(rays)

    class Net(torch.nn.Module):
        num_objs = 1

    for cls, extra in ((bake.BakedVolume, ()), (bake.BakedSHVolume, ()), (bake.SparseBakedVolume, (occ,))):
        with pytest.raises(ValueError, match="dtype"):
            cls.from_model(Net(), lo, hi, reso, *extra, dtype=torch.bfloat16)
