"""CPU tests of the visibility of a baked volume: the restatement of tests/baked_visibility_ref.py against baked_grad_ref.march and
against the properties the entries promise, the two entries of the ABI and every refusal, word for word and in order, the Python
layer's refusals (visibility, prune, fit_coarse_to_fine), and the input conditions of tests/test_hip_baked_visibility.py.  No call
reaches a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_visibility_ref as V

from pixelnerf_amd import _lib

RAYS_ENTRY, VIEWS_ENTRY = "pnr_baked_visibility_rays", "pnr_baked_visibility_views"


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("name", V.CASE_IDS)
def test_weights_are_those_of_baked_grad_ref_march(name):
    """sum_i w_i of the walk is march()'s alpha, to the last bit, at both precisions: the same samples, the same weights, the same stop"""
    case = V.BY_NAME[name]
    inp = V.inputs(case)
    for dtype in (torch.float64, torch.float32):
        info = {}
        V.visibility(inp["rays"], inp["stored"], V.C1, V.C2, V.STEP, dtype=dtype, info=info, **inp["kw"])
        alpha = G.march(inp["rays"], G._fp32(inp["stored"], dtype), V.C1, V.C2, V.STEP, dtype=dtype, **inp["kw"])[2]
        assert torch.equal(info["alpha"], alpha) and float(alpha.max()) > 0.5


@pytest.mark.parametrize("name", V.CASE_IDS)
def test_visibility_lies_between_zero_and_the_largest_weight(name):
    _, v64, v32, info = V.reference(V.BY_NAME[name])
    for v in (v64, v32):
        assert float(v.min()) >= 0.0 and 0.0 < float(v.max()) <= info["w_max"] * (1 + 1e-6)
    assert not bool(v64[~info["touched"]].any())


@pytest.mark.parametrize("name", ["rgba", "sh2_bits_terminate"])
def test_visibility_does_not_depend_on_order_or_batches(name):
    """a maximum: exactly the same field for permuted rays and for three accumulating calls"""
    inp, v64, _, _ = V.reference(V.BY_NAME[name])
    rays = inp["rays"]
    perm = np.random.RandomState(3).permutation(rays.shape[0])
    call = lambda r, out=None: V.visibility(r, inp["stored"], V.C1, V.C2, V.STEP, out=out, **inp["kw"])
    assert torch.equal(call(rays[perm]), v64)
    acc = None
    for part in np.array_split(perm, 3):
        acc = call(rays[part], acc)
    assert torch.equal(acc, v64)


# ---------------------------------------------------------------- 2. the input conditions of the GPU tests
@pytest.mark.parametrize("name", V.CASE_IDS)
def test_cases_meet_the_conditions_of_the_gpu_tests(name):
    case = V.BY_NAME[name]
    inp, v64, v32, info = V.reference(case)
    n = info["n"]
    assert inp["rays"].shape[0] <= 96
    assert float((v64 > 0).float().mean()) >= 0.25                      # a quarter of the grid points is seen
    assert int((info["chunks"] >= 2).sum()) >= 1                          # a ray with two active chunks
    assert int((n > 128).sum()) >= 1                                      # the carry crosses two chunk boundaries
    if case.terminate:
        assert int(info["stopped"].sum()) >= 1                            # a ray stops early ...
        free = V.visibility(inp["rays"], inp["stored"], V.C1, V.C2, V.STEP, **dict(inp["kw"], terminate=0.0))
        if case.kind is None:   # ... and in the RGBA case the stop shows in the field (behind the stop of the degree-2 case every
            assert not torch.equal(free, v64)   # weight is below a maximum another ray has set)
    else:
        assert int(((n > 0) & (n < 64)).sum()) >= 1                       # rays of fewer than 64 samples
    err32 = V.error(v32.double(), v64)
    print(f"{name}: seen {float((v64 > 0).float().mean()):.3f}, fp32 restatement against fp64 {err32:.2e}, bar {V.bar_from(err32):.2e}")
    assert err32 < 1e-5
    if case.thr is not None:   # a sparse volume holds every point the walk writes
        import sparse_baked_ref as SP
        assert not bool(v64[~torch.from_numpy(SP.kept_points(inp["occupied"]))].any())


def test_contention_rays_are_one_ray():
    rays = V.contention_rays(V.BY_NAME["rgba"])
    assert rays.shape == (64, 8) and (rays == rays[0]).all()
    inp = V.inputs(V.BY_NAME["rgba"])
    one = V.visibility(rays[:1], inp["stored"], V.C1, V.C2, V.STEP, **inp["kw"])
    assert torch.equal(V.visibility(rays, inp["stored"], V.C1, V.C2, V.STEP, **inp["kw"]), one) and float(one.max()) > 0


# ---------------------------------------------------------------- 3. the entries and their refusals
def test_visibility_entries_are_declared_exported_and_bound(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name, n_args in ((RAYS_ENTRY, 17), (VIEWS_ENTRY, 25)):
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(lib, name)
    # pnr_baked_ray_backward_*'s list without white_bkgd and the three upstream gradients
    for new, old in ((RAYS_ENTRY, "pnr_baked_ray_backward_rays"), (VIEWS_ENTRY, "pnr_baked_ray_backward_views")):
        args = list(_lib.PROTOTYPES[old][1])
        del args[-5:-2]        # d_rgb, d_depth, d_alpha
        del args[-4]           # white_bkgd
        assert args == list(_lib.PROTOTYPES[new][1])
    assert "pnr_baked_visibility.hip" in _lib.SOURCES


P = 64  # a non-null, 16-byte aligned stand-in for a device pointer
GOOD = dict(rays=P, R=4, poses=P, NV=1, W=4, H=4, stored=P, half=0, M=10, degree=2, index=None, bits=None, n=(4, 4, 4),
            c1=(-1.0, -1.0, -1.0), c2=(1.0, 1.0, 1.0), step=0.1, term=0.0, vis=P)


def _call(lib, name, **defect):
    a = dict(GOOD)
    a.update(defect)
    f3 = ctypes.c_float * 3
    args = [a["poses"], a["NV"], a["W"], a["H"], 10.0, 10.0, 2.0, 2.0, 0.5, 3.0] if name == VIEWS_ENTRY else [a["rays"], a["R"]]
    args += [a["stored"], a["half"], a["M"], a["degree"], a["index"], a["bits"], *a["n"], f3(*a["c1"]), f3(*a["c2"]), a["step"], a["term"],
             a["vis"], None]
    rc = getattr(lib, name)(*args)
    return rc, (lib.pnr_last_error().decode() if rc != 0 else "")


@pytest.mark.parametrize("name", [RAYS_ENTRY, VIEWS_ENTRY])
@pytest.mark.parametrize("half", [0, 1])
def test_every_refusal_of_the_visibility_entries(name, half):
    """each call carries one defect (or a pair that pins the order) and stand-in pointers that are never touched: the words and the
    order are those of pnr_baked_ray_backward_*, vis in the place of d_rays"""
    lib = _lib.load()
    camera = name == VIEWS_ENTRY
    sparse = dict(index=P, bits=P)
    src_bad, src_null, src_mis = (dict(NV=-1), dict(poses=None), dict(poses=P + 1)) if camera else (dict(R=-1), dict(rays=None), dict(rays=P + 1))
    none = dict(NV=0) if camera else dict(R=0)
    too_many = dict(W=2 ** 17, H=2 ** 17) if camera else dict(R=2 ** 34)
    what = "poses" if camera else "rays"
    aligned = "bits, d_rgb, d_depth, d_alpha and vis must be 4-byte aligned"
    expect = [
        (dict(degree=3), "degree must be -1 (RGBA), 0, 1 or 2"), (dict(degree=-2), "degree must be -1 (RGBA), 0, 1 or 2"),
        (dict(half=2), "storage_half must be 0 or 1"), (dict(half=-1), "storage_half must be 0 or 1"),
        (src_bad, "bad sizes (NV, W, H)" if camera else "bad sizes (R)"), (src_null, "null argument"),
        (src_mis, f"{what} must be 4-byte aligned"),
        (dict(M=-1, **sparse), "bad sizes (M)"),
        (dict(n=(1, 4, 4)), "every axis needs at least 2 grid points"),
        (dict(n=(2 ** 11, 2 ** 11, 2 ** 11)), "the grid must have fewer than 2^31 cells"),
        (dict(c1=GOOD["c2"], c2=GOOD["c1"]), "c1 / c2 must be finite with c1 < c2 on every axis"),
        (dict(step=0.0), "step must be finite and > 0"), (dict(step=float("nan")), "step must be finite and > 0"),
        (dict(term=1.0), "terminate must lie in [0, 1)"), (dict(term=float("nan")), "terminate must lie in [0, 1)"),
        (dict(vis=None), "null argument"), (dict(stored=None), "null argument"),
        (dict(index=P, bits=None), "null argument"),                      # sparse without bits
        (dict(stored=None, **sparse), "null argument"),
        (dict(stored=P + 8), "stored must be 16-byte aligned"), (dict(stored=P + 8, **sparse), "stored must be 16-byte aligned"),
        (dict(index=P + 2, bits=P), "index must be 4-byte aligned"),
        (dict(bits=P + 2), aligned), (dict(vis=P + 2), aligned),
        (too_many, "the number of rays exceeds the launch limit"),
        # two defects: the earlier check speaks
        (dict(degree=3, half=2), "degree must be -1 (RGBA), 0, 1 or 2"),
        (dict(half=2, **src_bad), "storage_half must be 0 or 1"),
        (dict(n=(1, 4, 4), **src_bad), "bad sizes (NV, W, H)" if camera else "bad sizes (R)"),
        (dict(M=-1, n=(1, 4, 4), **sparse), "bad sizes (M)"),
        (dict(step=0.0, term=1.0), "step must be finite and > 0"),
        (dict(term=1.0, vis=None), "terminate must lie in [0, 1)"),
        (dict(vis=None, stored=P + 8), "null argument"),
        (dict(stored=P + 8, vis=P + 2), "stored must be 16-byte aligned"),
        (dict(vis=P + 2, **too_many), aligned),
    ]
    for defect, words in expect:
        defect = dict(dict(half=half), **defect)
        assert _call(lib, name, **defect) == (-1, f"{name}: {words}"), (defect, _call(lib, name, **defect))
    # no rays: a no-op that looks at nothing else; a dense call does not look at M
    assert _call(lib, name, half=half, stored=None, vis=None, **src_null, **none) == (0, "")
    assert _call(lib, name, half=2, **none) == (-1, f"{name}: storage_half must be 0 or 1")
    assert _call(lib, name, half=half, term=1.0, **none) == (-1, f"{name}: terminate must lie in [0, 1)")
    assert _call(lib, name, half=half, M=-1, **too_many)[1].endswith("the number of rays exceeds the launch limit")
    assert _call(lib, name, half=half, M=0, stored=None, **sparse, **too_many)[1].endswith("the number of rays exceeds the launch limit")


# ---------------------------------------------------------------- 4. the Python layer
def test_python_layer_refuses_before_any_device_work():
    from pixelnerf_amd import ops
    from pixelnerf_amd.util import bake
    rays, vol = torch.zeros(3, 8), torch.zeros(4, 4, 4, 4)
    geo = ((4, 4, 4), (-1.0,) * 3, (1.0,) * 3, 0.1)
    with pytest.raises(ValueError, match=r"out must be a contiguous float32 tensor of shape \(4, 4, 4\)"):
        ops.baked_visibility(rays, vol, None, *geo, out=torch.zeros(4, 4, 5))
    with pytest.raises(ValueError, match=r"out must be a contiguous float32 tensor of shape \(4, 4, 4\)"):
        ops.baked_visibility(rays, vol.half(), None, *geo, out=torch.zeros(4, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"out must be a contiguous float32 tensor of shape \(5,\)"):
        ops.baked_visibility_views(torch.zeros(1, 4, 4), 4, 4, 10.0, None, 0.5, 3.0, torch.zeros(5, 4), None, *geo,
                                   index=torch.zeros(4, 4, 4, dtype=torch.int32), out=torch.zeros(4, 4, 4))
    with pytest.raises(ValueError, match=r"degree must be None / -1 \(RGBA\), 0, 1 or 2, got 3"):
        ops.baked_visibility(rays, vol, 3, *geo)
    with pytest.raises(ValueError, match="index and bits are mandatory"):
        ops.baked_visibility(rays, torch.zeros(5, 4), None, *geo, index=torch.zeros(4, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="terminate must lie in"):
        ops.baked_visibility(rays, vol, None, *geo, terminate=1.0)
    with pytest.raises(ValueError, match="the image must have at least one pixel"):
        ops.baked_visibility_views(torch.zeros(1, 4, 4), 0, 4, 10.0, None, 0.5, 3.0, vol, None, *geo)
    with pytest.raises(_lib.PixelNerfHipError, match="no CPU path"):
        ops.baked_visibility(rays, vol, None, *geo, out=torch.zeros(4, 4, 4))
    # the volume classes: a field of the wrong shape, for out and for prune, before anything looks at a device
    dense = object.__new__(bake.BakedVolume)
    dense.vol, dense.reso = vol, (4, 4, 4)
    sparse = object.__new__(bake.SparseBakedVolume)
    sparse.rows, sparse.reso = torch.zeros(5, 4), (4, 4, 4)
    with pytest.raises(ValueError, match=r"BakedVolume.visibility: out must be a contiguous float32 tensor of shape \(4, 4, 4\)"):
        dense.visibility(rays, out=torch.zeros(5))
    with pytest.raises(ValueError, match=r"SparseBakedVolume.visibility: out must be a contiguous float32 tensor of shape \(5,\)"):
        sparse.visibility(rays, out=torch.zeros(4, 4, 4))
    with pytest.raises(ValueError, match=r"BakedVolume.visibility_views: out must be"):
        dense.visibility_views(torch.zeros(1, 4, 4), 4, 4, 10.0, 0.5, 3.0, out=torch.zeros(4, 4, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="rays must be"):
        dense.visibility(torch.zeros(3, 7))
    with pytest.raises(ValueError, match=r"BakedVolume.prune: visibility must be a contiguous float32 tensor of shape \(4, 4, 4\)"):
        dense.prune(torch.zeros(5), 0.1)
    with pytest.raises(ValueError, match=r"SparseBakedVolume.prune: visibility must be a contiguous float32 tensor of shape \(5,\)"):
        sparse.prune(torch.zeros(4, 4, 4), 0.1)
    with pytest.raises(ValueError, match="visibility must be"):
        dense.prune(None, 0.1)
    for cls in (bake.BakedVolume, bake.BakedSHVolume, bake.SparseBakedVolume):
        assert callable(cls.visibility) and callable(cls.visibility_views)
    assert not hasattr(bake.BakedScene, "visibility")                                  # out of scope, by the header


def test_fit_coarse_to_fine_validates_before_any_device_work():
    from pixelnerf_amd.util import bake
    rays, rgb = torch.zeros(3, 8), torch.zeros(3, 3)
    dense = object.__new__(bake.BakedVolume)
    dense.vol, dense.reso = torch.zeros(4, 4, 4, 4), (4, 4, 4)
    sparse = object.__new__(bake.SparseBakedVolume)
    sparse.rows, sparse.reso = torch.zeros(5, 4), (4, 4, 4)
    with pytest.raises(TypeError, match="expected a baked volume"):
        bake.fit_coarse_to_fine(torch.zeros(4, 4, 4, 4), rays, rgb, [(None, 1)])
    for bad in ([], None, 5, [(4, 1, 2)], [4], [(None, -1)], [(None, 1.5)], [(None, True)], [(1, 1)], [((4, 4), 1)], [(4.5, 1)],
                [(None, 1), ("8", 1)]):
        with pytest.raises(ValueError, match="fit_coarse_to_fine: "):
            bake.fit_coarse_to_fine(dense, rays, rgb, bad)
    assert bake._check_stages("x", [(None, 0), (7, 3), ((5, 6, 7), 2)]) == [(None, 0), ((7, 7, 7), 3), ((5, 6, 7), 2)]
    for bad in (5, dict(dilate=1), dict(threshold=0.1, dilate=7), dict(threshold=0.1, keep=1), dict(threshold=float("nan"))):
        with pytest.raises(ValueError, match="fit_coarse_to_fine: prune"):
            bake.fit_coarse_to_fine(dense, rays, rgb, [(None, 1)], prune=bad)
    with pytest.raises(ValueError, match="the steps belong to the stages"):
        bake.fit_coarse_to_fine(dense, rays, rgb, [(None, 1)], steps=3)
    with pytest.raises(ValueError, match="rays must be"):
        bake.fit_coarse_to_fine(dense, torch.zeros(3, 7), rgb, [(None, 1)])
    # a sparse volume -- one from the start, or one that pruning makes -- refines by integer factors only: found on the host
    with pytest.raises(ValueError, match="stage 0: a sparse volume takes integer refinements only"):
        bake.fit_coarse_to_fine(sparse, rays, rgb, [(6, 1)])
    with pytest.raises(ValueError, match="stage 1: a sparse volume takes integer refinements only"):
        bake.fit_coarse_to_fine(dense, rays, rgb, [(5, 1), (8, 1)], prune=dict(threshold=0.1))
