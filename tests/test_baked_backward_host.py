"""CPU tests of the baked march's backward: the differentiable restatement of tests/baked_grad_ref.py against the numpy marches it
restates and against finite differences, the cases of tests/test_hip_baked_backward.py (their fp32 error, their distance to the
discontinuities of the march), the two new entries of the ABI and every refusal, word for word.  No call reaches a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_ref as B
import baked_sh_ref as S
import sparse_baked_ref as SP

from pixelnerf_amd import _lib

RAYS_ENTRY, VIEWS_ENTRY = "pnr_baked_backward_rays", "pnr_baked_backward_views"


# ---------------------------------------------------------------- 1. the restatement
def _close(got, want, tol=1e-12):
    for g, w in zip(got, want):
        assert np.abs(g.detach().numpy() - w).max() <= tol * max(1.0, np.abs(w).max())


@pytest.mark.parametrize("setting", list(B.SETTINGS))
def test_restatement_forward_is_the_rgba_march_in_fp64(setting):
    vol, rays = B.common_volume(), B.common_rays(setting)
    step = B.SETTINGS[setting][2]
    cells = SP.occupied_cells(vol[..., 3], 10.0)
    for kw in (dict(), dict(white_bkgd=True), dict(occupied=cells), dict(terminate=1e-2, white_bkgd=True),
               dict(occupied=cells, terminate=0.3)):
        got = G.march(rays, torch.from_numpy(vol).double(), B.C1, B.C2, step, **kw)
        _close(got, B.render_ref(rays, vol, B.C1, B.C2, step, **kw))


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_restatement_forward_is_the_sh_march_in_fp64(degree):
    coef, rays = S.common_coef(degree), B.common_rays("n133")
    step = B.SETTINGS["n133"][2]
    cells = SP.occupied_cells(coef[..., 0, 3], 10.0)
    for kw in (dict(), dict(white_bkgd=True, occupied=cells, terminate=1e-2)):
        got = G.march(rays, torch.from_numpy(coef).double(), B.C1, B.C2, step, degree=degree, **kw)
        _close(got, S.render_ref(rays, coef, B.C1, B.C2, step, degree, **kw))


@pytest.mark.parametrize("degree", [None, 1])
def test_restatement_passes_gradcheck(degree):
    """5 x 4 x 3 points, fp64, six rays through the box: torch.autograd.gradcheck of (rgb, depth, alpha) with respect to the stored
    values.  rgb and sigma are kept away from the clamp edges (the SH form), and sigma small enough that every sample counts."""
    rs = np.random.RandomState(5)
    reso, c1, c2 = (5, 4, 3), (-1.0, -0.8, -0.6), (1.1, 0.9, 0.7)
    shape = reso + ((4,) if degree is None else ((degree + 1) ** 2, 4))
    stored = rs.uniform(0.2, 0.8, shape).astype(np.float32)
    if degree is not None:
        stored[..., 1:, :] = rs.uniform(-0.05, 0.05, shape[:3] + (shape[3] - 1, 4))
    stored[..., 3] *= 3.0
    rows = []
    for k in range(6):
        cam = np.array([(3.0, 0.3, 0.2), (-0.5, 2.8, 1.0), (0.4, -1.0, 2.9)][k % 3])
        target = np.array(c1) + (0.25 + 0.5 * rs.uniform(size=3)) * (np.array(c2) - np.array(c1))
        d = (target - cam) / np.linalg.norm(target - cam)
        rows.append(np.concatenate((cam, d, [1.5, 1.5 + 19.5 * 0.15])))
    rays = np.asarray(rows, np.float32)
    leaf = torch.from_numpy(stored).double().requires_grad_(True)
    for white in (False, True):
        fn = lambda s: G.march(rays, s, c1, c2, 0.15, degree=degree, white_bkgd=white)
        assert torch.autograd.gradcheck(fn, (leaf,), eps=1e-6, atol=1e-7, rtol=1e-5)


# ---------------------------------------------------------------- 2. the cases the GPU test uses
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_no_case_brings_the_bar_to_its_cap(name):
    """torch's fp32 autograd through the restatement is within a tenth of the cap of the fp64 gradient on every case, so the bar a
    kernel is held to is 10 x a measured fp32 error and never the cap; and no sample of a case lies within 1e-5 box edges of a face
    of the box, where fp32 and fp64 could disagree on whether it exists (its gradient, unlike its value, would not be continuous
    there): an fp32 point o + t d with |o|, |t d| < 8 is off by less than 3 x 2^-24 x 8 = 1.5e-6, a tenth of that margin on the
    shortest edge (1.3)"""
    case = G.BY_NAME[name]
    inp, ref64, ref32 = G.reference(case)
    err32 = G.error(ref32, ref64)
    print(f"{name}: torch-fp32 error {err32:.3e}, bar {G.bar_from(err32):.3e}, max |ref| {float(ref64.abs().max()):.3e}")
    assert float(ref64.abs().max()) > 0 and bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(ref32).all())
    assert 10.0 * err32 < G.BAR_CAP, (name, err32)
    info = {}
    G.march(inp["rays"], torch.from_numpy(inp["stored"]).double(), G.C1, G.C2, inp["step"], info=info, **inp["kw"])
    assert info["face_margin"] > 1e-5, (name, info["face_margin"])
    n, _ = G.SETTINGS[case.setting]
    assert set(info["n"]) <= {0, n} and n in info["n"]   # (0: the ray with near >= far)


def test_contention_case_keeps_its_bar_below_the_cap():
    """2048 copies of one ray: their fp64 gradient is 2048 x the single ray's, and torch's fp32 autograd, which adds the copies one
    after the other, is still within a tenth of the cap"""
    many, single64, ref64, ref32 = G.contention()
    err32 = G.error(ref32, ref64)
    print(f"2048 copies: torch-fp32 error {err32:.3e}, bar {G.bar_from(err32):.3e}")
    assert many["rays"].shape[0] == 2048 and G.error(ref64, 2048.0 * single64) < 1e-12
    assert 10.0 * err32 < G.BAR_CAP


@pytest.mark.parametrize("name", [c.name for c in G.CASES if c.terminate > 0])
def test_termination_is_decided_the_same_in_fp32_and_fp64(name):
    """at every chunk boundary the march walks, the transmittance is a factor of at least 2 away from eps on either side: an fp32
    march (relative error of a product of < 200 factors: 1e-5) stops after the same chunk as the fp64 reference.  Some ray of the
    case does stop early, and some ray does not."""
    case = G.BY_NAME[name]
    inp = G.inputs(case)
    info = {}
    G.march(inp["rays"], torch.from_numpy(inp["stored"]).double(), G.C1, G.C2, inp["step"], info=info, **inp["kw"])
    eps, stopped, ran = case.terminate, 0, 0
    nchunks = G.SETTINGS[case.setting][0] // 64
    for bounds in info["boundaries"]:
        for T in bounds:
            assert T <= eps / 2 or T >= 2 * eps, (name, T)
        if bounds and bounds[-1] <= eps and len(bounds) < nchunks:
            stopped += 1
        elif len(bounds) == nchunks:
            ran += 1
    assert stopped > 0 and ran > 0, (name, stopped, ran)


def test_opaque_case_holds_a_sample_of_alpha_one():
    """the opaque case: some sample has alpha = 1 exactly in fp32, in the middle of its ray -- samples with sigma gradients on both
    sides of it"""
    inp = G.inputs(G.BY_NAME["rgba_n150_opaque"])
    vol = torch.from_numpy(inp["stored"])
    info = {}
    _, _, _ = G.march(inp["rays"], vol.double(), G.C1, G.C2, inp["step"], info=info)
    assert float(np.float32(1.0) - np.exp(np.float32(-(np.float32(0.03) * np.float32(1e4 * 0.06))))) == 1.0
    _, ref64, _ = G.reference(G.BY_NAME["rgba_n150_opaque"])
    assert float(ref64[4:6, 3:5, 3:5].abs().max()) > 0   # the block itself is reached


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_sh_cases_clamp_on_both_sides_and_keep_off_the_edges(degree):
    coef = np.array(G.sh_coef(degree))
    gap, below, above = G.sh_clamp_census(coef, G.case_rays("n150"), degree)
    assert gap >= G.SH_MARGIN, gap
    assert all(b > 0 for b in below) and all(a > 0 for a in above), (below, above)


# ---------------------------------------------------------------- 3. the ABI
def test_backward_entries_are_declared_exported_and_bound(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    assert lib.pnr_abi_version() == 12
    for name, n_args in ((RAYS_ENTRY, 20), (VIEWS_ENTRY, 28)):
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(lib, name)
    # the tail of the sparse march entries up to `terminate`, then the three upstream gradients, d_stored and the stream
    assert _lib.PROTOTYPES[RAYS_ENTRY][1][:15] == _lib.PROTOTYPES["pnr_baked_sparse_render_rays"][1][:15]
    assert _lib.PROTOTYPES[VIEWS_ENTRY][1][:23] == _lib.PROTOTYPES["pnr_baked_sparse_render_views"][1][:23]


P = 64  # a non-null, 16-byte aligned stand-in for a device pointer
GOOD = dict(rays=P, R=4, poses=P, NV=1, W=4, H=4, stored=P, M=10, degree=2, index=None, bits=None, n=(4, 4, 4), c1=(-1.0, -1.0, -1.0),
            c2=(1.0, 1.0, 1.0), step=0.1, term=0.0, d_rgb=P, d_depth=P, d_alpha=P, d_stored=P)


def _call(lib, name, **defect):
    a = dict(GOOD)
    a.update(defect)
    f3 = ctypes.c_float * 3
    args = [a["poses"], a["NV"], a["W"], a["H"], 10.0, 10.0, 2.0, 2.0, 0.5, 3.0] if name == VIEWS_ENTRY else [a["rays"], a["R"]]
    args += [a["stored"], a["M"], a["degree"], a["index"], a["bits"], *a["n"], f3(*a["c1"]), f3(*a["c2"]), a["step"], 0, a["term"],
             a["d_rgb"], a["d_depth"], a["d_alpha"], a["d_stored"], None]
    rc = getattr(lib, name)(*args)
    return rc, (lib.pnr_last_error().decode() if rc != 0 else "")


@pytest.mark.parametrize("name", [RAYS_ENTRY, VIEWS_ENTRY])
def test_every_refusal_of_the_backward_entries(name):
    """each call carries one defect (or a pair that pins the order) and stand-in pointers that are never touched: the words and the
    order are those of the march entries (tests/golden/baked_refusals.json)"""
    lib = _lib.load()
    camera = name == VIEWS_ENTRY
    sparse = dict(index=P, bits=P)
    src_bad, src_null, src_mis = (dict(NV=-1), dict(poses=None), dict(poses=P + 1)) if camera else (dict(R=-1), dict(rays=None), dict(rays=P + 1))
    none = dict(NV=0) if camera else dict(R=0)
    too_many = dict(W=2 ** 17, H=2 ** 17) if camera else dict(R=2 ** 34)
    what = "poses" if camera else "rays"
    expect = [
        (dict(degree=3), "degree must be -1 (RGBA), 0, 1 or 2"), (dict(degree=-2), "degree must be -1 (RGBA), 0, 1 or 2"),
        (src_bad, "bad sizes (NV, W, H)" if camera else "bad sizes (R)"), (src_null, "null argument"),
        (src_mis, f"{what} must be 4-byte aligned"),
        (dict(M=-1, **sparse), "bad sizes (M)"),
        (dict(n=(1, 4, 4)), "every axis needs at least 2 grid points"),
        (dict(n=(2 ** 11, 2 ** 11, 2 ** 11)), "the grid must have fewer than 2^31 cells"),
        (dict(c1=GOOD["c2"], c2=GOOD["c1"]), "c1 / c2 must be finite with c1 < c2 on every axis"),
        (dict(step=0.0), "step must be finite and > 0"), (dict(step=float("nan")), "step must be finite and > 0"),
        (dict(term=1.0), "terminate must lie in [0, 1)"), (dict(term=float("nan")), "terminate must lie in [0, 1)"),
        (dict(d_stored=None), "null argument"), (dict(stored=None), "null argument"),
        (dict(index=P, bits=None), "null argument"),                      # sparse without bits
        (dict(stored=None, **sparse), "null argument"),
        (dict(stored=P + 8), "stored must be 16-byte aligned"), (dict(stored=P + 8, **sparse), "stored must be 16-byte aligned"),
        (dict(index=P + 2, bits=P), "index must be 4-byte aligned"),
        (dict(bits=P + 2), "bits, d_rgb, d_depth, d_alpha and d_stored must be 4-byte aligned"),
        (dict(d_rgb=P + 2), "bits, d_rgb, d_depth, d_alpha and d_stored must be 4-byte aligned"),
        (dict(d_depth=P + 1), "bits, d_rgb, d_depth, d_alpha and d_stored must be 4-byte aligned"),
        (dict(d_alpha=P + 3), "bits, d_rgb, d_depth, d_alpha and d_stored must be 4-byte aligned"),
        (dict(d_stored=P + 2), "bits, d_rgb, d_depth, d_alpha and d_stored must be 4-byte aligned"),
        (too_many, "the number of rays exceeds the launch limit"),
        # two defects: the earlier check speaks
        (dict(degree=3, **src_bad), "degree must be -1 (RGBA), 0, 1 or 2"),
        (dict(n=(1, 4, 4), **src_bad), "bad sizes (NV, W, H)" if camera else "bad sizes (R)"),
        (dict(M=-1, n=(1, 4, 4), **sparse), "bad sizes (M)"),
        (dict(step=0.0, term=1.0), "step must be finite and > 0"),
        (dict(term=1.0, d_stored=None), "terminate must lie in [0, 1)"),
        (dict(d_stored=None, stored=P + 8), "null argument"),
        (dict(stored=P + 8, d_rgb=P + 2), "stored must be 16-byte aligned"),
        (dict(d_rgb=P + 2, **too_many), "bits, d_rgb, d_depth, d_alpha and d_stored must be 4-byte aligned"),
    ]
    for defect, words in expect:
        assert _call(lib, name, **defect) == (-1, f"{name}: {words}"), (defect, _call(lib, name, **defect))
    # no rays: a no-op that looks at nothing else; a dense call does not look at M; the upstream gradients are optional
    assert _call(lib, name, stored=None, d_stored=None, d_rgb=None, **src_null, **none) == (0, "")
    assert _call(lib, name, degree=3, **none) == (-1, f"{name}: degree must be -1 (RGBA), 0, 1 or 2")
    assert _call(lib, name, term=1.0, **none) == (-1, f"{name}: terminate must lie in [0, 1)")
    assert _call(lib, name, M=-1, **too_many)[1].endswith("the number of rays exceeds the launch limit")   # dense: M is not looked at
    assert _call(lib, name, d_rgb=None, d_depth=None, d_alpha=None, **too_many)[1].endswith("the number of rays exceeds the launch limit")
    assert _call(lib, name, M=0, stored=None, **sparse, **too_many)[1].endswith("the number of rays exceeds the launch limit")


def test_python_layer_refuses_before_any_device_work():
    """an fp16 volume (with the way out in the words), rays or poses that require grad, a bad degree, a volume of the wrong shape, a
    CPU volume: all raised from CPU tensors, before anything touches a device"""
    from pixelnerf_amd import autograd, ops
    from pixelnerf_amd.util import bake
    rays, vol = torch.zeros(3, 8), torch.zeros(4, 4, 4, 4)
    geo = ((4, 4, 4), (-1.0,) * 3, (1.0,) * 3, 0.1)
    with pytest.raises(TypeError, match=r"fp32 volumes only; fit the volume in fp32 and call half\(\) afterwards"):
        ops.baked_render_backward(rays, vol.half(), None, *geo)
    with pytest.raises(TypeError, match=r"fp32 volumes only; fit the volume in fp32 and call half\(\) afterwards"):
        ops.baked_render_views_backward(torch.zeros(1, 4, 4), 4, 4, 10.0, None, 0.5, 3.0, vol.half(), None, *geo)
    with pytest.raises(TypeError, match=r"fp32 volumes only; fit the volume in fp32 and call half\(\) afterwards"):
        autograd.baked_march_autograd(vol.half(), (rays,), None, *geo)
    with pytest.raises(ValueError, match="no gradient is given with respect to rays"):
        ops.baked_render_backward(rays.clone().requires_grad_(True), vol, None, *geo)
    with pytest.raises(ValueError, match="no gradient is given with respect to poses"):
        ops.baked_render_views_backward(torch.zeros(1, 4, 4, requires_grad=True), 4, 4, 10.0, None, 0.5, 3.0, vol, None, *geo)
    with pytest.raises(ValueError, match="no gradient is given with respect to rays"):
        autograd.baked_march_autograd(vol, (rays.clone().requires_grad_(True),), None, *geo)
    with pytest.raises(ValueError, match=r"degree must be None / -1 \(RGBA\), 0, 1 or 2, got 3"):
        ops.baked_render_backward(rays, vol, 3, *geo)
    with pytest.raises(ValueError, match=r"stored must be \(nx,ny,nz,4,4\) at degree 1"):
        ops.baked_render_backward(rays, vol, 1, *geo)
    with pytest.raises(ValueError, match="index and bits are mandatory"):
        ops.baked_render_backward(rays, torch.zeros(5, 4), None, *geo, index=torch.zeros(4, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="step must be finite and > 0"):
        ops.baked_render_backward(rays, vol, None, geo[0], geo[1], geo[2], 0.0)
    with pytest.raises(_lib.PixelNerfHipError, match="no CPU path"):
        ops.baked_render_backward(rays, vol, None, *geo)
    assert hasattr(bake.BakedVolume, "trainable") and hasattr(bake.BakedSHVolume, "trainable") and hasattr(bake.SparseBakedVolume, "trainable")
    assert callable(bake.fit) and issubclass(bake.TrainableBaked, torch.nn.Module)
