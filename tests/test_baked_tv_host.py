"""CPU tests of the total-variation prior: the restatement of tests/baked_tv_ref.py against finite differences and against the closed
forms a ramp and a constant block have, its sparse form against its dense form, the new entry of the ABI and every refusal, word
for word, and the host loop that tells tests/test_hip_baked_tv.py what the prior has to achieve.  No call reaches a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_tv_ref as T

from pixelnerf_amd import _lib

ENTRY = "pnr_baked_tv"


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("name", ["rgba_253_ones", "sh2_253_distinct", "rgba_253_all"])
def test_gradient_matches_central_differences(name):
    """every element of the (2,5,3) cases, dense and masked, h = 1e-6 in fp64: the truncation h^2 f'''/6 with f''' ~ 1/n^2 = O(10) is
    1e-11 and the rounding 1e-16 / h is 1e-10 per unit of value, against gradients of 1e-2: 1e-7 of the largest holds both"""
    case = T.BY_NAME[name]
    inp, value, g64 = T.reference(case)[:3]
    kept = inp["kept"]
    base = torch.tensor(np.array(inp["stored"], np.float32)).double()
    h, fd = 1e-6, torch.zeros_like(base)
    flat, out = base.reshape(-1), fd.reshape(-1)
    with torch.no_grad():
        for e in range(flat.numel()):
            keep = float(flat[e])
            flat[e] = keep + h
            up = float(T.tv(base, inp["weights"], T.EPS, kept))
            flat[e] = keep - h
            down = float(T.tv(base, inp["weights"], T.EPS, kept))
            flat[e] = keep
            out[e] = (up - down) / (2 * h)
    _, full = T.value_and_gradient(inp["stored"], inp["weights"], T.EPS, kept)
    err = T.error(fd, full)
    print(f"{name}: finite differences against autograd {err:.3e}")
    assert float(full.abs().max()) > 0 and err <= 1e-7
    if kept is not None:   # the rows' gradient is the masked gradient at ids; a dropped point (there is none here) would get 0
        assert torch.equal(g64, full.reshape((-1,) + tuple(full.shape[3:]))[torch.from_numpy(inp["ids"].astype(np.int64))])


def test_ramp_has_its_closed_form():
    """S = s i: d_x = s at the (nx-1) ny nz points that have an x neighbour, 0 at the ny nz others, d_y = d_z = 0:
    value = sum_c w_c ((nx-1) ny nz sqrt(s^2 + eps) + ny nz sqrt(eps)) / N"""
    case = T.BY_NAME["rgba_654_ramp"]
    inp, value = T.reference(case)[:2]
    nx, ny, nz = case.reso
    eps, s = float(np.float32(T.EPS)), T.RAMP_SLOPE
    want = sum(inp["weights"]) * ((nx - 1) * ny * nz * np.sqrt(s * s + eps) + ny * nz * np.sqrt(eps)) / (nx * ny * nz)
    assert abs(float(value) - want) <= 1e-13 * want
    assert np.array_equal(inp["stored"][2, 1, 3], np.full(4, 2 * s, np.float32))


@pytest.mark.parametrize("name", ["rgba_987_block", "sh1_987_block"])
def test_centre_of_a_constant_block_has_gradient_exactly_zero(name):
    case = T.BY_NAME[name]
    inp, _, g64, _, g32 = T.reference(case)
    assert np.all(inp["stored"][T.BLOCK] == inp["stored"][T.BLOCK_CENTRE])
    for g in (g64, g32):
        assert not bool(g[T.BLOCK_CENTRE].any()) and bool(g[T.BLOCK_CENTRE[0] + 2, T.BLOCK_CENTRE[1], T.BLOCK_CENTRE[2]].any())


@pytest.mark.parametrize("name", sorted(T.DENSE_OF))
def test_sparse_form_with_every_cell_on_is_the_dense_form(name):
    sparse, dense = T.reference(T.BY_NAME[name]), T.reference(T.BY_NAME[T.DENSE_OF[name]])
    assert bool(sparse[0]["kept"].all()) and np.array_equal(sparse[0]["stored"], dense[0]["stored"])
    assert sparse[0]["ids"].tolist() == list(range(sparse[0]["kept"].size))
    for k in (1, 3):
        assert float(sparse[k]) == float(dense[k])
    for k in (2, 4):
        assert torch.equal(sparse[k], dense[k].reshape(sparse[k].shape))


def test_cases_cover_what_they_claim():
    third = T.inputs(T.BY_NAME["rgba_987_third"])
    assert 0.2 < third["cells"].mean() < 0.45 and 0 < int(third["kept"].sum()) < third["kept"].size
    for case in T.CASES:
        inp, v64, g64, v32, g32 = T.reference(case)
        assert float(v64) > 0 and T.error(g32.double(), g64) < 2e-6 and abs(float(v32) - float(v64)) < 2e-6 * float(v64), case.name
        w = torch.tensor(inp["weights"]).reshape(g64.shape[-2:] if case.degree is not None else (4,))
        assert not bool(g64[..., w == 0].any()), case.name   # an element whose weight is 0 has gradient exactly 0


# ---------------------------------------------------------------- 2. the entry and its refusals
def test_entry_is_declared_bound_and_exported_within_abi_12():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pixelnerf_hip.h")).read()
    assert "#define PNR_ABI_VERSION 12" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert lib.pnr_abi_version() == 12
    decl = re.search(ENTRY + r"\s*\(([^;]*)\)\s*;", code)
    assert decl and len(decl.group(1).split(",")) == 16 == len(_lib.PROTOTYPES[ENTRY][1])
    assert hasattr(lib, ENTRY) and lib.pnr_baked_tv_workspace_bytes() == 16384   # fixed: no workspace grows with the volume


P = 64  # a non-null, 16-byte aligned stand-in for a device pointer
GOOD = dict(stored=P, M=10, degree=2, index=None, ids=None, n=(4, 4, 4), w=[1.0] * 36, eps=1e-8, scale=None, value32=P, value64=P, grad=P,
            workspace=P)


def _call(lib, **defect):
    a = dict(GOOD)
    a.update(defect)
    w = None if a["w"] is None else (ctypes.c_float * len(a["w"]))(*a["w"])
    rc = lib.pnr_baked_tv(a["stored"], a["M"], a["degree"], a["index"], a["ids"], *a["n"], w, a["eps"], a["scale"], a["value32"], a["value64"],
                          a["grad"], a["workspace"], None)
    return rc, (lib.pnr_last_error().decode() if rc != 0 else "")


def test_every_refusal_of_the_entry():
    """each call carries one defect (or a pair that pins the order) and stand-in pointers that are never touched"""
    lib = _lib.load()
    sparse = dict(index=P, ids=P)
    bad_w = lambda v: [1.0] * 35 + [v]
    aligned = "index, ids, scale and value32 must be 4-byte aligned, value64 and workspace 8-byte aligned"
    expect = [
        (dict(degree=3), "degree must be -1 (RGBA), 0, 1 or 2"), (dict(degree=-2), "degree must be -1 (RGBA), 0, 1 or 2"),
        (dict(index=P), "index and ids go together (both, or neither for a dense volume)"),
        (dict(ids=P), "index and ids go together (both, or neither for a dense volume)"),
        (dict(M=-1, **sparse), "bad sizes (M)"),
        (dict(n=(1, 4, 4)), "every axis needs at least 2 grid points"),
        (dict(n=(2 ** 11, 2 ** 11, 2 ** 11)), "the grid must have fewer than 2^31 cells"),
        (dict(n=(2, 2, 2 ** 30), **sparse), "the grid must have fewer than 2^31 points (ranks are int32)"),
        (dict(eps=0.0), "eps must be finite and > 0"), (dict(eps=-1e-8), "eps must be finite and > 0"),
        (dict(eps=float("nan")), "eps must be finite and > 0"), (dict(eps=float("inf")), "eps must be finite and > 0"),
        (dict(w=None), "null argument (w)"),
        (dict(w=bad_w(-1.0)), "every weight must be finite and >= 0"), (dict(w=bad_w(float("nan"))), "every weight must be finite and >= 0"),
        (dict(w=bad_w(float("inf"))), "every weight must be finite and >= 0"),
        (dict(workspace=None), "a value needs the workspace of pnr_baked_tv_workspace_bytes()"),
        (dict(workspace=None, value32=None), "a value needs the workspace of pnr_baked_tv_workspace_bytes()"),
        (dict(stored=None), "null argument"), (dict(stored=None, **sparse), "null argument"),
        (dict(stored=P + 8), "stored and grad must be 16-byte aligned"), (dict(grad=P + 4), "stored and grad must be 16-byte aligned"),
        (dict(index=P + 2, ids=P), aligned), (dict(index=P, ids=P + 1), aligned), (dict(scale=P + 2), aligned), (dict(value32=P + 2), aligned),
        (dict(value64=P + 4), aligned), (dict(workspace=P + 4), aligned),
        # two defects: the earlier check speaks
        (dict(degree=3, index=P), "degree must be -1 (RGBA), 0, 1 or 2"),
        (dict(index=P, M=-1), "index and ids go together (both, or neither for a dense volume)"),
        (dict(M=-1, n=(1, 4, 4), **sparse), "bad sizes (M)"),
        (dict(n=(1, 4, 4), eps=0.0), "every axis needs at least 2 grid points"),
        (dict(eps=0.0, w=bad_w(-1.0)), "eps must be finite and > 0"),
        (dict(w=bad_w(-1.0), workspace=None), "every weight must be finite and >= 0"),
        (dict(workspace=None, stored=None), "a value needs the workspace of pnr_baked_tv_workspace_bytes()"),
        (dict(stored=None, grad=P + 4), "null argument"),
        (dict(stored=P + 8, value64=P + 4), "stored and grad must be 16-byte aligned"),
    ]
    for defect, words in expect:
        assert _call(lib, **defect) == (-1, f"{ENTRY}: {words}"), (defect, _call(lib, **defect))
    # nothing asked for: a no-op that looks at no pointer; a weight beyond the row's E elements is not looked at; a dense call does
    # not look at M; the gradient alone needs no workspace (it is refused for its pointer's alignment: the last check, so all passed)
    assert _call(lib, value32=None, value64=None, grad=None, stored=None, workspace=None) == (0, "")
    assert _call(lib, degree=-1, w=[1.0] * 4 + [-1.0], value32=None, value64=None, grad=None) == (0, "")
    assert _call(lib, M=-1, value32=None, value64=None, grad=None) == (0, "")
    assert _call(lib, value32=None, value64=None, workspace=None, scale=P + 2) == (-1, f"{ENTRY}: {aligned}")


def test_python_layer_refuses_before_any_device_work():
    from pixelnerf_amd import autograd, ops
    from pixelnerf_amd.util import bake
    vol, reso = torch.zeros(4, 4, 4, 4), (4, 4, 4)
    with pytest.raises(TypeError, match=r"fp32 volumes only; fit the volume in fp32 and call half\(\) afterwards"):
        ops.baked_tv(vol.half(), None, reso, [1.0] * 4)
    with pytest.raises(TypeError, match=r"fp32 volumes only; fit the volume in fp32 and call half\(\) afterwards"):
        autograd.baked_tv_autograd(vol.half(), None, reso, [1.0] * 4)
    with pytest.raises(ValueError, match="stored must be contiguous"):
        ops.baked_tv(vol.permute(1, 0, 2, 3), None, reso, [1.0] * 4)
    with pytest.raises(ValueError, match=r"degree must be None / -1 \(RGBA\), 0, 1 or 2, got 3"):
        ops.baked_tv(vol, 3, reso, [1.0] * 4)
    with pytest.raises(ValueError, match=r"stored must be \(4,4,4,4,4\) at degree 1"):
        ops.baked_tv(vol, 1, reso, [1.0] * 16)
    with pytest.raises(ValueError, match="index and ids go together"):
        ops.baked_tv(torch.zeros(5, 4), None, reso, [1.0] * 4, index=torch.zeros(4, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="weights must be 4 finite numbers >= 0"):
        ops.baked_tv(vol, None, reso, [1.0, 1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match="weights must be 4 finite numbers >= 0"):
        ops.baked_tv(vol, None, reso, [1.0] * 5)
    with pytest.raises(ValueError, match="eps must be finite and > 0"):
        ops.baked_tv(vol, None, reso, [1.0] * 4, eps=0.0)
    with pytest.raises(_lib.PixelNerfHipError, match="no CPU path"):
        ops.baked_tv(vol, None, reso, [1.0] * 4)
    with pytest.raises(ValueError, match="rgb, sigma and sh must be finite and >= 0"):
        bake._tv_weights("x", 1, 1.0, -1.0, None)
    assert bake._tv_weights("x", None, 2.0, 3.0, 5.0) == [2.0, 2.0, 2.0, 3.0]
    assert bake._tv_weights("x", 1, 2.0, 3.0, None) == [2.0, 2.0, 2.0, 3.0] * 4
    assert bake._tv_weights("x", 1, 2.0, 3.0, 5.0) == [2.0, 2.0, 2.0, 3.0] + [5.0] * 12
    assert bake._tv_weights("x", 2, 1.0, 0.0, None) == T.weights("rgb", 2) and T.fit_weights(1, 2.0, 3.0, 5.0) == bake._tv_weights("x", 1, 2.0, 3.0, 5.0)
    for cls in (bake.BakedVolume, bake.BakedSHVolume, bake.SparseBakedVolume, bake.TrainableBaked):
        assert callable(cls.tv)
    import inspect
    sig = inspect.signature(bake.fit).parameters
    assert [sig[k].default for k in ("tv_rgb", "tv_sigma", "tv_sh", "tv_eps")] == [0.0, 0.0, None, 1e-8]


# ---------------------------------------------------------------- 3. what the prior achieves in the host loop
def test_prior_halves_the_total_variation_in_the_host_loop():
    """baked_grad_ref.fit_scene (12^3, RGBA), the host fp32 loop with and without the prior of baked_tv_ref.FIT_TV (rgb weight 0.1, eps
    1e-2; the reasons stand there): r_host = TV(fitted with) / TV(fitted without) <= 0.5, so the condition of the GPU test,
    ratio <= (1 + r_host) / 2, is one the reference meets with room.  Measured: r_host 0.4193, final mse 3.5395e-04 with the prior
    (fp64 loop: 3.53951522e-04, fp32: 3.53951502e-04) against 3.0778e-05 without."""
    without, plain = T.fit_ref(None, torch.float32, **G.FIT)
    assert without == G.fit_ref(None, torch.float32, **G.FIT)          # all weights 0: the loop of baked_grad_ref
    losses, fitted = T.fit_ref(None, torch.float32, **G.FIT, **T.FIT_TV)
    r_host = T.tv_of(fitted, None, **T.FIT_TV) / T.tv_of(plain, None, **T.FIT_TV)
    print(f"r_host {r_host:.4f}; final mse with the prior {losses[-1]:.6e}, without {without[-1]:.6e}")
    assert r_host <= 0.5
    assert losses[-1] < losses[0]
