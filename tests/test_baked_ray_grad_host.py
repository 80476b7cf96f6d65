"""Host tests of the yardstick tests/test_hip_baked_ray_grad.py uses (tests/baked_ray_grad_ref.py) and of what the ray-gradient
entries (pnr_baked_ray_backward_rays / _views) decide without a device: the restatement's forward is baked_grad_ref.march, its
fp64 d_rays agrees with central differences, the kept-rows rule drops what it should and no more, fp32 and fp64 name the same
cells on the kept rays, the entries are declared, exported and bound, every refusal comes back before any HIP call, and the
Rodrigues form of util.bake.register is finite at w = 0.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_ray_grad_ref as RG

from pixelnerf_amd import _lib

RAYS_ENTRY, VIEWS_ENTRY = "pnr_baked_ray_backward_rays", "pnr_baked_ray_backward_views"


@pytest.fixture(scope="module")
def repo_root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(case, inp):
    return list(range(inp["rays"].shape[0])) if case.rows is None else list(case.rows)


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_restatement_forward_is_the_march_of_baked_grad_ref(name):
    case = G.BY_NAME[name]
    inp = G.inputs(case)
    want = G.march(inp["rays"], torch.from_numpy(inp["stored"]).double(), G.C1, G.C2, inp["step"], **inp["kw"])
    got = RG.march(torch.from_numpy(inp["rays"]).double(), torch.from_numpy(inp["stored"]).double(), G.C1, G.C2, inp["step"], **inp["kw"])
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", G.CASE_IDS)
def test_fp64_ray_gradient_agrees_with_central_differences(name):
    """fp64, eps = 1e-7 on one column of every ray at a time, the loss of each ray on its own (rays do not interact): relative to
    the largest entry of the gradient the two agree to 1e-6 on the kept rows (measured 2e-10 .. 4.2e-9), and the difference along
    `far` is EXACTLY zero -- far only sets the sample count"""
    case = G.BY_NAME[name]
    inp, kept, ref64, _ = RG.reference(case)
    rays = torch.from_numpy(inp["rays"]).double()
    stored = torch.from_numpy(inp["stored"]).double()
    ups = (inp["d_rgb"], inp["d_depth"], inp["d_alpha"])
    loss = lambda r: RG.loss_per_ray(RG.march(r, stored, G.C1, G.C2, inp["step"], **inp["kw"]), *ups, torch.float64)
    eps = 1e-7
    fd = torch.zeros_like(ref64)
    with torch.no_grad():
        for col in range(8):
            hi, lo = rays.clone(), rays.clone()
            hi[:, col] += eps
            lo[:, col] -= eps
            fd[:, col] = (loss(hi) - loss(lo)) / (2 * eps)
    assert not bool(fd[:, 7].any()) and not bool(ref64[:, 7].any())
    err = RG.error(fd[kept], ref64[kept])
    print(f"{name}: central differences against autograd {err:.3e}")
    assert float(ref64[kept].abs().max()) > 0 and err <= 1e-6


# ---------------------------------------------------------------- 2. the kept rows
EXPECT_DROPPED = {"n40": {32, 34, 35}, "n64": {32, 35}, "n150": {35}, "n4500": set()}


@pytest.mark.parametrize("name", G.CASE_IDS)
def test_kept_rows_census_cap_and_cells(name):
    """the rule drops the in-plane ray and, at the coarse steps, the axis-parallel rays whose samples land on planes; never more than
    3 of 37; at least 27 kept rays of a full case have a gradient; and on the kept rays fp32 and fp64 agree on n, the cell and
    `active` of EVERY sample, so the two differentiate the same piece of the march"""
    case = G.BY_NAME[name]
    inp, kept, ref64, ref32 = RG.reference(case)
    rows = _rows(case, inp)
    dropped = {rows[i] for i in np.nonzero(~kept.numpy())[0]}
    assert dropped == EXPECT_DROPPED[case.setting] & set(rows), dropped
    assert len(dropped) <= RG.MAX_DROPPED
    nonzero = int((ref64[kept].abs().sum(dim=1) > 0).sum())
    print(f"{name}: dropped {sorted(dropped)}, kept rays with a gradient {nonzero}")
    if case.rows is None:
        assert nonzero >= RG.MIN_NONZERO
    else:
        assert nonzero >= min(RG.MIN_NONZERO, len(rows))
    infos = {}
    for dtype in (torch.float64, torch.float32):
        infos[dtype] = {}
        RG.march(torch.from_numpy(inp["rays"]).to(dtype), torch.from_numpy(inp["stored"]).to(dtype), G.C1, G.C2, inp["step"],
                 info=infos[dtype], **inp["kw"])
    a, b = infos[torch.float64], infos[torch.float32]
    assert torch.equal(a["n"], b["n"])
    assert torch.equal(a["active"][kept], b["active"][kept])
    live = a["active"][kept]
    assert torch.equal(a["idx"][kept][live], b["idx"][kept][live])
    # the error the bar is made from (1.6e-7 .. 7.7e-7; the long case 7e-7 .. 4e-6 by host, the opaque one 1.2e-5): no bar at its cap
    err32 = RG.error(ref32[kept].double(), ref64[kept])
    print(f"{name}: torch fp32 against fp64 on the kept rows {err32:.3e}")
    assert RG.bar_from(err32) < RG.BAR_CAP, err32


def test_the_in_plane_ray_is_why_the_rule_exists():
    """row 35 of case_rays lies in a cell plane: torch fp32 and fp64 differentiate different cells there and differ by percents"""
    inp, kept, ref64, ref32 = RG.reference(G.BY_NAME["rgba_n150"])
    assert not bool(kept[35])
    assert RG.error(ref32[35:36].double(), ref64[35:36]) > 1e-2


# ---------------------------------------------------------------- 3. the ABI
def test_ray_backward_entries_are_declared_exported_and_bound(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    assert lib.pnr_abi_version() == 12
    for name, n_args in ((RAYS_ENTRY, 21), (VIEWS_ENTRY, 29)):
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(lib, name)
    # pnr_baked_backward_*'s list with storage_half after `stored`
    for new, old, at in ((RAYS_ENTRY, "pnr_baked_backward_rays", 3), (VIEWS_ENTRY, "pnr_baked_backward_views", 11)):
        args = list(_lib.PROTOTYPES[new][1])
        assert args.pop(at) is ctypes.c_int and args == list(_lib.PROTOTYPES[old][1])


P = 64  # a non-null, 16-byte aligned stand-in for a device pointer
GOOD = dict(rays=P, R=4, poses=P, NV=1, W=4, H=4, stored=P, half=0, M=10, degree=2, index=None, bits=None, n=(4, 4, 4),
            c1=(-1.0, -1.0, -1.0), c2=(1.0, 1.0, 1.0), step=0.1, term=0.0, d_rgb=P, d_depth=P, d_alpha=P, d_rays=P)


def _call(lib, name, **defect):
    a = dict(GOOD)
    a.update(defect)
    f3 = ctypes.c_float * 3
    args = [a["poses"], a["NV"], a["W"], a["H"], 10.0, 10.0, 2.0, 2.0, 0.5, 3.0] if name == VIEWS_ENTRY else [a["rays"], a["R"]]
    args += [a["stored"], a["half"], a["M"], a["degree"], a["index"], a["bits"], *a["n"], f3(*a["c1"]), f3(*a["c2"]), a["step"], 0,
             a["term"], a["d_rgb"], a["d_depth"], a["d_alpha"], a["d_rays"], None]
    rc = getattr(lib, name)(*args)
    return rc, (lib.pnr_last_error().decode() if rc != 0 else "")


@pytest.mark.parametrize("name", [RAYS_ENTRY, VIEWS_ENTRY])
@pytest.mark.parametrize("half", [0, 1])
def test_every_refusal_of_the_ray_backward_entries(name, half):
    """each call carries one defect (or a pair that pins the order) and stand-in pointers that are never touched: the words and the
    order are those of pnr_baked_backward_*, d_rays in the place of d_stored, plus the storage_half rule after the degree's"""
    lib = _lib.load()
    camera = name == VIEWS_ENTRY
    sparse = dict(index=P, bits=P)
    src_bad, src_null, src_mis = (dict(NV=-1), dict(poses=None), dict(poses=P + 1)) if camera else (dict(R=-1), dict(rays=None), dict(rays=P + 1))
    none = dict(NV=0) if camera else dict(R=0)
    too_many = dict(W=2 ** 17, H=2 ** 17) if camera else dict(R=2 ** 34)
    what = "poses" if camera else "rays"
    aligned = "bits, d_rgb, d_depth, d_alpha and d_rays must be 4-byte aligned"
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
        (dict(d_rays=None), "null argument"), (dict(stored=None), "null argument"),
        (dict(index=P, bits=None), "null argument"),                      # sparse without bits
        (dict(stored=None, **sparse), "null argument"),
        (dict(stored=P + 8), "stored must be 16-byte aligned"), (dict(stored=P + 8, **sparse), "stored must be 16-byte aligned"),
        (dict(index=P + 2, bits=P), "index must be 4-byte aligned"),
        (dict(bits=P + 2), aligned), (dict(d_rgb=P + 2), aligned), (dict(d_depth=P + 1), aligned), (dict(d_alpha=P + 3), aligned),
        (dict(d_rays=P + 2), aligned),
        (too_many, "the number of rays exceeds the launch limit"),
        # two defects: the earlier check speaks
        (dict(degree=3, half=2), "degree must be -1 (RGBA), 0, 1 or 2"),
        (dict(half=2, **src_bad), "storage_half must be 0 or 1"),
        (dict(n=(1, 4, 4), **src_bad), "bad sizes (NV, W, H)" if camera else "bad sizes (R)"),
        (dict(M=-1, n=(1, 4, 4), **sparse), "bad sizes (M)"),
        (dict(step=0.0, term=1.0), "step must be finite and > 0"),
        (dict(term=1.0, d_rays=None), "terminate must lie in [0, 1)"),
        (dict(d_rays=None, stored=P + 8), "null argument"),
        (dict(stored=P + 8, d_rgb=P + 2), "stored must be 16-byte aligned"),
        (dict(d_rgb=P + 2, **too_many), aligned),
    ]
    for defect, words in expect:
        defect = dict(dict(half=half), **defect)
        assert _call(lib, name, **defect) == (-1, f"{name}: {words}"), (defect, _call(lib, name, **defect))
    # no rays: a no-op that looks at nothing else; a dense call does not look at M; the upstream gradients are optional
    assert _call(lib, name, half=half, stored=None, d_rays=None, d_rgb=None, **src_null, **none) == (0, "")
    assert _call(lib, name, half=2, **none) == (-1, f"{name}: storage_half must be 0 or 1")
    assert _call(lib, name, half=half, term=1.0, **none) == (-1, f"{name}: terminate must lie in [0, 1)")
    assert _call(lib, name, half=half, M=-1, **too_many)[1].endswith("the number of rays exceeds the launch limit")
    assert _call(lib, name, half=half, d_rgb=None, d_depth=None, d_alpha=None, **too_many)[1].endswith("the number of rays exceeds the launch limit")
    assert _call(lib, name, half=half, M=0, stored=None, **sparse, **too_many)[1].endswith("the number of rays exceeds the launch limit")


def test_python_layer_refuses_before_any_device_work():
    """from CPU tensors, before anything touches a device: a bad degree, a volume of the wrong shape, a sparse call without bits, a
    bad step, a CPU volume; an fp16 volume that requires grad; and the defaults of the trainable module keep their refusal"""
    from pixelnerf_amd import autograd, ops
    from pixelnerf_amd.util import bake
    rays, vol = torch.zeros(3, 8), torch.zeros(4, 4, 4, 4)
    geo = ((4, 4, 4), (-1.0,) * 3, (1.0,) * 3, 0.1)
    with pytest.raises(ValueError, match=r"degree must be None / -1 \(RGBA\), 0, 1 or 2, got 3"):
        ops.baked_ray_backward(rays, vol, 3, *geo)
    with pytest.raises(ValueError, match=r"stored must be \(nx,ny,nz,4,4\) at degree 1"):
        ops.baked_ray_backward(rays, vol.half(), 1, *geo)
    with pytest.raises(ValueError, match="index and bits are mandatory"):
        ops.baked_ray_backward(rays, torch.zeros(5, 4), None, *geo, index=torch.zeros(4, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="step must be finite and > 0"):
        ops.baked_ray_backward_views(torch.zeros(1, 4, 4), 4, 4, 10.0, None, 0.5, 3.0, vol, None, geo[0], geo[1], geo[2], 0.0)
    with pytest.raises(ValueError, match="the image must have at least one pixel"):
        ops.baked_ray_backward_views(torch.zeros(1, 4, 4), 0, 4, 10.0, None, 0.5, 3.0, vol, None, *geo)
    for stored in (vol, vol.half()):
        with pytest.raises(_lib.PixelNerfHipError, match="no CPU path"):
            ops.baked_ray_backward(rays.clone().requires_grad_(True), stored, None, *geo)
    with pytest.raises(TypeError, match=r"fp32 volumes only; fit the volume in fp32 and call half\(\) afterwards"):
        autograd.baked_march_rays_autograd(vol.half().requires_grad_(True), (rays,), None, *geo)
    with pytest.raises(TypeError, match="float32 or float16"):
        autograd.baked_march_rays_autograd(vol.double(), (rays,), None, *geo)
    with pytest.raises(ValueError, match=r"source must be \(rays,\) or \(poses, W, H, focal, c, z_near, z_far\)"):
        autograd.baked_march_rays_autograd(vol, (rays, 4, 4), None, *geo)
    with pytest.raises(ValueError, match="no gradient is given with respect to rays"):   # the entry without ray gradients keeps refusing
        autograd.baked_march_autograd(vol, (rays.clone().requires_grad_(True),), None, *geo)
    for cls in (bake.BakedVolume, bake.BakedSHVolume, bake.SparseBakedVolume):
        assert callable(cls.render_diff) and callable(cls.render_views_diff)
    with pytest.raises(TypeError, match="expected a baked volume"):
        bake.register(vol, torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4), 4, 4, 10.0, 0.5, 3.0)


# ---------------------------------------------------------------- 4. the pose update of register
def test_rodrigues_is_finite_and_exact_at_zero():
    """R(0) = I; dR/dw at 0 is the generator of each axis; no NaN in value or gradient at 0 or next to it; against the matrix
    exponential elsewhere; and the helper's restatement is the package's function"""
    from pixelnerf_amd.util import bake
    for dtype in (torch.float32, torch.float64):
        w = torch.zeros(2, 3, dtype=dtype, requires_grad=True)
        R = bake.rodrigues(w)
        assert torch.equal(R.detach(), torch.eye(3, dtype=dtype).expand(2, 3, 3))
        J = torch.autograd.functional.jacobian(lambda x: bake.rodrigues(x), torch.zeros(3, dtype=dtype))   # (3,3,3): dR_ij / dw_a
        assert bool(torch.isfinite(J).all())
        gen = torch.zeros(3, 3, 3, dtype=dtype)
        gen[2, 1, 0], gen[1, 2, 0], gen[0, 2, 1], gen[2, 0, 1], gen[1, 0, 2], gen[0, 1, 2] = 1, -1, 1, -1, 1, -1
        assert torch.equal(J, gen)
    for scale in (1e-9, 1e-4, 0.9e-3, 1.1e-3, 0.3, 2.5):
        w = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64) * scale
        K = torch.tensor([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=torch.float64)
        assert float((bake.rodrigues(w) - torch.linalg.matrix_exp(K)).abs().max()) < 1e-14
        assert torch.equal(bake.rodrigues(w), RG.rodrigues(w))
        J = torch.autograd.functional.jacobian(bake.rodrigues, w)
        assert bool(torch.isfinite(J).all())
    poses0 = torch.eye(4, dtype=torch.float64)[None].repeat(2, 1, 1)
    moved = bake.moved_poses(poses0, torch.zeros(2, 3, dtype=torch.float64), torch.tensor([[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]], dtype=torch.float64))
    assert torch.equal(moved[1], poses0[1]) and torch.equal(moved[0, :3, 3], torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64))
    assert torch.equal(moved, RG.moved_poses(poses0, torch.zeros(2, 3, dtype=torch.float64), moved[:, :3, 3]))


def test_host_registration_loop_converges_and_its_two_precisions_agree():
    """the yardstick of the GPU registration test: from 5 degrees and 0.12 off, 120 steps of Adam bring every camera's rotation and
    translation error down and the loss to about 1e-3 of its start; the fp32 and fp64 loops land on the same poses"""
    _, true, start = RG.reg_scene()
    true, start = torch.from_numpy(np.array(true)), torch.from_numpy(np.array(start))
    rot0, tr0 = RG.pose_errors(start, true)
    assert torch.allclose(rot0, torch.full((3,), 5.0, dtype=torch.float64), atol=1e-3) and torch.allclose(tr0, torch.full((3,), 0.12, dtype=torch.float64), atol=1e-5)
    p32, l32 = RG.register_ref(torch.float32)
    p64, l64 = RG.register_ref(torch.float64)
    rot32, tr32 = RG.pose_errors(p32, true)
    rot64, tr64 = RG.pose_errors(p64, true)
    print(f"host fp32: rotation {rot32.tolist()} deg, translation {tr32.tolist()}, loss {l32[0]:.4e} -> {l32[-1]:.4e}")
    print(f"host fp64: rotation {rot64.tolist()} deg, translation {tr64.tolist()}, loss {l64[0]:.4e} -> {l64[-1]:.4e}")
    assert float(rot32.mean()) <= 0.5 * 5.0 and float(tr32.mean()) <= 0.5 * 0.12
    assert l32[-1] < 0.05 * l32[0]
    assert torch.allclose(rot32, rot64, rtol=1e-2, atol=1e-3) and torch.allclose(tr32, tr64, rtol=1e-2, atol=1e-4)
    assert abs(l32[-1] - l64[-1]) <= 1e-2 * l64[-1]
