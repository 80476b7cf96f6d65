"""CPU tests of the view-dependent baked volumes: the numpy restatement (tests/baked_sh_ref.py) against baked_ref and against the
conditions the GPU parity bar rests on, the projection used for baking, and the header / binding / wrapper layer, whose argument
checks all come before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baked_ref as B
import baked_sh_ref as S
from pixelnerf_amd import _lib


@pytest.fixture(scope="module")
def coef2():
    return S.common_coef(2)


# ---------------------------------------------------------------- the restatement

@pytest.mark.parametrize("degree", [0, 1, 2])
def test_dc_only_is_the_rgba_restatement(coef2, degree):
    """coefficients k >= 1 zeroed: v_0 * 1 + 0 * Y_k is exact and the clamps change nothing, in fp32 and in fp64"""
    coef = coef2[..., :S.n_basis(degree), :].copy()
    coef[..., 1:, :] = 0.0
    vol = np.ascontiguousarray(coef[..., 0, :])
    assert np.array_equal(vol, B.common_volume())
    rays, step = S.common_rays("n40"), S.SETTINGS["n40"][2]
    cells = np.ones(tuple(n - 1 for n in S.RESO), bool)
    cells[2:4, 2:4, 2:4] = False                                      # the cells of the empty block
    for dtype in (np.float32, np.float64):
        for kw in (dict(), dict(white_bkgd=True), dict(terminate=1e-2), dict(occupied=cells)):
            want = B.render_ref(rays, vol, S.C1, S.C2, step, dtype=dtype, **kw)
            got = S.render_ref(rays, coef, S.C1, S.C2, step, degree, dtype=dtype, **kw)
            assert all(g.dtype == dtype and np.array_equal(g, w) for g, w in zip(got, want)), (dtype, kw)


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
def test_gpu_parity_inputs_carry_their_bar(coef2, setting, degree):
    """what tests/test_hip_baked_sh.py's parity bar rests on: the fp32 restatement differs from the fp64 one, by less than 1e-4,
    on every output; every clamp is exercised by the rays' directions; the empty parts stay empty for every direction"""
    coef = np.ascontiguousarray(coef2[..., :S.n_basis(degree), :])
    rays, step = S.common_rays(setting), S.SETTINGS[setting][2]
    assert (coef[..., 1:, 3][coef[..., 0, 3] == 0] == 0).all() and np.abs(coef[..., 1:, 3]).max() > 3.5
    assert np.abs(coef[..., 1:, :3]).max() <= 0.25
    lo = hi = neg = 0
    for d in rays[:26, 3:6]:
        Y = S.sh_basis(d, degree)
        raw = np.tensordot(coef.astype(np.float64), Y, axes=(3, 0))
        lo, hi = lo + (raw[..., :3] < 0).mean(), hi + (raw[..., :3] > 1).mean()
        neg += (raw[..., 3][coef[..., 0, 3] > 0] < 0).mean()
    print(f"degree {degree}: corner colours below 0 {lo / 26:.3f}, above 1 {hi / 26:.3f}; positive-DC sigmas below 0 {neg / 26:.3f}")
    assert lo / 26 > 0.02 and hi / 26 > 0.02 and neg / 26 > 0.02
    for white in (False, True):
        r64 = S.render_ref(rays, coef, S.C1, S.C2, step, degree, white_bkgd=white)
        r32 = S.render_ref(rays, coef, S.C1, S.C2, step, degree, white_bkgd=white, dtype=np.float32)
        g = S.gaps(r32, r64)
        print(f"degree {degree} {setting} white={white}: fp32 - fp64 gap rgb {g[0]:.3e} depth {g[1]:.3e} alpha {g[2]:.3e}")
        assert all(0.0 < x < 1e-4 for x in g), g
        alpha = r64[2]
        assert (alpha[:26] > 0.5).sum() >= 20
        assert (alpha[26:30] == 0).all() and alpha[36] == 0 and (r64[0][36] == (1.0 if white else 0.0)).all()
        assert (alpha[30:36] > 0).all()


def test_basis_is_orthonormal_and_bounded():
    dirs = S.fibonacci_directions(4096)
    Y = S.sh_basis(dirs, 2)
    assert Y.shape == (4096, 9) and (Y[:, 0] == 1).all()
    assert np.abs(Y.T @ Y / 4096 - np.eye(9)).max() < 1e-2
    assert (np.abs(Y[:, 1:]).max(axis=0) <= S.Y_MAX * (1 + 1e-6)).all()     # the maxima the skip grid's bound uses
    assert (np.abs(Y[:, 1:]).max(axis=0) >= S.Y_MAX * 0.98).all()
    assert np.array_equal(S.sh_basis(dirs, 1), Y[:, :4]) and np.array_equal(S.sh_basis(dirs, 0), Y[:, :1])
    assert np.array_equal(S.sh_basis(3.0 * dirs[5], 2, np.float32), S.sh_basis(np.float32(3.0) * dirs[5], 2, np.float32))
    for bad in ((0.0, 0.0, 0.0), (np.inf, 0.0, 0.0), (np.nan, 1.0, 0.0)):
        for dtype in (np.float32, np.float64):
            y = S.sh_basis(np.array(bad, np.float32), 2, dtype)
            assert y[0] == 1 and (y[1:] == 0).all(), (bad, y)
    y = S.sh_basis(np.array((1e30, 1e30, 0.0), np.float32), 2, np.float32)   # the squared norm overflows in fp32 (not in fp64)
    assert y[0] == 1 and (y[1:] == 0).all()
    with pytest.raises(ValueError):
        S.sh_basis(dirs, 3)


# ---------------------------------------------------------------- python, before any device work

def test_directions_and_projection():
    from pixelnerf_amd.util.bake import BakedSHVolume, sh_basis
    for n in (8, 18, 32):
        d = BakedSHVolume.directions(n)
        assert d.dtype == torch.float32 and tuple(d.shape) == (n, 3) and not d.is_cuda
        assert float((d.double().norm(dim=1) - 1.0).abs().max()) < 1e-6
        assert torch.equal(d, BakedSHVolume.directions(n))
        assert np.abs(d.numpy() - S.fibonacci_directions(n)).max() < 1e-7
    dirs = BakedSHVolume.directions(32)
    for dtype, np_dtype in ((torch.float32, np.float32), (torch.float64, np.float64)):   # the package's basis is the restatement's
        assert np.array_equal(sh_basis(dirs, 2, dtype).numpy(), S.sh_basis(dirs.numpy(), 2, np_dtype))
    assert np.array_equal(sh_basis(torch.zeros(3), 2).numpy(), np.array([1.0] + [0.0] * 8, np.float32))
    for degree, n_min in ((0, 2), (1, 8), (2, 18)):
        with pytest.raises(ValueError):
            BakedSHVolume.projection(n_min - 1, degree)
        P = BakedSHVolume.projection(n_min, degree)
        assert P.dtype == torch.float64 and tuple(P.shape) == ((degree + 1) ** 2, n_min)
    with pytest.raises(ValueError):
        BakedSHVolume.projection(32, 3)
    for n, degree, cond in ((32, 2, 1.06), (18, 2, 1.17), (8, 1, 1.17)):
        assert np.linalg.cond(S.sh_basis(S.fibonacci_directions(n), degree)) < cond
        assert np.abs(BakedSHVolume.projection(n, degree).numpy() - S.projection(BakedSHVolume.directions(n).numpy(), degree)).max() < 1e-12


def test_projection_in_fp32_keeps_its_bound():
    """fp32(P) applied sequentially in fp32, as from_model applies it, against the fp64 product: (M + 2) 2^-24 (|P| @ |v|)"""
    from pixelnerf_amd.util.bake import BakedSHVolume
    M = 32
    P = BakedSHVolume.projection(M, 2).numpy()
    v = np.random.RandomState(5).uniform(0.0, 1.0, (M, 1000, 4)).astype(np.float32)
    P32 = P.astype(np.float32)
    acc = np.zeros((9, 1000, 4), np.float32)
    for m in range(M):
        for k in range(9):
            acc[k] = acc[k] + v[m] * P32[k, m]
    want = np.tensordot(P, v.astype(np.float64), axes=(1, 0))
    bound = S.projection_bound(P, v)
    ratio = float((np.abs(acc.astype(np.float64) - want) / bound).max())
    print(f"fp32 projection, M = {M}, degree 2: worst error / bound = {ratio:.3f}")
    assert acc.dtype == np.float32 and ratio <= 1.0


def test_wrappers_refuse_before_any_device_work():
    from pixelnerf_amd import ops
    from pixelnerf_amd.util import bake
    from pixelnerf_amd.util.bake import BakedSHVolume
    coef, rays, poses = torch.zeros(4, 5, 6, 9, 4), torch.zeros(3, 8), torch.eye(4)[None]
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    assert bake.BakedSHVolume is BakedSHVolume and issubclass(BakedSHVolume, object)
    # CPU tensors: there is no CPU path
    with pytest.raises(_lib.PixelNerfHipError):
        BakedSHVolume.from_tensor(coef, lo, hi)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_sh_render(rays, coef, 2, (4, 5, 6), lo, hi, 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_sh_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, coef, 2, (4, 5, 6), lo, hi, 0.1)
    sh = BakedSHVolume.__new__(BakedSHVolume)                          # a volume object without its device parts
    sh.coef, sh.degree, sh.reso, sh.c1, sh.c2, sh.skip_threshold = coef, 2, (4, 5, 6), lo, hi, 0.0
    with pytest.raises(_lib.PixelNerfHipError):
        sh.render(rays, skip=False)
    with pytest.raises(_lib.PixelNerfHipError):
        sh.render_views(poses, 4, 4, 10.0, 0.5, 3.0, skip=False)
    assert sh.cell_size == (2 / 3, 2 / 4, 2 / 5)
    # the degree and the shape must agree
    for c, degree in ((coef, 1), (coef, 0), (coef[..., :4, :], 2), (coef, 3), (coef, -1), (torch.zeros(4, 5, 6, 4), 0),
                      (torch.zeros(4, 5, 6, 9, 3), 2), (torch.zeros(4, 5, 7, 9, 4), 2)):
        with pytest.raises(ValueError):
            ops.baked_sh_render(rays, c, degree, (4, 5, 6), lo, hi, 0.1)
        with pytest.raises(ValueError):
            ops.baked_sh_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, c, degree, (4, 5, 6), lo, hi, 0.1)
    # the march settings: _baked_args' refusals
    bad = [dict(reso=(4, 5)), dict(c1=hi, c2=lo), dict(c1=(0, 0)), dict(c2=(1.0, float("inf"), 1.0)), dict(step=0.0), dict(step=-1.0),
           dict(step=float("nan")), dict(step=float("inf")), dict(terminate=-0.1), dict(terminate=1.0), dict(terminate=float("nan"))]
    for kw in bad:
        a = dict(reso=(4, 5, 6), c1=lo, c2=hi, step=0.1, terminate=0.0)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.baked_sh_render(rays, coef, 2, a["reso"], a["c1"], a["c2"], a["step"], terminate=a["terminate"])
        with pytest.raises(ValueError):
            ops.baked_sh_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, coef, 2, a["reso"], a["c1"], a["c2"], a["step"],
                                      terminate=a["terminate"])
    with pytest.raises(ValueError):
        ops.baked_sh_render_views(poses, 0, 4, 10.0, None, 0.5, 3.0, coef, 2, (4, 5, 6), lo, hi, 0.1)
    for c, a, b in ((torch.zeros(4, 5, 6, 4), lo, hi), (torch.zeros(4, 5, 6, 9, 3), lo, hi), (torch.zeros(4, 5, 6, 5, 4), lo, hi),
                    (torch.zeros(4, 5, 6, 16, 4), lo, hi), (coef.double(), lo, hi), (torch.zeros(1, 5, 6, 9, 4), lo, hi), (coef, hi, lo),
                    (coef, lo, (1.0, 1.0))):
        with pytest.raises(ValueError):
            BakedSHVolume.from_tensor(c, a, b)
    with pytest.raises(ValueError):
        BakedSHVolume.from_tensor(coef, lo, hi, skip_threshold=float("nan"))
    with pytest.raises(ValueError):
        sh.render(torch.zeros(3, 7))
    with pytest.raises(ValueError):
        sh.render_views(torch.eye(4), 4, 4, 10.0, 0.5, 3.0)
    with pytest.raises(ValueError):
        sh.render_views(poses, 4, 4, 10.0, 0.5, 3.0, gt_rgb=torch.zeros(1, 4, 5, 3))
    with pytest.raises(ValueError):
        sh.at_direction((1.0, 0.0))

    class TwoObjects(torch.nn.Module):
        num_objs = 2

    with pytest.raises(ValueError, match="encode one object"):
        BakedSHVolume.from_model(TwoObjects(), lo, hi, (4, 5, 6))
    for kw in (dict(degree=2, n_dirs=17), dict(degree=1, n_dirs=7), dict(degree=3), dict(degree=-1)):
        with pytest.raises(ValueError):
            BakedSHVolume.from_model(torch.nn.Linear(3, 4), lo, hi, (4, 5, 6), **kw)


# ---------------------------------------------------------------- header, binding, entries

def test_header_declares_and_binding_binds(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in (("pnr_baked_sh_render_rays", 17), ("pnr_baked_sh_render_views", 25)):
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)", code)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
    lib = _lib.load()
    assert lib.pnr_abi_version() == 12
    assert hasattr(lib, "pnr_baked_sh_render_rays") and hasattr(lib, "pnr_baked_sh_render_views")
    assert "pnr_baked.hip" in _lib.SOURCES


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    lo, hi = _f3(-1, -1, -1), _f3(1, 1, 1)
    P = 64  # a non-null, 16-byte aligned stand-in for a device pointer: every call below must fail before it is touched

    def rays(R=4, rays_p=P, coef=P, degree=2, bits=None, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P, depth=P, alpha=P):
        return lib.pnr_baked_sh_render_rays(rays_p, R, coef, degree, bits, n[0], n[1], n[2], c1, c2, step, 0, term, rgb, depth, alpha, None)

    def views(poses=P, NV=1, W=4, H=4, coef=P, degree=2, n=(4, 4, 4), c1=lo, c2=hi, step=0.1, term=0.0, rgb=P, depth=P, alpha=P):
        return lib.pnr_baked_sh_render_views(poses, NV, W, H, 10.0, 10.0, 2.0, 2.0, 0.5, 3.0, coef, degree, None, n[0], n[1], n[2], c1, c2,
                                             step, 0, term, rgb, depth, alpha, None)

    for call in (rays, views):
        for degree in (3, -1, 9):
            assert call(degree=degree) == -1 and b"degree" in lib.pnr_last_error()
        for degree in (0, 1, 2):
            assert call(coef=P + 8, degree=degree) == -1 and b"16-byte" in lib.pnr_last_error()
            assert call(coef=None, degree=degree) == -1 and b"null" in lib.pnr_last_error()
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
    assert rays(R=-1) == -1 and rays(rays_p=None) == -1 and rays(rays_p=P + 1) == -1 and rays(bits=P + 2) == -1
    assert rays(R=2 ** 34) == -1 and b"launch limit" in lib.pnr_last_error()
    assert views(NV=-1) == -1 and views(W=0) == -1 and views(H=-3) == -1 and views(poses=None) == -1
    for degree in (0, 1, 2):
        assert rays(R=0, rays_p=None, coef=None, degree=degree, rgb=None, depth=None, alpha=None) == 0      # no rays: a no-op
        assert views(NV=0, poses=None, coef=None, degree=degree, rgb=None, depth=None, alpha=None) == 0
    assert rays(R=0, degree=3) == -1 and views(NV=0, degree=-1) == -1   # the degree is refused even then
