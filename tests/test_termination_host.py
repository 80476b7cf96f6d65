"""Host tests (no GPU) of early ray termination: pnr_termination_mark is declared, exported, bound and wrapped, and refuses bad
arguments before any HIP call; the ABI revision stays 12 and a library without the entry is reported as stale; the numpy
restatement of tests/termination_ref.py agrees with a hand-computed case, and on the frozen reference outputs of
tests/golden/adv_surface_sn64.npz the definition is neither vacuous nor hollowed out by ambiguity and keeps its error bound;
the renderer's refusals fire before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import termination_ref as T
from pixelnerf_amd import _lib

ENTRY = "pnr_termination_mark"
EPS = 1e-2


def test_header_declares_the_entry_and_the_abi_revision_stays_12(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    _lib.build_library()
    lib = _lib.load()
    assert ENTRY in _lib.PROTOTYPES and re.search(ENTRY + r"\s*\(", code)
    assert len(_lib.PROTOTYPES[ENTRY][1]) == 12
    assert hasattr(lib, ENTRY)
    assert lib.pnr_abi_version() == 12
    from pixelnerf_amd import ops
    from pixelnerf_amd.render import NeRFRenderer
    assert callable(ops.termination_mark)
    assert NeRFRenderer(n_coarse=4, n_fine=4).last_terminate_stats is None


def test_a_library_without_the_entry_is_reported_as_stale(monkeypatch):
    """the entry was added within revision 12: a revision-12 library built before it must give the usual rebuild message"""
    _lib.build_library()
    real = ctypes.CDLL(_lib.LIB_PATH)

    class Old:
        def __getattr__(self, name):
            if name == ENTRY:
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_lib.PixelNerfHipError, match=r"pnr_termination_mark.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_the_entry_refuses_bad_arguments_on_the_host():
    """PNR_E_INVALID (-1) before any HIP call; the addresses are dummies, never dereferenced"""
    _lib.build_library()
    lib = _lib.load()
    mark = lambda rays=64, z=64, rs=64, R=8, K=4, k0=0, k1=4, eps=EPS, keep_in=None, keep=64, t=None: lib.pnr_termination_mark(  # noqa: E731
        rays, z, rs, R, K, k0, k1, eps, keep_in, keep, t, None)
    err = lib.pnr_last_error
    assert mark(R=-1) == -1 and err().startswith(b"pnr_termination_mark:") and b"sizes" in err()
    assert mark(K=0, k1=0) == -1 and b"sizes" in err()
    assert mark(R=1 << 16, K=1 << 15, k1=4) == -1 and b"2^31" in err()
    for k0, k1 in ((-1, 4), (3, 2), (0, 5), (5, 5)):
        assert mark(k0=k0, k1=k1) == -1 and b"k_begin <= k_end <= K" in err(), (k0, k1)
    for eps in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert mark(eps=eps) == -1 and b"eps" in err(), eps
    for name in ("rays", "z", "rs", "keep"):
        assert mark(**{name: None}) == -1 and b"null" in err(), name
    assert mark(R=0) == 0 and mark(R=0, rays=None, z=None, rs=None, keep=None) == 0                # R = 0: a no-op
    assert mark(k0=4, k1=4, R=0) == 0 and mark(k0=0, k1=0, R=0) == 0                                # (empty stages are valid)


def test_stage_boundaries():
    assert T.stage_bounds(96, 4) == [0, 24, 48, 72, 96] and T.stage_bounds(192, 4) == [0, 48, 96, 144, 192]
    assert T.stage_bounds(96, 1) == [0, 96] and T.stage_bounds(11, 3) == [0, 2, 6, 11] and T.stage_bounds(3, 8) == [0, 2, 3]
    assert T.stage_bounds(1, 4) == [0, 1] and T.stage_bounds(96, [10, 11]) == [0, 10, 11, 96]
    for K, S in ((96, 4), (192, 8), (200, 7), (64, 64)):
        assert all(b % 2 == 0 for b in T.stage_bounds(K, S))                # no pair (2j, 2j+1) straddles a stage
    for bad in (0, -1, [0], [96], [5, 5], [7, 3]):
        with pytest.raises(ValueError):
            T.stage_bounds(96, bad)


def test_restatement_on_the_hand_made_rays():
    """opaque at sample 1; transparent throughout; crossing eps between two boundaries"""
    rays, z, rs, want = T.hand_case()
    f = T.factors(rays, z, rs)
    assert f.dtype == np.float32 and f[0, 1] == np.float32(1e-10) and (f[1] == 1.0).all()
    assert np.allclose(f[2], np.exp(-2.0), rtol=1e-6)
    for bounds, stop_want in want.items():
        stop, amb = T.stops(rays, z, rs, list(bounds), EPS)
        assert stop.tolist() == stop_want and not amb.any(), bounds
    lo, hi, nan = T.bracket(f, 2)
    assert lo[0] == 0.0 and hi[0] < 1e-6 and lo[1] > 0.999 and lo[2] <= np.exp(-4.0) <= hi[2] and hi[2] - lo[2] < 1e-6 and not nan.any()
    keep, lo, hi, amb = T.mark_ref(rays, z, rs, 2, 4, EPS, keep_in=np.array([[1, 1, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1]]))
    assert keep.tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 1]] and not amb.any()
    # an eps inside the bracket of ray 2 is undecided; a NaN factor keeps the ray alive, decided
    _, amb = T.stops(rays, z, rs, [0, 2, 4], float(np.exp(-4.0)))
    assert amb.tolist() == [False, False, True]
    rs[0, 0, 3] = np.nan                                                      # fmaxf drops it: still opaque at sample 1
    z[1, 1] = np.nan                                                          # a NaN interval: the transmittance is NaN
    stop, amb = T.stops(rays, z, rs, [0, 2, 4], EPS)
    assert stop.tolist() == [2, 4, 4] and not amb.any()
    # zeroing behind the stop, and the counts of a call
    out = T.zero_behind(rs, [2, 4, 3])
    assert not out[0, 2:].any() and np.array_equal(out[1], rs[1], equal_nan=True) and not out[2, 3:].any() and out[2, :3].all()
    assert T.counts(np.array([2, 4, 3]), [0, 2, 3, 4]) == {"evaluated": 9, "total": 12, "stopped_rays": 2, "rays": 3,
                                                            "stages": [(6, 6), (2, 3), (1, 3)]}


def test_the_golden_fine_pass_is_neither_vacuous_nor_hollow():
    """the frozen reference outputs of adv_surface_sn64 (96 rays, K = 192, boundaries 48 / 96 / 144), eps = 1e-2, 4 stages:
    44 rays stop, 72.1 % of the samples are evaluated, no ray is ambiguous, and Bound B holds in fp64 on the 85 rays whose
    intervals are all non-negative (max |d rgb| 2.6e-3; the others have a depth sample beyond `far`)"""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adv_surface_sn64.npz"))
    rays, z, rs = g["rays"].reshape(-1, 8), g["fine_z"], g["fine_rgbsigma"]
    R, K = z.shape
    bounds = T.stage_bounds(K, 4)
    assert bounds == [0, 48, 96, 144, 192]
    stop, amb = T.stops(rays, z, rs, bounds, EPS)
    c = T.counts(stop, bounds)
    delta = np.concatenate([z[:, 1:], rays[:, 7:8]], axis=1) - z
    ok = (delta >= 0).all(axis=1)
    white = bool(g["white_bkgd"])
    w_d, rgb_d, depth_d, t_end = T.composite64(rays, z, rs, white)
    w_t, rgb_t, depth_t, _ = T.composite64(rays, z, T.zero_behind(rs, stop), white)
    d_rgb, d_depth = np.abs(rgb_d - rgb_t).max(axis=1), np.abs(depth_d - depth_t)
    print(f"stopped {c['stopped_rays']} of {R}, evaluated {c['evaluated'] / c['total']:.4f}, ambiguous {int(amb.sum())}, rays with all "
          f"delta >= 0: {int(ok.sum())}, max |d rgb| on them {d_rgb[ok].max():.3e}, max |d depth| {d_depth[ok].max():.3e}")
    assert 0.30 <= c["stopped_rays"] / R <= 0.60
    assert c["evaluated"] / c["total"] <= 0.80
    assert amb.mean() <= T.AMBIGUOUS_CAP
    assert ok.sum() >= 80
    # Bound B: the weights behind the stop and the final transmittance sum to T at the stop, which is <= eps
    far = rays[:, 7].astype(np.float64)
    behind = np.arange(K)[None, :] >= stop[:, None]
    t_stop = (w_d * behind).sum(axis=1) + t_end
    stopped = ok & (stop < K)
    assert stopped.sum() >= 30 and (t_stop[stopped] <= EPS * (1 + 1e-6)).all()
    assert (d_rgb[ok] <= EPS).all() and (d_depth[ok] <= EPS * far[ok]).all()
    assert np.array_equal(w_t[~behind], w_d[~behind]) and not w_t[behind].any()
    sign = 1.0 if white else -1.0                                             # towards the background, on every channel
    assert (sign * (rgb_t - rgb_d)[ok] >= -1e-12).all()
    assert d_rgb.max() > 1e-4                                                 # (and it is not the dense render)


class _Untouchable:
    def __call__(self, *a, **k):
        raise AssertionError("the model must not be called")


def test_refusals_fire_before_any_device_work():
    import torch
    from pixelnerf_amd.render import NeRFRenderer
    rend = NeRFRenderer(n_coarse=4, n_fine=4).eval()
    model = _Untouchable()
    rays = torch.zeros((1, 3, 8))                                             # CPU tensors: nothing can launch
    pose = torch.eye(4)[None]
    par = rend.bind_parallel(model, None, simple_output=True)
    calls = [lambda **kw: rend(model, rays, **kw), lambda **kw: par(rays, **kw),
             lambda **kw: rend.render_views(model, pose, 4, 4, 10.0, 1.0, 2.0, **kw),
             lambda **kw: par.render_views(pose, 4, 4, 10.0, 1.0, 2.0, **kw)]
    for call in calls:
        for eps in (0.0, 1.0, -1e-2, 2.0, float("nan"), "a"):
            with pytest.raises(ValueError, match=r"terminate: eps must lie in \(0, 1\)"):
                call(terminate=eps)
        for stages in (0, -3, 2.5, [0, 4], [4, 4], [6, 2], [8], True):
            with pytest.raises(ValueError, match="terminate_stages"):
                call(terminate=EPS, terminate_stages=stages)
        with pytest.raises(NotImplementedError, match="generic model callable"):
            call(terminate=EPS)
        with pytest.raises(NotImplementedError, match="generic model callable"):
            call(terminate=EPS, terminate_stages=[2, 6])
    with pytest.raises(ValueError, match="ONE object"):
        rend(model, torch.zeros((2, 3, 8)), terminate=EPS)
    with pytest.raises(ValueError, match="ONE object"):
        rend.render_views(model, torch.eye(4).expand(2, 1, 4, 4), 4, 4, 10.0, 1.0, 2.0, terminate=EPS)
    with pytest.raises(NotImplementedError, match="under torch.no_grad"):
        rend(model, rays.clone().requires_grad_(True), terminate=EPS)
    coarse_only = NeRFRenderer(n_coarse=4, n_fine=0).eval()
    with pytest.raises(NotImplementedError, match="FINE pass"):
        coarse_only(model, rays, terminate=EPS)
    with pytest.raises(NotImplementedError, match="FINE pass"):
        coarse_only.render_views(model, pose, 4, 4, 10.0, 1.0, 2.0, terminate=EPS)
    assert rend.last_terminate_stats is None and coarse_only.last_terminate_stats is None
    assert rend.last_skip_stats is None

    # the ORDER of the refusals across feature sets: of two broken conditions the earlier one of the documented list (objects, fine
    # pass, grad, capture, non-fused model) is raised, whatever else is asked for; and a refused call leaves the stats alone
    class Reached(Exception):
        pass

    class Grid:
        def clip_rays(self, rays):
            raise Reached

    grid = Grid()
    sets = [dict(occupancy=grid), dict(occupancy=grid, skip_empty=True), dict(terminate=EPS), dict(occupancy=grid, terminate=EPS),
            dict(occupancy=grid, skip_empty=True, terminate=EPS)]
    skip_before, term_before = {"coarse": (1, 2), "fine": (3, 4)}, {"evaluated": 5, "total": 6, "stopped_rays": 1, "rays": 2, "stages": [(5, 6)]}
    two_rays, two_poses, grad_rays = torch.zeros((2, 3, 8)), torch.eye(4).expand(2, 1, 4, 4), rays.clone().requires_grad_(True)

    def entries(r, rays, poses):
        p = r.bind_parallel(model, None, simple_output=True)
        return [lambda **kw: r(model, rays, **kw), lambda **kw: p(rays, **kw),
                lambda **kw: r.render_views(model, poses, 4, 4, 10.0, 1.0, 2.0, **kw),
                lambda **kw: p.render_views(poses, 4, 4, 10.0, 1.0, 2.0, **kw)]

    def refused(r, call, exc, match, kw):
        r.last_skip_stats, r.last_terminate_stats = dict(skip_before), dict(term_before)
        with pytest.raises(exc, match=match):
            call(**kw)
        assert r.last_skip_stats == skip_before and r.last_terminate_stats == term_before, kw

    for kw in sets:
        for call in entries(coarse_only, two_rays, two_poses):                # two objects and no fine pass
            refused(coarse_only, call, ValueError, "ONE object", kw)
        for call in entries(coarse_only, grad_rays, pose)[:2]:                # no fine pass and rays that require grad
            refused(coarse_only, call, NotImplementedError, "FINE pass" if "terminate" in kw else "no_grad", kw)
        for call in entries(rend, grad_rays, pose)[:2]:                       # rays that require grad and the generic model
            refused(rend, call, NotImplementedError, "no_grad", kw)
    for call in entries(rend, rays, pose)[:2]:                                # a well-formed culled call passes every refusal, and
        refused(rend, call, Reached, None, dict(occupancy=grid))              # touches the grid only then
    for call in entries(rend, rays, pose)[2:]:                                # (render_views makes its rays on the device before it
        refused(rend, call, _lib.PixelNerfHipError, "no CPU path", dict(occupancy=grid))  # asks the grid: host poses end there)
