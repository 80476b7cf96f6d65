"""GPU tests (-m gpu) of the view-dependent baked volumes: pnr_baked_sh_render_rays / pnr_baked_sh_render_views through
ops.baked_sh_render / ops.baked_sh_render_views and util.bake.BakedSHVolume, against the fp64 restatement of tests/baked_sh_ref.py
(its own checks, and the checks of the inputs used here: tests/test_baked_sh_host.py).

Parity bar, per output, as tests/test_hip_baked.py: 4 x max |fp32 restatement - fp64 restatement| over the same inputs, computed
here; the factor covers the scan order of the product.  The measured gaps and the kernel's own errors are printed by the tests; the
record is profiles/baked_notes.md."""
import warnings

import numpy as np
import pytest
import torch

import baked_sh_ref as S

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def bake():
    from pixelnerf_amd.util import bake as _bake
    return _bake


@pytest.fixture(scope="module")
def common(dev, bake):
    """the shared coefficient volumes (degree 1 = the first 4 coefficients of degree 2), the rays per setting, and the restatement's
    answers (computed once, never modified)"""
    case = {"coef": {}, "sh": {}, "rays": {}, "ref": {}}
    for degree in (1, 2):
        case["coef"][degree] = S.common_coef(degree)
        case["sh"][degree] = bake.BakedSHVolume.from_tensor(torch.from_numpy(case["coef"][degree]).to(dev), S.C1, S.C2)
    for setting, (_, _, step) in S.SETTINGS.items():
        rays = S.common_rays(setting)
        case["rays"][setting] = torch.from_numpy(rays).to(dev)
        for degree in (1, 2):
            for white in (False, True):
                case["ref"][degree, setting, white] = tuple(
                    S.render_ref(rays, case["coef"][degree], S.C1, S.C2, step, degree, white_bkgd=white, dtype=dt) for dt in (np.float64, np.float32))
    return case


def _np(out):
    return tuple(t.cpu().numpy() for t in (out.rgb, out.depth, out.alpha))


def _equal(a, b):
    return torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.alpha, b.alpha)


def _hold_to_the_bar(tag, got, r64, r32):
    gap, err = S.gaps(r32, r64), S.gaps(got, r64)
    print(f"{tag}: fp32 - fp64 gap rgb {gap[0]:.3e} depth {gap[1]:.3e} alpha {gap[2]:.3e}; "
          f"kernel - fp64 rgb {err[0]:.3e} depth {err[1]:.3e} alpha {err[2]:.3e}")
    for name, g, e in zip(("rgb", "depth", "alpha"), gap, err):
        assert 0.0 < g < 1e-4, (name, g)
        assert e <= 4.0 * g, (name, e, 4.0 * g)


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
@pytest.mark.parametrize("degree", [1, 2])
def test_parity_with_the_fp64_restatement(common, degree, setting, white):
    step = S.SETTINGS[setting][2]
    sh = common["sh"][degree]
    assert sh.degree == degree and tuple(sh.coef.shape) == S.RESO + ((degree + 1) ** 2, 4)
    out = sh.render(common["rays"][setting], step=step, white_bkgd=white, skip=False)
    assert out.rgb.dtype == torch.float32 and tuple(out.rgb.shape) == (37, 3) and tuple(out.depth.shape) == tuple(out.alpha.shape) == (37,)
    r64, r32 = common["ref"][degree, setting, white]
    got = _np(out)
    _hold_to_the_bar(f"degree {degree} {setting} white={white}", got, r64, r32)
    bg = 1.0 if white else 0.0
    for r in (26, 27, 28, 29, 36):                                    # the misses and the near >= far ray: exactly the background
        assert (got[0][r] == bg).all() and got[1][r] == 0.0 and got[2][r] == 0.0, r


# ---------------------------------------------------------------- 2. the degenerate case is the RGBA march, bit for bit

@pytest.mark.parametrize("degree", [0, 2])
def test_dc_only_renders_the_bytes_of_the_rgba_volume(dev, bake, common, degree):
    coef = common["coef"][2][..., :(degree + 1) ** 2, :].copy()
    coef[..., 1:, :] = 0.0
    sh = bake.BakedSHVolume.from_tensor(torch.from_numpy(coef).to(dev), S.C1, S.C2)
    bv = bake.BakedVolume.from_tensor(torch.from_numpy(np.ascontiguousarray(coef[..., 0, :])).to(dev), S.C1, S.C2)
    assert sh.degree == degree and torch.equal(sh.occupancy.bits, bv.occupancy.bits)
    for setting, (_, _, step) in S.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in (dict(skip=False), dict(skip=True), dict(skip=False, terminate=1e-2), dict(skip=True, terminate=1e-2),
                   dict(skip=True, white_bkgd=True)):
            a, b = sh.render(rays, step=step, **kw), bv.render(rays, step=step, **kw)
            assert _equal(a, b), (setting, kw)
        assert float(a.alpha.max()) > 0.5


# ---------------------------------------------------------------- 3. one direction: the RGBA volume of that direction

def test_at_direction_is_the_volume_a_ray_sees(dev, bake, common):
    coef, sh = common["coef"][2], common["sh"][2]
    near, far, step = S.SETTINGS["n40"]
    d = np.array([-0.8, 0.45, -0.4])
    d = (d / np.linalg.norm(d)).astype(np.float32)
    rs = np.random.RandomState(9)
    lo, hi = np.array(S.C1), np.array(S.C2)
    rows = []
    for _ in range(8):                                                  # eight parallel rays through the inner part of the box
        target = lo + (0.3 + 0.4 * rs.uniform(size=3)) * (hi - lo)
        rows.append(np.concatenate((target - 3.0 * d.astype(np.float64), d, [near, far])))
    rays_np = np.asarray(rows, np.float32)
    assert (rays_np[:, 3:6] == d).all() and np.abs(d).min() > 0.3
    rays = torch.from_numpy(rays_np).to(dev)
    # the volume of that direction against the fp64 corner value
    bv = sh.at_direction(d)
    assert isinstance(bv, bake.BakedVolume) and tuple(bv.vol.shape) == S.RESO + (4,) and bv.c1 == sh.c1 and bv.c2 == sh.c2
    Y = S.sh_basis(d, 2)
    want = S.corner_value(coef, Y)
    bound = (9 + 2) * EPS24 * np.tensordot(np.abs(coef.astype(np.float64)), np.abs(Y), axes=(3, 0))
    err = np.abs(bv.vol.cpu().numpy().astype(np.float64) - want)
    print(f"at_direction: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    assert (want[..., :3] == 0).any() and (want[..., :3] == 1).any() and (want[..., 3][coef[..., 0, 3] > 0] == 0).any()   # clamps at work
    assert float((sh.at_direction(3.0 * d).vol - bv.vol).abs().max()) < 1e-4     # the length of d does not matter (to rounding)
    # the SH render of the rays against the restatement, at the parity bar
    out = sh.render(rays, step=step, skip=False)
    r64 = S.render_ref(rays_np, coef, S.C1, S.C2, step, 2)
    r32 = S.render_ref(rays_np, coef, S.C1, S.C2, step, 2, dtype=np.float32)
    _hold_to_the_bar("eight parallel rays, degree 2", _np(out), r64, r32)
    assert float(out.alpha.min()) > 0.5
    # ... which is the RGBA march through the volume of that direction: both are held to the same restatement
    via = bv.render(rays, step=step, skip=False)
    _hold_to_the_bar("the same rays through at_direction(d)", _np(via), r64, r32)
    # the higher coefficients are really read
    dc = bake.BakedSHVolume.from_tensor(torch.from_numpy(np.ascontiguousarray(coef[..., :1, :])).to(dev), S.C1, S.C2)
    diff = float((dc.render(rays, step=step, skip=False).rgb - out.rgb).abs().max())
    print(f"DC part alone against degree 2: max |d rgb| = {diff:.3f}")
    assert diff > 0.05


# ---------------------------------------------------------------- 4. skipping is exact; the same bytes twice

@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
@pytest.mark.parametrize("degree", [1, 2])
def test_skip_is_exact_and_calls_repeat(ops, common, degree, setting):
    sh, rays, step = common["sh"][degree], common["rays"][setting], S.SETTINGS[setting][2]
    assert sh.skip_threshold == 0.0 and sh.occupancy.dilate == 0 and 0.0 < sh.occupancy.occupied_fraction < 1.0
    for white in (False, True):
        plain = sh.render(rays, step=step, white_bkgd=white, skip=False)
        skipped = sh.render(rays, step=step, white_bkgd=white, skip=True)
        assert _equal(plain, skipped)
        assert _equal(plain, sh.render(rays, step=step, white_bkgd=white, skip=False))      # two calls, the same bytes
        assert _equal(skipped, sh.render(rays, step=step, white_bkgd=white, skip=True))
        rgb, depth, alpha = ops.baked_sh_render(rays, sh.coef, degree, sh.reso, sh.c1, sh.c2, step,
                                                bits=torch.zeros_like(sh.occupancy.bits), white_bkgd=white)
        assert (rgb == (1.0 if white else 0.0)).all() and (depth == 0).all() and (alpha == 0).all()  # nothing occupied: the background
    lead = sh.render(rays.reshape(37, 1, 8), step=step)                 # leading dimensions are kept
    assert tuple(lead.rgb.shape) == (37, 1, 3) and torch.equal(lead.rgb.reshape(37, 3), sh.render(rays, step=step).rgb)
    assert _equal(sh.render(rays), sh.render(rays, step=min(sh.cell_size)))   # step=None: the smallest cell edge
    bound = sh.sigma_bound().cpu().numpy().astype(np.float64)           # the field behind the skip grid
    s = np.abs(common["coef"][degree][..., 3].astype(np.float64))
    exact = common["coef"][degree][..., 0, 3].astype(np.float64) + (1.0 + 2.0 ** -16) * (s[..., 1:] * S.Y_MAX[:s.shape[-1] - 1]).sum(-1)
    assert (bound >= exact).all() and (bound <= exact * (1 + 2e-7)).all() and (bound[exact == 0] == 0).all()


# ---------------------------------------------------------------- 5. the camera form is the array form

@pytest.mark.parametrize("degree", [1, 2])
def test_views_equal_rays_of_the_same_cameras(dev, common, degree):
    from pixelnerf_amd import util
    sh = common["sh"][degree]
    poses = torch.stack([util.pose_spherical(30.0, -25.0, 3.0), util.pose_spherical(-110.0, 10.0, 2.6)]).float().to(dev)
    W, H, focal, c, z_near, z_far = 12, 10, (14.0, 11.5), (5.25, 5.5), 1.0, 4.6
    rays = util.gen_rays(poses, W, H, focal, z_near, z_far, c=c)
    assert tuple(rays.shape) == (2, H, W, 8)
    gt = torch.rand((2, H, W, 3), generator=torch.Generator().manual_seed(3)).to(dev)
    for kw in (dict(), dict(white_bkgd=True, skip=False, step=0.05), dict(terminate=1e-2)):
        views = sh.render_views(poses, W, H, focal, z_near, z_far, c=c, gt_rgb=gt, want_u8=True, **kw)
        assert _equal(views, sh.render(rays, **kw)), kw
        assert tuple(views.rgb.shape) == (2, H, W, 3) and tuple(views.depth.shape) == tuple(views.alpha.shape) == (2, H, W)
        assert tuple(views.psnr.shape) == tuple(views.ssim.shape) == (2,) and views.psnr.dtype == torch.float64
        assert views.rgb_u8.dtype == torch.uint8 and tuple(views.rgb_u8.shape) == (2, H, W, 3)
        assert float((views.depth_norm - (views.depth - z_near) / (z_far - z_near)).abs().max()) < 1e-6
        assert _equal(views, sh.render_views(poses, W, H, focal, z_near, z_far, c=c, **kw))
    assert float(views.alpha.max()) > 0.5 and float(views.alpha.min()) == 0.0       # the object and the background are both in view
    bare = sh.render_views(poses, W, H, focal, z_near, z_far, c=c)
    assert "psnr" not in bare and "rgb_u8" not in bare


# ---------------------------------------------------------------- 6. termination

@pytest.mark.parametrize("degree", [1, 2])
def test_termination_keeps_its_bound(common, degree):
    sh, eps = common["sh"][degree], 1e-2
    moved = 0.0
    for setting, (_, far, step) in S.SETTINGS.items():
        rays = common["rays"][setting]
        for skip in (False, True):
            plain = sh.render(rays, step=step, skip=skip)
            assert _equal(plain, sh.render(rays, step=step, skip=skip, terminate=None))
            assert _equal(plain, sh.render(rays, step=step, skip=skip, terminate=0.0))
            cut = sh.render(rays, step=step, skip=skip, terminate=eps)
            d_rgb, d_alpha, d_depth = (cut.rgb - plain.rgb).abs(), (cut.alpha - plain.alpha).abs(), (cut.depth - plain.depth).abs()
            print(f"degree {degree} {setting} terminate {eps} skip={skip}: max d rgb {float(d_rgb.max()):.3e}, d alpha "
                  f"{float(d_alpha.max()):.3e}, d depth {float(d_depth.max()):.3e}")
            assert (d_rgb <= eps).all() and (d_alpha <= eps).all() and (d_depth <= eps * far).all()
            moved = max(moved, float(d_alpha.max()))
    assert moved > 0.0                                                   # some ray of the 133-sample setting really stopped


# ---------------------------------------------------------------- 7. baking a network that IS a degree-2 function of the direction

class _Stub(torch.nn.Module):
    """net(xyz (1,N,3), coarse=, viewdirs=(1,N,3)) -> (1,N,4): at point n the degree-2 function sum_k c[n,k,:] Y_k(viewdirs),
    evaluated in fp64 with the basis of baked_sh_ref and rounded to fp32 once (so its own error is 2^-24 |value|)"""
    use_viewdirs = True

    def __init__(self, c, dev, ignore_direction=False):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.c, self.ignore = c, ignore_direction                         # c (N_total, 9, 4) fp64 numpy

    def forward(self, xyz, coarse=True, viewdirs=None):
        n = xyz.shape[1]
        vd = viewdirs[0].cpu().numpy()
        assert (vd == vd[0]).all()                                         # one direction per pass
        Y = S.sh_basis(vd[0], 2)
        if self.ignore:
            Y[1:] = 0.0
        out = np.tensordot(self.c[:n], Y, axes=(1, 0))
        return torch.from_numpy(out.astype(np.float32)).to(xyz.device)[None]


def test_baking_recovers_an_exact_network(dev, bake):
    reso, c1, c2, M = (5, 4, 3), (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8), 18
    rs = np.random.RandomState(31)
    c = np.empty((60, 9, 4))
    c[:, 0, :3], c[:, 0, 3] = 0.5, 5.0
    c[:, 1:, :3] = rs.uniform(-0.02, 0.02, (60, 8, 3))                   # sum_k max|Y_k| 0.02 = 0.31: rgb stays inside (0.1, 0.9)
    c[:, 1:, 3] = rs.uniform(-0.2, 0.2, (60, 8))                         # ... and sigma above 1.9
    dirs = bake.BakedSHVolume.directions(M).numpy()
    Ydirs = S.sh_basis(dirs, 2)
    values = np.einsum("nkc,mk->mnc", c, Ydirs)                          # (M, 60, 4): what the stub returns, before its rounding
    assert values[..., :3].min() > 0.1 and values[..., :3].max() < 0.9 and values[..., 3].min() > 0.0
    P = S.projection(dirs, 2)
    assert np.abs(np.einsum("km,mnc->nkc", P, values) - c).max() < 1e-12   # the function lies in the span: the fit is exact
    for ignore in (False, True):
        with warnings.catch_warnings():
            warnings.simplefilter("error", UserWarning)                  # real directions: no fake-direction warning
            sh = bake.BakedSHVolume.from_model(_Stub(c, dev, ignore), c1, c2, reso, degree=2, n_dirs=M)
        assert sh.degree == 2 and tuple(sh.coef.shape) == reso + (9, 4)
        v = values if not ignore else np.broadcast_to(c[None, :, 0, :], values.shape)
        # the fp32 projection, and the stub's one rounding carried through |P|
        bound = np.moveaxis(S.projection_bound(P, v) + EPS24 * np.tensordot(np.abs(P), np.abs(v), axes=(1, 0)), 0, 1) + 1e-12
        truth = c.copy()
        if ignore:
            truth[:, 1:, :] = 0.0
        err = np.abs(sh.coef.cpu().numpy().reshape(60, 9, 4).astype(np.float64) - truth)
        print(f"baking an exact degree-2 network (direction ignored: {ignore}): worst error / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
    # one more pass of the first kind renders: the volume is usable as baked
    rays = torch.tensor([[3.0, 0.1, 0.05, -1.0, 0.0, 0.0, 1.0, 5.0]], device=dev)
    assert float(sh.render(rays).alpha[0]) > 0.9


def test_a_network_without_view_directions_bakes_at_degree_0(dev, bake):
    class Plain(torch.nn.Module):
        use_viewdirs = False

        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))

        def forward(self, xyz, coarse=True, viewdirs=None):
            assert viewdirs is None
            return torch.cat((xyz[0].abs().clamp(0, 1), xyz[0, :, :1] ** 2), dim=1)[None]

    with pytest.warns(UserWarning, match="no view directions"):
        sh = bake.BakedSHVolume.from_model(Plain(), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (5, 4, 3), degree=2, n_dirs=18)
    assert sh.degree == 0 and tuple(sh.coef.shape) == (5, 4, 3, 1, 4)
    bv = bake.BakedVolume.from_model(Plain(), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (5, 4, 3))
    assert torch.equal(sh.coef[..., 0, :], bv.vol)


# ---------------------------------------------------------------- 8. baking the real network

def test_baking_through_the_model(ops, dev, bake):
    from helpers import scene_for
    from test_api_gpu import build_net
    scene, _ = scene_for("sn64")
    net = build_net(dev, scene)
    assert net.use_viewdirs and net.mlp_fine is not None
    c1, c2, reso, M = (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8), (5, 4, 3), 18
    net.train()
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)                      # real directions: no fake-direction warning
        sh = bake.BakedSHVolume.from_model(net, c1, c2, reso, degree=2, n_dirs=M)
    assert net.training                                                  # the flag is restored
    net.eval()
    assert sh.degree == 2 and tuple(sh.coef.shape) == reso + (9, 4) and sh.coef.is_cuda
    dirs = bake.BakedSHVolume.directions(M)
    with torch.no_grad():                                                # the network itself, once per direction, the fine one
        xyz, _ = ops.gen_grid_points(c1, c2, reso, device=dev, viewdirs=False)
        v = np.stack([net(xyz[None], coarse=False, viewdirs=dirs[m].to(dev).expand(60, 3).contiguous()[None])[0].cpu().numpy()
                      for m in range(M)]).astype(np.float64)             # (M, 60, 4)
    assert v.shape == (M, 60, 4) and np.abs(v - v[0]).max() > 0.0       # the network does look at the direction
    P = S.projection(dirs.numpy(), 2)
    want = np.moveaxis(np.tensordot(P, v, axes=(1, 0)), 0, 1)            # (60, 9, 4)
    bound = np.moveaxis(S.projection_bound(P, v), 0, 1)
    err = np.abs(sh.coef.cpu().numpy().reshape(60, 9, 4).astype(np.float64) - want)
    print(f"baking the network, M = {M}, degree 2: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")   # (sigma is exactly 0 at some points)
    assert (err <= bound).all()
    assert torch.equal(bake.BakedSHVolume.from_model(net, c1, c2, reso, degree=2, n_dirs=M, eval_batch_size=7).coef, sh.coef)
    assert torch.equal(bake.BakedSHVolume.from_model(net, c1, c2, reso, degree=2, n_dirs=M).coef, sh.coef)   # and from run to run
    coarse = bake.BakedSHVolume.from_model(net, c1, c2, reso, degree=1, n_dirs=8, coarse=True)
    assert coarse.degree == 1 and tuple(coarse.coef.shape) == reso + (4, 4)
    # a round trip through the state renders the same bytes
    rays = torch.from_numpy(S.common_rays("n40")).to(dev)
    state = {k: t.cpu() for k, t in sh.state_dict().items()}
    assert "coef" in state and "degree" not in state
    back = bake.BakedSHVolume.from_state_dict(state, device=dev)
    assert torch.equal(back.coef, sh.coef) and back.degree == 2 and back.c1 == sh.c1 and back.c2 == sh.c2
    assert back.skip_threshold == sh.skip_threshold and torch.equal(back.occupancy.bits, sh.occupancy.bits)
    a, b = sh.render(rays, white_bkgd=True), back.render(rays, white_bkgd=True)
    assert _equal(a, b) and float(a.alpha.max()) > 0.0
    net.num_objs = 2
    try:
        with pytest.raises(ValueError, match="encode one object"):
            bake.BakedSHVolume.from_model(net, c1, c2, reso)
    finally:
        net.num_objs = 1
    bad = sh.coef.clone()
    bad[3, 2, 1, 5, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        bake.BakedSHVolume.from_tensor(bad, c1, c2)
