"""GPU tests (-m gpu) of the baked-volume ray march: pnr_baked_render_rays / pnr_baked_render_views through ops.baked_render /
ops.baked_render_views and util.bake.BakedVolume, against the fp64 restatement of tests/baked_ref.py (its own checks, and the
checks of the inputs used here: tests/test_baked_host.py).

Parity bar, per output: 4 x max |fp32 restatement - fp64 restatement| over the same inputs, computed here -- what two correct fp32
implementations differ by; the factor covers the scan order of the product, which differs from the restatement's sequential loop.
The measured gaps and the kernel's own errors are printed by the test; the record is profiles/baked_notes.md."""
import warnings

import numpy as np
import pytest
import torch

import baked_ref as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def BakedVolume():
    from pixelnerf_amd.util.bake import BakedVolume as _BakedVolume
    return _BakedVolume


@pytest.fixture(scope="module")
def common(dev, BakedVolume):
    """the shared volume, its rays per setting, and the restatement's answers (computed once, never modified)"""
    vol = B.common_volume()
    case = {"vol": vol, "bv": BakedVolume.from_tensor(torch.from_numpy(vol).to(dev), B.C1, B.C2), "rays": {}, "ref": {}}
    for setting, (_, _, step) in B.SETTINGS.items():
        rays = B.common_rays(setting)
        case["rays"][setting] = torch.from_numpy(rays).to(dev)
        for white in (False, True):
            case["ref"][setting, white] = (B.render_ref(rays, vol, B.C1, B.C2, step, white_bkgd=white),
                                           B.render_ref(rays, vol, B.C1, B.C2, step, white_bkgd=white, dtype=np.float32))
    return case


def _np(out):
    return tuple(t.cpu().numpy() for t in (out.rgb, out.depth, out.alpha))


def _equal(a, b):
    return torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.alpha, b.alpha)


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("setting", sorted(B.SETTINGS))
def test_parity_with_the_fp64_restatement(common, setting, white):
    step = B.SETTINGS[setting][2]
    out = common["bv"].render(common["rays"][setting], step=step, white_bkgd=white, skip=False)
    assert out.rgb.dtype == torch.float32 and tuple(out.rgb.shape) == (37, 3) and tuple(out.depth.shape) == tuple(out.alpha.shape) == (37,)
    r64, r32 = common["ref"][setting, white]
    gap, err = B.gaps(r32, r64), B.gaps(_np(out), r64)
    print(f"{setting} white={white}: fp32 - fp64 gap rgb {gap[0]:.3e} depth {gap[1]:.3e} alpha {gap[2]:.3e}; "
          f"kernel - fp64 rgb {err[0]:.3e} depth {err[1]:.3e} alpha {err[2]:.3e}")
    for name, g, e in zip(("rgb", "depth", "alpha"), gap, err):
        assert 0.0 < g < 1e-4, (name, g)
        assert e <= 4.0 * g, (name, e, 4.0 * g)
    got = _np(out)
    bg = 1.0 if white else 0.0
    for r in (26, 27, 28, 29, 36):                                    # the misses and the near >= far ray: exactly the background
        assert (got[0][r] == bg).all() and got[1][r] == 0.0 and got[2][r] == 0.0, r


# ---------------------------------------------------------------- 2. skipping is exact; 5. the same bytes twice

@pytest.mark.parametrize("setting", sorted(B.SETTINGS))
def test_skip_is_exact_and_calls_repeat(ops, common, setting):
    bv, rays, step = common["bv"], common["rays"][setting], B.SETTINGS[setting][2]
    assert bv.skip_threshold == 0.0 and bv.occupancy.dilate == 0 and 0.0 < bv.occupancy.occupied_fraction < 1.0
    for white in (False, True):
        plain = bv.render(rays, step=step, white_bkgd=white, skip=False)
        skipped = bv.render(rays, step=step, white_bkgd=white, skip=True)
        assert _equal(plain, skipped)
        assert _equal(plain, bv.render(rays, step=step, white_bkgd=white, skip=False))      # two calls, the same bytes
        assert _equal(skipped, bv.render(rays, step=step, white_bkgd=white, skip=True))
        rgb, depth, alpha = ops.baked_render(rays, bv.vol, bv.reso, bv.c1, bv.c2, step, bits=torch.zeros_like(bv.occupancy.bits),
                                             white_bkgd=white)
        assert (rgb == (1.0 if white else 0.0)).all() and (depth == 0).all() and (alpha == 0).all()  # nothing occupied: the background
    lead = bv.render(rays.reshape(37, 1, 8), step=step)                 # leading dimensions are kept
    assert tuple(lead.rgb.shape) == (37, 1, 3) and tuple(lead.alpha.shape) == (37, 1)
    assert torch.equal(lead.rgb.reshape(37, 3), bv.render(rays, step=step).rgb)
    default = bv.render(rays)                                           # step=None: the smallest cell edge
    assert _equal(default, bv.render(rays, step=min(bv.cell_size)))


# ---------------------------------------------------------------- 3. termination

def test_termination_stops_and_keeps_its_bound(dev, BakedVolume):
    """25 x 3 x 3 points over [0,24] x [0,2]^2 (h = 1), rays along x with near 0, far 24, step 1/8: n = 192, sample i at
    x = (i + 1/2) / 8.  A wall (sigma on the planes x = 3, 4, 5: step * sum sigma = 3 sigma, T = exp(-3 sigma) ~ 5e-3) inside
    samples 0..63; a bright block (planes x = 19, 20, 21) inside samples 128..191."""
    vol = np.zeros((25, 3, 3, 4), np.float32)
    vol[..., :3] = 0.2
    vol[3:6, :, :, 3] = -np.log(5e-3) / 3.0
    vol[19:22, :, :, :3] = 1.0
    vol[19:22, :, :, 3] = 5.0
    bv = BakedVolume.from_tensor(torch.from_numpy(vol).to(dev), (0.0, 0.0, 0.0), (24.0, 2.0, 2.0))
    far, step, eps = 24.0, 0.125, 1e-2
    rays = torch.tensor([[0.0, y, z, 1.0, 0.0, 0.0, 0.0, far] for y, z in ((1.0, 1.0), (0.3, 1.7), (1.9, 0.2))], device=dev)
    ref = B.render_ref(rays.cpu().numpy(), vol, bv.c1, bv.c2, step)
    assert abs(1.0 - ref[2][0] - 5e-3 * np.exp(-15.0)) < 1e-4            # what is left behind both
    for skip in (False, True):
        plain = bv.render(rays, step=step, skip=skip)
        assert B.gaps(_np(plain), ref)[0] < 1e-5
        assert _equal(plain, bv.render(rays, step=step, skip=skip, terminate=None))
        assert _equal(plain, bv.render(rays, step=step, skip=skip, terminate=0.0))
        assert _equal(plain, bv.render(rays, step=step, skip=skip, terminate=1e-3))   # T ~ 5e-3 > eps behind chunks 0 and 1: no stop
        cut = bv.render(rays, step=step, skip=skip, terminate=eps)
        d_rgb, d_alpha = (cut.rgb - plain.rgb).abs().max(dim=1).values, (cut.alpha - plain.alpha).abs()
        d_depth = (cut.depth - plain.depth).abs()
        print(f"terminate {eps} skip={skip}: max d rgb {float(d_rgb.max()):.3e}, d alpha {float(d_alpha.max()):.3e}, "
              f"d depth {float(d_depth.max()):.3e}")
        assert (d_rgb > 0).all() and (d_rgb <= eps).all()                # every ray really stopped, within the bound
        assert (d_alpha <= eps).all() and (d_depth <= eps * far).all()
        refcut = B.render_ref(rays.cpu().numpy(), vol, bv.c1, bv.c2, step, terminate=eps)
        assert B.gaps(_np(cut), refcut)[0] < 1e-5


# ---------------------------------------------------------------- 4. the camera form is the array form

def test_views_equal_rays_of_the_same_cameras(dev, common):
    from pixelnerf_amd import util
    bv = common["bv"]
    poses = torch.stack([util.pose_spherical(30.0, -25.0, 3.0), util.pose_spherical(-110.0, 10.0, 2.6)]).float().to(dev)
    W, H, focal, c, z_near, z_far = 12, 10, (14.0, 11.5), (5.25, 5.5), 1.0, 4.6
    rays = util.gen_rays(poses, W, H, focal, z_near, z_far, c=c)
    assert tuple(rays.shape) == (2, H, W, 8)
    gt = torch.rand((2, H, W, 3), generator=torch.Generator().manual_seed(3)).to(dev)
    for kw in (dict(), dict(white_bkgd=True, skip=False, step=0.05), dict(terminate=1e-2)):
        views = bv.render_views(poses, W, H, focal, z_near, z_far, c=c, gt_rgb=gt, want_u8=True, **kw)
        arr = bv.render(rays, **kw)
        assert _equal(views, arr), kw
        assert tuple(views.rgb.shape) == (2, H, W, 3) and tuple(views.depth.shape) == tuple(views.alpha.shape) == (2, H, W)
        assert tuple(views.psnr.shape) == tuple(views.ssim.shape) == (2,) and views.psnr.dtype == torch.float64
        assert views.rgb_u8.dtype == torch.uint8 and tuple(views.rgb_u8.shape) == (2, H, W, 3)
        assert float((views.depth_norm - (views.depth - z_near) / (z_far - z_near)).abs().max()) < 1e-6
        assert _equal(views, bv.render_views(poses, W, H, focal, z_near, z_far, c=c, **kw))
    assert float(views.alpha.max()) > 0.5 and float(views.alpha.min()) == 0.0       # the object and the background are both in view
    bare = bv.render_views(poses, W, H, focal, z_near, z_far, c=c)
    assert "psnr" not in bare and "rgb_u8" not in bare


# ---------------------------------------------------------------- 6. baking

def test_baking_through_the_model(ops, dev, BakedVolume):
    from helpers import scene_for
    from test_api_gpu import build_net
    scene, _ = scene_for("sn64")
    net = build_net(dev, scene)
    assert net.use_viewdirs and net.mlp_fine is not None
    c1, c2, reso = (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8), (12, 10, 8)
    net.train()
    with pytest.warns(UserWarning, match="fake view dirs"):
        bv = BakedVolume.from_model(net, c1, c2, reso, eval_batch_size=64)
    assert net.training                                                  # the flag is restored
    net.eval()
    assert tuple(bv.vol.shape) == (12, 10, 8, 4) and bv.reso == reso and bv.vol.is_cuda
    with torch.no_grad():                                                # the same even chunk length, the fine network
        parts = []
        for first in range(0, 960, 64):
            xyz, vd = ops.gen_grid_points(c1, c2, reso, first, 64, device=dev)
            parts.append(net(xyz[None], coarse=False, viewdirs=vd[None])[0])
    assert torch.equal(bv.vol.view(-1, 4), torch.cat(parts))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        whole = BakedVolume.from_model(net, c1, c2, reso, eval_batch_size=100000)
        odd = BakedVolume.from_model(net, c1, c2, reso, eval_batch_size=65)       # rounded down to 64
        coarse = BakedVolume.from_model(net, c1, c2, reso, coarse=True)
    assert torch.equal(whole.vol, bv.vol) and torch.equal(odd.vol, bv.vol) and not torch.equal(coarse.vol, bv.vol)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # a constant direction is not the fake one: no warning
        fixed = BakedVolume.from_model(net, c1, c2, reso, viewdirs=(0.0, -2.0, 0.0))
    assert not torch.equal(fixed.vol, bv.vol)
    with torch.no_grad():
        xyz, _ = ops.gen_grid_points(c1, c2, reso, device=dev, viewdirs=False)
        direct = net(xyz[None], coarse=False, viewdirs=torch.tensor([0.0, -1.0, 0.0], device=dev).expand(960, 3).contiguous()[None])[0]
    assert torch.equal(fixed.vol.view(-1, 4), direct)
    # a round trip through the state renders the same bytes
    rays = torch.from_numpy(B.common_rays("n40")).to(dev)
    state = {k: v.cpu() for k, v in bv.state_dict().items()}
    back = BakedVolume.from_state_dict(state, device=dev)
    assert torch.equal(back.vol, bv.vol) and back.c1 == bv.c1 and back.c2 == bv.c2 and back.skip_threshold == bv.skip_threshold
    assert torch.equal(back.occupancy.bits, bv.occupancy.bits)
    a, b = bv.render(rays, white_bkgd=True), back.render(rays, white_bkgd=True)
    assert _equal(a, b) and float(a.alpha.max()) > 0.0
    net.num_objs = 2
    try:
        with pytest.raises(ValueError, match="encode one object"):
            BakedVolume.from_model(net, c1, c2, reso)
    finally:
        net.num_objs = 1
    bad = bv.vol.clone()
    bad[3, 4, 5, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        BakedVolume.from_tensor(bad, c1, c2)
