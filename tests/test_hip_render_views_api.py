"""GPU tests (-m gpu) of the cameras-to-images entry of the public classes: NeRFRenderer.render_views and
_RenderWrapper.render_views (what eval/eval.py:247-331 does per object, as one call).

The pin is an identity, not a tolerance: under the same torch.manual_seed the images equal, bit for bit, forward() over
util.gen_rays of the same cameras -- for the fused network in one call (no ray array) and in groups of views, and for everything
that falls back to the rays (exact fp32, a generic model callable, a composed-path network).  The metrics: PSNR within the 1e-4 dB
the project holds pnr_eval_epilogue to (tests/test_hip_neighbours.py), SSIM within 1e-10 of the fp64 restatement
(tests/test_hip_ssim.py) on the clamped image."""
import warnings

import numpy as np
import pytest
import torch

import ssim_ref
from helpers import scene_for
from testdata import synthetic

pytestmark = pytest.mark.gpu

W, H = 12, 10
FOCAL, C, Z_NEAR, Z_FAR = (22.4, 22.1), (6.0, 5.0), 1.2, 4.0
SAMPLES = dict(n_coarse=16, n_fine=24, n_fine_depth=8)
ANGLES = (20.0, 70.0, 150.0, 290.0, 200.0, 330.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def target_poses(dev, SB, NVt=3):
    p = torch.stack([torch.as_tensor(synthetic.pose_spherical(t, -20.0 - 2.0 * i, 2.732)) for i, t in enumerate(ANGLES[:SB * NVt])])
    return p.reshape(SB, NVt, 4, 4).float().to(dev)


def make(dev, scene_name, precision="f16x3", use_fine=True, **rend_kw):
    from pixelnerf_amd.render import NeRFRenderer
    from test_api_gpu import build_net
    scene, _ = scene_for(scene_name)
    net = build_net(dev, scene, use_fine=use_fine, precision=precision)
    kw = dict(SAMPLES, white_bkgd=True)
    kw.update(rend_kw)
    return net, NeRFRenderer(**kw).to(dev).eval(), target_poses(dev, scene["SB"])


def via_forward(rend, model, poses, seed, noise=None):
    """the identity's right-hand side: the rays of the cameras through forward, as images"""
    from pixelnerf_amd import util
    SB, NVt = poses.shape[:2]
    rays = util.gen_rays(poses.reshape(-1, 4, 4), W, H, FOCAL, Z_NEAR, Z_FAR, C).reshape(SB, -1, 8)
    torch.manual_seed(seed)
    with torch.no_grad():
        out = rend(model, rays, _noise=noise)
    last = out.fine if rend.using_fine else out.coarse
    return last.rgb.reshape(SB, NVt, H, W, 3), last.depth.reshape(SB, NVt, H, W)


def via_views(rend, model, poses, seed, **kw):
    torch.manual_seed(seed)
    return rend.render_views(model, poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C, **kw)


def assert_same_images(out, ref, what=""):
    assert out.rgb.shape == ref[0].shape and out.depth.shape == ref[1].shape, what
    assert torch.equal(out.rgb, ref[0]), f"{what}: rgb differs"
    assert torch.equal(out.depth, ref[1]), f"{what}: depth differs"


@pytest.mark.parametrize("precision", ["f16x3", "f16", "f32"])
@pytest.mark.parametrize("scene_name", ["sn64", "mv_mini"])
def test_render_views_equals_forward_over_the_rays_of_the_cameras(dev, scene_name, precision):
    net, rend, poses = make(dev, scene_name, precision)
    SB, NVt = poses.shape[:2]
    ref = via_forward(rend, net, poses, 21)
    assert torch.isfinite(ref[0]).all() and float(ref[0].std()) > 1e-3  # an image, not a constant
    one = via_views(rend, net, poses, 21)
    assert one.rgb.shape == (SB, NVt, H, W, 3) and one.depth.shape == (SB, NVt, H, W) and one.depth_norm.shape == (SB, NVt, H, W)
    assert "psnr" not in one and "ssim" not in one and "rgb_u8" not in one
    assert_same_images(one, ref, "one call")
    assert torch.allclose(one.depth_norm, (one.depth - Z_NEAR) / (Z_FAR - Z_NEAR), rtol=0, atol=1e-6)  # (bits: test_metrics_...)
    for k in (1, 2):
        assert_same_images(via_views(rend, net, poses, 21, views_per_call=k), ref, f"views_per_call={k}")
    assert not torch.equal(via_views(rend, net, poses, 22).rgb, ref[0])  # another seed, other draws
    # the bound wrapper users hold, in both output forms; grad mode on: it is an inference entry
    for simple in (True, False):
        par = rend.bind_parallel(net, None, simple_output=simple).eval()
        torch.manual_seed(21)
        got = par.render_views(poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C)
        assert_same_images(got, ref, "bind_parallel")
        assert not got.rgb.requires_grad
    if SB == 1:  # (NVt,4,4) poses for a single encoded object
        assert_same_images(via_views(rend, net, poses[0], 21), ref, "3-d poses")
    else:
        with pytest.raises(ValueError):
            via_views(rend, net, poses[0], 21)


@pytest.mark.parametrize("variant", ["no_fine_network", "coarse_only", "explicit_noise", "rng_torch", "lindisp_black", "centre_scalar_focal"])
def test_render_views_identity_under_the_renderer_options(dev, variant):
    use_fine, rend_kw, noise = True, {}, None
    if variant == "no_fine_network":
        use_fine = False                     # eval/eval.py:140: mlp_fine = None, the fine pass re-uses the coarse network
    elif variant == "coarse_only":
        rend_kw = dict(n_fine=0, n_fine_depth=0)   # using_fine is False: the coarse pass's image
    elif variant == "rng_torch":
        rend_kw = dict(rng="torch")
    elif variant == "lindisp_black":
        rend_kw = dict(lindisp=True, white_bkgd=False)
    net, rend, poses = make(dev, "mv_mini", use_fine=use_fine, **rend_kw)
    SB, NVt = poses.shape[:2]
    if variant == "explicit_noise":
        noise = {k: v.to(dev) for k, v in synthetic.make_noise(SB * NVt * H * W, 16, 24, 8, seed=3).items()}
    if variant == "coarse_only":
        assert not rend.using_fine
    if variant == "centre_scalar_focal":  # c=None is the image centre, a scalar focal both axes (util.gen_rays)
        from pixelnerf_amd import util
        rays = util.gen_rays(poses.reshape(-1, 4, 4), W, H, 22.4, Z_NEAR, Z_FAR).reshape(SB, -1, 8)
        torch.manual_seed(4)
        with torch.no_grad():
            f = rend(net, rays).fine
        ref = f.rgb.reshape(SB, NVt, H, W, 3), f.depth.reshape(SB, NVt, H, W)
        for k in (None, 2):
            torch.manual_seed(4)
            assert_same_images(rend.render_views(net, poses, W, H, 22.4, Z_NEAR, Z_FAR, views_per_call=k), ref, f"{variant} k={k}")
        return
    ref = via_forward(rend, net, poses, 4, noise=noise)
    for k in (None, 1, 2):
        assert_same_images(via_views(rend, net, poses, 4, views_per_call=k, _noise=noise), ref, f"{variant} views_per_call={k}")


def test_render_views_around_a_generic_model_callable(dev):
    net, rend, poses = make(dev, "mv_mini")

    class Plain(torch.nn.Module):
        use_viewdirs = True

        def forward(self, xyz, coarse=True, viewdirs=None):
            return net(xyz, coarse=coarse, viewdirs=viewdirs)

    model = Plain()
    ref = via_forward(rend, model, poses, 8)
    assert_same_images(via_views(rend, model, poses, 8), ref, "generic callable")
    assert_same_images(via_views(rend, model, poses, 8, views_per_call=1), ref, "generic callable, views_per_call")


def test_render_views_around_a_composed_path_network(dev):
    from pixelnerf_amd.render import NeRFRenderer
    from test_hip_composed import build_variant
    net = build_variant(dev, "code_viewdirs")[0]   # the reference's default code arrangement, on mv_mini
    assert not net.fused_supported()
    rend = NeRFRenderer(**SAMPLES, white_bkgd=True).to(dev).eval()
    poses = target_poses(dev, 2)
    ref = via_forward(rend, net, poses, 9)
    assert_same_images(via_views(rend, net, poses, 9), ref, "composed path")


@pytest.mark.parametrize("scene_name", ["sn64", "mv_mini"])
def test_metrics_against_ground_truth(dev, scene_name):
    from pixelnerf_amd import ops, util
    net, rend, poses = make(dev, scene_name)
    SB, NVt = poses.shape[:2]
    plain = via_views(rend, net, poses, 13)
    rs = np.random.RandomState(3)
    gt = np.clip(plain.rgb.cpu().numpy().clip(0, 1) + 0.05 * rs.randn(SB, NVt, H, W, 3), 0, 1).astype(np.float32)
    gt_d = torch.from_numpy(gt).to(dev)
    out = via_views(rend, net, poses, 13, gt_rgb=gt_d, want_u8=True, views_per_call=2)
    assert torch.equal(out.rgb, plain.rgb) and torch.equal(out.depth, plain.depth)  # unclamped, as simple_output returns them
    assert out.psnr.shape == (SB, NVt) and out.ssim.shape == (SB, NVt) and out.psnr.dtype == out.ssim.dtype == torch.float64
    assert out.rgb_u8.shape == (SB, NVt, H, W, 3) and out.rgb_u8.dtype == torch.uint8 and out.psnr.is_cuda and out.ssim.is_cuda
    clamped = plain.rgb.clamp(0.0, 1.0).cpu()
    for o in range(SB):
        for v in range(NVt):
            want = util.psnr(clamped[o, v], torch.from_numpy(gt[o, v]))
            got = float(out.psnr[o, v])
            s_want, s_got = ssim_ref.ssim_ref(clamped[o, v].numpy(), gt[o, v]), float(out.ssim[o, v])
            print(f"{scene_name} view ({o},{v}): psnr {got:.6f} dB (util.psnr {want:.6f})  ssim {s_got:.12f} (|diff| {abs(s_got - s_want):.2e})")
            assert abs(got - want) <= 1e-4
            assert abs(s_got - s_want) <= 1e-10
    ep = ops.eval_epilogue(plain.rgb.reshape(SB * NVt, -1, 3), plain.depth.reshape(SB * NVt, -1), Z_NEAR, Z_FAR, gt_rgb=gt_d.reshape(SB * NVt, -1, 3))
    assert torch.equal(out.rgb_u8.reshape(SB * NVt, -1, 3), ep["rgb_u8"])
    assert torch.equal(out.depth_norm.reshape(SB * NVt, -1), ep["depth_norm"])
    assert torch.equal(out.psnr.reshape(-1), ep["psnr"])
    with pytest.raises(ValueError):
        via_views(rend, net, poses, 13, gt_rgb=gt_d[..., :2])


def test_an_automatic_stream_scale_resolves_inside_render_views(dev):
    """the blow-up fixture of tests/test_stream_scale_host.py: the first call of a stream_scale="auto" net saturates, calibrates on
    its own rays and draws and is rendered again -- inside render_views exactly as inside forward"""
    from pixelnerf_amd.render import NeRFRenderer
    from test_hip_stream_scale import blown_net
    scene, _ = scene_for("mv_mini")
    rend = NeRFRenderer(**SAMPLES, white_bkgd=True).to(dev).eval()
    poses = target_poses(dev, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        net = blown_net(dev, scene, stream_scale="auto")
        assert net.stream_scale == "auto"
        out = via_views(rend, net, poses, 17)
        scales = net.stream_scale
        assert isinstance(scales, tuple) and all(isinstance(s, int) and s > 0 for s in scales)
        assert net.__dict__["_auto_syncs"] == 1
        assert_same_images(out, via_forward(rend, net, poses, 17), "auto scale, resolved by render_views")
        assert net.stream_scale == scales and net.__dict__["_auto_syncs"] == 1
        # and the other way round: resolved by forward on the same rays -> the same scales, the same image
        other = blown_net(dev, scene, stream_scale="auto")
        ref = via_forward(rend, other, poses, 17)
        assert other.stream_scale == scales
        assert_same_images(out, ref, "auto scale, resolved by forward")
        assert net._guard_report(wait=True) in (None, (0, 0))
    # in groups of views the first group resolves the scale (on its own rays: the same image where it picks the same scale)
    third = blown_net(dev, scene, stream_scale="auto")
    grouped = via_views(rend, third, poses, 17, views_per_call=1)
    assert third.stream_scale_resolved() and torch.isfinite(grouped.rgb).all()
    if third.stream_scale == scales:
        assert_same_images(grouped, ref, "auto scale, groups")


@pytest.mark.parametrize("rng", ["philox", "torch"])
def test_the_torch_generator_advances_as_for_one_forward(dev, rng):
    net, rend, poses = make(dev, "mv_mini", rng=rng)
    gen = torch.cuda.default_generators[dev.index]
    via_forward(rend, net, poses, 31)
    want = gen.get_offset()
    assert want > 0
    for k in (None, 1):
        via_views(rend, net, poses, 31, views_per_call=k)
        assert gen.get_offset() == want, f"views_per_call={k}"
    noise = {k: v.to(dev) for k, v in synthetic.make_noise(poses.shape[0] * poses.shape[1] * H * W, 16, 24, 8, seed=3).items()}
    via_views(rend, net, poses, 31, _noise=noise)
    assert gen.get_offset() == 0  # explicit draws: the generator is not touched


def test_sharding_wrappers_point_at_forward(dev):
    net, rend, poses = make(dev, "sn64")
    par = rend.bind_parallel(net, [0, 0], simple_output=True).eval()
    with pytest.raises(NotImplementedError, match="forward"):
        par.render_views(poses, W, H, FOCAL, Z_NEAR, Z_FAR)
