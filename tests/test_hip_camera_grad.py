"""
GPU tests (-m gpu) of the gradients with respect to the rays and the cameras (pnr_camera_backward, pnr_composite_backward_far,
pnr_gen_rays_backward): against torch autograd through the UNMODIFIED reference (tests/golden/camera_gradients.npz, frozen by
tools/make_camera_goldens.py: the train/train.py:199-215 loss with a frozen network, the rays, the source cameras' c2w, focal and
c as leaves, and a target camera through util.gen_rays), plus the properties the training path promises: parameter and latent
gradients unchanged when camera gradients are requested as well, bit-reproducible sums, nothing written to a frozen network.
"""
import numpy as np
import pytest
import torch

from helpers import load_golden
from testdata import synthetic

pytestmark = pytest.mark.gpu

SCENARIOS = {  # name: (scene, Kc, Kf, Kfd, rays per object, lindisp)  -- oracle/make_goldens.py SCENARIOS
    "train_64_32": ("train", 64, 32, 16, 32, False),
    "srn_mini_64_128": ("srn_mini", 64, 128, 16, 64, False),
    "dtu_mini_64_128": ("dtu_mini", 64, 128, 16, 64, False),
    "mv_mini_lindisp": ("mv_mini", 32, 16, 0, 32, True),
}
CAMERA_KEYS = ("rays", "c2w", "focal", "c")
# The position gradient runs through the derivative of a bilinear lookup, which jumps at cell edges and at the border clip:
# the reference's own fp32 result differs from the same reference evaluated in fp64 by up to 2.2e-3 on these tensors
# (train_64_32: rays 2.1e-3, c2w 2.2e-3, c 1.5e-3; mv_mini_lindisp: c 1.6e-3).  No fp32 implementation can meet 1e-3 against
# it; the fp32-class bar is set above that spread.
REL_TOL = 5e-3
# 16-bit operands: the rays take the bar of the existing 16-bit gradient tests.  The camera tensors are sums over every sample of
# a view with heavy cancellation (a (1,2) principal-point gradient sums ~10^4 terms of both signs), so the operand rounding shows
# in their MAGNITUDE (measured: train_64_32 c2w 3.1e-2, mv_mini_lindisp c 6.4e-2) while the direction stays (cosine >= 0.9995).
F16_REL_TOL = {"rays": 3e-2, "c2w": 1e-1, "focal": 1e-1, "c": 1e-1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def _setup(dev, name, precision, rays=None, noise=None, trainable=False):
    """the HIP twin of tools/make_camera_goldens.py `run`: -> (net, renderer, rays, noise, leaves dict)"""
    from helpers import mlp_params
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import default_model_conf
    gg = load_golden("camera_gradients")
    scene_name, Kc, Kf, Kfd, n_rays, lindisp = SCENARIOS[name]
    scene, meta = synthetic.make_scene(scene_name, seed=2)
    if rays is None:
        rays = synthetic.target_rays(meta, n_rays=n_rays)
    if noise is None:
        noise = synthetic.make_noise(rays.shape[0] * rays.shape[1], Kc, Kf, Kfd)
    net = make_model(default_model_conf(), precision=precision).to(dev).train()
    net.mlp_coarse.load_state_dict(mlp_params(11))
    net.mlp_fine.load_state_dict(mlp_params(12))
    for p in net.parameters():
        p.requires_grad_(trainable)
    lat = scene["latent"].to(dev).clone().requires_grad_(trainable)
    net.encoder.latent = lat
    ls = torch.tensor([lat.shape[-1], lat.shape[-2]], dtype=torch.float32, device=dev)
    net.encoder.latent_scaling = ls / (ls - 1) * 2.0
    c2w = torch.from_numpy(gg[f"{name}_c2w"]).to(dev).requires_grad_(True)
    focal = torch.from_numpy(gg[f"{name}_focal"]).to(dev).requires_grad_(True)
    c = torch.from_numpy(gg[f"{name}_c"]).to(dev).requires_grad_(True)
    r_wc = c2w[:, :3, :3].transpose(1, 2)  # what PixelNeRFNet.encode derives (models.py:112-141)
    net.poses = torch.cat((r_wc, -(r_wc @ c2w[:, :3, 3:4])), dim=-1)
    net.focal = focal * torch.tensor([1.0, -1.0], device=dev)
    net.c = c
    net.image_shape = scene["image_shape"].to(dev)
    net.num_objs, net.num_views_per_obj = scene["SB"], scene["NS"]
    rend = NeRFRenderer(n_coarse=Kc, n_fine=Kf, n_fine_depth=Kfd, white_bkgd=bool(meta["white_bkgd"]),
                        lindisp=lindisp).to(dev).train()
    rays = rays.to(dev).clone().requires_grad_(True)
    return net, rend, rays, {k: v.to(dev) for k, v in noise.items()}, dict(rays=rays, c2w=c2w, focal=focal, c=c, latent=lat)


def _loss(net, rend, rays, noise, gt):
    out = rend(net, rays, want_weights=True, _noise=noise)
    return ((out.coarse.rgb - gt) ** 2).mean() + ((out.fine.rgb - gt) ** 2).mean()


def camera_grads(dev, name, precision, trainable=False):
    gg = load_golden("camera_gradients")
    net, rend, rays, noise, leaves = _setup(dev, name, precision, trainable=trainable)
    loss = _loss(net, rend, rays, noise, torch.from_numpy(gg[f"{name}_gt"]).to(dev))
    loss.backward()
    return float(loss.item()), net, leaves


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_camera_gradients_match_reference_autograd(dev, name, precision):
    gg = load_golden("camera_gradients")
    loss, _, leaves = camera_grads(dev, name, precision)
    if precision != "f16":
        assert abs(loss - float(gg[f"{name}_loss"])) <= 2e-6 * max(1.0, float(gg[f"{name}_loss"]))
    report = []
    for key in CAMERA_KEYS:
        g = leaves[key].grad
        assert g is not None, f"{name}: no gradient reached {key}"
        got = g.detach().cpu().numpy()
        assert np.isfinite(got).all(), key
        rel, cos = _rel(got, gg[f"{name}_grad_{key}"])
        report.append(f"{key} {rel:.2e}")
        if precision == "f16":
            assert rel <= F16_REL_TOL[key] and cos >= 0.998, f"{name} {key}: rel {rel:.3e} cos {cos:.5f}"
        else:
            assert rel <= REL_TOL, f"{name} {key}: rel {rel:.3e}"
    print(f"{name} {precision}: relative error vs the reference's autograd: " + ", ".join(report))


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_target_pose_gradient_through_gen_rays(dev, precision):
    from pixelnerf_amd import util
    gg = load_golden("camera_gradients")
    name = "srn_mini_64_128"
    W = H = 8
    pose = torch.from_numpy(gg["gen_rays_pose"]).to(dev).requires_grad_(True)
    rays = util.gen_rays(pose, W, H, torch.tensor(8.203125), 0.8, 1.8, c=torch.tensor([4.0, 4.0]))
    assert rays.grad_fn is not None
    Kc, Kf, Kfd = SCENARIOS[name][1:4]
    noise = synthetic.make_noise(W * H, Kc, Kf, Kfd, seed=4321)
    net, rend, _, noise, _ = _setup(dev, name, precision, rays=torch.zeros(1, W * H, 8), noise=noise)
    loss = _loss(net, rend, rays.reshape(1, -1, 8), noise, torch.from_numpy(gg["gen_rays_gt"]).to(dev))
    loss.backward()
    rel, _ = _rel(pose.grad.cpu().numpy(), gg["gen_rays_grad_pose"])
    assert abs(float(loss.item()) - float(gg["gen_rays_loss"])) <= 2e-6
    assert rel <= REL_TOL, rel
    assert not pose.grad[:, 3].any()  # the bottom row of a c2w matrix does not enter gen_rays


def test_gen_rays_backward_matches_torch_autograd(dev):
    from pixelnerf_amd import ops
    gen = torch.Generator().manual_seed(5)
    poses = torch.eye(4).repeat(3, 1, 1)
    poses[:, :3, :4] += 0.3 * torch.randn(3, 3, 4, generator=gen)
    W, H, focal, c = 13, 9, (11.5, 12.25), (6.25, 4.5)
    g = torch.randn(3, H, W, 8, generator=gen)
    p = poses.clone().requires_grad_(True)
    (synthetic.gen_rays(p, W, H, focal, 0.5, 2.0, c=c) * g).sum().backward()
    got = ops.gen_rays_backward(g.to(dev), W, H, focal, c=c).cpu()
    rel = float((got - p.grad).norm() / p.grad.norm())
    assert rel <= 1e-5, rel


def test_all_inputs_trainable_leave_each_gradient_unchanged(dev):
    """parameters + latent + rays + cameras at once: the parameter / latent gradients are those of a run where only they
    require grad, the camera gradients those of the frozen-network run -- bit for bit"""
    gg = load_golden("camera_gradients")
    name = "train_64_32"
    gt = torch.from_numpy(gg[f"{name}_gt"]).to(dev)
    _, _, frozen = camera_grads(dev, name, "f16x3")
    net, rend, rays, noise, leaves = _setup(dev, name, "f16x3", trainable=True)
    _loss(net, rend, rays, noise, gt).backward()
    net_p, rend_p, rays_p, noise_p, leaves_p = _setup(dev, name, "f16x3", trainable=True)
    for k in CAMERA_KEYS:
        leaves_p[k].requires_grad_(False)
    net_p.poses, net_p.focal = net_p.poses.detach(), net_p.focal.detach()
    _loss(net_p, rend_p, rays_p, noise_p, gt).backward()
    for (k, p), (_, q) in zip(net.named_parameters(), net_p.named_parameters()):
        if q.grad is not None or p.grad is not None:
            assert torch.equal(p.grad, q.grad), k
    assert torch.equal(leaves["latent"].grad, leaves_p["latent"].grad)
    for k in CAMERA_KEYS:
        assert torch.equal(leaves[k].grad, frozen[k].grad), k


def test_camera_gradients_are_bit_reproducible(dev):
    _, _, a = camera_grads(dev, "dtu_mini_64_128", "f16x3")
    _, _, b = camera_grads(dev, "dtu_mini_64_128", "f16x3")
    for k in CAMERA_KEYS:
        assert torch.equal(a[k].grad, b[k].grad), k


def test_frozen_network_gets_no_gradient(dev):
    _, net, leaves = camera_grads(dev, "srn_mini_64_128", "f16x3")
    assert all(p.grad is None for p in net.parameters())
    assert net.encoder.latent.grad is None
    assert leaves["rays"].grad is not None
