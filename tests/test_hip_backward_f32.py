"""
GPU tests (-m gpu) of the fp32-precision training paths -- precision "f32" (pnr_eval_ray_samples_f32_train + pnr_mlp_backward_f32,
every product on the exact fp32 MFMA: the yardstick), "f16x3" in its default FUSED form (pnr_eval_ray_samples_split_train +
pnr_mlp_backward_split: the split-operand inference kernel in its training instantiation, one launch for the transposed
products, one batched split-operand weight-gradient launch) and "f16x3-gemms" (the same arithmetic as one split-operand GEMM
per layer, autograd.FUSED_SPLIT_TRAINING = False): every one of the 61 gradient tensors -- both ResnetFCs and
encoder.latent, including the position gradient through the depth samples (nerf.py:292) -- against the gradients of the
UNMODIFIED reference's own backward (tests/golden/gradients.npz, frozen by oracle/make_goldens.py: train/train.py:199-215
loss, torch autograd through src/render/nerf.py:251-303) at <= 1e-3 relative on the frozen subsample and on the norm.
Scenarios: train_64_32 (4 objects x 32 rays), srn_mini_64_128 (2 source views: pooling backward) and train_cfg5 =
BASELINE configs[4] at FULL size (4 objects x 128 rays, 64 + 32 (16 depth) samples).

It also pins the 16-bit training kernels to this path on the same inputs: the f16 gradients' distance to the fp32-HIP
gradients equals their distance to the reference's (both ~1e-2, the bar is 3e-2) -- i.e. the f16 error is operand
rounding, not a defect that happens to be small.
"""
import numpy as np
import pytest
import torch

from helpers import GRAD_SCENARIOS, grad_setup, load_golden
from testdata import synthetic

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def train_grads(dev, name, precision, loss_scale=1.0):
    from pixelnerf_amd import autograd
    fused = precision != "f16x3-gemms"
    precision = precision.split("-")[0]
    saved, autograd.FUSED_SPLIT_TRAINING = autograd.FUSED_SPLIT_TRAINING, fused
    try:
        return _train_grads(dev, name, precision, loss_scale)
    finally:
        autograd.FUSED_SPLIT_TRAINING = saved


def _train_grads(dev, name, precision, loss_scale=1.0):
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import default_model_conf
    gg = load_golden("gradients")
    g, scene, meta, mc, mf, rays, noise = grad_setup(name)
    Kc, Kf, Kfd = int(g["n_coarse"]), int(g["n_fine"]), int(g["n_fine_depth"])
    gt = torch.from_numpy(gg[f"{name}_gt"])
    net = make_model(default_model_conf(), precision=precision).to(dev).train()
    net.mlp_coarse.load_state_dict(mc)
    net.mlp_fine.load_state_dict(mf)
    lat = scene["latent"].to(dev).clone().requires_grad_(True)
    net.encoder.latent = lat
    ls = torch.tensor([lat.shape[-1], lat.shape[-2]], dtype=torch.float32, device=dev)
    net.encoder.latent_scaling = ls / (ls - 1) * 2.0
    net.poses, net.image_shape = scene["poses"].to(dev), scene["image_shape"].to(dev)
    net.focal, net.c = scene["focal"].to(dev), scene["c"].to(dev)
    net.num_objs, net.num_views_per_obj = scene["SB"], scene["NS"]
    rend = NeRFRenderer(n_coarse=Kc, n_fine=Kf, n_fine_depth=Kfd, white_bkgd=bool(g["white_bkgd"]),
                        lindisp=bool(g["lindisp"])).to(dev).train()
    out = rend(net, rays.to(dev), want_weights=True, _noise={k: v.to(dev) for k, v in noise.items()})
    loss = ((out.coarse.rgb - gt.to(dev)) ** 2).mean() + ((out.fine.rgb - gt.to(dev)) ** 2).mean()
    (loss * loss_scale).backward()
    grads = {"latent": lat.grad}
    grads.update({"coarse." + k: v.grad for k, v in net.mlp_coarse.named_parameters()})
    grads.update({"fine." + k: v.grad for k, v in net.mlp_fine.named_parameters()})
    assert len(grads) == 61
    return float(loss.item()), {k: v.detach().reshape(-1).cpu().numpy() for k, v in grads.items()}, gg


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16x3-gemms"])  # exact fp32 MFMA / split-operand fused / split-operand GEMM per layer
@pytest.mark.parametrize("name", GRAD_SCENARIOS)  # incl. the 3-view ones (README.md:204: DTU trains with 3 views): dtu_mini, train_mv3
def test_fp32_gradients_match_reference_autograd(dev, name, precision):
    loss, grads, gg = train_grads(dev, name, precision)
    ref_loss = float(gg[f"{name}_loss"])
    assert abs(loss - ref_loss) <= 2e-6 * max(1.0, ref_loss), (loss, ref_loss)
    worst = ("", 0.0)
    for key, flat in grads.items():
        assert np.isfinite(flat).all(), key
        ref_s, ref_n = gg[f"{name}_grad_{key}_sample"], float(gg[f"{name}_grad_{key}_norm"])
        got_s = flat[synthetic.grad_sample_index(flat.size, key)]
        e_n = abs(np.linalg.norm(flat.astype(np.float64)) - ref_n) / ref_n
        e_s = np.linalg.norm(got_s.astype(np.float64) - ref_s) / np.linalg.norm(ref_s.astype(np.float64))
        worst = max(worst, (key, max(e_n, e_s)), key=lambda t: t[1])
        assert e_n <= REL_TOL and e_s <= REL_TOL, f"{name} {key}: norm {e_n:.3e} sample {e_s:.3e}"
    print(f"{name} {precision}: worst relative gradient error vs the reference's autograd {worst[1]:.2e} ({worst[0]})")


def test_f16_gradient_error_is_operand_rounding(dev):
    """config 5 at full size: f16 training kernels vs the fp32 HIP path, tensor by tensor -- the same few-1e-3..1e-2 distance
    they have to the reference (bar 3e-2), with cosine >= 0.9995 everywhere"""
    _, g32, _ = train_grads(dev, "train_cfg5", "f32")
    _, g16, _ = train_grads(dev, "train_cfg5", "f16")
    rels = {}
    for k in g32:
        a, b = g16[k].astype(np.float64), g32[k].astype(np.float64)
        rels[k] = np.linalg.norm(a - b) / np.linalg.norm(b)
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert rels[k] <= 3e-2, (k, rels[k])
        assert cos >= 0.9995, (k, cos)
    print("f16 vs fp32-HIP gradients, config 5: max rel %.2e (%s), median %.2e" % (
        max(rels.values()), max(rels, key=rels.get), float(np.median(list(rels.values())))))


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("scene_name,B", [("train", 96), ("mv_mini", 45)])  # 45: ragged; mv_mini: 2 objects x 2 views (pooling)
def test_direct_forward_is_differentiable_at_fp32_precision(dev, scene_name, B, precision):
    """net(xyz, viewdirs) with grad enabled (src/model/models.py:146-266 under autograd) at the fp32-precision paths: outputs and
    the parameter / latent-grid gradients of a random linear functional against torch autograd through the oracle, 1e-3"""
    from helpers import mlp_params, scene_for
    from oracle import pnr_oracle as O
    from test_api_gpu import build_net
    scene, meta = scene_for(scene_name)
    SB = scene["SB"]
    gen = torch.Generator().manual_seed(13)
    xyz = (torch.rand(SB, B, 3, generator=gen) - 0.5) * 1.6
    vd = torch.nn.functional.normalize(torch.randn(SB, B, 3, generator=gen), dim=-1)
    gw = torch.randn(SB, B, 4, generator=gen)
    p = {k: v.clone().requires_grad_(True) for k, v in mlp_params(11).items()}
    sc = dict(scene)
    sc["latent"] = scene["latent"].clone().requires_grad_(True)
    ref = O.pixelnerf_forward(sc, p, xyz, vd)
    (ref * gw).sum().backward()
    net = build_net(dev, scene, precision=precision).train()
    lat = scene["latent"].to(dev).clone().requires_grad_(True)
    net.encoder.latent = lat
    out = net(xyz.to(dev), coarse=True, viewdirs=vd.to(dev))
    assert out.shape == (SB, B, 4) and out.requires_grad
    assert (out.detach().cpu() - ref.detach()).abs().max() <= 2e-5 * max(1.0, float(ref.detach().abs().max()))
    (out * gw.to(dev)).sum().backward()
    pairs = [("latent", lat.grad.cpu(), sc["latent"].grad)]
    pairs += [(k, v.grad.cpu(), p[k].grad) for k, v in net.mlp_coarse.named_parameters()]
    for k, a, b in pairs:
        rel = float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
        assert rel <= 1e-3, f"{k}: rel err {rel:.3e}"


@pytest.mark.parametrize("precision", ["f16x3", "f16x3-gemms"])
def test_split_gradients_follow_the_loss_scale(dev, precision):
    """the split-operand chains run at a power-of-two scale picked on the device (heads and tails are fp16): the gradients of a
    loss scaled by 1e-9 / 1e+9 are the scaled gradients, to rounding -- no underflow of small gradient rows, no overflow of large"""
    _, base, _ = train_grads(dev, "train_64_32", precision)
    for sc in (1e-9, 1e9):
        _, g, _ = train_grads(dev, "train_64_32", precision, loss_scale=sc)
        for k in base:
            a, b = g[k].astype(np.float64) / sc, base[k].astype(np.float64)
            assert np.isfinite(a).all(), (k, sc)
            assert np.linalg.norm(a - b) <= 2e-5 * np.linalg.norm(b) + 1e-30, (k, sc, np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("scene_name,R,K", [("train", 24, 37), ("mv_mini", 10, 45)])  # 888 / 450 points: ragged last tiles; mv_mini: 2 views
def test_fused_split_forward_keeps_the_operands_of_the_gemm_form(dev, scene_name, R, K):
    """What pnr_eval_ray_samples_split_train leaves behind (PnrSplitSaved) against the fp32 activations of the GEMM-per-layer
    forward on the same inputs: every operand image = relu of the saved pre-activation (head + tail, storage order), the lin_in
    operand / interpolated latent pairs, the stream in front of lin_out, the outputs, and the 1-bit relu masks bit for bit where
    the value is clearly away from zero."""
    from helpers import mlp_params, scene_for
    from pixelnerf_amd import ops
    scene, meta = scene_for(scene_name)
    SB, NS = scene["SB"], scene["NS"]
    sc = ops.make_scene(scene["latent"].to(dev), scene["poses"].to(dev), scene["focal"].to(dev), scene["c"].to(dev), scene["image_shape"], NS)
    rays = synthetic.target_rays(meta, n_rays=R).reshape(-1, 8).to(dev)
    z = torch.sort(ops.sample_coarse(rays, torch.rand(rays.shape[0], K, generator=torch.Generator().manual_seed(2)).to(dev)), dim=-1)[0]
    state = {k: v.to(dev) for k, v in mlp_params(11).items()}
    out_g, sv_g = ops.eval_ray_samples_f32_train(sc, ops.pack_mlp(state, "f32"), rays, z, split=True)
    out_f, sv_f = ops.eval_ray_samples_split_train(sc, ops.pack_mlp(state, "f16x3"), ops.fold_latent(sc, state, "f16x3"), rays, z)
    P = rays.shape[0] * K
    assert (out_f - out_g).abs().max() <= 2e-5
    perm = ops.storage_perm(dev)  # storage position e -> feature

    def value(pair):  # (2, rows, cols) f16 [head | tail] -> fp32 value
        return pair[0].float() + pair[1].float()

    def close(a, b, what):
        tol = 4e-6 * max(1.0, float(b.abs().max()))
        assert (a - b).abs().max() <= tol, (what, float((a - b).abs().max()), tol)

    close(value(sv_f.in_op), sv_g.in42, "lin_in operand")
    close(value(sv_f.zlat), sv_g.zlat, "interpolated latent")
    close(sv_f.x5, sv_g.x5, "stream in front of lin_out")
    for b in range(5):
        for img, pre, what in ((sv_f.a[b], sv_g.xin[b], f"relu(x) block {b}"), (sv_f.n[b], sv_g.net[b], f"relu(net) block {b}")):
            nat = torch.empty_like(pre)
            nat[:, perm] = value(img)  # storage order -> feature order
            close(nat, torch.relu(pre), what)
    # masks: the 64-bit words of pnr_device.h, decoded to [layer][view][point][feature] by the stage reference's own reader
    from mlp_bwd_ref import decode_relu_masks
    bits = decode_relu_masks(sv_f.masks, P, NS)
    layers = []
    for b in range(5):
        layers += [sv_g.xin[b], sv_g.net[b]]
    layers.append(sv_g.x5)
    checked = 0
    for li, pre in enumerate(layers):
        per_view = li < 6
        v = pre.cpu().numpy().reshape((NS if per_view else 1), P, 512)
        for view in range(NS if per_view else 1):
            bit, val = bits[li, view], v[view]
            sure = np.abs(val) > 1e-5  # the two forwards differ by rounding: skip values at the threshold
            assert ((bit == 1) == (val > 0))[sure].all(), (li, view)
            checked += int(sure.sum())
    assert checked > 0.9 * 11 * 0.5 * P * 512
