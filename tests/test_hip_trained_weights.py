"""
GPU tests (-m gpu): parity on TRAINED-LIKE weights.  Every frozen fixture of tests/golden uses kaiming-init + N(0, 0.03^2)
networks ("fog": density on 97-99 % of the samples); a drop-in will load trained checkpoints (README.md:55-57 of the
reference), whose weights, hidden-activation magnitudes and densities (thin shells, zero elsewhere) look different.  None
exists offline, so one is MADE here: both ResnetFCs and the feature grid are trained for a few hundred Adam steps on a
procedural scene (testdata/procedural.py: shaded spheres, white background; the reference's objective, train/train.py:199-215)
THROUGH THE HIP PATH ITSELF at the default precision, and then, at those weights,
  * the fp32-class path ("f16x3") is compared with the CPU oracle (oracle/pnr_oracle.py, pinned to the reference) per point and
    per render at the bars of tests/test_hip_split.py -- per-point |rgb| <= 2e-5, sigma rel <= 1e-4; coarse render 2e-5 /
    1e-4 span; fine render PSNR >= 85 dB with <= 2 % of rays allowed a cdf-bin flip -- on BASELINE S2 geometry (1 source view)
    and S3-like geometry (2 source views, pooled), 64 + 128 samples;
  * the config-5 gradient check is repeated: all 61 gradient tensors of the fused fp32-class training step against torch
    autograd through the oracle on the CPU, <= 1e-3 relative per tensor;
  * the fp16-range guard (PnrSplitAux.sat_flag) must stay silent: trained-like activations are inside the fp32-class contract.
"""
import numpy as np
import pytest
import torch

from helpers import assert_close_frac, mlp_params, scene_for
from oracle import pnr_oracle as O
from testdata import procedural, synthetic

pytestmark = pytest.mark.gpu

STEPS = 400


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _install(net, scene, lat, dev):
    net.encoder.latent = lat
    ls = torch.tensor([lat.shape[-1], lat.shape[-2]], dtype=torch.float32, device=dev)
    net.encoder.latent_scaling = ls / (ls - 1) * 2.0
    net.poses, net.image_shape = scene["poses"].to(dev), scene["image_shape"].to(dev)
    net.focal, net.c = scene["focal"].to(dev), scene["c"].to(dev)
    net.num_objs, net.num_views_per_obj = scene["SB"], scene["NS"]


@pytest.fixture(scope="module", params=["train", "train_mv"])
def trained(dev, request):
    """-> dict(name, scene (CPU, with the TRAINED grid), meta, mc, mf (CPU state dicts), pool, targets, losses)"""
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import default_model_conf
    name = request.param
    scene, meta = scene_for(name)
    SB = scene["SB"]
    net = make_model(default_model_conf()).to(dev).train()  # default precision: the fused fp32-class training kernels
    assert net.precision == "f16x3"
    net.mlp_coarse.load_state_dict(mlp_params(11))
    net.mlp_fine.load_state_dict(mlp_params(12))
    # the feature grid starts as a SMOOTH random field (an encoder's output varies slowly across the image; the white-noise grid of
    # the golden fixtures gives every sample an unrelated feature vector, which nothing can be fitted to in a few hundred steps)
    rs = np.random.RandomState(5)
    low = torch.from_numpy(rs.randn(scene["latent"].shape[0], 512, 4, 4).astype(np.float32))
    lat0 = torch.nn.functional.interpolate(low, size=tuple(scene["latent"].shape[-2:]), mode="bilinear", align_corners=True) * 0.5
    lat = lat0.to(dev).clone().requires_grad_(True)
    _install(net, scene, lat, dev)
    # three target views per object, all pixels; ground truth from the analytic spheres
    pools = []
    for o in range(SB):
        poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 40.0 * o + dt, meta["tgt"][1] + dp, meta["radius"])
                             for dt, dp in ((0.0, 0.0), (55.0, -10.0), (-70.0, 8.0))])
        pools.append(synthetic.gen_rays(poses, meta["W"], meta["H"], meta["focal"], meta["z_near"], meta["z_far"], c=meta["c"]).reshape(-1, 8))
    pool = torch.stack(pools).to(dev)
    centres, radii, tints = procedural.sphere_params(SB, seed=4)
    targets = procedural.sphere_targets(pool, centres, radii, tints)
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).to(dev).train()
    torch.manual_seed(7)
    losses = procedural.fit(net, rend, lat, pool, targets, steps=STEPS, rays_per_obj=128, lr=5e-4, seed=1)
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print(f"trained-like weights [{name}]: {STEPS} Adam steps through the HIP path, loss {first:.4f} -> {last:.4f}")
    assert np.isfinite(losses).all() and last < 0.7 * first, (first, last)
    assert net._guard_report(wait=True) in (None, (0, 0))
    sc = dict(scene)
    sc["latent"] = lat.detach().cpu().clone()
    sc["latent_init"] = lat0
    mc = {k: v.detach().cpu().clone() for k, v in net.mlp_coarse.state_dict().items()}
    mf = {k: v.detach().cpu().clone() for k, v in net.mlp_fine.state_dict().items()}
    del net, rend
    torch.cuda.empty_cache()
    return dict(name=name, scene=sc, meta=meta, mc=mc, mf=mf, pool=pool.cpu(), targets=targets.cpu(), losses=losses)


@pytest.mark.parametrize("name", ["train", "train_mv"])
def test_training_through_the_hip_path_is_bit_reproducible(dev, name):
    """Two runs of the same 12 Adam steps (both ResnetFCs + the feature grid, default precision, the renderer's own torch draws
    under one seed) end in the SAME bits: weight gradients are fixed-order split-K reductions, the grid gradient comes out of the
    LDS-slab scatter with at most two commuting adds per element (pnr_scatter.hip latent_scatter_owner_kernel; autograd.py keeps one
    zeroed buffer per pass).  This is what makes the trained-weights fixture above the same network on every run."""
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import default_model_conf
    scene, meta = scene_for(name)
    poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 40.0 * o, meta["tgt"][1], meta["radius"]) for o in range(scene["SB"])])
    pool = synthetic.gen_rays(poses, meta["W"], meta["H"], meta["focal"], meta["z_near"], meta["z_far"], c=meta["c"]).reshape(scene["SB"], -1, 8).to(dev)
    centres, radii, tints = procedural.sphere_params(scene["SB"], seed=4)
    targets = procedural.sphere_targets(pool, centres, radii, tints)

    def run():
        net = make_model(default_model_conf()).to(dev).train()
        net.mlp_coarse.load_state_dict(mlp_params(11))
        net.mlp_fine.load_state_dict(mlp_params(12))
        lat = scene["latent"].to(dev).clone().requires_grad_(True)
        _install(net, scene, lat, dev)
        rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).to(dev).train()
        torch.manual_seed(7)
        losses = procedural.fit(net, rend, lat, pool, targets, steps=12, rays_per_obj=128, lr=5e-4, seed=1)
        state = [p.detach().clone() for p in list(net.mlp_coarse.parameters()) + list(net.mlp_fine.parameters())] + [lat.detach().clone()]
        return losses, state

    l1, s1 = run()
    l2, s2 = run()
    assert l1 == l2, (l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(s1, s2))
    assert not torch.equal(s1[-1], scene["latent"].to(dev))  # the grid did move


def _object_scene(tr, obj=0):
    """the trained scene restricted to ONE object: S2 geometry for `train` (1 source view), S3-like for `train_mv` (2 views)"""
    s = tr["scene"]
    NS = s["NS"]
    return dict(latent=s["latent"][obj * NS:(obj + 1) * NS].contiguous(), poses=s["poses"][obj * NS:(obj + 1) * NS].contiguous(),
                focal=s["focal"], c=s["c"], image_shape=s["image_shape"], NS=NS, SB=1)


def _eval_net(dev, tr, scene1, precision="f16x3"):
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.util.conf import default_model_conf
    net = make_model(default_model_conf(), precision=precision).to(dev).eval()
    net.mlp_coarse.load_state_dict(tr["mc"])
    net.mlp_fine.load_state_dict(tr["mf"])
    _install(net, scene1, scene1["latent"].to(dev), dev)
    return net


def test_trained_weights_are_not_init_like(trained):
    """what 'trained-like' means here, printed for the record: weights moved by a sizeable fraction of their init scale, and the
    density went from fog to mostly-empty space with a shell"""
    tr = trained
    rel = {k: float((tr["mc"][k] - mlp_params(11)[k]).norm() / mlp_params(11)[k].norm()) for k in tr["mc"] if k.endswith("weight")}
    scene1 = _object_scene(tr)
    rays = tr["pool"][0, :4096:16]
    z = O.sample_coarse(rays, torch.full((rays.shape[0], 64), 0.5), 64)
    pts = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(1, -1, 3)
    vd = rays[:, None, 3:6].expand(-1, 64, -1).reshape(1, -1, 3)
    with torch.no_grad():
        sig_tr = O.pixelnerf_forward(scene1, tr["mc"], pts, vd)[..., 3]
        sig_in = O.pixelnerf_forward(dict(scene1, latent=tr["scene"]["latent_init"][:scene1["NS"]]), mlp_params(11), pts, vd)[..., 3]
    print(f"[{tr['name']}] relative weight change per tensor: min {min(rel.values()):.2f} median {float(np.median(list(rel.values()))):.2f} "
          f"max {max(rel.values()):.2f}; zero-density samples {float((sig_in <= 0).float().mean()):.2f} (init) -> "
          f"{float((sig_tr <= 0).float().mean()):.2f} (trained); max sigma {float(sig_in.max()):.1f} -> {float(sig_tr.max()):.1f}")
    assert float(np.median(list(rel.values()))) > 0.05


def test_per_point_parity_at_trained_weights(dev, trained):
    from pixelnerf_amd import ops
    tr = trained
    scene1 = _object_scene(tr)
    gen = torch.Generator().manual_seed(3)
    rays = tr["pool"][0][torch.randperm(tr["pool"].shape[1], generator=gen)[:64]]
    z = O.sample_coarse(rays, torch.rand(64, 48, generator=gen), 48)
    pts = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(1, -1, 3).contiguous()
    vd = rays[:, None, 3:6].expand(-1, 48, -1).reshape(1, -1, 3).contiguous()
    net = _eval_net(dev, tr, scene1)
    for coarse, p in ((True, tr["mc"]), (False, tr["mf"])):
        with torch.no_grad():
            ref = O.pixelnerf_forward(scene1, p, pts, vd)
            got = net(pts.to(dev), coarse=coarse, viewdirs=vd.to(dev)).cpu()
        e_rgb = float((got[..., :3] - ref[..., :3]).abs().max())
        e_s = float(((got[..., 3] - ref[..., 3]).abs() / ref[..., 3].clamp(min=1.0)).max())
        print(f"[{tr['name']}] f16x3 per point at trained weights ({'coarse' if coarse else 'fine'} net): rgb max err {e_rgb:.2e}, "
              f"sigma rel err {e_s:.2e} (max sigma {float(ref[..., 3].max()):.1f})")
        assert e_rgb <= 2e-5 and e_s <= 1e-4
    assert net._guard_report(wait=True) in (None, (0, 0))


def test_render_parity_at_trained_weights(dev, trained):
    from pixelnerf_amd.render import NeRFRenderer
    tr = trained
    scene1 = _object_scene(tr)
    gen = torch.Generator().manual_seed(5)
    R = 160
    rays = tr["pool"][0][torch.randperm(4096, generator=gen)[:R]]  # pixels of the first target view: object, silhouette, background
    noise = synthetic.make_noise(R, 64, 128, 16, seed=77)
    with torch.no_grad():
        ref = O.render(scene1, tr["mc"], tr["mf"], rays[None], noise, 64, 128, 16, white_bkgd=True)
    net = _eval_net(dev, tr, scene1)
    rend = NeRFRenderer(n_coarse=64, n_fine=128, n_fine_depth=16, white_bkgd=True).to(dev).eval()
    with torch.no_grad():
        out = rend(net, rays[None].to(dev), want_weights=True, _noise={k: v.to(dev) for k, v in noise.items()})
    span = float(tr["meta"]["z_far"] - tr["meta"]["z_near"])
    for p in ("coarse", "fine"):
        flips = 0.0 if p == "coarse" else 2e-2
        rgb = out[p].rgb.cpu().reshape(-1, 3)
        assert_close_frac(rgb.numpy(), ref[p]["rgb"].reshape(-1, 3).numpy(), 2e-5, max_frac=flips, loose_atol=0.05, what=f"{p} rgb")
        assert_close_frac(out[p].depth.cpu().reshape(-1).numpy(), ref[p]["depth"].reshape(-1).numpy(), 1e-4 * span, max_frac=flips,
                          loose_atol=0.05 * span, what=f"{p} depth")
        if p == "coarse":
            np.testing.assert_allclose(out[p].weights.cpu().reshape(R, -1).numpy(), ref[p]["weights"].reshape(R, -1).numpy(), rtol=0, atol=2e-5)
        ps = O.psnr(rgb, ref[p]["rgb"].reshape(-1, 3))
        print(f"[{tr['name']}] f16x3 render at trained weights, {p}: PSNR {ps:.1f} dB vs the CPU oracle "
              f"(weight of the heaviest sample: median {float(ref[p]['weights'].max(-1)[0].median()):.2f})")
        assert ps >= 85.0
    assert net._guard_report(wait=True) in (None, (0, 0))


def test_gradient_parity_at_trained_weights(dev, trained):
    """BASELINE config 5's step (64 + 32 (16 depth) samples, MSE coarse + MSE fine) at the trained weights: the fused fp32-class
    training kernels against torch autograd through the oracle, tensor by tensor"""
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import default_model_conf
    tr = trained
    scene = tr["scene"]
    SB, B = scene["SB"], 24
    gen = torch.Generator().manual_seed(9)
    idx = torch.randint(0, tr["pool"].shape[1], (SB, B), generator=gen)
    rays = torch.gather(tr["pool"], 1, idx.unsqueeze(-1).expand(-1, -1, 8))
    gt = torch.gather(tr["targets"], 1, idx.unsqueeze(-1).expand(-1, -1, 3))
    noise = synthetic.make_noise(SB * B, 64, 32, 16, seed=31)
    # CPU: torch autograd through the oracle
    pc = {k: v.clone().requires_grad_(True) for k, v in tr["mc"].items()}
    pf = {k: v.clone().requires_grad_(True) for k, v in tr["mf"].items()}
    sc = dict(scene)
    sc["latent"] = scene["latent"].clone().requires_grad_(True)
    # HIP
    net = make_model(default_model_conf()).to(dev).train()
    net.mlp_coarse.load_state_dict(tr["mc"])
    net.mlp_fine.load_state_dict(tr["mf"])
    lat = scene["latent"].to(dev).clone().requires_grad_(True)
    _install(net, scene, lat, dev)
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).to(dev).train()
    out = rend(net, rays.to(dev), want_weights=True, _noise={k: v.to(dev) for k, v in noise.items()})
    # the importance samples are a discontinuous function of the (detached) coarse weights, and trained densities are sharp: the
    # CPU side draws them from the HIP path's coarse weights, so a 1-ulp difference cannot put a sample -- and its share of the
    # grid gradient -- into the neighbouring bin on one side only (one run without this measured 5.7e-3 on the latent gradient of
    # the two-view scene, 1e-4 elsewhere; the diagnostic below counts the samples the oracle's own weights would move)
    ref = O.render(sc, pc, pf, rays, noise, 64, 32, 16, white_bkgd=True,
                   sampling_weights=out.coarse.weights.detach().cpu().reshape(SB * B, 64))
    ref_loss = ((ref["coarse"]["rgb"] - gt) ** 2).mean() + ((ref["fine"]["rgb"] - gt) ** 2).mean()
    ref_loss.backward()
    with torch.no_grad():  # for the record: how many fine samples the oracle places elsewhere when it samples from its OWN weights
        own = O.render(sc, pc, pf, rays, noise, 64, 32, 16, white_bkgd=True)
        moved = (own["fine"]["z"].reshape(SB * B, -1) - ref["fine"]["z"].detach().reshape(SB * B, -1)).abs() > 1e-4
        print(f"[{tr['name']}] fine samples that land in another cdf bin with the oracle's own coarse weights: {int(moved.sum())} of {moved.numel()} "
              f"(max |w_hip - w_oracle| = {float((out.coarse.weights.detach().cpu().reshape(SB * B, 64) - own['coarse']['weights'].reshape(SB * B, 64)).abs().max()):.1e})")
    loss = ((out.coarse.rgb - gt.to(dev)) ** 2).mean() + ((out.fine.rgb - gt.to(dev)) ** 2).mean()
    loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 5e-6 * max(1.0, float(ref_loss)), (float(loss), float(ref_loss))
    pairs = [("latent", lat.grad.cpu(), sc["latent"].grad)]
    pairs += [("coarse." + k, v.grad.cpu(), pc[k].grad) for k, v in net.mlp_coarse.named_parameters()]
    pairs += [("fine." + k, v.grad.cpu(), pf[k].grad) for k, v in net.mlp_fine.named_parameters()]
    assert len(pairs) == 61
    worst = ("", 0.0)
    for k, a, b in pairs:
        rel = float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
        worst = max(worst, (k, rel), key=lambda t: t[1])
        assert rel <= 1e-3, f"{k}: relative gradient error {rel:.3e}"
    print(f"[{tr['name']}] f16x3 gradients at trained weights: worst tensor {worst[1]:.2e} ({worst[0]}), loss {float(loss):.5f}")
