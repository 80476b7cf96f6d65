#!/usr/bin/env python3
"""
Camera-gradient fixture (tests/golden/camera_gradients.npz) from the UNMODIFIED reference, on the CPU.

Same setup as oracle/make_goldens.py `gradient_goldens` (seeded target, MSE(coarse rgb) + MSE(fine rgb), frozen noise in the
reference's draw order), with the network frozen and the cameras as leaves: `net.poses` is built from a leaf camera-to-world
tensor as src/model/models.py:112-114 builds it, `focal` (fy negated as models.py:129-130 does) and `c` are leaves, and the
rays are a leaf.  Stored per scenario: the full gradients of rays (R,8), c2w (NV,4,4), focal (1,2) and c (1,2), plus the
inputs the tests need to rebuild the run (c2w, focal, c, gt, loss).  One more entry differentiates the target camera through
the reference's util.gen_rays (an 8x8 image of srn_mini).

Usage:  python tools/make_camera_goldens.py      (needs the reference sources: PIXELNERF_REFERENCE, see oracle/make_goldens.py)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from make_goldens import SCENARIOS, SCENE_SEED, _TorchProxy, build_reference_net, set_encode_state  # noqa: E402
from testdata import synthetic  # noqa: E402

CAMERA_SCENARIOS = ("train_64_32", "srn_mini_64_128", "dtu_mini_64_128", "mv_mini_lindisp")
GEN_RAYS = dict(scenario="srn_mini_64_128", W=8, H=8, focal=8.203125, c=(4.0, 4.0))  # one small target image
OUT = os.path.join(ROOT, "tests", "golden", "camera_gradients.npz")


def camera_leaves(meta):
    """(c2w (NV,4,4), focal (1,2), c (1,2)) as leaves, and what encode() derives from them (models.py:112-141)"""
    c2w = meta["src_c2w"].float().clone().requires_grad_(True)
    focal = torch.tensor([meta["focal"]], dtype=torch.float32).requires_grad_(True)
    c = torch.tensor([meta["c"]], dtype=torch.float32).requires_grad_(True)
    rot = c2w[:, :3, :3].transpose(1, 2)
    poses = torch.cat((rot, -torch.bmm(rot, c2w[:, :3, 3:])), dim=-1)
    fl = focal.clone()
    fl[..., 1] *= -1.0
    return c2w, focal, c, poses, fl


def run(name, rays=None, noise=None):
    import render.nerf as ref_nerf

    scene_name, Kc, Kf, Kfd, n_rays, lindisp, use_fine = SCENARIOS[name]
    scene, meta = synthetic.make_scene(scene_name, seed=SCENE_SEED)
    if rays is None:
        rays = synthetic.target_rays(meta, n_rays=n_rays).clone().requires_grad_(True)
    SB, B = rays.shape[:2]
    if noise is None:
        noise = synthetic.make_noise(SB * B, Kc, Kf, Kfd)
    queue = [(kind, noise[k]) for kind, k in (("rand_like", "u1"), ("rand", "u2"), ("rand_like", "u3"), ("randn_like", "n4"))
             if k in noise]
    net = build_reference_net(use_fine).train()
    for p in net.parameters():
        p.requires_grad_(False)
    c2w, focal, c, poses, fl = camera_leaves(meta)
    scene = dict(scene, poses=poses, focal=fl, c=c)
    set_encode_state(net, scene)
    renderer = ref_nerf.NeRFRenderer(n_coarse=Kc, n_fine=Kf, n_fine_depth=Kfd, depth_std=0.01,
                                     white_bkgd=meta["white_bkgd"], lindisp=lindisp, eval_batch_size=50000).train()
    gt = torch.from_numpy(np.random.RandomState(77).uniform(0, 1, (SB, B, 3)).astype(np.float32))
    real_torch = ref_nerf.torch
    ref_nerf.torch = _TorchProxy(queue)
    try:
        out = renderer(net, rays, want_weights=True)
    finally:
        ref_nerf.torch = real_torch
    assert len(queue) == 0
    loss = ((out.coarse.rgb - gt) ** 2).mean() + ((out.fine.rgb - gt) ** 2).mean()
    loss.backward()
    return loss, gt, c2w, focal, c


def main():
    import util as ref_util

    torch.set_num_threads(1)  # one summation order: the file regenerates bit for bit
    rec = {}
    for name in CAMERA_SCENARIOS:
        scene_name, _, _, _, n_rays, _, _ = SCENARIOS[name]
        _, meta = synthetic.make_scene(scene_name, seed=SCENE_SEED)
        rays0 = synthetic.target_rays(meta, n_rays=n_rays).clone().requires_grad_(True)
        loss, gt, c2w, focal, c = run(name, rays=rays0)
        rec[f"{name}_loss"] = np.float64(loss.item())
        rec[f"{name}_gt"] = gt.numpy()
        rec[f"{name}_c2w"] = c2w.detach().numpy()
        rec[f"{name}_focal"] = focal.detach().numpy()
        rec[f"{name}_c"] = c.detach().numpy()
        rec[f"{name}_grad_rays"] = rays0.grad.reshape(-1, 8).numpy()
        rec[f"{name}_grad_c2w"] = c2w.grad.numpy()
        rec[f"{name}_grad_focal"] = focal.grad.numpy()
        rec[f"{name}_grad_c"] = c.grad.numpy()

    # target camera -> util.gen_rays (reference) -> render -> loss
    name, W, H = GEN_RAYS["scenario"], GEN_RAYS["W"], GEN_RAYS["H"]
    scene_name, Kc, Kf, Kfd = SCENARIOS[name][:4]
    _, meta = synthetic.make_scene(scene_name, seed=SCENE_SEED)
    t, p = meta["tgt"]
    tgt = (meta["pre"] @ synthetic.pose_spherical(t, p, meta["radius"]))[None].float().clone().requires_grad_(True)
    rays = ref_util.gen_rays(tgt, W, H, torch.tensor(GEN_RAYS["focal"]), meta["z_near"], meta["z_far"],
                             c=torch.tensor(GEN_RAYS["c"])).reshape(1, -1, 8)
    noise = synthetic.make_noise(W * H, Kc, Kf, Kfd, seed=4321)
    loss, gt, _, _, _ = run(name, rays=rays, noise=noise)
    rec["gen_rays_pose"] = tgt.detach().numpy()
    rec["gen_rays_loss"] = np.float64(loss.item())
    rec["gen_rays_gt"] = gt.numpy()
    rec["gen_rays_grad_pose"] = tgt.grad.numpy()
    np.savez(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
