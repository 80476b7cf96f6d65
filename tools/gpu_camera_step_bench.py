#!/usr/bin/env python3
"""One training / pose-refinement step at BASELINE config (5) shapes (sn64-style `train` scene, 4 objects x 128 rays,
64 coarse + 32 fine (16 depth), precision f16x3), forward + backward, in three variants:
  (a) trainable network (+ latent), as train/train.py does;
  (b) frozen network, trainable target pose: util.gen_rays(pose) -> rays of 128 pixels per object -> render -> MSE;
  (c) frozen network, trainable source poses (camera-to-world, through encode's w2c) + focal.
Prints one JSON line per variant (median of timed steps, ms) and writes them to --out when given."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from testdata import synthetic  # noqa: E402
from pixelnerf_amd import util  # noqa: E402
from pixelnerf_amd.model import make_model  # noqa: E402
from pixelnerf_amd.render import NeRFRenderer  # noqa: E402
from pixelnerf_amd.util.conf import default_model_conf  # noqa: E402


def setup(dev, variant):
    scene, meta = synthetic.make_scene("train")
    net = make_model(default_model_conf(), precision="f16x3").to(dev).train()
    net.mlp_coarse.load_state_dict(synthetic.make_mlp_params(11))
    net.mlp_fine.load_state_dict(synthetic.make_mlp_params(12))
    trainable = variant == "a"
    for p in net.parameters():
        p.requires_grad_(trainable)
    lat = scene["latent"].to(dev).clone().requires_grad_(trainable)
    net.encoder.latent = lat
    ls = torch.tensor([32.0, 32.0], device=dev)
    net.encoder.latent_scaling = ls / (ls - 1) * 2.0
    net.image_shape = scene["image_shape"].to(dev)
    net.num_objs, net.num_views_per_obj = scene["SB"], scene["NS"]
    c2w = meta["src_c2w"].float().to(dev).requires_grad_(variant == "c")
    focal = scene["focal"].to(dev).clone().requires_grad_(variant == "c")
    leaves = [lat] + list(net.parameters()) if trainable else ([c2w, focal] if variant == "c" else [])

    def encode_cameras():
        r_wc = c2w[:, :3, :3].transpose(1, 2)
        net.poses = torch.cat((r_wc, -(r_wc @ c2w[:, :3, 3:4])), dim=-1)
        net.focal, net.c = focal, scene["c"].to(dev)

    # target cameras: one per object (as synthetic.target_rays), 128 pixels each
    tgt = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 40.0 * o, meta["tgt"][1], meta["radius"])
                       for o in range(4)]).float().to(dev).requires_grad_(variant == "b")
    if variant == "b":
        leaves = [tgt]
    pix = torch.randperm(meta["W"] * meta["H"], generator=torch.Generator().manual_seed(3))[:128].to(dev)

    def rays():
        r = util.gen_rays(tgt, meta["W"], meta["H"], torch.tensor(meta["focal"]), meta["z_near"], meta["z_far"],
                          c=torch.tensor(meta["c"]))
        return r.reshape(4, -1, 8)[:, pix]

    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).to(dev).train()
    gt = torch.rand(4, 128, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(9))

    def step():
        encode_cameras()
        out = rend(net, rays())
        loss = ((out.coarse.rgb - gt) ** 2).mean() + ((out.fine.rgb - gt) ** 2).mean()
        for t in leaves:
            t.grad = None
        loss.backward()
        return loss

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    names = {"a": "trainable network", "b": "frozen network, trainable target pose",
             "c": "frozen network, trainable source poses + focal"}
    rows = []
    for v in ("a", "b", "c"):
        step = setup(dev, v)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        row = dict(variant=v, what=names[v], step_ms_median=round(statistics.median(ts), 3), step_ms_min=round(min(ts), 3),
                   steps=a.steps, shape="4 objects x 128 rays, 64+32(16), f16x3", device=torch.cuda.get_device_name(0))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
