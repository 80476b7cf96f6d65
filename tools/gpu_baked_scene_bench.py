#!/usr/bin/env python3
"""Scenes of several baked volumes on a trained-like object, on the GPU box: prints the table that goes into profiles/baked_notes.md
and one JSON line.

The object is the one tools/gpu_baked_bench.py bakes (procedural spheres, 400 Adam steps through the HIP path, scene "train", object
0), as an RGBA volume and as a degree-2 coefficient volume at 128^3 over [-1,1]^3, each in fp32 and in fp16.  N = 1, 2, 4, 8 copies
of it -- the SAME stored tensor under N poses: nothing is copied -- stand on a ring in the horizontal plane, copy j turned by
360 j / N degrees about the vertical (z) axis and moved to radius 1.5 / sin(pi / N), which keeps the turned boxes disjoint; N = 1 is
the object at the identity.  8 views of 128 x 128 look at the ring's centre from radius 9 (so every N has the same rays and the same
number of samples per ray), white background, step = the cell edge, skip on.

Per row the scene call (BakedScene.render_views: ONE launch) is timed against the SUM of the N single-volume render_views calls of
the same process, each with the cameras moved into its object's frame (inverse(object pose) @ camera pose: the same rays as that
object sees them).  Those entries are the parent commit's: they are the baseline.  The N images of the singles cannot be merged into
the scene's image; the sum says what the same loads cost without the object loop.

Timing: after warm-up the scene call and the N single calls ALTERNATE in one process, every call between two device events ended by a
device synchronise; (median, min) of REPS."""
import argparse
import json
import math
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_occupancy_bench import C1, C2, H, NVT, W, stats, timed, trained_object  # noqa: E402
from pixelnerf_amd.util.bake import BakedScene, BakedSHVolume, BakedVolume  # noqa: E402
from testdata import synthetic  # noqa: E402

REPS, WARMUP = 10, 2
CAM_RADIUS, Z_NEAR, Z_FAR, FOCAL = 9.0, 3.4, 14.6, 110.0


def ring_poses(n):
    """(n,4,4) object-to-world: copy j turned by 360 j / n degrees about z and moved out to the ring; n = 1: the identity"""
    poses = torch.eye(4).repeat(n, 1, 1)
    if n == 1:
        return poses
    radius = 1.5 / math.sin(math.pi / n)
    for j in range(n):
        a = 2.0 * math.pi * j / n
        poses[j, :3, :3] = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        poses[j, :3, 3] = torch.tensor([radius * math.cos(a), radius * math.sin(a), 0.0])
    return poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reso", type=int, default=128)
    ap.add_argument("--n-dirs", type=int, default=32)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 2, 4, 8])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake)
    net, meta, losses = trained_object(dev, args.steps)
    reso = [args.reso] * 3
    cams = torch.stack([synthetic.pose_spherical(45.0 * i, -20.0 - 3.0 * i, CAM_RADIUS) for i in range(NVT)]).float().to(dev)
    cam = (W, H, FOCAL, Z_NEAR, Z_FAR)
    rgba = BakedVolume.from_model(net, C1, C2, reso)
    sh2 = BakedSHVolume.from_model(net, C1, C2, reso, degree=2, n_dirs=args.n_dirs)
    volumes = {"rgba fp32": rgba, "rgba fp16": rgba.half(), "degree 2 fp32": sh2, "degree 2 fp16": sh2.half()}
    out = {"views": NVT, "image": [H, W], "reso": args.reso, "reps": REPS, "train_steps": args.steps, "loss_last10": float(sum(losses[-10:]) / 10),
           "camera": {"radius": CAM_RADIUS, "z": [Z_NEAR, Z_FAR], "focal": FOCAL}, "step": round(min(rgba.cell_size), 5),
           "samples_per_ray": math.ceil((Z_FAR - Z_NEAR) / min(rgba.cell_size)), "occupied_fraction": round(rgba.occupancy.occupied_fraction, 5),
           "rows": {}}
    for kind, vol in volumes.items():
        for n in args.counts:
            poses = ring_poses(n)
            scene = BakedScene([vol] * n, poses)
            local = [(torch.linalg.inv(poses[j].double()).float().to(dev) @ cams).contiguous() for j in range(n)]   # the cameras as object j sees them
            render_scene = lambda: scene.render_views(cams, *cam, white_bkgd=True)
            render_single = lambda j: vol.render_views(local[j], *cam, white_bkgd=True)
            img = render_scene()
            row = {"coverage": round(float((img.alpha > 0.5).float().mean()), 4)}
            if n == 1:
                one = render_single(0)
                row["bytes_of_the_single_entry"] = bool(torch.equal(img.rgb, one.rgb) and torch.equal(img.depth, one.depth))
            t_scene, t_sum = [], []
            for i in range(REPS + WARMUP):
                a = timed(render_scene)[0]
                b = sum(timed(lambda: render_single(j))[0] for j in range(n))
                if i >= WARMUP:
                    t_scene.append(a), t_sum.append(b)
            row["scene_ms"], row["singles_sum_ms"] = stats(t_scene), stats(t_sum)
            row["scene_over_sum"] = round(row["scene_ms"][0] / row["singles_sum_ms"][0], 3)
            out["rows"][f"{kind} N={n}"] = row
            del scene, img
        torch.cuda.empty_cache()

    print(f"scenes of baked volumes, trained-like object (scene train, {args.steps} steps, loss -> {out['loss_last10']:.4f}), {args.reso}^3, "
          f"occupied fraction {out['occupied_fraction']}; {NVT} views {H}x{W} from radius {CAM_RADIUS}, z in [{Z_NEAR}, {Z_FAR}], step "
          f"{out['step']} ({out['samples_per_ray']} samples per ray), skip on, white background; (median, min) of {REPS}")
    cols = ["coverage", "scene_ms", "singles_sum_ms", "scene_over_sum"]
    print("| volume, N | " + " | ".join(cols) + " |")
    print("|" + "---|" * (len(cols) + 1))
    for name, row in out["rows"].items():
        print(f"| {name} | " + " | ".join(str(row[c]) for c in cols) + " |")
    print("N = 1 renders the bytes of the single entry: " + str(all(r["bytes_of_the_single_entry"] for k, r in out["rows"].items() if k.endswith("N=1"))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
