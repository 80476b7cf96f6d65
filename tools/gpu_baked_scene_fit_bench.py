#!/usr/bin/env python3
"""Stored-value gradients of the scene march on a trained-like object, on the GPU box: prints the tables that go into
profiles/baked_notes.md ("Scene fitting") and one JSON line per part.

The scenes are those of tools/gpu_baked_scene_bench.py: N = 1, 2, 4, 8 copies of the 128^3 object on its ring, 8 views of 128 x 128
from radius 9, white background, step = the cell edge, skip on; RGBA and degree 2, fp32.  Every object is a tensor of its OWN (a
clone: N buffers, as a fit of N different objects has).  Upstream gradients: d_rgb = the image itself.

  cost   per row, alternating in one process after warm-up, each call between two device events:
           scene_fwd     BakedScene.render_views
           scene_stored  ops.baked_scene_stored_backward_views into N zeroed buffers (the zeroing is timed with it, as in a fit)
           singles_sum   the N ops.baked_render_views_backward calls it replaces, each with the cameras moved into its object's frame
                         (at N = 1: the single entry itself; beyond, they are NOT this gradient: the objects do not see each other)
         N = 1 also reports the largest difference to the single entry's gradient, relative to its largest element.
  fit    one step of util.bake.fit_scene: 2 objects of the ring, 4 views of 64 x 64 as rays, batch 4096; (total time of 20 steps
         after 5) / 20.

Run without --part, the tool is a driver: it starts each part as a child process of its own under its own time limit and stops at
the first that fails or runs out of time.  A part uses at most 16 CPU threads."""
import argparse
import json
import os
import subprocess
import sys
import warnings

PARTS = {"cost": 600, "fit": 300}   # seconds allowed per part


def driver(args):
    for part, limit in PARTS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--steps", str(args.steps), "--reso", str(args.reso)]
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"part {part}: ran out of its {limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"part {part}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=sorted(PARTS), default=None)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reso", type=int, default=128)
    ap.add_argument("--n-dirs", type=int, default=32)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 2, 4, 8])
    args = ap.parse_args()
    if args.part is None:
        sys.exit(driver(args))

    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    from gpu_baked_scene_bench import CAM_RADIUS, FOCAL, Z_FAR, Z_NEAR, ring_poses
    from gpu_occupancy_bench import C1, C2, H, NVT, W, stats, timed, trained_object
    from pixelnerf_amd import ops
    from pixelnerf_amd.util import bake
    from testdata import synthetic

    REPS, WARMUP = 10, 2
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake)
    net, meta, losses = trained_object(dev, args.steps)
    reso = [args.reso] * 3
    rgba = bake.BakedVolume.from_model(net, C1, C2, reso)
    out = {"part": args.part, "reso": args.reso, "reps": REPS, "train_steps": args.steps, "step": round(min(rgba.cell_size), 5), "rows": {}}

    if args.part == "cost":
        cams = torch.stack([synthetic.pose_spherical(45.0 * i, -20.0 - 3.0 * i, CAM_RADIUS) for i in range(NVT)]).float().to(dev)
        cam = (W, H, FOCAL, Z_NEAR, Z_FAR)
        sh2 = bake.BakedSHVolume.from_model(net, C1, C2, reso, degree=2, n_dirs=args.n_dirs)
        step = min(rgba.cell_size)
        for kind, vol in {"rgba": rgba, "degree 2": sh2}.items():
            for n in args.counts:
                poses = ring_poses(n)
                scene = bake.BakedScene([vol._around(vol._stored().clone()) for _ in range(n)], poses)
                objects = scene._objects(True)
                local = [(torch.linalg.inv(poses[j].double()).float().to(dev) @ cams).contiguous() for j in range(n)]
                d_rgb = scene.render_views(cams, *cam, white_bkgd=True).rgb.reshape(-1, 3).contiguous()
                buffers = [torch.empty_like(ob[0]) for ob in objects]

                def scene_stored():
                    for b in buffers:
                        b.zero_()
                    return ops.baked_scene_stored_backward_views(cams, W, H, FOCAL, None, Z_NEAR, Z_FAR, objects, step, d_rgb=d_rgb,
                                                                 white_bkgd=True, out=buffers)

                def single(j):
                    buffers[j].zero_()
                    v = scene.volumes[j]
                    return ops.baked_render_views_backward(local[j], W, H, FOCAL, None, Z_NEAR, Z_FAR, v._stored(), v.degree, v.reso, v.c1, v.c2,
                                                           step, d_rgb=d_rgb, bits=v.occupancy.bits, white_bkgd=True, out=buffers[j])

                scene_fwd = lambda: scene.render_views(cams, *cam, white_bkgd=True)
                got = [g.clone() for g in scene_stored()]
                row = {"touched": round(float(sum(int((g != 0).sum()) for g in got)) / sum(g.numel() for g in got), 4)}
                if n == 1:
                    one = single(0)
                    row["gap_to_single"] = float((got[0] - one).abs().max() / one.abs().max())
                t = {"scene_fwd": [], "scene_stored": [], "singles_sum": []}
                for i in range(REPS + WARMUP):
                    a = timed(scene_fwd)[0]
                    b = timed(scene_stored)[0]
                    c = sum(timed(lambda: single(j))[0] for j in range(n))
                    if i >= WARMUP:
                        t["scene_fwd"].append(a), t["scene_stored"].append(b), t["singles_sum"].append(c)
                for k, v in t.items():
                    row[k + "_ms"] = stats(v)
                row["stored_over_singles"] = round(row["scene_stored_ms"][0] / row["singles_sum_ms"][0], 3)
                row["stored_over_fwd"] = round(row["scene_stored_ms"][0] / row["scene_fwd_ms"][0], 3)
                out["rows"][f"{kind} N={n}"] = row
                del scene, got, buffers, objects
                torch.cuda.empty_cache()
        print(f"scene fitting, trained-like object ({args.steps} steps), {args.reso}^3; {NVT} views {H}x{W} from radius {CAM_RADIUS}, step "
              f"{out['step']}, skip on, white background, d_rgb = the image; (median, min) of {REPS}")
        cols = ["touched", "scene_fwd_ms", "scene_stored_ms", "singles_sum_ms", "stored_over_singles", "stored_over_fwd"]
        print("| volume, N | " + " | ".join(cols) + " |")
        print("|" + "---|" * (len(cols) + 1))
        for name, row in out["rows"].items():
            print(f"| {name} | " + " | ".join(str(row[c]) for c in cols) + " |")
        print("N = 1: largest difference to the single entry, relative: "
              + ", ".join(f"{k}: {r['gap_to_single']:.2e}" for k, r in out["rows"].items() if k.endswith("N=1")))
    else:
        size, views, steps, skip_first = 64, 4, 20, 5
        cams = torch.stack([synthetic.pose_spherical(90.0 * i, -20.0 - 3.0 * i, CAM_RADIUS) for i in range(views)]).float().to(dev)
        poses = ring_poses(2)
        known = bake.BakedScene([rgba, rgba], poses)
        rays = ops.gen_rays(cams, size, size, FOCAL * size / W, Z_NEAR, Z_FAR).reshape(-1, 8)
        target = known.render(rays, white_bkgd=True).rgb
        start = rgba.vol.clone()
        start[..., 3] *= 0.8
        scene = bake.BakedScene([rgba._around(start), rgba._around(start.clone())], poses)
        bake.fit_scene(scene, rays, target, steps=skip_first, white_bkgd=True, skip=True)
        ms, (_, ls) = timed(lambda: bake.fit_scene(scene, rays, target, steps=steps, white_bkgd=True, skip=True))
        out["rows"]["rgba"] = {"rays": rays.shape[0], "batch": 4096, "ms_per_step": round(ms / steps, 3), "loss_first": ls[0], "loss_last": ls[-1]}
        print(f"fit_scene, rgba: 2 objects, {rays.shape[0]} rays, batch 4096: {ms / steps:.3f} ms per step (loss {ls[0]:.3e} -> {ls[-1]:.3e} "
              f"in {steps} steps; the time includes building the module and the fitted scene once)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
