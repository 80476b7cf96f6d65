#!/usr/bin/env python3
"""Gradients of the scene march on a trained-like object, on the GPU box: prints the tables that go into profiles/baked_notes.md
("Scene gradients and placing objects") and one JSON line per part.

The scenes are those of tools/gpu_baked_scene_bench.py: N = 1, 2, 4, 8 copies of the 128^3 object on its ring (the SAME stored tensor
under N poses), 8 views of 128 x 128 from radius 9, white background, step = the cell edge, skip on; RGBA and degree 2, fp32 and fp16.
Upstream gradients: d_rgb = the image itself (every pixel that sees an object has one).

  cost   per row, alternating in one process after warm-up, each call between two device events:
           scene_bwd    ops.baked_scene_backward_views with the pose reduction (march backward + two reduction kernels)
           no_poses     the same with want_poses=False: the difference is the pose reduction alone (iii)
           singles_sum  the N ops.baked_ray_backward_views calls of the parent commit, each with the cameras moved into its object's
                        frame (at N = 1: THE baseline (i); beyond: what the same loads cost without the mixing (ii))
           scene_fwd    BakedScene.render_views, for the backward / forward ratio (ii)
         N = 1 also checks that d_rays is the single entry's bytes.
  place  one step of util.bake.place (iv): 2 objects of the ring, 4 views of 64 x 64, object 1 moved; (total time of 20 steps
         after 5) / 20.

Run without --part, the tool is a driver: it starts each part as a child process of its own under its own time limit and stops at
the first that fails or runs out of time.  A part uses at most 16 CPU threads."""
import argparse
import json
import os
import subprocess
import sys
import warnings

PARTS = {"cost": 900, "place": 420}   # seconds allowed per part


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
        volumes = {"rgba fp32": rgba, "rgba fp16": rgba.half(), "degree 2 fp32": sh2, "degree 2 fp16": sh2.half()}
        step = min(rgba.cell_size)
        for kind, vol in volumes.items():
            for n in args.counts:
                poses = ring_poses(n)
                scene = bake.BakedScene([vol] * n, poses)
                objects = scene._objects(True)
                local = [(torch.linalg.inv(poses[j].double()).float().to(dev) @ cams).contiguous() for j in range(n)]
                d_rgb = scene.render_views(cams, *cam, white_bkgd=True).rgb.reshape(-1, 3).contiguous()
                scene_bwd = lambda want=True: ops.baked_scene_backward_views(cams, W, H, FOCAL, None, Z_NEAR, Z_FAR, objects, step, d_rgb=d_rgb,
                                                                             white_bkgd=True, want_poses=want)
                single_bwd = lambda j: ops.baked_ray_backward_views(local[j], W, H, FOCAL, None, Z_NEAR, Z_FAR, vol._stored(), vol.degree, vol.reso,
                                                                    vol.c1, vol.c2, step, d_rgb=d_rgb, bits=vol.occupancy.bits, white_bkgd=True)
                scene_fwd = lambda: scene.render_views(cams, *cam, white_bkgd=True)
                got = scene_bwd()
                row = {"nonzero_rows": round(float(got[0].reshape(-1, 8).any(dim=1).float().mean()), 4)}
                if n == 1:
                    row["bytes_of_the_single_entry"] = bool(torch.equal(got[0], single_bwd(0)))
                t = {"scene_bwd": [], "no_poses": [], "singles_sum": [], "scene_fwd": []}
                for i in range(REPS + WARMUP):
                    a = timed(scene_bwd)[0]
                    b = timed(lambda: scene_bwd(False))[0]
                    c = sum(timed(lambda: single_bwd(j))[0] for j in range(n))
                    d = timed(scene_fwd)[0]
                    if i >= WARMUP:
                        t["scene_bwd"].append(a), t["no_poses"].append(b), t["singles_sum"].append(c), t["scene_fwd"].append(d)
                for k, v in t.items():
                    row[k + "_ms"] = stats(v)
                row["pose_reduction_ms"] = round(row["scene_bwd_ms"][0] - row["no_poses_ms"][0], 3)
                row["bwd_over_singles"] = round(row["scene_bwd_ms"][0] / row["singles_sum_ms"][0], 3)
                row["bwd_over_fwd"] = round(row["scene_bwd_ms"][0] / row["scene_fwd_ms"][0], 3)
                out["rows"][f"{kind} N={n}"] = row
                del scene, got
            torch.cuda.empty_cache()
        print(f"scene gradients, trained-like object ({args.steps} steps), {args.reso}^3; {NVT} views {H}x{W} from radius {CAM_RADIUS}, step "
              f"{out['step']}, skip on, white background, d_rgb = the image; (median, min) of {REPS}")
        cols = ["nonzero_rows", "scene_bwd_ms", "no_poses_ms", "pose_reduction_ms", "singles_sum_ms", "scene_fwd_ms", "bwd_over_singles", "bwd_over_fwd"]
        print("| volume, N | " + " | ".join(cols) + " |")
        print("|" + "---|" * (len(cols) + 1))
        for name, row in out["rows"].items():
            print(f"| {name} | " + " | ".join(str(row[c]) for c in cols) + " |")
        print("N = 1: d_rays is the bytes of the single entry: " + str(all(r["bytes_of_the_single_entry"] for k, r in out["rows"].items() if k.endswith("N=1"))))
    else:
        size, views, steps, skip_first = 64, 4, 20, 5
        cams = torch.stack([synthetic.pose_spherical(90.0 * i, -20.0 - 3.0 * i, CAM_RADIUS) for i in range(views)]).float().to(dev)
        cam = (size, size, FOCAL * size / W, Z_NEAR, Z_FAR)
        for kind, vol in {"rgba fp32": rgba, "rgba fp16": rgba.half()}.items():
            true = ring_poses(2)
            start = true.clone()
            start[1, :3] = bake.moved_poses(true[1:, :3], torch.tensor([[0.0, 0.0, 0.05]]), torch.tensor([[0.03, -0.02, 0.02]]))[0]
            target = bake.BakedScene([vol] * 2, true).render_views(cams, *cam, white_bkgd=True).rgb
            scene = bake.BakedScene([vol] * 2, start)
            bake.place(scene, target, cams, *cam, objects=[1], steps=skip_first, white_bkgd=True)
            ms, (_, ls) = timed(lambda: bake.place(scene, target, cams, *cam, objects=[1], steps=steps, white_bkgd=True))
            out["rows"][kind] = {"views": views, "image": size, "ms_per_step": round(ms / steps, 3), "loss_first": ls[0], "loss_last": ls[-1]}
            print(f"place, {kind}: 2 objects, {views} views {size}x{size}: {ms / steps:.3f} ms per step (loss {ls[0]:.3e} -> {ls[-1]:.3e} in {steps} steps)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
