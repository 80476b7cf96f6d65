#!/usr/bin/env python3
"""Ray gradients of the baked march and camera registration on the trained-like object of tools/gpu_baked_bench.py, on the GPU box:
prints the tables that go into profiles/baked_notes.md ("Ray gradients and registration") and one JSON line.

  cost      8 views of 128 x 128, skip on, on volumes baked from the network -- RGBA at 64^3 and 128^3, degree 2 at 128^3 -- in fp32
            and in fp16 storage: the forward march (ops.*_render_views through `volume._march`), the ray gradient
            (ops.baked_ray_backward_views) and, for the fp32 volumes, the stored-value backward (ops.baked_render_views_backward into
            a buffer zeroed once), every call between two device events, the forms ALTERNATING in one process, (median, min) of REPS
            in ms, and the ratio of each backward to the forward.
  register  util.bake.register on the 128^3 RGBA volume: --views cameras of 64 x 64 pixels of the object's orbit, the target the
            volume's own render of the true poses, the start --deg degrees (about a fixed axis per camera) and --shift (along a
            fixed direction per camera) off, --reg-steps steps of Adam at --lr: per camera the rotation and translation error at
            the end and the view's mean squared error at both ends, the loss at both ends and the wall time; a sweep over the
            starting error shows the basin."""
import argparse
import json
import math
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_occupancy_bench import C1, C2, H, NVT, W, stats, timed, trained_object  # noqa: E402
from pixelnerf_amd import ops  # noqa: E402
from pixelnerf_amd.util import bake  # noqa: E402
from testdata import synthetic  # noqa: E402

REPS, WARMUP = 10, 2
AXES = ((0.3, 0.8, -0.52), (-0.6, 0.2, 0.77), (0.5, -0.7, 0.5), (0.1, 0.5, 0.86))
SHIFTS = ((0.6, -0.64, 0.48), (-0.36, 0.8, 0.48), (0.0, 0.6, -0.8), (0.7, 0.1, -0.7))


def cost(volume, poses, cam, ups):
    Wc, Hc, focal, z_near, z_far = cam
    stored, degree, bits = volume._stored(), volume.degree, volume.occupancy.bits
    step = min(volume.cell_size)
    geo = (stored, degree, volume.reso, volume.c1, volume.c2, step)
    kw = dict(d_rgb=ups[0], d_depth=ups[1], d_alpha=ups[2], bits=bits, white_bkgd=True)
    forms = {
        "forward": lambda: volume._march((poses, Wc, Hc, focal, None, z_near, z_far), step, bits, True, 0.0),
        "ray_grad": lambda: ops.baked_ray_backward_views(poses, Wc, Hc, focal, None, z_near, z_far, *geo, **kw),
    }
    if stored.dtype == torch.float32:
        buf = torch.zeros_like(stored)
        forms["stored_grad"] = lambda: ops.baked_render_views_backward(poses, Wc, Hc, focal, None, z_near, z_far, *geo, out=buf, **kw)
    times = {k: [] for k in forms}
    for i in range(REPS + WARMUP):
        for k, fn in forms.items():
            t = timed(fn)[0]
            if i >= WARMUP:
                times[k].append(t)
    g = {k + "_ms": stats(v) for k, v in times.items()}
    g["ray_grad / forward"] = round(g["ray_grad_ms"][0] / g["forward_ms"][0], 2)
    if "stored_grad_ms" in g:
        g["stored_grad / forward"] = round(g["stored_grad_ms"][0] / g["forward_ms"][0], 2)
    a = ops.baked_ray_backward_views(poses, Wc, Hc, focal, None, z_near, z_far, *geo, **kw)
    g["same_bytes_twice"] = bool(torch.equal(a, ops.baked_ray_backward_views(poses, Wc, Hc, focal, None, z_near, z_far, *geo, **kw)))
    g["rows_nonzero"] = int((a.reshape(-1, 8).abs().sum(dim=1) > 0).sum())
    return g


def pose_errors(poses, true):
    rel = poses[:, :3, :3].double() @ true[:, :3, :3].double().transpose(1, 2)
    cos = ((rel[:, 0, 0] + rel[:, 1, 1] + rel[:, 2, 2]) - 1.0) / 2.0
    return torch.rad2deg(torch.acos(cos.clamp(-1.0, 1.0))), (poses[:, :3, 3] - true[:, :3, 3]).double().norm(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--part", choices=["cost", "register", "both"], default="both")
    ap.add_argument("--n-dirs", type=int, default=32)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reg-steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--starts", type=float, nargs="*", default=[2.0, 0.05, 5.0, 0.12, 10.0, 0.25, 20.0, 0.5],
                    help="pairs: degrees, shift (in units of the box half-edge)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake)
    net, meta, losses = trained_object(dev, args.steps)
    out = {"precision": net.precision, "reps": REPS, "train_steps": args.steps, "loss_last10": float(sum(losses[-10:]) / 10)}

    def cameras(n):
        return torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 360.0 / n * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                            for i in range(n)]).float().to(dev)

    volumes = {"64^3 RGBA": lambda: bake.BakedVolume.from_model(net, C1, C2, [64, 64, 64]),
               "128^3 RGBA": lambda: bake.BakedVolume.from_model(net, C1, C2, [128, 128, 128]),
               "128^3 L2": lambda: bake.BakedSHVolume.from_model(net, C1, C2, [128, 128, 128], degree=2, n_dirs=args.n_dirs)}

    if args.part in ("cost", "both"):
        poses = cameras(NVT)
        focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
        cam = (W, H, focal, meta["z_near"], meta["z_far"])
        R = NVT * H * W
        gen = torch.Generator(device=dev).manual_seed(3)
        ups = [torch.randn(s, generator=gen, device=dev) for s in ((R, 3), (R,), (R,))]
        out["cost"] = {}
        for name, make in volumes.items():
            volume = make()
            out["cost"][name + " fp32"] = cost(volume, poses, cam, ups)
            out["cost"][name + " fp16"] = cost(volume.half(), poses, cam, ups)
            del volume
            torch.cuda.empty_cache()
        print(f"{NVT} views {W} x {H}, skip on, step = the cell edge, all three upstream gradients given; times (median, min) of {REPS} in ms, "
              "forms alternating in one process")
        cols = ["forward_ms", "ray_grad_ms", "ray_grad / forward", "stored_grad_ms", "stored_grad / forward", "same_bytes_twice", "rows_nonzero"]
        print("| volume | " + " | ".join(cols) + " |")
        print("|" + "---|" * (len(cols) + 1))
        for name, g in out["cost"].items():
            print(f"| {name} | " + " | ".join(str(g.get(c, "-")) for c in cols) + " |")

    if args.part in ("register", "both"):
        n, size = args.views, args.size
        volume = volumes["128^3 RGBA"]()
        true = cameras(n)
        focal = (meta["focal"][0] * size / meta["W"], meta["focal"][1] * size / meta["H"])
        cam = (size, size, focal, meta["z_near"], meta["z_far"])
        target = volume.render_views(true, *cam, white_bkgd=True).rgb
        out["register"] = {"views": n, "size": size, "steps": args.reg_steps, "lr": args.lr, "rows": []}
        for deg, shift in zip(args.starts[0::2], args.starts[1::2]):
            w = torch.tensor([[c / math.sqrt(sum(x * x for x in a)) * math.radians(deg) for c in a] for a in AXES[:n]], device=dev)
            v = torch.tensor([[c / math.sqrt(sum(x * x for x in s)) * shift for c in s] for s in SHIFTS[:n]], device=dev)
            start = bake.moved_poses(true, w, v)
            rot0, tr0 = pose_errors(start, true)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            poses, rl = bake.register(volume, target, start, *cam, steps=args.reg_steps, lr=args.lr, white_bkgd=True)
            torch.cuda.synchronize()
            secs = time.perf_counter() - t0
            rot, tr = pose_errors(poses, true)
            end = volume.render_views(poses, *cam, white_bkgd=True).rgb
            per_view = lambda img: [float(f"{x:.3e}") for x in ((img - target) ** 2).mean(dim=(1, 2, 3)).tolist()]
            first = volume.render_views(start, *cam, white_bkgd=True).rgb
            out["register"]["rows"].append({"start_deg": deg, "start_shift": shift, "rot_deg_start": round(float(rot0.mean()), 3),
                                            "rot_deg_end_mean": round(float(rot.mean()), 3), "rot_deg_end_max": round(float(rot.max()), 3),
                                            "shift_end_mean": round(float(tr.mean()), 4), "shift_end_max": round(float(tr.max()), 4),
                                            "rot_deg_end": [round(x, 3) for x in rot.tolist()], "shift_end": [round(x, 4) for x in tr.tolist()],
                                            "mse_start": per_view(first), "mse_end": per_view(end),
                                            "loss_start": rl[0], "loss_end": rl[-1], "wall_s": round(secs, 2),
                                            "ms_per_step": round(1e3 * secs / max(args.reg_steps, 1), 2)})
        print(f"register: 128^3 RGBA volume, {n} views of {size} x {size}, target = the volume's render of the true poses, {args.reg_steps} steps of Adam "
              f"at lr {args.lr}, skip on")
        rcols = ["start_deg", "start_shift", "rot_deg_end", "shift_end", "mse_start", "mse_end", "loss_start", "loss_end", "wall_s", "ms_per_step"]
        print("| " + " | ".join(rcols) + " |")
        print("|" + "---|" * len(rcols))
        for r in out["register"]["rows"]:
            print("| " + " | ".join(f"{r[c]:.3e}" if c.startswith("loss") else str(r[c]) for c in rcols) + " |")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
