#!/usr/bin/env python3
"""Backward and fitting of baked volumes on the trained-like object of tools/gpu_baked_bench.py, on the GPU box: prints the tables
that go into profiles/baked_notes.md ("Backward and fitting") and one JSON line.

The object, the cameras and the network's render are tools/gpu_baked_bench.py's: procedural spheres, 400 Adam steps through the HIP
path, 8 held-IN views at 128 x 128 (the views of that tool), white background.  8 held-OUT views sit half-way between them (22.5
degrees further round).  Per volume (RGBA at --reso, degree 2 at --sh-reso, both baked from the network as there):

  fwd_ms / bwd_ms    ops.baked_render / baked_sh_render and ops.baked_render_backward on the SAME rays (the 131 072 rays of the held-in
                     views, step = the cell edge, white background, no bits), the backward with a random d_rgb into a buffer that
                     is zeroed once; bwd/fwd is the price of the gradient in forwards.  The same with the volume's skip grid (bits).
  touched            the number of elements of the gradient buffer that are not zero afterwards
  psnr_in / psnr_out PSNR of the baked image against the network's IN-BOX image (the samples outside [-1,1]^3 dropped: the content a
                     volume can hold) on the held-in and on the held-out views, before (`bake`) and after (`fit`) util.bake.fit on
                     the network's in-box renders of the held-in views: --fit-steps steps of Adam at each --lr, batches of --batch
                     rays; fit_s is the wall time of the fit

Timing: after warm-up forward and backward ALTERNATE in one process, every call between two device events ended by a device
synchronise; (median, min) of REPS."""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_occupancy_bench import C1, C2, H, KC, KF, KFD, NVT, W, psnr, stats, timed, trained_object  # noqa: E402
from pixelnerf_amd import ops, util  # noqa: E402
from pixelnerf_amd.render import NeRFRenderer  # noqa: E402
from pixelnerf_amd.util import bake  # noqa: E402
from pixelnerf_amd.util.occupancy import OccupancyGrid  # noqa: E402
from testdata import synthetic  # noqa: E402

REPS, WARMUP = 10, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reso", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--sh-reso", type=int, nargs="*", default=[64])
    ap.add_argument("--n-dirs", type=int, default=32)
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--lr", type=float, nargs="+", default=[1e-2, 5e-2])
    ap.add_argument("--batch", type=int, default=8192)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake)
    net, meta, losses = trained_object(dev, args.steps)
    rend = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).to(dev).eval()

    def cameras(offset):
        return torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + offset + 45.0 * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                            for i in range(NVT)]).float().to(dev)

    poses = {"in": cameras(0.0), "out": cameras(22.5)}
    focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
    cam = (W, H, focal, meta["z_near"], meta["z_far"])
    full = OccupancyGrid.from_density(torch.ones((128, 128, 128), device=dev), C1, C2, 0.5, dilate=0)
    box = {}
    for k, p in poses.items():
        torch.manual_seed(11)
        box[k] = rend.render_views(net, p, *cam, occupancy=full, skip_empty=True).rgb[0].reshape(NVT, H, W, 3)
    rays = util.gen_rays(poses["in"], *cam).reshape(-1, 8).contiguous()
    R = rays.shape[0]
    d_rgb = torch.randn((R, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    out = {"views": NVT, "image": [H, W], "rays": R, "precision": net.precision, "reps": REPS, "train_steps": args.steps,
           "loss_last10": float(sum(losses[-10:]) / 10), "fit": {"steps": args.fit_steps, "batch": args.batch}, "volumes": {}}

    def measure(name, volume):
        stored, degree = volume._stored(), volume.degree
        step = min(volume.cell_size)
        g = {"vol_MB": round(volume.nbytes / 2 ** 20, 1), "step": round(step, 5),
             "samples_per_ray": int(-(-(meta["z_far"] - meta["z_near"]) // step)), "occupied_fraction": round(volume.occupancy.occupied_fraction, 5)}
        for tag, bits in (("", None), ("_bits", volume.occupancy.bits)):
            if degree is None:
                fwd = lambda: ops.baked_render(rays, stored, volume.reso, C1, C2, step, bits=bits, white_bkgd=True)
            else:
                fwd = lambda: ops.baked_sh_render(rays, stored, degree, volume.reso, C1, C2, step, bits=bits, white_bkgd=True)
            buf = torch.zeros_like(stored)
            bwd = lambda: ops.baked_render_backward(rays, stored, degree, volume.reso, C1, C2, step, d_rgb=d_rgb, bits=bits, white_bkgd=True,
                                                    out=buf)
            tf, tb = [], []
            for i in range(REPS + WARMUP):
                a, b = timed(fwd)[0], timed(bwd)[0]
                if i >= WARMUP:
                    tf.append(a), tb.append(b)
            g["fwd" + tag + "_ms"], g["bwd" + tag + "_ms"] = stats(tf), stats(tb)
            g["bwd_over_fwd" + tag] = round(stats(tb)[0] / stats(tf)[0], 2)
            g["touched" + tag] = int((buf != 0).sum())
        before = {k: psnr(volume.render_views(p, *cam, white_bkgd=True, skip=False).rgb, box[k]) for k, p in poses.items()}
        g["psnr_in_bake"], g["psnr_out_bake"] = before["in"], before["out"]
        g["fits"] = {}
        for lr in args.lr:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fitted, fl = bake.fit(volume, rays, box["in"].reshape(-1, 3), steps=args.fit_steps, lr=lr, batch=args.batch, seed=0,
                                  white_bkgd=True)
            torch.cuda.synchronize()
            secs = time.perf_counter() - t0
            after = {k: psnr(fitted.render_views(p, *cam, white_bkgd=True, skip=False).rgb, box[k]) for k, p in poses.items()}
            g["fits"][str(lr)] = {"fit_s": round(secs, 2), "loss_first10": float(sum(fl[:10]) / 10), "loss_last10": float(sum(fl[-10:]) / 10),
                                  "psnr_in_fit": after["in"], "psnr_out_fit": after["out"]}
            del fitted
        out["volumes"][name] = g
        torch.cuda.empty_cache()

    for n in args.reso:
        measure(f"{n}^3 RGBA", bake.BakedVolume.from_model(net, C1, C2, [n, n, n]))
    for n in args.sh_reso:
        measure(f"{n}^3 L2", bake.BakedSHVolume.from_model(net, C1, C2, [n, n, n], degree=2, n_dirs=args.n_dirs))

    print(f"backward and fitting of baked volumes, trained-like object (scene train, {args.steps} steps, loss -> {out['loss_last10']:.4f}), "
          f"precision {net.precision}; {R} rays ({NVT} views {H}x{W}); times (median, min) of {REPS} in ms")
    cols = ["vol_MB", "step", "samples_per_ray", "occupied_fraction", "fwd_ms", "bwd_ms", "bwd_over_fwd", "touched", "fwd_bits_ms", "bwd_bits_ms",
            "bwd_over_fwd_bits", "touched_bits", "psnr_in_bake", "psnr_out_bake"]
    print("| volume | " + " | ".join(cols) + " |")
    print("|" + "---|" * (len(cols) + 1))
    for name, g in out["volumes"].items():
        print(f"| {name} | " + " | ".join(str(g[c]) for c in cols) + " |")
    fcols = ["fit_s", "loss_first10", "loss_last10", "psnr_in_fit", "psnr_out_fit"]
    print(f"fit: {args.fit_steps} steps of Adam, batches of {args.batch} rays of the held-in views, target = the network's in-box render")
    print("| volume | lr | psnr_in_bake | psnr_out_bake | " + " | ".join(fcols) + " |")
    print("|" + "---|" * (len(fcols) + 4))
    for name, g in out["volumes"].items():
        for lr, f in g["fits"].items():
            print(f"| {name} | {lr} | {g['psnr_in_bake']} | {g['psnr_out_bake']} | " + " | ".join(f"{f[c]:.3e}" if "loss" in c else str(f[c]) for c in fcols) + " |")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
