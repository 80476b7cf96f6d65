#!/usr/bin/env python3
"""The total-variation prior of baked volumes on the trained-like object of tools/gpu_baked_bench.py, on the GPU box: prints the tables
that go into profiles/baked_notes.md ("Total-variation prior") and one JSON line.

The object, the cameras and the network's in-box renders are tools/gpu_baked_fit_bench.py's.  Two parts (--part cost / fit / both):

  cost   one ops.baked_tv call on volumes baked from the network -- RGBA at --reso, degree 2 at --sh-reso, and the sparse rows of each
         under the threshold-50 grid (OccupancyGrid.from_model(net, C1, C2, reso, 50, dilate=1)) --: the value alone, the gradient
         alone (into a buffer zeroed once) and both, every call between two device events, the forms ALTERNATING in one process,
         (median, min) of REPS in ms.  Beside it: the same definition in torch eager fp32 on the same GPU (value under no_grad; value
         + gradient by autograd) with its peak extra memory; GB/s over the bytes a call has to move (stored read once; with a
         gradient, grad read and written once as well); and a torch device-to-device copy that moves the same number of bytes
         (reads half of them, writes half) in the same process.
  fit    util.bake.fit on the 64^3 RGBA and the 64^3 degree-2 volume with tv_rgb = tv_sigma in --tv (degree 2: also with tv_sh = 10 x
         that), lr 0.01, --fit-steps steps, batches of --batch rays of the 8 held-in views: psnr_in, psnr_out (8 held-out views
         half-way between), fit_s."""
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
EPS = 1e-8


def eager_tv(stored, w, eps):
    """the definition in torch eager on the device (dense form): what a caller without the kernel would write"""
    S = stored.reshape(tuple(stored.shape[:3]) + (-1,))
    diffs = []
    for axis in range(3):
        n = S.shape[axis]
        pad = list(S.shape)
        pad[axis] = 1
        diffs.append(torch.cat((S.narrow(axis, 1, n - 1) - S.narrow(axis, 0, n - 1), S.new_zeros(pad)), dim=axis))
    dx, dy, dz = diffs
    return (torch.sqrt(dx * dx + dy * dy + dz * dz + eps) * w).sum() / float(S.shape[0] * S.shape[1] * S.shape[2])


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 1)


def cost(name, volume, sparse_of=None):
    stored, degree = volume._stored(), volume.degree
    sparse = volume._stored_name == "rows"
    w = [1.0] * (4 if degree is None else 4 * (degree + 1) ** 2)
    extra = dict(index=volume.index, ids=volume.ids) if sparse else {}
    buf = torch.zeros_like(stored)
    nbytes = stored.numel() * 4
    forms = {
        "value": (lambda: ops.baked_tv(stored, degree, volume.reso, w, eps=EPS, **extra), nbytes),
        "grad": (lambda: ops.baked_tv(stored, degree, volume.reso, w, eps=EPS, want_value=False, grad_out=buf, **extra), 3 * nbytes),
        "both": (lambda: ops.baked_tv(stored, degree, volume.reso, w, eps=EPS, grad_out=buf, **extra), 3 * nbytes),
    }
    src = {k: torch.empty(max(b // 8, 1), dtype=torch.float32, device=stored.device) for k, (_, b) in forms.items()}
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    for k in forms:
        forms[k] = forms[k] + ((lambda k=k: dst[k].copy_(src[k])),)
    times = {k: [] for k in forms}
    copies = {k: [] for k in forms}
    for i in range(REPS + WARMUP):
        for k, (fn, _, cp) in forms.items():
            a, b = timed(fn)[0], timed(cp)[0]
            if i >= WARMUP:
                times[k].append(a), copies[k].append(b)
    g = {"rows_or_points": int(stored.shape[0]) if sparse else int(stored.shape[0] * stored.shape[1] * stored.shape[2]),
         "stored_MB": round(nbytes / 2 ** 20, 1)}
    for k, (_, b, _) in forms.items():
        g[k + "_ms"], g[k + "_copy_ms"] = stats(times[k]), stats(copies[k])
        g[k + "_GBps"] = round(b / stats(times[k])[0] / 1e6, 1)
        g[k + "_copy_GBps"] = round(b / stats(copies[k])[0] / 1e6, 1)
    if not sparse:   # the eager restatement is the dense form
        wt = torch.tensor(w, device=stored.device)

        def eager_value():
            with torch.no_grad():
                return eager_tv(stored, wt, EPS)

        def eager_both():
            leaf = stored.detach().requires_grad_(True)
            value = eager_tv(leaf, wt, EPS)
            value.backward()
            return value.detach(), leaf.grad

        ev, eb = [], []
        for i in range(3 + 1):
            a, b = timed(eager_value)[0], timed(eager_both)[0]
            if i >= 1:
                ev.append(a), eb.append(b)
        g["eager_value_ms"], g["eager_both_ms"] = stats(ev), stats(eb)
        g["eager_value_peak_MB"], g["eager_both_peak_MB"] = peak_extra(eager_value), peak_extra(eager_both)
        g["hip_both_peak_MB"] = peak_extra(forms["both"][0])
        v32 = ops.baked_tv(stored, degree, volume.reso, w, eps=EPS)[0]
        g["value_hip"], g["value_eager"] = float(v32), float(eager_value())
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--part", choices=["cost", "fit", "both"], default="both")
    ap.add_argument("--reso", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--sh-reso", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--n-dirs", type=int, default=32)
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--tv", type=float, nargs="*", default=[0.0, 1e-4, 1e-3, 1e-2, 1e-1])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake)
    net, meta, losses = trained_object(dev, args.steps)
    out = {"precision": net.precision, "reps": REPS, "train_steps": args.steps, "loss_last10": float(sum(losses[-10:]) / 10)}

    if args.part in ("cost", "both"):
        out["cost"] = {}
        for degree, resos in ((None, args.reso), (2, args.sh_reso)):
            for n in resos:
                tag = f"{n}^3 " + ("RGBA" if degree is None else "L2")
                if degree is None:
                    dense = bake.BakedVolume.from_model(net, C1, C2, [n, n, n])
                else:
                    dense = bake.BakedSHVolume.from_model(net, C1, C2, [n, n, n], degree=2, n_dirs=args.n_dirs)
                out["cost"][tag] = cost(tag, dense)
                occ = OccupancyGrid.from_model(net, C1, C2, [n, n, n], 50.0, dilate=1)
                out["cost"][tag + " sparse thr 50"] = cost(tag, dense.sparse(occ))
                del dense, occ
                torch.cuda.empty_cache()
        print(f"cost of one ops.baked_tv call, trained-like object (scene train, {args.steps} steps), all weights 1, eps {EPS}; times (median, min) of "
              f"{REPS} in ms; GB/s over stored (value) or 3 x stored (grad, both); copy: a device-to-device copy moving the same bytes")
        cols = ["rows_or_points", "stored_MB", "value_ms", "value_GBps", "value_copy_GBps", "grad_ms", "grad_GBps", "both_ms", "both_GBps", "both_copy_ms",
                "both_copy_GBps"]
        print("| volume | " + " | ".join(cols) + " |")
        print("|" + "---|" * (len(cols) + 1))
        for name, g in out["cost"].items():
            print(f"| {name} | " + " | ".join(str(g[c]) for c in cols) + " |")
        ecols = ["value_ms", "eager_value_ms", "eager_value_peak_MB", "both_ms", "eager_both_ms", "eager_both_peak_MB", "hip_both_peak_MB", "value_hip",
                 "value_eager"]
        print("the same definition in torch eager fp32 (dense forms); peak: extra device memory of one call in MB")
        print("| volume | " + " | ".join(ecols) + " |")
        print("|" + "---|" * (len(ecols) + 1))
        for name, g in out["cost"].items():
            if "eager_value_ms" in g:
                print(f"| {name} | " + " | ".join(str(g[c]) for c in ecols) + " |")

    if args.part in ("fit", "both"):
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
        volumes = {"64^3 RGBA": bake.BakedVolume.from_model(net, C1, C2, [64, 64, 64]),
                   "64^3 L2": bake.BakedSHVolume.from_model(net, C1, C2, [64, 64, 64], degree=2, n_dirs=args.n_dirs)}
        out["fit"] = {"steps": args.fit_steps, "batch": args.batch, "lr": args.lr, "rows": []}
        for name, volume in volumes.items():
            before = {k: psnr(volume.render_views(p, *cam, white_bkgd=True, skip=False).rgb, box[k]) for k, p in poses.items()}
            sweeps = [(t, None) for t in args.tv] + ([(t, 10.0 * t) for t in args.tv if t > 0] if volume.degree is not None else [])
            for t, sh in sweeps:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fitted, fl = bake.fit(volume, rays, box["in"].reshape(-1, 3), steps=args.fit_steps, lr=args.lr, batch=args.batch, seed=0,
                                      white_bkgd=True, tv_rgb=t, tv_sigma=t, tv_sh=sh)
                torch.cuda.synchronize()
                secs = time.perf_counter() - t0
                after = {k: psnr(fitted.render_views(p, *cam, white_bkgd=True, skip=False).rgb, box[k]) for k, p in poses.items()}
                out["fit"]["rows"].append({"volume": name, "tv_rgb=tv_sigma": t, "tv_sh": sh, "psnr_in_bake": before["in"], "psnr_out_bake": before["out"],
                                           "fit_s": round(secs, 2), "loss_last10": float(sum(fl[-10:]) / 10), "psnr_in_fit": after["in"],
                                           "psnr_out_fit": after["out"], "tv_before": round(volume.tv(), 5), "tv_after": round(fitted.tv(), 5)})
                del fitted
        print(f"fit with the prior: {args.fit_steps} steps of Adam at lr {args.lr}, batches of {args.batch} rays of the held-in views; tv_sh None: the DC weights")
        fcols = ["volume", "tv_rgb=tv_sigma", "tv_sh", "psnr_in_bake", "psnr_out_bake", "fit_s", "loss_last10", "psnr_in_fit", "psnr_out_fit", "tv_before",
                 "tv_after"]
        print("| " + " | ".join(fcols) + " |")
        print("|" + "---|" * len(fcols))
        for r in out["fit"]["rows"]:
            print("| " + " | ".join(f"{r[c]:.3e}" if c == "loss_last10" else str(r[c]) for c in fcols) + " |")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
