#!/usr/bin/env python3
"""fp32 against fp16 storage of baked volumes on the trained-like object of tools/gpu_baked_bench.py, on the GPU box: prints the table
that goes into profiles/baked_notes.md ("Half-precision storage") and one JSON line.  Same scene and protocol as
tools/gpu_baked_bench.py / gpu_baked_sparse_bench.py (procedural spheres, 400 Adam steps through the HIP path, scene "train", object 0;
8 views at 128 x 128, white background, step = the cell edge).  Per grid resolution (--reso, default 64^3, 128^3, 256^3 over
[-1,1]^3) and per kind (RGBA, SH degree 1, SH degree 2) the fp32 volume is baked once and `half()` of it is what is compared (it holds
the bytes of from_model(dtype=torch.float16)); at --sparse-reso (default 128) the `thr` sparse rows as well: the rows of
OccupancyGrid.from_model(net, c1, c2, reso, --threshold, dilate=1), fp32 and `half()`.  Per row:

  MiB32 / MiB16     bytes of the stored values (sparse rows: rows + index + bits)
  skip ms           render_views(skip=True), fp32 then half; `+ term`: with terminate=1e-2
  PSNR, max d rgb   the half volume's image against the fp32 volume's image (skip=True, no termination), unclamped rgb
  saturated         stored values beyond +-65504 (they are stored as +-65504)
  contract          the half image equals, under torch.equal, the fp32 march of half().float()

Timing: after 2 warm-up rounds the fp32 and the half calls ALTERNATE in one process, every call between two device events ended by a
device synchronise; (median, min) of REPS.
--trace-only: no table; per volume 2 warm-up and REPS alternating calls of the plain march, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/gpu_baked_half_bench.py --trace-only --reso 256 --degrees 2): kernel time alone."""
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
from pixelnerf_amd.util.bake import HALF_MAX, BakedSHVolume, BakedVolume  # noqa: E402
from pixelnerf_amd.util.occupancy import OccupancyGrid  # noqa: E402
from testdata import synthetic  # noqa: E402

REPS, WARMUP = 10, 2


def same(a, b):
    return bool(torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.alpha, b.alpha))


def stored(v):
    return v.vol if hasattr(v, "vol") else v.coef if hasattr(v, "coef") else v.rows


def image_gap(a, b):
    """(PSNR dB, max |d rgb|) of two unclamped images"""
    d = (a.rgb.double() - b.rgb.double())
    mse = float((d ** 2).mean())
    return (float("inf") if mse == 0.0 else round(-10.0 * math.log10(mse), 2)), float(d.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reso", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--degrees", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--n-dirs", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=50.0)
    ap.add_argument("--sparse-reso", type=int, nargs="*", default=[128])
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake, to_half's saturation count: counted below)
    net, meta, losses = trained_object(dev, args.steps)
    print(f"# trained {args.steps} steps, loss -> {sum(losses[-10:]) / 10:.4f}", flush=True)
    poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 45.0 * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                         for i in range(NVT)]).float().to(dev)
    focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
    cam = (W, H, focal, meta["z_near"], meta["z_far"])
    out = {"views": NVT, "image": [H, W], "precision": net.precision, "reps": REPS, "train_steps": args.steps, "threshold": args.threshold,
           "loss_last10": float(sum(losses[-10:]) / 10), "n_dirs": args.n_dirs, "rows": {}}

    def measure(name, v32, v16, mib):
        """one row: v32 and v16 = v32.half() hold the same grid; mib(v) -> MiB"""
        if args.trace_only:
            for _ in range(REPS + WARMUP):
                v32.render_views(poses, *cam, white_bkgd=True)
                v16.render_views(poses, *cam, white_bkgd=True)
            torch.cuda.synchronize()
            print(f"# {name}: traced", flush=True)
            return
        variants = {"skip": dict(), "term": dict(terminate=1e-2)}
        img = {(k, tag): v.render_views(poses, *cam, white_bkgd=True, **kw) for tag, kw in variants.items()
               for k, v in (("32", v32), ("16", v16))}
        times = {key: [] for key in img}
        for i in range(REPS + WARMUP):
            for tag, kw in variants.items():
                for k, v in (("32", v32), ("16", v16)):
                    t = timed(lambda: v.render_views(poses, *cam, white_bkgd=True, **kw))[0]
                    if i >= WARMUP:
                        times[k, tag].append(t)
        wide = v16.float()
        contract = all(same(img["16", tag], wide.render_views(poses, *cam, white_bkgd=True, **kw)) for tag, kw in variants.items())
        del wide
        psnr, worst = image_gap(img["16", "skip"], img["32", "skip"])
        row = {"MiB32": round(mib(v32), 1), "MiB16": round(mib(v16), 1), "skip_ms32": stats(times["32", "skip"]),
               "skip_ms16": stats(times["16", "skip"]), "term_ms32": stats(times["32", "term"]), "term_ms16": stats(times["16", "term"]),
               "psnr": psnr, "max_d_rgb": worst, "saturated": int((stored(v32).abs() > HALF_MAX).sum()), "contract": contract,
               "occupied32": round(v32.occupancy.occupied_fraction, 5), "occupied16": round(v16.occupancy.occupied_fraction, 5)}
        out["rows"][name] = row
        print(f"# {name}: {json.dumps(row)}", flush=True)

    for n in args.reso:
        reso = [n, n, n]
        for degree in [None] + list(args.degrees):
            name = f"{n}^3 " + ("RGBA" if degree is None else f"L{degree}")
            if degree is None:
                v32 = BakedVolume.from_model(net, C1, C2, reso)
            else:
                v32 = BakedSHVolume.from_model(net, C1, C2, reso, degree=degree, n_dirs=args.n_dirs)
            v16 = v32.half()
            measure(name, v32, v16, lambda v: v.nbytes / 2 ** 20)
            if n in args.sparse_reso:
                grid = OccupancyGrid.from_model(net, C1, C2, reso, args.threshold, dilate=1)
                s32 = v32.sparse(grid)
                s16 = s32.half()
                measure(name + " thr rows", s32, s16, lambda v: v.nbytes / 2 ** 20)
                del grid, s32, s16
            del v32, v16
            torch.cuda.empty_cache()
    if args.trace_only:
        return

    print(f"fp32 against fp16 storage, trained-like object (scene train, {args.steps} steps, loss -> {out['loss_last10']:.4f}), precision "
          f"{net.precision}; {NVT} views {H}x{W}; (median, min) ms of {REPS}; thr = OccupancyGrid.from_model at the volume's resolution, "
          f"threshold {args.threshold}, dilate 1")
    print("| volume | MiB fp32 | MiB half | skip ms fp32 | skip ms half | skip + terminate 1e-2 ms fp32 | ms half | PSNR half vs fp32 dB "
          "| max abs d rgb | saturated | occupied cells fp32 / half | contract holds |")
    print("|" + "---|" * 12)
    for name, r in out["rows"].items():
        print(f"| {name} | {r['MiB32']} | {r['MiB16']} | {r['skip_ms32']} | {r['skip_ms16']} | {r['term_ms32']} | {r['term_ms16']} | {r['psnr']} | "
              f"{r['max_d_rgb']:.2e} | {r['saturated']} | {r['occupied32']} / {r['occupied16']} | {r['contract']} |")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
