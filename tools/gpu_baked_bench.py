#!/usr/bin/env python3
"""Baked volumes on a trained-like object, on the GPU box: prints the table that goes into profiles/baked_notes.md and one JSON line.

The object is the one tools/gpu_occupancy_bench.py makes (procedural spheres, 400 Adam steps through the HIP path, scene "train",
object 0), rendered as there: 8 views at 128 x 128, white background.  Per grid resolution (64^3, 128^3, 256^3 over [-1,1]^3):

  bake_ms        BakedVolume.from_model (fine network, fake view directions, skip grid at threshold 0 included)
  plain_ms       render_views(skip=False), step = the cell edge
  skip_ms        render_views(skip=True): the same bytes (checked here), empty cells not read
  skip_term_ms   render_views(skip=True, terminate=1e-2)
  psnr_vs_net / max_abs_vs_net   the baked image (skip=True) against the network's render_views of the same cameras (64 + 128
                 samples).  This model is hazy well beyond the box (profiles/occupancy_notes.md), and a volume holds nothing outside
                 its box, so also:
  psnr_vs_net_box / max_abs_vs_net_box   against the network's render with the samples outside [-1,1]^3 dropped (a FULL occupancy
                 grid + skip_empty): the same content, so what is left is the approximation itself
  net_dense_ms / net_sparse_ms   the network's own call: dense, and with OccupancyGrid (128^3, threshold 50, dilate 1) + skip_empty

View-dependent volumes (--sh-reso, default 64^3 and 128^3; degree 1 and 2, BakedSHVolume.from_model with --n-dirs directions): the
same columns (bake_ms of ONE bake: it is n_dirs network passes), beside the RGBA rows of the same session.  And, to tell the
direction effect from the sampling effect: `rgba_view_dir`, per resolution, is an RGBA volume baked for EACH view with that view's
central ray direction (BakedVolume.from_model(viewdirs=d)) and rendered for that view alone -- the one-direction approximation with
nearly the right direction, so what it still lacks against the network's in-box image is the grid, the equidistant samples against
the network's 64 + 128 stochastic ones, and the spread of directions inside one view.

Timing: after warm-up the variants ALTERNATE in one process, every call between two device events ended by a device synchronise;
(median, min) of REPS."""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_occupancy_bench import C1, C2, H, KC, KF, KFD, NVT, W, psnr, stats, timed, trained_object  # noqa: E402
from pixelnerf_amd.render import NeRFRenderer  # noqa: E402
from pixelnerf_amd import util  # noqa: E402
from pixelnerf_amd.util.bake import BakedSHVolume, BakedVolume  # noqa: E402
from pixelnerf_amd.util.occupancy import OccupancyGrid  # noqa: E402
from testdata import synthetic  # noqa: E402

REPS, WARMUP, EPS = 10, 2, 1e-2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reso", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--sh-reso", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--n-dirs", type=int, default=32)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake)
    net, meta, losses = trained_object(dev, args.steps)
    rend = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).to(dev).eval()
    poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 45.0 * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                         for i in range(NVT)]).float().to(dev)
    focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
    cam = (W, H, focal, meta["z_near"], meta["z_far"])
    out = {"views": NVT, "image": [H, W], "net_samples": [KC, KF, KFD], "precision": net.precision, "reps": REPS, "eps": EPS,
           "train_steps": args.steps, "loss_last10": float(sum(losses[-10:]) / 10), "z": [meta["z_near"], meta["z_far"]]}

    def net_render(**kw):
        torch.manual_seed(11)
        return rend.render_views(net, poses, *cam, **kw)

    occ = OccupancyGrid.from_model(net, C1, C2, [128, 128, 128], 50.0, dilate=1)
    dense_img = net_render().rgb[0]
    full = OccupancyGrid.from_density(torch.ones((128, 128, 128), device=dev), C1, C2, 0.5, dilate=0)
    box_img = net_render(occupancy=full, skip_empty=True).rgb[0]
    out["psnr_net_box_vs_net"] = psnr(box_img, dense_img)
    td, ts = [], []
    for i in range(REPS + WARMUP):
        a = timed(net_render)[0]
        b = timed(lambda: net_render(occupancy=occ, skip_empty=True))[0]
        if i >= WARMUP:
            td.append(a), ts.append(b)
    out["net_dense_ms"], out["net_sparse_ms"] = stats(td), stats(ts)

    variants = {"plain": dict(skip=False), "skip": dict(skip=True), "skip_term": dict(skip=True, terminate=EPS)}

    def measure(bv, t_bake, nbytes):
        """the columns of one volume (RGBA or SH)"""
        img = {k: bv.render_views(poses, *cam, white_bkgd=True, **kw) for k, kw in variants.items()}
        times = {k: [] for k in variants}
        for i in range(REPS + WARMUP):
            for k, kw in variants.items():
                t = timed(lambda: bv.render_views(poses, *cam, white_bkgd=True, **kw))[0]
                if i >= WARMUP:
                    times[k].append(t)
        g = {"vol_MB": round(nbytes / 2 ** 20, 1), "step": round(min(bv.cell_size), 5),
             "samples_per_ray": int(-(-(meta["z_far"] - meta["z_near"]) // min(bv.cell_size))),
             "occupied_fraction": round(bv.occupancy.occupied_fraction, 5), "bake_ms": t_bake}
        for k in variants:
            g[k + "_ms"] = stats(times[k])
        g["skip_bit_equal"] = bool(torch.equal(img["plain"].rgb, img["skip"].rgb) and torch.equal(img["plain"].depth, img["skip"].depth))
        g["psnr_vs_net"] = psnr(img["skip"].rgb, dense_img)
        g["max_abs_vs_net"] = round(float((img["skip"].rgb.clamp(0, 1) - dense_img.clamp(0, 1)).abs().max()), 4)
        g["psnr_vs_net_box"] = psnr(img["skip"].rgb, box_img)
        g["max_abs_vs_net_box"] = round(float((img["skip"].rgb.clamp(0, 1) - box_img.clamp(0, 1)).abs().max()), 4)
        g["term_max_abs"] = float((img["skip_term"].rgb - img["skip"].rgb).abs().max())
        return g

    out["sh"], out["rgba_view_dir"] = {}, {}
    centre = util.gen_rays(poses, *cam)[:, H // 2, W // 2, 3:6]     # the central ray direction of every view
    if args.sh_reso:
        BakedSHVolume.from_model(net, C1, C2, [16, 16, 16], degree=2, n_dirs=args.n_dirs)  # (warm-up: an SH bake is timed once)
    for n in args.sh_reso:
        reso = [n, n, n]
        per_view = []
        for v in range(NVT):
            one = BakedVolume.from_model(net, C1, C2, reso, viewdirs=centre[v].tolist())
            per_view.append(one.render_views(poses[v:v + 1], *cam, white_bkgd=True).rgb)
            del one
        per_view = torch.cat(per_view)
        out["rgba_view_dir"][str(n)] = {"psnr_vs_net": psnr(per_view, dense_img), "psnr_vs_net_box": psnr(per_view, box_img),
                                        "max_abs_vs_net_box": round(float((per_view.clamp(0, 1) - box_img.clamp(0, 1)).abs().max()), 4)}
        for degree in (1, 2):
            t, sh = timed(lambda: BakedSHVolume.from_model(net, C1, C2, reso, degree=degree, n_dirs=args.n_dirs))
            out["sh"][f"{n}^3 L{degree}"] = measure(sh, round(t, 3), sh.coef.numel() * 4)
            del sh
            torch.cuda.empty_cache()

    out["grids"] = {}
    for n in args.reso:
        reso = [n, n, n]
        t_bake = [timed(lambda: BakedVolume.from_model(net, C1, C2, reso))[0] for _ in range(3)]
        bv = BakedVolume.from_model(net, C1, C2, reso)
        out["grids"][str(n)] = measure(bv, stats(t_bake), bv.vol.numel() * 4)
        del bv
        torch.cuda.empty_cache()

    print(f"baked volumes, trained-like object (scene train, {args.steps} steps, loss -> {out['loss_last10']:.4f}), precision {net.precision}; "
          f"{NVT} views {H}x{W}; network call {KC}+{KF} ({KFD} depth) samples: dense {out['net_dense_ms']} ms, "
          f"occupancy 128^3 thr 50 + skip_empty {out['net_sparse_ms']} ms (median, min of {REPS}); "
          f"the network's render without the samples outside the box against its dense render: {out['psnr_net_box_vs_net']} dB")
    cols = ["vol_MB", "step", "samples_per_ray", "occupied_fraction", "bake_ms", "plain_ms", "skip_ms", "skip_term_ms", "skip_bit_equal",
            "psnr_vs_net", "max_abs_vs_net", "psnr_vs_net_box", "max_abs_vs_net_box", "term_max_abs"]
    print("| reso | " + " | ".join(cols) + " |")
    print("|" + "---|" * (len(cols) + 1))
    for n, g in list((k + "^3", g) for k, g in out["grids"].items()) + list(out["sh"].items()):
        print(f"| {n} | " + " | ".join(f"{g[c]:.2e}" if c == "term_max_abs" else str(g[c]) for c in cols) + " |")
    for n, g in out["rgba_view_dir"].items():
        print(f"RGBA volume baked per view with the view's central direction, {n}^3: PSNR vs net {g['psnr_vs_net']} dB, vs net-in-box "
              f"{g['psnr_vs_net_box']} dB (max abs {g['max_abs_vs_net_box']})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
