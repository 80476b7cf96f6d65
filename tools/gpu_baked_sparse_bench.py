#!/usr/bin/env python3
"""Dense against sparse baked volumes on the trained-like object of tools/gpu_baked_bench.py, on the GPU box: prints the table that goes
into profiles/baked_notes.md ("Sparse baked volumes") and one JSON line.  Same scene and protocol as tools/gpu_baked_bench.py
(procedural spheres, 400 Adam steps through the HIP path, scene "train", object 0; 8 views at 128 x 128, white background, step = the
cell edge).  Per grid resolution (--reso, default 64^3, 128^3, 256^3 over [-1,1]^3) and per kind (RGBA, SH degree 1, SH degree 2), for
two occupancy grids -- `own`: the dense volume's skip grid (threshold 0, dilate 0), and `thr`: OccupancyGrid.from_model(net, c1, c2,
reso, --threshold, dilate=1), the grid one would bake sparsely with --:

  kept            M / P: the share of the grid points the sparse volume keeps
  dense_MB / sparse_MB   bytes of the dense tensor; rows + index + bits of the sparse volume
  bake_dense_ms   BakedVolume.from_model / BakedSHVolume.from_model (everything included)
  grid_ms         OccupancyGrid.from_model at the volume's resolution (`thr` only: the sparse bake needs the grid first)
  bake_sparse_ms  SparseBakedVolume.from_model with that grid (`thr` only); `bake_equal`: its rows equal the dense rows at ids
  dense_ms        dense render_views(skip=True) marched against the grid's bits
  sparse_ms       the sparse volume's render_views; `equal`: rgb, depth and alpha equal the dense call's under torch.equal

Timing: after warm-up the four render calls (dense own, sparse own, dense thr, sparse thr) ALTERNATE in one process, every call between
two device events ended by a device synchronise; (median, min) of REPS.  Bakes: (median, min) of 3 for RGBA, ONE bake after a warm-up
bake for SH (it is n_dirs network passes)."""
import argparse
import copy
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_occupancy_bench import C1, C2, H, NVT, W, stats, timed, trained_object  # noqa: E402
from pixelnerf_amd.util.bake import BakedSHVolume, BakedVolume, SparseBakedVolume  # noqa: E402
from pixelnerf_amd.util.occupancy import OccupancyGrid  # noqa: E402
from testdata import synthetic  # noqa: E402

REPS, WARMUP = 10, 2


def same(a, b):
    return bool(torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.alpha, b.alpha))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reso", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--degrees", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--n-dirs", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=50.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake)
    net, meta, losses = trained_object(dev, args.steps)
    print(f"# trained {args.steps} steps, loss -> {sum(losses[-10:]) / 10:.4f}", flush=True)
    poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 45.0 * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                         for i in range(NVT)]).float().to(dev)
    focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
    cam = (W, H, focal, meta["z_near"], meta["z_far"])
    out = {"views": NVT, "image": [H, W], "precision": net.precision, "reps": REPS, "train_steps": args.steps, "threshold": args.threshold,
           "loss_last10": float(sum(losses[-10:]) / 10), "n_dirs": args.n_dirs, "rows": {}}
    BakedSHVolume.from_model(net, C1, C2, [16, 16, 16], degree=2, n_dirs=args.n_dirs)  # (warm-up: an SH bake is timed once)

    def bake_dense(reso, degree):
        if degree is None:
            return BakedVolume.from_model(net, C1, C2, reso)
        return BakedSHVolume.from_model(net, C1, C2, reso, degree=degree, n_dirs=args.n_dirs)

    for n in args.reso:
        reso = [n, n, n]
        total = n ** 3
        t_grid = [timed(lambda: OccupancyGrid.from_model(net, C1, C2, reso, args.threshold, dilate=1))[0] for _ in range(3)]
        grid = OccupancyGrid.from_model(net, C1, C2, reso, args.threshold, dilate=1)
        for degree in [None] + list(args.degrees):
            name = f"{n}^3 " + ("RGBA" if degree is None else f"L{degree}")
            bake_reps = 3 if degree is None else 1
            t_dense, t_sparse, dense, baked = [], [], None, None
            for _ in range(bake_reps):               # (the last bake of each kind is the one that is rendered)
                del dense, baked
                t, dense = timed(lambda: bake_dense(reso, degree))
                t_dense.append(t)
                t, baked = timed(lambda: SparseBakedVolume.from_model(net, C1, C2, reso, grid, degree=degree, n_dirs=args.n_dirs))
                t_sparse.append(t)
            tensor = dense.vol if degree is None else dense.coef
            per_point = tensor.view(total, *tensor.shape[3:])
            bake_equal = bool(torch.equal(baked.rows, per_point.index_select(0, baked.ids.long())))
            dense_thr = copy.copy(dense)          # the dense tensor marched against the foreign grid's bits
            dense_thr.occupancy = grid
            calls = {"dense_own": dense, "sparse_own": dense.sparse(), "dense_thr": dense_thr, "sparse_thr": baked}
            img = {k: v.render_views(poses, *cam, white_bkgd=True) for k, v in calls.items()}
            times = {k: [] for k in calls}
            for i in range(REPS + WARMUP):
                for k, v in calls.items():
                    t = timed(lambda: v.render_views(poses, *cam, white_bkgd=True))[0]
                    if i >= WARMUP:
                        times[k].append(t)
            row = {"dense_MB": round(tensor.numel() * 4 / 2 ** 20, 1), "bake_dense_ms": stats(t_dense), "grid_ms": stats(t_grid),
                   "bake_sparse_ms": stats(t_sparse), "bake_equal": bake_equal}
            for tag in ("own", "thr"):
                sp, dn = calls["sparse_" + tag], calls["dense_" + tag]
                row[tag] = {"kept": round(sp.n_rows / total, 5), "occupied_cells": round(dn.occupancy.occupied_fraction, 5),
                            "sparse_MB": round(sp.nbytes / 2 ** 20, 1), "dense_ms": stats(times["dense_" + tag]),
                            "sparse_ms": stats(times["sparse_" + tag]), "equal": same(img["sparse_" + tag], img["dense_" + tag])}
            out["rows"][name] = row
            print(f"# {name}: {json.dumps(row)}", flush=True)
            del dense, dense_thr, baked, calls, img, tensor, per_point
            torch.cuda.empty_cache()

    print(f"dense against sparse baked volumes, trained-like object (scene train, {args.steps} steps, loss -> {out['loss_last10']:.4f}), "
          f"precision {net.precision}; {NVT} views {H}x{W}; (median, min) ms of {REPS}; thr = OccupancyGrid.from_model at the volume's "
          f"resolution, threshold {args.threshold}, dilate 1")
    print("| volume | grid | occupied cells | M / P | dense MiB | sparse MiB | bake dense ms | grid ms | bake sparse ms | bake rows equal "
          "| dense skip ms | sparse ms | images equal |")
    print("|" + "---|" * 13)
    for name, row in out["rows"].items():
        for tag in ("own", "thr"):
            g = row[tag]
            bake = (row["grid_ms"], row["bake_sparse_ms"], row["bake_equal"]) if tag == "thr" else ("--", "--", "--")
            print(f"| {name} | {tag} | {g['occupied_cells']} | {g['kept']} | {row['dense_MB']} | {g['sparse_MB']} | {row['bake_dense_ms']} | "
                  f"{bake[0]} | {bake[1]} | {bake[2]} | {g['dense_ms']} | {g['sparse_ms']} | {g['equal']} |")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
