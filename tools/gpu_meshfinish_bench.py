#!/usr/bin/env python3
"""Mesh finishing (floater removal, vertex normals, vertex colours) on the GPU box: prints the block that goes into
profiles/meshfinish_notes.md and one JSON line.

One process.  The object is the trained-like one of tools/gpu_occupancy_bench.py (scene "train", procedural spheres, 400 Adam steps
through the HIP path: a network that leaves haze around the object).  Every timed call sits between two device events and ends in a
device synchronise; (median, min) of 10 after 2 warm-up calls.

  labelling   ops.grid_components (pnr_grid_components: init + union + flatten, sizes and counts included, outputs allocated by the
              call) at 128^3 and 256^3 on (a) the density of the object -- max of the coarse and the fine pass, as
              OccupancyGrid.from_model takes it -- at thresholds 50 and 5, (b) a Bernoulli field at p = 0.32, the 6-connected
              percolation threshold: one tortuous giant component next to thousands of small ones.
              The yardstick is the density evaluation of the same run (2 x 128^3 points): labelling at 128^3 should be small against it.
  floaters    recon.remove_floaters(keep_largest=1) end to end (labelling + the torch selection + the one host read)
  attributes  ops.grid_normals and recon.vertex_colors on the mesh of the 128^3 grid at threshold 5 with keep_largest=1
  render      render_views(..., occupancy=) with the threshold-5 grid built with and without keep_largest=1: hit fraction and ms
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_occupancy_bench as ob  # noqa: E402
from pixelnerf_amd import ops  # noqa: E402
from pixelnerf_amd.render import NeRFRenderer  # noqa: E402
from pixelnerf_amd.util import recon  # noqa: E402
from pixelnerf_amd.util.occupancy import OccupancyGrid  # noqa: E402
from testdata import synthetic  # noqa: E402

C1, C2 = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
W = H = 128
NVT, KC, KF, KFD = 8, 64, 128, 16
REPS, WARMUP = 10, 2


def timed_stats(fn, reps=REPS, warmup=WARMUP):
    times = [ob.timed(fn)[0] for _ in range(reps + warmup)][warmup:]
    return round(statistics.median(times), 3), round(min(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--no-render", action="store_true")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    net, meta, losses = ob.trained_object(dev, args.steps)
    out = {"precision": net.precision, "reps": REPS, "train_steps": args.steps, "loss_first10": float(np.mean(losses[:10])),
           "loss_last10": float(np.mean(losses[-10:])), "labelling": {}}

    fields = {}
    for n in (128, 256):
        reso = [n, n, n]
        with torch.no_grad():
            sig = recon.density_grid(net, C1, C2, reso, coarse=(True, False))[0].view(*reso)
        fields[n] = sig
        rng = np.random.default_rng(n)
        bern = torch.from_numpy((rng.random((n, n, n), dtype=np.float32) > 1 - 0.32).astype(np.float32)).to(dev)
        for name, f, thr in ((f"density{n}_thr50", sig, 50.0), (f"density{n}_thr5", sig, 5.0), (f"bernoulli{n}_p0.32", bern, 0.5)):
            labels, sizes, counts = ops.grid_components(f, thr)
            n_in, n_comp = counts.tolist()
            again = ops.grid_components(f, thr)
            out["labelling"][name] = {"inside": n_in, "components": n_comp, "largest": int(sizes.max()),
                                      "same_bytes_twice": bool(torch.equal(again[0], labels) and torch.equal(again[1], sizes)),
                                      "components_ms": timed_stats(lambda: ops.grid_components(f, thr)),
                                      "labels_only_ms": timed_stats(lambda: ops.grid_components(f, thr, want_sizes=False)),
                                      "remove_floaters_ms": timed_stats(lambda: recon.remove_floaters(f, thr, keep_largest=1))}
    out["density_eval_2x128^3_ms"] = timed_stats(lambda: recon.density_grid(net, C1, C2, [128] * 3, coarse=(True, False)), reps=3, warmup=1)
    out["density_eval_1x128^3_ms"] = timed_stats(lambda: recon.density_grid(net, C1, C2, [128] * 3, coarse=True), reps=3, warmup=1)

    # the mesh of the object alone and its attributes
    field, thr = fields[128], 5.0
    filtered, info = recon.remove_floaters(field, thr, keep_largest=1)
    scale = [2.0 / 128] * 3
    v, t = ops.marching_cubes(filtered, thr, c1=C1, scale=scale)
    v_all, t_all = ops.marching_cubes(field, thr, c1=C1, scale=scale)
    nrm = ops.grid_normals(filtered, v, C1, scale)
    out["mesh"] = {"threshold": thr, "info": info, "vertices": int(v.shape[0]), "triangles": int(t.shape[0]),
                   "vertices_unfiltered": int(v_all.shape[0]), "triangles_unfiltered": int(t_all.shape[0]),
                   "marching_cubes_ms": timed_stats(lambda: ops.marching_cubes(filtered, thr, c1=C1, scale=scale)),
                   "grid_normals_ms": timed_stats(lambda: ops.grid_normals(filtered, v, C1, scale)),
                   "vertex_colors_origin_ms": timed_stats(lambda: recon.vertex_colors(net, v), reps=5, warmup=1),
                   "vertex_colors_normal_ms": timed_stats(lambda: recon.vertex_colors(net, v, viewdirs="normal", normals=nrm), reps=5, warmup=1),
                   "zero_normals": int((nrm.abs().sum(dim=1) == 0).sum())}

    if not args.no_render:
        rend = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).to(dev).eval()
        poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 45.0 * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                             for i in range(NVT)]).float().to(dev)
        focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
        cam = (W, H, focal, meta["z_near"], meta["z_far"])

        def render(**kw):
            torch.manual_seed(11)
            return rend.render_views(net, poses, *cam, **kw)

        dense = render()
        out["render"] = {}
        for thr in (50.0, 5.0):
            for name, kw in (("all", {}), ("keep_largest_1", {"keep_largest": 1})):
                occ = OccupancyGrid.from_density(fields[128], C1, C2, thr, dilate=1, **kw)
                img = render(occupancy=occ)
                out["render"][f"thr{thr:g}_{name}"] = {
                    "occupied_fraction": round(occ.occupied_fraction, 5), "hit_fraction": round(img.n_hit / img.hit.numel(), 5),
                    "info": occ.info, "psnr_vs_dense": ob.psnr(img.rgb, dense.rgb),
                    "culled_ms": timed_stats(lambda: render(occupancy=occ), reps=5, warmup=1),
                    "sparse_ms": timed_stats(lambda: render(occupancy=occ, skip_empty=True), reps=5, warmup=1)}
        out["render"]["dense_ms"] = timed_stats(render, reps=3, warmup=1)

    lines = [f"mesh finishing, trained-like object (scene train, {args.steps} steps, loss {out['loss_first10']:.4f} -> {out['loss_last10']:.4f}), "
             f"precision {net.precision}; (median, min) ms of {REPS}, device events",
             f"  density evaluation, 2 x 128^3 points: {out['density_eval_2x128^3_ms']}; 1 x 128^3: {out['density_eval_1x128^3_ms']}"]
    for name, g in out["labelling"].items():
        lines.append(f"  [{name}] " + ", ".join(f"{k} {v}" for k, v in g.items()))
    lines.append("  [mesh] " + ", ".join(f"{k} {v}" for k, v in out["mesh"].items()))
    for name, g in out.get("render", {}).items():
        lines.append(f"  [render {name}] " + (", ".join(f"{k} {v}" for k, v in g.items()) if isinstance(g, dict) else str(g)))
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
