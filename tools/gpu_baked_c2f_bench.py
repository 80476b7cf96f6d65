#!/usr/bin/env python3
"""Coarse-to-fine baked fits on the trained-like object of tools/gpu_baked_bench.py, on the GPU box: prints the tables that go into
profiles/baked_notes.md ("Coarse to fine") and one JSON line.

The object, the cameras, the in-box renders of the network and the held-out views are tools/gpu_baked_fit_bench.py's: 8 held-IN views
of 128 x 128 (131 072 rays), 8 held-OUT views half-way between them, white background.  Three parts (--only picks one):

  visibility   per volume (RGBA and degree 2 at 65^3 and 129^3, dense and sparse under an OccupancyGrid of its sigma at threshold 50,
               dilate 1): the forward march, the stored-value backward and the visibility pass on the SAME rays, back to back,
               step = the cell edge.  vis/fwd and vis/bwd are the price of the pass in forwards and against the backward; `seen`
               is the fraction of stored rows with visibility > 0.  Run the tool a second time with PIXELNERF_HIP_LIB naming a
               library built with -DPNR_VIS_NO_FILTER (tools/build_variant.sh) for the bare atomic.
  resample     65^3 -> 129^3 -> 257^3, RGBA and degree 2, dense and sparse: ops.baked_resample alone, and GB/s against the bytes it
               must move (the source once, the destination once; sparse: the rows, the index and the ids).
  fit          150 steps at 65^3 then 150 at 129^3 (util.bake.fit_coarse_to_fine, with and without pruning) against 300 steps at
               129^3 from a direct bake: wall time (the bakes apart), PSNR on the held-in and the held-out views, bytes.

Timing: after warm-up the calls ALTERNATE in one process, every call between two device events; (median, min) of REPS."""
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


def sigma_of(volume):
    return volume.vol[..., 3].float().contiguous() if volume.degree is None else volume.sigma_bound()


def bake_volume(net, kind, n, n_dirs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kind == "RGBA":
        v = bake.BakedVolume.from_model(net, C1, C2, [n, n, n])
    else:
        v = bake.BakedSHVolume.from_model(net, C1, C2, [n, n, n], degree=2, n_dirs=n_dirs)
    torch.cuda.synchronize()
    return v, round(time.perf_counter() - t0, 2)


def table(title, cols, rows):
    print(title)
    print("| " + " | ".join(cols) + " |")
    print("|" + "---|" * len(cols))
    for r in rows:
        print("| " + " | ".join(str(r[c]) for c in cols) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--only", choices=["visibility", "resample", "fit"], default=None)
    ap.add_argument("--n-dirs", type=int, default=32)
    ap.add_argument("--fit-steps", type=int, default=150)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--prune-threshold", type=float, default=1e-3)
    ap.add_argument("--kinds", nargs="+", default=["RGBA", "L2"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")  # (the fake-view-direction warning of every bake)
    net, meta, losses = trained_object(dev, args.steps)

    def cameras(offset):
        return torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + offset + 45.0 * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                            for i in range(NVT)]).float().to(dev)

    poses = {"in": cameras(0.0), "out": cameras(22.5)}
    focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
    cam = (W, H, focal, meta["z_near"], meta["z_far"])
    rays = util.gen_rays(poses["in"], *cam).reshape(-1, 8).contiguous()
    R = rays.shape[0]
    out = {"views": NVT, "image": [H, W], "rays": R, "precision": net.precision, "reps": REPS, "train_steps": args.steps,
           "library": os.environ.get("PIXELNERF_HIP_LIB", "product")}
    want = lambda part: args.only in (None, part)
    volumes = {}

    def volume(kind, n):
        if (kind, n) not in volumes:
            volumes[(kind, n)] = bake_volume(net, kind, n, args.n_dirs)
        return volumes[(kind, n)]

    # ---- visibility against the forward and the stored backward
    if want("visibility"):
        d_rgb = torch.randn((R, 3), generator=torch.Generator().manual_seed(1)).to(dev)
        rows = []
        for kind in args.kinds:
            for n in (65, 129):
                dense, _ = volume(kind, n)
                sparse = dense.sparse(OccupancyGrid.from_density(sigma_of(dense), C1, C2, 50.0, dilate=1))
                for layout, v in (("dense", dense), ("sparse", sparse)):
                    is_sparse = layout == "sparse"
                    stored, step = v._stored(), min(v.cell_size)
                    bits = v.occupancy.bits if is_sparse else None
                    index = v.index if is_sparse else None
                    grad = torch.zeros_like(stored)
                    vis = torch.zeros(v._vis_shape(), device=dev)
                    fwd = lambda: v.render(rays, white_bkgd=True, skip=is_sparse)
                    bwd = lambda: ops.baked_render_backward(rays, stored, v.degree, v.reso, C1, C2, step, d_rgb=d_rgb, bits=bits, index=index,
                                                            white_bkgd=True, out=grad)
                    see = lambda: ops.baked_visibility(rays, stored, v.degree, v.reso, C1, C2, step, bits=bits, index=index, out=vis)
                    tf, tb, tv, tv0 = [], [], [], []
                    for i in range(REPS + WARMUP):
                        a, b = timed(fwd)[0], timed(bwd)[0]
                        c = timed(see)[0]          # into a field that already holds the maxima: nearly every proposal is filtered
                        vis.zero_()
                        c0 = timed(see)[0]         # into a zeroed field: the first call of a run
                        if i >= WARMUP:
                            tf.append(a), tb.append(b), tv.append(c), tv0.append(c0)
                    rows.append({"volume": f"{n}^3 {kind} {layout}", "MB": round(v.nbytes / 2 ** 20, 1), "fwd_ms": stats(tf), "bwd_ms": stats(tb),
                                 "vis_zeroed_ms": stats(tv0), "vis_again_ms": stats(tv), "vis/fwd": round(stats(tv0)[0] / stats(tf)[0], 2),
                                 "vis/bwd": round(stats(tv0)[0] / stats(tb)[0], 3), "seen": round(float((vis > 0).float().mean()), 4),
                                 "vis_max": round(float(vis.max()), 4)})
                    del grad, vis
                del sparse
                torch.cuda.empty_cache()
        out["visibility"] = rows
        table(f"visibility against the forward march and the stored backward; {R} rays ({NVT} views {H}x{W}); (median, min) of {REPS} in ms; "
              f"library: {out['library']}", list(rows[0]), rows)

    # ---- resample: 65 -> 129 -> 257
    if want("resample"):
        rows = []
        for kind in args.kinds:
            dense, _ = volume(kind, 65)
            sparse = dense.sparse(OccupancyGrid.from_density(sigma_of(dense), C1, C2, 50.0, dilate=1))
            for layout, v in (("dense", dense), ("sparse", sparse)):
                for n in (129, 257):
                    new = (n, n, n)
                    if layout == "dense":
                        call = lambda: ops.baked_resample(v._stored(), v.degree, v.reso, new)
                        moved = lambda o: v._stored().numel() * 4 + o.numel() * 4
                    else:
                        fine = v.resample(new)
                        ids = fine.ids
                        call = lambda: ops.baked_resample(v.rows, v.degree, v.reso, new, index=v.index, ids_dst=ids)
                        moved = lambda o: v.rows.numel() * 4 + v.index.numel() * 4 + ids.numel() * 4 + o.numel() * 4
                    times = []
                    for i in range(REPS + WARMUP):
                        ms, o = timed(call)
                        if i >= WARMUP:
                            times.append(ms)
                    nbytes = moved(o)
                    rows.append({"volume": f"{v.reso[0]}^3 -> {n}^3 {kind} {layout}", "moved_MB": round(nbytes / 2 ** 20, 1), "ms": stats(times),
                                 "GB/s": round(nbytes / 1e9 / (stats(times)[0] / 1e3), 1)})
                    del o
                    if n == 129:   # the next step starts from this result
                        v = fine if layout == "sparse" else type(v)(call(), C1, C2)
                    torch.cuda.empty_cache()
        out["resample"] = rows
        table(f"ops.baked_resample; (median, min) of {REPS} in ms; GB/s against the bytes it must move", list(rows[0]), rows)
        volumes = {k: v for k, v in volumes.items() if k[1] <= 129}
        torch.cuda.empty_cache()

    # ---- the fit: coarse to fine against a direct fine fit
    if want("fit"):
        rend = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).to(dev).eval()
        full = OccupancyGrid.from_density(torch.ones((128, 128, 128), device=dev), C1, C2, 0.5, dilate=0)
        box = {}
        for k, p in poses.items():
            torch.manual_seed(11)
            box[k] = rend.render_views(net, p, *cam, occupancy=full, skip_empty=True).rgb[0].reshape(NVT, H, W, 3)
        target = box["in"].reshape(-1, 3)
        rows = []

        def report(name, v, secs, bake_s):
            q = {k: psnr(v.render_views(p, *cam, white_bkgd=True).rgb, box[k]) for k, p in poses.items()}
            rows.append({"run": name, "class": type(v).__name__, "bake_s": bake_s, "fit_s": round(secs, 2), "psnr_in": q["in"], "psnr_out": q["out"],
                         "MB": round(v.nbytes / 2 ** 20, 1)})

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return r, time.perf_counter() - t0

        kw = dict(lr=args.lr, batch=args.batch, seed=0, white_bkgd=True)
        for kind in args.kinds:
            coarse, bake65 = volume(kind, 65)
            fine, bake129 = volume(kind, 129)
            report(f"{kind}: bake 65^3", coarse, 0.0, bake65)
            report(f"{kind}: bake 129^3", fine, 0.0, bake129)
            (v, _), secs = clock(lambda: bake.fit(fine, rays, target, steps=2 * args.fit_steps, **kw))
            report(f"{kind}: {2 * args.fit_steps} steps at 129^3", v, secs, bake129)
            stages = [(None, args.fit_steps), (129, args.fit_steps)]
            (v, _), secs = clock(lambda: bake.fit_coarse_to_fine(coarse, rays, target, stages, **kw))
            report(f"{kind}: {args.fit_steps} at 65^3 + {args.fit_steps} at 129^3", v, secs, bake65)
            prune = dict(threshold=args.prune_threshold, dilate=1)
            (v, _), secs = clock(lambda: bake.fit_coarse_to_fine(coarse, rays, target, stages, prune=prune, **kw))
            report(f"{kind}: the same, pruned at {args.prune_threshold}", v, secs, bake65)
            del v
            torch.cuda.empty_cache()
        out["fit"] = rows
        table(f"coarse to fine: Adam lr {args.lr}, batches of {args.batch} rays of the held-in views, target = the network's in-box render; "
              "fit_s: wall time without the bake", list(rows[0]), rows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
