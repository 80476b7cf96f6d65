#!/usr/bin/env python3
"""Occupancy-grid ray culling on a trained-like object, on the GPU box: prints the block that goes into
profiles/occupancy_notes.md and one JSON line.

A random-init network is fog: it has no empty space to cull.  So the network and the feature grid are first trained as
tests/test_hip_trained_weights.py trains them (procedural spheres, 400 Adam steps through the HIP path, scene "train"), and object 0
is rendered: 8 views at 128 x 128, 64 coarse + 128 fine (16 depth) samples per ray, white background.

Grids: OccupancyGrid.from_model at 128^3 over [-1,1]^3, dilate 1, with the reference's default iso-level 50 (src/util/recon.py:17) as
threshold and with a tenth of it; and a FULL grid (every cell occupied), whose culled render does all the dense render's work plus
the culling machinery -- its excess over the dense render is the overhead at a 100 % hit fraction.

The `sparse` row is the culled call with skip_empty=True: the network runs only on the samples in occupied cells (kept share per
pass from NeRFRenderer.last_skip_stats; psnr_all_sparse against the dense image of the same seed), and skip_machinery_ms is mark +
compact + expand alone on the hit rays, once at the coarse and once at the fine pass's shape (stratified stand-in positions).

Timing: dense and culled calls ALTERNATE in one process after warm-up, every call between two device events ended by a device
synchronise; median and min of REPS.  Reported per grid: hit fraction, ms per call dense / culled / culled with tighten, the
expectation dense x hit fraction + clip + gather/scatter, PSNR of the culled image against the dense one over all pixels and over
the missed pixels alone.  Separately: from_model split into density evaluation and build, and clip_rays alone.
With --trace-only the timed part is skipped and a few calls of each kind run once (for a kernel trace of its own)."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pixelnerf_amd import ops  # noqa: E402
from pixelnerf_amd.model import make_model  # noqa: E402
from pixelnerf_amd.render import NeRFRenderer  # noqa: E402
from pixelnerf_amd.util import recon  # noqa: E402
from pixelnerf_amd.util.conf import default_model_conf  # noqa: E402
from pixelnerf_amd.util.occupancy import OccupancyGrid  # noqa: E402
from testdata import procedural, synthetic  # noqa: E402

RESO, C1, C2 = [128, 128, 128], [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
W = H = 128
NVT, KC, KF, KFD = 8, 64, 128, 16
REPS, WARMUP = 10, 2


def install(net, scene, lat, dev):
    net.encoder.latent = lat
    ls = torch.tensor([lat.shape[-1], lat.shape[-2]], dtype=torch.float32, device=dev)
    net.encoder.latent_scaling = ls / (ls - 1) * 2.0
    net.poses, net.image_shape = scene["poses"].to(dev), scene["image_shape"].to(dev)
    net.focal, net.c = scene["focal"].to(dev), scene["c"].to(dev)
    net.num_objs, net.num_views_per_obj = scene["SB"], scene["NS"]


def trained_object(dev, steps):
    """the training of tests/test_hip_trained_weights.py (scene "train"); -> (eval net that encoded object 0, meta, losses)"""
    scene, meta = synthetic.make_scene("train")
    SB = scene["SB"]
    net = make_model(default_model_conf()).to(dev).train()
    net.mlp_coarse.load_state_dict(synthetic.make_mlp_params(11))
    net.mlp_fine.load_state_dict(synthetic.make_mlp_params(12))
    rs = np.random.RandomState(5)
    low = torch.from_numpy(rs.randn(scene["latent"].shape[0], 512, 4, 4).astype(np.float32))
    lat0 = torch.nn.functional.interpolate(low, size=tuple(scene["latent"].shape[-2:]), mode="bilinear", align_corners=True) * 0.5
    lat = lat0.to(dev).clone().requires_grad_(True)
    install(net, scene, lat, dev)
    pools = []
    for o in range(SB):
        poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 40.0 * o + dt, meta["tgt"][1] + dp, meta["radius"])
                             for dt, dp in ((0.0, 0.0), (55.0, -10.0), (-70.0, 8.0))])
        pools.append(synthetic.gen_rays(poses, meta["W"], meta["H"], meta["focal"], meta["z_near"], meta["z_far"], c=meta["c"]).reshape(-1, 8))
    pool = torch.stack(pools).to(dev)
    centres, radii, tints = procedural.sphere_params(SB, seed=4)
    targets = procedural.sphere_targets(pool, centres, radii, tints)
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).to(dev).train()
    torch.manual_seed(7)
    losses = procedural.fit(net, rend, lat, pool, targets, steps=steps, rays_per_obj=128, lr=5e-4, seed=1)
    NS = scene["NS"]
    one = dict(scene, SB=1, latent=lat.detach()[:NS].contiguous(), poses=scene["poses"][:NS].contiguous())
    ev = make_model(default_model_conf()).to(dev).eval()
    ev.mlp_coarse.load_state_dict(net.mlp_coarse.state_dict())
    ev.mlp_fine.load_state_dict(net.mlp_fine.state_dict())
    for p in ev.parameters():
        p.requires_grad_(False)
    install(ev, one, one["latent"], dev)
    return ev, meta, losses


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(times):
    return round(statistics.median(times), 3), round(min(times), 3)


def psnr(a, b, mask=None):
    d = (a.clamp(0, 1) - b.clamp(0, 1)).double() ** 2
    if mask is not None:
        if not bool(mask.any()):
            return None
        d = d[mask]
    mse = float(d.mean())
    return float("inf") if mse == 0.0 else round(-10.0 * math.log10(mse), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    net, meta, losses = trained_object(dev, args.steps)
    rend = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).to(dev).eval()
    poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 45.0 * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                         for i in range(NVT)]).float().to(dev)
    focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
    cam = (W, H, focal, meta["z_near"], meta["z_far"])
    out = {"reso": RESO, "views": NVT, "image": [H, W], "samples": [KC, KF, KFD], "precision": net.precision, "reps": REPS,
           "train_steps": args.steps, "loss_first10": float(np.mean(losses[:10])), "loss_last10": float(np.mean(losses[-10:]))}

    def render(seed=11, **kw):
        torch.manual_seed(seed)
        return rend.render_views(net, poses, *cam, **kw)

    # the grids, and what they cost
    total = RESO[0] * RESO[1] * RESO[2]
    with torch.no_grad():
        sig = recon.density_grid(net, C1, C2, RESO, coarse=(True, False))[0]
    out["sigma_max"] = float(sig.max())
    out["sigma_share_above"] = {str(t): float((sig > t).float().mean()) for t in (50.0, 5.0, 0.0)}
    grids = {"thr50": OccupancyGrid.from_model(net, C1, C2, RESO, 50.0, dilate=1),
             "thr5": OccupancyGrid.from_model(net, C1, C2, RESO, 5.0, dilate=1),
             "full": OccupancyGrid.from_density(torch.ones(RESO, device=dev), C1, C2, 0.5, dilate=0)}
    rays = ops.gen_rays(poses, W, H, focal, meta["z_near"], meta["z_far"]).reshape(-1, 8)
    if not args.trace_only:
        field = sig.view(*RESO)
        t_density = [timed(lambda: recon.density_grid(net, C1, C2, RESO, coarse=(True, False)))[0] for _ in range(3)]
        t_build = [timed(lambda: ops.occupancy_build(field, 50.0, 1))[0] for _ in range(REPS + WARMUP)][WARMUP:]
        t_build4 = [timed(lambda: ops.occupancy_build(field, 50.0, 4))[0] for _ in range(REPS + WARMUP)][WARMUP:]
        t_clip = [timed(lambda: grids["thr5"].clip_rays(rays))[0] for _ in range(REPS + WARMUP)][WARMUP:]
        t_rays = [timed(lambda: ops.gen_rays(poses, W, H, focal, meta["z_near"], meta["z_far"]))[0] for _ in range(REPS + WARMUP)][WARMUP:]
        out.update(density_points=2 * total, density_ms=stats(t_density), build_dilate1_ms=stats(t_build), build_dilate4_ms=stats(t_build4),
                   clip_rays_ms=stats(t_clip), gen_rays_ms=stats(t_rays), rays=int(rays.shape[0]))

    dense_img = render()
    out["grids"] = {}
    for name, occ in grids.items():
        culled, tight = render(occupancy=occ), render(occupancy=occ, tighten=True)
        sparse = render(occupancy=occ, skip_empty=True)
        skip = dict(rend.last_skip_stats)
        hit = culled.hit
        g = {"occupied_fraction": round(occ.occupied_fraction, 5), "hit_fraction": round(culled.n_hit / hit.numel(), 5),
             "kept_pixels_bit_equal": bool(torch.equal(culled.rgb[hit], dense_img.rgb[hit])),
             "psnr_all": psnr(culled.rgb, dense_img.rgb), "psnr_missed": psnr(culled.rgb, dense_img.rgb, ~hit),
             "psnr_all_tighten": psnr(tight.rgb, dense_img.rgb), "psnr_missed_tighten": psnr(tight.rgb, dense_img.rgb, ~hit),
             "max_abs_missed": float((culled.rgb - dense_img.rgb)[~hit].abs().max()) if bool((~hit).any()) else None,
             "psnr_all_sparse": psnr(sparse.rgb, dense_img.rgb), "psnr_sparse_vs_culled": psnr(sparse.rgb, culled.rgb),
             "kept_share_coarse": round(skip["coarse"][0] / max(skip["coarse"][1], 1), 5),
             "kept_share_fine": round(skip["fine"][0] / max(skip["fine"][1], 1), 5), "kept_samples": [skip["coarse"], skip["fine"]]}
        if not args.trace_only:
            td, tc, tt, tsp = [], [], [], []
            for i in range(REPS + WARMUP):  # dense / culled / tightened / sparse alternate
                a = timed(render)[0]
                b = timed(lambda: render(occupancy=occ))[0]
                c = timed(lambda: render(occupancy=occ, tighten=True))[0]
                d = timed(lambda: render(occupancy=occ, skip_empty=True))[0]
                if i >= WARMUP:
                    td.append(a), tc.append(b), tt.append(c), tsp.append(d)
            # gather / scatter of the hit rows alone: index_select of the rays + index_copy_ of rgb and depth (+ the noise tensors' draw)
            idx = torch.nonzero(hit.reshape(-1)).flatten()
            full_rgb, full_d = torch.ones((rays.shape[0], 3), device=dev), torch.zeros((rays.shape[0],), device=dev)
            part_rgb, part_d = torch.rand((idx.numel(), 3), device=dev), torch.rand((idx.numel(),), device=dev)

            def plumbing():
                torch.nonzero(hit.reshape(-1)).flatten()
                rays.index_select(0, idx)
                ops.philox_noise_ids(idx, KC, KF, KFD, 1)
                full_rgb.index_copy_(0, idx, part_rgb)
                full_d.index_copy_(0, idx, part_d)
            tp = [timed(plumbing)[0] for _ in range(REPS + WARMUP)][WARMUP:]
            # mark + compact + expand alone (each pass's host read of the count included), on the hit rays at both passes' shapes
            sub = rays.index_select(0, idx)
            z_pass = [ops.sample_coarse(sub, torch.rand((idx.numel(), k), device=dev)) for k in (KC, KC + KF)] if idx.numel() else []

            def machinery():
                for z in z_pass:
                    index, _, _, m = ops.compact_samples(occ.mark_samples(sub, z), sub, z)
                    ops.expand_rgbsigma(index, torch.zeros((m, 4), device=dev) if m else None, z.numel())
            tm = [timed(machinery)[0] for _ in range(REPS + WARMUP)][WARMUP:]
            g.update(dense_ms=stats(td), culled_ms=stats(tc), tighten_ms=stats(tt), sparse_ms=stats(tsp), gather_noise_scatter_ms=stats(tp),
                     skip_machinery_ms=stats(tm))
            g["speedup_sparse_vs_dense"] = round(g["dense_ms"][0] / g["sparse_ms"][0], 3)
            g["speedup_sparse_vs_culled"] = round(g["culled_ms"][0] / g["sparse_ms"][0], 3)
            expect = g["dense_ms"][0] * g["hit_fraction"] + out["clip_rays_ms"][0] + out["gen_rays_ms"][0] + g["gather_noise_scatter_ms"][0]
            g["expected_ms"] = round(expect, 3)
            g["overhead_ms"] = round(g["culled_ms"][0] - expect, 3)
            g["speedup"] = round(g["dense_ms"][0] / g["culled_ms"][0], 3)
        out["grids"][name] = g

    lines = [f"occupancy culling, trained-like object (scene train, {args.steps} steps, loss {out['loss_first10']:.4f} -> {out['loss_last10']:.4f}), "
             f"precision {net.precision}",
             f"  {NVT} views {H}x{W}, {KC}+{KF} ({KFD} depth) samples, grid {RESO} dilate 1; sigma max {out['sigma_max']:.1f}, share of grid points "
             f"above 50 / 5 / 0: " + " / ".join(f"{out['sigma_share_above'][k]:.4f}" for k in ("50.0", "5.0", "0.0"))]
    if not args.trace_only:
        lines += [f"  (median, min) ms of {REPS}: density evaluation of 2 x {total} points {out['density_ms']}, build dilate 1 {out['build_dilate1_ms']}, "
                  f"dilate 4 {out['build_dilate4_ms']}, clip_rays of {out['rays']} rays {out['clip_rays_ms']}, gen_rays {out['gen_rays_ms']}"]
    for name, g in out["grids"].items():
        lines.append(f"  [{name}] " + ", ".join(f"{k} {v}" for k, v in g.items()))
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
