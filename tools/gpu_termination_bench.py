#!/usr/bin/env python3
"""Early ray termination on a trained-like object, on the GPU box: prints the table that goes into profiles/termination_notes.md and
one JSON line.

Scene and shapes are tools/gpu_occupancy_bench.py's: the procedural scene "train" trained for 400 Adam steps through the HIP path,
object 0, 8 views at 128 x 128, 64 coarse + 128 fine (16 depth) samples per ray, white background, default precision.

Variants: the call without `terminate`, and terminate = eps in {1e-2, 1e-3} x terminate_stages in {2, 4, 8} -- each once without a
grid (yardstick: the dense render_views call of the same run) and once with the threshold-50 grid + skip_empty (yardstick: that call
without `terminate`, same run).

Timing: ALL variants alternate in one process after two warm-up rounds, every call between two device events ended by a device
synchronise; (median, min) of REPS.  Per row: evaluated share of the fine samples, share of the rendered rays that stop, ms, the ms
of marking + compaction + placement alone (the stages of that row replayed on the call's own fine samples and outputs, with the
network left out), PSNR and max |d rgb| against the same run's image without `terminate`."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_occupancy_bench import C1, C2, H, KC, KF, KFD, NVT, RESO, W, psnr, stats, timed, trained_object  # noqa: E402
from pixelnerf_amd import ops  # noqa: E402
from pixelnerf_amd.render import NeRFRenderer  # noqa: E402
from pixelnerf_amd.render.accel import Accel, StagedPass  # noqa: E402
from pixelnerf_amd.util.occupancy import OccupancyGrid  # noqa: E402
from testdata import synthetic  # noqa: E402

REPS, WARMUP = 10, 2
EPS, STAGES = (1e-2, 1e-3), (2, 4, 8)


class Machinery(StagedPass):
    """the product's staged pass with the network left out: marking, the pair closure, compaction with its host read, expansion and
    placement remain"""

    def network(self, packed, tables, slot, rays, z):
        return torch.zeros(z.shape + (4,), device=z.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=REPS)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    net, meta, losses = trained_object(dev, args.steps)
    rend = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).to(dev).eval()
    poses = torch.stack([meta["pre"] @ synthetic.pose_spherical(meta["tgt"][0] + 45.0 * i, meta["tgt"][1] - 3.0 * i, meta["radius"])
                         for i in range(NVT)]).float().to(dev)
    focal = (meta["focal"][0] * W / meta["W"], meta["focal"][1] * H / meta["H"])
    cam = (W, H, focal, meta["z_near"], meta["z_far"])
    grid = OccupancyGrid.from_model(net, C1, C2, RESO, 50.0, dilate=1)

    def render(seed=11, **kw):
        torch.manual_seed(seed)
        return rend.render_views(net, poses, *cam, **kw)

    rows = {}
    for gname, gkw in (("no_grid", {}), ("thr50_skip_empty", dict(occupancy=grid, skip_empty=True))):
        rows[(gname, None, None)] = dict(gkw)
        for eps in EPS:
            for S in STAGES:
                rows[(gname, eps, S)] = dict(gkw, terminate=eps, terminate_stages=S)

    # one pass for the images, the counts and the inputs of the machinery replay
    info, base = {}, {}
    seen = {}
    real = ops.composite

    def spy(rays, z, rgbsigma, *a, **k):
        seen["last"] = (rays, z, rgbsigma)
        return real(rays, z, rgbsigma, *a, **k)

    for key, kw in rows.items():
        gname, eps, S = key
        ops.composite = spy
        try:
            img = render(**kw)
        finally:
            ops.composite = real
        if eps is None:
            base[gname] = img
            info[key] = {}
            continue
        st = rend.last_terminate_stats
        ref = base[gname]
        info[key] = {"evaluated_share": round(st["evaluated"] / max(st["total"], 1), 5), "stopped_share": round(st["stopped_rays"] / max(st["rays"], 1), 5),
                     "rays": st["rays"], "stages": st["stages"], "psnr": psnr(img.rgb, ref.rgb), "max_abs_rgb": float((img.rgb - ref.rgb).abs().max()),
                     "replay": seen["last"], "accel": Accel.parse(rend, kw.get("occupancy"), False, "occupancy" in kw, eps, S)}
    times = {key: [] for key in rows}
    mach = {key: [] for key in rows if key[1] is not None}
    for i in range(args.reps + WARMUP):  # every variant in every round
        for key, kw in rows.items():
            t = timed(lambda: render(**kw))[0]
            if i >= WARMUP:
                times[key].append(t)
        for key in mach:
            rays, z, rs = info[key]["replay"]  # the marks are the call's own: made on the outputs it ended with
            stages = Machinery(rend, net, rays, None, False, info[key]["accel"])
            t = timed(lambda: stages.terminated(None, None, z, 1, grid.mark_samples(rays, z) if key[0] != "no_grid" else None, marks_from=rs))[0]
            if i >= WARMUP:
                mach[key].append(t)

    out = {"views": NVT, "image": [H, W], "samples": [KC, KF, KFD], "precision": net.precision, "reps": args.reps, "train_steps": args.steps,
           "loss_first10": float(statistics.mean(losses[:10])), "loss_last10": float(statistics.mean(losses[-10:])),
           "grid_occupied_fraction": round(grid.occupied_fraction, 5), "rows": []}
    lines = [f"early termination, trained-like object (scene train, {args.steps} steps), precision {net.precision}, {NVT} views {H}x{W}, "
             f"{KC}+{KF} ({KFD} depth) samples; (median, min) ms of {args.reps}",
             "| grid | eps | S | evaluated share | stopped share | ms (median, min) | vs no terminate | machinery ms | PSNR dB | max abs d rgb |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for key in rows:
        gname, eps, S = key
        ms = stats(times[key])
        row = {"grid": gname, "eps": eps, "stages": S, "ms": ms}
        if eps is None:
            lines.append(f"| {gname} | - | - | 1 | 0 | {ms} | 1.000 | - | - | - |")
        else:
            i = info[key]
            ratio = round(ms[0] / stats(times[(gname, None, None)])[0], 3)
            row.update({k: i[k] for k in ("evaluated_share", "stopped_share", "rays", "stages", "psnr", "max_abs_rgb")},
                       machinery_ms=stats(mach[key]), ratio_to_no_terminate=ratio)
            lines.append(f"| {gname} | {eps:g} | {S} | {i['evaluated_share']:.4f} | {i['stopped_share']:.4f} | {ms} | {ratio:.3f} | "
                         f"{row['machinery_ms']} | {i['psnr']} | {i['max_abs_rgb']:.2e} |")
        out["rows"].append(row)
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
