#!/usr/bin/env python3
"""Mesh extraction (util.recon.marching_cubes) at 128^3 on the sn64 scene, on the GPU box: writes profiles/mesh_extract.txt.

Timed separately, device events, median of 20 runs after 3 warm-up runs:
  density   the chunk loop of recon.marching_cubes: pnr_gen_grid_points + net(xyz, coarse=True, viewdirs=) per chunk of
            eval_batch_size points, sigma gathered into one device grid (2 097 152 points)
  cubes     pnr_marching_cubes_count + pnr_marching_cubes_emit on that grid with the outputs allocated beforehand (the kernels
            alone), and ops.marching_cubes end to end (allocations and the one host read of the three counts included)
The level is the median of the grid's positive densities, so that the surface is not empty whatever the seeded network gives.
One JSON line at the end."""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pixelnerf_amd import _lib, ops  # noqa: E402
from pixelnerf_amd.model import make_model  # noqa: E402
from pixelnerf_amd.util.conf import default_model_conf  # noqa: E402
from testdata import synthetic  # noqa: E402

RESO, C1, C2 = [128, 128, 128], [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
REPS, WARMUP = 20, 3


def sn64_net(dev):
    scene, _ = synthetic.make_scene("sn64")
    net = make_model(default_model_conf()).to(dev).eval()
    net.mlp_coarse.load_state_dict(synthetic.make_mlp_params(11))
    net.mlp_fine.load_state_dict(synthetic.make_mlp_params(12))
    lat = scene["latent"].to(dev)
    net.encoder.latent = lat
    ls = torch.tensor([lat.shape[-1], lat.shape[-2]], dtype=torch.float32, device=dev)
    net.encoder.latent_scaling = ls / (ls - 1) * 2.0
    net.poses, net.image_shape = scene["poses"].to(dev), scene["image_shape"].to(dev)
    net.focal, net.c = scene["focal"].to(dev), scene["c"].to(dev)
    net.num_objs, net.num_views_per_obj = scene["SB"], scene["NS"]
    return net


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(statistics.median(times), 4), round(min(times), 4)


def main():
    dev = torch.device("cuda:0")
    net = sn64_net(dev)
    total = RESO[0] * RESO[1] * RESO[2]
    sigmas = torch.empty((total,), dtype=torch.float32, device=dev)
    out = {"reso": RESO, "points": total, "precision": net.precision, "reps": REPS}

    def density(chunk):
        with torch.no_grad():
            for first in range(0, total, chunk):
                n = min(chunk, total - first)
                xyz, vd = ops.gen_grid_points(C1, C2, RESO, first, n, device=dev)
                sigmas[first:first + n] = net(xyz[None], coarse=True, viewdirs=vd[None])[0, :, 3]

    for chunk in (100000, total):  # the reference's default chunk, and one call
        out[f"density_ms_chunk_{chunk}"] = median_ms(lambda: density(chunk))
    field = sigmas.view(*RESO)
    pos = sigmas[sigmas > 0]
    iso = float(pos.median()) if pos.numel() else 0.0
    lib = _lib.load()
    ws = torch.empty((lib.pnr_marching_cubes_workspace_bytes(*RESO) // 8,), dtype=torch.int64, device=dev)
    counts = torch.empty((3,), dtype=torch.int32, device=dev)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    _lib.check(lib.pnr_marching_cubes_count(field.data_ptr(), *RESO, iso, ws.data_ptr(), counts.data_ptr(), st()), "count")
    nv, nt, nonfinite = counts.tolist()
    verts = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
    tris = torch.empty((max(nt, 1), 3), dtype=torch.int32, device=dev)
    lo, sc = (ctypes.c_float * 3)(*C1), (ctypes.c_float * 3)(*[2.0 / r for r in RESO])
    count = lambda: _lib.check(lib.pnr_marching_cubes_count(field.data_ptr(), *RESO, iso, ws.data_ptr(), counts.data_ptr(), st()), "count")  # noqa: E731
    emit = lambda: _lib.check(lib.pnr_marching_cubes_emit(field.data_ptr(), *RESO, iso, lo, sc, ws.data_ptr(), verts.data_ptr(),  # noqa: E731
                                                          tris.data_ptr(), st()), "emit")
    out.update(isosurface=iso, vertices=nv, triangles=nt, nonfinite=nonfinite, count_ms=median_ms(count), emit_ms=median_ms(emit),
               count_emit_ms=median_ms(lambda: (count(), emit())),
               ops_marching_cubes_ms=median_ms(lambda: ops.marching_cubes(field, iso, c1=C1, scale=[2.0 / r for r in RESO])))
    lines = [f"mesh extraction at {RESO} on the sn64 scene, precision {net.precision}; (median, min) ms of {REPS} runs, device events",
             f"  surface at sigma = {iso:.4f}: {nv} vertices, {nt} triangles, {nonfinite} non-finite values"]
    lines += [f"  {k:32s} {v}" for k, v in out.items() if k.endswith("_ms") or k.startswith("density_ms")]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_extract.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
