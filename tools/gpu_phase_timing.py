#!/usr/bin/env python3
"""Per-phase time breakdown of the fused network kernel (wave 0 of workgroup 0).  The phase-timing entries exist in variant
builds only:  tools/build_variant.sh timing && PIXELNERF_HIP_LIB=build/libpnr_timing.so PIXELNERF_ALLOW_VARIANT=1 python tools/gpu_phase_timing.py"""
import ctypes, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pixelnerf_amd import _lib, ops
from testdata import synthetic

PHASES = ["sync_top", "geometry", "gather", "gemm_in_z0", "bar1", "write_x", "bar2", "gemm_fc0", "bar3", "write_net",
          "bar4", "gemm_fc1_z", "lin_out", "bar_out", "final", "table", "own_bias", "own_prologue", "own_ksteps"]


def phase_timing(entry, scene, packed, rays, z, tables):
    """{phase: [ticks of wave 0..7]} of workgroup 0, one single-view launch through `entry` (pnr_debug_phase_timing: f16,
    pnr_debug_phase_timing_split: f16x3) of the variant library"""
    lib = _lib.load()
    if not hasattr(lib, entry):
        sys.exit(f"{_lib.LIB_PATH} has no {entry}: build a variant (tools/build_variant.sh timing) and select it with "
                 "PIXELNERF_HIP_LIB=build/libpnr_timing.so PIXELNERF_ALLOW_VARIANT=1")
    fn = getattr(lib, entry)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(_lib.PnrScene)] + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
    tim = torch.zeros(8 * len(PHASES), dtype=torch.int64, device=rays.device)
    out = torch.empty((rays.shape[0], z.shape[1], 4), dtype=torch.float32, device=rays.device)
    _lib.check(fn(scene.ref, packed.ptr, ops._p(tables), ops._p(rays), ops._p(z), rays.shape[0], max(rays.shape[0] // scene.SB, 1),
                  z.shape[1], ops._p(out), ops._p(tim), ops._stream()), entry)
    torch.cuda.synchronize()
    t = tim.cpu().reshape(8, len(PHASES))
    return {p: t[:, i].tolist() for i, p in enumerate(PHASES)}


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    scene, meta = synthetic.make_scene("sn64")
    sc = ops.make_scene(scene["latent"].to(dev), scene["poses"].to(dev), scene["focal"].to(dev), scene["c"].to(dev), scene["image_shape"], 1)
    R, K = 16384, 192
    rays = synthetic.target_rays(meta).reshape(-1, 8).repeat(4, 1)[:R].contiguous().to(dev)
    z = torch.sort(ops.sample_coarse(rays, torch.rand(R, K, device=dev)), dim=-1)[0]
    state = {k: v.to(dev) for k, v in synthetic.make_mlp_params(11).items()}
    fold = "--no-fold" not in sys.argv
    pk = ops.pack_mlp(state, "f16", folded=fold)
    tab = ops.fold_latent(sc, state, "f16") if fold else None
    print("folded stream" if fold else "full stream (--no-fold)")
    for it in range(2):
        t = phase_timing("pnr_debug_phase_timing", sc, pk, rays, z, tab)
    MT = int(os.environ.get('PNR_TILE', '64'))
    ntile = ((R * K + MT - 1) // MT + 255) // 256
    tot = [sum(v[w] for v in t.values()) for w in range(8)]
    print(f"tile {MT} pts; tiles by WG0: {ntile}; per-tile ticks per wave: " + " ".join(f"{x/ntile:8.0f}" for x in tot))
    print("phase          " + " ".join(f"   wave{w}" for w in range(8)) + "   (ticks per tile)")
    for k, v in t.items():
        print(f"  {k:12s} " + " ".join(f"{x/ntile:8.0f}" for x in v))
