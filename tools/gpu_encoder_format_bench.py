#!/usr/bin/env python3
"""Encoder output formatting under autograd (src/model/encoder.py:150-163) on the GPU box.

1. The formatting forward + backward ALONE at the sn64, srn (64 x 64 grid) and DTU pyramid shapes:
     hip    pnr_pyramid_to_latent + pnr_pyramid_to_latent_backward on the channel-last grid gradient (the autograd node)
     torch  F.interpolate per stage + cat, and torch's backward of both on a contiguous NCHW gradient
     torch+ the same plus the two grid-sized layout changes a training step pays on that path: pnr_nchw_to_nhwc of the grid
            for the fused kernels, and permute().contiguous() of the channel-last grid gradient the scatter wrote
2. One config-5-shaped training step (4 objects x 128 rays, 64 + 32 (16) samples, precision f16x3) with the trainable ResNet-34:
   encode of 4 images of 64 x 64 in train mode, differentiable render, MSE, backward, Adam over encoder + both networks --
   with SpatialEncoder.hip_format_backward on and off, alternating.

Device-event times, medians after warm-up; one JSON line at the end.  On a tree without the backward entry (the parent
commit) part 1 reports only torch and both settings of part 2 take torch's path: that run is the yardstick."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pixelnerf_amd import autograd, ops  # noqa: E402
from pixelnerf_amd.model import make_model  # noqa: E402
from pixelnerf_amd.model.encoder import SpatialEncoder  # noqa: E402
from pixelnerf_amd.render import NeRFRenderer  # noqa: E402
from pixelnerf_amd.util.conf import Conf, default_model_conf  # noqa: E402
from testdata import synthetic  # noqa: E402

PYRAMIDS = {  # (NV, [(C, H, W)])
    "sn64": (4, [(64, 32, 32), (64, 32, 32), (128, 16, 16), (256, 8, 8)]),
    "srn": (2, [(64, 64, 64), (64, 64, 64), (128, 32, 32), (256, 16, 16)]),
    "dtu": (3, [(64, 150, 200), (64, 150, 200), (128, 75, 100), (256, 38, 50)]),
}
HAVE_HIP = hasattr(ops, "pyramid_to_latent_backward")


def timed_ms(fns, reps, warmup):
    """{name: median ms} of several zero-argument callables, run alternately (one after the other, `reps` rounds)"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, {k: round(min(v), 4) for k, v in times.items()}


def format_pair(dev, name, reps):
    NV, shapes = PYRAMIDS[name]
    gen = torch.Generator(device=dev).manual_seed(1)
    levels = [torch.randn((NV, C, H, W), device=dev, generator=gen).requires_grad_(True) for C, H, W in shapes]
    H0, W0 = shapes[0][1:]
    g_nhwc = torch.randn((NV, H0, W0, 512), device=dev, generator=gen)
    g_nchw = g_nhwc.permute(0, 3, 1, 2).contiguous()

    def torch_fwd():
        return torch.cat([F.interpolate(t, (H0, W0), mode="bilinear", align_corners=True) for t in levels], dim=1)

    def run_torch():
        torch.autograd.grad(torch_fwd(), levels, g_nchw)

    def run_torch_plus():
        lat = torch_fwd()
        ops.nchw_to_nhwc(lat.detach())
        torch.autograd.grad(lat, levels, g_nhwc.permute(0, 3, 1, 2).contiguous())

    fns = {"torch": run_torch, "torch+": run_torch_plus}
    if HAVE_HIP:
        def run_hip():
            lat, _ = autograd.pyramid_to_latent_autograd(levels)
            torch.autograd.grad(lat, levels, g_nhwc.permute(0, 3, 1, 2))

        def run_hip_bwd():
            ops.pyramid_to_latent_backward(g_nhwc, [tuple(t.shape) for t in levels])

        fns = {"hip": run_hip, "hip_backward_kernels": run_hip_bwd, **fns}
    med, low = timed_ms(fns, reps, warmup=5)
    grid = NV * H0 * W0 * 512 * 4
    stages = sum(NV * C * H * W * 4 for C, H, W in shapes)
    return {"NV": NV, "algorithmic_MB_one_direction": round((grid + stages) / 1e6, 2), "median_ms": med, "min_ms": low}


def training_step(dev, reps):
    torch.manual_seed(0)
    conf = default_model_conf()
    conf["encoder"] = Conf(backbone="resnet34", pretrained=False, num_layers=4, use_first_pool=False)
    net = make_model(conf, precision="f16x3").to(dev).train()
    net.mlp_coarse.load_state_dict(synthetic.make_mlp_params(11))
    net.mlp_fine.load_state_dict(synthetic.make_mlp_params(12))
    scene, meta = synthetic.make_scene("train", with_latent=False)
    rays = synthetic.target_rays(meta, n_rays=128).to(dev)  # (4,128,8)
    images = torch.rand(4, 3, 64, 64, device=dev) * 2 - 1
    poses = meta["src_c2w"].to(dev)
    focal = torch.tensor(119.4256, device=dev)
    gt = torch.rand(4, 128, 3, device=dev)
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-5, fused=True)

    def step(on):
        SpatialEncoder.hip_format_backward = on
        net.encode(images, poses, focal)
        out = rend(net, rays, want_weights=False)
        loss = ((out.coarse.rgb - gt) ** 2).mean() + ((out.fine.rgb - gt) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return type(net.encoder.latent.grad_fn).__name__

    nodes = {"on": step(True), "off": step(False)}
    try:
        med, low = timed_ms({"on": lambda: step(True), "off": lambda: step(False)}, reps, warmup=8)
    finally:
        SpatialEncoder.hip_format_backward = True
    return {"latent_grad_fn": nodes, "median_ms": med, "min_ms": low}


def main():
    dev = torch.device("cuda:0")
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 50
    only_step = "--step-only" in sys.argv  # a profiler run of the step alone
    res = {"tool": "gpu_encoder_format_bench", "hip_backward_entry": HAVE_HIP, "device": torch.cuda.get_device_name(0), "reps": reps}
    if not only_step:
        res["format_forward_backward"] = {name: format_pair(dev, name, reps) for name in PYRAMIDS}
    res["config5_step_trainable_resnet34"] = training_step(dev, reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
