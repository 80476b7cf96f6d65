#!/usr/bin/env python
"""The HOST cost of a call into the baked front-end: 2000 calls each of ops.baked_render, ops.baked_render_backward (into a given
`out`) and ops.baked_scene_render (two objects), 64 rays through a 4x4x4 volume -- sizes at which the kernels are nothing and the
Python in front of them is everything --, wall clock around the loop with one synchronise at the end, 7 repeats, the median.

    python tools/gpu_baked_host_cost.py                          # this checkout, one process, one JSON line
    python tools/gpu_baked_host_cost.py --against DIR --rounds 3 # DIR and this checkout alternated, one fresh process each

--against: a directory that holds another `pixelnerf_amd` package (the Python files of the parent commit, say), measured with THIS
checkout's library.  The last line compares the medians of the process medians with the spread (max - min) of DIR's own."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("baked_render", "baked_render_backward", "baked_scene_render")
N, REPEATS = 2000, 7


def measure(package_root):
    """one process: -> {call: the median us per call over REPEATS loops of N, "digest": of what the calls returned}"""
    if package_root != ROOT:
        os.environ.setdefault("PIXELNERF_HIP_LIB", os.path.join(ROOT, "pixel-nerf_amd", "csrc", "libpixelnerf_hip.so"))
    sys.path.insert(0, package_root)
    import torch
    from pixelnerf_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    R, reso, c1, c2, step = 64, (4, 4, 4), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 0.25
    origin = torch.tensor([0.0, 0.0, -3.0]) + 0.3 * torch.rand(R, 3, generator=g)
    direction = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.2 * (torch.rand(R, 3, generator=g) - 0.5), dim=1)
    rays = torch.cat([origin, direction, torch.full((R, 1), 1.0), torch.full((R, 1), 5.0)], dim=1).to(dev)
    vol = torch.rand(4, 4, 4, 4, generator=g).to(dev)
    d_rgb = torch.rand(R, 3, generator=g).to(dev)
    shift = torch.eye(4)
    shift[0, 3] = 0.5
    objects = [(vol, None, reso, c1, c2, torch.eye(4)), (vol.clone(), None, reso, c1, c2, shift)]
    out = torch.zeros_like(vol)
    calls = {"baked_render": lambda: ops.baked_render(rays, vol, reso, c1, c2, step),
             "baked_render_backward": lambda: ops.baked_render_backward(rays, vol, None, reso, c1, c2, step, d_rgb=d_rgb, out=out),
             "baked_scene_render": lambda: ops.baked_scene_render(rays, objects, step)}
    res = {"ops": ops.__file__}
    for name in CALLS:
        fn = calls[name]
        for _ in range(200):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(N):
                fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / N * 1e6)
        res[name] = round(statistics.median(times), 2)
    outputs = ops.baked_render(rays, vol, reso, c1, c2, step) + ops.baked_scene_render(rays, objects, step)
    res["digest"] = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in outputs)).hexdigest()[:16]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--against", default=None, help="a directory holding another pixelnerf_amd package")
    ap.add_argument("--rounds", type=int, default=3, help="processes per side with --against")
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)  # (what a child process measures)
    args = ap.parse_args()
    if args.against is None:
        print(json.dumps(measure(os.path.abspath(args.package_root))), flush=True)
        return 0
    sides = {"other": os.path.abspath(args.against), "this": ROOT}
    got = {side: [] for side in sides}
    for _ in range(args.rounds):
        for side, root in sides.items():  # a fresh process each: nothing of one side's imports or caches reaches the other
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--package-root", root], capture_output=True, text=True, timeout=300)
            if done.returncode != 0:
                print(done.stderr[-2000:], file=sys.stderr)
                return done.returncode
            got[side].append(json.loads(done.stdout.strip().splitlines()[-1]))
            print(side, got[side][-1], flush=True)
    assert len({r["digest"] for rs in got.values() for r in rs}) == 1, "the two packages do not return the same bytes"
    summary = {}
    for name in CALLS:
        other, this = [r[name] for r in got["other"]], [r[name] for r in got["this"]]
        spread, delta = round(max(other) - min(other), 2), round(statistics.median(this) - statistics.median(other), 2)
        summary[name] = {"other_us": other, "this_us": this, "other_spread_us": spread, "this_minus_other_us": delta, "within_spread": abs(delta) <= spread}
    print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
