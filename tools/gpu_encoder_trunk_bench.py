#!/usr/bin/env python3
"""Time of one inference encode (trunk + formatting pass) with SpatialEncoder.trunk = "torch" (PyTorch-ROCm / MIOpen) and "hip"
(csrc/pnr_conv.hip), launched eagerly and replayed from the captured HIP graph, at the shapes of profiles/encoder_notes.md.

The trunks alternate inside one process, window by window, and the median window is reported; every shape is warmed up first
(MIOpen picks its algorithms, the graph is captured).  A host clock around N calls that end in a device synchronise.

    python tools/gpu_encoder_trunk_bench.py [--root TREE] [--trunks torch,hip] [--out FILE.jsonl]

--root: import the package from another checkout (the parent commit's, for its torch trunk: `--root PARENT --trunks torch`)."""
import argparse
import json
import os
import statistics
import sys
import time

SHAPES = [  # (label, images, use_first_pool)
    ("sn64 1x64x64", (1, 3, 64, 64), False),
    ("sn64 16x64x64", (16, 3, 64, 64), False),
    ("2x128x128", (2, 3, 128, 128), True),
    ("3x400x300", (3, 3, 300, 400), True),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--trunks", default="torch,hip")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from pixelnerf_amd.model.encoder import SpatialEncoder

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    trunks = args.trunks.split(",")
    rows = []
    for label, shape, pool in SHAPES:
        torch.manual_seed(0)
        enc = SpatialEncoder("resnet34", pretrained=False, num_layers=4, use_first_pool=pool).to(dev).eval()
        img = (torch.rand(shape, device=dev) * 2 - 1)
        configs = [(t, g) for t in trunks for g in (False, True)]

        def run(trunk, graph, n):
            if trunk != "torch" or hasattr(SpatialEncoder, "trunk"):
                enc.trunk = trunk
            enc.use_graph = graph
            with torch.no_grad():
                for _ in range(n):
                    enc(img)
            torch.cuda.synchronize()

        for cfg in configs:
            run(*cfg, 5)
        times = {cfg: [] for cfg in configs}
        for _ in range(args.windows):
            for cfg in configs:
                t0 = time.perf_counter()
                run(*cfg, args.calls)
                times[cfg].append((time.perf_counter() - t0) / args.calls)
        for (trunk, graph), ts in times.items():
            row = {"shape": label, "trunk": trunk, "mode": "graph" if graph else "eager", "ms_median": statistics.median(ts) * 1e3,
                   "ms_min": min(ts) * 1e3, "ms_max": max(ts) * 1e3, "calls": args.calls, "windows": args.windows,
                   "root": os.path.basename(os.path.abspath(args.root))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
