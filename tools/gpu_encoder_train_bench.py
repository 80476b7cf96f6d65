#!/usr/bin/env python3
"""Time of one encoder forward + backward in training mode, launched eagerly, with SpatialEncoder.trunk = "torch" (PyTorch-ROCm /
MIOpen) and "hip_train" (csrc/pnr_conv_bwd.hip), at the shapes of profiles/encoder_notes.md ("Training trunk"), and of one full
config-5 training step (sn64: 4 objects x 128 rays, 64 + 32 (16 depth) samples, forward + backward + Adam over net.parameters())
with the encoder included.

Each trunk runs in a worker process of its own (a fresh child of this one, so "torch" can be imported from another checkout);
the workers take turns on the same device, window by window, and the median window is reported.  Every shape is warmed up first
(MIOpen picks its algorithms).  A host clock around N calls that end in a device synchronise.

    python tools/gpu_encoder_train_bench.py [--root PARENT_TREE] [--out FILE.jsonl]

--root: the checkout the "torch" worker imports the package from (the parent commit's tree, built); default: this tree."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [  # (label, images, use_first_pool)
    ("4x64x64 no pool", (4, 3, 64, 64), False),
    ("4x128x128", (4, 3, 128, 128), True),
    ("3x400x300", (3, 3, 300, 400), True),
]
STEP = "config-5 step, encoder included"


def worker(root, trunk):
    """reads commands from stdin: `setup <i>` (a shape of SHAPES, or -1 for the training step), `run <n>` -> seconds per call"""
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.model.encoder import SpatialEncoder
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import Conf, default_model_conf
    from testdata import synthetic

    dev = torch.device("cuda:0")
    call = None

    def set_trunk(enc):
        if trunk != "torch":
            enc.trunk = trunk

    def setup_encoder(i):
        _, shape, pool = SHAPES[i]
        torch.manual_seed(0)
        enc = SpatialEncoder("resnet34", pretrained=False, num_layers=4, use_first_pool=pool).to(dev).train()
        set_trunk(enc)
        img = torch.rand(shape, device=dev) * 2 - 1
        with torch.no_grad():
            cot = torch.randn_like(enc(img))

        def one():
            for p in enc.parameters():
                p.grad = None
            enc(img).backward(cot)
        return one

    def setup_step():
        scene, meta = synthetic.make_scene("train", with_latent=False)
        SB, NS = scene["SB"], scene["NS"]
        torch.manual_seed(0)
        conf = default_model_conf()
        conf["encoder"] = Conf(backbone="resnet34", pretrained=False, num_layers=4, use_first_pool=False)
        net = make_model(conf).to(dev).train()
        set_trunk(net.encoder)
        net.mlp_coarse.load_state_dict(synthetic.make_mlp_params(11))
        net.mlp_fine.load_state_dict(synthetic.make_mlp_params(12))
        images = torch.rand(SB, NS, 3, int(meta["H"]), int(meta["W"]), device=dev) * 2 - 1
        poses = meta["src_c2w"].reshape(SB, NS, 4, 4).to(dev)
        f = meta["focal"]
        focal = torch.tensor(float(f[0] if isinstance(f, (tuple, list)) else f), device=dev)
        rays = synthetic.target_rays(meta, n_rays=128).to(dev)
        gt = torch.rand(SB, 128, 3, device=dev)
        rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).to(dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)

        def one():
            net.encode(images, poses, focal)
            out = rend(net, rays, want_weights=False)
            loss = ((out.coarse.rgb - gt) ** 2).mean() + ((out.fine.rgb - gt) ** 2).mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return one

    for line in sys.stdin:
        cmd, arg = line.split()
        if cmd == "setup":
            call = setup_step() if int(arg) < 0 else setup_encoder(int(arg))
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            print("ready", flush=True)
        elif cmd == "run":
            n = int(arg)
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            torch.cuda.synchronize()
            print((time.perf_counter() - t0) / n, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=2, metavar=("ROOT", "TRUNK"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(*args.worker)
    sides = [("torch", os.path.abspath(args.root)), ("hip_train", HERE)]
    procs = {t: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, t], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                 text=True, bufsize=1) for t, root in sides}

    def ask(trunk, line):
        p = procs[trunk]
        p.stdin.write(line + "\n")
        p.stdin.flush()
        ans = p.stdout.readline().strip()
        if not ans:
            raise RuntimeError(f"the {trunk} worker ended (exit code {p.poll()}) at {line!r}")
        return ans

    rows = []
    try:
        for i, label in [(i, s[0]) for i, s in enumerate(SHAPES)] + [(-1, STEP)]:
            for t, _ in sides:
                ask(t, f"setup {i}")
            times = {t: [] for t, _ in sides}
            for _ in range(args.windows):
                for t, _ in sides:
                    times[t].append(float(ask(t, f"run {args.calls}")))
            for t, root in sides:
                row = {"what": label, "trunk": t, "mode": "eager", "ms_median": statistics.median(times[t]) * 1e3, "ms_min": min(times[t]) * 1e3,
                       "ms_max": max(times[t]) * 1e3, "calls": args.calls, "windows": args.windows, "root": os.path.basename(root)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        for p in procs.values():
            p.stdin.close()
        for p in procs.values():
            p.wait(timeout=60)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
