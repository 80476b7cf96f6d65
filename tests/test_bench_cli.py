"""bench.py's command line: a plain run carries the headline alone (the rest is --full's), and --dump-outputs writes what the
timed path returned in its last step -- the same bits from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench


def test_dump_outputs_writes_a_fixed_sample_of_large_outputs(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "MAX_DUMP_RAYS", 64)
    rgb = torch.arange(300 * 3, dtype=torch.float32).reshape(300, 3)
    depth = torch.arange(300, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rgb, depth)
    idx = np.load(tmp_path / "a" / "ray_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (64,) and np.all(np.diff(idx) > 0)
    r = np.load(tmp_path / "a" / "rgb.npy")
    assert r.dtype == np.float32 and r.shape == (64, 3)
    np.testing.assert_array_equal(r, rgb.numpy()[idx.astype(np.int64)])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "depth.npy"), idx.astype(np.float32))
    for n in ("rgb", "depth", "ray_index"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy")))
    bench.dump_outputs(str(tmp_path / "c"), rgb[:64], depth[:64])  # at the limit: every ray, no index file
    assert sorted(os.listdir(tmp_path / "c")) == ["depth.npy", "rgb.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "rgb.npy"), rgb[:64].numpy())


def test_gathered_outputs_drop_the_shard_padding():
    bufs = [torch.arange(12, dtype=torch.float32).reshape(3, 4), torch.arange(12, 24, dtype=torch.float32).reshape(3, 4)]
    rgb, depth = bench.gathered_outputs(bufs, [3, 2])
    assert torch.equal(rgb, torch.cat([bufs[0][:, :3], bufs[1][:2, :3]]))
    assert torch.equal(depth, torch.cat([bufs[0][:, 3], bufs[1][:2, 3]]))


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_its_last_step(repo_root, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines = []
    for d in ("a", "b"):
        res = subprocess.run([sys.executable, os.path.join(repo_root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                              "--rays", "8192", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode == 0, res.stderr[-2000:]
        out = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, res.stdout[-2000:]
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "rays/s" and d["higher_is_better"] is True and d["dtype"] == "f16x3"
    assert abs(d["value"] - 8192 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not {"f16_path", "cpu_baseline", "torch_eager_gpu_baseline", "psnr_db", "latency_4096_rays_ms", "extra"} & set(d)
    assert "traffic_live_error" not in d["roofline"] and "traffic_committed_profile" not in d["roofline"]
    rgb, depth = np.load(tmp_path / "a" / "rgb.npy"), np.load(tmp_path / "a" / "depth.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (8192, 3) and depth.dtype == np.float32 and depth.shape == (8192,)
    assert np.isfinite(rgb).all() and np.isfinite(depth).all()
    for n in ("rgb", "depth"):  # seeded inputs: the same arguments give the same outputs
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy")))
