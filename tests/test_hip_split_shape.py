"""
GPU tests (-m gpu) of the 16x16x32 MFMA core of the fp32-class INFERENCE kernel (pixel-nerf_amd/csrc/pnr_split.hip,
eval_split_kernel<.., TRAIN = false, ..>; pnr_layout.h slot16) next to the 32x32x16 core the training forward keeps:

  * per point against the exact path (precision "f32") at the bars of tests/test_hip_split.py -- |rgb| <= 2e-5, sigma rel <= 1e-4 --
    for P = 1, 15, 16, 17, 63, 64, 65, 129 points (ragged last 16-point tile, ragged last 64-point tile, more than one workgroup)
    and NS = 1, 2, 3 source views (the single-view and the multi-view instantiations);
  * eval_points = eval_ray_samples and guard on = guard off, bit for bit, at P = 65;
  * inference and training forward from ONE pack_mlp(.., "f16x3") blob (the two cores address the same packed streams): each
    within the per-point bar of fp32, within 2e-5 of each other on rgb, and NOT bit-equal (two cores, two summation orders);
  * one case at stream scale s > 0, same bar;
  * the training forward's outputs, dumped operand images, x5 and relu masks are the bits of the commit before the 16x16x32 core
    (tests/golden/split_train_bits.npz: SHA-256 digests recorded with tools/make_split_train_bits.py from that commit's library;
    the file names the commit in `recorded_from_commit`).
"""
import hashlib
import os

import numpy as np
import pytest
import torch

from helpers import mlp_params, scene_for

pytestmark = pytest.mark.gpu

SCENES = {1: "sn64", 2: "srn_mini", 3: "dtu_mini"}  # NS -> scene (one object each)
POINTS = [1, 15, 16, 17, 63, 64, 65, 129]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_train_bits.npz")
TRAIN_BITS_SCENES = ("sn64", "dtu_mini")  # the single-view and the multi-view training instantiation
R_BITS, K_BITS = 5, 13                     # 65 points: a ragged second tile


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


def dscene(ops, dev, name):
    s, _ = scene_for(name)
    return ops.make_scene(s["latent"].to(dev), s["poses"].to(dev), s["focal"].to(dev), s["c"].to(dev), s["image_shape"], s["NS"])


def seeded_samples(name, R, K, seed=7):
    """R target rays of the scene and K depths per ray, from a seeded CPU generator (no device code in the inputs)"""
    from testdata import synthetic
    _, meta = scene_for(name)
    rays = synthetic.target_rays(meta).reshape(-1, 8)
    gen = torch.Generator().manual_seed(seed)
    pick = torch.randperm(rays.shape[0], generator=gen)[:R]
    rays = rays[pick].contiguous()
    u = torch.rand(R, K, generator=gen)
    z = rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * ((torch.arange(K)[None, :] + u) / K)
    return rays, z.contiguous()


def points_of(rays, z):
    xyz = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(1, -1, 3).contiguous()
    vd = rays[:, None, 3:6].expand(-1, z.shape[1], -1).reshape(1, -1, 3).contiguous()
    return xyz, vd


class Net:
    """one scene on the device with its f16x3 blob / tables and its exact-path blob, shared by the tests of a module run"""

    def __init__(self, ops, dev, name, seed=11, stream_scale=0):
        self.sc = dscene(ops, dev, name)
        self.state = {k: v.to(dev) for k, v in mlp_params(seed).items()}
        self.pk = ops.pack_mlp(self.state, "f16x3", stream_scale=stream_scale)
        self.tab = ops.fold_latent(self.sc, self.state, "f16x3")
        self.exact = ops.pack_mlp(self.state, "f32")


@pytest.fixture(scope="module")
def nets(ops, dev):
    cache = {}

    def get(name, stream_scale=0):
        if (name, stream_scale) not in cache:
            cache[(name, stream_scale)] = Net(ops, dev, name, stream_scale=stream_scale)
        return cache[(name, stream_scale)]
    return get


def bars(out, ref, what):
    e_rgb = float((out[..., :3] - ref[..., :3]).abs().max())
    e_s = float(((out[..., 3] - ref[..., 3]).abs() / ref[..., 3].clamp(min=1.0)).max())
    print(f"{what}: rgb max err {e_rgb:.3e}, sigma rel err {e_s:.3e}")
    assert torch.isfinite(out).all(), what
    assert e_rgb <= 2e-5, f"{what}: rgb max err {e_rgb:.3e}"
    assert e_s <= 1e-4, f"{what}: sigma rel err {e_s:.3e}"


@pytest.mark.parametrize("NS", [1, 2, 3])
def test_per_point_against_the_exact_path(ops, dev, nets, NS):
    net = nets(SCENES[NS])
    rays, z = seeded_samples(SCENES[NS], max(POINTS), 1)
    xyz, vd = (t.to(dev) for t in points_of(rays, z))
    for P in POINTS:
        x, v = xyz[:, :P].contiguous(), vd[:, :P].contiguous()
        out = ops.eval_points(net.sc, net.pk, x, v, tables=net.tab)
        ref = ops.eval_points(net.sc, net.exact, x, v)
        assert out.shape[-2:] == (P, 4)
        bars(out, ref, f"NS {NS}, {P} points")


@pytest.mark.parametrize("NS", [1, 3])
def test_entries_and_guard_agree_bit_for_bit(ops, dev, nets, NS):
    net = nets(SCENES[NS])
    rays, z = seeded_samples(SCENES[NS], R_BITS, K_BITS)
    xyz, vd = (t.to(dev) for t in points_of(rays, z))
    rays, z = rays.to(dev), z.to(dev)
    a = ops.eval_ray_samples(net.sc, net.pk, rays, z, tables=net.tab)
    b = ops.eval_points(net.sc, net.pk, xyz, vd, tables=net.tab).reshape(a.shape)
    assert a.shape == (R_BITS, K_BITS, 4) and torch.equal(a, b)
    ops.saturation_guard_arm(dev)
    try:
        ga = ops.eval_ray_samples(net.sc, net.pk, rays, z, tables=net.tab)
        gb = ops.eval_points(net.sc, net.pk, xyz, vd, tables=net.tab).reshape(a.shape)
    finally:
        ops.saturation_guard_disarm(dev)
    assert ops.saturation_guard_poll(dev, wait=True) == (0, 0)
    assert torch.equal(a, ga) and torch.equal(a, gb)


@pytest.mark.parametrize("NS", [1, 3])
def test_inference_and_training_forward_from_one_blob(ops, dev, nets, NS):
    net = nets(SCENES[NS])
    rays, z = (t.to(dev) for t in seeded_samples(SCENES[NS], R_BITS, K_BITS))
    inf = ops.eval_ray_samples(net.sc, net.pk, rays, z, tables=net.tab)
    trn, _ = ops.eval_ray_samples_split_train(net.sc, net.pk, net.tab, rays, z)
    ref = ops.eval_ray_samples(net.sc, net.exact, rays, z)
    bars(inf, ref, f"NS {NS} inference (16x16x32 core)")
    bars(trn, ref, f"NS {NS} training forward (32x32x16 core)")
    d = float((inf[..., :3] - trn[..., :3]).abs().max())
    print(f"NS {NS}: inference vs training forward, rgb max diff {d:.3e}")
    assert d <= 2e-5
    assert not torch.equal(inf, trn), "two cores sum in two orders: bit-equal outputs mean both ran the same core"


@pytest.mark.parametrize("NS", [1, 2])
def test_stream_scale(ops, dev, nets, NS):
    net = nets(SCENES[NS], stream_scale=3)
    rays, z = seeded_samples(SCENES[NS], 65, 1)
    xyz, vd = (t.to(dev) for t in points_of(rays, z))
    out = ops.eval_points(net.sc, net.pk, xyz, vd, tables=net.tab)
    bars(out, ops.eval_points(net.sc, net.exact, xyz, vd), f"NS {NS}, stream scale 3")


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def train_bits(ops, dev, name):
    """-> {what: SHA-256} of everything the training forward leaves behind, on the seeded 65 samples of scene `name`"""
    net = Net(ops, dev, name)
    rays, z = (t.to(dev) for t in seeded_samples(name, R_BITS, K_BITS))
    out, saved = ops.eval_ray_samples_split_train(net.sc, net.pk, net.tab, rays, z)
    torch.cuda.synchronize()
    # masks: [layer][view][tile][thread] 64-bit words; the pooled layers (6..10: blocks 3-4 and the stream in front of lin_out)
    # write the slab of view 0 only, the rest of theirs is never written
    m = saved.masks.view(torch.int64).reshape(11, saved.NS, -1)
    d = {"out": digest(out), "x5": digest(saved.x5), "masks_view": digest(m[:6]), "masks_pooled": digest(m[6:, 0])}
    for b in range(5):
        d[f"a{b}"] = digest(saved.a[b])
        d[f"n{b}"] = digest(saved.n[b])
    return d


@pytest.mark.parametrize("name", TRAIN_BITS_SCENES)
def test_training_forward_bits_are_the_parent_commits(ops, dev, name):
    g = np.load(GOLDEN)
    got = train_bits(ops, dev, name)
    again = train_bits(ops, dev, name)
    assert got == again, "the training forward is not reproducible run to run"
    for k, v in got.items():
        assert str(g[f"{name}_{k}"]) == v, f"{name}: {k} differs from the recorded bits"
