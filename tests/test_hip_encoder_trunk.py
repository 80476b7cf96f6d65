"""GPU tests (-m gpu) of the encoder trunk in HIP (csrc/pnr_conv.hip; SpatialEncoder.trunk = "hip"): every layer against the
fp64 restatement and the DERIVED bound of tests/encoder_ref.py, the whole trunk against the module in double at ten times
torch-fp32's own error, and the property the trunk exists for -- equal bytes from call to call, per image whatever the batch,
replayed or eager, from process to process.  The figures these tests print are recorded in profiles/encoder_notes.md."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_ref as R
from helpers import mlp_params, scene_for
from pixelnerf_amd import _lib, ops
from pixelnerf_amd.model.encoder import SpatialEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (name, Cin, Cout, k, s, [input shapes]): the smallest maps where tiles, padding and stride phases can go wrong
LAYERS = [
    ("stem", 3, 64, 7, 2, [(2, 3, 37, 50)]),
    ("3x3s1_64", 64, 64, 3, 1, [(2, 64, 10, 13)]),
    ("3x3s2_64_128", 64, 128, 3, 2, [(2, 64, 10, 13)]),
    ("3x3s1_256", 256, 256, 3, 1, [(1, 256, 3, 4), (3, 256, 3, 4)]),
    ("3x3s1_512", 512, 512, 3, 1, [(1, 512, 2, 2)]),
    ("1x1s2_128_256", 128, 256, 1, 2, [(2, 128, 5, 7)]),
]
CASES = [(name, cin, cout, k, s, shp) for name, cin, cout, k, s, shapes in LAYERS for shp in shapes]
IDS = [f"{c[0]}-{'x'.join(map(str, c[5]))}" for c in CASES]


def _run(x, w, scale, shift, s, res, relu):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    y = ops.conv2d_affine(t(x), t(w), t(scale), t(shift), stride=s, residual=t(res), relu=relu)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _n_slices(cin, k):
    return _lib.load().pnr_conv2d_affine_slices(cin, k)


@pytest.mark.parametrize("name,cin,cout,k,s,shape", CASES, ids=IDS)
def test_layer_exact_family_bit_for_bit(name, cin, cout, k, s, shape):
    """integers small enough that every partial sum in every order is representable, power-of-two scale, integer shift and
    residual: the device must return the fp64 reference bit for bit"""
    N, _, H, W = shape
    K, p = cin * k * k, k // 2
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    x = R.exact_ints(N * cin * H, W, K, seed=1).reshape(shape)
    w = R.exact_ints(cout, K, K, seed=2).reshape(cout, cin, k, k)
    scale = (2.0 ** (np.arange(cout) % 3 - 1)).astype(np.float32)
    shift = (np.arange(cout) % 7 - 3).astype(np.float32)
    res_full = R.exact_ints(N * cout * Ho, Wo, K, seed=3).reshape(N, cout, Ho, Wo)
    for use_res in (False, True):
        for relu in (False, True):
            res = res_full if use_res else None
            want, _, _ = R.conv_affine(x, w, scale, shift, res, relu, k, s, p)
            assert np.abs(want).max() < 2.0 ** 24
            got = _run(x, w, scale, shift, s, res, relu)
            assert got.shape == want.shape
            assert np.array_equal(got.astype(np.float64), want), (name, use_res, relu, float(np.abs(got - want).max()))


@pytest.mark.parametrize("family", ["ranged", "cancelling"])
@pytest.mark.parametrize("name,cin,cout,k,s,shape", CASES, ids=IDS)
def test_layer_inside_the_derived_bound(name, cin, cout, k, s, shape, family):
    N, _, H, W = shape
    K, p = cin * k * k, k // 2
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    g = np.random.default_rng(7)
    if family == "ranged":
        x = R.ranged(N * cin * H, W, seed=1).reshape(shape)
        w = R.ranged(K, cout, seed=2, zero_cols=(3, 40)).T.reshape(cout, cin, k, k)  # two all-zero output channels: S = 0 there
    else:
        x = R.cancelling(N * cin * H, W, seed=1, along=1, flip=False).reshape(shape)
        w = R.cancelling(cout, K, seed=2, along=1).reshape(cout, cin, k, k)
    scale = (g.uniform(0.5, 1.5, cout) * np.where(np.arange(cout) % 5 == 0, -1, 1)).astype(np.float32)
    shift = (0.1 * g.standard_normal(cout)).astype(np.float32)
    res_full = R.ranged(N * cout * Ho, Wo, seed=3, lo=-4, hi=2).reshape(N, cout, Ho, Wo)
    n_sl = _n_slices(cin, k)
    worst = 0.0
    for use_res in (False, True):
        for relu in (False, True):
            res = res_full if use_res else None
            _, A, B = R.conv_affine(x, w, scale, shift, res, relu, k, s, p)
            value, bound, S = R.layer_bound(A, B, scale, shift, res, n_sl, N, Ho, Wo)
            want = np.maximum(value, 0.0) if relu else value
            got = _run(x, w, scale, shift, s, res, relu)
            err = np.abs(got.astype(np.float64) - want)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert (err <= bound).all(), (name, family, use_res, relu, ratio)
            dead = S == 0
            if family == "ranged":
                assert dead[:, 3].all() and dead[:, 40].all()
            plain = np.broadcast_to(shift[None, :, None, None], value.shape).astype(np.float32)
            plain = plain + res.astype(np.float32) if use_res else plain
            plain = np.maximum(plain, np.float32(0)) if relu else plain
            assert np.array_equal(got[dead], plain[dead]), "an output with S = 0 is exactly shift + res"
    print(f"\nencoder_notes layer {name} {'x'.join(map(str, shape))} {family}: K {K}, slices {n_sl}, worst |err| / bound = {worst:.4f}")


@pytest.mark.parametrize("shape", [(2, 64, 19, 25), (1, 64, 32, 32)])
def test_maxpool_equals_torch(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert torch.equal(ops.maxpool2d_3x3s2(x), F.max_pool2d(x, 3, 2, 1))
    assert np.array_equal(ops.maxpool2d_3x3s2(x).cpu().numpy(), R.maxpool(x.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ the whole trunk
def _encoder(backbone="resnet34", num_layers=4, use_first_pool=True, seed=0, trunk="hip"):
    torch.manual_seed(seed)
    enc = SpatialEncoder(backbone, pretrained=False, num_layers=num_layers, use_first_pool=use_first_pool)
    R.randomise_bn(enc, seed + 1)
    enc.trunk = trunk
    return enc.to(DEV).eval()


def _images(shape, seed=11):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


IMAGES = [(1, 3, 64, 64), (3, 3, 37, 50), (2, 3, 24, 32)]


@pytest.mark.parametrize("backbone,num_layers,pool,shapes", [
    ("resnet34", 4, True, IMAGES), ("resnet34", 4, False, IMAGES), ("resnet18", 4, True, IMAGES), ("resnet34", 5, True, IMAGES[:2]),
], ids=["r34", "r34_nopool", "r18", "r34_5levels"])
def test_trunk_against_fp64_at_ten_times_torch_fp32(backbone, num_layers, pool, shapes):
    enc = _encoder(backbone, num_layers, pool)
    enc.use_graph = False
    for shape in shapes:
        img = _images(shape)
        ref = R.trunk_levels(enc, img)
        f32 = R.trunk_levels(enc, img, dtype=torch.float32)
        with torch.no_grad():
            latent = enc(img.to(DEV))
            levels = list(enc.latents)
            assert len(levels) == num_layers == len(ref)
            for i, (h, r, c) in enumerate(zip(levels, ref, f32)):
                assert tuple(h.shape) == tuple(r.shape) and h.is_contiguous() and h.dtype == torch.float32
                e_hip = float((h.cpu().double() - r).abs().max())
                e_32 = float((c.double() - r).abs().max())
                print(f"\nencoder_notes trunk {backbone} L{num_layers} pool={int(pool)} {'x'.join(map(str, shape))} level {i}: "
                      f"e_hip {e_hip:.3e}, e_32 {e_32:.3e}, ratio {e_hip / e_32:.3f}")
                assert e_hip <= 10.0 * e_32, (shape, i, e_hip, e_32)
            # the latent is the existing formatting pass of exactly those levels
            nhwc, nchw = ops.pyramid_to_latent(levels, want_nchw=True)
            assert torch.equal(latent, nchw) and torch.equal(enc.latent_nhwc(), nhwc)


# ------------------------------------------------------------------------------------------------ reproducibility
def test_two_encodes_and_batch_against_single_images():
    enc = _encoder("resnet34", 4, False)
    enc.use_graph = False
    img = _images((3, 3, 37, 50)).to(DEV)
    with torch.no_grad():
        a = enc(img).clone()
        la = [t.clone() for t in enc.latents]
        b = enc(img).clone()
        assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(la, enc.latents))
        for n in range(3):
            one = enc(img[n:n + 1])
            assert torch.equal(one[0], a[n]), n
            assert all(torch.equal(x[0], y[n]) for x, y in zip(enc.latents, la)), n


def test_graph_replay_gives_the_bytes_of_eager():
    enc = _encoder("resnet34", 4, True)
    img = _images((2, 3, 64, 64)).to(DEV)
    with torch.no_grad():
        enc.use_graph = False
        eager = enc(img).clone()
        eager_nhwc = enc.latent_nhwc().clone()
        enc.use_graph = True
        first = enc(img).clone()     # captures, then replays
        assert len(enc.__dict__.get("_graphs", {})) == 1, "the encode was not captured"
        second = enc(img).clone()    # replays
        assert len(enc._graphs) == 1
        assert torch.equal(first, eager) and torch.equal(second, eager) and torch.equal(enc.latent_nhwc(), eager_nhwc)
        other = enc(img.flip(-1))    # the same capture, another image
        assert len(enc._graphs) == 1 and not torch.equal(other, eager)
        enc.use_graph = False
        assert torch.equal(enc(img.flip(-1)), other)


def test_a_fresh_process_gives_the_same_bytes(tmp_path, repo_root):
    enc = _encoder("resnet34", 4, False)
    img = _images((2, 3, 37, 50))
    torch.save(enc.state_dict(), tmp_path / "state.pt")
    torch.save(img, tmp_path / "images.pt")
    with torch.no_grad():
        here = enc(img.to(DEV)).cpu()
    child = os.path.join(repo_root, "tests", "encoder_trunk_child.py")
    done = subprocess.run([sys.executable, child, str(tmp_path / "state.pt"), str(tmp_path / "images.pt"), str(tmp_path / "latent.pt")],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    assert torch.equal(torch.load(tmp_path / "latent.pt"), here)


def test_encode_and_render_twice_gives_equal_pixels():
    """image to pixels: two rounds of net.encode + a render of 64 rays with one seed, at the default precision"""
    from testdata import synthetic
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import Conf, default_model_conf
    dev = torch.device(DEV)
    torch.manual_seed(0)
    conf = default_model_conf()
    conf["encoder"] = Conf(backbone="resnet34", pretrained=False, num_layers=4, use_first_pool=False, trunk="hip")
    net = make_model(conf).to(dev).eval()
    assert net.encoder.trunk == "hip" and net.precision == "f16x3"
    R.randomise_bn(net.encoder, 3)
    for m in (net.mlp_coarse, net.mlp_fine):
        m.load_state_dict(mlp_params(11))
    _, meta = scene_for("sn64")
    rays = synthetic.target_rays(meta, n_rays=64).to(dev)
    src = meta["src_c2w"].to(dev)
    rend = NeRFRenderer(n_coarse=16, n_fine=8, n_fine_depth=4, white_bkgd=True).to(dev).eval()
    render_par = rend.bind_parallel(net, None, simple_output=True).eval()
    img = _images((1, 3, 64, 64)).to(dev)
    rounds = []
    with torch.no_grad():
        for _ in range(2):
            net.encode(img, src, torch.tensor(119.4256, device=dev))
            torch.manual_seed(1)
            rgb, depth = render_par(rays)
            rounds.append((net.encoder.latent.clone(), rgb.clone(), depth.clone()))
    assert torch.isfinite(rounds[0][1]).all()
    for a, b in zip(*rounds):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the folded-weights cache
def test_new_weights_rebuild_the_folded_records():
    img = _images((2, 3, 24, 32)).to(DEV)
    enc = _encoder("resnet18", 4, True, seed=0)
    other = _encoder("resnet18", 4, True, seed=5)
    with torch.no_grad():
        old = enc(img).clone()
        assert torch.equal(enc(img), old)
        # load_state_dict of other weights: differs from the old encode, equals the module that owns those weights
        enc.load_state_dict(other.state_dict())
        new = enc(img).clone()
        assert not torch.equal(new, old) and torch.equal(new, other(img))
        # an in-place update of one BN buffer: the same, against a fresh module loaded from the updated state
        enc.model.layer2[0].bn1.running_mean.add_(0.25)
        upd = enc(img).clone()
        assert not torch.equal(upd, new)
        fresh = _encoder("resnet18", 4, True, seed=9)
        fresh.load_state_dict(enc.state_dict())
        assert torch.equal(fresh(img), upd)
        enc.use_graph = False
        assert torch.equal(enc(img), upd)
