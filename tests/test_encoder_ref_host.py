"""CPU tests of the encoder trunk's reference (tests/encoder_ref.py), of the host side of its entries (refusals, sizes, level
shapes) and of SpatialEncoder.trunk.  No GPU: every library call here is refused, or has no image, before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_ref as R
from pixelnerf_amd import _lib
from pixelnerf_amd.model.encoder import SpatialEncoder

KSP = [(7, 2, 3), (3, 1, 1), (3, 2, 1), (1, 2, 0)]
P = 0x10000  # a well-aligned address nothing dereferences: every call below is refused first


def _last():
    return _lib.load().pnr_last_error().decode()


@pytest.mark.parametrize("k,s,p", KSP)
def test_conv_affine_equals_torch_fp64(k, s, p):
    g = torch.Generator().manual_seed(k * 10 + s)
    x = torch.randn(2, 5, 11, 13, generator=g, dtype=torch.float64)
    w = torch.randn(6, 5, k, k, generator=g, dtype=torch.float64)
    scale, shift = torch.rand(6, generator=g, dtype=torch.float64) + 0.5, torch.randn(6, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, None, s, p) * scale[None, :, None, None] + shift[None, :, None, None]
    res = torch.randn(want.shape, generator=g, dtype=torch.float64)
    for use_res in (False, True):
        for relu in (False, True):
            ref = want + res if use_res else want
            ref = torch.relu(ref) if relu else ref
            got, A, B = R.conv_affine(x.numpy(), w.numpy(), scale.numpy(), shift.numpy(), res.numpy() if use_res else None, relu, k, s, p)
            assert got.shape == tuple(ref.shape) and A.shape == (ref.shape[0] * ref.shape[2] * ref.shape[3], 5 * k * k)
            np.testing.assert_allclose(got, ref.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(R.maxpool(x.numpy()), F.max_pool2d(x, 3, 2, 1).numpy())


def _encoder(backbone="resnet18", num_layers=4, use_first_pool=True, seed=0):
    torch.manual_seed(seed)
    enc = SpatialEncoder(backbone, pretrained=False, num_layers=num_layers, use_first_pool=use_first_pool)
    return R.randomise_bn(enc, seed + 1).eval()


def test_trunk_levels_equals_the_fp64_module_layer_by_layer():
    """trunk_levels is the module in double; the same levels built from conv_affine + maxpool + the folded batch norms agree"""
    enc = _encoder("resnet18", 3)
    img = torch.randn(2, 3, 21, 26, generator=torch.Generator().manual_seed(3))
    levels = R.trunk_levels(enc, img)
    m = enc.model

    def layer(x, conv, bn, res, relu):
        scale, shift = (t.double().numpy() for t in R.fold_bn(bn))
        k = conv.kernel_size[0]
        return R.conv_affine(x, conv.weight.detach().double().numpy(), scale, shift, res, relu, k, conv.stride[0], k // 2)[0]

    x = layer(img.double().numpy(), m.conv1, m.bn1, None, True)
    mine = [x]
    x = R.maxpool(x)
    for stage in (m.layer1, m.layer2):
        for blk in stage:
            idt = x if blk.downsample is None else layer(x, blk.downsample[0], blk.downsample[1], None, False)
            x = layer(layer(x, blk.conv1, blk.bn1, None, True), blk.conv2, blk.bn2, idt, True)
        mine.append(x)
    assert len(levels) == 3
    for a, b in zip(levels, mine):
        assert tuple(a.shape) == b.shape and a.dtype == torch.float64
        # the fold is rounded to fp32 once, the module divides in double: 2^-24 relative per layer
        np.testing.assert_allclose(b, a.numpy(), rtol=0, atol=2e-5 * float(a.abs().max()))


@pytest.mark.parametrize("pool", [True, False])
def test_level_shapes_equal_the_torch_trunk(pool):
    lib = _lib.load()
    enc = _encoder("resnet18", 5, pool)
    for H, W in [(8, 8), (9, 70), (17, 23), (33, 64), (64, 64), (70, 37), (50, 13)]:
        levels = R.trunk_levels(enc, torch.zeros(1, 3, H, W), dtype=torch.float32)
        for i, t in enumerate(levels):
            h, w = ctypes.c_int(), ctypes.c_int()
            assert lib.pnr_encoder_level_shape(H, W, i, int(pool), ctypes.byref(h), ctypes.byref(w)) == 0
            assert (h.value, w.value) == R.level_shape(H, W, i, pool) == tuple(t.shape[-2:]), (H, W, i)
            assert t.shape[1] == R.CHANNELS[i]
    assert lib.pnr_encoder_level_shape(0, 8, 0, 1, None, None) == -1 and "bad sizes" in _last()
    assert lib.pnr_encoder_level_shape(8, 8, 5, 1, None, None) == -1 and "level" in _last()


@pytest.mark.parametrize("k,s,p,cin,cout", [(7, 2, 3, 3, 64), (3, 1, 1, 64, 64), (3, 2, 1, 64, 128), (1, 2, 0, 64, 64)])
def test_the_exact_family_sees_a_wrong_restatement(k, s, p, cin, cout):
    K = cin * k * k
    x = R.exact_ints(2 * cin * 9, 11, K, seed=1).reshape(2, cin, 9, 11)
    w = R.exact_ints(cout, K, K, seed=2).reshape(cout, cin, k, k)
    scale = 2.0 ** (np.arange(cout) % 3 - 1)
    shift = (np.arange(cout) % 5 - 2).astype(np.float64)
    Ho, Wo = R.out_size(9, k, s, p), R.out_size(11, k, s, p)
    _, A, B = R.conv_affine(x, w, scale, shift, None, False, k, s, p)
    value, bound, _ = R.layer_bound(A, B, scale, shift, None, 1, 2, Ho, Wo)
    right = R.conv_affine(x, w, scale, shift, None, False, k, s, p)[0]
    assert np.array_equal(right, value) and np.array_equal(value.astype(np.float32).astype(np.float64), value), "exactly representable"
    muts = ["flip", "pad", "phase"] + (["transpose"] if cin == cout else [])
    if k == 1:
        muts.remove("flip")  # a 1x1 kernel has nothing to flip
    for mut in muts:
        wrong = R.conv_affine(x, w, scale, shift, None, False, k, s, p, mut=mut)[0]
        assert (np.abs(wrong - value) > bound).any(), mut


def test_slices_and_workspace_bytes_answer_as_documented():
    lib = _lib.load()
    assert [lib.pnr_conv2d_affine_slices(c, k) for c, k in [(3, 7), (64, 3), (128, 3), (256, 3), (512, 3), (1024, 3), (256, 1)]] \
        == [4, 4, 8, 16, 32, 32, 4]  # four quarters per slice
    assert lib.pnr_conv2d_affine_slices(0, 3) == 0
    assert lib.pnr_conv2d_affine_workspace_bytes(2, 64, 10, 13, 64, 3, 1) == 0
    assert lib.pnr_conv2d_affine_workspace_bytes(3, 256, 3, 4, 256, 3, 1) == 4 * 3 * 256 * 3 * 4 * 4
    assert lib.pnr_conv2d_affine_workspace_bytes(2, 64, 10, 13, 128, 3, 2) == 0
    assert lib.pnr_conv2d_affine_workspace_bytes(2, 128, 5, 7, 128, 3, 2) == 2 * 2 * 128 * 3 * 4 * 4
    assert lib.pnr_conv2d_affine_workspace_bytes(2, 64, 10, 13, 64, 5, 1) == 0      # a shape the entry refuses
    blocks = (ctypes.c_int * 4)(3, 4, 6, 3)
    assert lib.pnr_encoder_trunk_workspace_bytes(blocks, 4, 1, 2, 64, 64) > 0
    assert lib.pnr_encoder_trunk_workspace_bytes(blocks, 1, 1, 2, 64, 64) == 0      # the stem alone needs no scratch
    assert lib.pnr_encoder_trunk_workspace_bytes(blocks, 6, 1, 2, 64, 64) == 0
    assert lib.pnr_encoder_trunk_workspace_bytes(None, 4, 1, 2, 64, 64) == 0


def _conv(x=P, N=2, Cin=64, H=10, W=13, w=P, scale=P, shift=P, Cout=64, k=3, s=1, res=None, relu=1, y=P, ws=None, ws_bytes=0):
    return _lib.load().pnr_conv2d_affine(x, N, Cin, H, W, w, scale, shift, Cout, k, s, res, relu, y, ws, ws_bytes, None)


@pytest.mark.parametrize("kwargs,word", [
    (dict(x=None), "null argument"), (dict(w=None), "null argument"), (dict(scale=None), "null argument"),
    (dict(shift=None), "null argument"), (dict(y=None), "null argument"),
    (dict(x=P + 2), "misaligned"), (dict(res=P + 1), "misaligned"), (dict(y=P + 3), "misaligned"),
    (dict(N=-1), "bad sizes"), (dict(Cin=0), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=-3), "bad sizes"), (dict(Cout=0), "bad sizes"),
    (dict(k=5), "(ksize, stride)"), (dict(k=7, s=1), "(ksize, stride)"), (dict(k=1, s=1), "(ksize, stride)"), (dict(s=3), "(ksize, stride)"),
    (dict(Cin=32), "Cin must be"), (dict(Cin=3 * 64 + 1), "Cin must be"), (dict(Cout=96), "Cout must be"),
    (dict(Cin=256, Cout=256), "workspace too small"), (dict(Cin=256, Cout=256, ws=P, ws_bytes=4 * 2 * 256 * 10 * 13 * 4 - 1), "workspace too small"),
])
def test_conv_refusals(kwargs, word):
    assert _conv(**kwargs) == -1
    assert _last().startswith("pnr_conv2d_affine: ") and word in _last()


def test_empty_batches_are_no_ops_and_pool_refusals():
    lib = _lib.load()
    assert _conv(N=0) == 0
    assert lib.pnr_maxpool2d_3x3s2(P, 0, 64, 8, 8, P, None) == 0
    for args, word in [((None, 1, 64, 8, 8, P), "null argument"), ((P, 1, 64, 8, 8, None), "null argument"),
                       ((P + 2, 1, 64, 8, 8, P), "misaligned"), ((P, -1, 64, 8, 8, P), "bad sizes"), ((P, 1, 0, 8, 8, P), "bad sizes"),
                       ((P, 1, 64, 0, 8, P), "bad sizes")]:
        assert lib.pnr_maxpool2d_3x3s2(*args, None) == -1
        assert _last().startswith("pnr_maxpool2d_3x3s2: ") and word in _last()


def _records(blocks, n_levels):
    """well-formed records (fake addresses) of a trunk, in the order the layers run"""
    shapes = [(3, 64, 7, 2)]
    for st in range(n_levels - 1):
        C, cin = 64 << st, (64 if st == 0 else (64 << st) // 2)
        for b in range(blocks[st]):
            if b == 0 and st > 0:
                shapes.append((cin, C, 1, 2))
            shapes.append((cin if b == 0 else C, C, 3, (2 if st > 0 else 1) if b == 0 else 1))
            shapes.append((C, C, 3, 1))
    recs = (_lib.PnrConvRecord * len(shapes))()
    for r, (cin, cout, k, s) in zip(recs, shapes):
        r.w, r.scale, r.shift, r.cin, r.cout, r.ksize, r.stride = P, P, P, cin, cout, k, s
    return recs


def _trunk(recs=None, n_convs=None, blocks=(3, 4, 6, 3), n_levels=4, pool=1, images=P, NV=1, H=64, W=64, levels="ok", ws=P, ws_bytes=1 << 40):
    recs = _records(blocks if all(1 <= b <= 64 for b in blocks) else (1, 1, 1, 1), min(max(n_levels, 1), 5)) if recs is None else recs
    lv = (ctypes.c_void_p * 5)(*([P] * 5)) if levels == "ok" else levels
    return _lib.load().pnr_encoder_trunk_forward(recs, len(recs) if n_convs is None else n_convs, (ctypes.c_int * 4)(*blocks), n_levels,
                                                 pool, images, NV, H, W, lv, ws, ws_bytes, None)


def test_trunk_refusals_and_the_empty_batch():
    E = "pnr_encoder_trunk_forward: "
    assert ctypes.sizeof(_lib.PnrConvRecord) == 40
    cases = [(dict(n_levels=0), "n_levels"), (dict(n_levels=6), "n_levels"), (dict(blocks=(3, 0, 6, 3)), "block count"),
             (dict(blocks=(3, 4, 6, 65)), "block count"), (dict(NV=-1), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"),
             (dict(images=None), "null argument"), (dict(levels=None), "null argument"), (dict(images=P + 1), "misaligned"),
             (dict(levels=(ctypes.c_void_p * 5)(P, P, None, P, P)), "level pointer"),
             (dict(levels=(ctypes.c_void_p * 5)(P, P + 2, P, P, P)), "level pointer"),
             (dict(n_convs=5), "n_convs"), (dict(ws=None), "workspace too small"), (dict(ws_bytes=1024), "workspace too small")]
    for kwargs, word in cases:
        assert _trunk(**kwargs) == -1, kwargs
        assert _last().startswith(E) and word in _last(), (kwargs, _last())
    # resnet18's records handed to a resnet34 trunk of the same length cannot be: the count differs; a record out of place is named
    recs = _records((3, 4, 6, 3), 4)
    recs[8].stride = 1
    assert _trunk(recs=recs) == -1 and "conv record 8" in _last() and _last().startswith(E)
    recs = _records((3, 4, 6, 3), 4)
    recs[2].scale = None
    assert _trunk(recs=recs) == -1 and "conv record 2" in _last()
    recs = _records((3, 4, 6, 3), 4)
    recs[0].w = P + 2
    assert _trunk(recs=recs) == -1 and "conv record 0" in _last()
    assert _trunk(NV=0) == 0
    assert _trunk(NV=0, blocks=(2, 2, 2, 2), n_levels=5, pool=0) == 0


def test_trunk_attribute_conf_key_and_state_dict():
    from pixelnerf_amd.util.conf import Conf
    assert SpatialEncoder.trunk == "torch"
    enc = _encoder("resnet34")
    assert enc.trunk == "torch" and "trunk" not in enc.__dict__
    keys = list(enc.state_dict().keys())
    enc.trunk = "hip"
    assert list(enc.state_dict().keys()) == keys and not any("scale" in k or "shift" in k or "trunk" in k for k in keys)
    assert len(keys) == 1 + 5 + sum(n * 12 for n in (3, 4, 6, 3)) + 3 * 6 and keys[0] == "model.conv1.weight"
    assert SpatialEncoder.trunk == "torch", "the instance attribute leaves the class alone"
    assert "_hip_trunk" in SpatialEncoder._TRANSIENT
    a = SpatialEncoder.from_conf(Conf(backbone="resnet18", pretrained=False))
    b = SpatialEncoder.from_conf(Conf(backbone="resnet18", pretrained=False, trunk="hip"))
    assert a.trunk == "torch" and b.trunk == "hip"
    with pytest.raises(ValueError, match="trunk"):
        SpatialEncoder.from_conf(Conf(backbone="resnet18", pretrained=False, trunk="miopen"))


def test_hip_trunk_refuses_what_it_cannot_run():
    enc = _encoder("resnet18")
    enc.trunk = "hip"
    img = torch.zeros(1, 3, 16, 16)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"inference only.*not float32 on a HIP device.*encoder\.trunk = 'torch'"):
            enc(img)
        enc.train()
        with pytest.raises(RuntimeError, match=r"training mode.*net\.eval\(\)"):
            enc(img)
        enc.eval()
    with pytest.raises(RuntimeError, match=r"grad is enabled.*torch\.no_grad\(\)"):
        enc(img)
    enc.trunk = "torch"  # and the torch trunk is what it was
    with torch.no_grad():
        assert tuple(enc(img).shape) == (1, 512, 8, 8)
