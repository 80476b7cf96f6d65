"""CPU tests of the training trunk's reference (tests/encoder_train_ref.py) against torch's fp64 CPU autograd, of the host side
of the training entries (refusals, sizes), of SpatialEncoder.trunk = "hip_train", and the pre-check of the whole-trunk cases the
GPU test uses.  No GPU: every library call here is refused, or has no image, before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_ref as R
import encoder_train_ref as T
from pixelnerf_amd import _lib
from pixelnerf_amd.model.encoder import SpatialEncoder

KSP = [(7, 2, 3), (3, 1, 1), (3, 2, 1), (1, 2, 0)]
P = 0x10000  # a well-aligned address nothing dereferences: every call below is refused first


def _last():
    return _lib.load().pnr_last_error().decode()


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("k,s,p", KSP)
def test_conv_gradients_equal_torch_fp64_autograd(k, s, p):
    g = torch.Generator().manual_seed(k * 10 + s)
    for H, W in [(11, 13), (10, 12)]:  # both parities of the strided walk
        x = torch.randn(2, 5, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(6, 5, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, w, None, s, p)
        d_y = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(d_y)
        np.testing.assert_allclose(T.conv_backward_data(d_y.numpy(), w.detach().numpy(), tuple(x.shape), k, s, p), x.grad.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(T.conv_backward_weight(d_y.numpy(), x.detach().numpy(), k, s, p), w.grad.numpy(), rtol=0, atol=1e-11)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("relu,use_res", [(False, False), (True, False), (True, True)])
def test_batch_norm_equals_torch_fp64_autograd(frozen, relu, use_res):
    g = torch.Generator().manual_seed(3)
    v = torch.randn(3, 6, 4, 5, generator=g, dtype=torch.float64, requires_grad=True)
    gam = (torch.rand(6, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    bet = torch.randn(6, generator=g, dtype=torch.float64, requires_grad=True)
    rm, rv = torch.randn(6, generator=g, dtype=torch.float64), torch.rand(6, generator=g, dtype=torch.float64) + 0.5
    res = torch.randn(v.shape, generator=g, dtype=torch.float64, requires_grad=True)
    rm_t, rv_t = rm.clone(), rv.clone()
    y = F.batch_norm(v, rm_t, rv_t, gam, bet, training=not frozen, momentum=0.1, eps=1e-5)
    y = y + res if use_res else y
    y = torch.relu(y) if relu else y
    g_y = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(g_y)
    fwd = T.bn_forward(v.detach().numpy(), gam.detach().numpy(), bet.detach().numpy(), rm.numpy(), rv.numpy(), 1e-5, 0.1, frozen,
                       res.detach().numpy() if use_res else None, relu)
    np.testing.assert_allclose(fwd["y"], y.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(fwd["running_mean"], rm_t.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(fwd["running_var"], rv_t.numpy(), rtol=0, atol=1e-13)
    assert frozen == (np.array_equal(fwd["running_mean"], rm.numpy()) and np.array_equal(fwd["running_var"], rv.numpy()))
    bwd = T.bn_backward(g_y.numpy(), fwd["y"] if relu else None, v.detach().numpy(), fwd["mean"], fwd["invstd"], gam.detach().numpy(), frozen)
    np.testing.assert_allclose(bwd["d_v"], v.grad.numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(bwd["d_gamma"], gam.grad.numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(bwd["d_beta"], bet.grad.numpy(), rtol=0, atol=1e-11)
    if use_res:
        np.testing.assert_allclose(bwd["g"], res.grad.numpy(), rtol=0, atol=1e-12)
    # the wrong restatements are seen
    swapped = T.bn_forward(v.detach().numpy(), gam.detach().numpy(), bet.detach().numpy(), rm.numpy(), rv.numpy(), 1e-5, 0.1, frozen,
                           None, False, mut="unbiased")
    plain = T.bn_forward(v.detach().numpy(), gam.detach().numpy(), bet.detach().numpy(), rm.numpy(), rv.numpy(), 1e-5, 0.1, frozen, None, False)
    if not frozen:
        assert np.abs(swapped["running_var"] - plain["running_var"]).max() > 1e-4 and np.abs(swapped["y"] - plain["y"]).max() > 1e-4
        wrong = T.bn_backward(g_y.numpy(), fwd["y"] if relu else None, v.detach().numpy(), fwd["mean"], fwd["invstd"], gam.detach().numpy(), False,
                              mut="no_mean_terms")
        assert np.abs(wrong["d_v"] - bwd["d_v"]).max() > 1e-3


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 2, 1, 1), (2, 4, 8, 6)])
def test_maxpool_backward_equals_torch_and_sees_the_last_maximum(shape):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 3, shape, generator=g).double().requires_grad_(True)  # many ties
    y = F.max_pool2d(x, 3, 2, 1)
    g_y = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(g_y)
    assert np.array_equal(T.maxpool_backward(x.detach().numpy(), g_y.numpy()), x.grad.numpy())
    xf = x.detach().float().requires_grad_(True)
    F.max_pool2d(xf, 3, 2, 1).backward(g_y.float())
    assert np.array_equal(T.maxpool_backward(xf.detach().numpy(), g_y.float().numpy()), xf.grad.numpy()), "bit for bit in fp32 as well"
    if shape[-1] > 1:
        assert not np.array_equal(T.maxpool_backward(x.detach().numpy(), g_y.numpy(), mut="last"), x.grad.numpy())


@pytest.mark.parametrize("k,s,p,cin,cout", [(7, 2, 3, 3, 64), (3, 1, 1, 64, 64), (3, 2, 1, 64, 128), (1, 2, 0, 64, 64)])
def test_the_exact_family_sees_a_wrong_gradient(k, s, p, cin, cout):
    N, H, W = 2, 9, 11
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    Rd, Rw = cout * k * k, N * Ho * Wo
    d_y = R.exact_ints(N * cout * Ho, Wo, max(Rd, Rw), seed=3).reshape(N, cout, Ho, Wo)
    w = R.exact_ints(cout, cin * k * k, Rd, seed=2).reshape(cout, cin, k, k)
    x = R.exact_ints(N * cin * H, W, Rw, seed=1).reshape(N, cin, H, W)
    d_x = T.conv_backward_data(d_y, w, x.shape, k, s, p)
    d_w = T.conv_backward_weight(d_y, x, k, s, p)
    for v in (d_x, d_w):
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v) and np.abs(v).max() < 2.0 ** 24, "exactly representable"
    bx = T.grad_bound(T.conv_backward_data(np.abs(d_y), np.abs(w), x.shape, k, s, p), Rd, 4)
    bw = T.grad_bound(T.conv_backward_weight(np.abs(d_y), np.abs(x), k, s, p), Rw, 4)
    muts = ["flip", "phase"] + (["transpose"] if cin == cout else [])
    if k == 1:
        muts.remove("flip")
    for mut in muts:
        assert (np.abs(T.conv_backward_data(d_y, w, x.shape, k, s, p, mut=mut) - d_x) > bx).any(), mut
        assert (np.abs(T.conv_backward_weight(d_y, x, k, s, p, mut=mut) - d_w) > bw).any(), mut


# ------------------------------------------------------------------------------------------------ sizes and refusals
def test_slices_and_workspace_bytes_answer_as_documented():
    lib = _lib.load()
    assert [lib.pnr_conv2d_backward_weight_slices(p) for p in (0, 1, 1023, 1024, 16383, 16384, 10 ** 6)] == [0, 4, 4, 32, 32, 256, 256]
    assert lib.pnr_conv2d_backward_weight_workspace_bytes(2, 64, 5, 7, 128, 3, 2) == 0
    assert lib.pnr_conv2d_backward_weight_workspace_bytes(1, 3, 64, 64, 64, 7, 2) == 8 * 64 * 147 * 4
    assert lib.pnr_conv2d_backward_weight_workspace_bytes(1, 3, 256, 256, 64, 7, 2) == 64 * 64 * 147 * 4
    assert lib.pnr_conv2d_backward_data_workspace_bytes(2, 64, 5, 7, 64, 3, 1) == 0
    assert lib.pnr_conv2d_backward_data_workspace_bytes(3, 256, 3, 4, 256, 3, 1) == 4 * 3 * 256 * 3 * 4 * 4
    assert lib.pnr_conv2d_backward_data_workspace_bytes(2, 3, 13, 18, 64, 7, 2) == 5 * 2 * 3 * 13 * 18 * 4
    assert lib.pnr_conv2d_backward_data_workspace_bytes(2, 64, 5, 7, 64, 5, 1) == 0  # a shape the entry refuses
    assert lib.pnr_batchnorm2d_train_forward_workspace_bytes(2, 64, 5, 7) == lib.pnr_batchnorm2d_backward_workspace_bytes(2, 64, 5, 7) > 0
    assert lib.pnr_batchnorm2d_train_forward_workspace_bytes(2, 0, 5, 7) == 0
    blocks = (ctypes.c_int * 4)(2, 2, 2, 2)
    assert lib.pnr_encoder_trunk_train_saved_bytes(blocks, 4, 1, 2, 32, 40) > 0
    assert lib.pnr_encoder_trunk_train_workspace_bytes(blocks, 4, 1, 2, 32, 40) > 0
    assert lib.pnr_encoder_trunk_train_saved_bytes(blocks, 6, 1, 2, 32, 40) == 0
    assert lib.pnr_encoder_trunk_train_workspace_bytes(None, 4, 1, 2, 32, 40) == 0
    assert ctypes.sizeof(_lib.PnrConvTrainRecord) == 96


def _bn_fwd(v=P, N=2, C=64, H=5, W=7, gamma=P, beta=P, rm=P, rv=P, eps=1e-5, mom=0.1, frozen=0, res=None, relu=1, y=P, mean=P, invstd=P,
            ws=P, ws_bytes=1 << 30):
    return _lib.load().pnr_batchnorm2d_train_forward(v, N, C, H, W, gamma, beta, rm, rv, eps, mom, frozen, res, relu, y, mean, invstd, ws,
                                                     ws_bytes, None)


def _bn_bwd(g_y=P, y=P, v=P, mean=P, invstd=P, gamma=P, N=2, C=64, H=5, W=7, frozen=0, d_v=P, d_gamma=P, d_beta=P, d_res=None, ws=P,
            ws_bytes=1 << 30):
    return _lib.load().pnr_batchnorm2d_backward(g_y, y, v, mean, invstd, gamma, N, C, H, W, frozen, d_v, d_gamma, d_beta, d_res, ws, ws_bytes, None)


def _dgrad(d_y=P, w=P, N=2, Cin=64, H=5, W=7, Cout=64, k=3, s=1, d_x=P, ws=None, ws_bytes=0):
    return _lib.load().pnr_conv2d_backward_data(d_y, w, N, Cin, H, W, Cout, k, s, d_x, ws, ws_bytes, None)


def _wgrad(d_y=P, x=P, N=2, Cin=64, H=5, W=7, Cout=64, k=3, s=1, d_w=P, ws=None, ws_bytes=0):
    return _lib.load().pnr_conv2d_backward_weight(d_y, x, N, Cin, H, W, Cout, k, s, d_w, ws, ws_bytes, None)


def _pool_bwd(x=P, g_y=P, N=1, C=64, H=8, W=8, d_x=P):
    return _lib.load().pnr_maxpool2d_3x3s2_backward(x, g_y, N, C, H, W, d_x, None)


@pytest.mark.parametrize("fn,name,kwargs,word", [
    (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(v=None), "null argument"), (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(mean=None), "null argument"),
    (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(rm=None), "come together"), (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(rm=None, rv=None, frozen=1), "frozen"),
    (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(res=P + 2), "misaligned"), (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(C=0), "bad sizes"),
    (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(N=1, H=1, W=1), "more than one value"), (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(eps=-1.0), "eps"),
    (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(mom=1.5), "momentum"), (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(ws=None), "workspace too small"),
    (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(ws_bytes=64), "workspace too small"), (_bn_fwd, "pnr_batchnorm2d_train_forward", dict(ws=P + 4), "workspace too small"),
    (_bn_bwd, "pnr_batchnorm2d_backward", dict(g_y=None), "null argument"), (_bn_bwd, "pnr_batchnorm2d_backward", dict(d_beta=None), "null argument"),
    (_bn_bwd, "pnr_batchnorm2d_backward", dict(y=P + 1), "misaligned"), (_bn_bwd, "pnr_batchnorm2d_backward", dict(d_res=P + 2), "misaligned"),
    (_bn_bwd, "pnr_batchnorm2d_backward", dict(H=0), "bad sizes"), (_bn_bwd, "pnr_batchnorm2d_backward", dict(N=1, H=1, W=1), "more than one value"),
    (_bn_bwd, "pnr_batchnorm2d_backward", dict(ws_bytes=8), "workspace too small"),
    (_dgrad, "pnr_conv2d_backward_data", dict(d_y=None), "null argument"), (_dgrad, "pnr_conv2d_backward_data", dict(w=P + 2), "misaligned"),
    (_dgrad, "pnr_conv2d_backward_data", dict(k=5), "(ksize, stride)"), (_dgrad, "pnr_conv2d_backward_data", dict(Cin=32), "Cin must be"),
    (_dgrad, "pnr_conv2d_backward_data", dict(Cout=96), "Cout must be"), (_dgrad, "pnr_conv2d_backward_data", dict(N=-1), "bad sizes"),
    (_dgrad, "pnr_conv2d_backward_data", dict(Cin=256, Cout=256), "workspace too small"),
    (_dgrad, "pnr_conv2d_backward_data", dict(Cin=256, Cout=256, ws=P, ws_bytes=4 * 2 * 256 * 35 * 4 - 1), "workspace too small"),
    (_wgrad, "pnr_conv2d_backward_weight", dict(x=None), "null argument"), (_wgrad, "pnr_conv2d_backward_weight", dict(d_w=P + 3), "misaligned"),
    (_wgrad, "pnr_conv2d_backward_weight", dict(k=7, s=1), "(ksize, stride)"), (_wgrad, "pnr_conv2d_backward_weight", dict(N=0), "empty batch"),
    (_wgrad, "pnr_conv2d_backward_weight", dict(N=1, Cin=3, H=64, W=64, k=7, s=2), "workspace too small"),
    (_pool_bwd, "pnr_maxpool2d_3x3s2_backward", dict(x=None), "null argument"), (_pool_bwd, "pnr_maxpool2d_3x3s2_backward", dict(g_y=P + 2), "misaligned"),
    (_pool_bwd, "pnr_maxpool2d_3x3s2_backward", dict(W=0), "bad sizes"),
])
def test_layer_refusals(fn, name, kwargs, word):
    assert fn(**kwargs) == -1
    assert _last().startswith(name + ": ") and word in _last(), _last()


def test_empty_batches_and_an_unwanted_data_gradient_are_no_ops():
    assert _bn_fwd(N=0) == 0 and _bn_bwd(N=0) == 0 and _dgrad(N=0) == 0 and _pool_bwd(N=0) == 0
    assert _dgrad(d_x=None) == 0 and _dgrad(Cin=256, Cout=256, d_x=None) == 0
    assert _bn_fwd(N=1, H=1, W=1, frozen=1, ws_bytes=0) == -1 and "workspace" in _last()  # the frozen form takes M = 1 (refused later, on the workspace)


def _records(blocks, n_levels, grads=True):
    shapes = [(3, 64, 7, 2)]
    for st in range(n_levels - 1):
        C, cin = 64 << st, (64 if st == 0 else (64 << st) // 2)
        for b in range(blocks[st]):
            if b == 0 and st > 0:
                shapes.append((cin, C, 1, 2))
            shapes.append((cin if b == 0 else C, C, 3, (2 if st > 0 else 1) if b == 0 else 1))
            shapes.append((C, C, 3, 1))
    recs = (_lib.PnrConvTrainRecord * len(shapes))()
    for r, (cin, cout, k, s) in zip(recs, shapes):
        r.w = r.gamma = r.beta = r.running_mean = r.running_var = P
        if grads:
            r.d_w = r.d_gamma = r.d_beta = P
        r.eps, r.momentum, r.cin, r.cout, r.ksize, r.stride = 1e-5, 0.1, cin, cout, k, s
    return recs


def _trunk(backward=False, recs=None, n_convs=None, blocks=(2, 2, 2, 2), n_levels=4, pool=1, frozen=0, images=P, NV=2, H=32, W=40, levels="ok",
           d_levels="ok", saved=P, saved_bytes=1 << 40, d_images=None, ws=P, ws_bytes=1 << 40):
    lib = _lib.load()
    recs = _records(blocks if all(1 <= b <= 64 for b in blocks) else (1, 1, 1, 1), min(max(n_levels, 1), 5)) if recs is None else recs
    lv = (ctypes.c_void_p * 5)(*([P] * 5)) if levels == "ok" else levels
    n = len(recs) if n_convs is None else n_convs
    blk = (ctypes.c_int * 4)(*blocks)
    if backward:
        dl = (ctypes.c_void_p * 5)(*([P] * 5)) if d_levels == "ok" else d_levels
        return lib.pnr_encoder_trunk_backward(recs, n, blk, n_levels, pool, frozen, images, NV, H, W, lv, dl, saved, saved_bytes, d_images, ws,
                                              ws_bytes, None)
    return lib.pnr_encoder_trunk_train_forward(recs, n, blk, n_levels, pool, frozen, images, NV, H, W, lv, saved, saved_bytes, ws, ws_bytes, None)


@pytest.mark.parametrize("backward", [False, True])
def test_trunk_refusals_and_the_empty_batch(backward):
    E = "pnr_encoder_trunk_backward: " if backward else "pnr_encoder_trunk_train_forward: "
    cases = [(dict(n_levels=0), "n_levels"), (dict(blocks=(2, 0, 2, 2)), "block count"), (dict(NV=-1), "bad sizes"), (dict(H=0), "bad sizes"),
             (dict(images=None), "null argument"), (dict(levels=None), "null argument"), (dict(images=P + 1), "misaligned"),
             (dict(levels=(ctypes.c_void_p * 5)(P, P, None, P, P)), "level pointer"), (dict(n_convs=5), "n_convs"),
             (dict(saved=None), "saved buffer"), (dict(saved_bytes=1024), "saved buffer"), (dict(saved=P + 4), "saved buffer"),
             (dict(ws=None), "workspace too small"), (dict(ws_bytes=1024), "workspace too small"),
             (dict(NV=1, H=8, W=8), "more than one value")]  # stage 3 of an 8 x 8 image is one pixel: M = 1
    if backward:
        cases += [(dict(d_levels=None), "null argument"), (dict(d_levels=(ctypes.c_void_p * 5)(P, None, P, P, P)), "d_levels pointer"),
                  (dict(recs=_records((2, 2, 2, 2), 4, grads=False)), "d_w / d_gamma / d_beta"), (dict(d_images=P + 2), "misaligned")]
    for kwargs, word in cases:
        assert _trunk(backward, **kwargs) == -1, kwargs
        assert _last().startswith(E) and word in _last(), (kwargs, _last())
    recs = _records((2, 2, 2, 2), 4)
    recs[5].stride = 1
    assert _trunk(backward, recs=recs) == -1 and "conv record 5" in _last() and _last().startswith(E)
    recs = _records((2, 2, 2, 2), 4)
    recs[2].gamma = None
    assert _trunk(backward, recs=recs) == -1 and "conv record 2" in _last()
    recs = _records((2, 2, 2, 2), 4)
    recs[3].running_var = None
    assert _trunk(backward, recs=recs) == -1 and "conv record 3" in _last() and "running" in _last()
    assert _trunk(backward, NV=0) == 0
    assert _trunk(backward, NV=1, H=8, W=8, frozen=1, ws_bytes=0) == -1 and "workspace" in _last()  # M = 1 passes in the frozen form


# ------------------------------------------------------------------------------------------------ the knob
def test_hip_train_conf_key_state_dict_and_refusals():
    from pixelnerf_amd.util.conf import Conf
    enc = T.make_encoder("resnet18", 4, True)
    keys = list(enc.state_dict().keys())
    enc.trunk = "hip_train"
    assert list(enc.state_dict().keys()) == keys and SpatialEncoder.trunk == "torch"
    c = SpatialEncoder.from_conf(Conf(backbone="resnet18", pretrained=False, trunk="hip_train"))
    assert c.trunk == "hip_train" and list(c.state_dict().keys()) == keys
    with pytest.raises(ValueError, match="hip_train"):
        SpatialEncoder.from_conf(Conf(backbone="resnet18", pretrained=False, trunk="miopen"))
    img = torch.zeros(1, 3, 16, 16)
    for mode, grad in [(True, True), (False, True), (False, False), (True, False)]:
        enc.train(mode)
        with torch.set_grad_enabled(grad):
            with pytest.raises(RuntimeError, match=r"hip_train.*float32 images on a HIP device.*encoder\.trunk = 'torch'"):
                enc(img)
    # the other checks come before any device work: a fake "HIP" image is not needed, the helper is called directly
    enc.train()
    sizes = enc._trunk_out_sizes(16, 16)
    assert len(sizes) == len(enc._trunk_convs()) and sizes[0] == (8, 8) and sizes[-1] == (1, 1)
    levels = R.trunk_levels(enc, torch.zeros(1, 3, 37, 50), dtype=torch.float32)
    sz = enc._trunk_out_sizes(37, 50)
    assert sz[0] == tuple(levels[0].shape[-2:]) and sz[-1] == tuple(levels[-1].shape[-2:])
    # "hip" refuses as before
    enc.trunk = "hip"
    with pytest.raises(RuntimeError, match=r"training mode.*net\.eval\(\)"):
        with torch.no_grad():
            enc(img)
    enc.eval()
    with pytest.raises(RuntimeError, match=r"grad is enabled.*torch\.no_grad\(\)"):
        enc(img)


# ------------------------------------------------------------------------------------------------ the whole-trunk cases
@pytest.mark.parametrize("backbone,num_layers,pool,shape,frozen", T.TRUNK_CASES, ids=T.TRUNK_IDS)
def test_whole_trunk_cases_are_well_conditioned(backbone, num_layers, pool, shape, frozen):
    """a condition of the GPU test, not a measurement: on every gradient and buffer torch-fp32 is within 1e-4 (relative, max-abs)
    of torch-fp64, i.e. no ReLU mask or pool argmax flipped between the two, and every batch norm sees M >= 8 values"""
    enc = T.make_encoder(backbone, num_layers, pool)
    img = T.trunk_image(shape)
    assert min(shape[0] * h * w for h, w in enc._trunk_out_sizes(shape[2], shape[3])) >= 8
    lv64, g64, b64, G = T.trunk_autograd(enc, img, frozen)
    lv32, g32, b32, _ = T.trunk_autograd(enc, img, frozen, dtype=torch.float32, cotangents=G)
    assert set(g64) == set(g32) and len(g64) == 1 + 3 * len(enc._trunk_convs())
    worst = 0.0
    for name in g64:
        worst = max(worst, T.rel_err(g32[name], g64[name]))
        assert T.rel_err(g32[name], g64[name]) <= 1e-4, (name, T.rel_err(g32[name], g64[name]))
    for a, b in zip(lv32, lv64):
        assert T.rel_err(a, b) <= 1e-4
    for name in b64:
        if "num_batches" not in name:
            assert T.rel_err(b32[name], b64[name]) <= 1e-4, name
    print(f"\n{backbone} L{num_layers} pool={int(pool)} {shape} frozen={int(frozen)}: worst torch-fp32 relative error {worst:.2e}")
