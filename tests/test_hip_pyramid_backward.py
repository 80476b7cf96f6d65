"""GPU tests (-m gpu) of pnr_pyramid_to_latent_backward and the autograd node around the formatting pair.

Reference and bound: tests/pyramid_ref.py -- the interpolation matrices in the forward's fp32 arithmetic applied in fp64,
|hip - ref| <= (n + 4) * 2^-24 * A (worst case of an n-term fp32 sum of three-factor products, any order).  torch's own fp32
autograd of interpolate + cat on the CPU must pass the same bound: that pins the restatement to the reference's operator."""
import ctypes

import pytest
import torch

import pyramid_ref as R

pytestmark = pytest.mark.gpu

SHAPES = {
    # the sn64 pyramid: two "same" stages, integer ratios
    "sn64": ([(64, 32, 32), (64, 32, 32), (128, 16, 16), (256, 8, 8)], 2),
    # non-integer ratios, a 1 x 1 stage, W0 no multiple of any run length
    "odd": ([(64, 7, 9), (64, 4, 5), (128, 2, 3), (64, 1, 1)], 2),
    # five stages, H_s == 1 with W_s > 1, upsampling ratios of 9 and 32
    "five": ([(64, 19, 33), (64, 19, 33), (64, 10, 17), (64, 3, 2), (64, 1, 5)], 2),
    # the DTU ratios at half size: rounding moves i0
    "dtu_half": ([(64, 75, 100), (64, 38, 50), (128, 19, 25), (256, 10, 13)], 1),
}
DTU = ([(64, 150, 200), (64, 150, 200), (128, 75, 100), (256, 38, 50)], 3)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


_CASES = {}


def case(name):
    """the gradient (CPU, NCHW), the fp64 reference and the bound of one shape set: computed once, never modified"""
    if name not in _CASES:
        shapes, NV = SHAPES[name]
        gen = torch.Generator().manual_seed(1000 + sorted(SHAPES).index(name))
        g = torch.randn((NV, sum(s[0] for s in shapes), shapes[0][1], shapes[0][2]), generator=gen)
        refs, bounds = R.reference(g, shapes)
        _CASES[name] = (shapes, NV, g, refs, bounds)
    return _CASES[name]


def full_shapes(shapes, NV):
    return [(NV,) + tuple(s) for s in shapes]


def assert_within(got, refs, bounds, what, factor=1.0):
    for s, (a, r, b) in enumerate(zip(got, refs, bounds)):
        assert tuple(a.shape) == tuple(r.shape)
        assert torch.isfinite(a).all(), (what, s)
        ratio = R.worst_ratio(a, r, b)
        print(f"{what}: stage {s} worst |err| / bound = {ratio:.3f}")
        assert ratio <= factor, (what, s, ratio)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernel_matches_the_restated_operator(ops, dev, name):
    shapes, NV, g, refs, bounds = case(name)
    assert_within(R.torch_backward(g, shapes), refs, bounds, f"{name} torch cpu fp32")
    g_nchw = g.to(dev)
    g_nhwc = g_nchw.permute(0, 2, 3, 1).contiguous()
    a = ops.pyramid_to_latent_backward(g_nhwc, full_shapes(shapes, NV))
    b = ops.pyramid_to_latent_backward(g_nchw, full_shapes(shapes, NV), nchw=True)
    assert_within(a, refs, bounds, f"{name} channel-last")
    assert_within(b, refs, bounds, f"{name} nchw")
    for x, y in zip(a, ops.pyramid_to_latent_backward(g_nhwc, full_shapes(shapes, NV))):
        assert torch.equal(x, y)
    for x, y in zip(b, ops.pyramid_to_latent_backward(g_nchw, full_shapes(shapes, NV), nchw=True)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("nchw", [False, True], ids=["channel-last", "nchw"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_element_is_written(dev, name, nchw):
    """the C entry on stage buffers pre-filled with NaN: whatever the kernel leaves out stays non-finite"""
    from pixelnerf_amd import _lib
    shapes, NV, g, refs, bounds = case(name)
    g_dev = g.to(dev) if nchw else g.to(dev).permute(0, 2, 3, 1).contiguous()
    outs = [torch.full((NV,) + tuple(s), float("nan"), device=dev) for s in shapes]
    n = len(shapes)
    ints = lambda k: (ctypes.c_int * n)(*[s[k] for s in shapes])
    rc = _lib.load().pnr_pyramid_to_latent_backward(ctypes.c_void_p(g_dev.data_ptr()), int(nchw),
                                                    (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs]), ints(0), ints(1), ints(2), n, NV,
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert_within(outs, refs, bounds, f"{name} nan-prefilled")


def test_dtu_size_against_torch_on_device(ops, dev):
    """NV = 3 at the full DTU grid (the 64-bit view offsets), against torch's own backward on the same device at twice the
    bound (both sides sum in fp32); A and n are formed on the device from the same matrices."""
    shapes, NV = DTU
    gen = torch.Generator(device=dev).manual_seed(77)
    g = torch.randn((NV, 512, 150, 200), device=dev, generator=gen)
    want = R.torch_backward(g, shapes, device=dev)
    got = ops.pyramid_to_latent_backward(g.permute(0, 2, 3, 1).contiguous(), full_shapes(shapes, NV))
    got_nchw = ops.pyramid_to_latent_backward(g, full_shapes(shapes, NV), nchw=True)
    ga = g.abs().double()
    c = 0
    for s, (C, H, W) in enumerate(shapes):
        my, mx = R.axis_matrix(H, 150), R.axis_matrix(W, 200)
        n = int((my != 0).sum(0).max()) * int((mx != 0).sum(0).max())
        ty, tx = torch.from_numpy(my).to(dev).abs(), torch.from_numpy(mx).to(dev).abs()
        a = torch.einsum("yi,ncyx,xj->ncij", ty, ga[:, c:c + C], tx)
        bound = 2 * (n + 4) * R.U * a
        for what, t in (("channel-last", got[s]), ("nchw", got_nchw[s])):
            err = (t.double() - want[s].double()).abs()
            ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
            print(f"dtu {what}: stage {s} worst |err| / (2 x bound) = {ratio:.3f}")
            assert torch.isfinite(t).all() and ratio <= 1.0, (what, s, ratio)
        c += C
    for x, y in zip(got, ops.pyramid_to_latent_backward(g.permute(0, 2, 3, 1).contiguous(), full_shapes(shapes, NV))):
        assert torch.equal(x, y)


def test_function_around_the_pair(ops, dev):
    from pixelnerf_amd import autograd
    shapes, NV, g, refs, bounds = case("odd")
    gen = torch.Generator().manual_seed(5)
    levels = [torch.randn((NV,) + tuple(s), generator=gen).to(dev).requires_grad_(i != 2) for i, s in enumerate(shapes)]
    lat, nhwc = autograd.pyramid_to_latent_autograd(levels)
    assert type(lat.grad_fn).__name__ == "_PyramidFunctionBackward" and not nhwc.requires_grad
    want_nhwc, want_nchw = ops.pyramid_to_latent([t.detach() for t in levels])
    assert torch.equal(lat, want_nchw) and torch.equal(nhwc, want_nhwc)
    lat.backward(g.to(dev))  # a contiguous NCHW cotangent
    assert levels[2].grad is None
    keep = [i for i in range(len(shapes)) if i != 2]
    assert_within([levels[i].grad for i in keep], [refs[i] for i in keep], [bounds[i] for i in keep], "function, nchw cotangent")
    for t in levels:
        t.grad = None
    lat, _ = autograd.pyramid_to_latent_autograd(levels)
    lat.backward(g.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))  # channel-last memory: the no-copy path
    assert levels[2].grad is None
    assert_within([levels[i].grad for i in keep], [refs[i] for i in keep], [bounds[i] for i in keep], "function, channel-last cotangent")


def _resnet_net(dev):
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.util.conf import Conf, default_model_conf
    from helpers import mlp_params
    torch.manual_seed(0)
    conf = default_model_conf()
    conf["encoder"] = Conf(backbone="resnet34", pretrained=False, num_layers=4, use_first_pool=False)
    net = make_model(conf).to(dev).train()
    net.mlp_coarse.load_state_dict(mlp_params(11))
    net.mlp_fine.load_state_dict(mlp_params(12))
    return net


def test_encoder_trains_through_the_hip_pair(ops, dev, monkeypatch):
    """The real ResNet-34 encoder in train mode, one 64 x 64 image, a fixed cotangent, hip_format_backward on and off.
    `retain_grad()` on a level shows the formatting gradient PLUS what the next trunk stage sends back into it (MIOpen's
    backward: not reproducible, and driven by the deeper levels' gradients), so the bound is asserted on what the formatting
    backward itself hands to every level -- read off the autograd nodes (the HIP node's inputs; the four upsample nodes
    under torch's cat) -- and on the retained gradient of the LAST level, which has no other consumer."""
    from pixelnerf_amd.model.encoder import SpatialEncoder
    enc = _resnet_net(dev).encoder
    img = torch.rand(1, 3, 64, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 2 - 1
    cot = torch.randn(1, 512, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    assert SpatialEncoder.hip_format_backward
    handed, retained = {}, {}
    for on in (True, False):
        monkeypatch.setattr(SpatialEncoder, "hip_format_backward", on)
        enc.zero_grad(set_to_none=True)
        lat = enc(img)
        name = type(lat.grad_fn).__name__
        handed[on] = [None] * len(enc.latents)
        if on:
            assert name == "_PyramidFunctionBackward"
            with monkeypatch.context() as m:
                m.setattr(ops, "nchw_to_nhwc", lambda t: pytest.fail("latent_nhwc() launched a transpose"))
                nhwc = enc.latent_nhwc()
            assert nhwc is enc._nhwc[1]
            assert torch.equal(nhwc, lat.detach().permute(0, 2, 3, 1).contiguous())
            assert enc.latent_takes_channel_last_grad(lat)

            def from_node(grad_inputs, grad_outputs, store=handed[on]):
                store[:] = [t.clone() for t in grad_inputs]
            lat.grad_fn.register_hook(from_node)
        else:
            assert name.startswith("CatBackward") and not enc.latent_takes_channel_last_grad(lat)
            for i, (node, _) in enumerate(lat.grad_fn.next_functions):
                assert "Upsample" in type(node).__name__, type(node).__name__
                node.register_hook(lambda grad_inputs, grad_outputs, i=i, store=handed[on]: store.__setitem__(i, grad_inputs[0].clone()))
        for t in enc.latents:
            t.retain_grad()
        lat.backward(cot)
        retained[on] = [t.grad.clone() for t in enc.latents]
        assert torch.isfinite(enc.model.conv1.weight.grad).all() and float(enc.model.conv1.weight.grad.abs().sum()) > 0
    shapes = [tuple(t.shape[1:]) for t in enc.latents]
    assert shapes == [(64, 32, 32), (64, 32, 32), (128, 16, 16), (256, 8, 8)]
    refs, bounds = R.reference(cot, shapes)
    assert_within(handed[True], refs, bounds, "encoder, hip node")
    assert_within(handed[False], refs, bounds, "encoder, torch nodes")
    for i in range(len(shapes)):
        err = (handed[True][i].double() - handed[False][i].double()).abs().cpu()
        assert bool((err <= 2 * bounds[i]).all()), i
        tot = (retained[True][i].double() - retained[False][i].double()).abs().max()
        print(f"encoder: level {i} retained gradient, max |hip - torch| = {float(tot):.3e} (includes the trunk's share below the last level)")
    last = len(shapes) - 1
    assert_within([retained[True][last]], [refs[last]], [bounds[last]], "encoder, hip, retained last level")
    assert_within([retained[False][last]], [refs[last]], [bounds[last]], "encoder, torch, retained last level")


def test_training_step_end_to_end(ops, dev):
    from helpers import scene_for
    from testdata import synthetic
    from pixelnerf_amd.render import NeRFRenderer
    net = _resnet_net(dev)
    _, meta = scene_for("train_mv")
    _, meta1 = scene_for("sn64")
    rays = synthetic.target_rays(meta1, n_rays=64).to(dev)  # (1, 64, 8)
    noise = {k: v.to(dev) for k, v in synthetic.make_noise(64, 16, 8, 4).items()}
    images = torch.rand(1, 2, 3, 64, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(9)) * 2 - 1
    poses = meta["src_c2w"][:2].reshape(1, 2, 4, 4).to(dev)
    rend = NeRFRenderer(n_coarse=16, n_fine=8, n_fine_depth=4, white_bkgd=True).to(dev).train()
    gt = torch.rand(1, 64, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(10))

    def step():
        torch.manual_seed(21)
        out = rend(net, rays, want_weights=False, _noise=noise)
        return ((out.coarse.rgb - gt) ** 2).mean() + ((out.fine.rgb - gt) ** 2).mean()

    net.encode(images, poses, torch.tensor(119.4256, device=dev))
    lat = net.encoder.latent
    assert type(lat.grad_fn).__name__ == "_PyramidFunctionBackward" and tuple(lat.shape) == (2, 512, 32, 32)
    seen = []
    lat.register_hook(lambda g: seen.append(g))
    step().backward()
    w = net.encoder.model.conv1.weight.grad
    assert torch.isfinite(w).all() and float(w.abs().sum()) > 0
    assert len(seen) == 1
    g = seen[0]
    assert tuple(g.shape) == (2, 512, 32, 32) and g.permute(0, 2, 3, 1).is_contiguous() and not g.is_contiguous()
    # the same step on a leaf latent a caller assigned: the contiguous NCHW gradient of the permute().contiguous() branch,
    # the same bits as the channel-last tensor above holds (the render backward is bit-reproducible)
    leaf = lat.detach().clone().requires_grad_(True)
    net.encoder.latent = leaf
    net.zero_grad(set_to_none=True)
    step().backward()
    assert leaf.grad.is_contiguous() and tuple(leaf.grad.shape) == (2, 512, 32, 32)
    assert torch.equal(leaf.grad, g.contiguous())
