"""GPU tests (-m gpu) of the encoder trunk under training in HIP (csrc/pnr_conv_bwd.hip; SpatialEncoder.trunk = "hip_train"):
the two convolution gradients and the pool backward against the fp64 restatements and the DERIVED bounds of
tests/encoder_train_ref.py, batch norm and the whole trunk against fp64 at ten times torch-fp32's own error, and the property
the feature exists for -- equal bytes of every level, gradient and buffer from call to call, replayed or eager, from process to
process, and over whole Adam steps through the encoder.  The figures these tests print are recorded in profiles/encoder_notes.md.

Measured on an MI355X (worst ratios): see the "Training trunk" section of profiles/encoder_notes.md."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_ref as R
import encoder_train_ref as T
from encoder_train_child import run as run_trunk
from helpers import mlp_params, scene_for
from pixelnerf_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (name, Cin, Cout, k, s, input shape).  The last four sit on either side of the two cuts of the weight gradient's P-slicing
# (P = N Ho Wo; 1 slice below 1024, 8 below 16384, 64 from there): P = 1023, 1024, 16383, 16384
CASES = [
    ("stem", 3, 64, 7, 2, (2, 3, 13, 18)),
    ("3x3s1_64", 64, 64, 3, 1, (2, 64, 5, 7)),
    ("3x3s2_64_128_odd", 64, 128, 3, 2, (2, 64, 5, 7)),
    ("3x3s2_64_128_even", 64, 128, 3, 2, (2, 64, 6, 9)),
    ("1x1s2_64_128", 64, 128, 1, 2, (2, 64, 5, 7)),
    ("3x3s1_256", 256, 256, 3, 1, (3, 256, 3, 4)),
    ("stem_P1023", 3, 64, 7, 2, (3, 3, 21, 61)),
    ("stem_P1024", 3, 64, 7, 2, (1, 3, 64, 64)),
    ("stem_P16383", 3, 64, 7, 2, (3, 3, 85, 253)),
    ("stem_P16384", 3, 64, 7, 2, (1, 3, 256, 256)),
]
IDS = [c[0] for c in CASES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _sizes(cin, cout, k, s, shape):
    N, _, H, W = shape
    p = k // 2
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    return N, H, W, p, Ho, Wo, cout * k * k, N * Ho * Wo


def _slices(cout, k, P):
    lib = _lib.load()
    return lib.pnr_conv2d_affine_slices(cout, k), lib.pnr_conv2d_backward_weight_slices(P)


def test_the_cut_shapes_sit_on_the_cuts():
    lib = _lib.load()
    got = [(_sizes(*c[1:])[7], lib.pnr_conv2d_backward_weight_slices(_sizes(*c[1:])[7])) for c in CASES[6:]]
    assert got == [(1023, 4), (1024, 32), (16383, 32), (16384, 256)]
    assert lib.pnr_conv2d_affine_slices(256, 3) == 16 and lib.pnr_conv2d_affine_slices(64, 7) == 20  # sliced K of the data gradient


@pytest.mark.parametrize("name,cin,cout,k,s,shape", CASES, ids=IDS)
def test_conv_gradients_exact_family_bit_for_bit(name, cin, cout, k, s, shape):
    """integers small enough that every partial sum in every order is representable: both gradients equal the fp64 restatement"""
    N, H, W, p, Ho, Wo, Rd, Rw = _sizes(cin, cout, k, s, shape)
    d_y = R.exact_ints(N * cout * Ho, Wo, max(Rd, Rw), seed=3).reshape(N, cout, Ho, Wo)
    w = R.exact_ints(cout, cin * k * k, Rd, seed=2).reshape(cout, cin, k, k)
    x = R.exact_ints(N * cin * H, W, Rw, seed=1).reshape(shape)
    want_x, want_w = T.conv_backward_data(d_y, w, shape, k, s, p), T.conv_backward_weight(d_y, x, k, s, p)
    assert max(np.abs(want_x).max(), np.abs(want_w).max()) < 2.0 ** 24 and np.abs(want_w).max() > 0
    got_x = ops.conv2d_backward_data(_dev(d_y), _dev(w), shape, stride=s)
    got_w = ops.conv2d_backward_weight(_dev(d_y), _dev(x), k, stride=s)
    torch.cuda.synchronize()
    assert torch.equal(got_x.cpu().double(), torch.from_numpy(want_x)), (name, "data")
    assert torch.equal(got_w.cpu().double(), torch.from_numpy(want_w)), (name, "weight")


@pytest.mark.parametrize("family", ["ranged", "cancelling"])
@pytest.mark.parametrize("name,cin,cout,k,s,shape", CASES, ids=IDS)
def test_conv_gradients_inside_the_derived_bound(name, cin, cout, k, s, shape, family):
    N, H, W, p, Ho, Wo, Rd, Rw = _sizes(cin, cout, k, s, shape)
    if family == "ranged":
        d_y = R.ranged(N * cout * Ho, Wo, seed=3).reshape(N, cout, Ho, Wo)
        w = R.ranged(cin * k * k, cout, seed=2).T.reshape(cout, cin, k, k)
        x = R.ranged(N * cin * H, W, seed=1).reshape(shape)
    else:
        d_y = R.cancelling(N * cout * Ho, Wo, seed=3, along=1, flip=False).reshape(N, cout, Ho, Wo)
        w = R.cancelling(cout, cin * k * k, seed=2, along=1).reshape(cout, cin, k, k)
        x = R.cancelling(N * cin * H, W, seed=1, along=1).reshape(shape)
    sl_d, sl_w = _slices(cout, k, Rw)
    want_x, want_w = T.conv_backward_data(d_y, w, shape, k, s, p), T.conv_backward_weight(d_y, x, k, s, p)
    bx = T.grad_bound(T.conv_backward_data(np.abs(d_y), np.abs(w), shape, k, s, p), Rd, sl_d)
    bw = T.grad_bound(T.conv_backward_weight(np.abs(d_y), np.abs(x), k, s, p), Rw, sl_w)
    got_x = ops.conv2d_backward_data(_dev(d_y), _dev(w), shape, stride=s).cpu().numpy()
    got_w = ops.conv2d_backward_weight(_dev(d_y), _dev(x), k, stride=s).cpu().numpy()
    ex, ew = np.abs(got_x.astype(np.float64) - want_x), np.abs(got_w.astype(np.float64) - want_w)
    rx, rw = float((ex / bx).max()), float((ew / bw).max())
    print(f"\nencoder_notes grads {name} {'x'.join(map(str, shape))} {family}: data R {Rd} n_sl {sl_d} worst |err| / bound = {rx:.4f}; "
          f"weight R {Rw} n_sl {sl_w} worst |err| / bound = {rw:.4f}")
    assert (ex <= bx).all(), (name, family, "data", rx)
    assert (ew <= bw).all(), (name, family, "weight", rw)


def _pool_inputs(kind):
    g = torch.Generator().manual_seed(5)
    if kind == "ties":
        x = torch.randint(-2, 3, (2, 64, 7, 9), generator=g).float()
    elif kind == "one_pixel":
        x = torch.randint(-2, 3, (1, 64, 1, 1), generator=g).float()
    else:  # a post-ReLU map: half zeros
        x = torch.relu(torch.randn(2, 64, 8, 10, generator=g))
    gy = torch.randn(tuple(F.max_pool2d(x, 3, 2, 1).shape), generator=g)
    return x, gy


@pytest.mark.parametrize("kind", ["ties", "one_pixel", "post_relu"])
def test_maxpool_backward_equals_torch_cpu_bit_for_bit(kind):
    x, gy = _pool_inputs(kind)
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(gy)
    if kind == "post_relu":
        assert 0.4 < float((x == 0).float().mean()) < 0.6
    got = ops.maxpool2d_3x3s2_backward(x.to(DEV), gy.to(DEV)).cpu()
    assert torch.equal(got, xr.grad)
    ref = T.maxpool_backward(x.double().numpy(), gy.double().numpy())
    bound = 3 * R.U * T.maxpool_backward(x.double().numpy(), gy.double().abs().numpy())
    assert (np.abs(got.double().numpy() - ref) <= bound).all()
    assert torch.equal(ops.maxpool2d_3x3s2(x.to(DEV)).cpu(), F.max_pool2d(x, 3, 2, 1))


# ------------------------------------------------------------------------------------------------ batch norm
BN_CASES = [("2x64x5x7", (2, 64, 5, 7), False, False), ("3x256x2x2", (3, 256, 2, 2), False, False), ("4x64x1x2", (4, 64, 1, 2), False, False),
            ("constant_channel", (2, 64, 5, 7), True, False), ("frozen", (2, 64, 5, 7), False, True)]


@pytest.mark.parametrize("name,shape,constant,frozen", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_batch_norm_against_fp64_at_ten_times_torch_fp32(name, shape, constant, frozen):
    g = torch.Generator().manual_seed(17)
    C = shape[1]
    v = torch.randn(shape, generator=g) * 1.5 + 0.3
    if constant:
        v[:, 5] = 0.37  # var = 0
    gam, bet = torch.rand(C, generator=g) + 0.5, 0.1 * torch.randn(C, generator=g)
    rm, rv = 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    res, g_y = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    eps, mom = 1e-5, 0.1
    # fp64 restatement
    f = T.bn_forward(v.numpy(), gam.numpy(), bet.numpy(), rm.numpy(), rv.numpy(), eps, mom, frozen, res.numpy(), True)
    b = T.bn_backward(g_y.numpy(), f["y"], v.numpy(), f["mean"], f["invstd"], gam.numpy(), frozen)
    ref = dict(y=f["y"], save_mean=f["mean"], save_invstd=f["invstd"], running_mean=f["running_mean"], running_var=f["running_var"],
               d_v=b["d_v"], d_gamma=b["d_gamma"], d_beta=b["d_beta"])
    # torch fp32 on the CPU
    vt, gt, bt = v.clone().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    rm32, rv32 = rm.clone(), rv.clone()
    out, sm, si = torch.native_batch_norm(vt, gt, bt, rm32, rv32, not frozen, mom, eps)
    torch.relu(out + res).backward(g_y)
    if frozen:
        sm, si = rm32.clone(), (rv32 + eps).rsqrt()
    t32 = dict(y=torch.relu(out + res).detach(), save_mean=sm.detach(), save_invstd=si.detach(), running_mean=rm32, running_var=rv32,
               d_v=vt.grad, d_gamma=gt.grad, d_beta=bt.grad)
    # the device
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    y, mean, invstd = ops.batchnorm2d_train_forward(v.to(DEV), gam.to(DEV), bet.to(DEV), rmd, rvd, eps, mom, frozen=frozen,
                                                    residual=res.to(DEV), relu=True)
    d_v, d_gamma, d_beta, d_res = ops.batchnorm2d_backward(g_y.to(DEV), y, v.to(DEV), mean, invstd, gam.to(DEV), frozen=frozen, want_res=True)
    hip = dict(y=y, save_mean=mean, save_invstd=invstd, running_mean=rmd, running_var=rvd, d_v=d_v, d_gamma=d_gamma, d_beta=d_beta)
    assert torch.equal(d_res, torch.where(y > 0, g_y.to(DEV), torch.zeros((), device=DEV))), "the residual branch's gradient is the masked g"
    if frozen:
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv) and torch.equal(mean.cpu(), rm)
    for key, r in ref.items():
        r = torch.from_numpy(np.asarray(r))
        e_hip = float((hip[key].cpu().double() - r).abs().max())
        e_32 = float((t32[key].double() - r).abs().max())
        print(f"\nencoder_notes bn {name} {key}: e_hip {e_hip:.3e}, e_32 {e_32:.3e}, ratio {e_hip / e_32 if e_32 > 0 else float(e_hip > 0):.3f}")
        assert e_hip <= 10.0 * e_32, (name, key, e_hip, e_32)


def test_batch_norm_refuses_one_value_per_channel():
    v = torch.zeros(1, 64, 1, 1, device=DEV)
    one = torch.ones(64, device=DEV)
    with pytest.raises(_lib.PixelNerfHipError, match="pnr_batchnorm2d_train_forward: .*more than one value"):
        ops.batchnorm2d_train_forward(v, one, one, one.clone(), one.clone())
    y, mean, _ = ops.batchnorm2d_train_forward(v, one, one, one.clone(), one.clone(), frozen=True)  # the frozen form takes it
    assert tuple(y.shape) == (1, 64, 1, 1) and torch.equal(mean, one)


# ------------------------------------------------------------------------------------------------ the whole trunk
def _encoder(backbone, num_layers, pool, frozen=False, trunk="hip_train", seed=T.TRUNK_SEED):
    enc = T.make_encoder(backbone, num_layers, pool, seed)
    enc.trunk = trunk
    return enc.to(DEV).train(not frozen)


def _cot(enc, shape):
    """the fixed cotangents of a case, from the level shapes"""
    levels = [torch.empty((shape[0], R.CHANNELS[i]) + R.level_shape(shape[2], shape[3], i, enc.use_first_pool)) for i in range(enc.num_layers)]
    return T.level_cotangents(levels)


@pytest.mark.parametrize("backbone,num_layers,pool,shape,frozen", T.TRUNK_CASES, ids=T.TRUNK_IDS)
def test_trunk_gradients_against_fp64_at_ten_times_torch_fp32(backbone, num_layers, pool, shape, frozen):
    """loss sum <level_i, G_i>: every gradient (image + all conv / BN parameters), every level and every running buffer against
    torch's fp64 CPU autograd, at ten times the error torch's fp32 CPU autograd makes, per tensor in max-abs"""
    cpu = T.make_encoder(backbone, num_layers, pool)
    img = T.trunk_image(shape)
    lv64, g64, b64, G = T.trunk_autograd(cpu, img, frozen)
    lv32, g32, b32, _ = T.trunk_autograd(cpu, img, frozen, dtype=torch.float32, cotangents=G)
    enc = _encoder(backbone, num_layers, pool, frozen)
    out = run_trunk(enc, img.to(DEV), [g.to(DEV) for g in G])
    worst = ("", 0.0)

    def hold(what, hip, ref, f32):
        nonlocal worst
        e_hip, e_32 = float((hip.double() - ref).abs().max()), float((f32.double() - ref).abs().max())
        ratio = e_hip / e_32 if e_32 > 0 else float(e_hip > 0)
        worst = max(worst, (what, ratio), key=lambda t: t[1])
        assert e_hip <= 10.0 * e_32, (what, e_hip, e_32)

    for i in range(num_layers):
        hold(f"level{i}", out[f"level{i}"], lv64[i], lv32[i])
    assert len(g64) == 1 + 3 * len(enc._trunk_convs())
    for name in g64:
        hold("grad." + name, out["grad." + name], g64[name], g32[name])
    ran = {n.rsplit(".", 1)[0] for n in g64}
    for name in b64:
        if name.endswith("num_batches_tracked"):
            assert int(out["buffer." + name]) == int(b64[name]) == (0 if frozen or name.rsplit(".", 1)[0] not in ran else 1), name
        else:
            hold("buffer." + name, out["buffer." + name], b64[name], b32[name])
    assert not [k for k in out if k.startswith("grad.") and k[5:] not in g64]
    print(f"\nencoder_notes train trunk {backbone} L{num_layers} pool={int(pool)} {'x'.join(map(str, shape))} frozen={int(frozen)}: "
          f"worst e_hip / e_32 = {worst[1]:.3f} ({worst[0]})")


def _chain(enc, img, G, frozen):
    """the whole trunk forward + backward as the per-layer entries chained by hand -> the dict run_trunk returns"""
    m = enc.model
    names = {id(mod): n for n, mod in m.named_modules()}
    one = lambda c: (torch.ones(c, device=DEV), torch.zeros(c, device=DEV))
    tape, out = [], {}

    def layer(x, conv, bn, res, relu):
        sc, sh = one(conv.out_channels)
        v = ops.conv2d_affine(x, conv.weight.detach(), sc, sh, stride=conv.stride[0])
        y, mean, invstd = ops.batchnorm2d_train_forward(v, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                                                        bn.momentum, frozen=frozen, residual=res, relu=relu)
        rec = dict(x=x, conv=conv, bn=bn, v=v, y=y, mean=mean, invstd=invstd, relu=relu)
        tape.append(rec)
        return rec

    def layer_bwd(rec, g_y, want_res=False, want_x=True):
        conv, bn = rec["conv"], rec["bn"]
        d_v, d_g, d_b, d_res = ops.batchnorm2d_backward(g_y, rec["y"] if rec["relu"] else None, rec["v"], rec["mean"], rec["invstd"],
                                                        bn.weight.detach(), frozen=frozen, want_res=want_res)
        out["grad." + names[id(conv)] + ".weight"] = ops.conv2d_backward_weight(d_v, rec["x"], conv.kernel_size[0], conv.stride[0]).cpu()
        out["grad." + names[id(bn)] + ".weight"], out["grad." + names[id(bn)] + ".bias"] = d_g.cpu(), d_b.cpu()
        d_x = ops.conv2d_backward_data(d_v, conv.weight.detach(), tuple(rec["x"].shape), conv.stride[0]) if want_x else None
        return d_x, d_res

    stem = layer(img, m.conv1, m.bn1, None, True)
    levels, blocks = [stem["y"]], []
    cur = ops.maxpool2d_3x3s2(stem["y"]) if enc.use_first_pool else stem["y"]
    for stage in (m.layer1, m.layer2, m.layer3, m.layer4)[: enc.num_layers - 1]:
        for j, blk in enumerate(stage):
            down = layer(cur, blk.downsample[0], blk.downsample[1], None, False) if blk.downsample is not None else None
            c1 = layer(cur, blk.conv1, blk.bn1, None, True)
            c2 = layer(c1["y"], blk.conv2, blk.bn2, cur if down is None else down["y"], True)
            blocks.append((down, c1, c2, j == 0, len(levels)))
            cur = c2["y"]
        levels.append(cur)
    g = G[-1]
    for down, c1, c2, first, lvl in reversed(blocks):
        d_mid, g_res = layer_bwd(c2, g, want_res=True)
        d_cur, _ = layer_bwd(c1, d_mid)
        if down is not None:
            d_idt, _ = layer_bwd(down, g_res)
            g = d_cur + d_idt
        else:
            g = d_cur + g_res
        if first:
            if lvl == 1 and enc.use_first_pool:
                g = ops.maxpool2d_3x3s2_backward(levels[0], g) + G[0]
            else:
                g = g + G[lvl - 1]
    d_img, _ = layer_bwd(stem, g)
    out["grad.image"] = d_img.cpu()
    out.update({f"level{i}": t.cpu() for i, t in enumerate(levels)})
    for name, b in m.named_buffers():
        out["buffer." + name] = b.detach().cpu().clone()
    return out


@pytest.mark.parametrize("frozen", [False, True])
def test_the_trunk_is_its_parts(frozen):
    shape = (2, 3, 32, 40)
    img = T.trunk_image(shape).to(DEV)
    a, b = _encoder("resnet18", 4, True, frozen), _encoder("resnet18", 4, True, frozen)
    G = [g.to(DEV) for g in _cot(a, shape)]
    whole = run_trunk(a, img, G)
    parts = _chain(b, img, G, frozen)
    for key, t in whole.items():
        if key.endswith("num_batches_tracked"):
            continue
        assert key in parts and torch.equal(t, parts[key]), key


# ------------------------------------------------------------------------------------------------ reproducibility
def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_two_calls_give_equal_bytes():
    shape = (3, 3, 37, 50)
    img = T.trunk_image(shape).to(DEV)
    enc = _encoder("resnet34", 4, True)
    G = [g.to(DEV) for g in _cot(enc, shape)]
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    first = run_trunk(enc, img, G)
    enc.load_state_dict(state)
    _same(first, run_trunk(enc, img, G))
    assert not torch.equal(first["buffer.bn1.running_mean"], state["model.bn1.running_mean"].cpu())
    assert float(first["grad.layer3.0.downsample.0.weight"].abs().sum()) > 0


def test_graph_replay_gives_the_bytes_of_eager():
    shape = (2, 3, 32, 40)
    enc = _encoder("resnet18", 4, True)
    G = [g.to(DEV) for g in _cot(enc, shape)]
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    img = T.trunk_image(shape).to(DEV)
    eager = run_trunk(enc, img, G)
    enc.load_state_dict(state)
    params = [p for p in enc.model.parameters()]
    static = img.clone().requires_grad_(True)

    def step():
        levels = enc._stages(static)
        loss = sum((t * g).sum() for t, g in zip(levels, G))
        return levels, torch.autograd.grad(loss, [static] + params, allow_unused=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        levels, grads = step()
    for _ in range(2):
        enc.load_state_dict(state)
        graph.replay()
        torch.cuda.synchronize()
        out = {f"level{i}": t.cpu() for i, t in enumerate(levels)}
        out["grad.image"] = grads[0].cpu()
        for (name, _), g in zip(enc.model.named_parameters(), grads[1:]):
            if g is not None:
                out["grad." + name] = g.cpu()
        for name, b in enc.model.named_buffers():
            out["buffer." + name] = b.detach().cpu().clone()
        _same(eager, out)


def test_a_fresh_process_gives_the_same_bytes(tmp_path, repo_root):
    shape = (2, 3, 32, 40)
    enc = _encoder("resnet18", 4, True)
    img, G = T.trunk_image(shape), _cot(enc, shape)
    torch.save(enc.state_dict(), tmp_path / "state.pt")
    torch.save(img, tmp_path / "images.pt")
    torch.save(G, tmp_path / "cot.pt")
    here = run_trunk(enc, img.to(DEV), [g.to(DEV) for g in G])
    child = os.path.join(repo_root, "tests", "encoder_train_child.py")
    done = subprocess.run([sys.executable, child] + [str(tmp_path / n) for n in ("state.pt", "images.pt", "cot.pt", "out.pt")],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    _same(here, torch.load(tmp_path / "out.pt"))


def test_adam_steps_through_the_encoder_are_bit_reproducible():
    """two runs of 6 Adam steps of the WHOLE net -- encoder included, trunk "hip_train", default precision -- through net.encode
    and a render of 128 rays: equal bytes of every parameter and buffer, and the encoder's weights moved"""
    from testdata import synthetic
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import Conf, default_model_conf
    dev = torch.device(DEV)
    _, meta = scene_for("sn64")
    rays = synthetic.target_rays(meta, n_rays=128).to(dev)
    src = meta["src_c2w"].to(dev)
    noise = {k: v.to(dev) for k, v in synthetic.make_noise(128, 16, 8, 4).items()}
    img = (torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(11)) * 2 - 1).to(dev)
    gt = torch.rand(1, 128, 3, generator=torch.Generator().manual_seed(10)).to(dev)

    def run():
        torch.manual_seed(0)
        conf = default_model_conf()
        conf["encoder"] = Conf(backbone="resnet34", pretrained=False, num_layers=4, use_first_pool=False, trunk="hip_train")
        net = make_model(conf).to(dev).train()
        assert net.encoder.trunk == "hip_train" and net.precision == "f16x3"
        R.randomise_bn(net.encoder, 3)
        net.mlp_coarse.load_state_dict(mlp_params(11))
        net.mlp_fine.load_state_dict(mlp_params(12))
        start = net.encoder.model.conv1.weight.detach().clone()
        rend = NeRFRenderer(n_coarse=16, n_fine=8, n_fine_depth=4, white_bkgd=True).to(dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        losses = []
        for it in range(6):
            opt.zero_grad(set_to_none=True)
            net.encode(img, src, torch.tensor(119.4256, device=dev))
            assert type(net.encoder.latent.grad_fn).__name__ == "_PyramidFunctionBackward"
            torch.manual_seed(21 + it)
            out = rend(net, rays, want_weights=False, _noise=noise)
            loss = ((out.coarse.rgb - gt) ** 2).mean() + ((out.fine.rgb - gt) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        state = {k: v.detach().clone() for k, v in net.state_dict().items()}
        return losses, state, start

    l1, s1, start = run()
    l2, s2, _ = run()
    assert l1 == l2 and all(np.isfinite(l1)), (l1, l2)
    assert s1.keys() == s2.keys() and any(k.startswith("encoder.model.layer3") for k in s1)
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert not torch.equal(s1["encoder.model.conv1.weight"], start), "the encoder's weights moved"
    assert int(s1["encoder.model.bn1.num_batches_tracked"]) == 6


# ------------------------------------------------------------------------------------------------ the same bytes as "hip"
def test_eval_under_no_grad_gives_the_bytes_of_hip():
    img = T.trunk_image((2, 3, 37, 50)).to(DEV)
    a = _encoder("resnet18", 4, True, frozen=True, trunk="hip_train")
    b = _encoder("resnet18", 4, True, frozen=True, trunk="hip")
    with torch.no_grad():
        before = a(img).clone()
        assert torch.equal(before, b(img)) and all(torch.equal(x, y) for x, y in zip(a.latents, b.latents))
    # a call in training mode: gradients flow, the running statistics move, nothing else does
    a.train()
    lat = a(img)
    assert lat.requires_grad and type(lat.grad_fn).__name__ == "_PyramidFunctionBackward"
    lat.sum().backward()
    assert float(a.model.conv1.weight.grad.abs().sum()) > 0
    a.eval()
    with torch.no_grad():
        after = a(img).clone()
        assert not torch.equal(after, before), "the updated running statistics reach the next inference encode"
        fresh = _encoder("resnet18", 4, True, frozen=True, trunk="hip", seed=9)
        fresh.load_state_dict(a.state_dict())
        assert torch.equal(fresh(img), after)
        # put the old statistics back: the old bytes
        b_state = b.state_dict()
        a.load_state_dict(b_state)
        assert torch.equal(a(img), before)
