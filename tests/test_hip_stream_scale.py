"""
GPU tests (-m gpu) of the power-of-two stream scale of precision "f16x3" (include/pixelnerf_hip.h "stream scale";
pnr_split.hip, the SC forms of eval_split_kernel) and of its range probe (PnrSplitAux.range_probe).

Fixture: the homogeneous blow-up of test_stream_scale_host.py -- the hidden stream is A times the base network's, the outputs
are the base network's.  Every comparison is against the CPU oracle at the SAME (blown-up) weights, held to the fp32-class bars
of tests/test_hip_split.py: per point |rgb| <= 2e-5, sigma relative <= 1e-4; renders >= 85 dB.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from helpers import golden_setup, load_golden, mlp_params, scene_for
from oracle import pnr_oracle as O
from test_stream_scale_host import blow_up

pytestmark = pytest.mark.gpu

BAR_RGB, BAR_SIGMA, BAR_DB = 2e-5, 1e-4, 85.0
A_BIG = 48000.0  # deliberately not a power of two: the scaled kernel cannot reproduce the base network's bits by accident


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


def points(dev, name):
    g = load_golden("stages")
    return torch.from_numpy(g[f"{name}_xyz"]), torch.from_numpy(g[f"{name}_viewdirs"])


def oracle_points(name, params, combine_type="average"):
    scene, _ = scene_for(name)
    xyz, vd = points(None, name)
    with torch.no_grad():
        return O.pixelnerf_forward(scene, params, xyz, vd, combine_type=combine_type).numpy()


def errors(out, ref):
    e_rgb = float(np.abs(out[..., :3] - ref[..., :3]).max())
    e_s = float((np.abs(out[..., 3] - ref[..., 3]) / np.maximum(1.0, ref[..., 3])).max())
    return e_rgb, e_s


def eval_at(ops, dev, name, params, s, combine_max=False, guard=False, probe=False):
    """eval_points of `params` packed at stream scale s -> (outputs, guard bits | None, probe words | None)"""
    sc = dscene(ops, dev, name)
    state = {k: v.to(dev) for k, v in params.items()}
    pk = ops.pack_mlp(state, "f16x3", combine_max=combine_max, stream_scale=s)
    tab = ops.fold_latent(sc, state, "f16x3")
    xyz, vd = (t.to(dev) for t in points(dev, name))
    if guard:
        ops.saturation_guard_arm(dev)
    if probe:
        ops.range_probe_arm(dev)
    try:
        out = ops.eval_points(sc, pk, xyz, vd, tables=tab).cpu().numpy()
    finally:
        if probe:
            ops.range_probe_disarm(dev)
        if guard:
            ops.saturation_guard_disarm(dev)
    bits = ops.saturation_guard_poll(dev, wait=True) if guard else None
    words = ops.range_probe_read(dev) if probe else None
    return out, bits, words


def layer_maxima(name, params):
    """the 11 maxima the probe follows, from a plain fp32 forward on the CPU (resnetfc.py:132-184): relu(x) entering
    blocks[b].fc_0 (2b), relu(net) entering fc_1 (2b + 1), relu(x) in front of lin_out (10)"""
    scene, _ = scene_for(name)
    xyz, vd = points(None, name)
    SB, B, NS = xyz.shape[0], xyz.shape[1], scene["NS"]
    p = params
    with torch.no_grad():
        poses = scene["poses"]
        xr = torch.matmul(poses[:, None, :3, :3], O.repeat_interleave(xyz, NS).unsqueeze(-1))[..., 0]
        xc = xr + poses[:, None, :3, 3]
        code = O.positional_encoding(xr.reshape(-1, 3))
        d = torch.matmul(poses[:, None, :3, :3], O.repeat_interleave(vd.reshape(SB, B, 3, 1), NS)).reshape(-1, 3)
        uv = -xc[:, :, :2] / xc[:, :, 2:]
        focal, c = scene["focal"], scene["c"]
        uv = uv * O.repeat_interleave(focal.unsqueeze(1), NS if focal.shape[0] > 1 else 1)
        uv = uv + O.repeat_interleave(c.unsqueeze(1), NS if c.shape[0] > 1 else 1)
        lat = O.index_latent(scene["latent"], uv, scene["image_shape"])
        z = lat.transpose(1, 2).reshape(-1, lat.shape[1])
        lin = torch.nn.functional.linear
        x = lin(torch.cat((code, d), dim=1), p["lin_in.weight"], p["lin_in.bias"])
        m = []
        for b in range(5):
            if b == 3 and NS > 1:
                x = x.reshape(-1, NS, B, 512).mean(dim=1).reshape(-1, 512)
            if b < 3:
                x = x + lin(z, p[f"lin_z.{b}.weight"], p[f"lin_z.{b}.bias"])
            m.append(float(torch.relu(x).max()))
            net = lin(torch.relu(x), p[f"blocks.{b}.fc_0.weight"], p[f"blocks.{b}.fc_0.bias"])
            m.append(float(torch.relu(net).max()))
            x = x + lin(torch.relu(net), p[f"blocks.{b}.fc_1.weight"], p[f"blocks.{b}.fc_1.bias"])
        m.append(float(torch.relu(x).max()))
    return m


# ---------------------------------------------------------------- 1. s = 0 changes nothing
@pytest.mark.parametrize("name", ["sn64", "mv_mini"])
def test_scale_zero_is_the_unscaled_blob_and_the_unscaled_bits(ops, dev, name):
    sc = dscene(ops, dev, name)
    state = {k: v.to(dev) for k, v in mlp_params(11).items()}
    a, b = ops.pack_mlp(state, "f16x3"), ops.pack_mlp(state, "f16x3", stream_scale=0)
    assert torch.equal(a.buf, b.buf)
    tab = ops.fold_latent(sc, state, "f16x3")
    xyz, vd = (t.to(dev) for t in points(dev, name))
    assert torch.equal(ops.eval_points(sc, a, xyz, vd, tables=tab), ops.eval_points(sc, b, xyz, vd, tables=tab))
    # the bytes plus the s passed with the launch decide, nothing else: a buffer that held a scaled stream, packed at 0 again by
    # the caller and declared so (PackedMLP.stream_scale is what ops hands to the launch), is the unscaled blob and runs unscaled
    c = ops.pack_mlp(state, "f16x3", stream_scale=5)
    lib = ops._lib.load()
    w, keep = ops._weights_struct(state)
    ops._lib.check(lib.pnr_pack_mlp_split(ctypes.byref(w), ops._p(c.buf), ops._stream()), "pnr_pack_mlp_split")
    c.stream_scale = 0
    assert torch.equal(c.buf, a.buf)
    assert torch.equal(ops.eval_points(sc, c, xyz, vd, tables=tab), ops.eval_points(sc, a, xyz, vd, tables=tab))


# ---------------------------------------------------------------- 2. every scale site, single and multi-view
@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("name,combine_max", [("sn64", False), ("mv_mini", False), ("mv_mini", True)],
                         ids=["sn64", "mv_mini", "mv_mini_view_maximum"])
def test_blow_up_by_the_scale_runs_in_the_base_networks_class(ops, dev, name, combine_max, s):
    """A = 1.5 * 2^s at scale s: the stream inside the kernel is 1.5 x the base network's, so the base network's precision class
    applies and the per-point bars hold against the oracle at those weights"""
    for which, seed in (("coarse", 11), ("fine", 12)):
        params = blow_up(mlp_params(seed), 1.5 * 2.0 ** s)
        ref = oracle_points(name, params, "max" if combine_max else "average")
        out, bits, _ = eval_at(ops, dev, name, params, s, combine_max=combine_max, guard=True)
        e_rgb, e_s = errors(out, ref)
        print(f"STREAM SCALE s={s} A=1.5*2^{s} {name}{' max' if combine_max else ''} {which}: rgb max err {e_rgb:.3e}, sigma rel err {e_s:.3e}, guard {bits}")
        assert np.isfinite(out).all() and bits == (0, 0)
        assert e_rgb <= BAR_RGB, f"rgb max err {e_rgb:.3e}"
        assert e_s <= BAR_SIGMA, f"sigma rel err {e_s:.3e}"
        if combine_max:
            assert np.abs(out - oracle_points(name, params)).max() > 0.5  # not the view mean


def test_cost_of_over_scaling_an_in_range_network_is_printed(ops, dev):
    """NOT held to the bars: a scale larger than needed costs an absolute 2^(s-25) (true units) on every operand value -- heads and
    tails of small scaled values fall into the fp16 subnormals.  The figures go into INTEGRATION.md; "auto" never picks more than
    two bits over what the probe asks."""
    params = mlp_params(11)
    ref = oracle_points("sn64", params)
    for s in (0, 4, 8):
        out, _, _ = eval_at(ops, dev, "sn64", params, s)
        e_rgb, e_s = errors(out, ref)
        print(f"OVER-SCALING in-range sn64 network (|x| max 13) at s={s}: rgb max err {e_rgb:.3e}, sigma rel err {e_s:.3e}")
        assert np.isfinite(out).all() and e_rgb < 1e-2  # (sanity only: still the same function)


# ---------------------------------------------------------------- 3. the reason the feature exists, and the probe
@pytest.mark.parametrize("name", ["sn64", "mv_mini"])
def test_blown_up_network_saturates_unscaled_and_the_probe_finds_the_scale(ops, dev, name):
    params = blow_up(mlp_params(11), A_BIG)
    ref = oracle_points(name, params)
    out0, bits0, words0 = eval_at(ops, dev, name, params, 0, guard=True, probe=True)
    e_rgb0, e_s0 = errors(out0, ref)
    print(f"BLOWN UP A={A_BIG:g} {name} at s=0: guard {bits0}, rgb max err {e_rgb0:.3e}, sigma rel err {e_s0:.3e}")
    print(f"  probe at s=0 (under-reports behind the first saturated layer): {['%.4g' % v for v in words0[0]]}")
    assert bits0[0] & 0x7FF and bits0[1] == 0                  # the guard fires (the probe instantiation keeps its bits)
    assert e_rgb0 > BAR_RGB or e_s0 > BAR_SIGMA                # ... and the result IS out of class
    base = layer_maxima(name, mlp_params(11))                  # in exact arithmetic the blown-up stream is A x this
    # layer 0 saw no clamped operand: its maximum is the true one.  Lower bound: the fp32-class kernel agrees with the CPU forward
    # to ~1e-5 relative; 1 % is that with two orders of margin
    assert words0[0][0] >= 0.99 * A_BIG * base[0]
    assert words0[1] == [0.0] * 12                             # nothing ran in the fine slot
    s = ops.stream_scale_for(max(words0[0][:11]))
    for _ in range(5):                                         # calibration iterates: scales only grow
        out, bits, words = eval_at(ops, dev, name, params, s, guard=True, probe=True)
        need = ops.stream_scale_for(max(words[0][:11]))
        if need <= s:
            break
        s = need
    print(f"  chosen s = {s}; probe at s: {['%.4g' % v for v in words[0]]}")
    print(f"  A x CPU maxima of the base network: {['%.4g' % (A_BIG * v) for v in base]}")
    assert max(words[0][:11]) * 2.0 ** -s <= 16384.0 and words[0][11] == 0.0 and bits == (0, 0)
    for l in range(11):                                        # nothing saturates at s: all 11 maxima are the true ones
        assert 0.99 * A_BIG * base[l] <= words[0][l] <= 1.01 * A_BIG * base[l], (l, words[0][l], A_BIG * base[l])
    assert ops.stream_scale_for(0.99 * A_BIG * max(base)) <= s <= ops.stream_scale_for(1.01 * A_BIG * max(base))
    e_rgb, e_s = errors(out, ref)                              # the probe instantiation computes the scaled kernel's result
    print(f"  at s={s}: rgb max err {e_rgb:.3e}, sigma rel err {e_s:.3e}")
    assert e_rgb <= BAR_RGB and e_s <= BAR_SIGMA
    plain, _, _ = eval_at(ops, dev, name, params, s)
    assert np.array_equal(plain, out)                          # ... bit for bit


# ---------------------------------------------------------------- 4. at the calibrated scale, through the model API
def blown_net(dev, scene, stream_scale=0, A=A_BIG, use_fine=True):
    from test_api_gpu import build_net
    net = build_net(dev, scene, use_fine=use_fine, precision="f16x3")
    net.mlp_coarse.load_state_dict(blow_up(mlp_params(11), A))
    if use_fine:
        net.mlp_fine.load_state_dict(blow_up(mlp_params(12), A))
    net.stream_scale = stream_scale
    return net


@pytest.mark.parametrize("name", ["sn64", "mv_mini"])
def test_calibrated_points_are_in_class_and_the_guard_is_clean(dev, name):
    scene, _ = scene_for(name)
    net = blown_net(dev, scene)
    xyz, vd = (t.to(dev) for t in points(dev, name))
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        scales = net.calibrate_stream_scale(xyz=xyz, viewdirs=vd)
        print(f"calibrate_stream_scale [{name}] -> {scales} in {net.__dict__['_probe_passes']} probe passes; log {net.__dict__['_probe_log']}")
        assert net.stream_scale == scales and all(isinstance(s, int) and s > 0 for s in scales)
        for coarse, seed in ((True, 11), (False, 12)):
            out = net(xyz, coarse=coarse, viewdirs=vd).cpu().numpy()
            e_rgb, e_s = errors(out, oracle_points(name, blow_up(mlp_params(seed), A_BIG)))
            print(f"CALIBRATED {name} {'coarse' if coarse else 'fine'} s={scales}: rgb max err {e_rgb:.3e}, sigma rel err {e_s:.3e}")
            assert e_rgb <= BAR_RGB and e_s <= BAR_SIGMA
        assert net._guard_report(wait=True) in (None, (0, 0))


@pytest.mark.parametrize("use_fine", [True, False], ids=["two_networks", "mlp_fine_none"])
def test_calibrated_render_matches_the_oracle(dev, use_fine):
    """NeRFRenderer on sn64_64_128, coarse + fine, against the oracle render at the blown-up weights with the same noise; the
    oracle draws its importance samples from the device's coarse weights (the rule of tests/test_hip_trained_weights.py: a
    rounding-level difference in a coarse weight must not move a fine sample to another bin)"""
    from pixelnerf_amd.render import NeRFRenderer
    g, scene, meta, _, _, rays, noise = golden_setup("sn64_64_128")
    mc, mf = blow_up(mlp_params(11), A_BIG), (blow_up(mlp_params(12), A_BIG) if use_fine else None)
    net = blown_net(dev, scene, use_fine=use_fine)
    rend = NeRFRenderer(n_coarse=64, n_fine=128, n_fine_depth=16, white_bkgd=True).to(dev).eval()
    nz = {k: v.to(dev) for k, v in noise.items()}
    R = rays.shape[1]
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        scales = net.calibrate_stream_scale(rays=rays.to(dev), renderer=lambda m, r: rend(m, r, _noise=nz))
        out = rend(net, rays.to(dev), want_weights=True, _noise=nz)
        assert net._guard_report(wait=True) in (None, (0, 0))
    with torch.no_grad():
        ref = O.render(scene, mc, mf, rays, noise, 64, 128, 16, white_bkgd=True,
                       sampling_weights=out.coarse.weights.cpu().reshape(R, 64))
    for p in ("coarse", "fine"):
        rgb = out[p].rgb.cpu().reshape(-1, 3)
        ps = O.psnr(rgb, ref[p]["rgb"].reshape(-1, 3))
        err = float((rgb - ref[p]["rgb"].reshape(-1, 3)).abs().max())
        print(f"CALIBRATED render sn64_64_128 ({'two networks' if use_fine else 'mlp_fine=None'}) s={scales} {p}: PSNR {ps:.1f} dB, max |rgb| err {err:.3e}")
        assert ps >= BAR_DB, f"{p} PSNR {ps:.1f} dB"


# ---------------------------------------------------------------- 5. stream_scale="auto"
def test_auto_delivers_an_in_class_first_render_and_then_stays_asynchronous(dev):
    from pixelnerf_amd.render import NeRFRenderer
    g, scene, meta, _, _, rays, noise = golden_setup("sn64_64_128")
    mc, mf = blow_up(mlp_params(11), A_BIG), blow_up(mlp_params(12), A_BIG)
    net = blown_net(dev, scene, stream_scale="auto")
    assert net.stream_scale == "auto"
    rend = NeRFRenderer(n_coarse=64, n_fine=128, n_fine_depth=16, white_bkgd=True).to(dev).eval()
    nz = {k: v.to(dev) for k, v in noise.items()}
    R = rays.shape[1]
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # no saturated result is delivered, nothing is reported
        first = rend(net, rays.to(dev), want_weights=True, _noise=nz)
        scales = net.stream_scale
        assert isinstance(scales, tuple) and len(scales) == 2 and all(isinstance(s, int) and s > 0 for s in scales)
        syncs, passes, calls = net.__dict__["_auto_syncs"], net.__dict__["_probe_passes"], net.__dict__["_guard_calls"]
        assert syncs == 1
        second = rend(net, rays.to(dev), want_weights=True, _noise=nz)
        assert (net.__dict__["_auto_syncs"], net.__dict__["_probe_passes"]) == (syncs, passes)  # no further synchronisation
        assert net.__dict__["_guard_calls"] == calls + 1 and net.stream_scale == scales
        assert torch.equal(first.fine.rgb, second.fine.rgb) and torch.equal(first.coarse.rgb, second.coarse.rgb)
        assert net._guard_report(wait=True) in (None, (0, 0))
    with torch.no_grad():
        ref = O.render(scene, mc, mf, rays, noise, 64, 128, 16, white_bkgd=True,
                       sampling_weights=first.coarse.weights.cpu().reshape(R, 64))
    for p in ("coarse", "fine"):
        ps = O.psnr(first[p].rgb.cpu().reshape(-1, 3), ref[p]["rgb"].reshape(-1, 3))
        print(f"AUTO first render sn64_64_128 s={scales} {p}: PSNR {ps:.1f} dB ({passes} probe passes)")
        assert ps >= BAR_DB
    # the same through net(xyz): the first call of a fresh automatic net returns the in-class points
    net2 = blown_net(dev, scene, stream_scale="auto")
    xyz, vd = (t.to(dev) for t in points(dev, "sn64"))
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = net2(xyz, coarse=True, viewdirs=vd).cpu().numpy()
    e_rgb, e_s = errors(out, oracle_points("sn64", mc))
    print(f"AUTO first net(xyz) s={net2.stream_scale}: rgb max err {e_rgb:.3e}, sigma rel err {e_s:.3e}")
    assert e_rgb <= BAR_RGB and e_s <= BAR_SIGMA and net2.stream_scale[0] > 0


def test_auto_on_an_in_range_network_resolves_to_zero_and_renders_the_same_bits(dev):
    from pixelnerf_amd.render import NeRFRenderer
    from test_api_gpu import build_net
    g, scene, meta, _, _, rays, noise = golden_setup("sn64_64_128")
    rend = NeRFRenderer(n_coarse=64, n_fine=128, n_fine_depth=16, white_bkgd=True).to(dev).eval()
    nz = {k: v.to(dev) for k, v in noise.items()}
    plain, auto = build_net(dev, scene, precision="f16x3"), build_net(dev, scene, precision="f16x3")
    auto.stream_scale = "auto"
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        a = rend(plain, rays.to(dev), _noise=nz)
        b = rend(auto, rays.to(dev), _noise=nz)
    assert auto.stream_scale == (0, 0) and auto.__dict__.get("_probe_passes", 0) == 0
    assert torch.equal(a.fine.rgb, b.fine.rgb) and torch.equal(a.coarse.rgb, b.coarse.rgb) and torch.equal(a.fine.depth, b.fine.depth)


def test_auto_raises_the_scale_when_a_later_batch_saturates_on_its_own(dev):
    """same weights, same encoded scene; the first batch is in range (the automatic scale resolves to 0), a LATER batch alone
    saturates (the border rows of tests/test_hip_split.py): its verdict arrives asynchronously and is reported as ever; in automatic
    mode the report also raises the scale for the following calls and says that the earlier render was out of class.  The next
    call is a first call again (the scales changed): it calibrates on its own rays and is delivered in class."""
    from pixelnerf_amd.render import NeRFRenderer
    from test_api_gpu import build_net
    from test_hip_split import _border_row_scene
    scene, inside, outside = _border_row_scene(dev)
    net = build_net(dev, scene, precision="f16x3")
    net.stream_scale = "auto"
    rend = NeRFRenderer(n_coarse=64, n_fine=128, n_fine_depth=16, white_bkgd=True).to(dev).eval()
    with torch.no_grad():
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            rend(net, inside)
            assert net.stream_scale == (0, 0) and net._guard_report(wait=True) in (None, (0, 0))  # (the first call consumed its verdict)
        rend(net, outside)  # delivered out of class: nothing announced it
        with pytest.warns(RuntimeWarning, match=r"coarse network: .*blocks\.0\.fc_0.*EARLIER render was out of class"):
            net._guard_report(wait=True)
        raised = net.stream_scale
        assert raised[0] == 2
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            out = rend(net, outside)
            assert torch.isfinite(out.fine.rgb).all() and net._guard_report(wait=True) in (None, (0, 0))
        print(f"AUTO later batch: scale raised to {raised} by the report, {net.stream_scale} after the next call's calibration")
        assert net.stream_scale[0] >= raised[0]


# ---------------------------------------------------------------- 6. refusals
def test_training_and_sharding_refuse_what_they_cannot_do(ops, dev):
    from pixelnerf_amd.render import NeRFRenderer
    from test_api_gpu import build_net
    g, scene, meta, _, _, rays, noise = golden_setup("sn64_64_128")
    net = build_net(dev, scene, precision="f16x3")
    net.stream_scale = 6
    rend = NeRFRenderer(n_coarse=64, n_fine=128, n_fine_depth=16, white_bkgd=True).to(dev)
    nz = {k: v.to(dev) for k, v in noise.items()}
    net.train()
    net.mlp_coarse.lin_in.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="stream scale"):
        rend.train()(net, rays.to(dev), _noise=nz)
    xyz, vd = (t.to(dev) for t in points(dev, "sn64"))
    with pytest.raises(NotImplementedError, match="stream scale"):
        net(xyz, coarse=True, viewdirs=vd)
    net.stream_scale = 0  # ... and trains again at scale 0
    assert net(xyz, coarse=True, viewdirs=vd).requires_grad
    # the training forward takes a blob and the s it was packed with (PnrSplitAux.stream_scale_log2): any s != 0 is refused
    sc = dscene(ops, dev, "sn64")
    state = {k: v.to(dev) for k, v in mlp_params(11).items()}
    pk, tab = ops.pack_mlp(state, "f16x3", stream_scale=3), ops.fold_latent(sc, state, "f16x3")
    r = rays.reshape(-1, 8).to(dev)
    z = ops.sample_coarse(r, nz["u1"])
    with pytest.raises(ops._lib.PixelNerfHipError, match="stream scale"):
        ops.eval_ray_samples_split_train(sc, pk, tab, r, z)
    for prec in ("f16", "bf16"):
        with pytest.raises(ops._lib.PixelNerfHipError, match="stream scale"):
            ops.pack_mlp(state, prec, folded=True, stream_scale=3)
        with pytest.raises(ops._lib.PixelNerfHipError, match="stream scale"):
            ops.pack_mlp(state, prec, backward=True, stream_scale=3)
    assert ops.pack_mlp(state, "f32", stream_scale=3).stream_scale == 0  # the exact path ignores it
    # several devices / ranks: an unresolved "auto" is refused, an integer passes through
    net.eval()
    net.mlp_coarse.lin_in.weight.requires_grad_(False)
    net.stream_scale = "auto"
    par = rend.eval().bind_parallel(net, gpus=[0, 0])
    with pytest.raises(RuntimeError, match="calibrate_stream_scale"):
        par(rays.to(dev))
    net.stream_scale = 6
    with torch.no_grad():
        torch.manual_seed(3)
        rgb, depth = rend.bind_parallel(net, gpus=[0, 0], simple_output=True)(rays.to(dev))
        torch.manual_seed(3)
        rgb1, depth1 = rend.bind_parallel(net, gpus=None, simple_output=True)(rays.to(dev))
    assert torch.equal(rgb, rgb1) and torch.equal(depth, depth1)  # the same scale on every replica: sharded = whole, bit for bit


# ---------------------------------------------------------------- 6b. a blob is plain bytes; the library keeps no table of them
def _scaled_fixture(ops, dev, s):
    """sn64_64_128 with the coarse network blown up by 1.5 * 2^s: (scene, state, tables, rays (R,8), noise, render kwargs)"""
    g, scene, meta, mc, mf, rays, noise = golden_setup("sn64_64_128")
    sc = dscene(ops, dev, str(g["scene"]))
    state = {k: v.to(dev) for k, v in blow_up(mlp_params(11), 1.5 * 2.0 ** s).items()}
    r = rays.reshape(-1, 8).contiguous().to(dev)
    nz = {k: v.to(dev).reshape(r.shape[0], -1).contiguous() for k, v in noise.items()}
    kw = dict(depth_std=float(g["depth_std"]), white_bkgd=bool(g["white_bkgd"]), lindisp=bool(g["lindisp"]))
    return sc, state, ops.fold_latent(sc, state, "f16x3"), r, nz, (int(g["n_coarse"]), int(g["n_fine"]), int(g["n_fine_depth"])), kw


def test_a_copied_blob_runs_at_the_scale_its_owner_declares(ops, dev):
    """a scaled blob is position-independent bytes: a clone (a copy to another device, a blob restored from a file) launched with
    the s it was packed at gives the original's bits, also after the original is freed.  (Before ABI revision 12 the library
    chose the kernel form by the ADDRESS pnr_pack_mlp_split had seen: the copy ran unscaled on biases packed at 2^-s.)"""
    s = 6
    sc, state, tab, r, nz, (Kc, Kf, Kfd), kw = _scaled_fixture(ops, dev, s)
    xyz, vd = (t.to(dev) for t in points(dev, "sn64"))
    pk = ops.pack_mlp(state, "f16x3", stream_scale=s)
    copy = ops.PackedMLP(pk.buf.clone(), pk.precision, folded=True, stream_scale=s)
    assert copy.buf.data_ptr() != pk.buf.data_ptr()
    pts = ops.eval_points(sc, pk, xyz, vd, tables=tab)
    img = ops.render_forward(sc, pk, None, r, Kc, Kf, Kfd, nz, tables=(tab, None), **kw)
    assert torch.equal(ops.eval_points(sc, copy, xyz, vd, tables=tab), pts)
    got = ops.render_forward(sc, copy, None, r, Kc, Kf, Kfd, nz, tables=(tab, None), **kw)
    for p in ("coarse", "fine"):
        assert torch.equal(got[p]["rgb"], img[p]["rgb"]) and torch.equal(got[p]["depth"], img[p]["depth"]), p
    wrong = ops.PackedMLP(copy.buf, pk.precision, folded=True, stream_scale=0)  # (the declared s is what selects the form)
    assert not torch.equal(ops.eval_points(sc, wrong, xyz, vd, tables=tab), pts)
    del pk
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.equal(ops.eval_points(sc, copy, xyz, vd, tables=tab), pts)
    got = ops.render_forward(sc, copy, None, r, Kc, Kf, Kfd, nz, tables=(tab, None), **kw)
    assert torch.equal(got["fine"]["rgb"], img["fine"]["rgb"]) and torch.equal(got["coarse"]["rgb"], img["coarse"]["rgb"])


def test_three_hundred_live_scaled_blobs_pack_and_render(ops, dev):
    """packing at a scale records nothing: 300 blobs at s = 3, all alive (300 distinct addresses, ~14 MB each), all pack, and the
    last renders the bits of the first.  300 = the 256 entries of the address table revision 11 kept, plus a margin: there every
    re-calibration / checkpoint reload of a process added an entry, and the 257th pack failed."""
    s = 3
    sc, state, tab, r, nz, (Kc, Kf, Kfd), kw = _scaled_fixture(ops, dev, s)
    blobs = [ops.pack_mlp(state, "f16x3", stream_scale=s) for _ in range(300)]
    assert len({b.buf.data_ptr() for b in blobs}) == 300 and all(b.stream_scale == s for b in blobs)
    first = ops.render_forward(sc, blobs[0], None, r, Kc, Kf, Kfd, nz, tables=(tab, None), **kw)
    last = ops.render_forward(sc, blobs[-1], None, r, Kc, Kf, Kfd, nz, tables=(tab, None), **kw)
    assert torch.equal(blobs[0].buf, blobs[-1].buf)
    for p in ("coarse", "fine"):
        assert torch.isfinite(last[p]["rgb"]).all()
        assert torch.equal(first[p]["rgb"], last[p]["rgb"]) and torch.equal(first[p]["depth"], last[p]["depth"]), p
    del blobs
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 7. chunked = whole at s > 0
@pytest.mark.parametrize("name", ["sn64_64_128", "mv_mini_lindisp"])
def test_chunked_render_equals_the_whole_one_at_a_scale(ops, dev, name):
    """one render in two ray chunks equals the unchunked one bit for bit: per output element the products are
    summed in an order that does not depend on the tile a point falls into, and the scale sites are element-wise"""
    g, scene, meta, mc, mf, rays, noise = golden_setup(name)
    Kc, Kf, Kfd = int(g["n_coarse"]), int(g["n_fine"]), int(g["n_fine_depth"])
    sc = dscene(ops, dev, str(g["scene"]))
    s = 6
    nets = []
    for seed in (int(g["mlp_seed_coarse"]), int(g["mlp_seed_fine"])):
        state = {k: v.to(dev) for k, v in blow_up(mlp_params(seed), 1.5 * 2.0 ** s).items()}
        nets.append((ops.pack_mlp(state, "f16x3", stream_scale=s), ops.fold_latent(sc, state, "f16x3")))
    (pc, tc), (pf, tf) = nets
    SB, B = rays.shape[0], rays.shape[1]
    nz = {k: v.to(dev).reshape(SB, B, -1) for k, v in noise.items()}
    kw = dict(depth_std=float(g["depth_std"]), white_bkgd=bool(g["white_bkgd"]), lindisp=bool(g["lindisp"]), want_weights=True)

    def run(lo, hi):
        r = rays[:, lo:hi].reshape(-1, 8).contiguous().to(dev)
        n = {k: v[:, lo:hi].reshape(SB * (hi - lo), -1).contiguous() for k, v in nz.items()}
        return ops.render_forward(sc, pc, pf, r, Kc, Kf, Kfd, n, tables=(tc, tf), **kw)
    whole, half = run(0, B), B // 2 + 1  # (an odd split: the chunks' tiles do not line up with the whole batch's)
    parts = [run(0, half), run(half, B)]
    for p in ("coarse", "fine"):
        for k in ("rgb", "depth", "weights"):
            w = whole[p][k].reshape(SB, B, -1)
            c = torch.cat([q[p][k].reshape(SB, -1, w.shape[-1]) for q in parts], dim=1)
            assert torch.equal(w, c), (p, k)
