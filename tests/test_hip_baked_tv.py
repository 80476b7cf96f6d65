"""GPU tests (-m gpu) of the total-variation prior: pnr_baked_tv through ops.baked_tv, the autograd Function behind
`TrainableBaked.tv`, `volume.tv` and util.bake.fit's tv_* arguments.

The yardstick is tests/baked_tv_ref.py -- the definition restated in torch, its gradient by autograd in fp64 (its own checks:
tests/test_baked_tv_host.py).  Error and bar are tests/position_ref.py's: error = max|got - ref64| / max|ref64|, bar = 10 x the error
of torch's fp32 autograd through the same restatement on the same inputs (floor 2e-6, cap 2e-4); a value is held by the same rule
as a one-element array.  Every comparison prints the HIP error, the torch-fp32 error and the bar before it asserts."""
import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_tv_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def bake():
    from pixelnerf_amd.util import bake as _bake
    return _bake


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _tv(ops, dev, case, want_value=True, want_grad=True, grad_out=None, scale=None):
    """ops.baked_tv on the inputs of a case (the rows of a sparse one) -> (value32, value64, the gradient buffer)"""
    inp = T.inputs(case)
    sparse = case.sparse is not None
    stored = _t(inp["rows"] if sparse else inp["stored"], dev)
    if want_grad and grad_out is None:
        grad_out = torch.zeros_like(stored)
    v32, v64 = ops.baked_tv(stored, case.degree, case.reso, inp["weights"], eps=T.EPS, index=_t(inp["index"], dev) if sparse else None,
                            ids=_t(inp["ids"], dev) if sparse else None, want_value=want_value, grad_out=grad_out, scale=scale)
    return v32, v64, grad_out


def _hold(what, got, ref64, ref32, scale=1.0):
    """print the three numbers, then hold `got` to the bar; scale: what the reference is multiplied by"""
    got, ref64, ref32 = (torch.as_tensor(x).detach().cpu().double().reshape(-1) for x in (got, ref64, ref32))
    err, err32 = T.error(got, ref64 * scale), T.error(ref32 * scale, ref64 * scale)
    bar = T.bar_from(err32)
    print(f"{what}: HIP error {err:.3e}, torch-fp32 error {err32:.3e}, bar {bar:.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert err <= bar, (what, err, bar)
    return bar


# ---------------------------------------------------------------- 1. value and gradient against the fp64 restatement
@pytest.mark.parametrize("name", T.CASE_IDS)
def test_value_and_gradient_of_every_case_are_within_their_bars(dev, ops, name):
    """(9,8,7) at every kind (several blocks at degree 2), (2,2,2) and (2,5,3) where every point is on the border, a constant block, a
    ramp, kept sets with a third and with all of the cells on; weights all ones, rgb only, sigma only, distinct.  Case 5 of the
    issue -- a sparse volume against the masked restatement -- is the `third` cases here."""
    case = T.BY_NAME[name]
    inp, v64, g64, v32, g32 = T.reference(case)
    got32, got64, grad = _tv(ops, dev, case)
    assert grad.shape == g64.shape and grad.dtype == torch.float32 and got32.dtype == torch.float32 and got64.dtype == torch.float64
    _hold(name + " value64", got64, v64, v32)
    _hold(name + " value32", got32, v64, v32)
    assert float(got32) == float(got64.float())                       # one number, rounded once
    _hold(name + " gradient", grad, g64, g32)
    alone32, alone64, none = _tv(ops, dev, case, want_grad=False)     # either half alone gives the bytes of the pair
    assert none is None and torch.equal(alone32, got32) and torch.equal(alone64, got64)
    no32, no64, grad_alone = _tv(ops, dev, case, want_value=False)
    assert no32 is None and no64 is None and torch.equal(grad_alone, grad)


# ---------------------------------------------------------------- 2. exact zeros
@pytest.mark.parametrize("name", ["rgba_987_block", "sh1_987_block"])
def test_centre_of_a_constant_block_gets_exactly_zero(dev, ops, name):
    case = T.BY_NAME[name]
    g64 = T.reference(case)[2]
    grad = _tv(ops, dev, case)[2].cpu()
    assert not bool(g64[T.BLOCK_CENTRE].any()) and not bool(grad[T.BLOCK_CENTRE].any())
    assert bool((grad[g64 == 0] == 0).all()) and bool(grad.any())


@pytest.mark.parametrize("name", ["sh0_987_rgb", "sh1_987_sigma", "sh1_987_all"])
def test_elements_of_weight_zero_get_exactly_zero(dev, ops, name):
    case = T.BY_NAME[name]
    inp = T.inputs(case)
    grad = _tv(ops, dev, case)[2].cpu()
    w = torch.tensor(inp["weights"]).reshape(grad.shape[-2:])
    assert bool((w == 0).any()) and not bool(grad[..., w == 0].any()) and bool(grad[..., w != 0].any())


# ---------------------------------------------------------------- 3. reproducibility and accumulation
@pytest.mark.parametrize("name", ["sh2_987_distinct", "rgba_987_third"])
def test_same_bytes_on_every_call_and_exact_accumulation(dev, ops, name):
    case = T.BY_NAME[name]
    a32, a64, ga = _tv(ops, dev, case)
    b32, b64, gb = _tv(ops, dev, case)
    assert torch.equal(a32, b32) and torch.equal(a64, b64) and torch.equal(ga, gb) and bool(ga.any())
    _tv(ops, dev, case, grad_out=gb)                       # a second call into the same buffer: g + g is exact
    assert torch.equal(gb, 2.0 * ga)
    quarter = _tv(ops, dev, case, scale=0.25)[2]           # scaling by a power of two is exact
    assert torch.equal(quarter, 0.25 * ga)
    on_device = _tv(ops, dev, case, scale=torch.full((1,), 0.25, device=dev))[2]
    assert torch.equal(on_device, quarter)


def test_canaries_around_the_gradient_buffer_stay(dev, ops):
    case = T.BY_NAME["sh2_253_distinct"]
    inp, _, g64, _, g32 = T.reference(case)
    n, guard = inp["stored"].size, 64
    big = torch.full((n + 2 * guard,), 7.25, dtype=torch.float32, device=dev)
    out = big[guard:guard + n].view(inp["stored"].shape)
    out.zero_()
    assert _tv(ops, dev, case, grad_out=out)[2] is out
    _hold("into a view", out, g64, g32)
    assert bool((big[:guard] == 7.25).all()) and bool((big[guard + n:] == 7.25).all())


# ---------------------------------------------------------------- 4. sparse against dense, every cell on
@pytest.mark.parametrize("name", sorted(T.DENSE_OF))
def test_sparse_with_every_cell_on_gives_the_bytes_of_the_dense_entry(dev, ops, name):
    """the same float4 goes to the same thread of the same launch in both forms, so the value's reduction order is equal too: the
    value is held byte-equal, not merely within the bar"""
    sparse, dense = T.BY_NAME[name], T.BY_NAME[T.DENSE_OF[name]]
    s32, s64, gs = _tv(ops, dev, sparse)
    d32, d64, gd = _tv(ops, dev, dense)
    assert torch.equal(s32, d32) and torch.equal(s64, d64)
    ids = _t(T.inputs(sparse)["ids"], dev).long()
    assert torch.equal(gs, gd.reshape((-1,) + tuple(gd.shape[3:]))[ids]) and bool(gs.any())


def test_empty_sparse_volume_writes_zero(dev, ops):
    index = torch.full((4, 3, 2), -1, dtype=torch.int32, device=dev)
    rows, ids = torch.empty((0, 4), device=dev), torch.empty((0,), dtype=torch.int32, device=dev)
    grad = torch.empty((0, 4), device=dev)
    v32, v64 = ops.baked_tv(rows, None, (4, 3, 2), [1.0] * 4, index=index, ids=ids, grad_out=grad)
    assert float(v32) == 0.0 and float(v64) == 0.0


# ---------------------------------------------------------------- 6. autograd, the module and the volumes
@pytest.mark.parametrize("kind", ["rgba", "sh2", "sparse"])
def test_module_tv_backpropagates_the_direct_gradient(dev, ops, bake, kind):
    case = T.BY_NAME["sh2_987_distinct" if kind == "sh2" else "rgba_987_ones"]
    inp = T.inputs(case)
    stored = _t(inp["stored"], dev)
    volume = (bake.BakedSHVolume if kind == "sh2" else bake.BakedVolume).from_tensor(stored, G.C1, G.C2, skip_threshold=5.0)   # (28 % of the cells)
    prior = dict(rgb=0.75, sigma=0.5, sh=None if kind != "sh2" else 1.25, eps=T.EPS)
    w = bake._tv_weights("test", case.degree, prior["rgb"], prior["sigma"], prior["sh"])
    kept, extra = None, {}
    if kind == "sparse":
        volume = volume.sparse()
        assert 0 < volume.n_rows < stored.shape[0] * stored.shape[1] * stored.shape[2]
        kept, extra = (volume.index >= 0).cpu().numpy(), dict(index=volume.index, ids=volume.ids)
    refs = []
    for dtype in (torch.float64, torch.float32):
        value, g = T.value_and_gradient(inp["stored"], w, T.EPS, kept, dtype)
        if kind == "sparse":
            g = g.reshape(-1, 4)[volume.ids.cpu().long()]
        refs += [value, g]
    v64, g64, v32, g32 = refs
    module = volume.trainable()
    direct = torch.zeros_like(module.stored)
    d32, _ = ops.baked_tv(module.stored.detach(), case.degree, case.reso, w, eps=T.EPS, grad_out=direct, **extra)
    _hold(kind + " direct gradient", direct, g64, g32)
    value = module.tv(**prior)
    assert value.requires_grad and value.dim() == 0 and value.dtype == torch.float32 and torch.equal(value.detach(), d32)
    _hold(kind + " module.tv()", value, v64, v32)
    assert volume.tv(**prior) == float(d32)                # the volume's own method: the same number, as a float, no graph
    value.backward(retain_graph=True)
    assert torch.equal(module.stored.grad, direct)         # grad_output = 1 on the device: the bytes of the direct call
    module.stored.grad = None
    value.backward()                                       # a second backward: nothing was consumed
    assert torch.equal(module.stored.grad, direct)
    module.stored.grad = None
    (3 * module.tv(**prior)).backward()
    _hold(kind + " (3 tv).backward()", module.stored.grad, g64, g32, scale=3.0)


# ---------------------------------------------------------------- 7., 8. fit
def test_fit_with_the_prior_follows_the_host_loop_and_smooths(dev, bake):
    """util.bake.fit on baked_grad_ref.fit_scene (12^3, RGBA) with the prior of baked_tv_ref.FIT_TV, against the same loop through the
    fp32 restatement on the CPU (the same batches, the same optimiser).  The tolerance is the one test_hip_baked_backward.py applies
    to fit without a prior: 10 x the spread between the fp32 and the fp64 restatement runs of the final batch loss.  As there, the
    fp32 run depends on the host (torch orders its fp32 reductions by the threads it has), so the spread was measured on two hosts
    and the larger one is taken:
        fp64 3.5395152164e-04; fp32 3.5395150189e-04 (1 and 8 threads) and 3.5395161831e-04 (the GPU machine's host, 16 threads):
        spread 1.98e-11 and 9.67e-11, margin 9.7e-10
    (measured on the MI355X in two runs -- the march's backward adds with atomics, so runs differ --: final loss 3.5395182204e-04 and
    3.5395170562e-04, 2.04e-10 and 8.7e-11 from that host's fp32 loop).  The prior must also do its work:
    TV(fitted with) / TV(fitted without) <= (1 + r_host) / 2 with r_host the ratio of the host loop, which
    tests/test_baked_tv_host.py holds to <= 0.5 (measured: ratio 0.4193, r_host 0.4193, bound 0.7097)."""
    margin = 9.7e-10
    known, start, rays = (_t(np.array(a), dev) for a in G.fit_scene(None))
    target = bake.BakedVolume.from_tensor(known, G.FIT_C1, G.FIT_C2).render(rays, step=G.FIT_STEP, skip=False).rgb
    volume = bake.BakedVolume.from_tensor(start, G.FIT_C1, G.FIT_C2)
    plain, plain_losses = bake.fit(volume, rays, target, step=G.FIT_STEP, **G.FIT)
    fitted, losses = bake.fit(volume, rays, target, step=G.FIT_STEP, **G.FIT, **T.FIT_TV)
    host_plain = T.fit_ref(None, torch.float32, **G.FIT)
    host = T.fit_ref(None, torch.float32, **G.FIT, **T.FIT_TV)
    r_host = T.tv_of(host[1], None, **T.FIT_TV) / T.tv_of(host_plain[1], None, **T.FIT_TV)
    ratio = T.tv_of(fitted.vol.cpu().numpy(), None, **T.FIT_TV) / T.tv_of(plain.vol.cpu().numpy(), None, **T.FIT_TV)
    prior = {k[3:]: v for k, v in T.FIT_TV.items()}
    by_method = fitted.tv(**prior) / plain.tv(**prior)
    print(f"fit with the prior: first {losses[0]:.6e} (host {host[0][0]:.6e}), final {losses[-1]:.10e} (host {host[0][-1]:.10e}), "
          f"|difference| {abs(losses[-1] - host[0][-1]):.3e}, margin {margin:.1e}; TV ratio {ratio:.4f} (volume.tv: {by_method:.4f}), "
          f"r_host {r_host:.4f}, bound {(1 + r_host) / 2:.4f}; without the prior: final {plain_losses[-1]:.9e}")
    assert len(losses) == G.FIT["steps"] and type(fitted) is bake.BakedVolume and torch.equal(volume.vol, start)
    assert abs(losses[-1] - host[0][-1]) <= margin
    assert r_host <= 0.5 and ratio <= (1 + r_host) / 2
    assert abs(by_method - ratio) <= 1e-5 * ratio


def test_fit_without_weights_never_calls_the_prior(dev, ops, bake, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("ops.baked_tv was called")
    monkeypatch.setattr(ops, "baked_tv", refuse)
    known, start, rays = (_t(np.array(a), dev) for a in G.fit_scene(None))
    volume = bake.BakedVolume.from_tensor(start, G.FIT_C1, G.FIT_C2)
    fit = dict(G.FIT, steps=3)
    _, losses = bake.fit(volume, rays, known.new_zeros(rays.shape[0], 3), step=G.FIT_STEP, **fit, tv_rgb=0.0, tv_sigma=0.0, tv_sh=0.0)
    assert len(losses) == 3
    with pytest.raises(AssertionError, match="ops.baked_tv was called"):
        bake.fit(volume, rays, known.new_zeros(rays.shape[0], 3), step=G.FIT_STEP, **fit, tv_sigma=1e-3)


# ---------------------------------------------------------------- 9. refusals
def test_half_and_non_contiguous_volumes_are_refused_in_their_own_words(dev, ops, bake):
    case = T.BY_NAME["rgba_987_ones"]
    stored = _t(T.inputs(case)["stored"], dev)
    with pytest.raises(TypeError, match=r"gradients exist for fp32 volumes only; fit the volume in fp32 and call half\(\) afterwards"):
        ops.baked_tv(stored.half(), None, case.reso, [1.0] * 4)
    with pytest.raises(TypeError, match=r"BakedVolume.tv: gradients exist for fp32 volumes only"):
        bake.BakedVolume.from_tensor(stored, G.C1, G.C2).half().tv()
    swapped = stored.permute(1, 0, 2, 3)    # (8,9,7,4), not contiguous
    with pytest.raises(ValueError, match="stored must be contiguous"):
        ops.baked_tv(swapped, None, (8, 9, 7), [1.0] * 4)
    grad = torch.zeros_like(stored).permute(1, 0, 2, 3)
    with pytest.raises(ValueError, match="grad_out must be a contiguous float32 tensor"):
        ops.baked_tv(swapped.contiguous(), None, (8, 9, 7), [1.0] * 4, grad_out=grad)
