"""GPU tests (-m gpu) of the baked march's backward: pnr_baked_backward_rays / _views through ops.baked_render_backward /
ops.baked_render_views_backward, the autograd Function behind `volume.trainable()` and util.bake.fit.

The yardstick is tests/baked_grad_ref.py -- the march restated in torch, its gradient by autograd in fp64 (its own checks:
tests/test_baked_backward_host.py).  Error and bar are tests/position_ref.py's: error = max|got - ref64| / max|ref64|, bar = 10 x the
error of torch's fp32 autograd through the same restatement on the same inputs (floor 2e-6, cap 2e-4).  Every test prints the HIP
error, the torch-fp32 error and the bar before it asserts."""
import numpy as np
import pytest
import torch

import baked_grad_ref as G
import sparse_baked_ref as SP
from testdata import synthetic

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


def _bits(cells, dev):
    return None if cells is None else torch.from_numpy(SP.bits_from_cells(cells).copy()).to(dev)


def _backward(ops, dev, inp, case, stored=None, **kw):
    """ops.baked_render_backward on the inputs of a case (stored: another tensor in place of the case's)"""
    stored = _t(inp["stored"], dev) if stored is None else stored
    args = dict(d_rgb=_t(inp["d_rgb"], dev), d_depth=_t(inp["d_depth"], dev), d_alpha=_t(inp["d_alpha"], dev),
                bits=_bits(inp["occupied"], dev), white_bkgd=case.white, terminate=case.terminate)
    args.update(kw)
    return ops.baked_render_backward(_t(inp["rays"], dev), stored, case.kind, G.RESO, G.C1, G.C2, inp["step"], **args)


def _hold(what, got, ref64, ref32, scale=1.0):
    """print the three numbers, then hold `got` to the bar; scale: what the reference is multiplied by"""
    err, err32 = G.error(got.cpu(), ref64 * scale), G.error(ref32.double() * scale, ref64 * scale)
    bar = G.bar_from(err32)
    print(f"{what}: HIP error {err:.3e}, torch-fp32 error {err32:.3e}, bar {bar:.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert err <= bar, (what, err, bar)
    return bar


# ---------------------------------------------------------------- 1. the entry against the fp64 gradient
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_gradient_of_every_case_is_within_its_bar(dev, ops, name):
    """sample counts below, at and above a chunk and beyond the 64 chunk heads held in lanes; an opaque sample in the middle of a
    ray; each upstream gradient alone and all together; white background; degrees 0, 1, 2 with corners clamped on both sides; bits
    at threshold 0 and above; terminate over the dense part.  The rays that miss the box and the one with near >= far are in every
    case but the long one."""
    case = G.BY_NAME[name]
    inp, ref64, ref32 = G.reference(case)
    got = _backward(ops, dev, inp, case)
    assert got.shape == ref64.shape and got.dtype == torch.float32
    _hold(name, got, ref64, ref32)
    assert bool((got.cpu()[ref64 == 0] == 0).all()) or case.kind is None   # an SH coefficient no unclamped sample reaches: exact zero


def test_rays_without_samples_and_zero_upstream_give_exact_zeros(dev, ops):
    case = G.BY_NAME["rgba_n150"]
    inp = dict(G.inputs(case))
    rows = list(G.MISSING)
    lost = dict(inp, rays=inp["rays"][rows], d_rgb=inp["d_rgb"][rows], d_depth=inp["d_depth"][rows], d_alpha=inp["d_alpha"][rows])
    assert not bool(_backward(ops, dev, lost, case).any())
    zero = dict(inp, d_rgb=np.zeros_like(inp["d_rgb"]), d_depth=np.zeros_like(inp["d_depth"]), d_alpha=np.zeros_like(inp["d_alpha"]))
    assert not bool(_backward(ops, dev, zero, case).any())
    assert not bool(_backward(ops, dev, dict(inp, d_rgb=None, d_depth=None, d_alpha=None), case).any())
    none = ops.baked_render_backward(torch.empty((0, 8), device=dev), _t(inp["stored"], dev), None, G.RESO, G.C1, G.C2, inp["step"])
    assert none.shape == inp["stored"].shape and not bool(none.any())


def test_clamped_channels_receive_exact_zeros(dev, ops):
    """degree 1 with red above 1 and green below 0 at every corner for every ray (DC 3 and -2 against |sum_k c_k Y_k| <= 0.75):
    their coefficients receive exactly zero, blue and sigma do not"""
    case = G.BY_NAME["sh1_n150_white"]
    inp = dict(G.inputs(case))
    coef = np.array(inp["stored"])
    coef[..., 0, 0], coef[..., 0, 1] = 3.0, -2.0
    got = _backward(ops, dev, dict(inp, stored=coef), case).cpu()
    assert not bool(got[..., 0].any()) and not bool(got[..., 1].any())
    assert bool(got[..., 2].any()) and bool(got[..., 3].any())
    ref64 = G.gradient(inp["rays"], coef, G.C1, G.C2, inp["step"], inp["d_rgb"], inp["d_depth"], inp["d_alpha"], **inp["kw"])
    ref32 = G.gradient(inp["rays"], coef, G.C1, G.C2, inp["step"], inp["d_rgb"], inp["d_depth"], inp["d_alpha"], dtype=torch.float32,
                       **inp["kw"])
    _hold("sh1 clamped", got, ref64, ref32)


# ---------------------------------------------------------------- 2. sparse rows
@pytest.mark.parametrize("name", ["rgba_n150_bits10", "sh2_n150_bits10_terminate", "rgba_n150_bits0"])
def test_sparse_rows_gradient_is_the_dense_gradient_at_the_kept_points(dev, ops, name):
    case = G.BY_NAME[name]
    inp, ref64, ref32 = G.reference(case)
    index, ids = SP.sparse_points(inp["occupied"])
    tail = inp["stored"].shape[3:]
    rows = np.ascontiguousarray(inp["stored"].reshape((-1,) + tail)[ids])
    got = _backward(ops, dev, inp, case, stored=_t(rows, dev), index=_t(index, dev))
    assert got.shape == rows.shape
    flat = lambda g: g.reshape((-1,) + tail)
    keep = torch.from_numpy(ids.astype(np.int64))
    _hold(name + " rows", got, flat(ref64)[keep], flat(ref32)[keep])
    dense = _backward(ops, dev, inp, case).cpu()
    dropped = torch.ones(flat(dense).shape[0], dtype=torch.bool)
    dropped[keep] = False
    assert not bool(flat(dense)[dropped].any())          # nothing outside the kept set: the bits keep the march off it
    err = G.error(got.cpu(), flat(dense)[keep].double())
    print(f"{name}: rows against the dense gradient gathered at ids {err:.3e}")
    assert err <= G.bar_from(G.error(ref32, ref64))


# ---------------------------------------------------------------- 3. atomics: contention, accumulation, bounds
def test_2048_copies_of_one_ray(dev, ops):
    """every atomic of the launch lands on the same few hundred addresses; the reference (fp64 and torch fp32) is computed on the
    2048 copies themselves, and equals 2048 x the single-ray gradient"""
    many, single64, ref64, ref32 = G.contention()
    assert many["rays"].shape[0] == G.COPIES == 2048 and G.error(ref64, 2048.0 * single64) < 1e-12
    got = _backward(ops, dev, many, G.BY_NAME["rgba_n40"])
    _hold("2048 copies", got, single64, ref32 / 2048.0, scale=2048.0)


@pytest.mark.parametrize("name", ["rgba_n150", "sh2_n150"])
def test_second_call_doubles_and_canaries_stay(dev, ops, name):
    case = G.BY_NAME[name]
    inp, ref64, ref32 = G.reference(case)
    shape, width = inp["stored"].shape, int(np.prod(inp["stored"].shape[3:]))
    points, guard = int(np.prod(shape[:3])), 8
    big = torch.full(((points + 2 * guard) * width,), 7.25, dtype=torch.float32, device=dev)
    out = big[guard * width:(guard + points) * width].view(shape)
    out.zero_()
    assert _backward(ops, dev, inp, case, out=out) is out
    bar = _hold(name + " first call", out, ref64, ref32)
    _backward(ops, dev, inp, case, out=out)
    _hold(name + " second call", out, ref64, ref32, scale=2.0)
    assert bool((big[:guard * width] == 7.25).all()) and bool((big[(guard + points) * width:] == 7.25).all())
    assert bar <= G.BAR_CAP


# ---------------------------------------------------------------- 4. the views entry
def test_views_entry_is_the_rays_entry_on_gen_rays(dev, ops):
    """NV = 2 views of 5 x 4 pixels, 37 of the 40 rays through the dense part (checked on the host with testdata.synthetic.gen_rays:
    every sample 2.9e-5 box edges off the faces)"""
    inp = G.inputs(G.BY_NAME["rgba_n150"])
    poses = torch.stack((synthetic.pose_spherical(35.0, -20.0, 3.0), synthetic.pose_spherical(190.0, -35.0, 3.2))).to(dev)
    W, H, focal, z_near = 5, 4, 14.0, 1.2
    z_far = z_near + 149.5 * 0.03
    rays = ops.gen_rays(poses, W, H, focal, z_near, z_far).reshape(-1, 8)
    R = rays.shape[0]
    assert R == 2 * H * W
    rs = np.random.RandomState(99)
    up = [rs.standard_normal(s).astype(np.float32) for s in ((R, 3), (R,), (R,))]
    info = {}
    G.march(rays.cpu().numpy(), torch.from_numpy(inp["stored"]).double(), G.C1, G.C2, 0.03, info=info)
    assert info["face_margin"] > 1e-5 and set(info["n"]) == {150}
    ref = lambda dtype: G.gradient(rays.cpu().numpy(), inp["stored"], G.C1, G.C2, 0.03, *up, dtype=dtype, white_bkgd=True)
    ref64, ref32 = ref(torch.float64), ref(torch.float32)
    assert float(ref64.abs().max()) > 0
    vol = _t(inp["stored"], dev)
    kw = dict(d_rgb=_t(up[0], dev), d_depth=_t(up[1], dev), d_alpha=_t(up[2], dev), white_bkgd=True)
    by_rays = ops.baked_render_backward(rays, vol, None, G.RESO, G.C1, G.C2, 0.03, **kw)
    by_views = ops.baked_render_views_backward(poses, W, H, focal, None, z_near, z_far, vol, None, G.RESO, G.C1, G.C2, 0.03, **kw)
    bar = _hold("rays(gen_rays)", by_rays, ref64, ref32)
    _hold("views", by_views, ref64, ref32)
    assert G.error(by_views.cpu(), by_rays.cpu().double()) <= bar


# ---------------------------------------------------------------- 5. autograd and the trainable module
@pytest.mark.parametrize("kind", ["rgba", "sh2", "sparse"])
def test_trainable_renders_the_bytes_of_render_and_backpropagates(dev, ops, bake, kind):
    case = G.BY_NAME["sh2_n150" if kind == "sh2" else "rgba_n150"]
    inp, ref64, ref32 = G.reference(case)
    stored, rays = _t(inp["stored"], dev), _t(inp["rays"], dev)
    volume = (bake.BakedSHVolume if kind == "sh2" else bake.BakedVolume).from_tensor(stored, G.C1, G.C2, skip_threshold=10.0)
    skip = False
    if kind == "sparse":   # the kept rows of the skip grid: the dense reference with the same cells
        volume, skip = volume.sparse(), True
        cells = SP.cells_from_bits(volume.occupancy.bits.cpu().numpy(), G.RESO)
        args = (inp["rays"], inp["stored"], G.C1, G.C2, inp["step"], inp["d_rgb"], inp["d_depth"], inp["d_alpha"])
        keep = volume.ids.cpu().long()
        ref64, ref32 = (G.gradient(*args, dtype=dt, occupied=cells).reshape(-1, 4)[keep] for dt in (torch.float64, torch.float32))
    module = volume.trainable()
    assert isinstance(module, torch.nn.Module) and [p.shape for p in module.parameters()] == [volume._stored().shape]
    plain = volume.render(rays, step=inp["step"], skip=skip)
    assert not plain.rgb.requires_grad and plain.rgb.grad_fn is None
    out = module(rays, step=inp["step"], skip=skip)
    assert out.rgb.requires_grad and out.depth.requires_grad and out.alpha.requires_grad
    assert torch.equal(out.rgb, plain.rgb) and torch.equal(out.depth, plain.depth) and torch.equal(out.alpha, plain.alpha)
    loss = (out.rgb * _t(inp["d_rgb"], dev)).sum() + (out.depth * _t(inp["d_depth"], dev)).sum() + (out.alpha * _t(inp["d_alpha"], dev)).sum()
    loss.backward()
    _hold(kind + " loss.backward()", module.stored.grad, ref64, ref32)
    again = volume.render(rays, step=inp["step"], skip=skip)   # render keeps its no_grad behaviour and its bytes
    assert not again.rgb.requires_grad and torch.equal(again.rgb, plain.rgb)
    with torch.no_grad():
        module.stored[..., 3].mul_(0.5)
    fresh = module.volume()
    assert type(fresh) is type(volume) and torch.equal(fresh._stored(), module.stored.detach()) and fresh._stored() is not module.stored
    assert not torch.equal(fresh._stored(), volume._stored())   # the volume trainable() was called on is unchanged
    with pytest.raises(TypeError, match=r"fit the volume in fp32 and call half\(\) afterwards"):
        volume.half().trainable()
    with pytest.raises(ValueError, match="no gradient is given with respect to rays"):
        module(rays.clone().requires_grad_(True), step=inp["step"], skip=skip)


def test_trainable_forward_views_matches_forward_on_gen_rays(dev, ops, bake):
    inp = G.inputs(G.BY_NAME["rgba_n150"])
    volume = bake.BakedVolume.from_tensor(_t(inp["stored"], dev), G.C1, G.C2)
    poses = torch.stack((synthetic.pose_spherical(35.0, -20.0, 3.0), synthetic.pose_spherical(190.0, -35.0, 3.2))).to(dev)
    W, H, focal, z_near, z_far = 5, 4, 14.0, 1.2, 1.2 + 149.5 * 0.03
    a, b = volume.trainable(), volume.trainable()
    va = a.forward_views(poses, W, H, focal, z_near, z_far, step=0.03)
    vb = b(ops.gen_rays(poses, W, H, focal, z_near, z_far), step=0.03)
    plain = volume.render_views(poses, W, H, focal, z_near, z_far, step=0.03, skip=False)
    assert torch.equal(va.rgb, vb.rgb) and torch.equal(va.rgb, plain.rgb) and torch.equal(va.depth, plain.depth)
    (va.rgb.sum() + va.depth.sum()).backward()
    (vb.rgb.sum() + vb.depth.sum()).backward()
    err = G.error(a.stored.grad.cpu(), b.stored.grad.cpu().double())
    print(f"forward_views against forward(gen_rays): {err:.3e}")
    assert float(b.stored.grad.abs().max()) > 0 and err <= 2e-6   # the same sums in another order: the floor of the bar


# ---------------------------------------------------------------- 6. fit
@pytest.mark.parametrize("degree", [None, 1])
def test_fit_lowers_the_loss_as_the_host_loop_does(dev, bake, degree):
    """util.bake.fit on a 12^3 grid (RGBA, and degree 1), 512 rays, the target rendered from a known volume, the start a perturbed
    copy, 40 steps of Adam (lr 2e-2) on batches of 128: the final batch loss is below the first, and within a margin of the final
    loss of the same loop through the fp32 restatement on the CPU (baked_grad_ref.fit_ref: the same batches, the same optimiser).
    The margin is 10 x the spread between the fp32 and the fp64 restatement runs (the factor of the gradient bar).  The fp32 run
    depends on the host -- torch orders its fp32 reductions by the threads it has --, so the spread was measured on two hosts and the
    larger one is taken:
        RGBA      final loss fp64 3.077804285203109e-05; fp32 3.077805376960896e-05 (8 threads) and 3.077800284e-05 (the GPU
                  machine's host): spread 1.09e-11 and 4.00e-11, margin 4.0e-10
        degree 1  final loss fp64 2.0680260801468823e-04; fp32 2.0680252055171877e-04 and 2.068024041e-04: spread 8.75e-11 and
                  2.04e-10, margin 2.0e-9
    (the first losses are 1.348e-03 and 3.218e-03: the final ones are 2 % and 6 % of them)."""
    margin = {None: 4.0e-10, 1: 2.0e-9}[degree]
    known, start, rays = (_t(np.array(a), dev) for a in G.fit_scene(degree))
    cls = bake.BakedVolume if degree is None else bake.BakedSHVolume
    target = cls.from_tensor(known, G.FIT_C1, G.FIT_C2).render(rays, step=G.FIT_STEP, skip=False).rgb
    volume = cls.from_tensor(start, G.FIT_C1, G.FIT_C2)
    fitted, losses = bake.fit(volume, rays, target, step=G.FIT_STEP, **G.FIT)
    host = G.fit_ref(degree, torch.float32, **G.FIT)
    print(f"fit degree {degree}: first {losses[0]:.6e} (host {host[0]:.6e}), final {losses[-1]:.9e} (host {host[-1]:.9e}), "
          f"|difference| {abs(losses[-1] - host[-1]):.3e}, margin {margin:.1e}")
    assert len(losses) == G.FIT["steps"] and type(fitted) is cls and fitted is not volume
    assert torch.equal(volume._stored(), start)            # fit leaves the volume it was given alone
    assert losses[-1] < losses[0]
    assert abs(losses[-1] - host[-1]) <= margin
    if degree is None:
        assert float(fitted.vol[..., :3].min()) >= 0.0 and float(fitted.vol[..., :3].max()) <= 1.0 and float(fitted.vol[..., 3].min()) >= 0.0
