"""GPU tests (-m gpu) of the baked march's gradient with respect to its rays: pnr_baked_ray_backward_rays / _views through
ops.baked_ray_backward / ops.baked_ray_backward_views, autograd.baked_march_rays_autograd, `render_diff` / `render_views_diff` of
the volume classes, the opt-in flags of TrainableBaked and util.bake.register.

The yardstick is tests/baked_ray_grad_ref.py -- the march restated in torch with the rays as leaves, its gradient by autograd in fp64
(its own checks: tests/test_baked_ray_grad_host.py) -- on the rows its rule keeps: a sample on a cell plane has a one-sided
derivative that fp32 and fp64 take from different cells.  Error and bar are tests/position_ref.py's: error = max|got - ref64| /
max|ref64|, bar = 10 x the error of torch's fp32 autograd through the same restatement (floor 2e-6, cap 2e-4).  Every test prints
the HIP error, the torch-fp32 error and the bar before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_ray_grad_ref as RG
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


def _ray_backward(ops, dev, inp, case, stored=None, **kw):
    """ops.baked_ray_backward on the inputs of a case (stored: another tensor in place of the case's)"""
    stored = _t(inp["stored"], dev) if stored is None else stored
    args = dict(d_rgb=_t(inp["d_rgb"], dev), d_depth=_t(inp["d_depth"], dev), d_alpha=_t(inp["d_alpha"], dev),
                bits=_bits(inp["occupied"], dev), white_bkgd=case.white, terminate=case.terminate)
    args.update(kw)
    return ops.baked_ray_backward(_t(inp["rays"], dev), stored, case.kind, G.RESO, G.C1, G.C2, inp["step"], **args)


def _sparse(inp, dev):
    """-> (rows, index) on the device: the kept rows of the case's volume under its skip grid"""
    index, ids = SP.sparse_points(inp["occupied"])
    tail = inp["stored"].shape[3:]
    return _t(np.ascontiguousarray(inp["stored"].reshape((-1,) + tail)[ids]), dev), _t(index, dev)


# ---------------------------------------------------------------- 1. the entry against the fp64 gradient
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_ray_gradient_of_every_case_is_within_its_bar(dev, ops, name):
    """grid (9,8,7); 40, 64, 150 and 4500 samples -- below, at and above a chunk and 71 chunks, 7 beyond the heads held in lanes --;
    an opaque sample; each upstream gradient alone and all together; white background; degrees 0, 1, 2 with corners clamped on both
    sides (the basis' share of d_d); bits at threshold 0 and above; terminate.  On the kept rows; a second call gives the same
    bytes; the rays without samples get exact zeros and d_far is exactly zero everywhere."""
    case = G.BY_NAME[name]
    inp, kept, ref64, ref32 = RG.reference(case)
    got = _ray_backward(ops, dev, inp, case)
    assert got.shape == ref64.shape and got.dtype == torch.float32
    RG.hold(name, got.cpu(), ref64, ref32, kept)
    assert torch.equal(got, _ray_backward(ops, dev, inp, case))
    assert not bool(got[:, 7].any())
    if case.rows is None:
        assert not bool(got[list(G.MISSING)].any())
    assert not bool(got.cpu()[(ref64 == 0).all(dim=1)].any())   # a ray the reference gives nothing gets exact zeros


# ---------------------------------------------------------------- 2. layouts and storages: the same bytes
@pytest.mark.parametrize("name", ["rgba_n150_bits10", "sh2_n150_bits10_terminate"])
def test_sparse_rows_give_the_bytes_of_the_dense_call(dev, ops, name):
    case = G.BY_NAME[name]
    inp = G.inputs(case)
    rows, index = _sparse(inp, dev)
    dense = _ray_backward(ops, dev, inp, case)
    assert bool(dense.any()) and torch.equal(_ray_backward(ops, dev, inp, case, stored=rows, index=index), dense)


@pytest.mark.parametrize("layout", ["dense", "sparse"])
@pytest.mark.parametrize("name", ["rgba_n150_bits10", "sh2_n150_bits10_terminate"])
def test_half_volume_gives_the_bytes_of_its_widened_values(dev, ops, name, layout):
    """fp16 -> fp32 is exact: the half instantiation runs the fp32 one's operations on the widened values"""
    case = G.BY_NAME[name]
    inp = G.inputs(case)
    stored, kw = _t(inp["stored"], dev), {}
    if layout == "sparse":
        stored, kw["index"] = _sparse(inp, dev)
    half = stored.half()
    got = _ray_backward(ops, dev, inp, case, stored=half, **kw)
    assert half.dtype == torch.float16 and bool(got.any()) and bool(torch.isfinite(got).all())
    assert torch.equal(got, _ray_backward(ops, dev, inp, case, stored=half.float(), **kw))
    assert not torch.equal(got, _ray_backward(ops, dev, inp, case, stored=stored, **kw))   # (the rounding of the volume does show)


# ---------------------------------------------------------------- 3. every row is written
@pytest.mark.parametrize("name", ["rgba_n150", "sh2_n150"])
def test_every_row_is_written_and_exact_zeros_where_nothing_comes_back(dev, name):
    """the library entry itself, on a buffer pre-filled with NaN and with guard rows around it: rays that miss the box, the ray with
    near >= far and every ray whose upstream gradients are all zero (given as zeros, or not given) get a row of exact zeros;
    column 7 is exactly 0; nothing outside the (R,8) rows is touched"""
    from pixelnerf_amd import _lib
    lib = _lib.load()
    case = G.BY_NAME[name]
    inp = G.inputs(case)
    rays, stored = _t(inp["rays"], dev), _t(inp["stored"], dev)
    R, guard = rays.shape[0], 4
    f3 = ctypes.c_float * 3
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(d_rgb, d_depth, d_alpha):
        big = torch.full(((R + 2 * guard), 8), float("nan"), dtype=torch.float32, device=dev)
        out = big[guard:guard + R]
        with torch.cuda.device(dev):
            rc = lib.pnr_baked_ray_backward_rays(rays.data_ptr(), R, stored.data_ptr(), 0, 0, -1 if case.kind is None else case.kind, None,
                                                 None, *G.RESO, f3(*G.C1), f3(*G.C2), inp["step"], int(case.white), case.terminate,
                                                 ptr(d_rgb), ptr(d_depth), ptr(d_alpha), out.data_ptr(),
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[guard + R:]).all())
        return out

    ups = [_t(inp[k], dev) for k in ("d_rgb", "d_depth", "d_alpha")]
    full = call(*ups)
    assert bool(torch.isfinite(full).all()) and not bool(full[:, 7].any())
    missing = torch.zeros(R, dtype=torch.bool)
    missing[list(G.MISSING)] = True
    assert not bool(full[missing].any()) and bool(full[~missing].any())
    zeroed = [u.clone() for u in ups]
    some = [0, 3, 17, 30, 35]
    for u in zeroed:
        u[some] = 0
    part = call(*zeroed)
    assert not bool(part[some].any())
    others = torch.ones(R, dtype=torch.bool)
    others[some] = False
    assert torch.equal(part[others], full[others])
    for none in (call(None, None, None), call(*[torch.zeros_like(u) for u in ups])):
        assert torch.equal(none, torch.zeros_like(none))


# ---------------------------------------------------------------- 4. the views entry and the pose chain
def _views_case(dev, kind):
    """2 views of 5 x 4 pixels through the common volume (RGBA, or degree 2), upstream gradients zeroed on the rays the rule drops"""
    case = G.BY_NAME["rgba_n150" if kind is None else "sh2_n150"]
    inp = G.inputs(case)
    poses = torch.stack([synthetic.pose_spherical(*a) for a in RG.VIEW_ANGLES]).float()
    v = RG.VIEWS
    rays64 = RG.gen_rays(poses.double(), v["W"], v["H"], v["focal"], v["z_near"], v["z_far"]).reshape(-1, 8)
    kept = RG.kept_rows(rays64.float().numpy(), step=v["step"])
    R = rays64.shape[0]
    assert R == 40 and int(kept.sum()) >= 37
    rs = np.random.RandomState(99)
    ups = [rs.standard_normal(s).astype(np.float32) for s in ((R, 3), (R,), (R,))]
    for u in ups:
        u[~kept.numpy()] = 0
    return case, inp, poses, ups


@pytest.mark.parametrize("kind", [None, 2])
def test_views_entry_is_the_rays_entry_on_gen_rays_and_the_pose_chain_holds(dev, ops, bake, kind):
    case, inp, poses, ups = _views_case(dev, kind)
    v = RG.VIEWS
    W, H, focal, z_near, z_far, step = (v[k] for k in ("W", "H", "focal", "z_near", "z_far", "step"))
    stored, poses_d = _t(inp["stored"], dev), poses.to(dev)
    kw = dict(d_rgb=_t(ups[0], dev), d_depth=_t(ups[1], dev), d_alpha=_t(ups[2], dev), white_bkgd=True)
    rays = ops.gen_rays(poses_d, W, H, focal, z_near, z_far)
    by_rays = ops.baked_ray_backward(rays.reshape(-1, 8), stored, kind, G.RESO, G.C1, G.C2, step, **kw)
    by_views = ops.baked_ray_backward_views(poses_d, W, H, focal, None, z_near, z_far, stored, kind, G.RESO, G.C1, G.C2, step, **kw)
    assert by_views.shape == (2, H, W, 8) and bool(by_rays.any())
    assert torch.equal(by_views.reshape(-1, 8), by_rays)
    ref64, rays64 = RG.pose_gradients(poses.numpy(), inp["stored"], *ups, torch.float64, degree=kind, white_bkgd=True)
    ref32, rays32 = RG.pose_gradients(poses.numpy(), inp["stored"], *ups, torch.float32, degree=kind, white_bkgd=True)
    RG.hold(f"views d_rays (kind {kind})", by_rays.cpu(), rays64, rays32)
    cls = bake.BakedVolume if kind is None else bake.BakedSHVolume
    volume = cls.from_tensor(stored, G.C1, G.C2)
    leaf = poses_d.clone().requires_grad_(True)
    out = volume.render_views_diff(leaf, W, H, focal, z_near, z_far, step=step, white_bkgd=True, skip=False)
    plain = volume.render_views(poses_d, W, H, focal, z_near, z_far, step=step, white_bkgd=True, skip=False)
    assert torch.equal(out.rgb, plain.rgb) and torch.equal(out.depth, plain.depth) and torch.equal(out.alpha, plain.alpha)
    loss = (out.rgb.reshape(-1, 3) * kw["d_rgb"]).sum() + (out.depth.reshape(-1) * kw["d_depth"]).sum() + (out.alpha.reshape(-1) * kw["d_alpha"]).sum()
    loss.backward()
    assert leaf.grad.shape == (2, 4, 4) and not bool(leaf.grad[:, 3].any())
    RG.hold(f"d_poses (kind {kind})", leaf.grad.cpu(), ref64, ref32)
    assert torch.equal(leaf.grad, ops.gen_rays_backward(by_views, W, H, focal))


def test_render_diff_carries_the_bytes_of_render_on_every_volume_class(dev, ops, bake):
    """dense, view-dependent, sparse and half: the forward is `render`'s, the backward the direct call's bytes"""
    for name in ("rgba_n150_bits10", "sh2_n150_bits10_terminate"):
        case = G.BY_NAME[name]
        inp = G.inputs(case)
        cls = bake.BakedVolume if case.kind is None else bake.BakedSHVolume
        dense = cls.from_tensor(_t(inp["stored"], dev), G.C1, G.C2, skip_threshold=10.0)
        for volume in (dense, dense.sparse(), dense.half(), dense.sparse().half()):
            rays = _t(inp["rays"], dev).requires_grad_(True)
            out = volume.render_diff(rays, step=inp["step"], white_bkgd=case.white, terminate=case.terminate)
            plain = volume.render(rays.detach(), step=inp["step"], white_bkgd=case.white, terminate=case.terminate)
            assert out.rgb.requires_grad and torch.equal(out.rgb, plain.rgb) and torch.equal(out.depth, plain.depth) and torch.equal(out.alpha, plain.alpha)
            ups = [_t(inp[k], dev) for k in ("d_rgb", "d_depth", "d_alpha")]
            ((out.rgb * ups[0]).sum() + (out.depth * ups[1]).sum() + (out.alpha * ups[2]).sum()).backward()
            sparse = volume._stored_name == "rows"
            direct = ops.baked_ray_backward(rays.detach(), volume._stored(), case.kind, G.RESO, G.C1, G.C2, inp["step"], d_rgb=ups[0],
                                            d_depth=ups[1], d_alpha=ups[2], bits=volume.occupancy.bits, index=volume.index if sparse else None,
                                            white_bkgd=case.white, terminate=case.terminate)
            assert bool(direct.any()) and torch.equal(rays.grad, direct)


# ---------------------------------------------------------------- 5. rays and stored values together
@pytest.mark.parametrize("name", ["rgba_n150", "sh2_n150"])
def test_joint_gradients_of_rays_and_stored_values(dev, ops, bake, name):
    from pixelnerf_amd import autograd
    case = G.BY_NAME[name]
    inp, st64, st32 = G.reference(case)
    ups = [_t(inp[k], dev) for k in ("d_rgb", "d_depth", "d_alpha")]
    total = lambda o: (o[0] * ups[0]).sum() + (o[1] * ups[1]).sum() + (o[2] * ups[2]).sum()
    direct = _ray_backward(ops, dev, inp, case)
    err32 = G.error(st32.double(), st64)

    stored, rays = _t(inp["stored"], dev).requires_grad_(True), _t(inp["rays"], dev).requires_grad_(True)
    out = autograd.baked_march_rays_autograd(stored, (rays,), case.kind, G.RESO, G.C1, G.C2, inp["step"])
    total(out).backward()
    err = G.error(stored.grad.cpu(), st64)
    print(f"{name} joint: d_stored HIP error {err:.3e}, torch-fp32 error {err32:.3e}, bar {G.bar_from(err32):.3e}")
    assert err <= G.bar_from(err32) and torch.equal(rays.grad, direct)

    cls = bake.BakedVolume if case.kind is None else bake.BakedSHVolume
    module = cls.from_tensor(_t(inp["stored"], dev), G.C1, G.C2).trainable()
    rays = _t(inp["rays"], dev).requires_grad_(True)
    o = module(rays, step=inp["step"], ray_grad=True)
    assert torch.equal(o.rgb, out[0]) and torch.equal(o.depth, out[1])
    total((o.rgb, o.depth, o.alpha)).backward()
    assert G.error(module.stored.grad.cpu(), st64) <= G.bar_from(err32) and torch.equal(rays.grad, direct)
    # the defaults keep their refusals, in their words
    with pytest.raises(ValueError, match="no gradient is given with respect to rays"):
        module(_t(inp["rays"], dev).requires_grad_(True), step=inp["step"])
    with pytest.raises(ValueError, match="no gradient is given with respect to poses"):
        module.forward_views(torch.eye(4, device=dev)[None].requires_grad_(True), 4, 4, 10.0, 0.5, 3.0)
    with pytest.raises(ValueError, match="no gradient is given with respect to rays"):
        autograd.baked_march_autograd(stored, (_t(inp["rays"], dev).requires_grad_(True),), case.kind, G.RESO, G.C1, G.C2, inp["step"])
    with pytest.raises(TypeError, match=r"fit the volume in fp32 and call half\(\) afterwards"):
        autograd.baked_march_rays_autograd(stored.detach().half().requires_grad_(True), (rays,), case.kind, G.RESO, G.C1, G.C2, inp["step"])


def test_trainable_forward_views_with_pose_grad(dev, ops, bake):
    case, inp, poses, ups = _views_case(dev, None)
    v = RG.VIEWS
    cam = (v["W"], v["H"], v["focal"], v["z_near"], v["z_far"])
    module = bake.BakedVolume.from_tensor(_t(inp["stored"], dev), G.C1, G.C2).trainable()
    leaf = poses.to(dev).requires_grad_(True)
    out = module.forward_views(leaf, *cam, step=v["step"], white_bkgd=True, pose_grad=True)
    (out.rgb.reshape(-1, 3) * _t(ups[0], dev)).sum().backward()
    d_rays = ops.baked_ray_backward_views(poses.to(dev), v["W"], v["H"], v["focal"], None, v["z_near"], v["z_far"], module.stored.detach(), None,
                                          G.RESO, G.C1, G.C2, v["step"], d_rgb=_t(ups[0], dev), white_bkgd=True)
    assert bool(leaf.grad.any()) and torch.equal(leaf.grad, ops.gen_rays_backward(d_rays, v["W"], v["H"], v["focal"]))
    assert module.stored.grad is not None and bool(module.stored.grad.any())


# ---------------------------------------------------------------- 6. registration
@pytest.mark.parametrize("how,degree", [("loop", None), ("register_skip", None), ("register", 1)])
def test_registration_converges_as_the_host_loop_does(dev, bake, how, degree):
    """A 16^3 volume on [-1,1]^3 of three coloured Gaussian blobs (a tensor, no network), three cameras at radius 2.7, 12 x 12 pixels,
    focal 14, near 1.5, far 3.9, step 0.05, white background; the start 5 degrees and 0.12 off the true pose; 120 steps of Adam at
    lr 1e-2.  The reference is the same loop through the fp32 restatement on the host (tests/baked_ray_grad_ref.register_ref; its
    fp64 run agrees: tests/test_baked_ray_grad_host.py).  Required: the mean rotation and the mean translation error each at most
    half their start; each camera's final errors within 1.25 x the host loop's; the final loss within 1.25 x the host loop's (the
    allowance is for the fp32 reordering of a wave-wide sum over 120 Adam steps).  Once as an explicit loop over render_views_diff,
    once through util.bake.register against the skip grid, once on a degree-1 volume."""
    r = RG.REG
    stored, true, start = (_t(np.array(a), dev) for a in RG.reg_scene(degree))
    cls = bake.BakedVolume if degree is None else bake.BakedSHVolume
    volume = cls.from_tensor(stored, r["c1"], r["c2"])
    cam = (r["W"], r["H"], r["focal"], r["z_near"], r["z_far"])
    target = volume.render_views(true, *cam, step=r["step"], white_bkgd=True, skip=False).rgb
    if how == "loop":
        w = torch.zeros((3, 3), device=dev, requires_grad=True)
        v = torch.zeros((3, 3), device=dev, requires_grad=True)
        optimiser = torch.optim.Adam([w, v], lr=r["lr"])
        losses = []
        for _ in range(r["steps"]):
            out = volume.render_views_diff(bake.moved_poses(start, w, v), *cam, step=r["step"], white_bkgd=True, skip=False)
            loss = ((out.rgb - target) ** 2).mean()
            optimiser.zero_grad(set_to_none=True)
            loss.backward()
            optimiser.step()
            losses.append(loss.detach())
        poses, losses = bake.moved_poses(start, w, v).detach(), torch.stack(losses).tolist()
    else:
        poses, losses = bake.register(volume, target, start, *cam, steps=r["steps"], lr=r["lr"], step=r["step"], white_bkgd=True,
                                      skip=how == "register_skip")
    assert poses.shape == (3, 4, 4) and len(losses) == r["steps"]
    host_poses, host_losses = RG.register_ref(torch.float32, degree)
    rot0, tr0 = RG.pose_errors(start, true)
    rot, tr = RG.pose_errors(poses, true)
    hrot, htr = RG.pose_errors(host_poses, true.cpu())
    for k in range(3):
        print(f"{how} degree {degree} camera {k + 1}: rotation {float(rot0[k]):.2f} -> {float(rot[k]):.3f} deg (host {float(hrot[k]):.3f}, "
              f"ratio {float(rot[k] / hrot[k]):.4f}), translation {float(tr0[k]):.3f} -> {float(tr[k]):.4f} (host {float(htr[k]):.4f}, "
              f"ratio {float(tr[k] / htr[k]):.4f})")
    print(f"{how} degree {degree}: loss {losses[0]:.4e} -> {losses[-1]:.4e} (host {host_losses[0]:.4e} -> {host_losses[-1]:.4e}, "
          f"ratio {losses[-1] / host_losses[-1]:.4f})")
    assert float(rot.mean()) <= 0.5 * float(rot0.mean()) and float(tr.mean()) <= 0.5 * float(tr0.mean())
    assert bool((rot <= 1.25 * hrot).all()) and bool((tr <= 1.25 * htr).all())
    assert losses[-1] <= 1.25 * host_losses[-1]
