"""GPU tests (-m gpu) of the scene march's gradients with respect to the STORED VALUES of its objects:
pnr_baked_scene_stored_backward_rays / _views through ops.baked_scene_stored_backward, BakedScene.trainable and util.bake.fit_scene.
The header ("Gradients of the scene march with respect to the STORED VALUES") states the formulas; the reference is the fp64
autograd of the restatement tests/baked_scene_fit_ref.py (its own checks: tests/test_baked_scene_fit_host.py).

Error and bar, PER OBJECT: max|got - ref64| / max|ref64| over the object's stored tensor, bar = 10 x torch-fp32's own error through
the same restatement, floor 2e-6, cap 2e-4.  The rows the kept-rows rule drops carry exactly zero upstream gradients and are not
walked.  Every test prints the HIP error, the torch-fp32 error and the bar before it asserts."""
import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_ray_grad_ref as RG
import baked_scene_fit_ref as F
import baked_scene_grad_ref as R
import sparse_baked_ref as SP
from test_hip_baked_scene_grad import _objects, _t

pytestmark = pytest.mark.gpu

DEGREES = {"rgba": None, "sh0": 0, "sh1": 1, "sh2": 2}


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


def _ups(ref, dev, ups=None):
    ups = ref["ups"] if ups is None else ups
    return dict(d_rgb=_t(ups["d_rgb"], dev), d_depth=_t(ups["d_depth"], dev), d_alpha=_t(ups["d_alpha"], dev))


def _backward(ops, dev, ref, objects=None, ups=None, **kw):
    objects = _objects(ref["objects"], dev) if objects is None else objects
    return ops.baked_scene_stored_backward(_t(ref["rays"], dev), objects, ref["step"], **_ups(ref, dev, ups), **ref["kw"], **kw)


def _hold_all(what, got, ref, scale=1.0):
    assert len(got) == len(ref["ref64"])
    for j, (g, g64, g32) in enumerate(zip(got, ref["ref64"], ref["ref32"])):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(g64.shape), (what, j)
        F.hold(f"{what} object {j}", g, scale * g64, scale * g32)


# ---------------------------------------------------------------- 1. parity with the fp64 gradient
@pytest.mark.parametrize("setting", sorted(R.SETTINGS))
@pytest.mark.parametrize("name", ["overlap", "disjoint", "three"])
@pytest.mark.parametrize("kind", sorted(DEGREES))
def test_gradients_of_every_case_are_within_their_bars(dev, ops, kind, name, setting):
    """grids (9,8,7) and (5,6,4), 37 rays, generic poses; 150 samples plain, 150 with skip grids at threshold 10 and terminate 1e-2
    on the rows off the stop, 40 with the white background; all three upstream gradients"""
    ref = F.reference(DEGREES[kind], name, setting)
    got = _backward(ops, dev, ref)
    _hold_all(f"{kind} {name} {setting}", got, ref)
    if kind == "rgba":                                                  # what the reference leaves at exactly 0 stays there
        for g, g64 in zip(got, ref["ref64"]):
            assert bool((g64 == 0).any()) and not bool(g.cpu()[g64 == 0].any())


# ---------------------------------------------------------------- 2. a long ray: the heads beyond chunk 63 under mixing
def test_long_ray_rebuilds_its_heads_under_mixing(dev, ops):
    ref = F.long_reference()
    _hold_all("rgba long n4500", _backward(ops, dev, ref), ref)


# ---------------------------------------------------------------- 3. one object at the identity is the single stored backward
@pytest.mark.parametrize("kind", sorted(DEGREES))
def test_identity_pose_agrees_with_the_single_stored_backward(dev, ops, kind):
    """object A with its skip grid at threshold 10 (no contributing sample blends a sigma of exactly 0: baked_scene_fit_ref.
    identity_reference): within the bar of the reference, and within the same bar of ops.baked_render_backward"""
    degree = DEGREES[kind]
    ref = F.identity_reference(degree)
    objects = _objects(ref["objects"], dev)
    (got,) = _backward(ops, dev, ref, objects=objects)
    bar = F.hold(f"{kind} identity", got, ref["ref64"][0], ref["ref32"][0])
    stored, bits = objects[0][0], objects[0][6]
    single = ops.baked_render_backward(_t(ref["rays"], dev), stored, degree, G.RESO, G.C1, G.C2, ref["step"], bits=bits, **_ups(ref, dev),
                                       **ref["kw"])
    gap = F.error(got.cpu(), single.cpu().double())
    print(f"{kind} identity: gap to ops.baked_render_backward {gap:.3e}, bar {bar:.3e}")
    assert bool(single.any()) and gap <= bar
    assert F.error(single.cpu(), ref["single64"]) <= bar


# ---------------------------------------------------------------- 4. the listing order
@pytest.mark.parametrize("kind", ["rgba", "sh2"])
def test_swapped_listing_swaps_the_gradients(dev, ops, kind):
    ref = F.reference(DEGREES[kind], "overlap", "n150_bits10_terminate")
    objects = _objects(ref["objects"], dev)
    ab, ba = _backward(ops, dev, ref, objects=objects), _backward(ops, dev, ref, objects=objects[::-1])
    for j in (0, 1):
        bar = F.hold(f"{kind} swapped object {j}", ba[1 - j], ref["ref64"][j], ref["ref32"][j])
        assert F.error(ba[1 - j].cpu(), ab[j].cpu().double()) <= bar


# ---------------------------------------------------------------- 5. a frozen object
@pytest.mark.parametrize("kind", ["rgba", "sh2"])
def test_frozen_object_mixes_and_receives_nothing(dev, ops, kind):
    ref = F.reference(DEGREES[kind], "overlap", "n150")
    full = _backward(ops, dev, ref)
    got = _backward(ops, dev, ref, want=[True, False])
    assert got[1] is None and len(got) == 2
    bar = F.hold(f"{kind} frozen: object 0", got[0], ref["ref64"][0], ref["ref32"][0])
    assert F.error(got[0].cpu(), full[0].cpu().double()) <= bar
    other = _backward(ops, dev, ref, want=[False, True])
    assert other[0] is None
    F.hold(f"{kind} frozen: object 1", other[1], ref["ref64"][1], ref["ref32"][1])
    # alone in the scene object 0 gets ANOTHER gradient: the frozen one attenuates and mixes
    alone = ops.baked_scene_stored_backward(_t(ref["rays"], dev), _objects(ref["objects"], dev)[:1], ref["step"], **_ups(ref, dev), **ref["kw"])
    assert F.error(alone[0].cpu(), ref["ref64"][0]) > 10 * bar
    assert _backward(ops, dev, ref, want=[False, False]) == [None, None]


# ---------------------------------------------------------------- 6. accumulation
def test_second_call_accumulates_into_the_same_buffers(dev, ops):
    ref = F.reference(None, "three", "n150")
    first = _backward(ops, dev, ref)
    again = _backward(ops, dev, ref, out=first)
    assert all(a is b for a, b in zip(first, again))
    _hold_all("rgba three, twice", again, ref, scale=2.0)
    partly = _backward(ops, dev, ref, out=[None, first[1], None])
    assert partly[1] is first[1] and partly[0] is not first[0]
    F.hold("rgba three, object 1 three times", first[1], 3.0 * ref["ref64"][1], 3.0 * ref["ref32"][1])
    with pytest.raises(ValueError, match=r"out\[0\] must be a contiguous float32 tensor of shape"):
        _backward(ops, dev, ref, out=[first[1], None, None])
    with pytest.raises(ValueError, match="one buffer"):
        _backward(ops, dev, ref, out=first[:2])
    with pytest.raises(ValueError, match="one bool per object"):
        _backward(ops, dev, ref, want=[True])


# ---------------------------------------------------------------- 7. exact zeros
@pytest.mark.parametrize("kind", ["rgba", "sh2"])
def test_nothing_from_above_gives_exact_zeros(dev, ops, kind):
    ref = F.reference(DEGREES[kind], "disjoint", "n150")
    shapes = [tuple(ob["stored"].shape) for ob in ref["objects"]]
    rs = np.random.RandomState(3)
    Rn = len(ref["rays"])
    everywhere = dict(d_rgb=rs.standard_normal((Rn, 3)).astype(np.float32), d_depth=rs.standard_normal((Rn,)).astype(np.float32),
                      d_alpha=rs.standard_normal((Rn,)).astype(np.float32))
    missing = np.zeros((Rn,), np.float32)
    missing[list(G.MISSING)] = 1.0                                      # four rays miss every box, one has near >= far
    only_missing = {k: v * (missing[:, None] if v.ndim == 2 else missing) for k, v in everywhere.items()}
    zero = {k: np.zeros_like(v) for k, v in everywhere.items()}
    nothing = dict(d_rgb=None, d_depth=None, d_alpha=None)
    for what, ups in (("missing rows", only_missing), ("zero upstream", zero), ("no upstream", nothing)):
        got = _backward(ops, dev, ref, ups=ups)
        assert [tuple(g.shape) for g in got] == shapes and not any(bool(g.any()) for g in got), what
    assert all(bool(g.any()) for g in _backward(ops, dev, ref))         # (the case itself reaches both objects)
    none = ops.baked_scene_stored_backward(torch.zeros((0, 8), device=dev), _objects(ref["objects"], dev), ref["step"])
    assert [tuple(g.shape) for g in none] == shapes and not any(bool(g.any()) for g in none)


# ---------------------------------------------------------------- 8. sparse rows
@pytest.mark.parametrize("kind", ["rgba", "sh2"])
def test_sparse_rows_get_the_dense_gradient_at_their_kept_points(dev, ops, kind):
    """skip grids at threshold 10, terminate 1e-2: every object's kept rows against the dense reference at the kept points"""
    ref = F.reference(DEGREES[kind], "overlap", "n150_bits10_terminate")
    got = _backward(ops, dev, ref, objects=_objects(ref["objects"], dev, sparse=True))
    for j, (g, ob) in enumerate(zip(got, ref["objects"])):
        _, ids = SP.sparse_points(ob["occupied"])
        rows = lambda dense: dense.reshape((-1,) + tuple(dense.shape[3:]))[torch.as_tensor(np.asarray(ids)).long()]
        assert tuple(g.shape) == tuple(rows(ref["ref64"][j]).shape)
        F.hold(f"{kind} sparse object {j}", g, rows(ref["ref64"][j]), rows(ref["ref32"][j]))
        dropped = torch.ones(ref["ref64"][j].shape[:3], dtype=torch.bool).flatten()
        dropped[torch.as_tensor(np.asarray(ids)).long()] = False
        assert not bool(ref["ref64"][j].reshape((-1,) + tuple(g.shape[1:]))[dropped].any())     # the dense gradient lives on the kept points


# ---------------------------------------------------------------- 9. the views entry
@pytest.mark.parametrize("kind", ["rgba", "sh2"])
def test_views_entry_against_the_restatement_on_the_same_cameras(dev, ops, kind):
    from testdata import synthetic
    degree, v = DEGREES[kind], RG.VIEWS
    poses = torch.stack([synthetic.pose_spherical(*a) for a in RG.VIEW_ANGLES]).float()
    objects = R.cases(degree)["overlap"]
    rays = ops.gen_rays(poses.to(dev), v["W"], v["H"], v["focal"], v["z_near"], v["z_far"]).reshape(-1, 8)
    np_rays = rays.cpu().numpy()
    kept = R.kept_rows(np_rays, objects, v["step"]).numpy()
    assert int((~kept).sum()) <= R.MAX_DROPPED
    rs = np.random.RandomState(99)
    n = len(np_rays)
    ups = dict(d_rgb=rs.standard_normal((n, 3)).astype(np.float32), d_depth=rs.standard_normal((n,)).astype(np.float32),
               d_alpha=rs.standard_normal((n,)).astype(np.float32))
    ups = {k: val * (kept[:, None] if val.ndim == 2 else kept).astype(np.float32) for k, val in ups.items()}
    ref64 = F.gradients(np_rays, objects, v["step"], dtype=torch.float64, white_bkgd=True, **ups)
    ref32 = F.gradients(np_rays, objects, v["step"], dtype=torch.float32, white_bkgd=True, **ups)
    tuples = _objects(objects, dev)
    kw = dict(d_rgb=_t(ups["d_rgb"], dev), d_depth=_t(ups["d_depth"], dev), d_alpha=_t(ups["d_alpha"], dev), white_bkgd=True)
    by_views = ops.baked_scene_stored_backward_views(poses.to(dev), v["W"], v["H"], v["focal"], None, v["z_near"], v["z_far"], tuples, v["step"], **kw)
    by_rays = ops.baked_scene_stored_backward(rays, tuples, v["step"], **kw)
    for j in range(2):
        assert bool(ref64[j].any())
        bar = F.hold(f"{kind} views object {j}", by_views[j], ref64[j], ref32[j])
        assert F.error(by_views[j].cpu(), by_rays[j].cpu().double()) <= bar


# ---------------------------------------------------------------- 10. a volume listed twice
@pytest.mark.parametrize("kind", ["rgba", "sh2"])
def test_a_volume_listed_twice_gets_one_buffer_with_the_sum(dev, ops, kind):
    degree = DEGREES[kind]
    base = F.reference(degree, "overlap", "n150")
    a = base["objects"][0]
    objects = [a, dict(a, pose=R.POSE_OVERLAP)]                          # the SAME stored array at two poses
    kept = R.kept_rows(base["rays"], objects, base["step"]).numpy()
    assert int((~kept).sum()) <= R.MAX_DROPPED
    ups = {k: val * (kept[:, None] if val.ndim == 2 else kept).astype(np.float32) for k, val in base["ups"].items()}
    args = (base["rays"], objects, base["step"])
    ref64 = F.gradients(*args, dtype=torch.float64, share=True, **ups, **base["kw"])
    ref32 = F.gradients(*args, dtype=torch.float32, share=True, **ups, **base["kw"])
    tuples = _objects(objects, dev)
    tuples[1] = (tuples[0][0],) + tuples[1][1:]                          # one tensor, listed twice
    got = ops.baked_scene_stored_backward(_t(base["rays"], dev), tuples, base["step"], **_ups(base, dev, ups), **base["kw"])
    assert got[0] is got[1]
    F.hold(f"{kind} listed twice", got[0], ref64[0], ref32[0])
    # as two tensors with equal values: one buffer each, and their sum is the shared one's gradient
    apart = ops.baked_scene_stored_backward(_t(base["rays"], dev), _objects(objects, dev), base["step"], **_ups(base, dev, ups), **base["kw"])
    assert apart[0] is not apart[1] and not torch.equal(apart[0], apart[1])
    F.hold(f"{kind} listed twice, apart", apart[0] + apart[1], ref64[0], ref32[0])


# ---------------------------------------------------------------- 11. autograd and TrainableScene
@pytest.mark.parametrize("kind", ["rgba", "sh2", "rgba_sparse"])
def test_trainable_scene_renders_the_bytes_and_fills_the_gradients(dev, ops, bake, kind, monkeypatch):
    degree = 2 if kind == "sh2" else None
    sparse = kind.endswith("_sparse")
    ref = F.reference(degree, "overlap", "n150_bits10_terminate" if sparse else "n150")
    cls = bake.BakedVolume if degree is None else bake.BakedSHVolume
    volumes = [cls.from_tensor(_t(o["stored"], dev), o["c1"], o["c2"], skip_threshold=10.0 if sparse else 0.0) for o in ref["objects"]]
    if sparse:
        volumes = [v.sparse() for v in volumes]
    poses = torch.from_numpy(R.stack_poses(ref["objects"]))
    scene = bake.BakedScene(volumes, poses)
    rays = _t(ref["rays"], dev)
    kw = dict(step=ref["step"], white_bkgd=ref["kw"]["white_bkgd"], terminate=ref["kw"]["terminate"], skip=sparse)
    plain = scene.render(rays, **kw)
    same = lambda a, b: torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.alpha, b.alpha)

    calls = []
    real_stored, real_rays = ops.baked_scene_stored_backward, ops.baked_scene_backward
    monkeypatch.setattr(ops, "baked_scene_stored_backward", lambda *a, **k: (calls.append("stored"), real_stored(*a, **k))[1])
    monkeypatch.setattr(ops, "baked_scene_backward", lambda *a, **k: (calls.append("rays"), real_rays(*a, **k))[1])
    module = scene.trainable()
    assert len(module.stored) == 2 and all(p.requires_grad for p in module.stored)
    before = [v._stored().clone() for v in volumes]
    out = module(rays.reshape(37, 1, 8), **kw)
    assert tuple(out.rgb.shape) == (37, 1, 3) and out.rgb.requires_grad and float(plain.alpha.max()) > 0.5
    assert torch.equal(out.rgb.reshape(37, 3), plain.rgb) and torch.equal(out.depth.reshape(37), plain.depth) and torch.equal(out.alpha.reshape(37), plain.alpha)
    ups = _ups(ref, dev)
    loss = lambda o: ((o.rgb.reshape(37, 3) * ups["d_rgb"]).sum() + (o.depth.reshape(37) * ups["d_depth"]).sum()
                      + (o.alpha.reshape(37) * ups["d_alpha"]).sum())
    loss(out).backward()
    assert calls == ["stored"]                                          # the stored values alone ask: one call
    for j, (p, v) in enumerate(zip(module.stored, volumes)):
        want64, want32 = ref["ref64"][j], ref["ref32"][j]
        if sparse:
            ids = v.ids.cpu().long()
            want64, want32 = (g.reshape((-1,) + tuple(g.shape[3:]))[ids] for g in (want64, want32))
        F.hold(f"{kind} TrainableScene object {j}", p.grad, want64, want32)
    assert all(torch.equal(v._stored(), b) for v, b in zip(volumes, before))        # the scene's own volumes are not touched

    # the object poses ask too: the existing pose gradient, byte for byte (that path has no atomics), next to the stored one
    del calls[:]
    for p in module.stored:
        p.grad = None
    pose_leaf = poses.clone().requires_grad_(True)
    loss(module(rays, poses=pose_leaf, **kw)).backward()
    assert sorted(calls) == ["rays", "stored"]
    direct = real_rays(rays, scene._objects(sparse), ref["step"], **ups, white_bkgd=kw["white_bkgd"], terminate=kw["terminate"])
    assert bool(pose_leaf.grad.any()) and torch.equal(pose_leaf.grad, direct[2].reshape(2, 3, 4).cpu())
    assert all(p.grad is not None and bool(p.grad.any()) for p in module.stored)

    # a frozen object has no parameter, and the other's gradient is the full call's
    del calls[:]
    only = scene.trainable([1])
    assert len(only.stored) == 1 and len(list(only.parameters())) == 1
    loss(only(rays, **kw)).backward()
    want64, want32 = ref["ref64"][1], ref["ref32"][1]
    if sparse:
        ids = volumes[1].ids.cpu().long()
        want64, want32 = (g.reshape((-1,) + tuple(g.shape[3:]))[ids] for g in (want64, want32))
    F.hold(f"{kind} TrainableScene, object 0 frozen", only.stored[0].grad, want64, want32)
    assert calls == ["stored"]

    # forward_views: the bytes of render_views, and a gradient
    from testdata import synthetic
    cams = torch.stack([synthetic.pose_spherical(*a) for a in RG.VIEW_ANGLES]).float().to(dev)
    v = RG.VIEWS
    cam = (v["W"], v["H"], v["focal"], v["z_near"], v["z_far"])
    views = module.forward_views(cams, *cam, step=v["step"], white_bkgd=True, skip=sparse)
    plain_views = scene.render_views(cams, *cam, step=v["step"], white_bkgd=True, skip=sparse)
    assert torch.equal(views.rgb, plain_views.rgb) and torch.equal(views.depth, plain_views.depth) and torch.equal(views.alpha, plain_views.alpha)
    for p in module.stored:
        p.grad = None
    views.rgb.sum().backward()
    assert all(bool(p.grad.any()) for p in module.stored)

    # scene(): fresh volumes of the current values, the poses kept; tv: a scalar with a gradient
    fitted = module.scene()
    assert len(fitted) == 2 and torch.equal(fitted.poses, scene.poses) and all(a is not b for a, b in zip(fitted.volumes, volumes))
    assert all(torch.equal(a._stored(), b._stored()) for a, b in zip(fitted.volumes, volumes))
    assert only.scene().volumes[0] is volumes[0]
    tv = module.tv()
    single = sum(v.tv() for v in volumes)
    assert tv.dim() == 0 and tv.requires_grad and abs(float(tv.detach()) - single) <= 1e-6 * abs(single)
    assert same(scene.render(rays, **kw), plain)


def test_trainable_scene_gives_a_volume_listed_twice_one_parameter(dev, ops, bake):
    base = F.reference(None, "overlap", "n150")
    a = base["objects"][0]
    volume = bake.BakedVolume.from_tensor(_t(a["stored"], dev), a["c1"], a["c2"])
    poses = torch.from_numpy(np.stack((R.IDENTITY, R.POSE_OVERLAP)))
    module = bake.BakedScene([volume, volume], poses).trainable()
    assert len(module.stored) == 1 and module.slots == [0, 0]
    rays = _t(base["rays"], dev)
    ups = _ups(base, dev)
    out = module(rays, step=base["step"])
    ((out.rgb * ups["d_rgb"]).sum() + (out.depth * ups["d_depth"]).sum() + (out.alpha * ups["d_alpha"]).sum()).backward()
    tuples = _objects([a, dict(a, pose=R.POSE_OVERLAP)], dev)
    apart = ops.baked_scene_stored_backward(rays, tuples, base["step"], **ups)
    scale = float((apart[0] + apart[1]).abs().max())
    assert scale > 0 and float((module.stored[0].grad - (apart[0] + apart[1])).abs().max()) <= 1e-5 * scale   # (the atomics' order alone)


# ---------------------------------------------------------------- 12. fit_scene
def test_fit_scene_lowers_the_loss_as_the_host_loop_does(dev, bake):
    """util.bake.fit_scene on two 12^3 RGBA objects -- baked_grad_ref.fit_scene's blob at the identity, and the same blob with its
    colours rolled and its grid mirrored at baked_scene_grad_ref.POSE_OVERLAP's rotation with 0.6 of its translation --, 512 rays, the
    target rendered from the known pair, the start the perturbed pair, 40 steps of Adam (lr 2e-2) on batches of 128: the final batch
    loss is below the first, the fitted volumes are projected, the input scene is untouched, and the final loss is within a margin
    of the final loss of the same loop through the fp32 restatement on the CPU (baked_scene_fit_ref.fit_ref).  The margin is 10 x
    the spread between the fp32 and the fp64 restatement runs (the factor of the gradient bar).  The fp32 run depends on the host
    -- torch orders its fp32 reductions by the threads it has --, so the spread was measured on two hosts and the larger one is taken:
        final loss fp64 4.0158327866555e-05 on both; fp32 4.015828744741157e-05 and 4.015826925751753e-05 (the GPU machine's
        host): spread 4.04e-11 and 5.86e-11, margin 5.8e-10
    (the first loss is 9.926e-04: the final one is 4 % of it).  Measured on the MI355X: |difference| to the host loop 0.0e+00."""
    margin = 5.8e-10
    known, start, rays = (_t(np.array(a), dev) for a in F.fit_scene())
    poses = torch.from_numpy(F.FIT_POSES)
    pair = lambda stored: bake.BakedScene([bake.BakedVolume.from_tensor(stored[j].contiguous(), G.FIT_C1, G.FIT_C2) for j in range(2)], poses)
    target = pair(known).render(rays, step=G.FIT_STEP, skip=False).rgb
    scene = pair(start)
    fitted, losses = bake.fit_scene(scene, rays, target, step=G.FIT_STEP, **F.FIT)
    host = F.fit_ref(torch.float32, **F.FIT)
    host64 = F.fit_ref(torch.float64, **F.FIT)
    print(f"fit_scene: first {losses[0]:.6e} (host {host[0]:.6e}), final {losses[-1]!r} (host fp32 {host[-1]!r}, fp64 {host64[-1]!r}, "
          f"spread {abs(host[-1] - host64[-1]):.3e}), |difference| {abs(losses[-1] - host[-1]):.3e}, margin {margin:.1e}")
    assert len(losses) == F.FIT["steps"] and isinstance(fitted, bake.BakedScene) and fitted is not scene
    assert all(torch.equal(v.vol, start[j]) for j, v in enumerate(scene.volumes)) and torch.equal(fitted.poses, scene.poses)
    assert all(a is not b and not torch.equal(a.vol, b.vol) for a, b in zip(fitted.volumes, scene.volumes))
    assert losses[-1] < losses[0]
    assert abs(losses[-1] - host[-1]) <= margin
    for v in fitted.volumes:
        assert float(v.vol[..., :3].min()) >= 0.0 and float(v.vol[..., :3].max()) <= 1.0 and float(v.vol[..., 3].min()) >= 0.0
    # one object fitted in the presence of the other: the frozen one comes back as it was
    partly, _ = bake.fit_scene(scene, rays, target, objects=[1], steps=2, lr=2e-2, batch=128, seed=3, step=G.FIT_STEP)
    assert partly.volumes[0] is scene.volumes[0] and not torch.equal(partly.volumes[1].vol, start[1])
