"""GPU tests (-m gpu) of the scene march's gradients: pnr_baked_scene_backward_rays / _views through ops.baked_scene_backward,
BakedScene.render_diff / render_views_diff and util.bake.place.  The header ("Gradients of the scene march") states the formulas
and the guarantees; the parity cases hold d_rays, d_local and d_poses, each at its own bar, to the fp64 autograd of the restatement
tests/baked_scene_grad_ref.py (its own checks and the checks of the inputs used here: tests/test_baked_scene_grad_host.py), the
rest holds the guarantees bit for bit.

Error and bar: max|got - ref64| / max|ref64| over all rows (the rows the kept-rows rule drops carry exactly zero upstream gradients
and must come back as exact zeros), bar = 10 x torch-fp32's own error through the same restatement, floor 2e-6, cap 2e-4."""
import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_ray_grad_ref as RG
import baked_scene_grad_ref as R
import baked_scene_ref as S
import sparse_baked_ref as SP

pytestmark = pytest.mark.gpu

DEGREES = {"rgba": None, "sh2": 2}
OUTPUTS = ("d_rays", "d_local", "d_poses")


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


def _objects(objects, dev, half=False, sparse=False, poses=None):
    """baked_scene_ref.obj dicts -> the tuples ops.baked_scene_backward takes"""
    out = []
    for j, ob in enumerate(objects):
        stored = ob["stored"]
        bits = None if ob["occupied"] is None else _t(SP.bits_from_cells(ob["occupied"]).copy(), dev)
        index = None
        if sparse:
            index, ids = SP.sparse_points(ob["occupied"])
            stored, index = np.ascontiguousarray(stored.reshape((-1,) + stored.shape[3:])[ids]), _t(index, dev)
        stored = _t(stored, dev)
        pose = torch.from_numpy(np.array(ob["pose"] if poses is None else poses[j], np.float32))
        out.append((stored.half() if half else stored, ob["degree"], ob["stored"].shape[:3], ob["c1"], ob["c2"], pose, bits, index))
    return out


def _backward(ops, dev, ref, objects=None, rays=None, ups=None, **kw):
    ups = ref["ups"] if ups is None else ups
    rays = ref["rays"] if rays is None else rays
    objects = _objects(ref["objects"], dev) if objects is None else objects
    return ops.baked_scene_backward(_t(rays, dev), objects, ref["step"], d_rgb=_t(ups["d_rgb"], dev), d_depth=_t(ups["d_depth"], dev),
                                    d_alpha=_t(ups["d_alpha"], dev), **ref["kw"], **kw)


def _hold_all(what, got, ref):
    N = len(ref["objects"])
    R_ = len(ref["rays"])
    assert tuple(got[0].shape) == (R_, 8) and tuple(got[1].shape) == (R_, N, 6) and tuple(got[2].shape) == (N, 12)
    for g, g64, g32, name in zip(got, ref["ref64"], ref["ref32"], OUTPUTS):
        assert g.dtype == torch.float32
        RG.hold(f"{what} {name}", g.cpu().reshape(g64.shape), g64, g32)
    off = ~ref["held"]
    assert not bool(got[0].cpu()[off].any()) and not bool(got[1].cpu()[off].any())      # exact zeros where nothing comes from above
    assert not bool(got[0][:, 7].any())                                                 # d_far


# ---------------------------------------------------------------- 1. parity with the fp64 gradient
@pytest.mark.parametrize("setting", sorted(R.SETTINGS))
@pytest.mark.parametrize("name", ["overlap", "disjoint", "three"])
@pytest.mark.parametrize("kind", sorted(DEGREES))
def test_gradients_of_every_case_are_within_their_bars(dev, ops, kind, name, setting):
    """grids (9,8,7) and (5,6,4), 37 rays, generic poses; 150 samples plain, 150 with skip grids at threshold 10 and terminate 1e-2
    on the rows off the stop, 40 with the white background; all three upstream gradients"""
    ref = R.reference(DEGREES[kind], name, setting)
    got = _backward(ops, dev, ref)
    _hold_all(f"{kind} {name} {setting}", got, ref)
    assert bool(got[2].any(dim=1).all())                                                # every object's pose gets a gradient


# ---------------------------------------------------------------- 2. a long ray: the heads beyond chunk 63 under mixing
def test_long_ray_rebuilds_its_heads_under_mixing(dev, ops):
    ref = R.long_reference()
    _hold_all("rgba long n4500", _backward(ops, dev, ref), ref)


# ---------------------------------------------------------------- 3. (a): one object at the identity is the single ray backward
@pytest.mark.parametrize("kind", sorted(DEGREES))
def test_a_identity_pose_gives_the_single_ray_backward_bytes(dev, ops, kind):
    case = G.BY_NAME["rgba_n150" if kind == "rgba" else "sh2_n150"]
    inp, kept, ref64, ref32 = RG.reference(case)
    ups = [_t(inp[k], dev) for k in ("d_rgb", "d_depth", "d_alpha")]
    stored, rays = _t(inp["stored"], dev), _t(inp["rays"], dev)
    for kw in (dict(white_bkgd=True, terminate=1e-2), dict()):
        single = ops.baked_ray_backward(rays, stored, case.kind, G.RESO, G.C1, G.C2, inp["step"], d_rgb=ups[0], d_depth=ups[1], d_alpha=ups[2], **kw)
        d_rays, d_local, d_poses = ops.baked_scene_backward(rays, [(stored, case.kind, G.RESO, G.C1, G.C2, torch.eye(4))], inp["step"],
                                                            d_rgb=ups[0], d_depth=ups[1], d_alpha=ups[2], **kw)
        assert bool(single.any()) and torch.equal(d_rays, single), kw
        assert tuple(d_local.shape) == (37, 1, 6) and tuple(d_poses.shape) == (1, 12)
    # in its own frame the object sees the world ray: d_local is the row's first six columns, at the parity bar
    RG.hold(f"{kind} identity d_local", d_local[:, 0].cpu(), ref64[:, :6], ref32[:, :6], kept)
    only = ops.baked_scene_backward(rays, [(stored, case.kind, G.RESO, G.C1, G.C2, torch.eye(4))], inp["step"], d_rgb=ups[0], d_depth=ups[1],
                                    d_alpha=ups[2], want_poses=False, **kw)
    assert only[2] is None and torch.equal(only[0], d_rays) and torch.equal(only[1], d_local)


# ---------------------------------------------------------------- 4. (d): two objects commute
@pytest.mark.parametrize("kind", sorted(DEGREES))
def test_d_two_objects_commute(dev, ops, kind):
    ref = R.reference(DEGREES[kind], "overlap", "n150_bits10_terminate")
    objects = _objects(ref["objects"], dev)
    ab, ba = _backward(ops, dev, ref, objects=objects), _backward(ops, dev, ref, objects=objects[::-1])
    assert bool(ab[1][:, 1].any()) and bool(ab[2][1].any())
    assert torch.equal(ab[0], ba[0]) and torch.equal(ab[1], ba[1].flip(1)) and torch.equal(ab[2], ba[2].flip(0))


# ---------------------------------------------------------------- 5. written rows, exact zeros, equal bytes
@pytest.mark.parametrize("kind", sorted(DEGREES))
def test_every_row_is_written_and_zeros_are_exact(dev, ops, kind):
    from pixelnerf_amd import _lib
    ref = R.reference(DEGREES[kind], "disjoint", "n150")
    lib, objects = _lib.load(), _objects(ref["objects"], dev)
    arr, _, keep = ops._baked_scene("test", objects, ref["step"], 0.0)
    rays, Rn = _t(ref["rays"], dev), len(ref["rays"])
    ups = {k: _t(v, dev).clone() for k, v in ref["ups"].items()}
    ups["d_rgb"][5], ups["d_depth"][5], ups["d_alpha"][5] = 0.0, 0.0, 0.0              # a ray that hits, with nothing from above
    d_rays = torch.full((Rn, 8), float("nan"), device=dev)
    d_local = torch.full((Rn, 2, 6), float("nan"), device=dev)
    d_poses = torch.full((2, 12), float("nan"), device=dev)
    ws = torch.empty(lib.pnr_baked_scene_backward_workspace_bytes() // 8, dtype=torch.float64, device=dev)
    rc = lib.pnr_baked_scene_backward_rays(rays.data_ptr(), Rn, arr, 2, ref["step"], 0, 0.0, ups["d_rgb"].data_ptr(), ups["d_depth"].data_ptr(),
                                           ups["d_alpha"].data_ptr(), d_rays.data_ptr(), d_local.data_ptr(), d_poses.data_ptr(), ws.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    assert rc == 0
    assert bool(torch.isfinite(d_rays).all()) and bool(torch.isfinite(d_local).all()) and bool(torch.isfinite(d_poses).all())
    zero_rows = list(G.MISSING) + [5]                                                   # four miss every box, one has near >= far
    assert not bool(d_rays[zero_rows].any()) and not bool(d_local[zero_rows].any()) and bool(d_rays[0].any())
    # the same through ops, twice: equal bytes
    np_ups = {k: v.cpu().numpy() for k, v in ups.items()}
    first, second = _backward(ops, dev, ref, objects=objects, ups=np_ups), _backward(ops, dev, ref, objects=objects, ups=np_ups)
    for a, b, c in zip(first, second, (d_rays, d_local, d_poses)):
        assert torch.equal(a, b) and torch.equal(a, c)
    # upstream only on rays that miss B: its pose gets 12 exact zeros, its rows of d_local zeros
    misses_b = (~ref["met"][:, 1]).numpy()
    assert 4 <= int((misses_b & ref["held"].numpy() & ref["met"][:, 0].numpy()).sum())
    masked = {k: v * (misses_b[:, None] if v.ndim == 2 else misses_b).astype(np.float32) for k, v in ref["ups"].items()}
    got = _backward(ops, dev, ref, objects=objects, ups=masked)
    assert not bool(got[2][1].any()) and not bool(got[1][:, 1].any()) and bool(got[2][0].any()) and bool(got[1][:, 0].any())
    # no rays: nothing is marched, the poses' gradient is still written, as zeros
    none = ops.baked_scene_backward(torch.zeros((0, 8), device=dev), objects, ref["step"])
    assert tuple(none[0].shape) == (0, 8) and tuple(none[1].shape) == (0, 2, 6) and tuple(none[2].shape) == (2, 12) and not bool(none[2].any())


# ---------------------------------------------------------------- 6. layout and storage: the same bytes
@pytest.mark.parametrize("kind", sorted(DEGREES))
def test_sparse_rows_and_half_volumes_give_the_dense_fp32_bytes(dev, ops, kind):
    ref = R.reference(DEGREES[kind], "overlap", "n150_bits10_terminate")
    dense = _backward(ops, dev, ref)
    assert all(bool(g.any()) for g in dense)
    sparse = _backward(ops, dev, ref, objects=_objects(ref["objects"], dev, sparse=True))
    assert all(torch.equal(a, b) for a, b in zip(sparse, dense))
    # fp16 -> fp32 is exact: a half volume gives the bytes of the call on its widened values
    for layout in (False, True):
        half = _objects(ref["objects"], dev, half=True, sparse=layout)
        widened = [(ob[0].float(),) + ob[1:] for ob in half]
        assert half[0][0].dtype == torch.float16 and not torch.equal(widened[0][0], _objects(ref["objects"], dev, sparse=layout)[0][0])
        a, b = _backward(ops, dev, ref, objects=half), _backward(ops, dev, ref, objects=widened)
        assert all(bool(g.any()) for g in a) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 7. the views entry
def _views_inputs(degree, dev):
    from testdata import synthetic
    v = RG.VIEWS
    poses = torch.stack([synthetic.pose_spherical(*a) for a in RG.VIEW_ANGLES]).float()
    objects = R.cases(degree)["overlap"]
    rs = np.random.RandomState(99)
    n = poses.shape[0] * v["H"] * v["W"]
    ups = dict(d_rgb=rs.standard_normal((n, 3)).astype(np.float32), d_depth=rs.standard_normal((n,)).astype(np.float32),
               d_alpha=rs.standard_normal((n,)).astype(np.float32))
    return v, poses, objects, ups


@pytest.mark.parametrize("kind", sorted(DEGREES))
def test_views_entry_gives_the_rays_entry_bytes_and_the_camera_gradient(dev, ops, bake, kind):
    degree = DEGREES[kind]
    v, poses, objects, ups = _views_inputs(degree, dev)
    cam = (v["W"], v["H"], v["focal"], None, v["z_near"], v["z_far"])
    tuples = _objects(objects, dev)
    kw = dict(d_rgb=_t(ups["d_rgb"], dev), d_depth=_t(ups["d_depth"], dev), d_alpha=_t(ups["d_alpha"], dev), white_bkgd=True)
    rays = ops.gen_rays(poses.to(dev), v["W"], v["H"], v["focal"], v["z_near"], v["z_far"]).reshape(-1, 8)
    by_rays = ops.baked_scene_backward(rays, tuples, v["step"], **kw)
    by_views = ops.baked_scene_backward_views(poses.to(dev), *cam, tuples, v["step"], **kw)
    assert tuple(by_views[0].shape) == (2, v["H"], v["W"], 8) and bool(by_rays[0].any()) and bool(by_rays[2].any())
    assert torch.equal(by_views[0].reshape(-1, 8), by_rays[0]) and torch.equal(by_views[1], by_rays[1]) and torch.equal(by_views[2], by_rays[2])

    # through render_views_diff: the camera gradient against the restatement's, composed with gen_rays; rays off the rule get no upstream
    np_rays = rays.cpu().numpy()
    kept = R.kept_rows(np_rays, objects, v["step"]).numpy()
    assert int((~kept).sum()) <= R.MAX_DROPPED
    ups = {k: val * (kept[:, None] if val.ndim == 2 else kept).astype(np.float32) for k, val in ups.items()}

    def restated(dtype):
        leaf = R._fp32(poses.numpy(), dtype).requires_grad_(True)
        obj_leaf = R._fp32(R.stack_poses(objects), dtype).requires_grad_(True)
        r = RG.gen_rays(leaf, v["W"], v["H"], v["focal"], v["z_near"], v["z_far"]).reshape(-1, 8)
        out = R.march(r, obj_leaf, objects, v["step"], white_bkgd=True)
        RG.loss_per_ray(out, ups["d_rgb"], ups["d_depth"], ups["d_alpha"], dtype).sum().backward()
        return leaf.grad, obj_leaf.grad

    cam64, obj64 = restated(torch.float64)
    cam32, obj32 = restated(torch.float32)
    cls = bake.BakedVolume if degree is None else bake.BakedSHVolume
    scene = bake.BakedScene([cls.from_tensor(_t(o["stored"], dev), o["c1"], o["c2"]) for o in objects], torch.from_numpy(R.stack_poses(objects)))
    leaf = poses.to(dev).requires_grad_(True)
    obj_leaf = torch.from_numpy(R.stack_poses(objects)).requires_grad_(True)
    out = scene.render_views_diff(leaf, v["W"], v["H"], v["focal"], v["z_near"], v["z_far"], obj_poses=obj_leaf, step=v["step"], white_bkgd=True,
                                  skip=False)
    plain = scene.render_views(poses.to(dev), v["W"], v["H"], v["focal"], v["z_near"], v["z_far"], step=v["step"], white_bkgd=True, skip=False)
    assert torch.equal(out.rgb, plain.rgb) and torch.equal(out.depth, plain.depth) and torch.equal(out.alpha, plain.alpha)
    ((out.rgb.reshape(-1, 3) * _t(ups["d_rgb"], dev)).sum() + (out.depth.reshape(-1) * _t(ups["d_depth"], dev)).sum()
     + (out.alpha.reshape(-1) * _t(ups["d_alpha"], dev)).sum()).backward()
    RG.hold(f"{kind} views d_cameras", leaf.grad.cpu(), cam64, cam32)
    RG.hold(f"{kind} views d_obj_poses", obj_leaf.grad, obj64, obj32)
    assert obj_leaf.grad.device.type == "cpu" and tuple(obj_leaf.grad.shape) == (2, 3, 4)


# ---------------------------------------------------------------- 8. the Python surface
@pytest.mark.parametrize("kind", ["rgba", "sh2", "rgba_half", "rgba_sparse"])
def test_render_diff_gives_the_bytes_of_render_and_gradients_reach_rays_and_poses(dev, ops, bake, kind, monkeypatch):
    degree = 2 if kind == "sh2" else None
    ref = R.reference(degree, "overlap", "n150")
    cls = bake.BakedVolume if degree is None else bake.BakedSHVolume
    volumes = [cls.from_tensor(_t(o["stored"], dev), o["c1"], o["c2"]) for o in ref["objects"]]
    if kind.endswith("_half"):
        volumes = [v.half() for v in volumes]
    if kind.endswith("_sparse"):
        volumes = [v.sparse() for v in volumes]
    poses = torch.from_numpy(R.stack_poses(ref["objects"]))
    scene = bake.BakedScene(volumes, poses)
    rays = _t(ref["rays"], dev)
    plain = scene.render(rays, step=ref["step"])
    same = lambda a, b: torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.alpha, b.alpha)

    calls = []
    real = ops.baked_scene_backward
    monkeypatch.setattr(ops, "baked_scene_backward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = scene.render_diff(rays, step=ref["step"])                                     # no requires_grad anywhere: no graph
    assert same(out, plain) and not out.rgb.requires_grad and float(plain.alpha.max()) > 0.5
    ray_leaf, pose_leaf = rays.clone().requires_grad_(True), poses.clone().requires_grad_(True)
    out = scene.render_diff(ray_leaf.reshape(37, 1, 8), poses=pose_leaf, step=ref["step"])
    assert tuple(out.rgb.shape) == (37, 1, 3) and torch.equal(out.rgb.reshape(37, 3), plain.rgb) and torch.equal(out.alpha.reshape(37), plain.alpha)
    assert calls == []
    ups = [_t(ref["ups"][k], dev) for k in ("d_rgb", "d_depth", "d_alpha")]
    ((out.rgb.reshape(37, 3) * ups[0]).sum() + (out.depth.reshape(37) * ups[1]).sum() + (out.alpha.reshape(37) * ups[2]).sum()).backward()
    assert calls == [1]                                                                 # one backward call for both gradients
    direct = real(rays, scene._objects(True), ref["step"], d_rgb=ups[0], d_depth=ups[1], d_alpha=ups[2])
    assert bool(ray_leaf.grad.any()) and torch.equal(ray_leaf.grad, direct[0])
    assert bool(pose_leaf.grad.any()) and torch.equal(pose_leaf.grad, direct[2].reshape(2, 3, 4).cpu())
    # only the rays ask: the pose reduction is not run; (N,4,4) poses get a (N,4,4) gradient whose last row is zero
    ray_leaf.grad = None
    scene.render_diff(ray_leaf, step=ref["step"]).rgb.sum().backward()
    assert bool(ray_leaf.grad.any())
    full = torch.cat((poses, torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(2, 1, 4)), dim=1).requires_grad_(True)
    (scene.render_diff(rays, poses=full, step=ref["step"]).rgb * ups[0]).sum().backward()
    assert tuple(full.grad.shape) == (2, 4, 4) and bool(full.grad[:, :3].any()) and not bool(full.grad[:, 3].any())
    assert same(scene.render(rays, step=ref["step"]), plain)                            # render keeps its bytes


# ---------------------------------------------------------------- 9. placing an object
@pytest.mark.parametrize("how", ["loop", "place_skip"])
def test_place_converges_as_the_host_loop_does(dev, bake, how):
    """Two 16^3 volumes (tensors, no network): object 0, baked_ray_grad_ref.REG's blobs on [-1,1]^3 at the identity, fixed; object 1,
    two blobs on [-0.6,0.6]^3 beside and partly in front of it; the three REG_CAMERAS, 12 x 12 pixels, focal 14, near 1.5, far 3.9,
    step 0.05, white background; the start 8 degrees and 0.1 off; 120 steps of Adam at lr 1e-2 on object 1 alone.  The reference is
    the same loop through the fp32 restatement on the host (baked_scene_grad_ref.place_ref; its fp64 run agrees:
    tests/test_baked_scene_grad_host.py).  Required: rotation and translation error each at most half their start; each within
    1.25 x the host loop's; the final loss within 1.25 x the host loop's; object 0's pose returned bit for bit."""
    r, p = RG.REG, R.PLACE
    first, second, true, start, cams = (_t(np.array(a), dev) for a in R.place_scene())
    volumes = [bake.BakedVolume.from_tensor(first, r["c1"], r["c2"]), bake.BakedVolume.from_tensor(second, p["c1"], p["c2"])]
    cam = (r["W"], r["H"], r["focal"], r["z_near"], r["z_far"])
    target = bake.BakedScene(volumes, true.cpu()).render_views(cams, *cam, step=r["step"], white_bkgd=True, skip=False).rgb
    scene = bake.BakedScene(volumes, start.cpu())
    if how == "loop":
        poses0 = start.cpu()
        w = torch.zeros((1, 3), requires_grad=True)
        v = torch.zeros((1, 3), requires_grad=True)
        current = lambda: torch.cat((poses0[:1], bake.moved_poses(poses0[1:], w, v)), dim=0)
        optimiser = torch.optim.Adam([w, v], lr=p["lr"])
        losses = []
        for _ in range(p["steps"]):
            out = scene.render_views_diff(cams, *cam, obj_poses=current(), step=r["step"], white_bkgd=True, skip=False)
            loss = ((out.rgb - target) ** 2).mean()
            optimiser.zero_grad(set_to_none=True)
            loss.backward()
            optimiser.step()
            losses.append(loss.detach())
        poses, losses = current().detach(), torch.stack(losses).tolist()
    else:
        placed, losses = bake.place(scene, target, cams, *cam, objects=[1], steps=p["steps"], lr=p["lr"], step=r["step"], white_bkgd=True,
                                    skip=True)
        assert placed.volumes == volumes and placed is not scene and torch.equal(scene.poses, start.cpu())
        poses = placed.poses
    assert tuple(poses.shape) == (2, 3, 4) and len(losses) == p["steps"]
    assert torch.equal(poses[0], start.cpu()[0])                                        # the fixed object: bit for bit
    host_poses, host_losses = R.place_ref(torch.float32)
    rot0, tr0 = R.place_errors(start.cpu(), true.cpu())
    rot, tr = R.place_errors(poses, true.cpu())
    hrot, htr = R.place_errors(host_poses, true.cpu())
    print(f"{how}: rotation {rot0:.2f} -> {rot:.3f} deg (host {hrot:.3f}, ratio {rot / hrot:.4f}), translation {tr0:.3f} -> {tr:.5f} "
          f"(host {htr:.5f}, ratio {tr / htr:.4f}), loss {losses[0]:.4e} -> {losses[-1]:.4e} (host {host_losses[0]:.4e} -> "
          f"{host_losses[-1]:.4e}, ratio {losses[-1] / host_losses[-1]:.4f})")
    assert rot <= 0.5 * rot0 and tr <= 0.5 * tr0
    assert rot <= 1.25 * hrot and tr <= 1.25 * htr
    assert losses[-1] <= 1.25 * host_losses[-1]
