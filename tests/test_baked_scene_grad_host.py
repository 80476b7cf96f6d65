"""Host tests (no GPU) of the scene march's gradients: the three symbols, every refusal of pnr_baked_scene_backward_rays / _views and
of ops.baked_scene_backward, BakedScene.render_diff / render_views_diff and util.bake.place that needs no device, and the
restatement tests/baked_scene_grad_ref.py checked against itself: its forward is baked_scene_ref.render_ref, its pose gradient equals
central differences of its own loss, the 12-number gradient projected through moved_poses equals autograd straight to (w, v), and
the placing loop on the host converges."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_scene_grad_ref as R
import baked_scene_ref as S
from pixelnerf_amd import _lib
from test_baked_scene_host import P, _array, _fake, _object


# ---------------------------------------------------------------- the symbols

def test_header_declares_and_binding_binds(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("pnr_baked_scene_backward_rays", 15), ("pnr_baked_scene_backward_views", 23)):
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert len(_lib.PROTOTYPES[name][1]) == nargs
    assert re.search(r"\bsize_t pnr_baked_scene_backward_workspace_bytes\s*\(\s*void\s*\)", code)
    lib = _lib.load()
    for name in ("pnr_baked_scene_backward_rays", "pnr_baked_scene_backward_views", "pnr_baked_scene_backward_workspace_bytes"):
        assert hasattr(lib, name), name
    assert lib.pnr_baked_scene_backward_workspace_bytes() == 512 * 8 * 12 * 8
    assert ctypes.sizeof(_lib.PnrBakedObject) == 128


# ---------------------------------------------------------------- refusals of the two entries, before any device work

@pytest.mark.parametrize("form", ["rays", "views"])
def test_entries_refuse_bad_arguments_before_any_device_work(form):
    lib = _lib.load()

    def call(objects=None, n=None, step=0.1, term=0.0, src=P, R=4, d_rgb=P, d_depth=P, d_alpha=P, d_rays=P, d_local=P, d_poses=None, ws=None):
        objects = _array(_object()) if objects is None else objects
        n = (len(objects) if objects is not None else 1) if n is None else n
        tail = (objects, n, step, 0, term, d_rgb, d_depth, d_alpha, d_rays, d_local, d_poses, ws, None)
        if form == "rays":
            return lib.pnr_baked_scene_backward_rays(src, R, *tail)
        return lib.pnr_baked_scene_backward_views(src, R, 4, 4, 10.0, 10.0, 2.0, 2.0, 0.5, 3.0, *tail)

    def refused(fragment, **kw):
        assert call(**kw) == -1, fragment
        msg = lib.pnr_last_error()
        assert fragment in msg and msg.startswith(b"pnr_baked_scene_backward_" + form.encode()), (fragment, msg)

    # the forward's refusals, in its order and words
    refused(b"n_objects must lie in [1, 8]", n=0)
    refused(b"n_objects must lie in [1, 8]", objects=_array(*[_object() for _ in range(9)]), n=9)
    assert call(objects=ctypes.POINTER(_lib.PnrBakedObject)(), n=1) == -1 and b"null argument (objects)" in lib.pnr_last_error()
    refused(b"object 1: reserved must be 0", objects=_array(_object(), _object(reserved=1)))
    refused(b"object 1: mixed kinds", objects=_array(_object(), _object(degree=2)))
    refused(b"object 2: mixed kinds", objects=_array(_object(), _object(), _object(half=1)))
    refused(b"object 1: mixed kinds", objects=_array(_object(), _object(index=P, bits=P, M=10)))
    for step in (0.0, -0.1, float("inf"), float("nan")):
        refused(b"step must be finite and > 0", step=step)
    for term in (-0.01, 1.0, float("nan")):
        refused(b"terminate must lie in [0, 1)", term=term)
    refused(b"null argument", src=None)
    refused(b"4-byte aligned", src=P + 1)
    refused(b"bad sizes", R=-1)
    refused(b"mixed kinds", objects=_array(_object(), _object(degree=2)), step=0.0)         # the order: kinds before step
    refused(b"step must be", step=0.0, d_rays=None)                                          # ... step before the outputs
    # d_rays / d_local in the place of rgb / depth / alpha
    refused(b"null argument", d_rays=None)
    refused(b"null argument", d_local=None)
    assert call(d_rgb=None, d_depth=None, d_alpha=None, objects=_array(_object(degree=3))) == -1    # absent upstream gradients are legal
    align = b"d_rgb, d_depth, d_alpha, d_rays, d_local and d_poses must be 4-byte aligned"
    for name in ("d_rgb", "d_depth", "d_alpha", "d_rays", "d_local"):
        refused(align, **{name: P + 2})
    refused(align, d_poses=P + 2, ws=P)
    # one more: d_poses without a workspace, or with a misaligned one
    refused(b"d_poses needs the workspace of pnr_baked_scene_backward_workspace_bytes(), 8-byte aligned", d_poses=P)
    refused(b"d_poses needs the workspace", d_poses=P, ws=P + 4)
    refused(b"d_poses needs the workspace", d_poses=P, src=None, R=0, d_rays=None, d_local=None)    # at R = 0 too: d_poses is written
    # per object, under its position, in the words of the single ray backward
    refused(b"object 0: degree must be -1 (RGBA), 0, 1 or 2", objects=_array(_object(degree=3)))
    refused(b"object 0: storage_half must be 0 or 1", objects=_array(_object(half=2)))
    refused(b"object 1: every axis needs at least 2 grid points", objects=_array(_object(), _object(n=(1, 4, 4))))
    refused(b"object 1: c1 / c2 must be finite with c1 < c2", objects=_array(_object(), _object(c1=(1, 1, 1), c2=(-1, -1, -1))))
    refused(b"object 1: null argument", objects=_array(_object(), _object(stored=None)))
    refused(b"object 1: stored must be 16-byte aligned", objects=_array(_object(), _object(stored=P + 8)))
    refused(b"object 0: bits, d_rgb, d_depth, d_alpha and d_rays must be 4-byte aligned", objects=_array(_object(bits=P + 2)))
    refused(b"object 0: bad sizes (M)", objects=_array(_object(index=P, bits=P, M=-1)))
    refused(b"object 0: null argument", objects=_array(_object(index=P, bits=None, M=10)))
    refused(b"object 0: index must be 4-byte aligned", objects=_array(_object(index=P + 2, bits=P, M=10)))
    bad = b"pose must be finite and rigid"
    eye = np.eye(4)[:3]
    for pose in (eye * 1.01, eye * np.array([[1.0], [1.0], [-1.0]]), np.where(np.arange(12).reshape(3, 4) == 3, np.nan, eye)):
        refused(b"object 1: " + bad, objects=_array(_object(), _object(pose=pose)))
    # no rays: a no-op (d_poses absent: nothing at all is launched) -- and refusals come first
    none = dict(src=None, R=0, d_rgb=None, d_depth=None, d_alpha=None, d_rays=None, d_local=None)
    assert call(objects=_array(_object(pose=R.POSE_OVERLAP), _object()), **none) == 0
    assert call(objects=_array(_object(stored=None)), **none) == 0
    assert call(objects=_array(_object(pose=eye * 2)), **none) == -1 and bad in lib.pnr_last_error()
    assert call(objects=_array(_object(reserved=3)), **none) == -1 and b"reserved" in lib.pnr_last_error()


# ---------------------------------------------------------------- refusals of ops, BakedScene and place that need no device

def test_wrappers_refuse_before_any_device_work():
    from pixelnerf_amd import autograd, ops
    from pixelnerf_amd.util import bake
    vol, rays, cams = torch.zeros(4, 5, 6, 4), torch.zeros(3, 8), torch.eye(4)[None]
    lo, hi, eye = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), torch.eye(4)
    one = (vol, None, (4, 5, 6), lo, hi, eye)
    for entry, lead in ((ops.baked_scene_backward, (rays,)), (ops.baked_scene_backward_views, (cams, 4, 4, 10.0, None, 0.5, 3.0))):
        for objects in ([], [one] * 9, None):
            with pytest.raises(ValueError, match="1 to 8"):
                entry(*lead, objects, 0.1)
        with pytest.raises(ValueError, match="object 0: pose"):
            entry(*lead, [(vol, None, (4, 5, 6), lo, hi, eye * 1.01)], 0.1)
        with pytest.raises(ValueError, match="objects 0 and 1 differ in kind"):
            entry(*lead, [one, (vol.half(), None, (4, 5, 6), lo, hi, eye)], 0.1)
        for kw in (dict(step=0.0), dict(terminate=1.0)):
            with pytest.raises(ValueError, match="object 0"):
                entry(*lead, [one], kw.get("step", 0.1), terminate=kw.get("terminate", 0.0))
        with pytest.raises(_lib.PixelNerfHipError):                    # CPU tensors: there is no CPU path
            entry(*lead, [one], 0.1)
    with pytest.raises(ValueError, match="at least one pixel"):
        ops.baked_scene_backward_views(cams, 0, 4, 10.0, None, 0.5, 3.0, [one], 0.1)
    with pytest.raises(ValueError, match="source must be"):
        autograd.baked_scene_march_autograd((rays, 4), [one[:5] + (None, None)], eye[None, :3], 0.1)
    with pytest.raises(ValueError, match=r"obj_poses must be a float tensor \(1,3,4\)"):
        autograd.baked_scene_march_autograd((rays,), [one[:5] + (None, None)], eye[None], 0.1)

    a, b = _fake(bake.BakedVolume, vol), _fake(bake.BakedVolume, torch.zeros(3, 3, 3, 4))
    scene = bake.BakedScene([a, b], torch.eye(4)[None].repeat(2, 1, 1))
    assert "render_diff" in bake.BakedScene.__doc__ and "Inference only" not in bake.BakedScene.__doc__
    with pytest.raises(ValueError, match=r"rays must be \(...,8\)"):
        scene.render_diff(torch.zeros(3, 7))
    with pytest.raises(ValueError, match="poses_c2w must be"):
        scene.render_views_diff(torch.eye(4), 4, 4, 10.0, 0.5, 3.0)
    for bad in (torch.eye(4)[None], torch.eye(3)[None].repeat(2, 1, 1), torch.eye(4)[None].repeat(2, 1, 1).long(), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match=r"object poses must be a float tensor \(2,3,4\) or \(2,4,4\)"):
            scene.render_diff(rays, poses=bad, skip=False)
        with pytest.raises(ValueError, match="object poses must be"):
            scene.render_views_diff(cams, 4, 4, 10.0, 0.5, 3.0, obj_poses=bad, skip=False)
    with pytest.raises(ValueError, match="object 1: pose is not rigid"):
        scene.render_diff(rays, poses=torch.stack([torch.eye(4), torch.eye(4) * 1.5]), skip=False)
    with pytest.raises(_lib.PixelNerfHipError):
        scene.render_diff(rays, skip=False)
    with pytest.raises(_lib.PixelNerfHipError):
        scene.render_views_diff(cams, 4, 4, 10.0, 0.5, 3.0, obj_poses=torch.eye(4)[None, :3].repeat(2, 1, 1).requires_grad_(True), skip=False)

    target = torch.zeros(1, 4, 4, 3)
    with pytest.raises(TypeError, match="expected a BakedScene"):
        bake.place(a, target, cams, 4, 4, 10.0, 0.5, 3.0)
    with pytest.raises(ValueError, match="cam_poses must be"):
        bake.place(scene, target, torch.eye(4), 4, 4, 10.0, 0.5, 3.0)
    with pytest.raises(ValueError, match="target_rgb must be"):
        bake.place(scene, torch.zeros(1, 4, 5, 3), cams, 4, 4, 10.0, 0.5, 3.0)
    with pytest.raises(ValueError, match="steps must be >= 0"):
        bake.place(scene, target, cams, 4, 4, 10.0, 0.5, 3.0, steps=-1)
    for objects in ([], [2], [0, 0], [-1]):
        with pytest.raises(ValueError, match="objects must be distinct indices"):
            bake.place(scene, target, cams, 4, 4, 10.0, 0.5, 3.0, objects=objects)
    same, losses = bake.place(scene, target, cams, 4, 4, 10.0, 0.5, 3.0, objects=[1], steps=0)   # no step: no device work
    assert losses == [] and torch.equal(same.poses, scene.poses) and same.volumes == scene.volumes


# ---------------------------------------------------------------- the restatement against itself

@pytest.mark.parametrize("degree", [None, 2], ids=["rgba", "sh2"])
def test_forward_is_the_scene_restatement(degree):
    """gap < 1e-12 relative in fp64 against baked_scene_ref.render_ref, with the skip grids, terminate and the white background"""
    objects = R.with_bits(R.cases(degree)["three"], 10.0)
    rays, step = G.case_rays("n150"), G.SETTINGS["n150"][1]
    for kw in (dict(), dict(white_bkgd=True, terminate=1e-2)):
        ref = S.render_ref(rays, objects, step, **kw)
        with torch.no_grad():
            out = R.march(R._fp32(rays, torch.float64), R._fp32(R.stack_poses(objects), torch.float64), objects, step, **kw)
        for got, want in zip(out, ref):
            assert np.abs(got.numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), kw
        assert float(np.abs(ref[2]).max()) > 0.5


@pytest.mark.parametrize("name", ["overlap", "disjoint", "three"])
def test_cases_keep_their_rays_and_meet_every_object(name):
    """the kept-rows rule with the generic poses: at most MAX_DROPPED of 37 (object A at the identity drops 3 at n40 and 1 at n150,
    the posed objects none), every object met by at least MIN_MET held rays, and upstream gradients exactly 0 off the held rows"""
    for degree in (None, 2):
        for setting, want in (("n150", 1), ("n150_bits10_terminate", 1), ("n40_white", 3)):
            ref = R.reference(degree, name, setting)
            assert int((~ref["kept"]).sum()) == want <= R.MAX_DROPPED
            assert int(ref["met"].sum(dim=0).min()) >= R.MIN_MET
            off = ~ref["held"].numpy()
            assert not ref["ups"]["d_rgb"][off].any() and not ref["ups"]["d_depth"][off].any() and not ref["ups"]["d_alpha"][off].any()
            assert all(bool(torch.isfinite(g).all()) for g in ref["ref64"] + ref["ref32"])
            for g64, g32, what in zip(ref["ref64"], ref["ref32"], ("d_rays", "d_local", "d_poses")):   # the GPU test's bar is defined
                assert R.bar_from(R.error(g32.double(), g64)) <= R.RG.BAR_CAP, (degree, setting, what)
            assert not ref["ref64"][0][off].any() and not ref["ref64"][1][off].any()
    long = R.long_reference()
    assert int(long["met"].sum(dim=0).min()) >= R.MIN_MET


@pytest.mark.parametrize("degree", [None, 2], ids=["rgba", "sh2"])
def test_pose_gradient_is_the_central_difference_of_its_own_loss(degree):
    """fp64: autograd's 12-number pose gradient against central differences of the restatement's loss on the held rays, pose step
    1e-6, relative agreement 1e-5 of the largest entry of the object's gradient.  (No ray had to be dropped beyond the rule's.)"""
    ref = R.reference(degree, "overlap", "n150")
    rays, objects, step, ups = ref["rays"], ref["objects"], ref["step"], ref["ups"]
    poses = torch.from_numpy(R.stack_poses(objects)).double()
    ray_t = R._fp32(rays, torch.float64)

    def loss(p):
        with torch.no_grad():
            return float(R.RG.loss_per_ray(R.march(ray_t, p, objects, step), ups["d_rgb"], ups["d_depth"], ups["d_alpha"], torch.float64).sum())

    want = ref["ref64"][2]
    h = 1e-6
    for j in range(len(objects)):
        scale = float(want[j].abs().max())
        assert scale > 0
        for r in range(3):
            for a in range(4):
                up, down = poses.clone(), poses.clone()
                up[j, r, a] += h
                down[j, r, a] -= h
                fd = (loss(up) - loss(down)) / (2 * h)
                assert abs(fd - float(want[j, r, a])) <= 1e-5 * scale, (j, r, a, fd, float(want[j, r, a]))


def test_tangent_projection_is_autograd_straight_to_w_and_v():
    """the 12-number gradient projected through moved_poses equals the gradient of the same loss taken straight to (w, v)"""
    ref = R.reference(None, "three", "n150")
    rays, objects, step, ups = ref["rays"], ref["objects"], ref["step"], ref["ups"]
    poses0 = torch.from_numpy(R.stack_poses(objects)).double()
    w = torch.zeros((3, 3), dtype=torch.float64, requires_grad=True)
    v = torch.zeros((3, 3), dtype=torch.float64, requires_grad=True)
    out = R.march(R._fp32(rays, torch.float64), R.moved_poses(poses0, w, v), objects, step)
    R.RG.loss_per_ray(out, ups["d_rgb"], ups["d_depth"], ups["d_alpha"], torch.float64).sum().backward()
    d_w, d_v = R.project(ref["ref64"][2], poses0)
    assert float(w.grad.abs().max()) > 0 and float(v.grad.abs().max()) > 0
    assert float((d_w - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())
    assert float((d_v - v.grad).abs().max()) <= 1e-12 * float(v.grad.abs().max())
    assert torch.equal(d_v, ref["ref64"][2][:, :, 3])                  # the translation is its own tangent
    # util.bake.moved_poses on (N,3,4) is the restated one
    from pixelnerf_amd.util import bake
    wr, vr = torch.randn(3, 3, dtype=torch.float64), torch.randn(3, 3, dtype=torch.float64)
    assert torch.equal(bake.moved_poses(poses0, wr, vr), R.moved_poses(poses0, wr, vr))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_host_place_loop_converges(dtype):
    """the placing loop through the restatement: both errors of the moved object fall to at most half their start (8 degrees and
    0.1), the loss falls, and the fixed object stays where it is"""
    _, _, true, start, _ = R.place_scene()
    rot0, shift0 = R.place_errors(torch.from_numpy(start), torch.from_numpy(true))
    assert abs(rot0 - R.PLACE["start_deg"]) < 1e-3 and abs(shift0 - R.PLACE["start_shift"]) < 1e-6
    poses, losses = R.place_ref(dtype)
    rot, shift = R.place_errors(poses, torch.from_numpy(true))
    print(f"place ({dtype}): rotation {rot0:.3f} -> {rot:.3f} degrees, translation {shift0:.4f} -> {shift:.4f}, loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert rot <= 0.5 * rot0 and shift <= 0.5 * shift0
    assert losses[-1] < 0.25 * losses[0]
    assert torch.equal(poses[0], torch.from_numpy(start[0]).to(dtype))
