"""Host tests (no GPU) of the scene march's stored-value gradients: the two symbols pnr_baked_scene_stored_backward_rays / _views,
their refusals with stand-in pointers (every one comes before any device work), the Python refusals that need no device, and the
restatement tests/baked_scene_fit_ref.py against its anchors: baked_scene_grad_ref.march (the forward, torch.equal),
baked_grad_ref.gradient (one object at the identity), central differences in fp64, and the sum rule of a volume listed twice."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_scene_fit_ref as F
import baked_scene_grad_ref as R
import baked_scene_ref as S
from pixelnerf_amd import _lib
from test_baked_scene_host import P, _array, _fake, _object

ENTRIES = (("pnr_baked_scene_stored_backward_rays", 12), ("pnr_baked_scene_stored_backward_views", 20))


@pytest.fixture(autouse=True, scope="module")
def _the_entries_are_bound():
    """everything here, the restatement's own anchors included, is the yardstick of the two entries: without them it says nothing"""
    assert all(name in _lib.PROTOTYPES for name, _ in ENTRIES), "the scene's stored backward is not bound"


# ---------------------------------------------------------------- the symbols

def test_header_declares_and_binding_binds(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name, nargs in ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert len(_lib.PROTOTYPES[name][1]) == nargs and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.PnrBakedObject) == 128                   # the gradient buffers travel as a separate argument
    assert "get no gradient" not in src and "are not differentiated)" not in src


# ---------------------------------------------------------------- refusals of the two entries, before any device work

def _ptrs(*values):
    return (ctypes.c_void_p * len(values))(*values)


@pytest.mark.parametrize("form", ["rays", "views"])
def test_entries_refuse_bad_arguments_before_any_device_work(form):
    lib = _lib.load()
    default = object()

    def call(objects=None, n=None, step=0.1, term=0.0, src=P, R=4, d_rgb=P, d_depth=P, d_alpha=P, d_stored=default):
        objects = _array(_object()) if objects is None else objects
        n = (len(objects) if objects is not None else 1) if n is None else n
        if d_stored is default:
            d_stored = _ptrs(*([P] * max(n, 1)))
        tail = (objects, n, step, 0, term, d_rgb, d_depth, d_alpha, d_stored, None)
        if form == "rays":
            return lib.pnr_baked_scene_stored_backward_rays(src, R, *tail)
        return lib.pnr_baked_scene_stored_backward_views(src, R, 4, 4, 10.0, 10.0, 2.0, 2.0, 0.5, 3.0, *tail)

    def refused(fragment, **kw):
        assert call(**kw) == -1, fragment
        msg = lib.pnr_last_error()
        assert fragment in msg and msg.startswith(b"pnr_baked_scene_stored_backward_" + form.encode()), (fragment, msg)

    # the scene entries' refusals, in their order and words
    refused(b"n_objects must lie in [1, 8]", n=0)
    refused(b"n_objects must lie in [1, 8]", objects=_array(*[_object() for _ in range(9)]), n=9)
    assert call(objects=ctypes.POINTER(_lib.PnrBakedObject)(), n=1) == -1 and b"null argument (objects)" in lib.pnr_last_error()
    refused(b"object 1: reserved must be 0", objects=_array(_object(), _object(reserved=1)))
    refused(b"object 1: mixed kinds", objects=_array(_object(), _object(degree=2)))
    refused(b"object 1: mixed kinds", objects=_array(_object(), _object(half=1)))
    refused(b"object 1: mixed kinds", objects=_array(_object(), _object(index=P, bits=P, M=10)))
    # half storage: the fit's words, after the kinds and before everything else
    fp32_only = b"gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards"
    refused(fp32_only, objects=_array(_object(half=1), _object(half=1)))
    refused(fp32_only, objects=_array(_object(half=1)), step=0.0, d_stored=None)
    refused(fp32_only, objects=_array(_object(half=2)))
    refused(b"mixed kinds", objects=_array(_object(half=1), _object()))
    for step in (0.0, -0.1, float("inf"), float("nan")):
        refused(b"step must be finite and > 0", step=step)
    for term in (-0.01, 1.0, float("nan")):
        refused(b"terminate must lie in [0, 1)", term=term)
    refused(b"null argument", src=None)
    refused(b"4-byte aligned", src=P + 1)
    refused(b"bad sizes", R=-1)
    refused(b"step must be", step=0.0, d_stored=None)                                        # step before the outputs
    # the new ones: a null array with rays to march, a misaligned entry
    refused(b"null argument (d_stored)", d_stored=None)
    align = b"d_rgb, d_depth, d_alpha and every d_stored[j] must be 4-byte aligned"
    for name in ("d_rgb", "d_depth", "d_alpha"):
        refused(align, **{name: P + 2})
    refused(align, d_stored=_ptrs(P + 2))
    refused(align, objects=_array(_object(), _object()), d_stored=_ptrs(None, P + 1))
    assert call(d_rgb=None, d_depth=None, d_alpha=None, objects=_array(_object(degree=3))) == -1     # absent upstream gradients are legal
    # per object, under its position, in the words of the single stored backward
    refused(b"object 0: degree must be -1 (RGBA), 0, 1 or 2", objects=_array(_object(degree=3)))
    refused(b"object 1: every axis needs at least 2 grid points", objects=_array(_object(), _object(n=(1, 4, 4))))
    refused(b"object 1: null argument", objects=_array(_object(), _object(stored=None)))
    refused(b"object 1: stored must be 16-byte aligned", objects=_array(_object(), _object(stored=P + 8)))
    refused(b"object 0: bits, d_rgb, d_depth, d_alpha and d_stored must be 4-byte aligned", objects=_array(_object(bits=P + 2)))
    refused(b"object 0: null argument", objects=_array(_object(index=P, bits=None, M=10)))
    refused(b"object 1: pose must be finite and rigid", objects=_array(_object(), _object(pose=np.eye(4)[:3] * 1.01)))
    # a frozen object is checked like any other
    refused(b"object 0: stored must be 16-byte aligned", objects=_array(_object(stored=P + 8)), d_stored=_ptrs(None))
    # no rays: a no-op, d_stored may be NULL or all NULL -- and refusals come first
    none = dict(src=None, R=0, d_rgb=None, d_depth=None, d_alpha=None)
    assert call(objects=_array(_object(pose=R.POSE_OVERLAP), _object()), d_stored=None, **none) == 0
    assert call(objects=_array(_object(), _object()), d_stored=_ptrs(None, None), **none) == 0
    assert call(objects=_array(_object()), d_stored=_ptrs(P + 2), **none) == -1 and align in lib.pnr_last_error()
    assert call(objects=_array(_object(half=1)), d_stored=None, **none) == -1 and fp32_only in lib.pnr_last_error()
    assert call(objects=_array(_object(reserved=3)), d_stored=None, **none) == -1 and b"reserved" in lib.pnr_last_error()


# ---------------------------------------------------------------- refusals of ops, autograd, BakedScene and fit_scene that need no device

def test_wrappers_refuse_before_any_device_work():
    from pixelnerf_amd import autograd, ops
    from pixelnerf_amd.util import bake
    vol, rays, cams = torch.zeros(4, 5, 6, 4), torch.zeros(3, 8), torch.eye(4)[None]
    lo, hi, eye = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), torch.eye(4)
    one = (vol, None, (4, 5, 6), lo, hi, eye)
    for entry, lead in ((ops.baked_scene_stored_backward, (rays,)), (ops.baked_scene_stored_backward_views, (cams, 4, 4, 10.0, None, 0.5, 3.0))):
        for objects in ([], [one] * 9, None):
            with pytest.raises(ValueError, match="1 to 8"):
                entry(*lead, objects, 0.1)
        with pytest.raises(TypeError, match=r"object 1: gradients exist for fp32 volumes only; fit the volume in fp32 and call half\(\) afterwards"):
            entry(*lead, [one, (vol.half(), None, (4, 5, 6), lo, hi, eye)], 0.1)
        with pytest.raises(ValueError, match="no gradient is given with respect to"):
            entry(lead[0].clone().requires_grad_(True), *lead[1:], [one], 0.1)
        with pytest.raises(ValueError, match="object 0: pose"):
            entry(*lead, [(vol, None, (4, 5, 6), lo, hi, eye * 1.01)], 0.1)
        with pytest.raises(_lib.PixelNerfHipError):                    # CPU tensors: there is no CPU path
            entry(*lead, [one], 0.1)
    with pytest.raises(ValueError, match="at least one pixel"):
        ops.baked_scene_stored_backward_views(cams, 0, 4, 10.0, None, 0.5, 3.0, [one], 0.1)
    meta = (None, (4, 5, 6), lo, hi, None, None)
    with pytest.raises(ValueError, match="source must be"):
        autograd.baked_scene_fit_autograd((rays, 4), [vol], [meta], eye[None, :3], 0.1)
    with pytest.raises(ValueError, match="must list the same objects"):
        autograd.baked_scene_fit_autograd((rays,), [vol, vol], [meta], eye[None, :3], 0.1)
    with pytest.raises(TypeError, match="fp32 volumes only"):
        autograd.baked_scene_fit_autograd((rays,), [vol.half()], [meta], eye[None, :3], 0.1)
    with pytest.raises(ValueError, match=r"obj_poses must be a float tensor \(1,3,4\)"):
        autograd.baked_scene_fit_autograd((rays,), [vol], [meta], eye[None], 0.1)

    a, b = _fake(bake.BakedVolume, vol), _fake(bake.BakedVolume, torch.zeros(3, 3, 3, 4))
    poses2 = torch.eye(4)[None].repeat(2, 1, 1)
    scene = bake.BakedScene([a, b], poses2)
    assert "get no gradient" not in bake.BakedScene.__doc__ and "fit_scene" in bake.BakedScene.__doc__
    halves = bake.BakedScene([_fake(bake.BakedVolume, vol.half()), _fake(bake.BakedVolume, vol.half())], poses2)
    with pytest.raises(TypeError, match=r"BakedScene.trainable: gradients exist for fp32 volumes only; fit the volume in fp32 and call half\(\)"):
        halves.trainable()
    for objects in ([], [2], [0, 0], [-1]):
        with pytest.raises(ValueError, match="objects must be distinct indices"):
            scene.trainable(objects)
    with pytest.raises(TypeError, match="expected a BakedScene"):
        bake.TrainableScene(a)

    # the module: copies of the chosen, the others referenced; a volume listed twice is one parameter
    module = scene.trainable()
    assert len(module.stored) == 2 and module.slots == [0, 1]
    assert torch.equal(module.stored[0], vol) and module.stored[0].data_ptr() != vol.data_ptr()
    only = scene.trainable([1])
    assert len(only.stored) == 1 and only.slots == [None, 0] and tuple(only.stored[0].shape) == (3, 3, 3, 4)
    assert only._tensors()[0] is vol and only._tensors()[1] is only.stored[0]
    twice = bake.BakedScene([a, b, a], torch.eye(4)[None].repeat(3, 1, 1)).trainable()
    assert len(twice.stored) == 2 and twice.slots == [0, 1, 0] and twice._tensors()[0] is twice._tensors()[2]
    assert bake.BakedScene([a, b, a], torch.eye(4)[None].repeat(3, 1, 1)).trainable([2]).slots == [0, None, 0]
    with pytest.raises(ValueError, match=r"rays must be \(...,8\)"):
        module(torch.zeros(3, 7))
    with pytest.raises(ValueError, match="poses_c2w must be"):
        module.forward_views(torch.eye(4), 4, 4, 10.0, 0.5, 3.0)
    with pytest.raises(ValueError, match="object poses must be"):
        module(rays, poses=torch.eye(4)[None])

    target = torch.zeros(3, 3)
    with pytest.raises(TypeError, match="expected a BakedScene"):
        bake.fit_scene(a, rays, target)
    with pytest.raises(ValueError, match=r"rays must be \(...,8\)"):
        bake.fit_scene(scene, torch.zeros(3, 7), target)
    for bad in (torch.zeros(3, 4), torch.zeros(2, 3), np.zeros((3, 3))):
        with pytest.raises(ValueError, match=r"target_rgb must be \(3, 3\)"):
            bake.fit_scene(scene, rays, bad)
    with pytest.raises(ValueError, match="steps must be >= 0 and batch >= 1"):
        bake.fit_scene(scene, rays, target, batch=0)
    with pytest.raises(ValueError, match="objects must be distinct indices"):
        bake.fit_scene(scene, rays, target, objects=[2])
    with pytest.raises(TypeError, match="fp32 volumes only"):
        bake.fit_scene(halves, rays, target)
    with pytest.raises(ValueError, match="no rays"):
        bake.fit_scene(scene, torch.zeros(0, 8), torch.zeros(0, 3))


# ---------------------------------------------------------------- the restatement against its anchors

def _case(degree, name="three", setting="n150_bits10_terminate"):
    ray_setting, thr, terminate, white = R.SETTINGS[setting]
    objects = R.cases(degree)[name]
    if thr is not None:
        objects = R.with_bits(objects, thr)
    return G.case_rays(ray_setting), objects, G.SETTINGS[ray_setting][1], dict(white_bkgd=white, terminate=terminate)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("degree", [None, 2], ids=["rgba", "sh2"])
def test_forward_is_the_scene_restatement_bit_for_bit(degree, dtype):
    for setting in ("n150_bits10_terminate", "n40_white"):
        rays, objects, step, kw = _case(degree, setting=setting)
        with torch.no_grad():
            args = (F._fp32(rays, dtype), F._fp32(R.stack_poses(objects), dtype))
            mine = F.march(*args, F.leaves(objects, dtype), objects, step, **kw)
            theirs = R.march(*args, objects, step, **kw)
        assert all(torch.equal(a, b) for a, b in zip(mine, theirs)) and float(mine[2].max()) > 0.5


@pytest.mark.parametrize("degree", [None, 0, 1, 2], ids=["rgba", "sh0", "sh1", "sh2"])
def test_one_object_at_the_identity_is_the_single_gradient(degree):
    ref = F.identity_reference(degree)
    gap = G.error(ref["ref64"][0], ref["single64"])
    print(f"degree {degree}: gap to baked_grad_ref.gradient {gap:.3e}")
    assert bool(ref["single64"].any()) and gap < 1e-12
    if degree is None:   # and with a skip grid and terminate, on the single backward's own case
        case = G.BY_NAME["rgba_n150_bits10_terminate"]
        inp, ref64, _ = G.reference(case)
        ups = {k: inp[k] for k in ("d_rgb", "d_depth", "d_alpha")}
        (got,) = F.gradients(inp["rays"], [S.obj(inp["stored"], occupied=inp["occupied"])], inp["step"], white_bkgd=case.white,
                             terminate=case.terminate, **ups)
        assert bool(ref64.any()) and G.error(got, ref64) < 1e-12


def test_where_the_mixture_has_no_density_its_colour_is_the_constant_zero():
    """the convention of the mixing, seen from the stored values: baked_grad_ref.sh_coef has points whose sigma coefficients are all
    exactly 0 -- ON the clamp's edge, where its derivative is 1 --, so samples blend a sigma of exactly 0 through an open clamp.
    There the single march's g_i keeps d_rgb . c_i and the scene's does not: the two gradients differ in the sigma channel of those
    points and nowhere else."""
    case = G.BY_NAME["sh2_n150"]
    inp, ref64, _ = G.reference(case)
    ups = {k: inp[k] for k in ("d_rgb", "d_depth", "d_alpha")}
    (got,) = F.gradients(inp["rays"], [S.obj(inp["stored"], degree=2)], inp["step"], **ups)
    differs = (got - ref64).abs() > 1e-12 * float(ref64.abs().max())
    empty = torch.from_numpy((np.asarray(inp["stored"])[..., :, 3] == 0).all(axis=-1))
    assert bool(differs.any()) and not bool(differs[..., :3].any()) and not bool(differs[~empty].any())


@pytest.mark.parametrize("degree", [None, 2], ids=["rgba", "sh2"])
@pytest.mark.parametrize("name", ["overlap", "three"])
def test_gradient_is_the_central_difference_of_its_own_loss(degree, name):
    """a handful of stored elements per object, drawn among those within a tenth of the largest gradient (the difference of two fp64 losses resolves them); h = 1e-5"""
    ref = F.reference(degree, name, "n150_bits10_terminate")
    objects, dtype = ref["objects"], torch.float64
    rays, poses = F._fp32(ref["rays"], dtype), F._fp32(R.stack_poses(objects), dtype)

    def loss(stored):
        with torch.no_grad():
            out = F.march(rays, poses, stored, objects, ref["step"], **ref["kw"])
            return float(F.RG.loss_per_ray(out, ref["ups"]["d_rgb"], ref["ups"]["d_depth"], ref["ups"]["d_alpha"], dtype).sum())

    rs = np.random.RandomState(5)
    for j, g in enumerate(ref["ref64"]):
        flat = g.flatten()
        live = torch.nonzero(flat.abs() > 0.1 * flat.abs().max()).flatten().numpy()
        for e in rs.choice(live, 4, replace=False):
            h = 1e-5
            sides = []
            for sign in (1.0, -1.0):
                stored = [F._fp32(ob["stored"], dtype) for ob in objects]
                stored[j].view(-1)[e] += sign * h
                sides.append(loss(stored))
            fd = (sides[0] - sides[1]) / (2 * h)
            rel = abs(fd - float(flat[e])) / abs(float(flat[e]))
            print(f"{degree} {name} object {j} element {e}: autograd {float(flat[e]):.6e}, central difference {fd:.6e}, rel {rel:.2e}")
            assert rel < 1e-6


@pytest.mark.parametrize("degree", [None, 2], ids=["rgba", "sh2"])
def test_a_volume_listed_twice_gets_the_sum_of_its_listings(degree):
    a, _ = S.stored_pair(degree)
    objects = [S.obj(a, degree=degree), S.obj(a, R.POSE_OVERLAP, degree=degree)]
    ref = R.reference(degree, "overlap", "n150")                       # (its rays and upstream gradients will do)
    args = (ref["rays"], objects, ref["step"])
    apart = F.gradients(*args, **ref["ups"], **ref["kw"])
    shared = F.gradients(*args, share=True, **ref["ups"], **ref["kw"])
    assert shared[0] is shared[1] and apart[0] is not apart[1]
    assert bool(apart[0].any()) and bool(apart[1].any()) and not torch.equal(apart[0], apart[1])
    assert G.error(shared[0], apart[0] + apart[1]) < 1e-13
    # the same volume at the SAME pose: the two listings' gradients are equal
    same = F.gradients(ref["rays"], [objects[0], objects[0]], ref["step"], **ref["ups"], **ref["kw"])
    assert bool(same[0].any()) and G.error(same[1], same[0]) < 1e-13


def test_references_reach_every_object_and_the_host_fit_loop_descends():
    for degree in (None, 0, 1, 2):
        ref = F.reference(degree, "three", "n150_bits10_terminate")    # (asserts a non-zero gradient for every object)
        assert len(ref["ref64"]) == 3 and all(g.shape == torch.Size(ob["stored"].shape) for g, ob in zip(ref["ref64"], ref["objects"]))
    assert len(F.long_reference()["ref64"]) == 2
    losses = {dtype: F.fit_ref(dtype, **F.FIT) for dtype in (torch.float32, torch.float64)}
    spread = abs(losses[torch.float32][-1] - losses[torch.float64][-1])
    print(f"host fit_scene loop: first {losses[torch.float64][0]:.6e}, final fp64 {losses[torch.float64][-1]!r}, fp32 "
          f"{losses[torch.float32][-1]!r}, spread {spread:.3e}")
    assert losses[torch.float64][-1] < 0.25 * losses[torch.float64][0]
