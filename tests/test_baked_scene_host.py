"""Host tests (no GPU) of the scene march: the layout of PnrBakedObject, every refusal of pnr_baked_scene_render_rays / _views and
of ops.baked_scene_render / util.bake.BakedScene that needs no device, and the restatement tests/baked_scene_ref.py held to the
properties the header states -- (a), (b), (d), (e) bit for bit in fp32, (c), and the fp32 - fp64 gaps that are the GPU test's bar."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import baked_ref as B
import baked_scene_ref as S
import baked_sh_ref as SH
from pixelnerf_amd import _lib


# ---------------------------------------------------------------- the struct and the prototypes

def test_struct_layout_against_the_header_compiled_by_gcc(repo_root, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _lib.PnrBakedObject
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pixelnerf_hip.h"', 'int main(void) {',
             '  printf("max %d\\n", PNR_BAKED_SCENE_MAX_OBJECTS);', '  printf("size %zu\\n", sizeof(PnrBakedObject));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(PnrBakedObject, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["max"]) == 8 == _lib.BAKED_SCENE_MAX_OBJECTS
    assert int(got["size"]) == ctypes.sizeof(cls) == 128
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


def test_header_declares_and_binding_binds(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("pnr_baked_scene_render_rays", 11), ("pnr_baked_scene_render_views", 19)):
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert len(_lib.PROTOTYPES[name][1]) == nargs
    assert hasattr(_lib.load(), "pnr_baked_scene_render_rays")


# ---------------------------------------------------------------- refusals of the two entries, before any device work

P = 64  # a non-null, 16-byte aligned stand-in for a device pointer: every call below must fail before it is touched


def _object(stored=P, bits=None, index=None, M=0, n=(4, 5, 6), degree=-1, half=0, reserved=0, c1=(-1, -1, -1), c2=(1, 1, 1), pose=None):
    o = _lib.PnrBakedObject()
    o.stored, o.bits, o.index, o.M = stored, bits, index, M
    o.nx, o.ny, o.nz = n
    o.degree, o.storage_half, o.reserved = degree, half, reserved
    o.c1[:], o.c2[:] = [float(v) for v in c1], [float(v) for v in c2]
    o.pose[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] if pose is None else [float(v) for v in np.asarray(pose).flatten()[:12]]
    return o


def _array(*objects):
    return (_lib.PnrBakedObject * len(objects))(*objects)


@pytest.mark.parametrize("form", ["rays", "views"])
def test_entries_refuse_bad_arguments_before_any_device_work(form):
    lib = _lib.load()

    def call(objects=None, n=None, step=0.1, term=0.0, src=P, R=4, rgb=P, depth=P, alpha=P):
        objects = _array(_object()) if objects is None else objects
        n = (len(objects) if objects is not None else 1) if n is None else n
        if form == "rays":
            return lib.pnr_baked_scene_render_rays(src, R, objects, n, step, 0, term, rgb, depth, alpha, None)
        return lib.pnr_baked_scene_render_views(src, R, 4, 4, 10.0, 10.0, 2.0, 2.0, 0.5, 3.0, objects, n, step, 0, term, rgb, depth, alpha, None)

    def refused(fragment, **kw):
        assert call(**kw) == -1, fragment
        msg = lib.pnr_last_error()
        assert fragment in msg and msg.startswith(b"pnr_baked_scene_render_" + form.encode()), (fragment, msg)

    nine = _array(*[_object() for _ in range(9)])
    refused(b"n_objects must lie in [1, 8]", n=0)
    refused(b"n_objects must lie in [1, 8]", objects=nine, n=9)
    refused(b"n_objects must lie in [1, 8]", n=-1)
    assert call(objects=ctypes.POINTER(_lib.PnrBakedObject)(), n=1) == -1 and b"null argument (objects)" in lib.pnr_last_error()
    refused(b"object 1: reserved must be 0", objects=_array(_object(), _object(reserved=1)))
    refused(b"object 1: mixed kinds", objects=_array(_object(), _object(degree=2)))
    refused(b"object 2: mixed kinds", objects=_array(_object(), _object(), _object(half=1)))
    refused(b"object 1: mixed kinds", objects=_array(_object(), _object(index=P, bits=P, M=10)))
    # what concerns the call as a whole, in the single-volume entries' words
    for step in (0.0, -0.1, float("inf"), float("nan")):
        refused(b"step must be finite and > 0", step=step)
    for term in (-0.01, 1.0, 1.5, float("nan")):
        refused(b"terminate must lie in [0, 1)", term=term)
    refused(b"null argument", src=None)
    refused(b"4-byte aligned", src=P + 1)
    refused(b"bad sizes", R=-1)
    refused(b"null argument", rgb=None)
    refused(b"null argument", depth=None)
    refused(b"null argument", alpha=None)
    refused(b"rgb, depth and alpha must be 4-byte aligned", rgb=P + 2)
    # per object, everything the single-volume check refuses, under the object's position
    refused(b"object 0: degree must be -1 (RGBA), 0, 1 or 2", objects=_array(_object(degree=3)))
    refused(b"object 0: degree must be", objects=_array(_object(degree=-2), _object(degree=-2)))
    refused(b"object 0: storage_half must be 0 or 1", objects=_array(_object(half=2)))
    refused(b"object 1: every axis needs at least 2 grid points", objects=_array(_object(), _object(n=(1, 4, 4))))
    refused(b"object 1: the grid must have fewer than 2^31 cells", objects=_array(_object(), _object(n=(2049, 2049, 2049))))
    refused(b"object 1: c1 / c2 must be finite with c1 < c2", objects=_array(_object(), _object(c1=(1, 1, 1), c2=(-1, -1, -1))))
    refused(b"object 0: c1 / c2 must be finite", objects=_array(_object(c2=(1, float("nan"), 1))))
    refused(b"object 1: null argument", objects=_array(_object(), _object(stored=None)))
    refused(b"object 1: stored must be 16-byte aligned", objects=_array(_object(), _object(stored=P + 8)))
    refused(b"object 0: bits, rgb, depth and alpha must be 4-byte aligned", objects=_array(_object(bits=P + 2)))
    refused(b"object 0: bad sizes (M)", objects=_array(_object(index=P, bits=P, M=-1)))
    refused(b"object 0: null argument", objects=_array(_object(index=P, bits=None, M=10)))      # sparse rows without their grid
    refused(b"object 0: index must be 4-byte aligned", objects=_array(_object(index=P + 2, bits=P, M=10)))
    # the pose: finite and rigid
    bad = b"pose must be finite and rigid"
    eye = np.eye(4)[:3]
    for pose in (eye * 1.01, eye * np.array([[1.0], [1.0], [-1.0]]), eye + np.array([[0, 2e-4, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]),
                 np.where(np.arange(12).reshape(3, 4) == 3, np.nan, eye), np.where(np.arange(12).reshape(3, 4) == 5, np.inf, eye),
                 np.zeros((3, 4))):
        refused(b"object 1: " + bad, objects=_array(_object(), _object(pose=pose)))
    # within the bar: an fp32 rotation, and a shear below 1e-4
    ang = np.float32(0.7)
    rot = np.array([[np.cos(ang), -np.sin(ang), 0, 5.0], [np.sin(ang), np.cos(ang), 0, -2.0], [0, 0, 1, 0.5]], np.float32)
    small_shear = eye + np.array([[0, 5e-5, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    none = dict(src=None, R=0, rgb=None, depth=None, alpha=None)
    assert call(objects=_array(_object(pose=rot), _object(pose=small_shear)), **none) == 0      # no rays: a no-op
    assert call(objects=_array(_object(stored=None)), **none) == 0
    assert call(objects=_array(_object(pose=eye * 2)), **none) == -1 and bad in lib.pnr_last_error()   # refusals come before the no-op


# ---------------------------------------------------------------- refusals of ops and BakedScene that need no device

def _fake(cls, stored, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    """a volume object without its device parts"""
    from pixelnerf_amd.util import bake
    v = cls.__new__(cls)
    setattr(v, cls._stored_name, stored)
    v.c1, v.c2, v.skip_threshold = lo, hi, 0.0
    if cls is bake.SparseBakedVolume:
        v.reso, v.degree = (4, 5, 6), (None if stored.dim() == 2 else {1: 0, 4: 1, 9: 2}[stored.shape[1]])
    else:
        v.reso = tuple(stored.shape[:3])
        if cls is bake.BakedSHVolume:
            v.degree = {1: 0, 4: 1, 9: 2}[stored.shape[3]]
    return v


def test_wrappers_refuse_before_any_device_work():
    from pixelnerf_amd import ops
    from pixelnerf_amd.util.bake import BakedScene, BakedSHVolume, BakedVolume, SparseBakedVolume
    vol, rays, poses = torch.zeros(4, 5, 6, 4), torch.zeros(3, 8), torch.eye(4)[None]
    lo, hi, eye = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), torch.eye(4)
    one = (vol, None, (4, 5, 6), lo, hi, eye)
    for objects in ([], [one] * 9, None):
        with pytest.raises(ValueError, match="1 to 8"):
            ops.baked_scene_render(rays, objects, 0.1)
    with pytest.raises(ValueError, match="object 0 must be"):
        ops.baked_scene_render(rays, [(vol, None, (4, 5, 6))], 0.1)
    with pytest.raises(TypeError, match="object 1: stored"):
        ops.baked_scene_render(rays, [one, (vol.double(), None, (4, 5, 6), lo, hi, eye)], 0.1)
    # the pose: its shape, finite, rigid
    nan_t = eye.clone()
    nan_t[0, 3] = float("nan")
    for pose in (torch.eye(3), eye * 1.01, torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0])), eye + 2e-4 * torch.eye(4).roll(1, 1), nan_t):
        with pytest.raises(ValueError, match="object 0: pose"):
            ops.baked_scene_render(rays, [(vol, None, (4, 5, 6), lo, hi, pose)], 0.1)
    assert ops._baked_pose("x", eye[:3]) == ops._baked_pose("x", eye.numpy()) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    # one kind per scene
    for other in ((torch.zeros(4, 5, 6, 9, 4), 2), (vol.half(), None)):
        with pytest.raises(ValueError, match="objects 0 and 1 differ in kind"):
            ops.baked_scene_render(rays, [one, (other[0], other[1], (4, 5, 6), lo, hi, eye)], 0.1)
    with pytest.raises(ValueError, match="objects 0 and 1 differ in kind"):
        ops.baked_scene_render(rays, [one, (torch.zeros(7, 4), None, (4, 5, 6), lo, hi, eye, torch.zeros(2, dtype=torch.int32),
                                            torch.zeros(4, 5, 6, dtype=torch.int32))], 0.1)
    # per object, the single-volume wrappers' checks under the object's position
    for kw in (dict(reso=(4, 5)), dict(reso=(1, 5, 6)), dict(c1=hi, c2=lo), dict(degree=3), dict(step=0.0), dict(step=float("nan")),
               dict(terminate=1.0), dict(terminate=-0.1)):
        a = dict(reso=(4, 5, 6), c1=lo, c2=hi, degree=None, step=0.1, terminate=0.0)
        a.update(kw)
        with pytest.raises(ValueError, match="object 0"):
            ops.baked_scene_render(rays, [(vol, a["degree"], a["reso"], a["c1"], a["c2"], eye)], a["step"], terminate=a["terminate"])
        with pytest.raises(ValueError, match="object 0"):
            ops.baked_scene_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, [(vol, a["degree"], a["reso"], a["c1"], a["c2"], eye)], a["step"],
                                         terminate=a["terminate"])
    with pytest.raises(ValueError, match="at least one pixel"):
        ops.baked_scene_render_views(poses, 0, 4, 10.0, None, 0.5, 3.0, [one], 0.1)
    with pytest.raises(ValueError, match="index and bits are mandatory"):
        ops.baked_scene_render(rays, [(torch.zeros(7, 4), None, (4, 5, 6), lo, hi, eye, None, torch.zeros(4, 5, 6, dtype=torch.int32))], 0.1)
    with pytest.raises(_lib.PixelNerfHipError):                        # CPU tensors: there is no CPU path
        ops.baked_scene_render(rays, [one], 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_scene_render_views(poses, 4, 4, 10.0, None, 0.5, 3.0, [one], 0.1)

    # BakedScene
    a, b = _fake(BakedVolume, vol), _fake(BakedVolume, torch.zeros(3, 3, 3, 4))
    scene = BakedScene([a, b], torch.eye(4)[None].repeat(2, 1, 1))
    assert len(scene) == 2 and scene.poses.dtype == torch.float32 and scene.poses.device.type == "cpu" and scene.volumes == [a, b]
    assert tuple(BakedScene([a], torch.eye(4)[None, :3]).poses.shape) == (1, 3, 4)
    assert scene._march_args(None, None) == (min(min(a.cell_size), min(b.cell_size)), 0.0) and scene._march_args(0.25, 0.5) == (0.25, 0.5)
    moved = scene.with_pose(1, torch.tensor(S.POSE_OVERLAP))
    assert moved is not scene and moved.volumes[1] is b and torch.equal(scene.poses[1], torch.eye(4))
    assert torch.equal(moved.poses[1, :3], torch.tensor(S.POSE_OVERLAP)) and torch.equal(moved.poses[0], torch.eye(4))
    with pytest.raises(IndexError):
        scene.with_pose(2, torch.eye(4))
    with pytest.raises(ValueError, match="rigid"):
        scene.with_pose(0, torch.eye(4) * 2)
    with pytest.raises(ValueError, match=r"\(3,4\) or \(4,4\)"):
        scene.with_pose(0, torch.eye(3))
    for volumes in ([], [a] * 9, a):
        with pytest.raises(ValueError, match="1 to 8"):
            BakedScene(volumes, torch.eye(4)[None])
    with pytest.raises(ValueError, match="not a baked volume"):
        BakedScene([a, vol], torch.eye(4)[None].repeat(2, 1, 1))
    two = torch.eye(4)[None].repeat(2, 1, 1)
    mixed = [_fake(BakedVolume, vol.half()), _fake(BakedSHVolume, torch.zeros(4, 5, 6, 4, 4)), _fake(SparseBakedVolume, torch.zeros(7, 4))]
    for other in mixed:
        with pytest.raises(ValueError) as err:
            BakedScene([a, other], two)
        text = str(err.value)
        assert "volumes 0 and 1 differ in kind" in text
        for fix in (".float()", ".half()", ".sparse(occ)", ".to_dense()", "sh.at_direction(d)"):
            assert fix in text, fix
    with pytest.raises(ValueError, match="volumes 0 and 2"):
        BakedScene([a, b, mixed[0]], torch.eye(4)[None].repeat(3, 1, 1))
    with pytest.raises(ValueError, match="differ in kind"):          # the degree is part of the kind
        BakedScene([_fake(BakedSHVolume, torch.zeros(4, 5, 6, 4, 4)), _fake(BakedSHVolume, torch.zeros(4, 5, 6, 9, 4))], two)
    for poses_bad in (torch.eye(4)[None], torch.eye(4), torch.eye(3)[None].repeat(2, 1, 1)):
        with pytest.raises(ValueError, match="poses must be"):
            BakedScene([a, b], poses_bad)
    with pytest.raises(ValueError, match="object 1: pose is not rigid"):
        BakedScene([a, b], torch.stack([torch.eye(4), torch.eye(4) * 1.5]))
    with pytest.raises(ValueError, match=r"rays must be \(...,8\)"):
        scene.render(torch.zeros(3, 7))
    with pytest.raises(ValueError, match="poses_c2w must be"):
        scene.render_views(torch.eye(4), 4, 4, 10.0, 0.5, 3.0)
    with pytest.raises(ValueError, match="gt_rgb must be"):
        scene.render_views(poses, 4, 4, 10.0, 0.5, 3.0, gt_rgb=torch.zeros(1, 4, 5, 3))
    with pytest.raises(_lib.PixelNerfHipError):
        scene.render(rays, skip=False)


# ---------------------------------------------------------------- the restatement satisfies what the header states

def _same(x, y):
    return all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(x, y))


@pytest.fixture(scope="module")
def shared():
    """the shared inputs per setting, and the fp32 renders several tests compare (computed once, never modified)"""
    case = {"A": S.common_volume(), "B": S.common_volume(seed=99), "cA": SH.common_coef(2), "rays": {}, "step": {}}
    for setting, (_, _, step) in S.SETTINGS.items():
        case["rays"][setting], case["step"][setting] = S.common_rays(setting), step
    return case


def test_the_basis_restated_is_the_shared_one(shared):
    for d in shared["rays"]["n40"][:, 3:6]:
        for degree in (0, 1, 2):
            assert np.array_equal(S.basis(d, degree, np.float32), SH.sh_basis(d, degree, np.float32))
            assert np.array_equal(S.basis(d.astype(np.float64), degree), SH.sh_basis(d, degree))
    assert np.array_equal(S.basis(np.zeros(3, np.float32), 2, np.float32), np.array([1] + [0] * 8, np.float32))


@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
def test_a_one_object_at_the_identity_is_the_single_march(shared, setting):
    rays, step = shared["rays"][setting], shared["step"][setting]
    for white in (False, True):
        for term in (0.0, 1e-2):
            kw = dict(white_bkgd=white, terminate=term, dtype=np.float32)
            assert _same(S.render_ref(rays, [S.obj(shared["A"])], step, **kw), B.render_ref(rays, shared["A"], S.C1, S.C2, step, **kw))
    kw = dict(dtype=np.float32)
    assert _same(S.render_ref(rays, [S.obj(shared["cA"], degree=2)], step, **kw), SH.render_ref(rays, shared["cA"], S.C1, S.C2, step, 2, **kw))
    occupied = (shared["A"][..., 3] > 0)
    occupied = np.stack([occupied[i:8 + i, j:7 + j, k:6 + k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]).any(axis=0)
    assert _same(S.render_ref(rays, [S.obj(shared["A"], occupied=occupied)], step, **kw),
                 B.render_ref(rays, shared["A"], S.C1, S.C2, step, occupied=occupied, **kw))
    assert _same(S.whiten(S.render_ref(rays, [S.obj(shared["A"])], step, **kw)), S.render_ref(rays, [S.obj(shared["A"])], step, white_bkgd=True, **kw))


@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
def test_b_a_signed_permutation_is_the_single_march_on_the_moved_rays(shared, setting):
    rays, step = shared["rays"][setting], shared["step"][setting]
    moved = S.object_rays(rays, S.POSE_OVERLAP, np.float32)
    assert moved.dtype == np.float32 and np.array_equal(moved[:, 6:], rays[:, 6:])
    # Rz^T (x, y, z) = (y, -x, z), exactly, on q = o - t formed by one fp32 subtraction
    q = rays[:, 0:3] - S.POSE_OVERLAP[:, 3][None]
    assert np.array_equal(moved[:, 0:3], np.stack((q[:, 1], -q[:, 0], q[:, 2]), axis=1))
    assert np.array_equal(moved[:, 3:6], np.stack((rays[:, 4], -rays[:, 3], rays[:, 5]), axis=1))
    kw = dict(dtype=np.float32)
    assert _same(S.render_ref(rays, [S.obj(shared["A"], S.POSE_OVERLAP)], step, **kw), B.render_ref(moved, shared["A"], S.C1, S.C2, step, **kw))
    got = S.render_ref(rays, [S.obj(shared["cA"], S.POSE_OVERLAP, degree=2)], step, **kw)
    assert _same(got, SH.render_ref(moved, shared["cA"], S.C1, S.C2, step, 2, **kw))
    assert not _same(got, SH.render_ref(rays, shared["cA"], S.C1, S.C2, step, 2, **kw))


@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
def test_d_two_objects_commute_and_e_a_volume_twice_is_sigma_doubled(shared, setting):
    rays, step = shared["rays"][setting], shared["step"][setting]
    kw = dict(dtype=np.float32)
    a, b = S.obj(shared["A"]), S.obj(shared["B"], S.POSE_OVERLAP)
    ab = S.render_ref(rays, [a, b], step, **kw)
    assert _same(ab, S.render_ref(rays, [b, a], step, **kw))
    assert not _same(ab, S.render_ref(rays, [a], step, **kw))                      # B is in view
    doubled = shared["A"].copy()
    doubled[..., 3] *= 2
    assert _same(S.render_ref(rays, [a, a], step, **kw), S.render_ref(rays, [S.obj(doubled)], step, **kw))
    ca, cb = S.obj(shared["cA"], degree=2), S.obj(S.common_coef_b(2), S.POSE_OVERLAP, degree=2)
    assert _same(S.render_ref(rays, [ca, cb], step, **kw), S.render_ref(rays, [cb, ca], step, **kw))


@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
def test_c_an_object_a_ray_never_meets_changes_nothing(shared, setting):
    rays, step = shared["rays"][setting], shared["step"][setting]
    kw = dict(dtype=np.float32)
    a, b = S.obj(shared["A"]), S.obj(shared["B"], S.POSE_DISJOINT)
    alone = S.render_ref(rays, [b], step, **kw)
    never = alone[2] == 0
    assert int(never.sum()) == 31 and int((~never).sum()) == 6
    both, only_a = S.render_ref(rays, [a, b], step, **kw), S.render_ref(rays, [a], step, **kw)
    assert all(np.array_equal(x[never], y[never]) for x, y in zip(both, only_a))
    assert not np.array_equal(both[0][~never], only_a[0][~never])


@pytest.mark.parametrize("degree", [None, 2], ids=["rgba", "degree2"])
@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
def test_gpu_parity_inputs_carry_their_bar(setting, degree):
    """the fp32 - fp64 gap of every scene the GPU test renders lies in (0, 1e-4): 4 x the gap is its bar"""
    rays, step = S.common_rays(setting), S.SETTINGS[setting][2]
    for name, objects in S.cases(degree).items():
        r64, r32 = S.render_ref(rays, objects, step), S.render_ref(rays, objects, step, dtype=np.float32)
        for out in ((r32, r64), (S.whiten(r32), S.whiten(r64))):
            for g in S.gaps(*out):
                assert 0.0 < g < 1e-4, (name, g)
        missed = r64[2] == 0                                              # rays that miss every object, and the near >= far ray
        assert missed[36] and int(missed.sum()) >= 2 and int((~missed).sum()) >= 26, (name, np.nonzero(missed)[0])
        assert (r64[0][missed] == 0).all() and (r64[1][missed] == 0).all()
