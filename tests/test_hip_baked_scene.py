"""GPU tests (-m gpu) of the scene march: pnr_baked_scene_render_rays / _views through ops.baked_scene_render and
util.bake.BakedScene.  The header ("Scenes of several baked volumes") states what the rules imply, (a) .. (h); every one is held
here bit for bit against the single-volume entries or against the kernel itself, and the mixing against the fp64 restatement of
tests/baked_scene_ref.py (its own checks, and the checks of the inputs used here: tests/test_baked_scene_host.py).

Parity bar, per output, as tests/test_hip_baked.py: 4 x max |fp32 restatement - fp64 restatement| over the same inputs, computed
here; the factor covers the scan order of the product, which differs from the restatement's sequential loop."""
import numpy as np
import pytest
import torch

import baked_scene_ref as S
import baked_sh_ref as SH

pytestmark = pytest.mark.gpu

KINDS = ["rgba", "sh0", "sh1", "sh2", "rgba_half", "sh2_half", "rgba_sparse", "sh2_sparse"]
DEGREE = {"rgba": None, "sh2": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bake():
    from pixelnerf_amd.util import bake as _bake
    return _bake


def _volume(bake, dev, stored, c1=S.C1, c2=S.C2):
    stored = torch.from_numpy(np.ascontiguousarray(stored)).to(dev)
    return (bake.BakedVolume if stored.dim() == 4 else bake.BakedSHVolume).from_tensor(stored, c1, c2)


@pytest.fixture(scope="module")
def common(dev, bake):
    """the shared rays per setting, objects A and B of both kinds, and every kind of A (made once, never modified)"""
    case = {"rays": {s: torch.from_numpy(S.common_rays(s)).to(dev) for s in S.SETTINGS}, "np_rays": {s: S.common_rays(s) for s in S.SETTINGS}}
    for kind, degree in DEGREE.items():
        a, b = S.stored_pair(degree)
        case["A", kind], case["B", kind] = _volume(bake, dev, a), _volume(bake, dev, b)
    case["A", "sh0"], case["A", "sh1"] = _volume(bake, dev, SH.common_coef(0)), _volume(bake, dev, SH.common_coef(1))
    for kind in ("rgba", "sh2"):
        case["A", kind + "_half"], case["A", kind + "_sparse"] = case["A", kind].half(), case["A", kind].sparse()
    return case


def _pose(*poses):
    return torch.from_numpy(np.stack([np.asarray(p, np.float32)[:3] for p in poses]))


def _np(out):
    return tuple(t.cpu().numpy() for t in (out.rgb, out.depth, out.alpha))


def _equal(a, b):
    return torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.alpha, b.alpha)


# ---------------------------------------------------------------- 1. (a): one object at the identity is the single-volume march

@pytest.mark.parametrize("kind", KINDS)
def test_a_identity_pose_renders_the_single_volume_bytes(bake, common, kind):
    vol = common["A", kind]
    scene = bake.BakedScene([vol], _pose(S.IDENTITY))
    assert len(scene) == 1
    for setting, (_, _, step) in S.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in (dict(), dict(skip=False), dict(white_bkgd=True), dict(terminate=1e-2), dict(white_bkgd=True, terminate=1e-2, skip=False)):
            if kind.endswith("_sparse") and not kw.get("skip", True):
                continue                                                # a sparse volume has no unskipped march
            single, got = vol.render(rays, step=step, **kw), scene.render(rays, step=step, **kw)
            assert got.rgb.dtype == torch.float32 and tuple(got.rgb.shape) == (37, 3) and tuple(got.depth.shape) == tuple(got.alpha.shape) == (37,)
            assert _equal(got, single), (setting, kw)
            assert float(single.alpha.max()) > 0.5
    assert _equal(scene.render(rays), vol.render(rays))                 # step=None: the smallest cell edge
    lead = scene.render(rays.reshape(37, 1, 8))                         # leading dimensions are kept
    assert tuple(lead.rgb.shape) == (37, 1, 3) and tuple(lead.alpha.shape) == (37, 1)


# ---------------------------------------------------------------- 2. (b): a signed permutation is the single march on the moved rays

@pytest.mark.parametrize("kind", sorted(DEGREE))
def test_b_quarter_turn_renders_the_single_volume_on_the_moved_rays(bake, dev, common, kind):
    vol = common["A", kind]
    scene = bake.BakedScene([vol], _pose(S.POSE_OVERLAP))
    for setting, (_, _, step) in S.SETTINGS.items():
        rays = common["rays"][setting]
        moved = torch.from_numpy(S.object_rays(common["np_rays"][setting], S.POSE_OVERLAP, np.float32)).to(dev)   # the same fp32 operations
        for kw in (dict(), dict(white_bkgd=True, skip=False)):
            got = scene.render(rays, step=step, **kw)
            assert _equal(got, vol.render(moved, step=step, **kw)), (setting, kw)
            assert not _equal(got, vol.render(rays, step=step, **kw))
    if kind == "sh2":                                                   # the basis is evaluated on the ROTATED direction
        wrong = moved.clone()
        wrong[:, 3:6] = rays[:, 3:6]
        assert not torch.equal(got.rgb, vol.render(wrong, step=step, **kw).rgb)


# ---------------------------------------------------------------- 3. parity with the fp64 restatement

@pytest.fixture(scope="module")
def parity(bake, dev):
    """per (kind, setting, case): the scene on the device, and the restatement's answers in fp64 and fp32 (computed once)"""
    out = {}
    for kind, degree in DEGREE.items():
        for name, objects in S.cases(degree).items():
            scene = bake.BakedScene([_volume(bake, dev, o["stored"], o["c1"], o["c2"]) for o in objects], _pose(*[o["pose"] for o in objects]))
            for setting, (_, _, step) in S.SETTINGS.items():
                rays = S.common_rays(setting)
                out[kind, setting, name] = (scene, S.render_ref(rays, objects, step), S.render_ref(rays, objects, step, dtype=np.float32))
    return out


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("name", ["overlap", "disjoint", "three"])
@pytest.mark.parametrize("setting", sorted(S.SETTINGS))
@pytest.mark.parametrize("kind", sorted(DEGREE))
def test_parity_with_the_fp64_restatement(common, parity, kind, setting, name, white):
    scene, r64, r32 = parity[kind, setting, name]
    assert len(scene) == (3 if name == "three" else 2)
    if name == "three":
        assert scene.volumes[1].reso == S.SMALL_RESO and len({v.reso for v in scene.volumes}) == 2
    missed = (r64[2] == 0) & (r32[2] == 0)
    if white:
        r64, r32 = S.whiten(r64), S.whiten(r32)
    out = scene.render(common["rays"][setting], step=S.SETTINGS[setting][2], white_bkgd=white, skip=False)
    got = _np(out)
    gap, err = S.gaps(r32, r64), S.gaps(got, r64)
    print(f"{kind} {setting} {name} white={white}: fp32 - fp64 gap rgb {gap[0]:.3e} depth {gap[1]:.3e} alpha {gap[2]:.3e}; "
          f"kernel - fp64 rgb {err[0]:.3e} depth {err[1]:.3e} alpha {err[2]:.3e}")
    for what, g, e in zip(("rgb", "depth", "alpha"), gap, err):
        assert 0.0 < g < 1e-4, (what, g)
        assert e <= 4.0 * g, (what, e, 4.0 * g)
    assert missed[36] and int(missed.sum()) >= 2                        # rays that miss everything, and the near >= far ray:
    bg = 1.0 if white else 0.0                                          # exactly the background
    assert (got[0][missed] == bg).all() and (got[1][missed] == 0.0).all() and (got[2][missed] == 0.0).all()


# ---------------------------------------------------------------- 4. (c): an object a ray never meets leaves its bytes alone

@pytest.mark.parametrize("kind", sorted(DEGREE))
def test_c_an_object_with_no_density_on_a_ray_changes_nothing(bake, common, kind):
    a, b = common["A", kind], common["B", kind]
    for setting, (_, _, step) in S.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in (dict(), dict(skip=False, white_bkgd=True)):
            alone = bake.BakedScene([b], _pose(S.POSE_DISJOINT)).render(rays, step=step, **kw)
            never = alone.alpha == 0
            print(f"{kind} {setting} {kw}: B alone leaves {int(never.sum())} rays at alpha 0, {int((~never).sum())} see it")
            assert int(never.sum()) >= 20 and int((~never).sum()) >= 4, (int(never.sum()), int((~never).sum()))
            both = bake.BakedScene([a, b], _pose(S.IDENTITY, S.POSE_DISJOINT)).render(rays, step=step, **kw)
            only_a = bake.BakedScene([a], _pose(S.IDENTITY)).render(rays, step=step, **kw)
            assert torch.equal(both.rgb[never], only_a.rgb[never]) and torch.equal(both.depth[never], only_a.depth[never])
            assert torch.equal(both.alpha[never], only_a.alpha[never])
            assert not torch.equal(both.rgb[~never], only_a.rgb[~never])  # B is seen where it stands
            flipped = bake.BakedScene([b, a], _pose(S.POSE_DISJOINT, S.IDENTITY)).render(rays, step=step, **kw)
            assert torch.equal(flipped.rgb[never], only_a.rgb[never]) and torch.equal(flipped.alpha[never], only_a.alpha[never])


# ---------------------------------------------------------------- 5. (d), (e), (f), (g)

@pytest.mark.parametrize("kind", sorted(DEGREE))
def test_d_e_f_g_bit_for_bit(bake, dev, common, kind):
    a, b = common["A", kind], common["B", kind]
    doubled = a._stored().clone()
    doubled[..., 3] *= 2
    a2 = type(a).from_tensor(doubled, a.c1, a.c2)
    ab = bake.BakedScene([a, b], _pose(S.IDENTITY, S.POSE_OVERLAP))
    ba = bake.BakedScene([b, a], _pose(S.POSE_OVERLAP, S.IDENTITY))
    assert ab.with_pose(1, S.POSE_DISJOINT).volumes[1] is b
    for setting, (_, _, step) in S.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in (dict(), dict(white_bkgd=True, terminate=1e-2)):
            out = ab.render(rays, step=step, **kw)
            assert _equal(out, ba.render(rays, step=step, **kw)), ("d", setting, kw)
            assert not _equal(out, a.render(rays, step=step, **kw))
            for pose in (S.IDENTITY, S.POSE_OVERLAP):
                twice = bake.BakedScene([a, a], _pose(pose, pose)).render(rays, step=step, **kw)
                assert _equal(twice, bake.BakedScene([a2], _pose(pose)).render(rays, step=step, **kw)), ("e", setting, kw)
            assert _equal(twice, a2.render(torch.from_numpy(S.object_rays(common["np_rays"][setting], S.POSE_OVERLAP)).to(dev), step=step, **kw))
            assert _equal(out, ab.render(rays, step=step, skip=False, **kw)), ("f", setting, kw)
            assert _equal(out, ab.render(rays, step=step, **kw)), ("g", setting, kw)
            assert _equal(out, ab.with_pose(1, S.POSE_DISJOINT).with_pose(1, S.POSE_OVERLAP).render(rays, step=step, **kw))
    # (d) for the other layouts: sparse rows, and fp16
    for suffix, other in (("_sparse", b.sparse()), ("_half", b.half())):
        x, y = common["A", kind + suffix], other
        assert _equal(bake.BakedScene([x, y], _pose(S.IDENTITY, S.POSE_OVERLAP)).render(rays, step=step),
                      bake.BakedScene([y, x], _pose(S.POSE_OVERLAP, S.IDENTITY)).render(rays, step=step))
    sparse_scene = bake.BakedScene([common["A", kind + "_sparse"], b.sparse()], _pose(S.IDENTITY, S.POSE_OVERLAP))
    assert _equal(sparse_scene.render(rays, step=step), ab.render(rays, step=step))      # the sparse rows render the dense bytes
    assert _equal(sparse_scene.render(rays, step=step, skip=False), ab.render(rays, step=step))   # (they always march against their grid)


# ---------------------------------------------------------------- 6. (h): the camera form is the array form

def test_h_views_equal_rays_of_the_same_cameras(bake, dev, common):
    from pixelnerf_amd import util
    scene = bake.BakedScene([common["A", "sh2"], common["B", "sh2"]], _pose(S.IDENTITY, S.POSE_DISJOINT))
    poses = torch.stack([util.pose_spherical(30.0, -25.0, 3.4), util.pose_spherical(-110.0, 10.0, 3.0)]).float().to(dev)
    z_near, z_far = 1.0, 5.5
    W, H, focal, c = 5, 4, (4.5, 4.0), (2.25, 2.5)                      # 2 views of 5 x 4
    rays = util.gen_rays(poses, W, H, focal, z_near, z_far, c=c)
    assert tuple(rays.shape) == (2, H, W, 8)
    for kw in (dict(), dict(white_bkgd=True, skip=False, step=0.05), dict(terminate=1e-2)):
        views = scene.render_views(poses, W, H, focal, z_near, z_far, c=c, want_u8=True, **kw)
        assert _equal(views, scene.render(rays, **kw)), kw
        assert tuple(views.rgb.shape) == (2, H, W, 3) and tuple(views.depth.shape) == tuple(views.alpha.shape) == (2, H, W)
        assert views.rgb_u8.dtype == torch.uint8 and tuple(views.rgb_u8.shape) == (2, H, W, 3) and "psnr" not in views
        assert float((views.depth_norm - (views.depth - z_near) / (z_far - z_near)).abs().max()) < 1e-6
    assert float(views.alpha.max()) > 0.5 and float(views.alpha.min()) == 0.0
    bare = scene.render_views(poses, W, H, focal, z_near, z_far, c=c)
    assert "psnr" not in bare and "rgb_u8" not in bare
    # with a ground truth (SSIM's window needs 7 pixels each way): the outputs _Baked.render_views has, shaped as there
    W, H, focal, c = 9, 8, (8.0, 7.5), (4.25, 4.5)
    gt = torch.rand((2, H, W, 3), generator=torch.Generator().manual_seed(3)).to(dev)
    single = common["A", "sh2"].render_views(poses, W, H, focal, z_near, z_far, c=c, gt_rgb=gt, want_u8=True)
    views = scene.render_views(poses, W, H, focal, z_near, z_far, c=c, gt_rgb=gt, want_u8=True)
    assert _equal(views, scene.render(util.gen_rays(poses, W, H, focal, z_near, z_far, c=c)))
    assert sorted(views.keys()) == sorted(single.keys()) == ["alpha", "depth", "depth_norm", "psnr", "rgb", "rgb_u8", "ssim"]
    for key in single.keys():
        assert tuple(views[key].shape) == tuple(single[key].shape) and views[key].dtype == single[key].dtype, key
    assert tuple(views.psnr.shape) == tuple(views.ssim.shape) == (2,) and views.psnr.dtype == torch.float64


# ---------------------------------------------------------------- 7. termination

def test_termination_of_a_front_object_keeps_its_bound(bake, dev):
    """tests/test_hip_baked.py's opaque construction as two objects: the wall (25 x 3 x 3 points over [0,24] x [0,2]^2, sigma on the
    planes x = 3, 4, 5: T ~ 5e-3 behind it, inside samples 0..63) is the FRONT object; the bright block (5 x 3 x 3 points over
    [0,4] x [0,2]^2, planes 1, 2, 3) stands at [I | (18, 0, 0)], world x = 19..21, inside samples 128..191."""
    wall = np.zeros((25, 3, 3, 4), np.float32)
    wall[..., :3] = 0.2
    wall[3:6, :, :, 3] = -np.log(5e-3) / 3.0
    block = np.zeros((5, 3, 3, 4), np.float32)
    block[1:4, :, :, :3] = 1.0
    block[1:4, :, :, 3] = 5.0
    lo, wall_hi, block_hi = (0.0, 0.0, 0.0), (24.0, 2.0, 2.0), (4.0, 2.0, 2.0)
    behind = S.pose_of(np.eye(3), (18.0, 0.0, 0.0))
    scene = bake.BakedScene([_volume(bake, dev, wall, lo, wall_hi), _volume(bake, dev, block, lo, block_hi)], _pose(S.IDENTITY, behind))
    objects = [S.obj(wall, S.IDENTITY, lo, wall_hi), S.obj(block, behind, lo, block_hi)]
    far, step, eps = 24.0, 0.125, 1e-2
    rays = torch.tensor([[0.0, y, z, 1.0, 0.0, 0.0, 0.0, far] for y, z in ((1.0, 1.0), (0.3, 1.7), (1.9, 0.2))], device=dev)
    ref = S.render_ref(rays.cpu().numpy(), objects, step)
    assert abs(1.0 - ref[2][0] - 5e-3 * np.exp(-15.0)) < 1e-4            # what is left behind both
    for skip in (False, True):
        plain = scene.render(rays, step=step, skip=skip)
        assert S.gaps(_np(plain), ref)[0] < 1e-5
        assert _equal(plain, scene.render(rays, step=step, skip=skip, terminate=0.0))
        assert _equal(plain, scene.render(rays, step=step, skip=skip, terminate=1e-3))   # T ~ 5e-3 > eps behind chunks 0 and 1: no stop
        cut = scene.render(rays, step=step, skip=skip, terminate=eps)
        d_rgb, d_alpha = (cut.rgb - plain.rgb).abs().max(dim=1).values, (cut.alpha - plain.alpha).abs()
        d_depth = (cut.depth - plain.depth).abs()
        print(f"terminate {eps} skip={skip}: max d rgb {float(d_rgb.max()):.3e}, d alpha {float(d_alpha.max()):.3e}, "
              f"d depth {float(d_depth.max()):.3e}")
        assert not _equal(cut, plain) and (d_rgb > 0).any()              # the march really stopped ...
        assert (d_rgb <= eps).all() and (d_alpha <= eps).all() and (d_depth <= eps * far).all()   # ... within the bound
        assert S.gaps(_np(cut), S.render_ref(rays.cpu().numpy(), objects, step, terminate=eps))[0] < 1e-5


# ---------------------------------------------------------------- 8. refusals that need device tensors

def test_refusals_with_device_tensors(bake, dev, common):
    from pixelnerf_amd import _lib, ops
    a, rays = common["A", "rgba"], common["rays"]["n40"]
    eye = torch.eye(4)
    with pytest.raises(ValueError, match="volumes 0 and 1 differ in kind"):
        bake.BakedScene([a, common["A", "rgba_half"]], _pose(S.IDENTITY, S.IDENTITY))
    with pytest.raises(ValueError, match="volumes 0 and 1 differ in kind"):
        bake.BakedScene([a, common["A", "sh2"]], _pose(S.IDENTITY, S.IDENTITY))
    with pytest.raises(ValueError, match="volumes 0 and 1 differ in kind"):
        bake.BakedScene([a, common["A", "rgba_sparse"]], _pose(S.IDENTITY, S.IDENTITY))
    with pytest.raises(ValueError, match="differ in kind"):
        bake.BakedScene([common["A", "sh1"], common["A", "sh2"]], _pose(S.IDENTITY, S.IDENTITY))
    for n in (0, 9):
        with pytest.raises(ValueError, match="1 to 8"):
            bake.BakedScene([a] * n, eye[None].repeat(n, 1, 1))
    assert len(bake.BakedScene([a] * 8, eye[None].repeat(8, 1, 1))) == 8
    for pose in (eye * 1.01, torch.diag(torch.tensor([1.0, -1.0, 1.0, 1.0])), eye + 1e-3 * eye.roll(1, 1)):
        with pytest.raises(ValueError, match="not rigid"):
            bake.BakedScene([a], pose[None])
        with pytest.raises(ValueError, match="not rigid"):
            ops.baked_scene_render(rays, [(a.vol, None, a.reso, a.c1, a.c2, pose)], 0.1)
    one = (a.vol, None, a.reso, a.c1, a.c2, eye)
    with pytest.raises(ValueError, match="object 1 lives on cpu"):       # a volume on another device
        ops.baked_scene_render(rays, [one, (a.vol.cpu(), None, a.reso, a.c1, a.c2, eye)], 0.1)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.baked_scene_render(rays.cpu(), [one], 0.1)
    for objects in ([], [one] * 9):
        with pytest.raises(ValueError, match="1 to 8"):
            ops.baked_scene_render(rays, objects, 0.1)
    with pytest.raises(ValueError, match="differ in kind"):
        ops.baked_scene_render(rays, [one, (a.vol.half(), None, a.reso, a.c1, a.c2, eye)], 0.1)
    with pytest.raises(TypeError):
        ops.baked_scene_render(rays, [(a.vol.double(), None, a.reso, a.c1, a.c2, eye)], 0.1)
    with pytest.raises(ValueError, match="expected shape"):              # the tensor against its reso
        ops.baked_scene_render(rays, [(a.vol, None, (9, 8, 8), a.c1, a.c2, eye)], 0.1)
    with pytest.raises(ValueError, match="bits"):
        ops.baked_scene_render(rays, [(a.vol, None, a.reso, a.c1, a.c2, eye, a.occupancy.bits[:-1])], 0.1)
    # eight objects render, and the call with a (3,4) numpy pose is the call with a (4,4) tensor
    rgb8 = ops.baked_scene_render(rays, [one] * 8, 0.1)[0]
    assert torch.isfinite(rgb8).all()
    assert torch.equal(ops.baked_scene_render(rays, [(a.vol, None, a.reso, a.c1, a.c2, S.IDENTITY)], 0.1)[0],
                       ops.baked_scene_render(rays, [one], 0.1)[0])
