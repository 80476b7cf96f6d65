"""Host tests (no GPU) of the shared entry prologue (csrc/pnr_entry.h) and of the latent scatter's plan (csrc/pnr_scatter_plan.h).

Every exported entry that takes a PnrScene is called with dummy device addresses and ONE defect at a time: a defective scene,
defective sample sizes, a point count or a feature grid beyond what the entry's kernels index.  Each must be refused on the host
(PNR_E_INVALID = -1, the message opening with the entry's exported name); a well-formed call must NOT be refused there -- without
a device it fails at its first HIP call (PNR_E_HIP = -2).  The addresses are never dereferenced on the host; the module skips
itself where a device is visible, so that a wrongly accepted call can never launch."""
import ctypes

import pytest
import torch

from pixelnerf_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy addresses: host-only checks, never run where a launch could succeed")

A = 64            # a dummy, 16-byte aligned device address
BIG = 1 << 40     # "large enough" workspace size


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def make_scene(SB=2, NS=1, Hl=8, Wl=8, n_focal=1, n_c=1):
    sc = _lib.PnrScene()
    sc.latent_nhwc, sc.poses, sc.focal, sc.c = A, A, A, A
    sc.SB, sc.NS, sc.Hl, sc.Wl, sc.n_focal, sc.n_c = SB, NS, Hl, Wl, n_focal, n_c
    sc.img_w, sc.img_h = 64.0, 64.0
    return sc


def _filled(cls):
    o = cls()
    for name, typ in cls._fields_:
        if typ is ctypes.c_void_p:
            setattr(o, name, A)
        elif issubclass(typ, ctypes.Array):
            for i in range(typ._length_):
                getattr(o, name)[i] = A
    return o


DUMPS, F32SAVED, SPLITSAVED = _filled(_lib.PnrTrainDumps), _filled(_lib.PnrF32Saved), _filled(_lib.PnrSplitSaved)
WEIGHTS = _filled(_lib.PnrMlpWeights)
_ref = ctypes.byref
OUTS = (A, A, A, A, A, A, A)  # rgb_c .. weights_f, workspace

# name -> (kind, call(lib, a)); a: sc (PnrScene pointer or None), R, n (rays_per_obj), K, rays, z  /  B, xyz, vd  /  NV, W, H, K.
# kinds: "samples" (scene + ray samples), "render" (scene + rays, Kc = K, no fine pass), "views" (scene + cameras), "points",
#        "scene" (scene only), "size" (returns a size or a flag: 0 on a defect)
ENTRIES = {
    "pnr_eval_ray_samples": ("samples", lambda L, a: L.pnr_eval_ray_samples(a["sc"], A, 0, a["rays"], a["z"], a["R"], a["n"], a["K"], A, None)),
    "pnr_eval_ray_samples_folded": ("samples", lambda L, a: L.pnr_eval_ray_samples_folded(a["sc"], A, A, 0, a["rays"], a["z"], a["R"], a["n"], a["K"], A, None)),
    "pnr_eval_ray_samples_split": ("samples", lambda L, a: L.pnr_eval_ray_samples_split(a["sc"], A, A, a["rays"], a["z"], a["R"], a["n"], a["K"], A, None, None)),
    "pnr_eval_ray_samples_train": ("samples", lambda L, a: L.pnr_eval_ray_samples_train(a["sc"], A, 0, a["rays"], a["z"], a["R"], a["n"], a["K"], A, _ref(DUMPS), None)),
    "pnr_eval_ray_samples_split_train": ("samples", lambda L, a: L.pnr_eval_ray_samples_split_train(
        a["sc"], A, A, a["rays"], a["z"], a["R"], a["n"], a["K"], A, _ref(SPLITSAVED), None, None)),
    "pnr_eval_ray_samples_f32": ("samples", lambda L, a: L.pnr_eval_ray_samples_f32(
        a["sc"], _ref(WEIGHTS), a["rays"], a["z"], a["R"], a["n"], a["K"], A, A, BIG, None)),
    "pnr_eval_ray_samples_f32_train": ("samples", lambda L, a: L.pnr_eval_ray_samples_f32_train(
        a["sc"], _ref(WEIGHTS), a["rays"], a["z"], a["R"], a["n"], a["K"], A, _ref(F32SAVED), 0, None)),
    "pnr_fold_latent_f32_rows": ("samples", lambda L, a: L.pnr_fold_latent_f32_rows(
        a["sc"], _ref(WEIGHTS), a["rays"], a["z"], a["R"], a["n"], a["K"], A, A, BIG, None, None)),
    "pnr_position_backward": ("samples", lambda L, a: L.pnr_position_backward(a["sc"], a["rays"], a["z"], a["R"], a["n"], a["K"], A, A, A, None)),
    "pnr_depth_sample_backward": ("samples", lambda L, a: L.pnr_depth_sample_backward(
        a["sc"], a["rays"], a["z"], a["R"], a["n"], a["K"], A, A, 1, A, 0.01, A, A, A, A, None)),
    "pnr_camera_backward": ("samples", lambda L, a: L.pnr_camera_backward(
        a["sc"], a["rays"], a["z"], a["R"], a["n"], a["K"], 0, A, A, None, None, None, None, 0, None, 0.01, A, A, A, A, A, None)),
    "pnr_latent_scatter": ("samples", lambda L, a: L.pnr_latent_scatter(a["sc"], a["rays"], a["z"], a["R"], a["n"], a["K"], A, A, A, BIG, None)),
    "pnr_latent_scatter_workspace_bytes": ("size", lambda L, a: L.pnr_latent_scatter_workspace_bytes(a["sc"], a["R"], a["n"], a["K"])),
    "pnr_latent_scatter_single_owner": ("size", lambda L, a: L.pnr_latent_scatter_single_owner(a["sc"], a["R"], a["n"], a["K"])),
    "pnr_render_forward": ("render", lambda L, a: L.pnr_render_forward(
        a["sc"], A, A, 0, a["rays"], a["R"], a["n"], a["K"], 0, 0, 0.01, 0, 0, A, A, A, A, *OUTS, None)),
    "pnr_render_forward_folded": ("render", lambda L, a: L.pnr_render_forward_folded(
        a["sc"], A, A, A, A, 0, a["rays"], a["R"], a["n"], a["K"], 0, 0, 0.01, 0, 0, A, A, A, A, *OUTS, None, None, None)),
    "pnr_render_forward_seeded": ("render", lambda L, a: L.pnr_render_forward_seeded(
        a["sc"], A, A, A, A, 0, a["rays"], a["R"], a["n"], a["K"], 0, 0, 0.01, 0, 0, 7, 0, 0, *OUTS, None, None, None)),
    "pnr_render_views": ("views", lambda L, a: L.pnr_render_views(
        a["sc"], A, A, A, A, 0, A, a["NV"], a["W"], a["H"], 1.0, 1.0, 1.0, 1.0, 0.5, 2.0, a["K"], 0, 0, 0.01, 0, 0,
        None, None, None, None, 7, *OUTS, None, None, None)),
    "pnr_eval_points": ("points", lambda L, a: L.pnr_eval_points(a["sc"], A, 0, a["xyz"], a["vd"], a["B"], A, None)),
    "pnr_eval_points_folded": ("points", lambda L, a: L.pnr_eval_points_folded(a["sc"], A, A, 0, a["xyz"], a["vd"], a["B"], A, None)),
    "pnr_eval_points_split": ("points", lambda L, a: L.pnr_eval_points_split(a["sc"], A, A, a["xyz"], a["vd"], a["B"], A, None, None)),
    "pnr_eval_points_f32": ("points", lambda L, a: L.pnr_eval_points_f32(a["sc"], _ref(WEIGHTS), a["xyz"], a["vd"], a["B"], A, A, BIG, None)),
    "pnr_point_features_f32": ("points", lambda L, a: L.pnr_point_features_f32(a["sc"], a["xyz"], a["vd"], a["B"], A, A, None)),
    "pnr_fold_latent": ("scene", lambda L, a: L.pnr_fold_latent(a["sc"], _ref(WEIGHTS), 0, A, None)),
    "pnr_fold_latent_f32": ("scene", lambda L, a: L.pnr_fold_latent_f32(a["sc"], _ref(WEIGHTS), A, None, None)),
    "pnr_folded_tables_bytes": ("size", lambda L, a: L.pnr_folded_tables_bytes(a["sc"])),
    "pnr_folded_tables_f32_bytes": ("size", lambda L, a: L.pnr_folded_tables_f32_bytes(a["sc"])),
    "pnr_fold_latent_f32_rows_workspace_bytes": ("size", lambda L, a: L.pnr_fold_latent_f32_rows_workspace_bytes(a["sc"])),
}
# the entries whose kernels index the feature grid (or a folded table of its size) with 32-bit element offsets
GRID_LIMITED = ["pnr_eval_ray_samples", "pnr_eval_ray_samples_folded", "pnr_eval_ray_samples_split", "pnr_eval_ray_samples_train",
                "pnr_eval_ray_samples_split_train", "pnr_fold_latent_f32_rows", "pnr_latent_scatter", "pnr_render_forward",
                "pnr_render_forward_folded", "pnr_render_forward_seeded", "pnr_render_views", "pnr_eval_points",
                "pnr_eval_points_folded", "pnr_eval_points_split"]


def args(sc, **kw):
    """a well-formed call on scene sc (SB objects): 2 rays / 8 points per object, 8 samples per ray; views of 2 x 1 pixels"""
    SB = sc.SB if sc is not None else 2
    a = dict(sc=_ref(sc) if sc is not None else None, R=2 * SB, n=2, K=8, rays=A, z=A, B=8, xyz=A, vd=A, NV=SB, W=2, H=1)
    a.update(kw)
    return a


SCENE_DEFECTS = {
    "null scene": (None, b"null argument"),
    "SB=0": (dict(SB=0), b"bad scene shape"),
    "NS=0": (dict(NS=0), b"bad scene shape"),
    "Hl=1": (dict(Hl=1), b"bad scene shape"),
    "Wl=1": (dict(Wl=1), b"bad scene shape"),
    "n_focal=2, SB=3": (dict(SB=3, n_focal=2), b"1 or SB rows"),
    "n_c=2, SB=3": (dict(SB=3, n_c=2), b"1 or SB rows"),
}
SIZES = (b"bad sizes", b"bad sample counts")
# defect -> (overrides of args(), message, the kinds it applies to); R = 2^20 rays x K = 2^11 samples (points: 2 x 2^30) are 2^31 points
SAMPLE_DEFECTS = {
    "R=-1": (dict(R=-1), SIZES, ("samples", "render", "size")),
    "K=0": (dict(K=0), SIZES, ("samples", "render", "views", "size")),
    "rays_per_obj=0": (dict(n=0), SIZES, ("samples", "render", "size")),
    "R != SB*rays_per_obj": (dict(R=6), (b"R != SB * rays_per_obj",), ("samples", "render", "size")),
    "null rays": (dict(rays=None), (b"null rays",), ("samples", "render")),
    "null z": (dict(z=None), (b"null rays/z",), ("samples",)),
    "2^31 points": (dict(R=1 << 20, n=1 << 19, K=1 << 11, B=1 << 30, NV=2, W=1 << 10, H=1 << 10), (b"too many points",),
                    ("samples", "render", "views", "points")),
    "B=-1": (dict(B=-1), SIZES, ("points",)),
    "null xyz": (dict(xyz=None), (b"null xyz/viewdirs",), ("points",)),
    "null viewdirs": (dict(vd=None), (b"null xyz/viewdirs",), ("points",)),
}


def refused(lib, name, a, reasons):
    kind, call = ENTRIES[name]
    rc = call(lib, a)
    if kind == "size":
        return rc == 0
    msg = lib.pnr_last_error()
    return rc == -1 and msg.startswith(name.encode() + b":") and any(r in msg for r in reasons)


def test_the_table_names_every_entry_that_takes_a_scene():
    takes_scene = sorted(n for n, (_, argtypes) in _lib.PROTOTYPES.items() if ctypes.POINTER(_lib.PnrScene) in argtypes)
    assert sorted(ENTRIES) == takes_scene
    assert set(GRID_LIMITED) <= set(ENTRIES)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_a_well_formed_call_is_not_refused_on_the_host(lib, name):
    kind, call = ENTRIES[name]
    rc = call(lib, args(make_scene()))
    if kind == "size":
        assert rc >= 0 and (rc > 0 or name == "pnr_latent_scatter_single_owner"), rc
    else:
        assert rc == -2, (rc, lib.pnr_last_error())  # reached a HIP call: no device here


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_a_defective_scene_is_refused_before_any_hip_call(lib, name):
    for defect, (fields, reason) in SCENE_DEFECTS.items():
        sc = None if fields is None else make_scene(**fields)
        assert refused(lib, name, args(sc), (reason,)), (defect, lib.pnr_last_error())


@pytest.mark.parametrize("name", sorted(n for n, (k, _) in ENTRIES.items() if k in ("samples", "render", "views", "points")) +
                         ["pnr_latent_scatter_workspace_bytes", "pnr_latent_scatter_single_owner"])
def test_defective_samples_are_refused_before_any_hip_call(lib, name):
    kind = ENTRIES[name][0]
    applied = 0
    for defect, (over, reasons, kinds) in SAMPLE_DEFECTS.items():
        if kind in kinds:
            assert refused(lib, name, args(make_scene(), **over), reasons), (defect, lib.pnr_last_error())
            applied += 1
    assert applied >= 2


@pytest.mark.parametrize("name", GRID_LIMITED)
def test_the_grid_limit_is_2_to_the_32_elements(lib, name):
    """one image of 2897 x 2897 texels x 512 channels is 4 297 015 808 elements, of 2896 x 2896 it is 4 294 049 792 < 2^32"""
    assert 2897 * 2897 * 512 > 2 ** 32 - 1 >= 2896 * 2896 * 512
    over = make_scene(SB=1, Hl=2897, Wl=2897)
    assert refused(lib, name, args(over), (b"feature grid too large",)), lib.pnr_last_error()
    fits = make_scene(SB=1, Hl=2896, Wl=2896)
    assert ENTRIES[name][1](lib, args(fits)) == -2, lib.pnr_last_error()


# pnr_latent_scatter_workspace_bytes / pnr_latent_scatter_single_owner of SB = 2, NS = 2, R = 2n, rays_per_obj = n, as the library
# answered before the three copies of the form decision became one plan (256 compute units: the count without a device, and the
# MI355X's own).  The last row has 2 x 4097 = 8194 tiles (> 8192): the global-atomic form, no workspace.
SCATTER_PINS = [
    ((16, 16, 24, 10), 24320, 0),
    ((40, 40, 24, 10), 24320, 0),
    ((50, 60, 24, 10), 39876, 1),
    ((64, 64, 24, 10), 39876, 1),
    ((72, 80, 24, 10), 40116, 1),
    ((16, 16, 600, 20), 580864, 0),
    ((32, 32, 128, 96), 590080, 0),
    ((150, 200, 64, 24), 182164, 1),
    ((33, 97, 200, 16), 373380, 1),
    ((300, 400, 8, 8), 29028, 1),
    ((64, 131104, 24, 10), 0, 0),
]


@pytest.mark.parametrize("shape,nbytes,single_owner", SCATTER_PINS)
def test_scatter_plan_pins(lib, shape, nbytes, single_owner):
    Hl, Wl, n, K = shape
    sc = make_scene(SB=2, NS=2, Hl=Hl, Wl=Wl)
    assert lib.pnr_latent_scatter_workspace_bytes(_ref(sc), 2 * n, n, K) == nbytes
    assert lib.pnr_latent_scatter_single_owner(_ref(sc), 2 * n, n, K) == single_owner
