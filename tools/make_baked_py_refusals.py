#!/usr/bin/env python
"""Every refusal of the Python front-end of the baked volumes, as it words it: exception type and str(exception) in full.

    python tools/make_baked_py_refusals.py            # the "cpu" section of tests/golden/baked_py_refusals.json
    python tools/make_baked_py_refusals.py --device   # its "device" section (needs a HIP device; launches no kernel), written
                                                      # against the "cpu" section that is there: record that one first

One layer above tools/make_baked_refusals.py: the calls go to the 26 public baked functions of pixelnerf_amd.ops (the 27th,
ops.baked_march, is younger than the fixture: `march_cases` holds it to the named function it must pick), to the five baked *_autograd functions
and to the util.bake methods that refuse.  Each call carries ONE defect, or one of a few pairs that pin the order of the checks, or
none: an all-valid call on CPU tensors ends in the PixelNerfHipError "no CPU path" that names the first tensor looked at.  The
"device" section repeats the calls that need no object of util.bake on HIP tensors with NO rays (R = 0) -- every call is refused,
or returns without a launch -- which reaches the checks behind the first device check.  With two devices visible it also records
the device-mismatch messages ("two devices" labels); with one they are absent from both sides of the comparison.
tests/test_baked_py_refusals_host.py and tests/test_hip_baked_py_refusals.py record the same calls with the checkout and compare
them with the fixture, which was written by this script at the commit before the front-end moved into ops_baked.py.

Coverage: the 69 `raise` statements of the baked front-end at that commit, in file order, and what reaches each
(cpu: a label of the "cpu" section; device: a label of the "device" section, behind the first device check; two: needs two devices).
 _baked_march_args   3 entries each ............ cpu  baked_render: reso has 2 entries
                     at least 2 points ......... cpu  baked_render: reso=(1, 2, 2)
                     c1 below c2 ............... cpu  baked_render: c1>=c2
                     step ...................... cpu  baked_render: step=0.0
                     terminate ................. cpu  baked_render: terminate=1.0
 _baked_volume       degree .................... cpu  baked_sh_render: degree=3
                     shape ..................... cpu  baked_sh_render: stored tail (3,)
                     coef spans ................ cpu  baked_sh_render: reso=(3, 2, 2)
                     index and bits mandatory .. cpu  baked_sparse_render: bits=None
                     16-byte aligned ........... device  baked_render: stored misaligned
                     index ..................... device  baked_sparse_render: index int64
 _image_size         at least one pixel ........ cpu  baked_render_views: W=0
 _baked_source       lives on .................. two  baked_render: two devices
 sparse_points       not a tensor .............. cpu  sparse_points: bits is a list
                     no CPU path ............... cpu  sparse_points: valid
                     reso 3 entries ............ device  sparse_points: reso has 2 entries
                     fewer than 2^31 points .... device, by reading (a bitfield of 268 MB)
 gen_grid_points_at  not a tensor .............. cpu  gen_grid_points_at: ids is a list
                     no CPU path ............... cpu  gen_grid_points_at: valid
                     1-d int32 ................. device  gen_grid_points_at: ids int64
                     3 entries each ............ device  gen_grid_points_at: c1 has 2 entries
 _baked_pose         (3,4) or (4,4) ............ cpu  baked_scene_render: pose (4, 3)
                     not finite ................ cpu  baked_scene_render: pose NaN
                     not rigid ................. cpu  baked_scene_render: pose scaled
 _baked_scene        list of 1 to 8 ............ cpu  baked_scene_render: objects is a dict
                     object j must be .......... cpu  baked_scene_render: object of 5
                     stored float32 or float16 . cpu  baked_scene_render: stored int32
                     differ in kind ............ cpu  baked_scene_render: kinds differ (dtype)
                     object j lives on ......... two  baked_scene_render: two devices (objects)
 _baked_scene_launch the volumes live on ....... two  baked_scene_render: two devices
 _baked_scene_backward   the volumes live on ... two  baked_scene_backward: two devices
                     d_* lives on .............. two  baked_scene_backward: two devices (d_rgb)
 _baked_scene_stored_backward  fp32 only ....... cpu  baked_scene_stored_backward: stored float16
                     no gradient w.r.t. rays ... cpu  baked_scene_stored_backward: source requires grad
                     the volumes live on ....... two  baked_scene_stored_backward: two devices
                     d_* lives on .............. two  baked_scene_stored_backward: two devices (d_rgb)
                     want one bool per object .. device  baked_scene_stored_backward: want of 3
                     out a list ................ device  baked_scene_stored_backward: out of 3
                     shares its stored tensor .. device  baked_scene_stored_backward: shared, two buffers
                     out[j] added into ......... device  baked_scene_stored_backward: out[0] shape
 _baked_backward     fp32 only ................. cpu  baked_render_backward: stored float16
                     no gradient w.r.t. rays ... cpu  baked_render_backward: source requires grad
                     d_* lives on .............. two  baked_render_backward: two devices (d_rgb)
                     out added into ............ device  baked_render_backward: out shape
 _baked_ray_backward d_* lives on .............. two  baked_ray_backward: two devices (d_rgb)
 _stored_tail        degree .................... cpu  baked_resample: degree=3
 _baked_visibility   out max-accumulated ....... cpu  baked_visibility: out shape
                     out lives on .............. device  baked_visibility: out on the host
 baked_resample      3 entries each ............ cpu  baked_resample: reso has 2 entries
                     at least 2 points ......... cpu  baked_resample: reso_dst=(1, 2, 2)
                     float32 or float16 ........ cpu  baked_resample: stored int32
                     shape ..................... cpu  baked_resample: stored tail (3,)
                     aligned ................... device  baked_resample: stored misaligned
                     index ..................... device  baked_resample: index int64
                     ids_dst ................... device  baked_resample: ids_dst int64
 baked_tv            fp32 only ................. cpu  baked_tv: stored float16
                     degree .................... cpu  baked_tv: degree=3
                     reso 3 entries ............ cpu  baked_tv: reso has 2 entries
                     at least 2 points ......... cpu  baked_tv: reso=(1, 2, 2)
                     index and ids together .... cpu  baked_tv: index without ids
                     shape ..................... cpu  baked_tv: stored tail (3,)
                     contiguous ................ cpu  baked_tv: stored not contiguous
                     weights ................... cpu  baked_tv: 3 weights
                     eps ....................... cpu  baked_tv: eps=0.0
                     16-byte aligned ........... device  baked_tv: stored misaligned
                     index ..................... device  baked_tv: index int64
                     ids ....................... device  baked_tv: ids of 2
                     grad_out added into ....... device  baked_tv: grad_out shape
                     scale ..................... device  baked_tv: scale float64
(The d_* shape and dtype refusals are ops._f32's, behind the first device check: device  baked_render_backward: d_rgb shape, ...)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "baked_py_refusals.json")

RESO, C1, C2, STEP = (2, 2, 2), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 0.5
FORWARD = ("baked_render", "baked_sh_render", "baked_sparse_render", "baked_half_render", "baked_sparse_half_render")
SINGLE = ("baked_render_backward", "baked_ray_backward", "baked_visibility")  # (head, stored, degree, reso, c1, c2, step, **kw)
SCENE = ("baked_scene_render", "baked_scene_backward", "baked_scene_stored_backward")  # (head, objects, step, **kw)
VIEWS = {"baked_render_backward": "baked_render_views_backward"}  # every other name: name + "_views"


def outcome(thunk):
    try:
        out = thunk()
    except Exception as e:  # noqa: BLE001 (the type is what is recorded)
        return [type(e).__name__, str(e)]
    shapes = [None if o is None else tuple(o.shape) for o in (out if isinstance(out, (tuple, list)) else (out,))]
    return ["", f"returned {shapes}"]


class Maker:
    """the tensors of the calls on `dev`: one ray on the host, none on a device (no call may launch)"""

    def __init__(self, dev):
        self.dev, self.on_device = torch.device(dev), torch.device(dev).type == "cuda"
        self.n = 0 if self.on_device else 1
        self.other = torch.device("cuda", 1) if self.on_device and torch.cuda.device_count() > 1 else None

    def z(self, *shape, dtype=torch.float32, dev=None):
        return torch.zeros(shape, dtype=dtype, device=dev or self.dev)

    def misaligned(self, *shape, dtype=torch.float32):
        numel = 1
        for s in shape:
            numel *= s
        return self.z(numel + 1, dtype=dtype)[1:].view(shape)

    def not_contiguous(self, *shape):
        return self.z(*shape[:-2], shape[-1], shape[-2]).transpose(-1, -2)

    def stored(self, degree=None, sparse=False, half=False, lead=None):
        tail = (4,) if degree in (None, -1) else ((degree + 1) ** 2, 4)
        return self.z(*(lead or ((3,) if sparse else RESO)), *tail, dtype=torch.float16 if half else torch.float32)

    def head(self, views, rays=None, W=1, H=1):
        if not views:
            return (self.z(self.n, 8) if rays is None else rays,)
        return (self.z(self.n, 4, 4) if rays is None else rays, W, H, 1.0, None, 0.5, 3.0)

    def pose(self):
        return torch.eye(4)


def forward_cases(mk, ops, name, views):
    sparse, half, takes_degree = "sparse" in name, "half" in name, name != "baked_render"
    good_degree = 1 if "_sh_" in name else None
    fn = getattr(ops, name + ("_views" if views else ""))

    def call(**d):
        a = dict(rays=None, W=1, H=1, degree=good_degree, reso=RESO, c1=C1, c2=C2, step=STEP, terminate=0.0,
                 bits=mk.z(1, dtype=torch.int32) if sparse else None, index=mk.z(*RESO, dtype=torch.int32))
        a.update(d)
        st = a["stored"] if "stored" in a else mk.stored(good_degree, sparse, half)
        vol = (st, a["degree"]) if takes_degree else (st,)
        if sparse:
            return fn(*mk.head(views, a["rays"], a["W"], a["H"]), *vol, a["index"], a["bits"], a["reso"], a["c1"], a["c2"], a["step"],
                      terminate=a["terminate"])
        return fn(*mk.head(views, a["rays"], a["W"], a["H"]), *vol, a["reso"], a["c1"], a["c2"], a["step"], bits=a["bits"],
                  terminate=a["terminate"])

    i32 = torch.int32
    out = [("valid", {}), ("reso has 2 entries", dict(reso=(2, 2))), ("reso=(1, 2, 2)", dict(reso=(1, 2, 2))), ("reso=(3, 2, 2)", dict(reso=(3, 2, 2))),
           ("c1>=c2", dict(c1=C2, c2=C1)), ("c1 NaN", dict(c1=(float("nan"), -1.0, -1.0))), ("c2 has 2 entries", dict(c2=(1.0, 1.0))),
           ("step=0.0", dict(step=0.0)), ("step=inf", dict(step=float("inf"))), ("terminate=1.0", dict(terminate=1.0)),
           ("terminate=-0.1", dict(terminate=-0.1)), ("stored is a list", dict(stored=[1.0])),
           ("stored tail (3,)", dict(stored=mk.z(*((3,) if sparse else RESO), *((4, 3) if good_degree else (3,))))),
           ("stored has one axis more", dict(stored=mk.z(*((3,) if sparse else RESO), 4, 4, 4))),
           ("step + terminate", dict(step=0.0, terminate=1.0)), ("reso + step", dict(reso=(1, 2, 2), step=0.0)),
           # behind the first device check
           ("stored of the other dtype", dict(stored=mk.stored(good_degree, sparse, not half))),
           ("stored misaligned", dict(stored=mk.misaligned(*((3,) if sparse else RESO), *((4, 4) if good_degree else (4,)),
                                                           dtype=torch.float16 if half else torch.float32))),
           ("bits int64", dict(bits=mk.z(1, dtype=torch.int64))), ("bits of 2", dict(bits=mk.z(2, dtype=i32))), ("bits is a list", dict(bits=[0])),
           ("bits on the host", dict(bits=torch.zeros(1, dtype=i32))),
           ("rays (n,7)" if not views else "poses (n,3,4)", dict(rays=mk.z(mk.n, 7) if not views else mk.z(mk.n, 3, 4))),
           ("source float64", dict(rays=mk.z(mk.n, 8, dtype=torch.float64) if not views else mk.z(mk.n, 4, 4, dtype=torch.float64))),
           ("source is a list", dict(rays=[0.0])), ("source on the host", dict(rays=torch.zeros(1, 8) if not views else torch.zeros(1, 4, 4))),
           ("stored misaligned + bits of 2", dict(stored=mk.misaligned(*((3,) if sparse else RESO), *((4, 4) if good_degree else (4,)),
                                                                       dtype=torch.float16 if half else torch.float32), bits=mk.z(2, dtype=i32))),
           ("bits of 2 + source is a list", dict(bits=mk.z(2, dtype=i32), rays=[0.0]))]
    if not sparse:
        out.append(("stored spans (3, 2, 2)", dict(stored=mk.stored(good_degree, False, half, lead=(3, 2, 2)))))
    if takes_degree:
        out += [("degree=3", dict(degree=3)), ("degree=-2", dict(degree=-2)), ("degree=-1", dict(degree=-1)), ("degree=None", dict(degree=None)),
                ("degree=0", dict(degree=0)), ("degree=3 + reso", dict(degree=3, reso=(1, 2, 2))), ("degree=3 + stored is a list", dict(degree=3, stored=[1.0]))]
    if sparse:
        out += [("bits=None", dict(bits=None)), ("index=None", dict(index=None)), ("index int64", dict(index=mk.z(*RESO, dtype=torch.int64))),
                ("index (2, 2, 3)", dict(index=mk.z(2, 2, 3, dtype=i32))), ("index is a list", dict(index=[0])),
                ("index on the host", dict(index=torch.zeros(RESO, dtype=i32))), ("bits=None + step", dict(bits=None, step=0.0)),
                ("bits of 2 + index int64", dict(bits=mk.z(2, dtype=i32), index=mk.z(*RESO, dtype=torch.int64)))]
    if views:
        out += [("W=0", dict(W=0)), ("H=-1", dict(H=-1)), ("W=0 + step", dict(W=0, step=0.0))]
        if takes_degree:
            out.append(("W=0 + degree=3", dict(W=0, degree=3)))
    if mk.other is not None:
        out.append(("two devices", dict(rays=mk.z(0, 8, dev=mk.other) if not views else mk.z(0, 4, 4, dev=mk.other))))
    return [(label, (lambda d=d: call(**d))) for label, d in out]


def single_cases(mk, ops, name, views):
    """the stored backward, the ray backward and visibility: (head, stored, degree, reso, c1, c2, step, **kw)"""
    fn = getattr(ops, VIEWS.get(name, name + "_views") if views else name)
    grads, has_out = name != "baked_visibility", name != "baked_ray_backward"
    n, i32 = mk.n, torch.int32

    def call(**d):
        a = dict(rays=None, W=1, H=1, stored=mk.stored(), degree=None, reso=RESO, c1=C1, c2=C2, step=STEP)
        a.update(d)
        kw = {k: v for k, v in a.items() if k not in ("rays", "W", "H", "stored", "degree", "reso", "c1", "c2", "step")}
        return fn(*mk.head(views, a["rays"], a["W"], a["H"]), a["stored"], a["degree"], a["reso"], a["c1"], a["c2"], a["step"], **kw)

    source = (lambda: mk.z(n, 4, 4)) if views else (lambda: mk.z(n, 8))
    sparse = dict(stored=mk.stored(None, True), bits=mk.z(1, dtype=i32), index=mk.z(*RESO, dtype=i32))
    out = [("valid", {}), ("valid, sparse at degree 1", dict(sparse, stored=mk.stored(1, True), degree=1)),
           ("valid, degree=-1", dict(degree=-1)), ("stored float16", dict(stored=mk.stored(half=True))),
           ("source requires grad", dict(rays=source().requires_grad_())), ("degree=3", dict(degree=3)), ("degree=-2", dict(degree=-2)),
           ("stored is a list", dict(stored=[1.0])), ("stored tail (3,)", dict(stored=mk.z(*RESO, 3))),
           ("rows tail (3,)", dict(sparse, stored=mk.z(3, 3))), ("reso has 2 entries", dict(reso=(2, 2))), ("reso=(1, 2, 2)", dict(reso=(1, 2, 2))),
           ("c1>=c2", dict(c1=C2, c2=C1)), ("step=0.0", dict(step=0.0)), ("terminate=1.0", dict(terminate=1.0)),
           ("bits=None with an index", dict(sparse, bits=None)), ("degree=3 + step", dict(degree=3, step=0.0)),
           ("source requires grad + degree=3", dict(rays=source().requires_grad_(), degree=3)),
           ("stored float16 + source requires grad", dict(stored=mk.stored(half=True), rays=source().requires_grad_())),
           # behind the first device check
           ("stored int32", dict(stored=mk.z(*RESO, 4, dtype=i32))), ("stored spans (3, 2, 2)", dict(stored=mk.stored(lead=(3, 2, 2)))),
           ("stored misaligned", dict(stored=mk.misaligned(*RESO, 4))), ("bits of 2", dict(bits=mk.z(2, dtype=i32))),
           ("index int64", dict(sparse, index=mk.z(*RESO, dtype=torch.int64))), ("index (2, 2, 3)", dict(sparse, index=mk.z(2, 2, 3, dtype=i32))),
           ("source (n,7)", dict(rays=mk.z(n, 3, 4) if views else mk.z(n, 7))), ("source is a list", dict(rays=[0.0])),
           ("source on the host", dict(rays=torch.zeros(1, 4, 4) if views else torch.zeros(1, 8))),
           ("stored misaligned + source is a list", dict(stored=mk.misaligned(*RESO, 4), rays=[0.0]))]
    if views:
        out += [("W=0", dict(W=0)), ("W=0 + stored float16", dict(W=0, stored=mk.stored(half=True)))]
    if grads:
        out += [("d_rgb shape", dict(d_rgb=mk.z(n + 1, 3))), ("d_rgb (n,4)", dict(d_rgb=mk.z(n, 4))), ("d_rgb float64", dict(d_rgb=mk.z(n, 3, dtype=torch.float64))),
                ("d_rgb is a list", dict(d_rgb=[0.0])), ("d_depth shape", dict(d_depth=mk.z(n, 1))), ("d_depth float16", dict(d_depth=mk.z(n, dtype=torch.float16))),
                ("d_alpha shape", dict(d_alpha=mk.z(n + 2))), ("d_alpha int32", dict(d_alpha=mk.z(n, dtype=i32))),
                ("d_alpha on the host", dict(d_alpha=torch.zeros(n))), ("valid, every d_*", dict(d_rgb=mk.z(n, 3).requires_grad_(), d_depth=mk.z(n), d_alpha=mk.z(n))),
                ("source is a list + d_rgb shape", dict(rays=[0.0], d_rgb=mk.z(n + 1, 3))), ("d_rgb shape + d_depth shape", dict(d_rgb=mk.z(n + 1, 3), d_depth=mk.z(n, 1)))]
    if has_out:
        shape, rows = (RESO + (4,), (3, 4)) if grads else (RESO, (3,))
        out += [("valid, out given", dict(out=mk.z(*shape))), ("out shape", dict(out=mk.z(3, *shape[1:]))), ("out not contiguous", dict(out=mk.not_contiguous(*shape))),
                ("out float64", dict(out=mk.z(*shape, dtype=torch.float64))), ("out requires grad", dict(out=mk.z(*shape).requires_grad_())),
                ("out is a list", dict(out=[0.0])), ("out on the host", dict(out=torch.zeros(shape))),
                ("out shape, sparse", dict(sparse, out=mk.z(*shape))), ("valid, sparse, out given", dict(sparse, out=mk.z(*rows))),
                ("out shape + degree=3", dict(out=mk.z(3, *shape[1:]), degree=3)), ("out shape + source is a list", dict(out=mk.z(3, *shape[1:]), rays=[0.0]))]
        if grads:
            out.append(("d_rgb shape + out shape", dict(d_rgb=mk.z(n + 1, 3), out=mk.z(3, *shape[1:]))))
    if mk.other is not None:
        out.append(("two devices", dict(rays=mk.z(0, 4, 4, dev=mk.other) if views else mk.z(0, 8, dev=mk.other))))
        if grads:
            out.append(("two devices (d_rgb)", dict(d_rgb=mk.z(0, 3, dev=mk.other))))
        if has_out:
            out.append(("two devices (out)", dict(out=mk.z(*(RESO + (4,) if grads else RESO), dev=mk.other))))
    return [(label, (lambda d=d: call(**d))) for label, d in out]


def scene_cases(mk, ops, name, views):
    fn = getattr(ops, name + ("_views" if views else ""))
    grads, fit = name != "baked_scene_render", name == "baked_scene_stored_backward"
    n, i32 = mk.n, torch.int32

    def ob(stored=None, degree=None, reso=RESO, c1=C1, c2=C2, pose=None, *rest):
        return (mk.stored(degree) if stored is None else stored, degree, reso, c1, c2, mk.pose() if pose is None else pose) + rest

    def call(objects=None, rays=None, W=1, H=1, step=STEP, **kw):
        if fit and "want_poses" in kw:
            kw.pop("want_poses")
        return fn(*mk.head(views, rays, W, H), [ob(), ob()] if objects is None else objects, step, **kw)

    nan_pose, scaled = torch.eye(4), torch.eye(4) * 2.0
    nan_pose[0, 3] = float("nan")
    source = (lambda: mk.z(n, 4, 4)) if views else (lambda: mk.z(n, 8))
    rows = lambda: ob(mk.stored(None, True), None, RESO, C1, C2, None, mk.z(1, dtype=i32), mk.z(*RESO, dtype=i32))
    quiet = dict(want_poses=False) if grads and not fit else {}  # (the pose reduction of an all-valid call would be a launch)
    out = [("valid", dict(quiet)), ("valid, sparse", dict(quiet, objects=[rows()])), ("objects is a dict", dict(objects={})), ("no objects", dict(objects=[])),
           ("9 objects", dict(objects=[ob()] * 9)), ("object of 5", dict(objects=[ob()[:5]])), ("object is a tensor", dict(objects=[mk.stored()])),
           ("stored int32", dict(objects=[ob(mk.z(*RESO, 4, dtype=i32))])), ("stored is a list", dict(objects=[ob([1.0])])),
           ("pose (4, 3)", dict(objects=[ob(pose=torch.zeros(4, 3))])), ("pose NaN", dict(objects=[ob(pose=nan_pose)])),
           ("pose scaled", dict(objects=[ob(), ob(pose=scaled)])), ("kinds differ (degree)", dict(objects=[ob(), ob(degree=0)])),
           ("kinds differ (dtype)", dict(objects=[ob(), ob(mk.stored(half=True))])), ("kinds differ (layout)", dict(objects=[ob(), rows()])),
           ("degree=3", dict(objects=[ob(), ob(mk.stored(), 3), ob(mk.stored(), 3)])), ("stored tail (3,)", dict(objects=[ob(mk.z(*RESO, 3))])),
           ("reso=(1, 2, 2) of object 1", dict(objects=[ob(), ob(reso=(1, 2, 2))])), ("c1>=c2", dict(objects=[ob(c1=C2, c2=C1)])),
           ("step=0.0", dict(step=0.0)), ("terminate=1.0", dict(terminate=1.0)),
           ("rows without bits", dict(objects=[ob(mk.stored(None, True), None, RESO, C1, C2, None, None, mk.z(*RESO, dtype=i32))])),
           ("pose scaled of object 1 + degree=3 of object 0", dict(objects=[ob(mk.stored(), 3), ob(mk.stored(), 3, pose=scaled)])),
           ("degree=3 of object 0 + step", dict(objects=[ob(mk.stored(), 3)], step=0.0)),
           # behind the first device check
           ("stored misaligned", dict(objects=[ob(mk.misaligned(*RESO, 4))])), ("stored spans (3, 2, 2)", dict(objects=[ob(mk.stored(lead=(3, 2, 2)))])),
           ("bits of 2", dict(objects=[ob(None, None, RESO, C1, C2, None, mk.z(2, dtype=i32))])),
           ("source (n,7)", dict(rays=mk.z(n, 3, 4) if views else mk.z(n, 7))), ("source is a list", dict(rays=[0.0])),
           ("source on the host", dict(rays=torch.zeros(1, 4, 4) if views else torch.zeros(1, 8))),
           ("stored misaligned + source is a list", dict(objects=[ob(mk.misaligned(*RESO, 4))], rays=[0.0]))]
    if views:
        out += [("W=0", dict(W=0)), ("W=0 + objects is a dict", dict(W=0, objects={}))]
    if grads:
        out += [("d_rgb shape", dict(d_rgb=mk.z(n + 1, 3))), ("d_rgb float64", dict(d_rgb=mk.z(n, 3, dtype=torch.float64))), ("d_rgb is a list", dict(d_rgb=[0.0])),
                ("d_depth shape", dict(d_depth=mk.z(n, 1))), ("d_alpha shape", dict(d_alpha=mk.z(n + 2))), ("d_alpha on the host", dict(d_alpha=torch.zeros(n))),
                ("valid, every d_*", dict(quiet, d_rgb=mk.z(n, 3).requires_grad_(), d_depth=mk.z(n), d_alpha=mk.z(n))),
                ("source is a list + d_rgb shape", dict(rays=[0.0], d_rgb=mk.z(n + 1, 3))), ("d_rgb shape + d_depth shape", dict(d_rgb=mk.z(n + 1, 3), d_depth=mk.z(n, 1)))]
    if fit:
        S = mk.stored()
        twice = [ob(S), ob(S)]
        buf = lambda *lead: mk.z(*(lead or RESO), 4)
        out += [("stored float16", dict(objects=[ob(), ob(mk.stored(half=True))])), ("source requires grad", dict(rays=source().requires_grad_())),
                ("stored float16 + source requires grad", dict(objects=[ob(mk.stored(half=True))], rays=source().requires_grad_())),
                ("source requires grad + objects is a dict", dict(objects={}, rays=source().requires_grad_())),
                ("want of 3", dict(want=[True] * 3)), ("out of 3", dict(out=[None] * 3)), ("out is a tensor", dict(out=buf())),
                ("want of 3 + out of 3", dict(want=[True] * 3, out=[None] * 3)), ("d_rgb shape + want of 3", dict(d_rgb=mk.z(n + 1, 3), want=[True] * 3)),
                ("out[0] shape", dict(out=[buf(3, 2, 2), None])), ("out[1] not contiguous", dict(out=[None, mk.not_contiguous(*RESO, 4)])),
                ("out[0] float64", dict(out=[mk.z(*RESO, 4, dtype=torch.float64), None])), ("out[1] requires grad", dict(out=[None, buf().requires_grad_()])),
                ("out[0] is a list", dict(out=[[0.0], None])), ("out[0] on the host", dict(out=[torch.zeros(RESO + (4,)), None])),
                ("out[0] shape, frozen", dict(out=[buf(3, 2, 2), None], want=[False, True])), ("valid, out given", dict(out=[buf(), buf()])),
                ("valid, frozen", dict(want=[False, False])), ("shared, two buffers", dict(objects=twice, out=[buf(), buf()])),
                ("valid, shared, one buffer", dict(objects=twice, out=[None, None])), ("out of 3 + out[0] shape", dict(out=[buf(3, 2, 2)] * 3))]
    if mk.other is not None:
        out += [("two devices", dict(rays=mk.z(0, 4, 4, dev=mk.other) if views else mk.z(0, 8, dev=mk.other))),
                ("two devices (objects)", dict(objects=[ob(), ob(mk.z(*RESO, 4, dev=mk.other))]))]
        if grads:
            out.append(("two devices (d_rgb)", dict(d_rgb=mk.z(0, 3, dev=mk.other))))
    return [(label, (lambda d=d: call(**d))) for label, d in out]


def grid_cases(mk, ops):
    """sparse_points, gen_grid_points_at, baked_resample, baked_tv: no rays.  On a device an all-valid call would launch: left out"""
    i32, i64 = torch.int32, torch.int64
    host = not mk.on_device
    sp, gp, rs, tv = ops.sparse_points, ops.gen_grid_points_at, ops.baked_resample, ops.baked_tv
    bits, ids, index = mk.z(1, dtype=i32), mk.z(3, dtype=i32), mk.z(*RESO, dtype=i32)
    out = [("sparse_points: bits is a list", lambda: sp([0], RESO)), ("sparse_points: bits on the host", lambda: sp(torch.zeros(1, dtype=i32), RESO)),
           ("sparse_points: reso has 2 entries", lambda: sp(bits, (2, 2))), ("sparse_points: reso=(1, 2, 2)", lambda: sp(bits, (1, 2, 2))),
           ("sparse_points: bits of 2", lambda: sp(mk.z(2, dtype=i32), RESO)), ("sparse_points: bits int64", lambda: sp(mk.z(1, dtype=i64), RESO)),
           ("gen_grid_points_at: ids is a list", lambda: gp(C1, C2, RESO, [0])), ("gen_grid_points_at: ids on the host", lambda: gp(C1, C2, RESO, torch.zeros(3, dtype=i32))),
           ("gen_grid_points_at: ids int64", lambda: gp(C1, C2, RESO, mk.z(3, dtype=i64))), ("gen_grid_points_at: ids (3, 1)", lambda: gp(C1, C2, RESO, mk.z(3, 1, dtype=i32))),
           ("gen_grid_points_at: c1 has 2 entries", lambda: gp(C1[:2], C2, RESO, ids)),
           ("gen_grid_points_at: ids int64 + c1 has 2 entries", lambda: gp(C1[:2], C2, RESO, mk.z(3, dtype=i64)))]
    if host:
        out += [("sparse_points: valid", lambda: sp(bits, RESO)), ("gen_grid_points_at: valid", lambda: gp(C1, C2, RESO, ids))]

    st = mk.stored
    none = mk.z(0, dtype=i32)  # ids_dst of no rows: an all-valid call that launches nothing
    out += [("baked_resample: valid, no rows asked", lambda: rs(st(), None, RESO, (3, 3, 3), ids_dst=none)),
            ("baked_resample: valid, sparse float16 at degree 1", lambda: rs(st(1, True, True), 1, RESO, (3, 3, 3), index=index, ids_dst=none)),
            ("baked_resample: degree=3", lambda: rs(st(), 3, RESO, (3, 3, 3))), ("baked_resample: reso has 2 entries", lambda: rs(st(), None, (2, 2), (3, 3, 3))),
            ("baked_resample: reso_dst has 2 entries", lambda: rs(st(), None, RESO, (3, 3))), ("baked_resample: reso=(1, 2, 2)", lambda: rs(st(), None, (1, 2, 2), (3, 3, 3))),
            ("baked_resample: reso_dst=(1, 2, 2)", lambda: rs(st(), None, RESO, (1, 2, 2))), ("baked_resample: stored is a list", lambda: rs([1.0], None, RESO, (3, 3, 3))),
            ("baked_resample: stored int32", lambda: rs(mk.z(*RESO, 4, dtype=i32), None, RESO, (3, 3, 3))),
            ("baked_resample: stored tail (3,)", lambda: rs(mk.z(*RESO, 3), None, RESO, (3, 3, 3))),
            ("baked_resample: stored spans (3, 2, 2)", lambda: rs(st(lead=(3, 2, 2)), None, RESO, (3, 3, 3))),
            ("baked_resample: rows at degree 1 against degree 0", lambda: rs(st(1, True), 0, RESO, (3, 3, 3), index=index)),
            ("baked_resample: degree=3 + reso has 2 entries", lambda: rs(st(), 3, (2, 2), (3, 3, 3))),
            ("baked_resample: reso + stored int32", lambda: rs(mk.z(*RESO, 4, dtype=i32), None, (1, 2, 2), (3, 3, 3))),
            ("baked_resample: stored misaligned", lambda: rs(mk.misaligned(*RESO, 4), None, RESO, (3, 3, 3))),
            ("baked_resample: stored misaligned, float16", lambda: rs(mk.misaligned(*RESO, 4, dtype=torch.float16), None, RESO, (3, 3, 3))),
            ("baked_resample: index int64", lambda: rs(st(None, True), None, RESO, (3, 3, 3), index=mk.z(*RESO, dtype=i64))),
            ("baked_resample: index (2, 2, 3)", lambda: rs(st(None, True), None, RESO, (3, 3, 3), index=mk.z(2, 2, 3, dtype=i32))),
            ("baked_resample: index on the host", lambda: rs(st(None, True), None, RESO, (3, 3, 3), index=torch.zeros(RESO, dtype=i32))),
            ("baked_resample: ids_dst int64", lambda: rs(st(), None, RESO, (3, 3, 3), ids_dst=mk.z(0, dtype=i64))),
            ("baked_resample: ids_dst (0, 1)", lambda: rs(st(), None, RESO, (3, 3, 3), ids_dst=mk.z(0, 1, dtype=i32))),
            ("baked_resample: ids_dst is a list", lambda: rs(st(), None, RESO, (3, 3, 3), ids_dst=[0])),
            ("baked_resample: stored misaligned + index int64", lambda: rs(mk.misaligned(3, 4), None, RESO, (3, 3, 3), index=mk.z(*RESO, dtype=i64))),
            ("baked_resample: index int64 + ids_dst int64", lambda: rs(st(None, True), None, RESO, (3, 3, 3), index=mk.z(*RESO, dtype=i64), ids_dst=mk.z(0, dtype=i64)))]

    w4, quiet = [1.0] * 4, dict(want_value=False)  # (no value and no gradient asked: nothing is launched)
    sparse = lambda **kw: tv(st(None, True), None, RESO, w4, **dict(dict(quiet, index=index, ids=ids), **kw))
    dense = lambda **kw: tv(st(), None, RESO, w4, **dict(quiet, **kw))
    out += [("baked_tv: valid, nothing asked", lambda: dense()), ("baked_tv: valid, sparse, nothing asked", lambda: sparse()),
            ("baked_tv: stored float16", lambda: tv(st(half=True), None, RESO, w4)), ("baked_tv: degree=3", lambda: tv(st(), 3, RESO, w4)),
            ("baked_tv: reso has 2 entries", lambda: tv(st(), None, (2, 2), w4)), ("baked_tv: reso=(1, 2, 2)", lambda: tv(st(), None, (1, 2, 2), w4)),
            ("baked_tv: index without ids", lambda: tv(st(None, True), None, RESO, w4, index=index)), ("baked_tv: ids without index", lambda: tv(st(None, True), None, RESO, w4, ids=ids)),
            ("baked_tv: stored is a list", lambda: tv([1.0], None, RESO, w4)), ("baked_tv: stored tail (3,)", lambda: tv(mk.z(*RESO, 3), None, RESO, w4)),
            ("baked_tv: stored spans (3, 2, 2)", lambda: tv(st(lead=(3, 2, 2)), None, RESO, w4)), ("baked_tv: stored not contiguous", lambda: tv(mk.not_contiguous(2, 2, 2, 4), None, (2, 2, 4), w4)),
            ("baked_tv: 3 weights", lambda: tv(st(), None, RESO, [1.0] * 3)), ("baked_tv: a negative weight", lambda: tv(st(), None, RESO, [1.0, 1.0, -1.0, 1.0])),
            ("baked_tv: 16 weights as a tensor at degree 1", lambda: tv(st(1), 1, RESO, torch.ones(4, 4), **quiet)), ("baked_tv: a weight NaN", lambda: tv(st(), None, RESO, [float("nan")] * 4)),
            ("baked_tv: eps=0.0", lambda: tv(st(), None, RESO, w4, eps=0.0)), ("baked_tv: eps=inf", lambda: tv(st(), None, RESO, w4, eps=float("inf"))),
            ("baked_tv: stored float16 + degree=3", lambda: tv(st(half=True), 3, RESO, w4)), ("baked_tv: degree=3 + reso", lambda: tv(st(), 3, (2, 2), w4)),
            ("baked_tv: stored not contiguous + 3 weights", lambda: tv(mk.not_contiguous(2, 2, 2, 4), None, (2, 2, 4), [1.0] * 3)),
            ("baked_tv: 3 weights + eps=0.0", lambda: tv(st(), None, RESO, [1.0] * 3, eps=0.0)),
            ("baked_tv: stored misaligned", lambda: tv(mk.misaligned(*RESO, 4), None, RESO, w4, **quiet)),
            ("baked_tv: index int64", lambda: sparse(index=mk.z(*RESO, dtype=i64))), ("baked_tv: index (2, 2, 3)", lambda: sparse(index=mk.z(2, 2, 3, dtype=i32))),
            ("baked_tv: index on the host", lambda: sparse(index=torch.zeros(RESO, dtype=i32))), ("baked_tv: ids of 2", lambda: sparse(ids=mk.z(2, dtype=i32))),
            ("baked_tv: ids int64", lambda: sparse(ids=mk.z(3, dtype=i64))), ("baked_tv: index int64 + ids of 2", lambda: sparse(index=mk.z(*RESO, dtype=i64), ids=mk.z(2, dtype=i32))),
            ("baked_tv: grad_out shape", lambda: dense(grad_out=mk.z(3, 2, 2, 4))), ("baked_tv: grad_out not contiguous", lambda: dense(grad_out=mk.not_contiguous(*RESO, 4))),
            ("baked_tv: grad_out float64", lambda: dense(grad_out=mk.z(*RESO, 4, dtype=torch.float64))), ("baked_tv: grad_out requires grad", lambda: dense(grad_out=mk.z(*RESO, 4).requires_grad_())),
            ("baked_tv: grad_out is a list", lambda: dense(grad_out=[0.0])), ("baked_tv: grad_out on the host", lambda: dense(grad_out=torch.zeros(RESO + (4,)))),
            ("baked_tv: ids of 2 + grad_out shape", lambda: sparse(ids=mk.z(2, dtype=i32), grad_out=mk.z(4, 4))),
            ("baked_tv: scale float64", lambda: dense(scale=mk.z(1, dtype=torch.float64))), ("baked_tv: scale of 2", lambda: dense(scale=mk.z(2))),
            ("baked_tv: scale on the host", lambda: dense(scale=torch.zeros(1))), ("baked_tv: valid, scale a number", lambda: dense(scale=2.0)),
            ("baked_tv: valid, scale a 0-dim tensor that requires grad", lambda: dense(scale=mk.z().requires_grad_())),
            ("baked_tv: grad_out shape + scale of 2", lambda: dense(grad_out=mk.z(3, 2, 2, 4), scale=mk.z(2)))]
    if mk.other is not None:
        out += [("baked_tv: two devices (grad_out)", lambda: dense(grad_out=mk.z(*RESO, 4, dev=mk.other))), ("baked_tv: two devices (scale)", lambda: dense(scale=mk.z(1, dev=mk.other))),
                ("baked_resample: two devices (index)", lambda: rs(st(None, True), None, RESO, (3, 3, 3), index=mk.z(*RESO, dtype=i32, dev=mk.other)))]
    return out


def autograd_cases(mk, autograd):
    """the five baked *_autograd functions.  A forward without rays launches nothing; no backward is run"""
    n, i32 = mk.n, torch.int32
    rays, cam = (mk.z(n, 8),), (mk.z(n, 4, 4), 1, 1, 1.0, None, 0.5, 3.0)
    geo = (RESO, C1, C2, STEP)
    sparse = dict(bits=mk.z(1, dtype=i32), index=mk.z(*RESO, dtype=i32))
    march, march_rays, tv = autograd.baked_march_autograd, autograd.baked_march_rays_autograd, autograd.baked_tv_autograd
    scene, fit = autograd.baked_scene_march_autograd, autograd.baked_scene_fit_autograd
    vol = lambda stored=None, degree=None: (mk.stored(degree) if stored is None else stored, degree, RESO, C1, C2, None, None)
    meta = (None, RESO, C1, C2, None, None)
    eye = torch.eye(4)[:3].expand(2, 3, 4).contiguous()
    out = []
    for name, fn in (("baked_march_autograd", march), ("baked_march_rays_autograd", march_rays)):
        for kind, source in (("rays", rays), ("camera", cam)):
            out += [(f"{name}: valid, {kind}", lambda fn=fn, source=source: fn(mk.stored(), source, None, *geo)),
                    (f"{name}: valid, {kind}, degree 1", lambda fn=fn, source=source: fn(mk.stored(1), source, 1, *geo)),
                    (f"{name}: valid, {kind}, degree -1", lambda fn=fn, source=source: fn(mk.stored(), source, -1, *geo)),
                    (f"{name}: valid, {kind}, sparse", lambda fn=fn, source=source: fn(mk.stored(None, True), source, None, *geo, **sparse)),
                    (f"{name}: valid, {kind}, sparse at degree 0", lambda fn=fn, source=source: fn(mk.stored(0, True), source, 0, *geo, **sparse)),
                    (f"{name}: {kind}, degree=3", lambda fn=fn, source=source: fn(mk.stored(), source, 3, *geo)),
                    (f"{name}: {kind}, stored float16", lambda fn=fn, source=source: fn(mk.stored(half=True), source, None, *geo)),
                    (f"{name}: {kind}, sparse float16 at degree 1", lambda fn=fn, source=source: fn(mk.stored(1, True, True), source, 1, *geo, **sparse)),
                    (f"{name}: {kind}, float16 at degree 2", lambda fn=fn, source=source: fn(mk.stored(2, half=True), source, 2, *geo))]
        out += [(f"{name}: stored is a list", lambda fn=fn: fn([1.0], rays, None, *geo)), (f"{name}: stored int32", lambda fn=fn: fn(mk.z(*RESO, 4, dtype=i32), rays, None, *geo)),
                (f"{name}: rays require grad", lambda fn=fn: fn(mk.stored(), (mk.z(n, 8).requires_grad_(),), None, *geo)),
                (f"{name}: poses require grad", lambda fn=fn: fn(mk.stored(), (mk.z(n, 4, 4).requires_grad_(),) + cam[1:], None, *geo)),
                (f"{name}: source[0] is a list", lambda fn=fn: fn(mk.stored(), ([0.0],), None, *geo)),
                (f"{name}: float16 that requires grad", lambda fn=fn: fn(mk.stored(half=True).requires_grad_(), rays, None, *geo)),
                (f"{name}: float16 that requires grad + source[0] is a list", lambda fn=fn: fn(mk.stored(half=True).requires_grad_(), ([0.0],), None, *geo))]
        if fn is march_rays:  # (baked_march_autograd has no check of its own: a source of another length is Python's TypeError)
            out.append((f"{name}: source of 2", lambda fn=fn: fn(mk.stored(), (mk.z(n, 8), 1), None, *geo)))
    for name, fn, objs in (("baked_scene_march_autograd", scene, lambda: [vol(), vol()]), ("baked_scene_fit_autograd", fit, None)):
        call = (lambda source, poses, fn=fn, objs=objs: fn(source, objs(), poses, STEP)) if objs else \
            (lambda source, poses, fn=fn: fn(source, [mk.stored(), mk.stored()], [meta, meta], poses, STEP))
        out += [(f"{name}: valid, rays", lambda call=call: call(rays, eye)), (f"{name}: valid, camera", lambda call=call: call(cam, eye)),
                (f"{name}: valid, poses on the device in float64", lambda call=call: call(rays, eye.to(mk.dev, torch.float64))),
                (f"{name}: source of 2", lambda call=call: call((mk.z(n, 8), 1), eye)), (f"{name}: source[0] is a list", lambda call=call: call(([0.0],), eye)),
                (f"{name}: obj_poses (2,4,4)", lambda call=call: call(rays, torch.eye(4).expand(2, 4, 4))), (f"{name}: obj_poses of 3", lambda call=call: call(rays, torch.eye(4)[:3].expand(3, 3, 4))),
                (f"{name}: obj_poses int64", lambda call=call: call(rays, eye.long())), (f"{name}: obj_poses is a list", lambda call=call: call(rays, [0.0])),
                (f"{name}: obj_poses scaled", lambda call=call: call(rays, eye * 2.0)), (f"{name}: source of 2 + obj_poses of 3", lambda call=call: call((mk.z(n, 8), 1), torch.eye(4)[:3].expand(3, 3, 4)))]
    out += [("baked_scene_march_autograd: object of 6", lambda: scene(rays, [vol()[:6], vol()[:6]], eye, STEP)),
            ("baked_scene_march_autograd: obj_poses of 3 + object of 6", lambda: scene(rays, [vol()[:6], vol()[:6]], torch.eye(4)[:3].expand(3, 3, 4), STEP)),
            ("baked_scene_march_autograd: degree=3", lambda: scene(rays, [vol(None, 3), vol(None, 3)], eye, STEP)),
            ("baked_scene_fit_autograd: no stored", lambda: fit(rays, [], [], eye[:0], STEP)), ("baked_scene_fit_autograd: 2 stored, 1 meta", lambda: fit(rays, [mk.stored(), mk.stored()], [meta], eye, STEP)),
            ("baked_scene_fit_autograd: meta of 5", lambda: fit(rays, [mk.stored()], [meta[:5]], eye[:1], STEP)),
            ("baked_scene_fit_autograd: stored float16", lambda: fit(rays, [mk.stored(), mk.stored(half=True)], [meta, meta], eye, STEP)),
            ("baked_scene_fit_autograd: stored is a list", lambda: fit(rays, [[1.0]], [meta], eye[:1], STEP)),
            ("baked_scene_fit_autograd: meta of 5 + stored float16", lambda: fit(rays, [mk.stored(half=True)], [meta[:5]], eye[:1], STEP)),
            ("baked_scene_fit_autograd: stored float16 + obj_poses of 3", lambda: fit(rays, [mk.stored(half=True)], [meta], eye, STEP)),
            ("baked_scene_fit_autograd: valid, one tensor listed twice", lambda: (lambda s: fit(rays, [s, s], [meta, meta], eye, STEP))(mk.stored().requires_grad_())),
            ("baked_tv_autograd: stored float16", lambda: tv(mk.stored(half=True), None, RESO, [1.0] * 4)), ("baked_tv_autograd: stored is a list", lambda: tv([1.0], None, RESO, [1.0] * 4)),
            ("baked_tv_autograd: degree=3", lambda: tv(mk.stored(), 3, RESO, [1.0] * 4)), ("baked_tv_autograd: 3 weights", lambda: tv(mk.stored(), None, RESO, [1.0] * 3))]
    if not mk.on_device:
        out.append(("baked_tv_autograd: valid", lambda: tv(mk.stored(), None, RESO, [1.0] * 4)))
    return out


def bake_cases():
    """util.bake, on the host alone (a volume on a device builds its skip grid: launches).  The volumes are stood up without
    their constructors, which refuse a host tensor -- that refusal is the first call recorded"""
    import types
    from pixelnerf_amd.util import bake
    i32 = torch.int32
    occ = types.SimpleNamespace(bits=torch.zeros(1, dtype=i32), reso=RESO, c1=C1, c2=C2)

    def stand_up(cls, stored, degree=None):
        v = object.__new__(cls)
        setattr(v, cls._stored_name, stored)
        v.reso, v.c1, v.c2, v.skip_threshold, v.occupancy = RESO, C1, C2, 0.0, occ
        if cls is not bake.BakedVolume:
            v.degree = degree
        if cls is bake.SparseBakedVolume:
            v.index, v.ids = torch.zeros(RESO, dtype=i32), torch.zeros(3, dtype=i32)
        return v

    z = torch.zeros
    kinds = {"BakedVolume": stand_up(bake.BakedVolume, z(2, 2, 2, 4)), "BakedVolume, float16": stand_up(bake.BakedVolume, z(2, 2, 2, 4).half()),
             "BakedSHVolume": stand_up(bake.BakedSHVolume, z(2, 2, 2, 4, 4), 1), "BakedSHVolume, float16": stand_up(bake.BakedSHVolume, z(2, 2, 2, 4, 4).half(), 1),
             "SparseBakedVolume": stand_up(bake.SparseBakedVolume, z(3, 4)), "SparseBakedVolume at degree 1": stand_up(bake.SparseBakedVolume, z(3, 4, 4), 1),
             "SparseBakedVolume, float16": stand_up(bake.SparseBakedVolume, z(3, 4).half()),
             "SparseBakedVolume, float16 at degree 0": stand_up(bake.SparseBakedVolume, z(3, 1, 4).half(), 0)}
    rays, poses, cam = z(1, 8), z(1, 4, 4), (1, 1, 1.0, 0.5, 3.0)
    out = [("BakedVolume: on the host", lambda: bake.BakedVolume(z(2, 2, 2, 4), C1, C2)), ("BakedSHVolume: on the host", lambda: bake.BakedSHVolume(z(2, 2, 2, 4, 4), C1, C2))]
    for kind, v in kinds.items():
        out += [(f"{kind}.render: valid", lambda v=v: v.render(rays)), (f"{kind}.render_views: valid", lambda v=v: v.render_views(poses, *cam)),
                (f"{kind}.render_diff: valid", lambda v=v: v.render_diff(rays)), (f"{kind}.render_views_diff: valid", lambda v=v: v.render_views_diff(poses, *cam)),
                (f"{kind}.visibility: valid", lambda v=v: v.visibility(rays)), (f"{kind}.visibility_views: valid", lambda v=v: v.visibility_views(poses, *cam)),
                (f"{kind}.tv", lambda v=v: v.tv()), (f"{kind}.trainable().forward", lambda v=v: v.trainable()(rays)),
                (f"{kind}.trainable().forward: skip", lambda v=v: v.trainable()(rays, skip=True)),
                (f"{kind}.trainable().forward: ray_grad", lambda v=v: v.trainable()(rays, ray_grad=True)),
                (f"{kind}.trainable().forward_views", lambda v=v: v.trainable().forward_views(poses, *cam)),
                (f"{kind}.trainable().forward_views: pose_grad", lambda v=v: v.trainable().forward_views(poses, *cam, pose_grad=True)),
                (f"{kind}.trainable().tv", lambda v=v: v.trainable().tv())]
    v, s = kinds["BakedVolume"], kinds["SparseBakedVolume"]
    t = v.trainable()
    focal2, c2 = torch.tensor([1.0, 2.0]), torch.tensor([0.5, 0.5])
    for what, fn in (("render", v.render), ("render_diff", v.render_diff), ("visibility", v.visibility), ("trainable().forward", t)):
        out += [(f"BakedVolume.{what}: rays (1,7)", lambda fn=fn: fn(z(1, 7))), (f"BakedVolume.{what}: rays is a list", lambda fn=fn: fn([0.0])),
                (f"BakedVolume.{what}: rays 0-dim", lambda fn=fn: fn(z(()))), (f"BakedVolume.{what}: rays (2,1,8) in float64", lambda fn=fn: fn(z(2, 1, 8, dtype=torch.float64)))]
    for what, fn in (("render_views", v.render_views), ("render_views_diff", v.render_views_diff), ("visibility_views", v.visibility_views),
                     ("trainable().forward_views", t.forward_views)):
        out += [(f"BakedVolume.{what}: poses (1,3,4)", lambda fn=fn: fn(z(1, 3, 4), *cam)), (f"BakedVolume.{what}: poses is a list", lambda fn=fn: fn([0.0], *cam)),
                (f"BakedVolume.{what}: focal and c as tensors", lambda fn=fn: fn(poses, 1, 1, focal2, 0.5, 3.0, c=c2)),
                (f"BakedVolume.{what}: focal a one-element tensor", lambda fn=fn: fn(poses, 1, 1, torch.tensor([1.0]), 0.5, 3.0)),
                (f"BakedVolume.{what}: W=0", lambda fn=fn: fn(poses, 0, 1, 1.0, 0.5, 3.0))]
    out += [("BakedVolume.render_views: gt_rgb shape", lambda: v.render_views(poses, *cam, gt_rgb=z(1, 2, 2, 3))),
            ("BakedVolume.render: skip=False", lambda: v.render(rays, skip=False)), ("SparseBakedVolume.render: skip=False", lambda: s.render(rays, skip=False)),
            ("SparseBakedVolume.visibility: skip=False", lambda: s.visibility(rays, skip=False)),
            ("BakedVolume.visibility: out shape", lambda: v.visibility(rays, out=z(3, 2, 2))), ("SparseBakedVolume.visibility: out shape", lambda: s.visibility(rays, out=z(2, 2, 2))),
            ("BakedVolume.visibility: rays (1,7) + out shape", lambda: v.visibility(z(1, 7), out=z(3, 2, 2))),
            ("BakedVolume.visibility_views: poses (1,3,4) + out shape", lambda: v.visibility_views(z(1, 3, 4), *cam, out=z(3, 2, 2))),
            ("BakedVolume.render: step=0.0", lambda: v.render(rays, step=0.0)), ("BakedVolume.render: terminate=1.0", lambda: v.render(rays, terminate=1.0)),
            ("fit: rays (1,7)", lambda: bake.fit(v, z(1, 7), z(1, 3))), ("fit: target shape", lambda: bake.fit(v, rays, z(2, 3))), ("fit: no rays", lambda: bake.fit(v, z(0, 8), z(0, 3))),
            ("fit: steps=-1", lambda: bake.fit(v, rays, z(1, 3), steps=-1)), ("fit: valid", lambda: bake.fit(v, rays, z(1, 3), steps=1)),
            ("fit: rays (1,7) + float16", lambda: bake.fit(kinds["BakedVolume, float16"], z(1, 7), z(1, 3))),
            ("fit_coarse_to_fine: rays (1,7)", lambda: bake.fit_coarse_to_fine(v, z(1, 7), z(1, 3), [(None, 1)])),
            ("fit_coarse_to_fine: no stages + rays (1,7)", lambda: bake.fit_coarse_to_fine(v, z(1, 7), z(1, 3), [])),
            ("fit_coarse_to_fine: valid", lambda: bake.fit_coarse_to_fine(v, rays, z(1, 3), [(None, 1)]))]
    scene = bake.BakedScene([v, v], torch.eye(4).expand(2, 4, 4))
    sparse_scene = bake.BakedScene([s], torch.eye(4)[None])
    ts = scene.trainable()
    bad_poses = z(2, 4, 3)
    for what, fn in (("BakedScene.render", scene.render), ("BakedScene.render_diff", scene.render_diff), ("TrainableScene.forward", ts)):
        out += [(f"{what}: rays (1,7)", lambda fn=fn: fn(z(1, 7))), (f"{what}: rays is a list", lambda fn=fn: fn([0.0])), (f"{what}: valid", lambda fn=fn: fn(rays)),
                (f"{what}: valid, skip=False", lambda fn=fn: fn(rays, skip=False))]
    for what, fn in (("BakedScene.render_views", scene.render_views), ("BakedScene.render_views_diff", scene.render_views_diff),
                     ("TrainableScene.forward_views", ts.forward_views)):
        out += [(f"{what}: poses (1,3,4)", lambda fn=fn: fn(z(1, 3, 4), *cam)), (f"{what}: valid", lambda fn=fn: fn(poses, *cam)),
                (f"{what}: focal and c as tensors", lambda fn=fn: fn(poses, 1, 1, focal2, 0.5, 3.0, c=c2))]
    out += [("BakedScene.render_diff: poses (2,4,3)", lambda: scene.render_diff(rays, poses=bad_poses)), ("BakedScene.render_diff: rays (1,7) + poses (2,4,3)", lambda: scene.render_diff(z(1, 7), poses=bad_poses)),
            ("BakedScene.render_views_diff: obj_poses (2,4,3)", lambda: scene.render_views_diff(poses, *cam, obj_poses=bad_poses)),
            ("BakedScene.render_views_diff: poses (1,3,4) + obj_poses (2,4,3)", lambda: scene.render_views_diff(z(1, 3, 4), *cam, obj_poses=bad_poses)),
            ("TrainableScene.forward: poses (2,4,3)", lambda: ts(rays, poses=bad_poses)), ("TrainableScene.forward: rays (1,7) + poses (2,4,3)", lambda: ts(z(1, 7), poses=bad_poses)),
            ("TrainableScene.forward_views: obj_poses (2,4,3)", lambda: ts.forward_views(poses, *cam, obj_poses=bad_poses)), ("TrainableScene.tv", lambda: ts.tv()),
            ("BakedScene of sparse volumes: render", lambda: sparse_scene.render(rays)), ("BakedScene of sparse volumes: render_diff", lambda: sparse_scene.render_diff(rays)),
            ("BakedScene of sparse volumes: trainable().forward", lambda: sparse_scene.trainable()(rays)), ("BakedScene of sparse volumes: trainable().tv", lambda: sparse_scene.trainable().tv()),
            ("BakedScene: kinds differ", lambda: bake.BakedScene([v, s], torch.eye(4).expand(2, 4, 4))), ("BakedScene: pose scaled", lambda: bake.BakedScene([v], torch.eye(4)[None] * 2.0)),
            ("fit_scene: rays (1,7)", lambda: bake.fit_scene(scene, z(1, 7), z(1, 3))), ("fit_scene: target shape", lambda: bake.fit_scene(scene, rays, z(2, 3))),
            ("fit_scene: valid", lambda: bake.fit_scene(scene, rays, z(1, 3), steps=1)),
            ("register: valid", lambda: bake.register(v, z(1, 1, 1, 3), poses, 1, 1, 1.0, 0.5, 3.0, steps=1)),
            ("place: valid", lambda: bake.place(scene, z(1, 1, 1, 3), poses, 1, 1, 1.0, 0.5, 3.0, steps=1))]
    return out


def march_cases(dev):
    """ops.baked_march, younger than the fixture, against the named function it must pick: -> [(label, the call of baked_march, the
    call of that function)] for every kind of stored tensor, along rays and over views.  A valid call, and two refusals that name the
    function that spoke (`step` on the host, the `bits` behind the first device check): the two outcomes must be equal"""
    from pixelnerf_amd import ops
    mk, i32, out = Maker(dev), torch.int32, []
    kinds = (("baked_render", None, False, False), ("baked_render", -1, False, False), ("baked_sh_render", 1, False, False),
             ("baked_sparse_render", None, True, False), ("baked_sparse_render", 2, True, False), ("baked_half_render", None, False, True),
             ("baked_half_render", 0, False, True), ("baked_sparse_half_render", -1, True, True), ("baked_sparse_half_render", 1, True, True))
    for name, degree, sparse, half in kinds:
        for views in (False, True):
            fn = getattr(ops, name + ("_views" if views else ""))
            for defect, step, nbits in (("valid", STEP, 1), ("step=0.0", 0.0, 1), ("bits of 2", STEP, 2)):
                source, stored = mk.head(views), mk.stored(degree, sparse, half)
                bits, index = mk.z(nbits, dtype=i32), mk.z(*RESO, dtype=i32) if sparse else None
                volume = (stored,) if name == "baked_render" else (stored, degree)
                named = (lambda fn=fn, a=(*source, *volume, index, bits, RESO, C1, C2, step): fn(*a)) if sparse else \
                    (lambda fn=fn, a=(*source, *volume, RESO, C1, C2, step), bits=bits: fn(*a, bits=bits))
                out.append((f"{fn.__name__} at degree {degree}: {defect}", named,
                            lambda a=(source, stored, degree, RESO, C1, C2, step), bits=bits, index=index: ops.baked_march(*a, bits=bits, index=index)))
    return out


def cases(dev):
    """-> [(label, thunk)] of every call on `dev` ("cpu": the whole list; a HIP device: what needs no object of util.bake)"""
    from pixelnerf_amd import autograd, ops
    mk = Maker(dev)
    out = []
    for views in (False, True):
        for family, names in ((forward_cases, FORWARD), (single_cases, SINGLE), (scene_cases, SCENE)):
            for name in names:
                full = VIEWS.get(name, name + "_views") if views else name
                out += [(f"{full}: {label}", thunk) for label, thunk in family(mk, ops, name, views)]
    out += grid_cases(mk, ops) + autograd_cases(mk, autograd)
    if not mk.on_device:
        out += bake_cases()
    return out


def record(dev):
    """{label: [exception type name or "", str(exception) or what returned]} of every call on `dev`"""
    import warnings
    got = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for label, thunk in cases(dev):
            assert label not in got, label
            got[label] = outcome(thunk)
    return got


# ---- the fixture.  A label is "<function>: <defect>"; an outcome that begins with its function's name is stored with "~" in its
# place, every distinct outcome once ("outcomes"), and a section maps function -> defect -> the outcome's number.  The device
# section holds only what differs from the host's outcome of the same label (most refusals come before any device is looked at);
# "host_only" lists the host's labels that the device does not have, so the device's label set stands in the file too

def _nest(labels):
    out = {}
    for label in sorted(labels):
        function, _, defect = label.partition(": ")  # (a label without a defect: the function alone)
        out.setdefault(function, []).append(defect)
    return out


def _flat(nested):
    return [f"{function}: {defect}" if defect else function for function, defects in nested.items() for defect in defects]


def pack(cpu, differs, host_only, device_count):
    """cpu: {label: outcome}; differs: the device's {label: outcome} where it is not the host's; host_only: the labels of cpu that
    the device does not have"""
    outcomes, sections = [], {"cpu": {}, "device": {}}
    for section, got in (("cpu", cpu), ("device", differs)):
        for function, defects in _nest(got).items():
            for defect, label in zip(defects, _flat({function: defects})):
                kind, message = got[label]
                entry = [kind, "~" + message[len(function):] if message.startswith(function + ": ") else message]
                if entry not in outcomes:
                    outcomes.append(entry)
                sections[section].setdefault(function, {})[defect] = outcomes.index(entry)
    return dict(outcomes=outcomes, device_count=device_count, host_only=_nest(host_only), **sections)


def unpack(fixture):
    """-> (cpu {label: outcome}, device {label: outcome}: the host's outcome unless the fixture's device section says another)"""
    out = []
    for section in ("cpu", "device"):
        out.append({label: [fixture["outcomes"][k][0], fixture["outcomes"][k][1].replace("~", function, 1)
                            if fixture["outcomes"][k][1].startswith("~: ") else fixture["outcomes"][k][1]]
                    for function, defects in fixture[section].items() for (defect, k), label in zip(defects.items(), _flat({function: defects}))})
    cpu, differs = out
    absent = set(_flat(fixture["host_only"]))
    return cpu, {**{label: o for label, o in cpu.items() if label not in absent}, **differs}


def dump(fixture, path):
    """one line per outcome and per function: a diff of the fixture reads as the refusals that changed"""
    row = lambda v: json.dumps(v, sort_keys=True)
    lines = ['"outcomes": [\n' + ",\n".join(row(o) for o in fixture["outcomes"]) + "\n]"]
    for section in ("cpu", "device", "host_only"):
        lines.append(f'"{section}": {{\n' + ",\n".join(f"{row(f)}: {row(d)}" for f, d in sorted(fixture[section].items())) + "\n}")
    lines.append(f'"device_count": {row(fixture["device_count"])}')
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    old = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else None
    cpu, device = unpack(old) if old else ({}, {})
    device_count = old["device_count"] if old else 0
    if "--device" in sys.argv[1:]:  # against the host section that is there: record that one first
        device, device_count = record("cuda:0"), min(torch.cuda.device_count(), 2)
    else:
        cpu = record("cpu")
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    differs = {k: v for k, v in device.items() if cpu.get(k) != v}
    dump(pack(cpu, differs, set(cpu) - set(device), device_count), out)
    print(f"{len(cpu)} calls on the host, {len(device)} on the device ({len(differs)} differ) -> {out}")
