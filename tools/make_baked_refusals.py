#!/usr/bin/env python
"""Every refusal of the ten pnr_baked_*render* entries, as the library words it: return code and pnr_last_error() in full.

    python tools/make_baked_refusals.py            # writes tests/golden/baked_refusals.json and nothing else

All of it runs before any device work (no GPU needed): each call carries ONE defect, or one of a few pairs that pin the order of the
checks, and stand-in pointers that are never touched.  tests/test_baked_refusals_host.py records the same calls with the library of
the checkout and compares them with the fixture, which was written by this script at the commit before the entries were folded
into one checked description (pnr_baked.h: baked_check, which baked_render and every other family of baked entries calls)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "baked_refusals.json")

P = 64  # a non-null, 16-byte aligned stand-in for a device pointer
ENTRIES = {  # name -> (camera?, takes a degree?, sparse?)
    "pnr_baked_render_rays": (False, False, False), "pnr_baked_render_views": (True, False, False),
    "pnr_baked_sh_render_rays": (False, True, False), "pnr_baked_sh_render_views": (True, True, False),
    "pnr_baked_sparse_render_rays": (False, True, True), "pnr_baked_sparse_render_views": (True, True, True),
    "pnr_baked_half_render_rays": (False, True, False), "pnr_baked_half_render_views": (True, True, False),
    "pnr_baked_sparse_half_render_rays": (False, True, True), "pnr_baked_sparse_half_render_views": (True, True, True),
}
GOOD = dict(rays=P, R=4, poses=P, NV=1, W=4, H=4, vol=P, M=10, degree=2, index=P, bits=P, n=(4, 4, 4), c1=(-1.0, -1.0, -1.0),
            c2=(1.0, 1.0, 1.0), step=0.1, term=0.0, rgb=P, depth=P, alpha=P)


def call(lib, name, **defect):
    camera, has_degree, sparse = ENTRIES[name]
    a = dict(GOOD)
    a.update(defect)
    f3 = ctypes.c_float * 3
    args = [a["poses"], a["NV"], a["W"], a["H"], 10.0, 10.0, 2.0, 2.0, 0.5, 3.0] if camera else [a["rays"], a["R"]]
    args += [a["vol"]] + ([a["M"]] if sparse else []) + ([a["degree"]] if has_degree else []) + ([a["index"]] if sparse else [])
    args += [a["bits"], *a["n"], f3(*a["c1"]), f3(*a["c2"]), a["step"], 0, a["term"], a["rgb"], a["depth"], a["alpha"], None]
    rc = getattr(lib, name)(*args)
    return [rc, lib.pnr_last_error().decode() if rc != 0 else ""]


def defects(name):
    """(label, arguments) of every call made to entry `name`"""
    camera, has_degree, sparse = ENTRIES[name]
    degrees = [None] if not has_degree else ([0, 1, 2] if "_sh_" in name else [-1, 0, 1, 2])
    out = []
    if has_degree:
        out += [(f"degree={d}", dict(degree=d)) for d in (-3, -2, -1, 3, 9) if d not in degrees]
    if camera:
        out += [("NV=-1", dict(NV=-1)), ("W=0", dict(W=0)), ("H=-3", dict(H=-3)), ("poses=null", dict(poses=None)),
                ("poses misaligned", dict(poses=P + 1)), ("launch limit", dict(W=2 ** 17, H=2 ** 17))]
    else:
        out += [("R=-1", dict(R=-1)), ("rays=null", dict(rays=None)), ("rays misaligned", dict(rays=P + 1)),
                ("launch limit", dict(R=2 ** 34))]
    for d in degrees:
        at = {} if d is None else dict(degree=d)
        tag = "" if d is None else f" at degree {d}"
        out += [(f"vol=null{tag}", dict(vol=None, **at)), (f"vol misaligned{tag}", dict(vol=P + 8, **at))]
    if sparse:
        out += [("M=-1", dict(M=-1)), ("index=null", dict(index=None)), ("index misaligned", dict(index=P + 2)),
                ("bits=null", dict(bits=None))]
    out.append(("bits misaligned", dict(bits=P + 2)))
    for o in ("rgb", "depth", "alpha"):
        out += [(f"{o}=null", {o: None}), (f"{o} misaligned", {o: P + 2})]
    out += [(f"dims={n}", dict(n=n)) for n in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 0, 0), (2 ** 11, 2 ** 11, 2 ** 11))]
    out += [("c1>=c2", dict(c1=GOOD["c2"], c2=GOOD["c1"])), ("c1==c2 on y", dict(c1=(-1.0, 1.0, -1.0))),
            ("c1 NaN", dict(c1=(float("nan"), -1.0, -1.0)))]
    out += [(f"step={s}", dict(step=s)) for s in (0.0, -0.1, float("inf"), float("nan"))]
    out += [(f"terminate={t}", dict(term=t)) for t in (-0.01, 1.0, float("nan"))]
    # two defects: the earlier check speaks
    src_bad = dict(NV=-1) if camera else dict(R=-1)
    src_null = dict(poses=None) if camera else dict(rays=None)
    none = dict(NV=0) if camera else dict(R=0)
    if has_degree:
        out.append(("degree=3 + bad source", dict(degree=3, **src_bad)))
        out.append(("degree=3 + no rays", dict(degree=3, **none)))
    both = dict(c1=GOOD["c2"], c2=GOOD["c1"])
    too_many = dict(W=2 ** 17, H=2 ** 17) if camera else dict(R=2 ** 34)
    out += [("bad source + dims", dict(n=(1, 4, 4), **src_bad)), ("null source + step", dict(step=0.0, **src_null)),
            ("dims + c1>=c2", dict(n=(1, 4, 4), **both)), ("c1>=c2 + step", dict(step=0.0, **both)),
            ("step + terminate", dict(step=0.0, term=1.0)), ("terminate + rgb=null", dict(term=1.0, rgb=None)),
            ("rgb=null + vol misaligned", dict(rgb=None, vol=P + 8)), ("vol=null + bits misaligned", dict(vol=None, bits=P + 2)),
            ("vol misaligned + rgb misaligned", dict(vol=P + 8, rgb=P + 2)), ("rgb misaligned + launch limit", dict(rgb=P + 2, **too_many)),
            ("no rays: nothing else is looked at", dict(vol=None, bits=None, rgb=None, depth=None, alpha=None, index=None, **src_null, **none)),
            ("no rays + terminate", dict(term=1.0, **none))]
    if sparse:
        out += [("bad source + M=-1", dict(M=-1, **src_bad)), ("M=-1 + dims", dict(M=-1, n=(1, 4, 4))), ("no rays + M=-1", dict(M=-1, **none)),
                ("M=0 + rgb=null", dict(M=0, vol=None, index=None, bits=None, rgb=None)),
                ("vol misaligned + index misaligned", dict(vol=P + 8, index=P + 2)),
                ("index misaligned + bits misaligned", dict(index=P + 2, bits=P + 2))]
    return out


def record(lib):
    """{entry: {label: [return code, message]}} with the library `lib` (pixelnerf_amd._lib.load())"""
    return {name: {label: call(lib, name, **d) for label, d in defects(name)} for name in ENTRIES}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from pixelnerf_amd import _lib
    got = record(_lib.load())
    with open(FIXTURE, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v) for v in got.values())} calls of {len(got)} entries -> {FIXTURE}")
