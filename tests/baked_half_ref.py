"""The inputs the host and the GPU tests of the half-precision baked volumes share (include/pixelnerf_hip.h, "Half-precision baked
volumes"), and numpy's own statement of the rounding: `half_round` is np.clip + astype(float16), nothing of util.bake.

The fixtures start from the volumes of the fp32 tests (baked_ref.common_volume, baked_sh_ref.common_coef) and plant, at inner points
where sigma > 0, what fp16 storage can get wrong: fp16 subnormals, a sigma of exactly 65504, one of 1e6 (saturates), a -0.0.  nz = 7
gives pair bases of both parities.  `check_preconditions` asserts, on the host, that the fixture can tell a march of the wrong values
from a march of the right ones."""
import functools

import numpy as np

import baked_ref as B
import baked_sh_ref as S

HALF_MAX = 65504.0
RESO, C1, C2, SETTINGS = B.RESO, B.C1, B.C2, B.SETTINGS
KINDS = ["rgba", 0, 1, 2]                                                  # the RGBA volume and the three degrees
KIND_IDS = ["rgba", "L0", "L1", "L2"]

# (point, channel, value): all at points with a positive sigma (x in {5, 6} or y == 5, inside the inner part [2:-2] of the grid)
PLANTS = (((5, 3, 3), 3, 3e-6), ((5, 3, 3), 0, 2e-7),                      # fp16 subnormals: below 2^-14 = 6.1e-5
          ((5, 2, 3), 3, 2e-6), ((5, 2, 3), 2, 2e-7),
          ((6, 5, 2), 3, 65504.0),                                        # the largest finite fp16
          ((5, 5, 4), 3, 1e6),                                            # saturates
          ((6, 3, 2), 1, -0.0))


def half_round(x):
    """round to nearest even into fp16 after saturating at +-65504 (numpy's own conversion)"""
    return np.clip(np.asarray(x, np.float32), np.float32(-HALF_MAX), np.float32(HALF_MAX)).astype(np.float16)


def value_bound(v):
    """what rounding may move a value v, |v| <= 65504, by: max(2^-11 |v|, 2^-25)"""
    return np.maximum(2.0 ** -11 * np.abs(np.asarray(v, np.float64)), 2.0 ** -25)


def fixture_volume():
    """(9,8,7,4) fp32: the shared volume with the plants"""
    vol = B.common_volume().copy()
    for (i, j, k), ch, value in PLANTS:
        assert vol[i, j, k, 3] > 0, (i, j, k)
        vol[i, j, k, ch] = np.float32(value)
    return vol


def fixture_coef(degree):
    """(9,8,7,B,4) fp32: the shared coefficients, the DC part with the plants; one higher coefficient an fp16 subnormal (degree >= 1)"""
    coef = S.common_coef(degree).copy()
    coef[..., 0, :] = fixture_volume()
    if degree >= 1:
        coef[6, 4, 3, 2, 3] = np.float32(-4e-6)
        coef[6, 4, 3, 1, 0] = np.float32(3e-7)
    return coef


def fixture(kind):
    return fixture_volume() if kind == "rgba" else fixture_coef(kind)


def tiny_sigma(kind):
    """the fixture with sigma = 1e-8 (positive, below 2^-25: it rounds to 0 in fp16) on the 3x3x3 block of points [2:5, 2:5, 2:5]
    that is empty in the shared volume, and every higher sigma coefficient 0 there: the fp32 skip grid has the block's cells on, the
    half one has them off"""
    a = fixture(kind).copy()
    if kind == "rgba":
        a[2:5, 2:5, 2:5, 3] = np.float32(1e-8)
    else:
        a[2:5, 2:5, 2:5, 0, 3] = np.float32(1e-8)
    return a


def render_ref(kind, rays, values, step, **kw):
    """the fp64 / fp32 restatements of the fp32 tests, on `values` (fp32-representable)"""
    if kind == "rgba":
        return B.render_ref(rays, values, C1, C2, step, **kw)
    return S.render_ref(rays, values, C1, C2, step, kind, **kw)


@functools.lru_cache(maxsize=None)
def check_preconditions(kind):
    """-> (subnormals, at 65504, saturated, changed share, rays that differ) of the fixture of `kind`; asserts what the bit test
    needs: at least one subnormal fp16, one 65504 that was stored as such and one saturated value after rounding, more than half
    of the stored values changed by the rounding, and the fp64 restatement of the rounded volume different from that of the
    unrounded one on a ray that hits the box"""
    a = fixture(kind)
    h = half_round(a)
    wide = h.astype(np.float32)
    assert np.isfinite(wide).all()
    mag = np.abs(wide)
    subnormal = int(((mag > 0) & (mag < 2.0 ** -14)).sum())
    exact_max = int(((a == np.float32(HALF_MAX)) & (wide == np.float32(HALF_MAX))).sum())
    saturated = int((np.abs(a) > HALF_MAX).sum())
    assert subnormal >= 1 and exact_max >= 1 and saturated >= 1, (subnormal, exact_max, saturated)
    assert (mag[np.abs(a) > HALF_MAX] == np.float32(HALF_MAX)).all()
    assert np.signbit(wide[6, 3, 2, 1] if kind == "rgba" else wide[6, 3, 2, 0, 1]) and (wide[6, 3, 2, 1] if kind == "rgba" else wide[6, 3, 2, 0, 1]) == 0
    changed = float((wide != a).mean())
    assert changed > 0.5, changed
    setting = "n40"
    rays, step = B.common_rays(setting), SETTINGS[setting][2]
    r_round = render_ref(kind, rays, wide, step, dtype=np.float64)
    r_plain = render_ref(kind, rays, a, step, dtype=np.float64)
    differ = np.flatnonzero((r_round[0] != r_plain[0]).any(axis=1) & (r_plain[2] > 0))
    assert differ.size >= 1
    return subnormal, exact_max, saturated, changed, int(differ.size)
