"""Test helper (not a test): early ray termination (include/pixelnerf_hip.h, pnr_termination_mark; NeRFRenderer.forward(terminate=))
restated in numpy, plus the seeded inputs the host and the GPU tests share.

The transmittance in front of a boundary is a product of per-sample factors f = 1 - (1 - exp(-delta max(sigma, 0))) + 1e-10.  A fully
opaque sample has alpha rounded to 1 and f = 1e-10, and a one-ulp difference between two expf implementations moves a small factor
by a large RELATIVE amount: an fp64 product is therefore no usable reference and a relative tolerance on T means nothing.  What
can be stated is a bracket.  Every factor is computed here in float32 exactly as the kernel computes it; the kernel's own factor
differs from it by at most 3 ulp of 1 ABSOLUTE (expf within 2 ulp of a value <= 1 in the common case, two more roundings of numbers
near 1), and the fp32 product of up to K factors adds a relative error below K 2^-24 < 2e-5.  So with
    lo = prod max(f - 3 2^-23, 0) (1 - 2e-5),   hi = prod (f + 3 2^-23) (1 + 2e-5)   (in fp64)
the device value lies in [lo, hi]; a boundary is DECIDED when hi <= eps (stopped) or lo > eps (alive), and a ray with an undecided
boundary is AMBIGUOUS: either outcome is right for it.  The tests bound the number of ambiguous rays (2 %)."""
import numpy as np

ABS = 3.0 * 2.0 ** -23
REL = 2e-5
AMBIGUOUS_CAP = 0.02


def stage_bounds(K, stages):
    """terminate_stages -> [0, b_1, ..., K].  An int S: b_s = 2 ((K s) // (2 S)), zeros and duplicates dropped (for even K no pair
    (2j, 2j+1) straddles a stage); a sequence: the interior boundaries, strictly increasing inside (0, K), as given."""
    K = int(K)
    if isinstance(stages, (int, np.integer)):
        S = int(stages)
        if S < 1:
            raise ValueError("stages < 1")
        inner = []
        for s in range(1, S):
            b = 2 * ((K * s) // (2 * S))
            if 0 < b < K and (not inner or b > inner[-1]):
                inner.append(b)
    else:
        inner = [int(b) for b in stages]
        if any(not 0 < b < K for b in inner) or any(b1 <= b0 for b0, b1 in zip(inner, inner[1:])):
            raise ValueError("boundaries not increasing inside (0, K)")
    return [0] + inner + [K]


def factors(rays, z, rgbsigma):
    """-> f (R,K) float32, the kernel's operations one by one: delta = z_next - z (the last: far - z), alpha = 1 - expf(-delta
    fmaxf(sigma, 0)) (fmaxf drops a NaN sigma), f = (1 - alpha) + 1e-10"""
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 8)
    z = np.asarray(z, dtype=np.float32).reshape(rays.shape[0], -1)
    sigma = np.asarray(rgbsigma, dtype=np.float32).reshape(z.shape[0], z.shape[1], 4)[..., 3]
    with np.errstate(all="ignore"):
        znext = np.concatenate([z[:, 1:], rays[:, 7:8]], axis=1)
        delta = (znext - z).astype(np.float32)
        arg = (-delta * np.fmax(sigma, np.float32(0.0))).astype(np.float32)
        alpha = (np.float32(1.0) - np.exp(arg).astype(np.float32)).astype(np.float32)
        return ((np.float32(1.0) - alpha).astype(np.float32) + np.float32(1e-10)).astype(np.float32)


def bracket(f, k):
    """f (R,K) float32 -> (lo, hi, nan) (R,) of the transmittance in front of sample k; nan: a factor in front of k is NaN (the
    transmittance is NaN: the ray stays alive, decided)"""
    f64 = np.asarray(f, dtype=np.float32)[:, :k].astype(np.float64)
    nan = np.isnan(f64).any(axis=1)
    with np.errstate(all="ignore"):
        g = np.where(np.isnan(f64), 1.0, f64)
        lo = np.prod(np.maximum(g - ABS, 0.0), axis=1) * (1.0 - REL)
        hi = np.prod(g + ABS, axis=1) * (1.0 + REL)
    return lo, hi, nan


def mark_ref(rays, z, rgbsigma, k_begin, k_end, eps, keep_in=None):
    """pnr_termination_mark -> (keep (R,K) uint8 -- exact on the decided rays --, lo, hi (R,) of t_front, ambiguous (R,) bool)"""
    z = np.asarray(z, dtype=np.float32)
    R, K = z.shape
    lo, hi, nan = bracket(factors(rays, z, rgbsigma), k_begin)
    stopped = (hi <= eps) & ~nan
    ambiguous = ~nan & ~stopped & ~(lo > eps)
    keep = np.zeros((R, K), dtype=np.uint8)
    keep[:, k_begin:k_end] = 1
    keep[stopped] = 0
    if keep_in is not None:
        keep &= (np.asarray(keep_in).reshape(R, K) != 0).astype(np.uint8)
    return keep, lo, hi, ambiguous


def stops(rays, z, rgbsigma, bounds, eps):
    """the stop rule on the DENSE outputs (rgb sigma already 0 where a grid calls the sample empty): -> (stop (R,) int -- the first
    boundary b_s, 1 <= s < S, with T <= eps, K for a ray that never stops --, ambiguous (R,) bool -- the ray met an undecided
    boundary before a decided stop; its `stop` is then one of the two admissible outcomes)"""
    z = np.asarray(z, dtype=np.float32)
    R, K = z.shape
    f = factors(rays, z, rgbsigma)
    stop = np.full(R, K, dtype=np.int64)
    ambiguous = np.zeros(R, dtype=bool)
    for b in bounds[1:-1]:
        lo, hi, nan = bracket(f, b)
        live = (stop == K) & ~ambiguous
        stopped = live & ~nan & (hi <= eps)
        ambiguous |= live & ~nan & ~stopped & ~(lo > eps)
        stop[stopped] = b
    return stop, ambiguous


def zero_behind(rgbsigma, stop):
    """the dense outputs (R,K,4) with rgb sigma := 0 at every sample k >= stop[r]"""
    out = np.array(rgbsigma, dtype=np.float32, copy=True)
    out[np.arange(out.shape[1])[None, :] >= np.asarray(stop)[:, None]] = 0.0
    return out


def composite64(rays, z, rgbsigma, white_bkgd):
    """nerf.py:178-182,223-249 in fp64 -> (weights (R,K), rgb (R,3), depth (R,), T_end (R,))"""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 8)
    z = np.asarray(z, dtype=np.float64)
    rs = np.asarray(rgbsigma, dtype=np.float64)
    delta = np.concatenate([z[:, 1:], rays[:, 7:8]], axis=1) - z
    alpha = 1.0 - np.exp(-delta * np.maximum(rs[..., 3], 0.0))
    fac = 1.0 - alpha + 1e-10
    T = np.concatenate([np.ones((z.shape[0], 1)), np.cumprod(fac, axis=1)], axis=1)
    w = alpha * T[:, :-1]
    rgb = (w[..., None] * rs[..., :3]).sum(axis=1)
    if white_bkgd:
        rgb = rgb + 1.0 - w.sum(axis=1, keepdims=True)
    return w, rgb, (w * z).sum(axis=1), T[:, -1]


def counts(stop, bounds, keep_in=None):
    """what last_terminate_stats holds for one call: evaluated = samples in front of their ray's stop (and kept by keep_in)"""
    stop = np.asarray(stop)
    R, K = len(stop), bounds[-1]
    live = np.arange(K)[None, :] < stop[:, None]
    if keep_in is not None:
        live &= np.asarray(keep_in).reshape(R, K) != 0
    return {"evaluated": int(live.sum()), "total": R * K, "stopped_rays": int((stop < K).sum()), "rays": R,
            "stages": [(int(live[:, a:b].sum()), R * (b - a)) for a, b in zip(bounds[:-1], bounds[1:])]}


# ---------------------------------------------------------------- seeded inputs shared by the host and the GPU tests

def hand_case():
    """three rays, K = 4, unit spacing (z = 0, 1, 2, 3; far = 4), boundaries at 2 (and 4), eps = 1e-2 -> (rays, z, rgbsigma, stop):
    ray 0 is opaque at sample 1 (sigma 100: alpha rounds to 1, T in front of 2 is 1e-10): stops at 2;
    ray 1 is transparent throughout: never stops;
    ray 2 has T = exp(-4) = 1.8e-2 in front of 2 and exp(-6) = 2.5e-3 in front of 3 -- it crosses eps BETWEEN the boundaries 2 and
    4, so with the boundaries [0, 2, 4] it never stops, and with [0, 2, 3, 4] it stops at 3."""
    rays = np.zeros((3, 8), dtype=np.float32)
    rays[:, 5], rays[:, 7] = 1.0, 4.0
    z = np.tile(np.arange(4, dtype=np.float32), (3, 1))
    rs = np.zeros((3, 4, 4), dtype=np.float32)
    rs[..., :3] = 0.5
    rs[0, 1, 3] = 100.0
    rs[2, :, 3] = 2.0
    return rays, z, rs, {(0, 2, 4): [2, 4, 4], (0, 2, 3, 4): [2, 4, 3]}


MARK_SHAPES = [(1, 1), (3, 63), (5, 64), (7, 65), (64, 96), (16, 200)]
K_BEGINS = (0, 1, 63, 64, 65)


def mark_case(R, K, seed=0):
    """sorted z in [1, 4) with far = 4, sigma drawn so that the rays go opaque at varied depths: a per-ray onset uniform over the
    ray (beyond its end for a quarter of them: those stay alive), behind it sigma ~ exp(N(2, 1.5)); 20 % of all sigmas exactly 0,
    a few fully opaque (1e4), negative ones (relu) -- and a NaN sigma on the last ray, which is otherwise transparent (alive)
    -> (rays (R,8), z (R,K), rgbsigma (R,K,4), keep_in (R,K) uint8)"""
    rs = np.random.RandomState(700 + 13 * R + K + seed)
    rays = rs.standard_normal((R, 8)).astype(np.float32)
    rays[:, 6], rays[:, 7] = 1.0, 4.0
    z = np.sort(rs.uniform(1.0, 4.0, (R, K)), axis=1).astype(np.float32)
    onset = rs.uniform(0.0, 1.33, (R, 1)) * K
    sigma = np.where(np.arange(K)[None, :] >= onset, np.exp(rs.normal(2.0, 1.5, (R, K))), rs.uniform(-1.0, 0.05, (R, K)))
    sigma[rs.uniform(size=(R, K)) < 0.20] = 0.0
    sigma[rs.uniform(size=(R, K)) < 0.02] = 1e4
    rgbsigma = np.concatenate([rs.uniform(0, 1, (R, K, 3)), sigma[..., None]], axis=2).astype(np.float32)
    rgbsigma[-1, :, 3] = 0.0
    rgbsigma[-1, 0, 3] = np.nan
    keep_in = (rs.uniform(size=(R, K)) < 0.6).astype(np.uint8) * np.uint8(1 + seed % 3)
    return rays, z, rgbsigma, keep_in
