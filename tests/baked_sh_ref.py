"""numpy restatement of the view-dependent baked-volume march (include/pixelnerf_hip.h, "baked volumes", the spherical-harmonic
paragraph), and the inputs the host and the GPU tests of it share.  Like baked_ref.render_ref it walks the samples of a ray one
after the other in `dtype`: fp64 is the yardstick, fp32 what a correct fp32 implementation of the same formulas differs from it by.

The march is restated here and not borrowed from baked_ref.render_ref: that one rounds the volume it is given to fp32, and the
volume "this object seen from direction d" is a COMPUTED quantity, so going through it would put an fp32 rounding into the fp64
yardstick.  The inputs proper -- rays, coef, c1, c2, step -- are rounded to fp32 first and then carried in `dtype`, as there."""
import numpy as np

import baked_ref as B

MAX_SAMPLES = B.MAX_SAMPLES
# max |Y_k| on the sphere, k = 1..8
Y_MAX = np.array([np.sqrt(3.0)] * 3 + [np.sqrt(15.0) / 2, np.sqrt(15.0) / 2, np.sqrt(5.0), np.sqrt(15.0) / 2, np.sqrt(15.0) / 2])


def n_basis(degree):
    if degree not in (0, 1, 2):
        raise ValueError(f"degree must be 0, 1 or 2, got {degree}")
    return (degree + 1) ** 2


def sh_basis(d, degree, dtype=np.float64):
    """d (3,) or (N,3), fp32-representable -> Y (B,) or (N,B) in `dtype`; Y_0 = 1.  The constants are rounded to fp32 once."""
    dt = np.dtype(dtype).type
    nb = n_basis(degree)
    d = np.asarray(d, np.float32).astype(dtype)
    single = d.ndim == 1
    d = d.reshape(-1, 3)
    c1, c2, c20, c22 = (dt(np.float32(v)) for v in (np.sqrt(3.0), np.sqrt(15.0), np.sqrt(5.0) / 2.0, np.sqrt(15.0) / 2.0))
    with np.errstate(all="ignore"):
        n2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        s = np.sqrt(n2)
        x, y, z = d[:, 0] / s, d[:, 1] / s, d[:, 2] / s
        cols = [np.ones_like(x), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c20 * (dt(3.0) * (z * z) - dt(1.0)), c2 * (x * z),
                c22 * (x * x - y * y)]
    Y = np.stack(cols[:nb], axis=1).astype(dtype)
    bad = ~(np.isfinite(n2) & (n2 != 0))
    Y[bad, 1:] = 0
    return Y[0] if single else Y


def corner_value(coef, Y, dtype=np.float64):
    """coef (...,B,4), Y (B,) in `dtype` -> (...,4): the sum over k in the order k = 0, 1, ..., each product and sum rounded on its
    own, then rgb clamped to [0,1] and sigma to >= 0"""
    coef = np.asarray(coef, np.float32).astype(dtype)
    Y = np.asarray(Y, dtype)
    v = coef[..., 0, :] * Y[0]
    for k in range(1, coef.shape[-2]):
        v = v + coef[..., k, :] * Y[k]
    v = np.where(v < 0, np.zeros_like(v), v)
    v[..., :3] = np.where(v[..., :3] > 1, np.ones_like(v[..., :3]), v[..., :3])
    return v


def render_ref(rays, coef, c1, c2, step, degree, white_bkgd=False, occupied=None, terminate=0.0, dtype=np.float64):
    """rays (R,8), coef (nx,ny,nz,B,4) with B = (degree+1)^2, occupied None or (nx-1,ny-1,nz-1) bool, terminate eps in [0,1)
    -> rgb (R,3), depth (R,), alpha (R,) in `dtype`"""
    dt = np.dtype(dtype).type
    nb = n_basis(degree)
    rays = np.asarray(rays, np.float32).astype(dtype)
    coef = np.asarray(coef, np.float32).astype(dtype)
    assert coef.ndim == 5 and coef.shape[3] == nb and coef.shape[4] == 4, coef.shape
    reso = coef.shape[:3]
    c1 = np.asarray(c1, np.float32).astype(dtype)
    c2 = np.asarray(c2, np.float32).astype(dtype)
    h = B.cell_size(c1, c2, reso, dtype)
    step, eps, tiny = dt(np.float32(step)), dt(np.float32(terminate)), dt(1e-10)
    half, one, zero = dt(0.5), dt(1.0), dt(0.0)
    R = rays.shape[0]
    rgb, depth, alpha = np.zeros((R, 3), dtype), np.zeros((R,), dtype), np.zeros((R,), dtype)
    for r in range(R):
        o, d, near, far = rays[r, 0:3], rays[r, 3:6], rays[r, 6], rays[r, 7]
        n = 0
        if np.isfinite(rays[r]).all() and near < far:
            count = np.ceil((far - near) / step)
            if count <= MAX_SAMPLES:
                n = int(count)
        Y = sh_basis(rays[r, 3:6], degree, dtype)  # (exact: the direction is fp32-representable)
        T = one
        acc = np.zeros((5,), dtype)  # r, g, b, depth, alpha
        for i in range(n):
            t = near + (dt(i) + half) * step
            p = o + t * d
            inside = bool(np.all(p >= c1) and np.all(p <= c2))
            val = np.zeros((4,), dtype)
            if inside:
                u = (p - c1) / h
                cell = np.minimum(np.maximum(np.floor(u), zero), (np.asarray(reso) - 2).astype(dtype))
                f = np.minimum(np.maximum(u - cell, zero), one)
                ix, iy, iz = (int(c) for c in cell)
                if occupied is None or occupied[ix, iy, iz]:
                    v = corner_value(coef[ix:ix + 2, iy:iy + 2, iz:iz + 2], Y, dtype)   # (2,2,2,4): clamped per corner, before the blend
                    vz = v[:, :, 0] + f[2] * (v[:, :, 1] - v[:, :, 0])   # along z, then y, then x
                    vy = vz[:, 0] + f[1] * (vz[:, 1] - vz[:, 0])
                    val = vy[0] + f[0] * (vy[1] - vy[0])
            a = one - np.exp(-(step * val[3]))
            w = a * T
            acc[0:3] += w * val[0:3]
            acc[3] += w * t
            acc[4] += w
            T = T * (one - a + tiny)
            if eps > 0 and (i + 1) % 64 == 0 and T <= eps:
                break
        if white_bkgd:
            acc[0:3] = acc[0:3] + one - acc[4]
        rgb[r], depth[r], alpha[r] = acc[0:3], acc[3], acc[4]
    return rgb, depth, alpha


# ---------------------------------------------------------------- the inputs of tests/test_hip_baked_sh.py (checked on the host too)
RESO, C1, C2, SETTINGS, common_rays, gaps = B.RESO, B.C1, B.C2, B.SETTINGS, B.common_rays, B.gaps


def common_coef(degree=2, seed=20240608):
    """(9,8,7,B,4): the DC part is baked_ref.common_volume(); rgb coefficients k >= 1 uniform in [-0.25, 0.25]; sigma coefficients
    k >= 1 uniform in [-4, 4] where the DC sigma is > 0 and exactly 0 elsewhere (the zero outer layers and the empty block stay
    empty for every direction).  Degree 1 is the first 4 coefficients of degree 2."""
    rs = np.random.RandomState(seed)
    coef = np.empty(RESO + (9, 4), np.float32)
    coef[..., 0, :] = B.common_volume()
    coef[..., 1:, :3] = rs.uniform(-0.25, 0.25, RESO + (8, 3))
    sig = rs.uniform(-4.0, 4.0, RESO + (8,)).astype(np.float32)
    coef[..., 1:, 3] = np.where(coef[..., 0, 3][..., None] > 0, sig, np.float32(0.0))
    return np.ascontiguousarray(coef[..., :n_basis(degree), :])


def fibonacci_directions(n):
    """the spherical Fibonacci set of BakedSHVolume.directions, restated: z_m = 1 - (2m+1)/M, phi_m = m pi (3 - sqrt 5), fp64 -> fp32"""
    m = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * m + 1.0) / n
    phi = m * np.pi * (3.0 - np.sqrt(5.0))
    rho = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack((rho * np.cos(phi), rho * np.sin(phi), z), axis=1).astype(np.float32)


def projection(dirs, degree):
    """P = pinv(Y(dirs)) in fp64 from the fp32 directions: (B, M)"""
    return np.linalg.pinv(sh_basis(dirs, degree, np.float64))


def projection_bound(P, v):
    """what applying fp32(P) (B,M) to values v (M,...) sequentially in fp32 may differ from the fp64 product by, elementwise:
    (M + 2) 2^-24 (|P| @ |v|) -- one rounding of P, one of each product, M - 1 of the running sum, to first order"""
    P, v = np.abs(np.asarray(P, np.float64)), np.abs(np.asarray(v, np.float64))
    return (P.shape[1] + 2) * 2.0 ** -24 * np.tensordot(P, v, axes=(1, 0))
