"""numpy restatement of the baked-volume ray march (include/pixelnerf_hip.h, "baked volumes"), and the inputs the host and the GPU
tests share.  render_ref walks the samples of a ray one after the other -- no scan, no chunks beyond the termination check -- in
`dtype`: fp64 is the yardstick, fp32 shows what a correct fp32 implementation of the same formulas differs from it by.

The inputs are what the kernel gets: rays, vol, c1, c2 and step are rounded to fp32 FIRST and then carried in `dtype`."""
import numpy as np

MAX_SAMPLES = 2 ** 20


def cell_size(c1, c2, reso, dtype=np.float64):
    """h = (c2 - c1) / (n - 1) per axis from the fp32 corners: rounded once from fp64"""
    c1, c2 = np.asarray(c1, np.float32).astype(np.float64), np.asarray(c2, np.float32).astype(np.float64)
    return ((c2 - c1) / (np.asarray(reso, np.float64) - 1.0)).astype(dtype)


def render_ref(rays, vol, c1, c2, step, white_bkgd=False, occupied=None, terminate=0.0, dtype=np.float64):
    """rays (R,8), vol (nx,ny,nz,4), occupied None or (nx-1,ny-1,nz-1) bool, terminate eps in [0,1)
    -> rgb (R,3), depth (R,), alpha (R,) in `dtype`"""
    dt = np.dtype(dtype).type
    rays = np.asarray(rays, np.float32).astype(dtype)
    vol = np.asarray(vol, np.float32).astype(dtype)
    reso = vol.shape[:3]
    c1 = np.asarray(c1, np.float32).astype(dtype)
    c2 = np.asarray(c2, np.float32).astype(dtype)
    h = cell_size(c1, c2, reso, dtype)
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
                    v = vol[ix:ix + 2, iy:iy + 2, iz:iz + 2]   # (2,2,2,4)
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


# ---------------------------------------------------------------- the inputs of tests/test_hip_baked.py (checked on the host too)
RESO = (9, 8, 7)                 # three different axis lengths: a swapped axis or stride shows
C1, C2 = (-1.0, -0.8, -0.6), (1.1, 0.9, 0.7)
# (near, far, step): n = ceil(132.5) = 133 -- two full chunks and a tail of 5 -- and n = ceil(39.5) = 40, less than one chunk
SETTINGS = {"n133": (1.2, 1.2 + 132.5 * 0.03, 0.03), "n40": (1.2, 1.2 + 39.5 * 0.1, 0.1)}
N_SAMPLES = {"n133": 133, "n40": 40}


def common_volume(seed=20240607):
    """seeded rgb in [0,1] and sigma in [0,30]; sigma exactly 0 on the two outermost layers of points of every face (fp32 and
    fp64 may disagree on whether a sample near a face is inside the box: it cannot change a value) and in the 3x3x3 block of
    points [2:5, 2:5, 2:5]"""
    rs = np.random.RandomState(seed)
    vol = np.empty(RESO + (4,), np.float32)
    vol[..., :3] = rs.uniform(0.0, 1.0, RESO + (3,))
    sigma = rs.uniform(0.0, 30.0, RESO).astype(np.float32)
    keep = np.zeros(RESO, bool)
    keep[2:-2, 2:-2, 2:-2] = True
    keep[2:5, 2:5, 2:5] = False
    vol[..., 3] = np.where(keep, sigma, 0.0)
    return vol


def common_rays(setting, seed=77):
    """the R = 37 rays: 26 that hit from 3 camera positions, 4 that miss the box, 2 with the origin inside it, 3 axis-parallel ones
    (two zero direction components), 1 lying in a cell plane, 1 with near >= far"""
    near, far, _ = SETTINGS[setting]
    rs = np.random.RandomState(seed)
    lo, hi = np.array(C1), np.array(C2)
    rows = []

    def add(o, d, nr=near, fr=far, normalise=True):
        d = np.asarray(d, np.float64)
        rows.append(np.concatenate((np.asarray(o, np.float64), d / np.linalg.norm(d) if normalise else d, [nr, fr])))

    cams = [(3.0, 0.3, 0.2), (-0.5, 2.8, 1.0), (0.4, -1.0, 2.9)]
    for k in range(26):                                   # hits: towards a point of the inner part of the box
        cam = np.array(cams[k % 3])
        target = lo + (0.25 + 0.5 * rs.uniform(size=3)) * (hi - lo)
        add(cam, target - cam)
    add((3.0, 0.3, 0.2), (1.0, 0.0, 0.0))                 # misses: away from the box, past it on three sides
    add((3.0, 3.0, 0.0), (-1.0, 0.0, 0.0))
    add((0.0, -3.0, 2.0), (0.0, 1.0, 0.0))
    add((-3.0, 0.1, -2.5), (1.0, 0.0, 0.02))
    add((0.1, 0.05, 0.0), (0.3, -0.2, 0.9), nr=0.0, fr=far - near)   # origins inside the box
    add((-0.4, 0.3, -0.1), (-1.0, 0.5, 0.25), nr=0.0, fr=far - near)
    add((-3.0, 0.13, 0.07), (1.0, 0.0, 0.0), normalise=False)        # axis-parallel
    add((0.37, -3.1, 0.21), (0.0, 1.0, 0.0), normalise=False)
    add((0.52, 0.33, 3.2), (0.0, 0.0, -1.0), normalise=False)
    plane_y = np.float32(C1[1]) + np.float32(3.0) * cell_size(C1, C2, RESO, np.float32)[1]   # the plane between cells j = 2 and 3
    add((-3.0, plane_y, 0.11), (1.0, 0.0, 0.0), normalise=False)      # in a cell plane
    add((3.0, 0.3, 0.2), (-1.0, 0.0, 0.0), nr=2.0, fr=1.0)           # near >= far
    rays = np.asarray(rows, np.float32)
    assert rays.shape == (37, 8)
    return rays


def gaps(a, b):
    """max |a - b| per output of two (rgb, depth, alpha) triples, in fp64"""
    return tuple(float(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max()) for x, y in zip(a, b))
