"""Test helper (not a test): the occupancy grid of include/pixelnerf_hip.h (pnr_occupancy_build / pnr_occupancy_clip_rays) restated
in numpy fp64 straight from the definitions -- no traversal: `build_ref` is the 8-corner test and a (2d+1)^3 maximum filter,
`clip_ref` a brute-force slab test of every ray against EVERY occupied cell -- plus the seeded inputs the host and the GPU tests
share (the GPU test repeats the host test's not-vacuous condition on the very same rays)."""
import numpy as np

DELTA = 2.0 ** -12   # cells grown / shrunk by DELTA * h per side: the one-sided bracket of tests/test_hip_occupancy.py
EPS = 2.0 ** -24


def build_ref(field, threshold, dilate=0):
    """field (nx,ny,nz) -> occupied cells (nx-1,ny-1,nz-1) bool.  Raw: any of the 8 corners > threshold (fp32 compare) or not
    finite; occupied: a raw-occupied cell within Chebyshev distance `dilate`."""
    f = np.asarray(field, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        pt = ~np.isfinite(f) | (f > np.float32(threshold))
    raw = np.zeros(tuple(n - 1 for n in f.shape), dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                raw |= pt[dx:dx + raw.shape[0], dy:dy + raw.shape[1], dz:dz + raw.shape[2]]
    d = int(dilate)
    pad = np.pad(raw, d, mode="constant", constant_values=False)
    occ = np.zeros_like(raw)
    for dx in range(2 * d + 1):
        for dy in range(2 * d + 1):
            for dz in range(2 * d + 1):
                occ |= pad[dx:dx + raw.shape[0], dy:dy + raw.shape[1], dz:dz + raw.shape[2]]
    return occ


def pack_bits(occ):
    """cells (cx,cy,cz) bool -> uint32 words: cell index (i cy + j) cz + k, bit (index & 31) of word (index >> 5)"""
    flat = np.asarray(occ, dtype=bool).ravel()
    flat = np.concatenate([flat, np.zeros((-len(flat)) % 32, dtype=bool)])
    return np.packbits(flat, bitorder="little").view("<u4").astype(np.uint32)


def unpack_bits(words, cells_shape):
    n = int(np.prod(cells_shape))
    flat = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return flat[:n].astype(bool).reshape(cells_shape), flat[n:]


def clip_ref(rays, occ, c1, c2, pad=0.0, inflate=0.0, chunk=256):
    """rays (R,8), occ (cx,cy,cz) bool, c1 / c2 the box of the (cx+1,cy+1,cz+1) grid points.  Every occupied cell, grown by
    inflate * h per side (negative: shrunk), is intersected with the segment t in [near, far] (closed intervals, per-axis slabs;
    a zero direction component is inside the slab or not).  -> hit (R,) bool, t_enter, t_exit (R,) fp64: over the cells hit the
    smallest entry / largest exit parameter, then max(near, t_enter - pad) / min(far, t_exit + pad); (near, far) on a miss."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 8)
    occ = np.asarray(occ, dtype=bool)
    lo_box = np.asarray(c1, dtype=np.float32).astype(np.float64)
    hi_box = np.asarray(c2, dtype=np.float32).astype(np.float64)
    h = (hi_box - lo_box) / np.array(occ.shape, dtype=np.float64)
    cells = np.argwhere(occ).astype(np.float64)                      # (M,3)
    lo = lo_box + cells * h - inflate * h
    hi = lo_box + (cells + 1.0) * h + inflate * h
    R = rays.shape[0]
    hit = np.zeros(R, dtype=bool)
    t_enter, t_exit = rays[:, 6].copy(), rays[:, 7].copy()
    if len(cells) == 0:
        return hit, t_enter, t_exit
    for s in range(0, R, chunk):
        o, d = rays[s:s + chunk, None, 0:3], rays[s:s + chunk, None, 3:6]
        near, far = rays[s:s + chunk, 6], rays[s:s + chunk, 7]
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (lo[None] - o) / d, (hi[None] - o) / d
        zero = np.broadcast_to(d == 0.0, ta.shape)
        inside = (lo[None] <= o) & (o <= hi[None])
        t_in = np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
        t_out = np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
        te = np.maximum(t_in.max(axis=2), near[:, None])             # (r,M)
        tx = np.minimum(t_out.min(axis=2), far[:, None])
        ok = te <= tx
        hit[s:s + chunk] = ok.any(axis=1)
        e = np.where(ok, te, np.inf).min(axis=1)
        x = np.where(ok, tx, -np.inf).max(axis=1)
        any_ = ok.any(axis=1)
        t_enter[s:s + chunk] = np.where(any_, np.maximum(near, e - pad), near)
        t_exit[s:s + chunk] = np.where(any_, np.minimum(far, x + pad), far)
    return hit, t_enter, t_exit


# ---------------------------------------------------------------- seeded inputs shared by the host and the GPU tests

C1, C2, RESO = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (9, 9, 9)


def random_cells(seed=0, frac=0.10, shape=(8, 8, 8)):
    """the occupied cells of the 9x9x9 clip fixture: about `frac` of them, independently"""
    return np.random.RandomState(1000 + seed).uniform(size=shape) < frac


def _unit(rs, n):
    v = rs.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def sphere_rays(seed=0, n=4096, near=0.5, far=4.5, radius=2.5, aim=1.2):
    """origins on the sphere of `radius`, aimed at uniform points of [-aim, aim]^3, unit directions -> (n,8) float32"""
    rs = np.random.RandomState(seed)
    o = radius * _unit(rs, n)
    d = rs.uniform(-aim, aim, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d, np.full((n, 1), near), np.full((n, 1), far)], axis=1).astype(np.float32)


def inside_rays(occ, seed=0, n=256, far=3.0):
    """origins inside the box; the first quarter inside occupied cells (near their centres), near = 0"""
    rs = np.random.RandomState(50 + seed)
    o = rs.uniform(-1.0, 1.0, (n, 3))
    cells = np.argwhere(occ)
    if len(cells):
        h = 2.0 / np.array(occ.shape)
        pick = cells[rs.randint(0, len(cells), n // 4)]
        o[:n // 4] = -1.0 + (pick + 0.5 + rs.uniform(-0.3, 0.3, (n // 4, 3))) * h
    d = _unit(rs, n)
    return np.concatenate([o, d, np.zeros((n, 1)), np.full((n, 1), far)], axis=1).astype(np.float32)


def axis_rays(seed=0, n_random=96):
    """axis-parallel rays through the box, both directions of every axis: random transverse positions, and transverse positions
    EXACTLY on cell planes (c1 + i h is exact in fp32 for this grid), the box faces included"""
    rs = np.random.RandomState(70 + seed)
    planes = -1.0 + 0.25 * np.arange(9)
    rows = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        trans = [tuple(t) for t in rs.uniform(-1.0, 1.0, (n_random // 3, 2))]
        trans += [(p, float(q)) for p in planes for q in rs.uniform(-1.0, 1.0, 2)]        # in a plane of u
        trans += [(float(q), p) for p in planes for q in rs.uniform(-1.0, 1.0, 2)]        # in a plane of v
        trans += [(p, q) for p in planes[::2] for q in planes[::4]]                       # along a cell edge
        for n, (a, b) in enumerate(trans):
            sign = 1.0 if n % 2 == 0 else -1.0
            o, d = np.zeros(3), np.zeros(3)
            o[axis], o[u], o[v] = -2.0 * sign, a, b
            d[axis] = sign
            rows.append(np.concatenate([o, d, [0.25, 3.75]]))
    return np.array(rows, dtype=np.float32)


def missing_rays(seed=0, n=256):
    """rays that pass the box at a distance: the line's closest point to the centre is 1.8 .. 2.4 away (the box's corners are
    at sqrt(3)), the origin 2.5 before that point"""
    rs = np.random.RandomState(90 + seed)
    q = _unit(rs, n)
    d = np.cross(q, _unit(rs, n))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = rs.uniform(1.8, 2.4, (n, 1)) * q - 2.5 * d
    return np.concatenate([o, d, np.full((n, 1), 0.5), np.full((n, 1), 4.5)], axis=1).astype(np.float32)


def unclassifiable_rays():
    """a NaN / inf component, a zero direction, near >= far: the device must answer hit = 1 with unchanged bounds"""
    base = np.array([0.0, 0.0, -2.5, 0.0, 0.0, 1.0, 0.5, 4.5], dtype=np.float32)
    rows = []
    for col, val in ((0, np.nan), (4, np.nan), (6, np.nan), (7, np.inf), (2, -np.inf), (5, np.inf)):
        r = base.copy()
        r[col] = val
        rows.append(r)
    z = base.copy()
    z[3:6] = 0.0
    rows.append(z)
    for near, far in ((4.5, 0.5), (2.0, 2.0)):
        r = base.copy()
        r[6], r[7] = near, far
        rows.append(r)
    far_away = base.copy()
    far_away[0] = 50.0                                               # (misses the box, and is classifiable: the control)
    rows.append(far_away)
    return np.array(rows, dtype=np.float32)


def vacuity(rays, occ, c1=C1, c2=C2, pad=0.0):
    """-> (share of rays whose hit flag differs between the grown and the shrunk cells, share hit by the shrunk cells)"""
    grown = clip_ref(rays, occ, c1, c2, pad, +DELTA)[0]
    shrunk = clip_ref(rays, occ, c1, c2, pad, -DELTA)[0]
    return float((grown != shrunk).mean()), float(shrunk.mean())


def check_clip(rays, occ, pad, dev_hit, dev_bounds, c1=C1, c2=C2, what=""):
    """The one-sided bracket of a device result (hit (R,), t_bounds (R,2)) between the restatement on cells shrunk and grown by
    DELTA * h, without exclusions: hit(-DELTA) => hit_device => hit(+DELTA), and for the rays hit on both sides
    t_enter in [t_enter(+DELTA) - tau, t_enter(-DELTA) + tau], t_exit in [t_exit(-DELTA) - tau, t_exit(+DELTA) + tau] with
    tau = 8 * 2^-24 * max(1, |t|); a miss keeps (near, far).  Prints the figures before it asserts.
    -> (ambiguous share, share hit by the shrunk cells)"""
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 8)
    dev_hit = np.asarray(dev_hit).reshape(-1).astype(bool)
    tb = np.asarray(dev_bounds, dtype=np.float64).reshape(-1, 2)
    g_hit, g_en, g_ex = clip_ref(rays, occ, c1, c2, pad, +DELTA)
    s_hit, s_en, s_ex = clip_ref(rays, occ, c1, c2, pad, -DELTA)
    both = s_hit & g_hit
    tau = lambda t: 8 * EPS * np.maximum(1.0, np.abs(t))  # noqa: E731
    en_lo, en_hi = g_en - tau(g_en), s_en + tau(s_en)
    ex_lo, ex_hi = s_ex - tau(s_ex), g_ex + tau(g_ex)
    en_out = np.maximum(en_lo - tb[:, 0], tb[:, 0] - en_hi)[both]
    ex_out = np.maximum(ex_lo - tb[:, 1], tb[:, 1] - ex_hi)[both]
    print(f"clip {what}: {len(rays)} rays, hit device {dev_hit.mean():.4f} shrunk {s_hit.mean():.4f} grown {g_hit.mean():.4f}, "
          f"ambiguous {(s_hit != g_hit).mean():.5f}; worst excess over the bracket: t_enter "
          f"{en_out.max() if both.any() else 0.0:.3e}, t_exit {ex_out.max() if both.any() else 0.0:.3e} (<= 0 passes)")
    assert not (s_hit & ~dev_hit).any(), f"{what}: {int((s_hit & ~dev_hit).sum())} rays hit by the shrunk cells are culled"
    assert not (dev_hit & ~g_hit).any(), f"{what}: {int((dev_hit & ~g_hit).sum())} rays kept that miss the grown cells"
    assert (en_out <= 0).all() and (ex_out <= 0).all(), what
    miss = ~dev_hit
    assert np.array_equal(tb[miss, 0], rays[miss, 6].astype(np.float64)) and np.array_equal(tb[miss, 1], rays[miss, 7].astype(np.float64)), what
    assert (tb[:, 0] >= rays[:, 6]).all() and (tb[:, 1] <= rays[:, 7]).all(), what
    return float((s_hit != g_hit).mean()), float(s_hit.mean())


def clip_cases(seed=0):
    """every (name, rays (R,8) float32, occupied cells) of the clip test; each is run at pad 0 and 0.1"""
    occ = random_cells(seed)
    main = sphere_rays(seed)
    cut = main.copy()
    cut[:, 6], cut[:, 7] = 2.2, 2.8
    single = np.zeros_like(occ)
    single[5, 2, 3] = True
    return [("sphere", main, occ), ("near_far_cut", cut, occ), ("inside", inside_rays(occ, seed), occ),
            ("axis_parallel", axis_rays(seed), occ), ("missing", missing_rays(seed), occ),
            ("single_cell", main[:1024], single), ("full_grid", np.concatenate([main[:512], axis_rays(seed)[::3]]), np.ones_like(occ)),
            ("empty_grid", main[:512], np.zeros_like(occ))]
