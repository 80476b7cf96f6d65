"""Test helper (not a test): the per-sample skipping of include/pixelnerf_hip.h (pnr_occupancy_mark_samples / pnr_compact_samples /
pnr_expand_rgbsigma) restated in numpy straight from the definitions, plus the seeded inputs the host and the GPU tests share.

`mark_ref` follows the header operation by operation in fp32 -- numpy's float32 product, sum, difference and quotient are the
individually rounded IEEE operations the kernel is required to use -- so a device result is expected to EQUAL it; `ambiguous`
names the samples on which a last-place difference could change the cell (within AMBIGUOUS of a cell plane, in cell units, in
fp64), which the GPU test excludes from the equality and bounds in number."""
import numpy as np

import occ_ref

AMBIGUOUS = 1e-4     # cell units


def _grid(shape_cells, c1, c2):
    c1 = np.asarray(c1, dtype=np.float32)
    c2 = np.asarray(c2, dtype=np.float32)
    n = np.asarray(shape_cells, dtype=np.int64) + 1                   # grid points per axis
    h = ((c2.astype(np.float64) - c1.astype(np.float64)) / (n - 1).astype(np.float64)).astype(np.float32)
    return c1, c2, n, h


def mark_ref(rays, z, occ, c1, c2):
    """rays (R,8), z (R,K), occ (cx,cy,cz) bool -> keep (R,K) uint8.  P = o + z d (product and sum rounded to fp32 separately);
    keep = 1 iff c1 <= P <= c2 on every axis and the cell clamp(floor((P - c1) / h), 0, n - 2) is occupied; a sample with a
    non-finite z, origin or direction component: 1."""
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 8)
    z = np.asarray(z, dtype=np.float32).reshape(rays.shape[0], -1)
    occ = np.asarray(occ, dtype=bool)
    c1, c2, n, h = _grid(occ.shape, c1, c2)
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    with np.errstate(all="ignore"):
        finite = np.isfinite(z) & np.isfinite(o).all(axis=2) & np.isfinite(d).all(axis=2)
        prod = (z[:, :, None] * d).astype(np.float32)
        P = (o + prod).astype(np.float32)
        inside = ((P >= c1) & (P <= c2)).all(axis=2)
        q = ((P - c1).astype(np.float32) / h).astype(np.float32)
        cell = np.floor(q)
        cell = np.where(np.isnan(cell), 0.0, cell)
        cell = np.minimum(np.maximum(cell, 0.0), (n - 2).astype(np.float32)).astype(np.int64)
    bit = occ[cell[..., 0], cell[..., 1], cell[..., 2]]
    return (~finite | (inside & bit)).astype(np.uint8)


def ambiguous(rays, z, occ_shape, c1, c2):
    """(R,K) bool: finite samples whose point lies within AMBIGUOUS of a cell plane (the box faces included) on some axis, in cell
    units, computed in fp64 from the fp32 inputs"""
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 8).astype(np.float64)
    z = np.asarray(z, dtype=np.float32).reshape(rays.shape[0], -1).astype(np.float64)
    c1f, c2f, n, _ = _grid(occ_shape, c1, c2)
    h = (c2f.astype(np.float64) - c1f.astype(np.float64)) / (n - 1)
    with np.errstate(all="ignore"):
        P = rays[:, None, 0:3] + z[:, :, None] * rays[:, None, 3:6]
        q = (P - c1f.astype(np.float64)) / h
        near_plane = (np.abs(q - np.round(q)) < AMBIGUOUS) & (q > -1.0) & (q < n)
        return np.isfinite(P).all(axis=2) & near_plane.any(axis=2)


def compact_ref(keep, rays, z):
    """-> (index (M,) int32 ascending, rays_c (M,8), z_c (M,), M)"""
    keep = np.asarray(keep).reshape(-1)
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 8)
    z = np.asarray(z, dtype=np.float32).reshape(rays.shape[0], -1)
    K = z.shape[1]
    index = np.flatnonzero(keep != 0).astype(np.int32)
    return index, rays[index // K], z.reshape(-1)[index], int(index.size)


def expand_ref(index, rgbsigma_c, N):
    out = np.zeros((int(N), 4), dtype=np.float32)
    if len(index):
        out[np.asarray(index, dtype=np.int64)] = np.asarray(rgbsigma_c, dtype=np.float32).reshape(-1, 4)
    return out


# ---------------------------------------------------------------- seeded inputs shared by the host and the GPU tests

C1, C2 = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def ball_cells(n_points=17, radius=0.5):
    """cells of the n^3-point grid over [-1,1]^3 with a corner within `radius` of the origin"""
    g = np.linspace(-1.0, 1.0, n_points)
    x, y, zz = np.meshgrid(g, g, g, indexing="ij")
    return occ_ref.build_ref((np.sqrt(x * x + y * y + zz * zz) <= radius).astype(np.float32), 0.5, 0)


def sphere_case(seed=0, n_rays=256, K=32, near=0.8, far=3.2):
    """the sphere case: origins on the sphere of radius 2, directions towards a uniform point of the ball of radius 0.8 (unit
    length), K stratified samples in [near, far] -> (rays (R,8), z (R,K), occupied cells of the 17^3 ball grid)"""
    rs = np.random.RandomState(300 + seed)
    v = rs.standard_normal((n_rays, 3))
    o = 2.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    t = rs.standard_normal((n_rays, 3))
    t = 0.8 * t / np.linalg.norm(t, axis=1, keepdims=True) * rs.uniform(size=(n_rays, 1)) ** (1.0 / 3.0)
    d = t - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n_rays, 1), near), np.full((n_rays, 1), far)], axis=1).astype(np.float32)
    z = (near + (far - near) * (np.arange(K)[None, :] + rs.uniform(size=(n_rays, K))) / K).astype(np.float32)
    return rays, z, ball_cells()


def random_grid_case(seed=0, n_rays=128, K=24):
    """a (5,6,7)-point grid over a non-cubic box (120 cells: the last word is partial) with ~30 % random bits"""
    rs = np.random.RandomState(400 + seed)
    occ = rs.uniform(size=(4, 5, 6)) < 0.30
    c1, c2 = (-0.9, -1.0, -0.7), (0.8, 1.1, 1.0)
    v = rs.standard_normal((n_rays, 3))
    o = 2.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    d = rs.uniform(-0.7, 0.7, (n_rays, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n_rays, 1), 0.5), np.full((n_rays, 1), 3.5)], axis=1).astype(np.float32)
    z = (0.5 + 3.0 * (np.arange(K)[None, :] + rs.uniform(size=(n_rays, K))) / K).astype(np.float32)
    return rays, z, occ, c1, c2


def hand_case():
    """K = 1 hand-made samples on the 9^3-point grid over [-1,1]^3 (h = 0.25, planes exact in fp32), every cell occupied but
    (0,0,0) and (7,7,7) -> (rays (R,8), z (R,1), occ, expected keep (R,) -- None where only the restatement speaks)"""
    occ = np.ones((8, 8, 8), dtype=bool)
    occ[0, 0, 0] = occ[7, 7, 7] = False
    nan, inf = np.nan, np.inf
    rows = [
        # origin, direction, z, expected
        ((0.1, 0.1, 0.1), (1.0, 0.0, 0.0), 0.3, 1),          # origin inside the box
        ((0.1, 0.2, 0.3), (0.0, 0.0, 0.0), 5.0, 1),          # zero direction: the point is the origin
        ((nan, 0.0, 0.0), (1.0, 0.0, 0.0), 1.0, 1),          # NaN origin component: kept
        ((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), inf, 1),         # infinite z: kept
        ((0.0, 0.0, -2.0), (0.0, inf, 1.0), 1.5, 1),         # infinite direction component: kept
        ((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 0.5, 0),         # before the box
        ((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 3.5, 0),         # beyond the box
        ((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 3.0, 1),         # exactly on the c2 face (z = 1): the last cell (.,.,7), occupied
        ((0.9, 0.9, -2.0), (0.0, 0.0, 1.0), 3.0, 0),         # on the c2 face in cell (7,7,7): empty
        ((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 1.0, 1),         # exactly on the c1 face (z = -1): cell (.,.,0), occupied
        ((-0.9, -0.9, -2.0), (0.0, 0.0, 1.0), 1.0, 0),       # on the c1 face in cell (0,0,0): empty
        ((-0.9, -0.9, -2.0), (0.0, 0.0, 1.0), 1.3, 1),       # one cell further (0,0,1)
        ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 1.0, 0),          # the c2 corner itself: cell (7,7,7)
        ((2.0, 0.0, 0.0), (-1.0, 0.0, 0.0), 0.5, 0),         # outside on x alone
    ]
    rays = np.array([list(o) + list(d) + [0.0, 6.0] for o, d, _, _ in rows], dtype=np.float32)
    z = np.array([[zz] for _, _, zz, _ in rows], dtype=np.float32)
    return rays, z, occ, np.array([e for _, _, _, e in rows], dtype=np.uint8)


def keep_patterns(R, K, seed=0):
    """the keep masks of the compaction test, (name, (R,K) uint8)"""
    N = R * K
    rs = np.random.RandomState(500 + seed)
    flat = {"none": np.zeros(N, np.uint8), "all": np.ones(N, np.uint8), "alternating": (np.arange(N) % 2).astype(np.uint8),
            "random_0.2": (rs.uniform(size=N) < 0.2).astype(np.uint8) * np.uint8(1 + seed % 3),  # (any non-zero byte keeps)
            "last_only": np.zeros(N, np.uint8), "first_only": np.zeros(N, np.uint8)}
    flat["last_only"][-1] = 1
    flat["first_only"][0] = 1
    return [(name, m.reshape(R, K)) for name, m in flat.items()]


COMPACT_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (256, 32), (1024, 67)]
