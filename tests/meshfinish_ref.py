"""Test helper (not a test): CPU restatements of what include/pixelnerf_hip.h says about pnr_grid_components and pnr_grid_normals,
and the seeded inputs that tests/test_meshfinish_host.py and tests/test_hip_meshfinish.py share.

  * components_ref: scipy.ndimage.label with its default 6-connected structure -- an independent algorithm, not a port of the
    kernel's union-find -- relabelled to the smallest linear index of every component with ndimage.minimum over an index grid;
  * components_bfs: a plain breadth-first flood fill, the check of the relabelling;
  * normals_ref: the gradient formula in the dtype asked for (float64: the yardstick; float32: how much plain fp32 arithmetic loses
    against it, which sets the bar of the GPU test);
  * remove_floaters_ref: the selection rule of util.recon.remove_floaters on the CPU labels.
"""
import collections

import numpy as np


def inside_mask(field, threshold):
    """finite and > threshold (threshold as the float32 the entry takes); == threshold, NaN and +-inf are outside"""
    f = np.asarray(field, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(f) & (f > np.float32(threshold))


def components_ref(field, threshold):
    """-> (labels (nx,ny,nz) int32: -1 outside, else the smallest linear index of the voxel's component; sizes (N,) int32: the
    voxel count at that index, 0 elsewhere; (n_inside, n_components))"""
    from scipy import ndimage
    inside = inside_mask(field, threshold)
    lab, n = ndimage.label(inside)                     # default structure: 6-connectivity
    index = np.arange(inside.size, dtype=np.int64).reshape(inside.shape)
    labels = np.full(inside.shape, -1, dtype=np.int32)
    sizes = np.zeros(inside.size, dtype=np.int32)
    if n:
        ids = np.arange(1, n + 1)
        roots = np.asarray(ndimage.minimum(index, lab, ids)).astype(np.int64).reshape(-1)
        lut = np.concatenate(([-1], roots))
        labels = lut[lab].astype(np.int32)
        sizes[roots] = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    return labels, sizes, (int(inside.sum()), int(n))


def components_bfs(field, threshold):
    """the same three results by a flood fill in ascending linear order: the first voxel of a component met is its smallest"""
    inside = inside_mask(field, threshold)
    nx, ny, nz = inside.shape
    labels = np.full(inside.shape, -1, dtype=np.int32)
    sizes = np.zeros(inside.size, dtype=np.int32)
    n = 0
    for start in range(inside.size):
        s = np.unravel_index(start, inside.shape)
        if not inside[s] or labels[s] >= 0:
            continue
        n += 1
        labels[s] = start
        queue, count = collections.deque([s]), 0
        while queue:
            i, j, k = queue.popleft()
            count += 1
            for q in ((i - 1, j, k), (i + 1, j, k), (i, j - 1, k), (i, j + 1, k), (i, j, k - 1), (i, j, k + 1)):
                if 0 <= q[0] < nx and 0 <= q[1] < ny and 0 <= q[2] < nz and inside[q] and labels[q] < 0:
                    labels[q] = start
                    queue.append(q)
        sizes[start] = count
    return labels, sizes, (int(inside.sum()), n)


def select_components(sizes, keep_largest=None, min_voxels=None):
    """roots kept by util.recon.remove_floaters: at least min_voxels voxels AND among the keep_largest biggest, ties in size to the
    smaller root index"""
    roots = np.flatnonzero(sizes > 0)
    order = roots[np.argsort(-sizes[roots].astype(np.int64), kind="stable")]
    if keep_largest is not None:
        order = order[:int(keep_largest)]
    if min_voxels is not None:
        order = order[sizes[order] >= int(min_voxels)]
    return np.sort(order)


def remove_floaters_ref(field, isosurface, keep_largest=None, min_voxels=None):
    """-> (filtered field, kept-voxel mask, labels): every voxel of a dropped component set to isosurface"""
    f = np.array(field, dtype=np.float32)
    labels, sizes, _ = components_ref(f, isosurface)
    kept = np.isin(labels, select_components(sizes, keep_largest, min_voxels))
    f[(labels >= 0) & ~kept] = np.float32(isosurface)
    return f, kept, labels


def normals_ref(field, vertices, c1, scale, dtype=np.float64):
    """pnr_grid_normals restated with every operation in `dtype`: p = (v - c1) / scale clamped to the grid, cell = floor(p) clamped
    to n - 2, central differences (one-sided at the border), trilinear blend a + t (b - a) along x, y, z, component a divided by
    scale[a], normal = -g / |g|, (0,0,0) where g is zero or not finite.  c1, scale enter as the float32 values the entry takes.
    -> (normals (V,3) dtype, |g| (V,) float64, cells (V,3) int)"""
    f = np.asarray(field, dtype=np.float32).astype(dtype)
    v = np.asarray(vertices, dtype=np.float32).astype(dtype)
    lo = np.asarray(c1, dtype=np.float32).astype(dtype)
    sc = np.asarray(scale, dtype=np.float32).astype(dtype)
    n = np.array(f.shape)
    half = dtype(0.5)
    grads = []
    for a in range(3):
        m = np.moveaxis(f, a, 0)
        d = np.empty_like(m)
        d[1:-1] = (m[2:] - m[:-2]) * half
        d[0] = m[1] - m[0]
        d[-1] = m[-1] - m[-2]
        grads.append(np.moveaxis(d, 0, a))
    p = (v - lo) / sc
    p = np.minimum(np.maximum(p, dtype(0)), (n - 1).astype(dtype))
    cell = np.minimum(np.floor(p).astype(np.int64), n - 2)
    t = p - cell.astype(dtype)
    g = np.empty_like(v)
    i, j, k = cell[:, 0], cell[:, 1], cell[:, 2]
    lerp = lambda a, b, w: a + w * (b - a)  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(3):
            G = grads[a]
            c = [G[i + (q & 1), j + (q >> 1 & 1), k + (q >> 2)] for q in range(8)]
            x00, x10 = lerp(c[0], c[1], t[:, 0]), lerp(c[2], c[3], t[:, 0])
            x01, x11 = lerp(c[4], c[5], t[:, 0]), lerp(c[6], c[7], t[:, 0])
            g[:, a] = lerp(lerp(x00, x10, t[:, 1]), lerp(x01, x11, t[:, 1]), t[:, 2]) / sc[a]
        nrm = np.sqrt((g * g).sum(axis=1, dtype=dtype))
        ok = np.isfinite(nrm) & (nrm > 0)
        normals = np.where(ok[:, None], -g / np.where(ok, nrm, dtype(1))[:, None], dtype(0)).astype(dtype)
    return normals, np.where(ok, nrm, 0.0).astype(np.float64), cell


# ---------------------------------------------------------------- shared inputs

def pattern_2x2x2(case, threshold=0.5):
    """corner c = dx + 2 dy + 4 dz inside iff bit c of `case`; the outside corners take, in corner order, the value == threshold,
    NaN, +inf, then values below: each of the three must count as outside"""
    outside = iter([threshold, np.nan, np.inf])
    f = np.empty((2, 2, 2), dtype=np.float32)
    for c in range(8):
        f[c & 1, c >> 1 & 1, c >> 2] = threshold + 1.0 + c if case >> c & 1 else next(outside, threshold - 1.0 - c)
    return f


RANDOM_CASES = (((5, 6, 7), 0.45, 0), ((17, 9, 33), 0.32, 1), ((64, 64, 64), 0.32, 2))


def random_field(shape, p, seed):
    """Bernoulli(p) voxels as a 0 / 1 field (threshold 0.5): p = 0.32 sits at the 6-connected percolation threshold"""
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) > 1 - p).astype(np.float32)


def serpentine():
    """(2,33,33), plane x = 1 empty; in plane x = 0 every even row y is inside, every odd row has ONE inside voxel, alternately at
    z = 32 and z = 0: one chain of 17 * 33 + 16 = 577 voxels"""
    f = np.zeros((2, 33, 33), dtype=np.float32)
    f[0, 0::2, :] = 1.0
    for n, y in enumerate(range(1, 33, 2)):
        f[0, y, 32 if n % 2 == 0 else 0] = 1.0
    return f


def serpentine_variants():
    """the chain as it is; flipped along y and z (the pattern is symmetric under that flip: the same field, walked from the other
    end); transposed in (y, z) and flipped along y, where voxel 0 -- the label -- has two chain neighbours, i.e. the smallest
    index lies INSIDE the chain (33 voxels from its start), not at an end"""
    s = serpentine()
    return {"as it is": s, "flipped y z": np.ascontiguousarray(s[:, ::-1, ::-1]),
            "transposed, flipped y": np.ascontiguousarray(s.transpose(0, 2, 1)[:, ::-1, :])}


def smooth_field(shape, seed):
    """seeded random values filtered once with a 3-tap box along every axis (tests/test_hip_mesh.py's field)"""
    rs = np.random.RandomState(seed)
    f = rs.standard_normal([n + 2 for n in shape])
    f = (f[:-2] + f[1:-1] + f[2:]) / 3.0
    f = (f[:, :-2] + f[:, 1:-1] + f[:, 2:]) / 3.0
    f = (f[:, :, :-2] + f[:, :, 1:-1] + f[:, :, 2:]) / 3.0
    return f.astype(np.float32)


def solid(name, n=33):
    """100 x signed distance (inside positive) of a sphere r = 0.6 / a torus (0.55, 0.25) on n^3 over [-1,1]^3, and the analytic
    outward normal as a function of points (V,3)"""
    g = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    if name == "sphere":
        f = 0.6 - np.sqrt(x * x + y * y + z * z)
        normal = lambda p: p / np.linalg.norm(p, axis=1, keepdims=True)  # noqa: E731
    else:
        f = 0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)

        def normal(p):
            rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
            d = np.stack((p[:, 0] * (1 - 0.55 / rho), p[:, 1] * (1 - 0.55 / rho), p[:, 2]), axis=1)
            return d / np.linalg.norm(d, axis=1, keepdims=True)
    return (100.0 * f).astype(np.float32), normal


def floater_scene(n=33):
    """33^3 over [-1,1]^3, iso 0: a sphere r = 0.5 at the origin, a sphere r = 0.12 near a corner, three isolated single voxels
    above the level.  field = 100 x (largest signed distance), the single voxels at +5.  -> (field, c1, scale)"""
    g = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    big = 0.5 - np.sqrt(x * x + y * y + z * z)
    small = 0.12 - np.sqrt((x - 0.75) ** 2 + (y - 0.75) ** 2 + (z - 0.75) ** 2)
    f = (100.0 * np.maximum(big, small)).astype(np.float32)
    for idx in ((2, 3, 4), (29, 3, 16), (4, 28, 7)):
        f[idx] = 5.0
    h = 2.0 / (n - 1)
    return f, (-1.0, -1.0, -1.0), (h, h, h)


def mesh_components(triangles, n_vertices):
    """number of connected components of the mesh's vertex graph (vertices no triangle uses count one each)"""
    parent = np.arange(n_vertices)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for t in np.asarray(triangles, dtype=np.int64):
        r = sorted(find(int(a)) for a in t)
        parent[r[1]] = parent[r[2]] = r[0]
    return len({find(a) for a in range(n_vertices)})


def crossed_edges(inside):
    """(nx,ny,nz,3) bool: the grid edge from a point towards +axis carries a vertex; row-major order = the mesher's vertex order"""
    cross = np.zeros(inside.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    return cross
