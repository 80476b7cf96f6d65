"""numpy restatement of the marching-cubes semantics of include/pixelnerf_hip.h (pnr_marching_cubes_count / _emit), the
yardstick of tests/test_hip_mesh.py.  The case tables are arguments (the library hands its own out through
pnr_marching_cubes_tables; tests/test_mesh_host.py checks them), everything else is restated here:

  * inside iff finite and > iso (iso as the float32 the entry takes); == iso and non-finite values are outside;
  * one vertex per grid edge whose ends differ, ordered by owning point (the lower end, linear index (i ny + j) nz + k), then
    axis x, y, z; t = (iso - f_a) / (f_b - f_a) from the lower end a -- in fp64 here, the device rounds to fp32 three times --
    with the vertex on the finite end when the other end is not finite; position = ((i,j,k) + t e_axis) * scale + c1;
  * triangles: cells in ascending linear order, table order within a cell, table winding.
"""
import numpy as np


def corner_offset(c):
    return c & 1, (c >> 1) & 1, (c >> 2) & 1


def edge_lower_corner(e):
    """(axis, (dx, dy, dz) of the lower end) of cube edge e = 4 axis + r: the other two axes, in order, carry (r & 1, r >> 1)"""
    axis, r = e >> 2, e & 3
    o = [0, 0, 0]
    u, v = [a for a in range(3) if a != axis]
    o[u], o[v] = r & 1, r >> 1
    return axis, tuple(o)


def edge_corners(e):
    axis, o = edge_lower_corner(e)
    lo = o[0] + 2 * o[1] + 4 * o[2]
    return lo, lo + (1 << axis)


def marching_cubes_ref(field, iso, edge_mask, tri, c1=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """-> vertices (nv,3) float64, triangles (nt,3) int32, n_nonfinite"""
    f = np.asarray(field, dtype=np.float32)
    nx, ny, nz = f.shape
    iso = np.float64(np.float32(iso))
    finite = np.isfinite(f)
    inside = finite & (f > np.float32(iso))
    f64 = f.astype(np.float64)
    # vertices: (point, axis) in linear order
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    vid = np.cumsum(cross.reshape(-1)).reshape(cross.shape) - 1
    ii, jj, kk, aa = np.nonzero(cross)  # row-major: exactly the vertex order
    e = np.eye(3, dtype=np.int64)[aa]
    fa = f64[ii, jj, kk]
    fb = f64[ii + e[:, 0], jj + e[:, 1], kk + e[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (iso - fa) / (fb - fa)
    t = np.where(~np.isfinite(fb), 0.0, np.where(~np.isfinite(fa), 1.0, t))
    index = np.stack((ii, jj, kk), axis=1).astype(np.float64) + t[:, None] * e
    vertices = index * np.asarray(scale, np.float64) + np.asarray(c1, np.float64)
    # triangles
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = corner_offset(c)
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    lower = [edge_lower_corner(k) for k in range(12)]
    tris = []
    for i, j, k in zip(*np.nonzero((case != 0) & (case != 255))):
        cs = case[i, j, k]
        assert edge_mask[cs] != 0
        row = tri[cs]
        for n in range(0, 16, 3):
            if row[n] < 0:
                break
            ids = []
            for ed in row[n:n + 3]:
                axis, (dx, dy, dz) = lower[ed]
                assert cross[i + dx, j + dy, k + dz, axis], "the table uses an edge that carries no vertex"
                ids.append(vid[i + dx, j + dy, k + dz, axis])
            tris.append(ids)
    triangles = np.array(tris, dtype=np.int32).reshape(-1, 3)
    return vertices, triangles, int((~finite).sum())


def mesh_topology(triangles):
    """-> (every undirected edge is shared by exactly two triangles, and traversed once in each direction; V - E + F)"""
    t = np.asarray(triangles, dtype=np.int64)
    d = np.concatenate((t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]))
    und = np.sort(d, axis=1)
    _, counts = np.unique(und, axis=0, return_counts=True)
    closed = bool((counts == 2).all()) and len(np.unique(d, axis=0)) == len(d)
    return closed, len(np.unique(t)) - len(counts) + len(t)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)
