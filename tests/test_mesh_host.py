"""Host tests (no GPU) of the mesh extraction: the contract of the marching-cubes case tables the kernels use (read through
pnr_marching_cubes_tables), util.gen_grid, recon.save_obj and the refusals of the new C entries before any HIP call.

The table contract is what makes the mesh closed: (1) a case's triangles use exactly the cube edges whose ends differ; (2) on
every cube face the boundary of the case's patch -- as directed segments between the face's edges -- is ONE function of the
face's four inside flags, the same for all six faces (faces mapped onto each other by the cyclic axis order, which keeps
handedness) and, with the direction reversed, for the two cells that share a face; (3) every triangle edge that is not such a
boundary segment is used exactly twice, once in each direction."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mc_ref as M
from pixelnerf_amd import _lib, ops


@pytest.fixture(scope="module")
def tables():
    _lib.build_library()
    return ops.marching_cubes_tables()


def _case_edges(tri_row):
    """-> directed triangle edges [(a, b)] of one case"""
    out = []
    for n in range(0, 16, 3):
        if tri_row[n] < 0:
            assert (tri_row[n:] == -1).all()
            break
        a, b, c = (int(v) for v in tri_row[n:n + 3])
        assert len({a, b, c}) == 3
        out += [(a, b), (b, c), (c, a)]
    return out


def _face_local(e, axis, side):
    """cube edge e on face (axis, side) in face-local terms, or None when it is not on the face: (u, v) = the next two axes in
    cyclic order (right-handed with the axis); -> ('u' | 'v' = the edge's direction, its position along the other one)"""
    ea, o = M.edge_lower_corner(e)
    if ea == axis or o[axis] != side:
        return None
    u, v = (axis + 1) % 3, (axis + 2) % 3
    return ("u", o[v]) if ea == u else ("v", o[u])


def test_triangles_use_exactly_the_crossed_edges(tables):
    edge_mask, tri = tables
    assert tri.shape == (256, 16) and (tri[:, 15] == -1).all() and tri.min() == -1 and tri.max() == 11
    for cs in range(256):
        crossed = {e for e in range(12) if ((cs >> M.edge_corners(e)[0]) & 1) != ((cs >> M.edge_corners(e)[1]) & 1)}
        assert {e for e in range(12) if edge_mask[cs] >> e & 1} == crossed, cs
        assert {a for a, _ in _case_edges(tri[cs])} == crossed, cs
    assert not _case_edges(tri[0]) and not _case_edges(tri[255])


def test_face_boundaries_are_one_function_of_the_face_flags_and_interiors_close(tables):
    _, tri = tables
    rule = {}
    for cs in range(256):
        directed = _case_edges(tri[cs])
        uses = {}
        for a, b in directed:
            uses.setdefault(frozenset((a, b)), []).append((a, b))
        on_face = {(axis, side): set() for axis in range(3) for side in (0, 1)}
        for key, lst in uses.items():
            if len(lst) == 2:  # interior: once in each direction
                assert lst[0] == lst[1][::-1], (cs, lst)
                continue
            assert len(lst) == 1, (cs, lst)
            a, b = lst[0]
            faces = [fs for fs in on_face if _face_local(a, *fs) and _face_local(b, *fs)]
            assert len(faces) == 1, f"case {cs}: the edge {a}-{b} is used once but lies on no face"
            on_face[faces[0]].add((a, b))
        for (axis, side), segs in on_face.items():
            u, v = (axis + 1) % 3, (axis + 2) % 3
            flags = []
            for fv in (0, 1):
                for fu in (0, 1):
                    o = [0, 0, 0]
                    o[axis], o[u], o[v] = side, fu, fv
                    flags.append((cs >> (o[0] + 2 * o[1] + 4 * o[2])) & 1)
            # seen from the cell on the high side of the face (whose LOW face it is) the neighbour's segments run the other way
            local = frozenset((_face_local(a, axis, side), _face_local(b, axis, side)) if side == 1 else
                              (_face_local(b, axis, side), _face_local(a, axis, side)) for a, b in segs)
            assert rule.setdefault(tuple(flags), local) == local, f"case {cs} face {(axis, side)} flags {flags}"
    assert len(rule) == 16
    for flags, local in rule.items():
        n_in = sum(flags)
        diagonal = n_in == 2 and flags[0] == flags[3]
        assert len(local) == (0 if n_in in (0, 4) else 2 if diagonal else 1), flags


def test_single_corner_winds_outwards(tables):
    """case 1 (corner 0 inside): with the vertices at the edge midpoints the normal points away from the corner"""
    _, tri = tables
    mid = lambda e: (np.array(M.corner_offset(M.edge_corners(e)[0])) + np.array(M.corner_offset(M.edge_corners(e)[1]))) / 2.0  # noqa: E731
    v0, v1, v2 = (mid(int(e)) for e in tri[1][:3])
    assert np.cross(v1 - v0, v2 - v0) @ np.ones(3) > 0
    v0, v1, v2 = (mid(int(e)) for e in tri[254][:3])
    assert np.cross(v1 - v0, v2 - v0) @ np.ones(3) < 0


def test_restatement_gives_closed_outward_meshes(tables):
    """the numpy restatement with these tables on two analytic solids (the GPU tests repeat this on the device's output)"""
    edge_mask, tri = tables
    g = np.linspace(-1.0, 1.0, 17)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    for name, field, euler in (("sphere", 0.6 - np.sqrt(x * x + y * y + z * z), 2),
                               ("torus", 0.2 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z), 0)):
        v, t, nonfinite = M.marching_cubes_ref(field.astype(np.float32), 0.0, edge_mask, tri)
        closed, chi = M.mesh_topology(t)
        assert nonfinite == 0 and closed and chi == euler and M.signed_volume(v, t) > 0, name


@pytest.mark.parametrize("args,ij", [(((-1, 1, 5), (-1, 1, 4), (-1, 1, 3)), True), (((0, 1, 10), (-1, 1, 20)), False),
                                     (((-0.3, 0.7, 7), (2, 2, 3), (1, -1, 1)), True)])
def test_gen_grid_is_the_reference_expression(args, ij):
    """src/util/util.py:93-110 restated with numpy: float32 linspace per axis, meshgrid, one row per point"""
    from pixelnerf_amd import util
    got = util.gen_grid(*args, ij_indexing=ij)
    axes = [np.linspace(lo, hi, sz, dtype=np.float32) for lo, hi, sz in args]
    mesh = np.meshgrid(*axes, indexing="ij" if ij else "xy")
    ref = np.vstack(mesh).reshape(len(args), -1).T
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    assert np.array_equal(got.numpy(), ref)
    if ij and len(args) == 3:  # x is the slowest axis
        n = args[2][2]
        assert np.array_equal(got.numpy()[:n, 2], axes[2]) and (got.numpy()[:n, 0] == axes[0][0]).all()


@pytest.mark.parametrize("colour", [False, True])
def test_save_obj_round_trip(tmp_path, colour):
    from pixelnerf_amd.util import recon
    rs = np.random.RandomState(3)
    v = rs.uniform(-2, 2, (37, 3))
    v[0] = (0.00005, -0.00005, 1.0)  # rounding of %.4f on both sides of zero
    t = rs.randint(0, 37, (55, 3)).astype(np.int32)
    rgb = rs.uniform(0, 1, (37, 3)) if colour else None
    path = tmp_path / "mesh.obj"
    recon.save_obj(v, t, str(path), vert_rgb=rgb)
    lines = []  # the reference's writer, line by line (src/util/recon.py:90-106)
    for i, p in enumerate(v):
        if colour:
            lines.append("v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (p[0], p[1], p[2], rgb[i][0], rgb[i][1], rgb[i][2]))
        else:
            lines.append("v %.4f %.4f %.4f\n" % (p[0], p[1], p[2]))
    for f in t:
        lines.append("f %d %d %d\n" % (f[0] + 1, f[1] + 1, f[2] + 1))
    text = path.read_text()
    assert text == "".join(lines)
    back_v = np.array([[float(w) for w in ln.split()[1:4]] for ln in text.splitlines() if ln.startswith("v ")])
    back_f = np.array([[int(w) for w in ln.split()[1:]] for ln in text.splitlines() if ln.startswith("f ")])
    assert np.abs(back_v - v).max() <= 0.5e-4 + 1e-12 and np.array_equal(back_f - 1, t)
    recon.save_obj(torch.from_numpy(v), torch.from_numpy(t), str(path), vert_rgb=None if rgb is None else torch.from_numpy(rgb))
    assert path.read_text() == text  # tensors are accepted as well


def test_entries_refuse_bad_arguments_on_the_host():
    """PNR_E_INVALID (-1) before any HIP call; the addresses are dummies, never dereferenced"""
    _lib.build_library()
    lib = _lib.load()
    one, zero = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(0, 0, 0)
    count = lambda field=64, n=(4, 4, 4), iso=0.0, ws=64, counts=64: lib.pnr_marching_cubes_count(  # noqa: E731
        field, n[0], n[1], n[2], iso, ws, counts, None)
    emit = lambda field=64, n=(4, 4, 4), iso=0.0, c1=zero, sc=one, ws=64, v=64, t=64: lib.pnr_marching_cubes_emit(  # noqa: E731
        field, n[0], n[1], n[2], iso, c1, sc, ws, v, t, None)
    for n in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, -2, 4)):
        assert count(n=n) == -1 and b"at least 2" in lib.pnr_last_error(), n
        assert emit(n=n) == -1 and b"at least 2" in lib.pnr_last_error(), n
        assert lib.pnr_marching_cubes_workspace_bytes(*n) == 0
    big = (895, 895, 895)  # 3 * 895^3 = 2 150 752 125 >= 2^31; 894^3 stays below
    assert 3 * 895 ** 3 >= 2 ** 31 > 3 * 894 ** 3
    assert count(n=big) == -1 and b"2^31" in lib.pnr_last_error()
    assert emit(n=big) == -1 and b"2^31" in lib.pnr_last_error()
    assert lib.pnr_marching_cubes_workspace_bytes(*big) == 0
    assert lib.pnr_marching_cubes_workspace_bytes(894, 894, 894) > 12 * 894 ** 3
    assert count(field=None) == -1 and b"field" in lib.pnr_last_error()
    assert count(ws=None) == -1 and b"workspace" in lib.pnr_last_error()
    assert count(ws=60) == -1 and b"aligned" in lib.pnr_last_error()
    assert count(counts=None) == -1 and b"counts_dev" in lib.pnr_last_error()
    assert count(iso=float("nan")) == -1 and b"iso" in lib.pnr_last_error()
    assert emit(field=None) == -1 and emit(ws=None) == -1 and emit(v=None) == -1 and emit(t=None) == -1
    assert emit(c1=None) == -1 and b"c1" in lib.pnr_last_error()
    assert emit(sc=None) == -1 and emit(iso=float("inf")) == -1
    # the workspace: 12 bytes per grid point + 12 per scan block of 1024 points, padded to 8
    assert lib.pnr_marching_cubes_workspace_bytes(9, 8, 7) == 504 * 8 + 504 * 4 + 8 + 8
    assert lib.pnr_marching_cubes_tables(None, None) == -1
    lo, hi, reso = (ctypes.c_double * 3)(-1, -1, -1), (ctypes.c_double * 3)(1, 1, 1), (ctypes.c_int * 3)(4, 3, 2)
    grid = lambda lo=lo, hi=hi, reso=reso, first=0, n=24, xyz=64: lib.pnr_gen_grid_points(lo, hi, reso, first, n, xyz, None, None)  # noqa: E731
    assert grid(lo=None) == -1 and grid(hi=None) == -1 and grid(reso=None) == -1
    assert grid(xyz=None) == -1 and b"xyz" in lib.pnr_last_error()
    assert grid(first=20, n=5) == -1 and b"leaves the grid" in lib.pnr_last_error()
    assert grid(first=-1) == -1 and grid(n=-1) == -1
    assert grid(reso=(ctypes.c_int * 3)(4, 0, 2)) == -1 and b"reso" in lib.pnr_last_error()
    assert grid(hi=(ctypes.c_double * 3)(1, float("nan"), 1)) == -1
    assert grid(first=24, n=0, xyz=None) == 0  # no rows: a no-op


def test_header_declares_the_entries_and_the_abi_revision_stays_12(repo_root):
    import re
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    for name in ("pnr_gen_grid_points", "pnr_marching_cubes_workspace_bytes", "pnr_marching_cubes_count",
                 "pnr_marching_cubes_emit", "pnr_marching_cubes_tables"):
        assert name in _lib.PROTOTYPES and re.search(name + r"\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)), name
    assert "pnr_mesh.hip" in _lib.SOURCES


def test_operators_refuse_cpu_tensors():
    from pixelnerf_amd.util import recon
    with pytest.raises(_lib.PixelNerfHipError):
        ops.marching_cubes(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.gen_grid_points([-1, -1, -1], [1, 1, 1], [4, 4, 4], device="cpu")

    class Host(torch.nn.Module):
        use_viewdirs = False

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, xyz, coarse=True, viewdirs=None):
            return xyz.new_zeros(*xyz.shape[:2], 4)

    with pytest.raises(_lib.PixelNerfHipError):
        recon.marching_cubes(Host(), reso=[4, 4, 4])  # its parameters live on the host
    two = Host()
    two.num_objs = 2
    with pytest.raises(ValueError, match="2 objects"):
        recon.marching_cubes(two, reso=[4, 4, 4])
