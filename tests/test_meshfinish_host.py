"""Host tests (no GPU) of the mesh finishing: the two C entries are declared, exported, bound (within ABI revision 12: no struct or
argument list changed) and refuse bad arguments before any HIP call; the relabelled scipy reference of tests/meshfinish_ref.py
agrees with a plain flood fill and its shared cases are not vacuous; the fp64 restatement of the normal formula reaches the
analytic normals the GPU test asks the device for; save_obj / save_ply write what they say; util.recon and
util.occupancy.OccupancyGrid validate their new arguments before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mc_ref as M
import meshfinish_ref as R
from pixelnerf_amd import _lib

ENTRIES = ("pnr_grid_components", "pnr_grid_normals")


def test_header_declares_the_entries_within_abi_revision_12(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    _lib.build_library()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and re.search(name + r"\s*\(", code), name
        assert hasattr(lib, name), name
    assert lib.pnr_abi_version() == _lib.ABI_VERSION
    assert "pnr_meshfinish.hip" in _lib.SOURCES
    from pixelnerf_amd import ops
    from pixelnerf_amd.util import recon
    for name in ("grid_components", "grid_normals"):
        assert callable(getattr(ops, name))
    for name in ("remove_floaters", "vertex_normals", "vertex_colors", "extract_mesh", "save_ply"):
        assert callable(getattr(recon, name))


def test_a_library_without_the_entries_is_reported_as_stale(monkeypatch):
    _lib.build_library()
    real = ctypes.CDLL(_lib.LIB_PATH)

    class Old:
        def __getattr__(self, name):
            if name in ENTRIES:
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_lib.PixelNerfHipError, match=r"pnr_grid_components.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_entries_refuse_bad_arguments_on_the_host():
    """PNR_E_INVALID (-1) before any HIP call; the addresses are dummies, never dereferenced"""
    _lib.build_library()
    lib = _lib.load()
    comp = lambda field=64, n=(4, 4, 4), thr=0.5, labels=64: lib.pnr_grid_components(  # noqa: E731
        field, n[0], n[1], n[2], thr, labels, None, None, None)
    for n in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (4, -1, 4)):
        assert comp(n=n) == -1 and b"at least 1" in lib.pnr_last_error(), n
    assert comp(n=(1291, 1291, 1291)) == -1 and b"2^31" in lib.pnr_last_error() and 1291 ** 3 >= 2 ** 31
    assert comp(n=(65536, 65536, 1)) == -1 and b"2^31" in lib.pnr_last_error()
    assert comp(thr=float("nan")) == -1 and b"NaN" in lib.pnr_last_error()
    assert comp(field=None) == -1 and b"null" in lib.pnr_last_error()
    assert comp(labels=None) == -1 and b"null" in lib.pnr_last_error()
    lo, sc = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(0.1, 0.2, 0.3)
    nrm = lambda field=64, n=(4, 4, 4), c1=lo, scale=sc, v=64, V=8, out=64: lib.pnr_grid_normals(  # noqa: E731
        field, n[0], n[1], n[2], c1, scale, v, V, out, None)
    for n in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        assert nrm(n=n) == -1 and b"at least 2" in lib.pnr_last_error(), n
    assert nrm(n=(1291, 1291, 1291)) == -1 and b"2^31" in lib.pnr_last_error()
    assert nrm(c1=None) == -1 and nrm(scale=None) == -1 and b"c1 / scale" in lib.pnr_last_error()
    for bad in (0.0, float("inf"), float("nan")):
        assert nrm(scale=(ctypes.c_float * 3)(0.1, bad, 0.3)) == -1 and b"scale" in lib.pnr_last_error(), bad
    assert nrm(scale=(ctypes.c_float * 3)(0.1, -0.2, 0.3), V=0) == 0                                # a negative scale is ordinary
    assert nrm(V=-1) == -1
    for name in ("field", "v", "out"):
        assert nrm(**{name: None}) == -1 and b"null" in lib.pnr_last_error(), name
    assert nrm(field=None, v=None, out=None, V=0) == 0                                              # V = 0: a no-op


def test_ops_refuse_cpu_tensors():
    from pixelnerf_amd import ops
    with pytest.raises(_lib.PixelNerfHipError):
        ops.grid_components(torch.zeros(3, 3, 3), 0.5)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.grid_normals(torch.zeros(3, 3, 3), torch.zeros(4, 3), (0, 0, 0), (1, 1, 1))


# ---------------------------------------------------------------- the reference

def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_relabelled_reference_agrees_with_a_flood_fill():
    shape, p, seed = R.RANDOM_CASES[0]
    field = R.random_field(shape, p, seed)
    ref, bfs = R.components_ref(field, 0.5), R.components_bfs(field, 0.5)
    assert _same(ref, bfs) and ref[2] == (104, 8)
    assert ref[0].dtype == np.int32 and ref[0].shape == shape and ref[1].shape == (5 * 6 * 7,)
    lab, sizes, (n_in, n_comp) = ref
    roots = np.flatnonzero(sizes)
    assert len(roots) == n_comp and sizes.sum() == n_in == (lab >= 0).sum()
    assert (lab.ravel()[roots] == roots).all() and (lab.ravel()[lab.ravel() >= 0] <= np.flatnonzero(lab.ravel() >= 0)).all()
    for case in (0, 1, 0b10010110, 0b01101001, 255, 0b11101000):
        assert _same(R.components_ref(R.pattern_2x2x2(case), 0.5), R.components_bfs(R.pattern_2x2x2(case), 0.5)), case
    s = R.serpentine()
    for f in (s, np.ascontiguousarray(s[:, ::-1, ::-1])):
        assert _same(R.components_ref(f, 0.5), R.components_bfs(f, 0.5))


def test_shared_cases_are_what_they_claim():
    # the three special values of the 2x2x2 patterns are outside
    f = R.pattern_2x2x2(0b00001000)
    assert f[0, 0, 0] == np.float32(0.5) and np.isnan(f[1, 0, 0]) and np.isposinf(f[0, 1, 0])
    assert R.inside_mask(f, 0.5).sum() == 1 and R.inside_mask(R.pattern_2x2x2(0), 0.5).sum() == 0
    # the diagonal pattern: four corners, no two joined by an edge
    assert R.components_ref(R.pattern_2x2x2(0b10010110), 0.5)[2] == (4, 4)
    # the random fields: 346 and 13 546 components; the 64^3 one has a giant component next to thousands of small ones
    assert R.components_ref(R.random_field(*R.RANDOM_CASES[1]), 0.5)[2][1] == 346
    lab, sizes, (n_in, n_comp) = R.components_ref(R.random_field(*R.RANDOM_CASES[2]), 0.5)
    assert (n_in, n_comp, int(sizes.max())) == (84176, 13546, 31418)
    assert n_comp >= 1000 and sizes.max() >= 0.1 * n_in
    # the serpentine: one chain of 577 voxels with label 0; flipped along y and z the chain is walked from its other end
    lab, sizes, counts = R.components_ref(R.serpentine(), 0.5)
    assert counts == (577, 1) and sizes[0] == 577 and (lab[lab >= 0] == 0).all()
    fl = np.ascontiguousarray(R.serpentine()[:, ::-1, ::-1])
    lab, sizes, counts = R.components_ref(fl, 0.5)
    root = int(lab.max())
    assert counts == (577, 1) and sizes[root] == 577 and root == np.flatnonzero(fl.ravel() > 0.5)[0]
    mid = R.serpentine_variants()["transposed, flipped y"]
    lab, sizes, counts = R.components_ref(mid, 0.5)
    assert counts == (577, 1) and sizes[0] == 577 and mid[0, 0, 0] == 1 and mid[0, 0, 1] == 1 and mid[0, 1, 0] == 1  # two neighbours
    assert _same(R.components_ref(mid, 0.5), R.components_bfs(mid, 0.5))
    # the floater scene: the sphere, the small sphere, three single voxels
    f, _, _ = R.floater_scene()
    lab, sizes, counts = R.components_ref(f, 0.0)
    assert counts[1] == 5 and sorted(sizes[sizes > 0])[:3] == [1, 1, 1] and sorted(sizes[sizes > 0])[3] >= 2
    assert len(R.select_components(sizes, keep_largest=1)) == 1 and len(R.select_components(sizes, min_voxels=2)) == 2
    assert len(R.select_components(sizes, keep_largest=4, min_voxels=2)) == 2


def test_selection_breaks_ties_towards_the_smaller_root():
    sizes = np.zeros(40, dtype=np.int32)
    sizes[[3, 9, 20, 31]] = [5, 7, 5, 7]
    assert R.select_components(sizes, keep_largest=1).tolist() == [9]
    assert R.select_components(sizes, keep_largest=3).tolist() == [3, 9, 31]
    assert R.select_components(sizes, keep_largest=3, min_voxels=6).tolist() == [9, 31]
    assert R.select_components(sizes, min_voxels=8).tolist() == []


@pytest.fixture(scope="module")
def tables():
    from pixelnerf_amd import ops
    return ops.marching_cubes_tables()  # (a host entry)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_fp64_normals_reach_the_analytic_ones(tables, name):
    """what the GPU test holds the device to (dot >= 0.999, i.e. 1 - dot <= 1e-3) is reachable with room: the formula itself, in
    fp64, must use at most half of that budget.  Measured: min dot 0.999998 on the sphere, 0.999904 on the torus."""
    field, analytic = R.solid(name)
    h = 2.0 / 32
    v, t, _ = M.marching_cubes_ref(field, 0.0, *tables, c1=(-1.0, -1.0, -1.0), scale=(h, h, h))
    n, g, _ = R.normals_ref(field, v, (-1.0, -1.0, -1.0), (h, h, h))
    dots = (n * analytic(v)).sum(axis=1)
    print(f"{name}: {len(v)} vertices, min n . analytic = {dots.min():.6f}")
    assert len(v) > 1000 and dots.min() >= 0.9995
    tri = v[t]
    face = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((n[t] * face[:, None, :]).sum(axis=2) > 0).all()
    n32, _, _ = R.normals_ref(field, v, (-1.0, -1.0, -1.0), (h, h, h), dtype=np.float32)
    assert n32.dtype == np.float32 and np.abs(n32 - n).max() < 1e-4


def test_normals_ref_on_a_linear_field_and_a_flat_one():
    i, j, k = np.meshgrid(np.arange(4.0), np.arange(5.0), np.arange(6.0), indexing="ij")
    field = 2.0 * i - 3.0 * j + 0.5 * k
    pts = np.array([[0.1, 0.2, 0.3], [2.9, 3.9, 4.9], [1.5, 2.0, 2.5], [-4.0, 9.0, 2.0]])
    c1, scale = np.array([1.0, -2.0, 0.5]), np.array([0.5, 2.0, 0.25])
    n, g, cell = R.normals_ref(field, pts * scale + c1, c1, scale)
    grad = np.array([2.0, -3.0, 0.5]) / scale
    assert np.allclose(n, -grad / np.linalg.norm(grad), atol=1e-6) and np.allclose(g, np.linalg.norm(grad), rtol=1e-6)
    assert cell.tolist() == [[0, 0, 0], [2, 3, 4], [1, 2, 2], [0, 3, 2]]
    n, g, _ = R.normals_ref(np.full((4, 5, 6), 7.0), pts, (0, 0, 0), (1, 1, 1))
    assert (n == 0).all() and (g == 0).all()


# ---------------------------------------------------------------- files

def _mesh():
    rs = np.random.RandomState(5)
    v = rs.uniform(-2, 2, (7, 3))
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], dtype=np.int32)
    rgb = rs.uniform(0, 1, (7, 3))
    n = rs.standard_normal((7, 3))
    return v, t, rgb, n / np.linalg.norm(n, axis=1, keepdims=True)


def _reference_obj(v, t, rgb=None):
    """src/util/recon.py:81-106 restated: a line per vertex, a line per face"""
    out = []
    for i in range(len(v)):
        line = "v %.4f %.4f %.4f" % tuple(v[i])
        if rgb is not None:
            line += " %.4f %.4f %.4f" % tuple(rgb[i])
        out.append(line + "\n")
    for f in t:
        out.append("f %d %d %d\n" % tuple(int(a) + 1 for a in f))
    return "".join(out)


def test_save_obj_without_normals_writes_the_reference_bytes(tmp_path):
    from pixelnerf_amd.util import recon
    v, t, rgb, _ = _mesh()
    recon.save_obj(v, t, str(tmp_path / "a.obj"))
    recon.save_obj(torch.from_numpy(v), torch.from_numpy(t), str(tmp_path / "b.obj"), vert_rgb=torch.from_numpy(rgb))
    recon.save_obj(v, t, str(tmp_path / "c.obj"), vert_rgb=rgb, vert_normals=None)
    assert (tmp_path / "a.obj").read_text() == _reference_obj(v, t)
    assert (tmp_path / "b.obj").read_text() == _reference_obj(v, t, rgb) == (tmp_path / "c.obj").read_text()


def test_save_obj_with_normals(tmp_path):
    from pixelnerf_amd.util import recon
    v, t, rgb, n = _mesh()
    recon.save_obj(v, t, str(tmp_path / "n.obj"), vert_rgb=rgb, vert_normals=torch.from_numpy(n))
    lines = (tmp_path / "n.obj").read_text().splitlines()
    assert len(lines) == 7 + 7 + 4
    assert lines[:7] == _reference_obj(v, t, rgb).splitlines()[:7]
    assert lines[7:14] == ["vn %.4f %.4f %.4f" % tuple(r) for r in n]
    assert lines[14:] == ["f %d//%d %d//%d %d//%d" % tuple(int(a) + 1 for a in np.repeat(f, 2)) for f in t]
    assert lines[14] == "f 1//1 2//2 3//3"
    with pytest.raises(ValueError, match="normals"):
        recon.save_obj(v, t, str(tmp_path / "bad.obj"), vert_normals=n[:3])


def _parse_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    elements = []
    for line in header[2:-1]:
        w = line.split()
        if w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[1] == "list":
            elements[-1][2].append((w[4], types[w[2]], types[w[3]]))
        else:
            elements[-1][2].append((w[2], types[w[1]]))
    out, pos = {}, end
    for name, count, props in elements:
        if len(props) == 1 and len(props[0]) == 3:
            rows = []
            for _ in range(count):
                n = int(np.frombuffer(raw, props[0][1], 1, pos)[0])
                pos += np.dtype(props[0][1]).itemsize
                rows.append(np.frombuffer(raw, props[0][2], n, pos))
                pos += n * np.dtype(props[0][2]).itemsize
            out[name] = rows
        else:
            dt = np.dtype([(p[0], p[1]) for p in props])
            out[name] = np.frombuffer(raw, dt, count, pos)
            pos += count * dt.itemsize
    assert pos == len(raw)
    return out


def test_save_ply_round_trip(tmp_path):
    from pixelnerf_amd.util import recon
    v, t, rgb, n = _mesh()
    rgb[0] = (0.0, 1.0, 0.5)
    rgb[1] = (-0.2, 1.7, 0.999)
    path = str(tmp_path / "m.ply")
    recon.save_ply(path, torch.from_numpy(v), torch.from_numpy(t), vert_rgb=rgb, vert_normals=n)
    ply = _parse_ply(path)
    vert = ply["vertex"]
    assert vert.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(np.stack([vert[c] for c in "xyz"], axis=1), v.astype(np.float32))
    assert np.array_equal(np.stack([vert[c] for c in ("nx", "ny", "nz")], axis=1), n.astype(np.float32))
    u8 = np.stack([vert[c] for c in ("red", "green", "blue")], axis=1)
    assert u8.dtype == np.uint8 and u8[0].tolist() == [0, 255, 128] and u8[1].tolist() == [0, 255, 255]
    assert np.array_equal(u8[2:], np.rint(rgb[2:] * 255).astype(np.uint8))
    assert len(ply["face"]) == 4 and all(len(f) == 3 for f in ply["face"]) and np.array_equal(np.stack(ply["face"]), t)
    recon.save_ply(path, v, t)
    bare = _parse_ply(path)
    assert bare["vertex"].dtype.names == ("x", "y", "z") and len(bare["vertex"]) == 7 and np.array_equal(np.stack(bare["face"]), t)
    recon.save_ply(path, v[:0], t[:0], vert_rgb=rgb[:0])
    assert len(_parse_ply(path)["vertex"]) == 0
    with pytest.raises(ValueError, match="colours"):
        recon.save_ply(path, v, t, vert_rgb=rgb[:2])


# ---------------------------------------------------------------- argument validation (before any device work)

class _Net:
    use_viewdirs = True

    def __call__(self, *a, **k):
        raise AssertionError("the network must not be called")


@pytest.mark.parametrize("kw", [{"keep_largest": 0}, {"keep_largest": -3}, {"min_voxels": 0}, {"keep_largest": 1.5},
                                {"min_voxels": True}, {"keep_largest": 2, "min_voxels": -1}])
def test_floater_arguments_are_validated(kw):
    from pixelnerf_amd.util import recon
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    field = torch.zeros(3, 3, 3)
    with pytest.raises(ValueError, match="integer >= 1"):
        recon.remove_floaters(field, 0.5, **kw)
    with pytest.raises(ValueError, match="integer >= 1"):
        OccupancyGrid.from_density(field, (-1, -1, -1), (1, 1, 1), 0.5, **kw)
    with pytest.raises(ValueError, match="integer >= 1"):
        recon.extract_mesh(_Net(), reso=[3, 3, 3], **kw)


def test_remove_floaters_without_arguments_returns_the_field_itself():
    from pixelnerf_amd.util import recon
    field = torch.zeros(3, 3, 3)                         # a CPU tensor: any launch would be refused
    out, info = recon.remove_floaters(field, 0.5)
    assert out is field and info is None


def test_viewdirs_argument_is_validated():
    from pixelnerf_amd.util import recon
    v = torch.zeros(4, 3)
    for bad in ("camera", "", "Origin"):
        with pytest.raises(ValueError, match="'origin', 'normal'"):
            recon.vertex_colors(_Net(), v, viewdirs=bad)
        with pytest.raises(ValueError, match="'origin', 'normal'"):
            recon.extract_mesh(_Net(), reso=[3, 3, 3], viewdirs=bad)
    with pytest.raises(ValueError, match="needs the normals"):
        recon.vertex_colors(_Net(), v, viewdirs="normal")
    with pytest.raises(ValueError, match=r"\(4, 3\) tensor"):
        recon.vertex_colors(_Net(), v, viewdirs=torch.zeros(5, 3))
    with pytest.raises(ValueError, match=r"\(V,3\)"):
        recon.vertex_colors(_Net(), torch.zeros(4, 2))


def test_vertex_colors_chunks_are_even_and_the_flag_is_restored():
    """a recording stand-in for the network: chunk lengths, the directions handed over, eval mode during the calls"""
    from pixelnerf_amd.util import recon

    class Net(torch.nn.Module):
        use_viewdirs = True

        def __init__(self):
            super().__init__()
            self.calls = []

        def forward(self, xyz, coarse=True, viewdirs=None):
            assert not self.training and not torch.is_grad_enabled() and xyz.shape[0] == 1 and viewdirs.shape == xyz.shape
            self.calls.append((xyz.shape[1], coarse, viewdirs[0].clone()))
            return torch.cat((xyz * 2.0, xyz[..., :1]), dim=-1)

    pts = torch.arange(33.0).reshape(11, 3) - 15.0
    pts[5] = 0.0
    net = Net().train()
    with pytest.warns(UserWarning, match="fake view dirs"):
        c = recon.vertex_colors(net, pts, eval_batch_size=5, coarse=False)
    assert net.training and [n for n, _, _ in net.calls] == [4, 4, 3] and not any(co for _, co, _ in net.calls)
    assert torch.equal(c, pts * 2.0) and c.dtype == torch.float32
    vd = torch.cat([d for _, _, d in net.calls])
    assert torch.equal(vd, recon.origin_viewdirs(pts)) and (vd[5] == 0).all()
    assert torch.allclose(vd[0], -pts[0] / pts[0].norm())
    net.calls.clear()
    normals = torch.nn.functional.normalize(torch.ones(11, 3), dim=1)
    recon.vertex_colors(net, pts, viewdirs="normal", normals=normals, eval_batch_size=1)   # rounded down to even, at least 2
    assert [n for n, _, _ in net.calls] == [2, 2, 2, 2, 2, 1] and torch.equal(torch.cat([d for _, _, d in net.calls]), -normals)
    net.calls.clear()
    given = torch.randn(11, 3)
    recon.vertex_colors(net, pts, viewdirs=given)
    assert [n for n, _, _ in net.calls] == [11] and torch.equal(net.calls[0][2], given)
    assert recon.vertex_colors(net, pts[:0], viewdirs=given[:0]).shape == (0, 3)
