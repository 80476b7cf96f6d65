"""GPU tests (-m gpu) of the mesh finishing: pnr_grid_components / pnr_grid_normals through ops.grid_components /
ops.grid_normals, and util.recon.remove_floaters / vertex_normals / vertex_colors / extract_mesh and
OccupancyGrid.from_density(keep_largest=) on top of them, against the CPU restatements of tests/meshfinish_ref.py (their own
checks: tests/test_meshfinish_host.py).

Labels, sizes and counts are integers: exact equality with scipy.ndimage.label relabelled to the smallest linear index.
Normals: against the fp64 restatement of the formula, within 10 x the largest component error the fp32 restatement of the same
formula shows against the fp64 one on the same inputs (floor 1e-6) -- the yardstick is the reference arithmetic, never the kernel."""
import warnings

import numpy as np
import pytest
import torch

import mc_ref as M
import meshfinish_ref as R
import occ_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from pixelnerf_amd.util import recon as _recon
    return _recon


def _to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _components(ops, dev, field, thr, what):
    """labels, sizes, counts against the reference, exactly; a second call and a call without sizes give the same label bytes"""
    f = _to(dev, field)
    labels, sizes, counts = ops.grid_components(f, thr)
    assert labels.dtype == sizes.dtype == counts.dtype == torch.int32 and labels.is_cuda
    assert tuple(labels.shape) == tuple(field.shape) and tuple(sizes.shape) == (field.size,) and tuple(counts.shape) == (2,)
    rl, rs, rc = R.components_ref(field, thr)
    got_l, got_s, got_c = labels.cpu().numpy(), sizes.cpu().numpy(), tuple(counts.tolist())
    assert got_c == rc, (what, got_c, rc)
    assert np.array_equal(got_l, rl), what
    assert np.array_equal(got_s, rs), what
    again, none, again_c = ops.grid_components(f, thr, want_sizes=False)
    assert none is None and torch.equal(again, labels) and torch.equal(again_c, counts), what
    return got_l, got_s, got_c


def test_all_256_patterns_of_a_2x2x2_grid(ops, dev):
    for case in range(256):
        field = R.pattern_2x2x2(case)
        _, _, counts = _components(ops, dev, field, 0.5, f"pattern {case}")
        assert counts[0] == bin(case).count("1")                     # == threshold, NaN and +inf are outside
    assert not R.inside_mask(R.pattern_2x2x2(0b11111000), 0.5)[[0, 1, 0], [0, 0, 1], [0, 0, 0]].any()


@pytest.mark.parametrize("shape,p,seed", R.RANDOM_CASES, ids=["5x6x7", "17x9x33", "64x64x64"])
def test_random_fields(ops, dev, shape, p, seed):
    field = R.random_field(shape, p, seed)
    _, sizes, (n_in, n_comp) = _components(ops, dev, field, 0.5, f"random {shape}")
    print(f"random {shape} p = {p}: {n_in} inside, {n_comp} components, the largest {sizes.max()}")
    if shape == (64, 64, 64):                                        # not vacuous: a giant component among thousands of small ones
        assert n_comp >= 1000 and sizes.max() >= 0.1 * n_in


@pytest.mark.parametrize("variant", ["as it is", "flipped y z", "transposed, flipped y"])
def test_long_chains(ops, dev, variant):
    field = R.serpentine_variants()[variant]
    labels, sizes, counts = _components(ops, dev, field, 0.5, f"serpentine {variant}")
    assert counts == (577, 1) and sizes[0] == 577 and (labels[labels >= 0] == 0).all()


def test_extremes(ops, dev):
    labels, sizes, counts = _components(ops, dev, np.ones((32, 32, 32), np.float32), 0.5, "all inside")
    assert (labels == 0).all() and sizes[0] == 32768 and counts == (32768, 1)
    labels, sizes, counts = _components(ops, dev, np.zeros((32, 32, 32), np.float32), 0.5, "all outside")
    assert (labels == -1).all() and counts == (0, 0) and not sizes.any()
    labels, _, counts = _components(ops, dev, np.array([1, 1, 0, 1, 0], np.float32).reshape(1, 1, 5), 0.5, "1x1x5")
    assert labels.ravel().tolist() == [0, 0, -1, 3, -1] and counts == (3, 2)
    _components(ops, dev, np.ones((1, 7, 1), np.float32), float("-inf"), "threshold -inf")
    _components(ops, dev, np.ones((3, 1, 2), np.float32), float("inf"), "threshold +inf")
    with pytest.raises(ValueError):
        ops.grid_components(torch.zeros((0, 4, 4), device=dev), 0.5)
    with pytest.raises(ops._lib.PixelNerfHipError, match="NaN"):
        ops.grid_components(torch.zeros((2, 2, 2), device=dev), float("nan"))


# ---------------------------------------------------------------- normals

def test_normals_against_the_fp64_restatement(ops, dev):
    shape, iso = (11, 13, 17), 0.02
    field = R.smooth_field(shape, 4321)
    c1, scale = (-1.0, 0.5, 2.0), (0.25, 0.1, 3.0)
    f = _to(dev, field)
    v, _ = ops.marching_cubes(f, iso, c1=c1, scale=scale)
    n = ops.grid_normals(f, v, c1, scale)
    assert n.dtype == torch.float32 and tuple(n.shape) == tuple(v.shape) and n.is_cuda
    assert torch.equal(n, ops.grid_normals(f, v, c1, scale))                           # the same bytes from call to call
    vh = v.cpu().numpy()
    ref, g, cell = R.normals_ref(field, vh, c1, scale)
    ref32, _, _ = R.normals_ref(field, vh, c1, scale, dtype=np.float32)
    sel = g >= 1e-3 * g.max()
    border = ((cell == 0) | (cell == np.array(shape) - 2)).any(axis=1)
    bar = max(10.0 * np.abs(ref32.astype(np.float64) - ref)[sel].max(), 1e-6)
    err = np.abs(n.cpu().numpy().astype(np.float64) - ref)[sel].max()
    print(f"normals {shape}: {len(vh)} vertices, {sel.sum()} compared, {(border & sel).sum()} of them in a border cell, "
          f"max component error {err:.3e}, bar {bar:.3e}")
    assert len(vh) > 300 and sel.sum() > 0.9 * len(vh) and (border & sel).sum() >= 10
    assert np.isfinite(n.cpu().numpy()).all() and err <= bar
    assert np.abs(np.linalg.norm(n.cpu().numpy().astype(np.float64), axis=1)[sel] - 1.0).max() <= 1e-6
    # a locally flat field: no gradient, no normal
    flat = field.copy()
    flat[2:7, 3:8, 4:9] = 0.75
    at = (np.array([[4.3, 5.5, 6.2], [3.5, 4.5, 5.5]]) * np.array(scale) + np.array(c1)).astype(np.float32)
    out = ops.grid_normals(_to(dev, flat), torch.from_numpy(at).to(dev), c1, scale).cpu().numpy()
    assert (out == 0).all()
    # points off the grid are clamped to it, a NaN point lands on the grid too: every row is a unit vector or zero
    wild = torch.tensor([[1e30, -1e30, 0.0], [float("nan"), 1.0, 5.0], [float("inf"), float("-inf"), 2.5]], device=dev)
    lens = ops.grid_normals(f, wild, c1, scale).norm(dim=1).cpu().numpy()
    assert ((np.abs(lens - 1.0) < 1e-6) | (lens == 0)).all()
    assert tuple(ops.grid_normals(f, v[:0], c1, scale).shape) == (0, 3)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_on_analytic_solids(ops, dev, name):
    field, analytic = R.solid(name)
    h = 2.0 / 32
    c1, scale = (-1.0, -1.0, -1.0), (h, h, h)
    f = _to(dev, field)
    v, t = ops.marching_cubes(f, 0.0, c1=c1, scale=scale)
    n = ops.grid_normals(f, v, c1, scale).cpu().numpy().astype(np.float64)
    vh, th = v.cpu().numpy().astype(np.float64), t.cpu().numpy()
    dots = (n * analytic(vh)).sum(axis=1)
    tri = vh[th]
    face = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    agree = (n[th] * face[:, None, :]).sum(axis=2)
    print(f"{name} 33^3: {len(vh)} vertices, min n . analytic = {dots.min():.6f}, min n . face normal (unnormalised) = {agree.min():.3e}")
    assert len(vh) > 1000 and dots.min() >= 0.999
    assert (agree > 0).all()


# ---------------------------------------------------------------- floaters

@pytest.fixture(scope="module")
def floaters(ops, dev):
    """the scene, its unfiltered device mesh and the CPU labels, computed once"""
    field, c1, scale = R.floater_scene()
    f = _to(dev, field)
    v, t = ops.marching_cubes(f, 0.0, c1=c1, scale=scale)
    inside = R.inside_mask(field, 0.0)
    cross = R.crossed_edges(inside)
    ii, jj, kk, aa = np.nonzero(cross)                                 # row-major: the mesher's vertex order
    e = np.eye(3, dtype=np.int64)[aa]
    lower_inside = inside[ii, jj, kk]
    end = np.where(lower_inside[:, None], np.stack((ii, jj, kk), 1), np.stack((ii, jj, kk), 1) + e)   # the edge's inside end
    assert len(ii) == len(v)
    return {"field": field, "dev_field": f, "c1": c1, "scale": scale, "v": v.cpu().numpy(), "t": t.cpu().numpy(), "inside_end": end}


@pytest.mark.parametrize("kw,n_mesh", [({"keep_largest": 1}, 1), ({"min_voxels": 2}, 2)], ids=["keep_largest_1", "min_voxels_2"])
def test_floaters_through_the_mesher(ops, recon, dev, floaters, kw, n_mesh):
    fs = floaters
    assert R.mesh_components(fs["t"], len(fs["v"])) == 5                # the object, the small sphere, three single voxels
    filtered, info = recon.remove_floaters(fs["dev_field"], 0.0, **kw)
    ref_f, kept, labels = R.remove_floaters_ref(fs["field"], 0.0, **kw)
    assert filtered.cpu().numpy().tobytes() == ref_f.tobytes()
    _, _, (n_in, n_comp) = R.components_ref(fs["field"], 0.0)
    assert info == {"n_components": n_comp, "n_kept": n_mesh, "voxels_inside": n_in, "voxels_dropped": int(((labels >= 0) & ~kept).sum())}
    assert all(type(x) is int for x in info.values()) and info["voxels_dropped"] > 0
    v, t = ops.marching_cubes(filtered, 0.0, c1=fs["c1"], scale=fs["scale"])
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert R.mesh_components(t, len(v)) == n_mesh
    if n_mesh == 1:
        closed, chi = M.mesh_topology(t)
        assert closed and chi == 2
    # the kept part of the unfiltered mesh, bit for bit: vertices on the crossed edges whose inside end is kept, in order ...
    end = fs["inside_end"]
    v_kept = kept[end[:, 0], end[:, 1], end[:, 2]]
    assert len(v) == v_kept.sum() and v.tobytes() == fs["v"][v_kept].tobytes()
    rows = {r.tobytes() for r in fs["v"]}
    assert all(r.tobytes() in rows for r in v)
    # ... and the triangles all of whose vertices are kept, renumbered
    t_kept = v_kept[fs["t"]].all(axis=1)
    assert len(t) == t_kept.sum() and 0 < len(t) < len(fs["t"])
    renumber = np.cumsum(v_kept) - 1
    assert np.array_equal(t, renumber[fs["t"][t_kept]].astype(np.int32))
    # both filters at once, and nothing to drop
    both, info2 = recon.remove_floaters(fs["dev_field"], 0.0, keep_largest=4, min_voxels=2)
    assert both.cpu().numpy().tobytes() == R.remove_floaters_ref(fs["field"], 0.0, keep_largest=4, min_voxels=2)[0].tobytes()
    assert info2["n_kept"] == 2
    same, info3 = recon.remove_floaters(fs["dev_field"], 0.0, keep_largest=9)
    assert torch.equal(same, fs["dev_field"]) and info3["n_kept"] == 5 and info3["voxels_dropped"] == 0


def test_ties_in_size_go_to_the_smaller_root(recon, dev):
    field = np.zeros((4, 4, 9), np.float32)
    field[3, 3, 0:2] = 1.0
    field[0, 1, 4:6] = 1.0
    field[2, 0, 7:9] = 1.0
    out, info = recon.remove_floaters(_to(dev, field), 0.5, keep_largest=2)
    expect = field.copy()
    expect[3, 3, 0:2] = 0.5                                             # the largest root index of the three loses
    assert np.array_equal(out.cpu().numpy(), expect) and info["n_kept"] == 2 and info["voxels_dropped"] == 2
    assert out.cpu().numpy().tobytes() == R.remove_floaters_ref(field, 0.5, keep_largest=2)[0].tobytes()


# ---------------------------------------------------------------- through the model

RESO, C1, C2 = [12, 10, 9], [-1, -1, -1], [1, 1, 1]


@pytest.fixture(scope="module")
def model_case(dev, recon):
    """the sn64 fixture scene in a fused network at the default precision (tests/test_hip_mesh.py's), its density grid and the
    median sigma as the level"""
    from helpers import scene_for
    from test_api_gpu import build_net
    scene, _ = scene_for("sn64")
    net = build_net(dev, scene)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sigmas, reso = recon.density_grid(net, C1, C2, RESO)
    return net, sigmas.view(*reso), float(sigmas.median())


def test_extract_mesh_through_the_model(ops, recon, dev, model_case):
    net, grid, iso = model_case
    assert net.precision == "f16x3" and net.use_viewdirs
    net.train()
    with pytest.warns(UserWarning, match="fake view dirs"):
        mesh = recon.extract_mesh(net, C1, C2, RESO, isosurface=iso, keep_largest=1)
    assert net.training                                                  # the flag is restored
    net.eval()
    v, t, n, c = mesh.vertices, mesh.triangles, mesh.normals, mesh.colors
    V = v.shape[0]
    assert V > 50 and t.shape[0] > 50 and all(x.is_cuda for x in (v, t, n, c))
    assert (v.dtype, t.dtype, n.dtype, c.dtype) == (torch.float32, torch.int32, torch.float32, torch.float32)
    assert tuple(v.shape) == tuple(n.shape) == tuple(c.shape) == (V, 3) and t.shape[1] == 3
    # info against the labelling of the same grid
    _, sizes, counts = ops.grid_components(grid, iso)
    n_in, n_comp = counts.tolist()
    assert mesh.info["voxels_inside"] == n_in and mesh.info["n_components"] == n_comp and mesh.info["n_kept"] == 1
    assert mesh.info["voxels_dropped"] == n_in - int(sizes.max())
    # the pieces: the filtered grid's mesh, its normals, the network's rgb in ONE direct call
    filtered, _ = recon.remove_floaters(grid, iso, keep_largest=1)
    scale = (np.array(C2, np.float64) - np.array(C1)) / np.array(RESO)
    rv, rt = ops.marching_cubes(filtered, iso, c1=np.array(C1, np.float64), scale=scale)
    assert torch.equal(rv, v) and torch.equal(rt, t)
    assert torch.equal(n, ops.grid_normals(filtered, v, C1, scale)) and torch.equal(n, recon.vertex_normals(filtered, v, C1, scale))
    with torch.no_grad():
        direct = net(v[None], coarse=True, viewdirs=recon.origin_viewdirs(v)[None])[0, :, :3]
        direct_n = net(v[None], coarse=True, viewdirs=(-n)[None])[0, :, :3]
        direct_fine = net(v[None], coarse=False, viewdirs=(-n)[None])[0, :, :3]
    assert torch.equal(c, direct)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ebs in (1000, 1001, 100000):                                 # 1080 grid points: two chunks, the second one odd-placed at 1001
            m = recon.extract_mesh(net, C1, C2, RESO, isosurface=iso, keep_largest=1, eval_batch_size=ebs)
            assert torch.equal(m.vertices, v) and torch.equal(m.triangles, t) and torch.equal(m.normals, n) and torch.equal(m.colors, c), ebs
        for ebs in (50, 51, 2, 1):                                       # many chunks of the vertices themselves
            assert torch.equal(recon.vertex_colors(net, v, eval_batch_size=ebs), c), ebs
        by_normal = recon.extract_mesh(net, C1, C2, RESO, isosurface=iso, keep_largest=1, viewdirs="normal", normals=False)
        assert by_normal.normals is None and torch.equal(by_normal.colors, direct_n) and not torch.equal(direct_n, direct)
        assert torch.equal(recon.vertex_colors(net, v, viewdirs="normal", normals=n, eval_batch_size=64), direct_n)
        assert torch.equal(recon.vertex_colors(net, v, viewdirs=-n, coarse=False, eval_batch_size=64), direct_fine)
        bare = recon.extract_mesh(net, C1, C2, RESO, isosurface=iso, normals=False, colors=False)
        mv, mt = recon.marching_cubes(net, C1, C2, RESO, isosurface=iso, as_tensors=True)
    assert bare.normals is None and bare.colors is None and bare.info is None
    assert torch.equal(bare.vertices, mv) and torch.equal(bare.triangles, mt)   # without a filter: marching_cubes' own mesh


# ---------------------------------------------------------------- occupancy

def test_occupancy_grid_of_the_object_only(ops, dev, floaters):
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    field = floaters["field"].copy()
    field[30, 30, 2] = np.nan                                            # far from everything: outside for the labelling, occupied for culling
    c1, c2 = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    f = _to(dev, field)
    plain = OccupancyGrid.from_density(f, c1, c2, 0.0, dilate=1)
    only = OccupancyGrid.from_density(f, c1, c2, 0.0, dilate=1, keep_largest=1)
    ref_f, kept, labels = R.remove_floaters_ref(field, 0.0, keep_largest=1)
    assert np.isnan(ref_f[30, 30, 2])
    ref = OccupancyGrid.from_density(_to(dev, ref_f), c1, c2, 0.0, dilate=1)
    assert torch.equal(only.bits, ref.bits) and int(only.n_occupied) == int(ref.n_occupied)
    assert int(only.n_occupied) < int(plain.n_occupied)
    assert plain.info is None and only.info["n_kept"] == 1 and only.info["n_components"] == 5
    assert only.info["voxels_dropped"] == int(((labels >= 0) & ~kept).sum()) > 0
    cells, _ = occ_ref.unpack_bits(only.bits.cpu().numpy().view(np.uint32), (32, 32, 32))
    assert cells[29:31, 29:31, 1:3].all()                                # the NaN point's cells stay occupied
    assert np.array_equal(cells, occ_ref.build_ref(ref_f, 0.0, dilate=1))
    assert not cells[1:3, 2:4, 3:5].any()                                # where a single-voxel floater was
    both = OccupancyGrid.from_density(f, c1, c2, 0.0, dilate=0, min_voxels=2)
    assert np.array_equal(occ_ref.unpack_bits(both.bits.cpu().numpy().view(np.uint32), (32, 32, 32))[0],
                          occ_ref.build_ref(R.remove_floaters_ref(field, 0.0, min_voxels=2)[0], 0.0, dilate=0))
