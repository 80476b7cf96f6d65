"""GPU tests (-m gpu) of the mesh extraction: pnr_gen_grid_points / pnr_marching_cubes_count / pnr_marching_cubes_emit through
ops.gen_grid_points / ops.marching_cubes, and util.recon.marching_cubes through the model, against the numpy restatement of
tests/mc_ref.py run with the library's own case tables (their contract: tests/test_mesh_host.py).

Exact: the three counts, the vertex order (which edge every vertex sits on) and the whole triangle array.
Positions: per coordinate |pos - ref| <= 8 * 2^-24 * max(1, |index|) in index space -- the field values are exact, t takes three
fp32 roundings (numerator, denominator, quotient; t <= 1), index + t one more, against the restatement's fp64.  In world space
(index * scale + c1 with fp32 scale and c1) the bound scales by `scale` and gains 4 * 2^-24 * max(1, |world|) for the rounding of
scale, of the product and of the sum."""
import numpy as np
import pytest
import torch

import mc_ref as M

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def tables(ops):
    return ops.marching_cubes_tables()


def _run(ops, dev, field, iso, check_finite=True, **kw):
    f = torch.from_numpy(np.ascontiguousarray(field, dtype=np.float32)).to(dev)
    v, t, counts = ops.marching_cubes(f, iso, check_finite=check_finite, return_counts=True, **kw)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda and t.is_cuda
    assert tuple(v.shape) == (counts[0], 3) and tuple(t.shape) == (counts[1], 3)
    return v.cpu().numpy(), t.cpu().numpy(), counts


def _check_against_ref(ops, dev, tables, field, iso, what, check_finite=True):
    """counts and triangles exact, positions row by row (that is the vertex order) within the index-space bound;
    -> (vertices, triangles, counts) of the device"""
    v, t, counts = _run(ops, dev, field, iso, check_finite=check_finite)
    rv, rt, rnf = M.marching_cubes_ref(field, iso, *tables)
    assert counts == (len(rv), len(rt), rnf), (what, counts, (len(rv), len(rt), rnf))
    assert np.array_equal(t, rt), what
    bound = 8 * EPS * np.maximum(1.0, np.abs(rv))
    err = np.abs(v.astype(np.float64) - rv)
    print(f"mesh {what}: {counts[0]} vertices, {counts[1]} triangles, max |pos - ref| / bound = "
          f"{(err / bound).max() if len(rv) else 0.0:.3f}")
    assert np.isfinite(v).all() and (err <= bound).all(), what
    return v, t, counts


def _cell(case, mag):
    f = np.empty((2, 2, 2), np.float32)
    for c in range(8):
        dx, dy, dz = M.corner_offset(c)
        f[dx, dy, dz] = mag[c] if (case >> c) & 1 else -mag[c]
    return f


def test_all_256_single_cells(ops, dev, tables):
    edge_mask, tri = tables
    rs = np.random.RandomState(256)
    for case in range(256):
        v, t, counts = _run(ops, dev, _cell(case, np.ones(8, np.float32)), 0.0)
        rv, rt, _ = M.marching_cubes_ref(_cell(case, np.ones(8, np.float32)), 0.0, *tables)
        assert counts == (bin(int(edge_mask[case])).count("1"), int((tri[case] >= 0).sum()) // 3, 0), case
        assert np.array_equal(t, rt) and np.array_equal(v.astype(np.float64), rv), case  # +-1: every t is exactly 1/2
        f = _cell(case, rs.uniform(0.05, 1.0, 8).astype(np.float32))
        v, t, counts = _run(ops, dev, f, 0.0)
        rv, rt, _ = M.marching_cubes_ref(f, 0.0, *tables)
        assert np.array_equal(t, rt) and (np.abs(v - rv) <= 8 * EPS * np.maximum(1.0, np.abs(rv))).all(), case


def _smooth_field(shape, seed):
    """seeded random values filtered once with a 3-tap box along every axis"""
    rs = np.random.RandomState(seed)
    f = rs.standard_normal([n + 2 for n in shape])
    f = (f[:-2] + f[1:-1] + f[2:]) / 3.0
    f = (f[:, :-2] + f[:, 1:-1] + f[:, 2:]) / 3.0
    f = (f[:, :, :-2] + f[:, :, 1:-1] + f[:, :, 2:]) / 3.0
    return f.astype(np.float32)


def test_random_smooth_field_and_repeatability(ops, dev, tables):
    field = _smooth_field((9, 8, 7), 987)
    v, t, counts = _check_against_ref(ops, dev, tables, field, 0.02, "smooth 9x8x7")
    assert counts[0] > 50 and counts[1] > 50
    f = torch.from_numpy(field).to(dev)
    a, b = ops.marching_cubes(f, 0.02), ops.marching_cubes(f, 0.02)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])          # identical bytes from call to call
    assert a[0].cpu().numpy().tobytes() == v.tobytes() and a[1].cpu().numpy().tobytes() == t.tobytes()
    # world space: index * scale + c1
    c1, scale = (-1.0, 0.5, 2.0), (0.25, 0.1, 3.0)
    w, tw, _ = _run(ops, dev, field, 0.02, c1=c1, scale=scale)
    rv, _, _ = M.marching_cubes_ref(field, 0.02, *tables)
    sc32, c32 = np.array(scale, np.float32).astype(np.float64), np.array(c1, np.float32).astype(np.float64)
    ref = rv * sc32 + c32
    bound = 8 * EPS * np.maximum(1.0, np.abs(rv)) * sc32 + 4 * EPS * np.maximum(1.0, np.abs(ref))
    assert np.array_equal(tw, t) and (np.abs(w - ref) <= bound).all()


def test_grid_with_nan_inf_and_values_on_the_level(ops, dev, tables):
    field = _smooth_field((6, 5, 4), 31)
    iso = np.float32(0.05)
    field[2, 2, 1] = np.nan
    field[4, 1, 2] = np.inf
    for idx in ((1, 1, 1), (3, 3, 2), (0, 0, 0), (5, 4, 3), (2, 3, 1)):
        field[idx] = iso
    with pytest.raises(ValueError, match="non-finite"):
        ops.marching_cubes(torch.from_numpy(field).to(dev), float(iso))
    v, t, counts = _check_against_ref(ops, dev, tables, field, float(iso), "specials 6x5x4", check_finite=False)
    assert counts[2] == 2 and counts[0] > 0 and np.isfinite(v).all()


def _solid(name, n=33):
    g = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    if name == "sphere":
        return (0.6 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)
    return (0.2 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).astype(np.float32)


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0)])
def test_analytic_solids_are_closed_and_wound_outwards(ops, dev, name, euler):
    n = 33
    h = 2.0 / (n - 1)
    v, t, counts = _run(ops, dev, _solid(name, n), 0.0, c1=(-1.0, -1.0, -1.0), scale=(h, h, h))
    closed, chi = M.mesh_topology(t)
    vol = M.signed_volume(v, t)
    print(f"{name} 33^3: {counts[0]} vertices, {counts[1]} triangles, V-E+F = {chi}, signed volume {vol:.4f} "
          f"(the solid's: {4.0 / 3.0 * np.pi * 0.6 ** 3 if name == 'sphere' else 2.0 * np.pi ** 2 * 0.55 * 0.2 ** 2:.4f})")
    assert closed and chi == euler
    assert vol > 0                                                           # the winding: normals point out of the solid
    if name == "sphere":
        # |x| is linear along no edge: the interpolated crossing misses the sphere by at most h^2/8 * max (|x|)'' = h^2 / (8 (0.6 - h));
        # fp32: the index-space term (index <= 32) times h, the world transform, and the field's own rounding (gradient 1), per
        # coordinate, times sqrt(3) for the norm
        fp32 = np.sqrt(3.0) * (8 * EPS * 32 * h + 4 * EPS * 1.0) + EPS
        r = np.linalg.norm(v.astype(np.float64), axis=1)
        print(f"sphere: max | |v| - 0.6 | = {np.abs(r - 0.6).max():.3e}, bound {h * h / (8 * (0.6 - h)) + fp32:.3e}")
        assert (np.abs(r - 0.6) <= h * h / (8 * (0.6 - h)) + fp32).all()


@pytest.mark.parametrize("shape", [(2, 2, 262400), (11, 13, 17)], ids=["2x2xN_two_scan_chunks", "11x13x17"])
def test_grids_that_do_not_fill_the_scan_blocks(ops, dev, tables, shape):
    """1 049 600 points = 1025 scan blocks of 1024 (the last one partial; the scan of the block sums takes a second chunk with a
    carry) and 2431 points = 3 blocks, the last one partial"""
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    field = np.sin(0.0113 * k + 0.9 * i + 1.7 * j + 0.4) if shape[2] > 1000 else np.sin(0.7 * i) + np.cos(0.9 * j) + np.sin(0.5 * k + 0.3 * i)
    _, _, counts = _check_against_ref(ops, dev, tables, field.astype(np.float32), 0.1, "x".join(map(str, shape)))
    assert counts[0] > 100


@pytest.mark.parametrize("reso", [(5, 7, 3), (4, 6, 8)], ids=["odd", "even"])
def test_gen_grid_points_equals_the_host_grid(ops, dev, reso):
    from pixelnerf_amd import util
    c1, c2 = [-1, -1.5, -0.25], [1, 1.5, 0.25]
    ref = util.gen_grid(*zip(c1, c2, reso), ij_indexing=True).numpy()
    xyz, vd = ops.gen_grid_points(c1, c2, reso, device=dev)
    assert xyz.shape == ref.shape and vd.shape == ref.shape
    assert xyz.cpu().numpy().tobytes() == ref.tobytes()                      # numpy's float32 linspace, bit for bit
    part, pvd = ops.gen_grid_points(c1, c2, reso, first=37, count=50, device=dev)
    assert torch.equal(part, xyz[37:87]) and torch.equal(pvd, vd[37:87])     # any sub-range of the rows: the chunks of recon
    assert ops.gen_grid_points(c1, c2, reso, device=dev, viewdirs=False)[1] is None
    d = vd.cpu().numpy()
    p = ref.astype(np.float64)
    nrm = np.linalg.norm(p, axis=1)
    origin = nrm == 0
    assert origin.sum() == (1 if all(n % 2 for n in reso) else 0)
    assert (d[origin] == 0).all()                                            # the reference has NaN here (0/0)
    exact = -p[~origin] / nrm[~origin, None]
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    assert np.isfinite(d).all() and (np.abs(d[~origin] - exact) <= 2 * ulp).all()
    with pytest.raises(ops._lib.PixelNerfHipError, match="leaves the grid"):
        ops.gen_grid_points(c1, c2, reso, first=len(ref) - 10, count=11, device=dev)


# ---------------------------------------------------------------- through the model

RESO, C1, C2 = [12, 10, 9], [-1, -1, -1], [1, 1, 1]


@pytest.fixture(scope="module")
def model_case(dev):
    """the sn64 fixture scene: the CPU oracle's sigma on the 1080 grid points and the network on the device"""
    from helpers import mlp_params, scene_for
    from oracle import pnr_oracle as O
    from pixelnerf_amd import util
    from test_api_gpu import build_net
    scene, _ = scene_for("sn64")
    xyz = util.gen_grid(*zip(C1, C2, RESO), ij_indexing=True)
    vd = -xyz / torch.norm(xyz, dim=-1, keepdim=True)
    with torch.no_grad():
        sigma = O.pixelnerf_forward(scene, mlp_params(11), xyz[None], vd[None])[0, :, 3].numpy()
    return build_net(dev, scene), scene, sigma


def test_recon_marching_cubes_through_the_model(ops, dev, tables, model_case):
    from pixelnerf_amd.util import recon
    net, scene, sigma_ref = model_case
    iso = float(np.median(sigma_ref))
    xyz, vd = ops.gen_grid_points(C1, C2, RESO, device=dev)
    with torch.no_grad():
        grid = net(xyz[None], coarse=True, viewdirs=vd[None])[0, :, 3].cpu().numpy()
    e_s = (np.abs(grid - sigma_ref) / np.maximum(1.0, sigma_ref)).max()
    print(f"recon sn64 {RESO}: isosurface {iso:.4f}, sigma rel err vs oracle {e_s:.3e}")
    assert e_s <= 1e-4
    net.train()
    with pytest.warns(UserWarning, match="fake view dirs"):
        v, t = recon.marching_cubes(net, C1, C2, RESO, isosurface=iso, as_tensors=True)
    assert net.training                                                      # the flag is restored
    net.eval()
    assert v.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32 and len(v) > 0 and len(t) > 0
    # the restatement on the device's own grid, in the reference's scaling (c2 - c1) / reso
    scale = (np.array(C2, np.float64) - np.array(C1)) / np.array(RESO)
    rv, rt, nonfinite = M.marching_cubes_ref(grid.reshape(RESO), iso, *tables)
    assert nonfinite == 0 and np.array_equal(t.cpu().numpy(), rt)
    sc32 = scale.astype(np.float32).astype(np.float64)
    ref = rv * sc32 + np.array(C1, np.float64)
    bound = 8 * EPS * np.maximum(1.0, np.abs(rv)) * sc32 + 4 * EPS * np.maximum(1.0, np.abs(ref))
    assert (np.abs(v.cpu().numpy() - ref) <= bound).all()
    with pytest.warns(UserWarning):
        nv, nt = recon.marching_cubes(net, C1, C2, RESO, isosurface=iso)
        cv, ct = recon.marching_cubes(net, C1, C2, RESO, isosurface=iso, eval_batch_size=250, as_tensors=True)
        av, at = recon.marching_cubes(net, C1, C2, RESO, isosurface=iso, align_to_grid=True, as_tensors=True)
    assert nv.dtype == np.float64 and nt.dtype == np.int32                   # numpy, like the reference
    assert np.array_equal(nv, v.cpu().numpy().astype(np.float64)) and np.array_equal(nt, t.cpu().numpy())
    assert torch.equal(cv, v) and torch.equal(ct, t)                         # chunks of 250 points: the same bytes
    # align_to_grid: the same mesh at the linspace's true spacing (c2 - c1) / (reso - 1)
    true32 = ((np.array(C2, np.float64) - np.array(C1)) / (np.array(RESO) - 1)).astype(np.float32).astype(np.float64)
    ref_a = rv * true32 + np.array(C1, np.float64)
    bound_a = 8 * EPS * np.maximum(1.0, np.abs(rv)) * true32 + 4 * EPS * np.maximum(1.0, np.abs(ref_a))
    assert torch.equal(at, t) and (np.abs(av.cpu().numpy() - ref_a) <= bound_a).all()
    assert not torch.equal(av, v)


def test_recon_refuses_a_net_that_encoded_two_objects(dev, model_case):
    from pixelnerf_amd.util import recon
    net = model_case[0]
    saved = net.num_objs
    try:
        net.num_objs = 2
        with pytest.raises(ValueError, match="2 objects"), pytest.warns(UserWarning):
            recon.marching_cubes(net, C1, C2, RESO)
    finally:
        net.num_objs = saved
