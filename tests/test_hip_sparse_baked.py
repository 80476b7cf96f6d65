"""GPU tests (-m gpu) of the sparse baked volumes: pnr_sparse_points_mark, pnr_gen_grid_points_at and pnr_baked_sparse_render_rays /
_views through ops.sparse_points, ops.gen_grid_points_at, ops.baked_sparse_render(_views) and util.bake.SparseBakedVolume.  Every
contract here is bit-exact (torch.equal): the kept set against the numpy restatement of tests/sparse_baked_ref.py (its own checks:
tests/test_sparse_baked_host.py), the march against the dense march with the same bits, the sparse bake against the dense bake."""
import warnings

import numpy as np
import pytest
import torch

import baked_ref as B
import baked_sh_ref as S
import sparse_baked_ref as SP

pytestmark = pytest.mark.gpu

P_TOTAL = B.RESO[0] * B.RESO[1] * B.RESO[2]
KINDS = ["rgba", 0, 1, 2]                                                  # the RGBA rows and the three degrees


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def bake():
    from pixelnerf_amd.util import bake as _bake
    return _bake


@pytest.fixture(scope="module")
def common(dev, bake):
    """the dense volumes of the baked tests (never modified), at skip_threshold 0 and 10, and the rays per setting"""
    coef2 = S.common_coef(2)
    case = {"np": {"rgba": B.common_volume()}, "dense": {}, "rays": {s: torch.from_numpy(B.common_rays(s)).to(dev) for s in B.SETTINGS}}
    for degree in (0, 1, 2):
        case["np"][degree] = np.ascontiguousarray(coef2[..., :(degree + 1) ** 2, :])
    for kind in KINDS:
        for thr in (0.0, 10.0):
            t = torch.from_numpy(case["np"][kind]).to(dev)
            case["dense"][kind, thr] = (bake.BakedVolume if kind == "rgba" else bake.BakedSHVolume).from_tensor(t, B.C1, B.C2, skip_threshold=thr)
    return case


def _equal(a, b):
    a, b = (tuple(x) if isinstance(x, tuple) else (x.rgb, x.depth, x.alpha) for x in (a, b))
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _dense_march(ops, dense, rays, step, bits, **kw):
    """ops.baked_render / ops.baked_sh_render on the dense tensor with the given bits"""
    if hasattr(dense, "vol"):
        return ops.baked_render(rays, dense.vol, dense.reso, dense.c1, dense.c2, step, bits=bits, **kw)
    return ops.baked_sh_render(rays, dense.coef, dense.degree, dense.reso, dense.c1, dense.c2, step, bits=bits, **kw)


# ---------------------------------------------------------------- 1. the kept set

def test_sparse_points_equal_the_restatement(dev, ops):
    one = np.zeros((3, 3, 3), np.float32)
    one[2, 2, 2] = 1.0                                                     # a corner of the last cell alone
    fields = {"empty": np.zeros((5, 4, 3), np.float32), "full": np.ones((5, 4, 3), np.float32), "2x2x2": np.ones((2, 2, 2), np.float32),
              "3x3x3 last": one}
    cases = [(name, fields[name], 0.0, cells) for name, cells in SP.grids().items()]
    sigma = B.common_volume()[..., 3]
    cases += [(f"shared thr {thr}", sigma, thr, SP.occupied_cells(sigma, thr)) for thr in (0.0, 10.0)]
    for name, field, thr, cells in cases:
        bits, count = ops.occupancy_build(torch.from_numpy(np.ascontiguousarray(field)).to(dev), thr, dilate=0)
        assert np.array_equal(SP.cells_from_bits(bits.cpu().numpy(), field.shape), cells) and int(count) == int(cells.sum()), name
        index, ids = ops.sparse_points(bits, field.shape)
        want_index, want_ids = SP.sparse_points(cells)
        assert index.dtype == ids.dtype == torch.int32 and tuple(index.shape) == field.shape and index.device == ids.device == bits.device
        assert np.array_equal(index.cpu().numpy(), want_index), name
        assert np.array_equal(ids.cpu().numpy(), want_ids), name
        again = ops.sparse_points(bits, field.shape)
        assert torch.equal(again[0], index) and torch.equal(again[1], ids)
    assert ops.sparse_points(bits, B.RESO)[1].numel() < 198               # (the last case: threshold 10)
    with pytest.raises(ValueError):
        ops.sparse_points(bits, (9, 8, 8))                                 # bits of another grid


# ---------------------------------------------------------------- 2. the points of a list of ids

def test_gen_grid_points_at_equals_the_rows_of_gen_grid_points(dev, ops):
    for c1, c2, reso in ((B.C1, B.C2, B.RESO), ((-1.1, -0.7, -0.3), (0.9, 1.3, 0.77), (9, 8, 7)), ((0.1, 0.2, 0.3), (0.7, 1.9, 2.3), (3, 1, 5))):
        total = reso[0] * reso[1] * reso[2]
        xyz, vd = ops.gen_grid_points(c1, c2, reso, device=dev)
        rs = np.random.RandomState(4)
        lists = [np.arange(total), np.sort(rs.choice(total, total // 3, replace=False)), rs.randint(0, total, 50), np.array([total - 1, 0, 0])]
        for ids_np in lists:
            ids = torch.from_numpy(ids_np.astype(np.int32)).to(dev)
            got_xyz, got_vd = ops.gen_grid_points_at(c1, c2, reso, ids)
            assert torch.equal(got_xyz, xyz[ids.long()]) and torch.equal(got_vd, vd[ids.long()])
            only_xyz, none = ops.gen_grid_points_at(c1, c2, reso, ids, viewdirs=False)
            assert none is None and torch.equal(only_xyz, got_xyz)
        bad = torch.tensor([3, -1, total, 5, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=dev)
        got_xyz, got_vd = ops.gen_grid_points_at(c1, c2, reso, bad)
        ok = torch.tensor([True, False, False, True, False, False], device=dev)
        assert torch.isnan(got_xyz[~ok]).all() and torch.isnan(got_vd[~ok]).all()
        assert torch.equal(got_xyz[ok], xyz[bad[ok].long()]) and torch.equal(got_vd[ok], vd[bad[ok].long()])
    empty_xyz, empty_vd = ops.gen_grid_points_at(B.C1, B.C2, B.RESO, torch.empty((0,), dtype=torch.int32, device=dev))
    assert tuple(empty_xyz.shape) == tuple(empty_vd.shape) == (0, 3)


# ---------------------------------------------------------------- 3. the bytes of the dense march

@pytest.mark.parametrize("kind", KINDS, ids=["rgba", "L0", "L1", "L2"])
def test_sparse_renders_the_bytes_of_the_dense_march(dev, ops, bake, common, kind):
    from pixelnerf_amd import util
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    keyword_sets = (dict(skip=True), dict(skip=True, terminate=1e-2), dict(skip=True, white_bkgd=True))
    for thr in (0.0, 10.0):
        dense = common["dense"][kind, thr]
        sp = dense.sparse()
        assert isinstance(sp, bake.SparseBakedVolume) and sp.degree == (None if kind == "rgba" else kind)
        assert 0 < sp.n_rows < P_TOTAL and (thr > 0 or kind != "rgba" or sp.n_rows == 198)
        assert tuple(sp.rows.shape) == (sp.n_rows,) + tuple(common["np"][kind].shape[3:]) and sp.occupancy is dense.occupancy
        assert sp.nbytes == 4 * (sp.rows.numel() + P_TOTAL + sp.occupancy.bits.numel()) < common["np"][kind].nbytes
        per_point = torch.from_numpy(common["np"][kind]).to(dev).reshape(P_TOTAL, *sp.rows.shape[1:])
        assert torch.equal(sp.rows, per_point[sp.ids.long()])
        for setting, (_, _, step) in B.SETTINGS.items():
            rays = common["rays"][setting]
            for kw in keyword_sets:
                a, b = sp.render(rays, step=step, **kw), dense.render(rays, step=step, **kw)
                assert _equal(a, b), (thr, setting, kw)
                assert _equal(a, sp.render(rays, step=step, **kw)), (thr, setting, kw)          # two calls, the same bytes
            assert float(a.alpha.max()) > 0.5                               # (not an empty image)
            for kw in (dict(skip=False), dict(skip=False, terminate=1e-2)):
                with pytest.raises(ValueError, match="skip=False"):
                    sp.render(rays, step=step, **kw)
        assert _equal(sp.render(rays), dense.render(rays))                 # step=None: the smallest cell edge
    # a foreign grid: the dense march with ITS bits
    dense = common["dense"][kind, 0.0]
    sigma = torch.from_numpy(np.ascontiguousarray(B.common_volume()[..., 3])).to(dev)
    grid = OccupancyGrid.from_density(sigma, B.C1, B.C2, 5.0, dilate=1)
    sp = dense.sparse(grid)
    assert sp.occupancy is grid and 0 < sp.n_rows < P_TOTAL and sp.n_rows != dense.sparse().n_rows
    for setting, (_, _, step) in B.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in (dict(), dict(terminate=1e-2), dict(white_bkgd=True)):
            a = sp.render(rays, step=step, **kw)
            assert _equal(a, _dense_march(ops, dense, rays, step, grid.bits, **kw)), (setting, kw)
        assert float(a.alpha.max()) > 0.5
    with pytest.raises(ValueError, match="spans"):
        dense.sparse(OccupancyGrid.from_density(sigma, B.C1, (1.1, 0.9, 0.8), 5.0, dilate=1))
    # the camera form is the array form
    poses = torch.stack([util.pose_spherical(30.0, -25.0, 3.0), util.pose_spherical(-110.0, 10.0, 2.6)]).float().to(dev)
    W, H, focal, c, z_near, z_far = 12, 10, (14.0, 11.5), (5.25, 5.5), 1.0, 4.6
    rays = util.gen_rays(poses, W, H, focal, z_near, z_far, c=c)
    sp = dense.sparse()
    for kw in (dict(), dict(white_bkgd=True, step=0.05), dict(terminate=1e-2)):
        views = sp.render_views(poses, W, H, focal, z_near, z_far, c=c, want_u8=True, **kw)
        assert _equal(views, sp.render(rays, **kw)), kw
        assert _equal(views, dense.render_views(poses, W, H, focal, z_near, z_far, c=c, **kw)), kw
        assert tuple(views.rgb.shape) == (2, H, W, 3) and views.rgb_u8.dtype == torch.uint8
        assert _equal(views, sp.render_views(poses, W, H, focal, z_near, z_far, c=c, **kw))
    assert float(views.alpha.max()) > 0.5 and float(views.alpha.min()) == 0.0


# ---------------------------------------------------------------- 4. an index value that names no pair of rows drops the sample

@pytest.mark.parametrize("kind", ["rgba", 2], ids=["rgba", "L2"])
def test_invalid_rows_are_dropped_not_read(dev, ops, common, kind):
    dense = common["dense"][kind, 0.0]
    sp = dense.sparse()
    M, degree = sp.n_rows, sp.degree
    nx, ny, nz = B.RESO
    sy, sx = nz, ny * nz
    # rows inside a larger allocation of NaN: a wrong kernel reads NaN, never memory that is not ours
    big = torch.full((M + 16,) + tuple(sp.rows.shape[1:]), float("nan"), device=dev)
    big[8:8 + M] = sp.rows
    rows = big[8:8 + M]
    assert rows.is_contiguous() and rows.data_ptr() % 16 == 0
    cells = SP.cells_from_bits(sp.occupancy.bits.cpu().numpy(), B.RESO)
    occupied = sorted((tuple(int(v) for v in c) for c in np.argwhere(cells)), key=lambda c: (c[0] - 4) ** 2 + (c[1] - 3) ** 2 + (c[2] - 3) ** 2)
    # five pair-base points of occupied cells near the centre of the box: the four bases of the nearest one and one more cell's
    (i, j, k), (i2, j2, k2) = occupied[0], occupied[6]
    p000 = (i * ny + j) * nz + k
    tampered = dict(zip((p000, p000 + sy, p000 + sx, p000 + sx + sy, (i2 * ny + j2) * nz + k2), (-1, -2, M - 1, M, M + 1)))
    assert len(tampered) == 5
    index = sp.index.clone()
    flat = index.view(-1)
    for p, value in tampered.items():
        assert 0 <= int(flat[p]) <= M - 2                                  # a kept pair base
        flat[p] = value
    # the cells with a tampered point among their four pair bases: (pi - a, pj - b, pk), a, b in {0, 1}, where they exist
    cleared = cells.copy()
    hit = set()
    for p in tampered:
        pi, pj, pk = p // sx, (p // sy) % ny, p % nz
        for a in (0, 1):
            for b in (0, 1):
                ci, cj = pi - a, pj - b
                if 0 <= ci <= nx - 2 and 0 <= cj <= ny - 2 and pk <= nz - 2:
                    hit.add((ci, cj, pk))
                    cleared[ci, cj, pk] = False
    assert 5 <= len(hit) <= 20 and int(cells.sum()) - int(cleared.sum()) >= 5
    bits_cleared = torch.from_numpy(SP.bits_from_cells(cleared)).to(dev)
    changed = False
    for setting, (_, _, step) in B.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in (dict(), dict(white_bkgd=True), dict(terminate=1e-2)):
            got = ops.baked_sparse_render(rays, rows, degree, index, sp.occupancy.bits, B.RESO, B.C1, B.C2, step, **kw)
            assert all(bool(torch.isfinite(t).all()) for t in got), (setting, kw)
            want = _dense_march(ops, dense, rays, step, bits_cleared, **kw)
            assert _equal(got, want), (setting, kw)
            changed = changed or not _equal(got, _dense_march(ops, dense, rays, step, sp.occupancy.bits, **kw))
            # the untampered index through the same allocation: the plain sparse render
            assert _equal(ops.baked_sparse_render(rays, rows, degree, sp.index, sp.occupancy.bits, B.RESO, B.C1, B.C2, step, **kw),
                          _dense_march(ops, dense, rays, step, sp.occupancy.bits, **kw))
    assert changed                                                         # some ray went through a tampered cell
    assert torch.isnan(big[:8]).all() and torch.isnan(big[8 + M:]).all()


# ---------------------------------------------------------------- 5. nothing kept: the background

def test_an_empty_volume_renders_the_background(dev, ops, bake):
    rays = torch.from_numpy(B.common_rays("n40")).to(dev)
    step = B.SETTINGS["n40"][2]
    bits, _ = ops.occupancy_build(torch.zeros(B.RESO, device=dev), 0.0, dilate=0)
    index, ids = ops.sparse_points(bits, B.RESO)
    assert ids.numel() == 0 and bool((index == -1).all())
    for degree, shape in ((None, (0, 4)), (0, (0, 1, 4)), (2, (0, 9, 4))):
        rows = torch.empty(shape, device=dev)
        for white in (False, True):
            rgb, depth, alpha = ops.baked_sparse_render(rays, rows, degree, index, bits, B.RESO, B.C1, B.C2, step, white_bkgd=white)
            assert (rgb == (1.0 if white else 0.0)).all() and (depth == 0).all() and (alpha == 0).all()
    for dense in (bake.BakedVolume.from_tensor(torch.zeros(B.RESO + (4,), device=dev), B.C1, B.C2),
                  bake.BakedSHVolume.from_tensor(torch.zeros(B.RESO + (9, 4), device=dev), B.C1, B.C2)):
        sp = dense.sparse()
        assert sp.n_rows == 0 and tuple(sp.to_dense().shape) == tuple((dense.vol if hasattr(dense, "vol") else dense.coef).shape)
        for white in (False, True):
            out = sp.render(rays, step=step, white_bkgd=white)
            assert (out.rgb == (1.0 if white else 0.0)).all() and (out.depth == 0).all() and (out.alpha == 0).all()
    # full bits over an index that keeps nothing (M = 0): every sample is dropped, nothing is read
    full, _ = ops.occupancy_build(torch.ones(B.RESO, device=dev), 0.0, dilate=0)
    rgb, depth, alpha = ops.baked_sparse_render(rays, torch.empty((0, 4), device=dev), None, index, full, B.RESO, B.C1, B.C2, step)
    assert (rgb == 0).all() and (depth == 0).all() and (alpha == 0).all()


# ---------------------------------------------------------------- 6. the sparse bake, stub networks

class _Stub(torch.nn.Module):
    """net(xyz (1,N,3), coarse=, viewdirs=(1,N,3)) -> (1,N,4): an element-wise function of the point and the direction (a row does
    not depend on its place in the batch); `seen` records the number of points of every pass"""
    use_viewdirs = True

    def __init__(self, dev):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.seen = []

    def forward(self, xyz, coarse=True, viewdirs=None):
        self.seen.append(xyz.shape[1])
        p, d = xyz[0], viewdirs[0]
        rgb = (0.5 + 0.3 * torch.sin(3.0 * p) + 0.1 * d).clamp(0.0, 1.0)
        sigma = (2.0 + p[:, :1] * d[:, 1:2] + p[:, 2:3] * p[:, 1:2] + d[:, :1] * d[:, 2:3]).clamp_min(0.0)
        return torch.cat((rgb, sigma), dim=1)[None]


class Plain(torch.nn.Module):
    use_viewdirs = False

    def __init__(self, dev):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.seen = []

    def forward(self, xyz, coarse=True, viewdirs=None):
        assert viewdirs is None
        self.seen.append(xyz.shape[1])
        return torch.cat((xyz[0].abs().clamp(0, 1), xyz[0, :, :1] ** 2), dim=1)[None]


def _one_point_grid(dev, reso, c1, c2):
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    field = torch.zeros(reso, device=dev)
    field[reso[0] - 2, 1, 1] = 1.0
    return OccupancyGrid.from_density(field, c1, c2, 0.0, dilate=0)


def _sparse_bake_equals_dense(bake, net, occ, reso, c1, c2, seen=None, **kw):
    """rows == dense[ids] for RGBA and degree 2, whatever eval_batch_size, run to run; with `seen`, the points per pass"""
    P = reso[0] * reso[1] * reso[2]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                    # the fake-direction / no-view-direction warnings
        dense_rgba = bake.BakedVolume.from_model(net, c1, c2, reso, **kw).vol.reshape(P, 4)
        dense_sh = bake.BakedSHVolume.from_model(net, c1, c2, reso, degree=2, n_dirs=18, **kw).coef
        dense_sh = dense_sh.reshape(P, -1, 4)
        passes = 18 if getattr(net, "use_viewdirs", False) else 1
        if seen is not None:
            assert seen == [P] * (1 + passes)
            del seen[:]
        sp = bake.SparseBakedVolume.from_model(net, c1, c2, reso, occ, **kw)
        M = sp.n_rows
        assert 0 < M < P and (P % 2 == 1 or M % 2 == 0) and sp.degree is None and tuple(sp.rows.shape) == (M, 4)
        assert torch.equal(sp.rows, dense_rgba[sp.ids.long()])
        sh = bake.SparseBakedVolume.from_model(net, c1, c2, reso, occ, degree=2, n_dirs=18, **kw)
        assert sh.degree == (2 if passes > 1 else 0) and torch.equal(sh.ids, sp.ids) and torch.equal(sh.index, sp.index)
        assert torch.equal(sh.rows, dense_sh[sp.ids.long()])
        if seen is not None:
            assert seen == [M] * (1 + passes)                              # M points per pass, not P
            del seen[:]
        for again in (dict(eval_batch_size=7), dict()):
            assert torch.equal(bake.SparseBakedVolume.from_model(net, c1, c2, reso, occ, eval_batch_size=again.get("eval_batch_size", 100000),
                                                                 **kw).rows, sp.rows)
            assert torch.equal(bake.SparseBakedVolume.from_model(net, c1, c2, reso, occ, degree=2, n_dirs=18,
                                                                 eval_batch_size=again.get("eval_batch_size", 100000), **kw).rows, sh.rows)
        if seen is not None:
            chunks = [6] * (M // 6) + ([M % 6] if M % 6 else [])
            assert seen == chunks + [n for n in chunks for _ in range(passes)] + [M] * (1 + passes)
            del seen[:]
    return sp, sh


@pytest.mark.parametrize("reso", [(5, 4, 3), (5, 3, 3)], ids=["P even", "P odd"])
def test_sparse_bake_of_stub_networks(dev, bake, reso):
    c1, c2 = (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)
    occ = _one_point_grid(dev, reso, c1, c2)
    assert int(occ.n_occupied) == 8
    for net in (_Stub(dev), Plain(dev)):
        net.train()
        sp, sh = _sparse_bake_equals_dense(bake, net, occ, reso, c1, c2, seen=net.seen)
        assert net.training                                                # the flag is restored
        assert sp.occupancy is occ and sp.reso == reso and sp.c1 == c1 and sp.c2 == c2
    with pytest.warns(UserWarning, match="no view directions"):
        bake.SparseBakedVolume.from_model(Plain(dev), c1, c2, reso, occ, degree=2, n_dirs=18)
    with pytest.raises(ValueError):
        bake.SparseBakedVolume.from_model(_Stub(dev), c1, c2, reso, occ, degree=2, n_dirs=17)
    with pytest.raises(ValueError):
        bake.SparseBakedVolume.from_model(_Stub(dev), c1, c2, reso, occ, viewdirs="centre")
    # a constant direction, as BakedVolume.from_model takes it
    net = _Stub(dev)
    fixed = bake.SparseBakedVolume.from_model(net, c1, c2, reso, occ, viewdirs=(0.0, -2.0, 0.0))
    want = bake.BakedVolume.from_model(net, c1, c2, reso, viewdirs=(0.0, -2.0, 0.0)).vol.reshape(-1, 4)
    assert torch.equal(fixed.rows, want[fixed.ids.long()])


# ---------------------------------------------------------------- 7. the sparse bake, the real network

@pytest.mark.parametrize("precision", [None, "f32"], ids=["default", "f32"])
def test_sparse_bake_through_the_model(dev, bake, precision):
    from helpers import scene_for
    from test_api_gpu import build_net
    scene, _ = scene_for("sn64")
    net = build_net(dev, scene, precision=precision)
    assert net.use_viewdirs and net.mlp_fine is not None
    c1, c2 = (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)
    for reso in ((5, 4, 3), (5, 3, 3)):                                    # P even; P odd
        occ = _one_point_grid(dev, reso, c1, c2)
        sp, sh = _sparse_bake_equals_dense(bake, net, occ, reso, c1, c2)
        assert float(sh.rows.abs().max()) > 0.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            coarse = bake.SparseBakedVolume.from_model(net, c1, c2, reso, occ, coarse=True)
            want = bake.BakedVolume.from_model(net, c1, c2, reso, coarse=True).vol.reshape(-1, 4)
        assert torch.equal(coarse.rows, want[coarse.ids.long()]) and not torch.equal(coarse.rows, sp.rows)


# ---------------------------------------------------------------- 8. the state, and the dense form

@pytest.mark.parametrize("kind", ["rgba", 2], ids=["rgba", "L2"])
def test_state_round_trip_and_to_dense(dev, ops, bake, common, kind):
    dense = common["dense"][kind, 10.0]
    sp = dense.sparse()
    state = {k: t.cpu() for k, t in sp.state_dict().items()}
    assert sorted(state) == ["bits", "c1", "c2", "reso", "rows"]
    back = bake.SparseBakedVolume.from_state_dict(state, device=dev)
    assert torch.equal(back.rows, sp.rows) and torch.equal(back.index, sp.index) and torch.equal(back.ids, sp.ids)
    assert torch.equal(back.occupancy.bits, sp.occupancy.bits) and int(back.occupancy.n_occupied) == int(sp.occupancy.n_occupied)
    assert back.degree == sp.degree and back.reso == sp.reso and back.c1 == sp.c1 and back.c2 == sp.c2 and back.nbytes == sp.nbytes
    full = sp.to_dense()
    kept = torch.zeros(P_TOTAL, dtype=torch.bool, device=dev)
    kept[sp.ids.long()] = True
    per_point = full.reshape(P_TOTAL, -1)
    assert tuple(full.shape) == tuple(common["np"][kind].shape) and bool((per_point[~kept] == 0).all())
    assert torch.equal(per_point[kept], torch.from_numpy(common["np"][kind]).to(dev).reshape(P_TOTAL, -1)[kept])
    wrapped = (bake.BakedVolume if kind == "rgba" else bake.BakedSHVolume).from_tensor(full, sp.c1, sp.c2)
    for setting, (_, _, step) in B.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in (dict(), dict(white_bkgd=True, terminate=1e-2)):
            a = sp.render(rays, step=step, **kw)
            assert _equal(a, back.render(rays, step=step, **kw)), (setting, kw)
            assert _equal(a, _dense_march(ops, wrapped, rays, step, sp.occupancy.bits, **kw)), (setting, kw)
        assert float(a.alpha.max()) > 0.5
