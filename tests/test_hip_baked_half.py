"""GPU tests (-m gpu) of the half-precision baked volumes: pnr_baked_half_render_rays / _views and pnr_baked_sparse_half_render_rays /
_views through ops.baked_half_render(_views), ops.baked_sparse_half_render(_views) and the dtype surface of util.bake.  The contract
needs no tolerance (fp16 -> fp32 is exact): marching a half volume gives the BYTES of the fp32 march of the same values widened to
fp32 -- every comparison of a march here is torch.equal.  The inputs are tests/baked_half_ref.py's (their own checks:
tests/test_baked_half_host.py); the one comparison with a bar is the fp64 restatement's, at the fp32 tests' bar."""
import warnings

import numpy as np
import pytest
import torch

import baked_half_ref as HR
import baked_ref as B
import sparse_baked_ref as SP

pytestmark = pytest.mark.gpu

P_TOTAL = B.RESO[0] * B.RESO[1] * B.RESO[2]
KW_SETS = [dict(white_bkgd=w, terminate=t) for w in (False, True) for t in (0.0, 1e-2)]


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


def _cls(bake, kind):
    return bake.BakedVolume if kind == "rgba" else bake.BakedSHVolume


def _stored(v):
    return v.vol if hasattr(v, "vol") else v.coef if hasattr(v, "coef") else v.rows


def _to_half(bake, t):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                    # the fixture's one saturated sigma
        return bake.to_half(t)


@pytest.fixture(scope="module")
def common(dev, bake):
    """per kind: the unrounded fixture `a32`, h = to_half(fixture) as `h16`, its widening `w32`, and the three volume objects
    (never modified); the rays per setting"""
    case = {"rays": {s: torch.from_numpy(B.common_rays(s)).to(dev) for s in B.SETTINGS}}
    for kind in HR.KINDS:
        a32 = torch.from_numpy(HR.fixture(kind)).to(dev)
        h16 = _to_half(bake, a32)
        assert h16.dtype == torch.float16 and np.array_equal(h16.cpu().view(torch.int16).numpy(), HR.half_round(HR.fixture(kind)).view(np.int16))
        w32 = h16.float()
        case[kind] = dict(a32=a32, h16=h16, w32=w32, plain=_cls(bake, kind).from_tensor(a32, B.C1, B.C2),
                          half=_cls(bake, kind).from_tensor(h16, B.C1, B.C2), wide=_cls(bake, kind).from_tensor(w32, B.C1, B.C2))
    return case


def _triple(x):
    return tuple(x) if isinstance(x, tuple) else (x.rgb, x.depth, x.alpha)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(_triple(a), _triple(b)))


def _march32(ops, kind, t, rays, step, bits, reso=B.RESO, **kw):
    if kind == "rgba":
        return ops.baked_render(rays, t, reso, B.C1, B.C2, step, bits=bits, **kw)
    return ops.baked_sh_render(rays, t, kind, reso, B.C1, B.C2, step, bits=bits, **kw)


def _march16(ops, kind, t, rays, step, bits, reso=B.RESO, **kw):
    return ops.baked_half_render(rays, t, -1 if kind == "rgba" else kind, reso, B.C1, B.C2, step, bits=bits, **kw)


def _cameras(dev):
    from pixelnerf_amd import util
    poses = torch.stack([util.pose_spherical(30.0, -25.0, 3.0), util.pose_spherical(-110.0, 10.0, 2.6)]).float().to(dev)
    return poses, 12, 10, (14.0, 11.5), (5.25, 5.5), 1.0, 4.6


# ---------------------------------------------------------------- 1. the contract

@pytest.mark.parametrize("kind", HR.KINDS, ids=HR.KIND_IDS)
def test_half_march_gives_the_bytes_of_the_fp32_march_of_the_widened_values(dev, ops, common, kind):
    from pixelnerf_amd import util
    HR.check_preconditions(kind)
    c = common[kind]
    half, wide, plain = c["half"], c["wide"], c["plain"]
    assert half.dtype == torch.float16 and wide.dtype == plain.dtype == torch.float32
    assert torch.equal(half.occupancy.bits, wide.occupancy.bits)           # the skip grid of the widened values
    differs = False
    for setting, (_, _, step) in B.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in KW_SETS:
            for bits in (None, half.occupancy.bits):
                got = _march16(ops, kind, c["h16"], rays, step, bits, **kw)
                assert all(t.dtype == torch.float32 for t in got)
                assert _equal(got, _march32(ops, kind, c["w32"], rays, step, bits, **kw)), (setting, kw, bits is None)
                assert _equal(got, _march16(ops, kind, c["h16"], rays, step, bits, **kw))        # two calls, the same bytes
                assert all(bool(torch.isfinite(t).all()) for t in got)
                differs = differs or not _equal(got, _march32(ops, kind, c["a32"], rays, step, bits, **kw))
            for skip in (False, True):                                     # the classes dispatch on the dtype
                a = half.render(rays, step=step, skip=skip, **kw)
                assert _equal(a, wide.render(rays, step=step, skip=skip, **kw)), (setting, kw, skip)
                assert _equal(a, _march16(ops, kind, c["h16"], rays, step, half.occupancy.bits if skip else None, **kw))
            assert _equal(half.render(rays, step=step, skip=True, **kw), half.render(rays, step=step, skip=False, **kw))
        assert float(a.alpha.max()) > 0.5                                  # (not an empty image)
    assert differs                                                         # not the march of the unrounded values
    # the camera form: 2 views of 12 x 10
    poses, W, H, focal, cc, z_near, z_far = _cameras(dev)
    rays = util.gen_rays(poses, W, H, focal, z_near, z_far, c=cc)
    degree = -1 if kind == "rgba" else kind
    for kw in KW_SETS:
        for skip in (False, True):
            views = half.render_views(poses, W, H, focal, z_near, z_far, c=cc, skip=skip, want_u8=True, **kw)
            assert _equal(views, wide.render_views(poses, W, H, focal, z_near, z_far, c=cc, skip=skip, **kw)), (kw, skip)
            assert _equal(views, half.render(rays, skip=skip, **kw)), (kw, skip)
            assert tuple(views.rgb.shape) == (2, H, W, 3) and views.rgb_u8.dtype == torch.uint8
            bits = half.occupancy.bits if skip else None
            direct = ops.baked_half_render_views(poses, W, H, focal, cc, z_near, z_far, c["h16"], degree, B.RESO, B.C1, B.C2,
                                                 min(half.cell_size), bits=bits, **kw)
            assert _equal((views.rgb.reshape(-1, 3), views.depth.reshape(-1), views.alpha.reshape(-1)), direct)
    assert float(views.alpha.max()) > 0.5 and float(views.alpha.min()) == 0.0
    assert not _equal(views, plain.render_views(poses, W, H, focal, z_near, z_far, c=cc, skip=True, **KW_SETS[-1]))


# ---------------------------------------------------------------- 2. sparse

def _grid_of_cells(dev, cells, c1=B.C1, c2=B.C2):
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    bits = torch.from_numpy(SP.bits_from_cells(cells)).to(dev)
    reso = tuple(n + 1 for n in cells.shape)
    return OccupancyGrid(bits, reso, c1, c2, float("nan"), 0, torch.tensor(int(cells.sum()), dtype=torch.int32, device=dev))


@pytest.mark.parametrize("kind", HR.KINDS, ids=HR.KIND_IDS)
def test_sparse_half_equals_the_fp32_sparse_march_and_the_half_dense_march(dev, ops, bake, common, kind):
    c = common[kind]
    half, degree = c["half"], (None if kind == "rgba" else kind)
    # (a) the volume's own skip grid
    sp = half.sparse()
    assert isinstance(sp, bake.SparseBakedVolume) and sp.dtype == torch.float16 and sp.degree == degree and 0 < sp.n_rows < P_TOTAL
    assert torch.equal(sp.rows, c["h16"].reshape(P_TOTAL, *sp.rows.shape[1:])[sp.ids.long()])       # gathered, no arithmetic
    sp32 = sp.float()
    assert sp32.dtype == torch.float32 and sp32.index is sp.index and sp32.ids is sp.ids and sp32.occupancy is sp.occupancy
    assert torch.equal(sp32.rows, sp.rows.float()) and sp.nbytes == sp32.nbytes - 2 * sp.rows.numel()
    for setting, (_, _, step) in B.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in KW_SETS:
            a = sp.render(rays, step=step, **kw)
            assert _equal(a, sp32.render(rays, step=step, **kw)), (setting, kw)
            assert _equal(a, half.render(rays, step=step, skip=True, **kw)), (setting, kw)
            assert _equal(a, ops.baked_sparse_half_render(rays, sp.rows, degree, sp.index, sp.occupancy.bits, B.RESO, B.C1, B.C2, step, **kw))
        assert float(a.alpha.max()) > 0.5
    poses, W, H, focal, cc, z_near, z_far = _cameras(dev)
    for kw in KW_SETS:
        views = sp.render_views(poses, W, H, focal, z_near, z_far, c=cc, **kw)
        assert _equal(views, sp32.render_views(poses, W, H, focal, z_near, z_far, c=cc, **kw)), kw
        assert _equal(views, half.render_views(poses, W, H, focal, z_near, z_far, c=cc, skip=True, **kw)), kw
    assert float(views.alpha.max()) > 0.5
    # (b) foreign grids of tests/sparse_baked_ref.py on crops of the fixture that hold sigma > 0 (65504 and the saturated one too):
    # all cells on, and (3,3,3) with only the last cell on (27 points: the last one has no partner)
    grids = SP.grids()
    for name, crop in (("full", c["h16"][4:9, 4:8, 2:5]), ("3x3x3 last", c["h16"][4:7, 3:6, 2:5])):
        cells = grids[name]
        reso = tuple(n + 1 for n in cells.shape)
        crop = crop.contiguous()
        assert tuple(crop.shape[:3]) == reso and float(crop[..., 3].float().max() if kind == "rgba" else crop[..., 0, 3].float().max()) > 0
        dense = _cls(bake, kind).from_tensor(crop, B.C1, B.C2)
        grid = _grid_of_cells(dev, cells)
        sp = dense.sparse(grid)
        assert sp.dtype == torch.float16 and sp.occupancy is grid and sp.n_rows == SP.sparse_points(cells)[1].size
        sp32 = sp.float()
        hit = False
        for setting, (_, _, step) in B.SETTINGS.items():
            rays = common["rays"][setting]
            for kw in KW_SETS:
                a = sp.render(rays, step=step, **kw)
                assert _equal(a, sp32.render(rays, step=step, **kw)), (name, setting, kw)
                assert _equal(a, _march16(ops, kind, crop, rays, step, grid.bits, reso=reso, **kw)), (name, setting, kw)
                assert _equal(a, _march32(ops, kind, crop.float(), rays, step, grid.bits, reso=reso, **kw)), (name, setting, kw)
            hit = hit or float(a.alpha.max()) > 0.0
        assert hit, name


@pytest.mark.parametrize("kind", ["rgba", 2], ids=["rgba", "L2"])
def test_invalid_half_rows_are_dropped_not_read(dev, ops, common, kind):
    """tests/test_hip_sparse_baked.py's test_invalid_rows_are_dropped_not_read, for fp16 rows"""
    c = common[kind]
    half = c["half"]
    sp = half.sparse()
    M, degree = sp.n_rows, sp.degree
    nx, ny, nz = B.RESO
    sy, sx = nz, ny * nz
    # rows inside a larger allocation of NaN: a wrong kernel reads NaN, never memory that is not ours
    big = torch.full((M + 16,) + tuple(sp.rows.shape[1:]), float("nan"), dtype=torch.float16, device=dev)
    big[8:8 + M] = sp.rows
    rows = big[8:8 + M]
    assert rows.is_contiguous() and rows.data_ptr() % 16 == 0 and rows.dtype == torch.float16
    cells = SP.cells_from_bits(sp.occupancy.bits.cpu().numpy(), B.RESO)
    occupied = sorted((tuple(int(v) for v in cc) for cc in np.argwhere(cells)), key=lambda cc: (cc[0] - 4) ** 2 + (cc[1] - 3) ** 2 + (cc[2] - 3) ** 2)
    (i, j, k), (i2, j2, k2) = occupied[0], occupied[6]
    p000 = (i * ny + j) * nz + k
    tampered = dict(zip((p000, p000 + sy, p000 + sx, p000 + sx + sy, (i2 * ny + j2) * nz + k2), (-1, -2, M - 1, M, M + 1)))
    assert len(tampered) == 5
    index = sp.index.clone()
    flat = index.view(-1)
    for p, value in tampered.items():
        assert 0 <= int(flat[p]) <= M - 2                                  # a kept pair base
        flat[p] = value
    cleared = cells.copy()
    for p in tampered:
        pi, pj, pk = p // sx, (p // sy) % ny, p % nz
        for a in (0, 1):
            for b in (0, 1):
                ci, cj = pi - a, pj - b
                if 0 <= ci <= nx - 2 and 0 <= cj <= ny - 2 and pk <= nz - 2:
                    cleared[ci, cj, pk] = False
    assert int(cells.sum()) - int(cleared.sum()) >= 5
    bits_cleared = torch.from_numpy(SP.bits_from_cells(cleared)).to(dev)
    changed = False
    for setting, (_, _, step) in B.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in (dict(), dict(white_bkgd=True), dict(terminate=1e-2)):
            got = ops.baked_sparse_half_render(rays, rows, degree, index, sp.occupancy.bits, B.RESO, B.C1, B.C2, step, **kw)
            assert all(bool(torch.isfinite(t).all()) for t in got), (setting, kw)
            assert _equal(got, _march16(ops, kind, c["h16"], rays, step, bits_cleared, **kw)), (setting, kw)
            assert _equal(got, _march32(ops, kind, c["w32"], rays, step, bits_cleared, **kw)), (setting, kw)
            untampered = _march16(ops, kind, c["h16"], rays, step, sp.occupancy.bits, **kw)
            changed = changed or not _equal(got, untampered)
            assert _equal(ops.baked_sparse_half_render(rays, rows, degree, sp.index, sp.occupancy.bits, B.RESO, B.C1, B.C2, step, **kw),
                          untampered)
    assert changed                                                         # some ray went through a tampered cell
    assert torch.isnan(big[:8]).all() and torch.isnan(big[8 + M:]).all()
    # nothing kept: the background, nothing read
    empty_bits, _ = ops.occupancy_build(torch.zeros(B.RESO, device=dev), 0.0, dilate=0)
    empty_index, ids = ops.sparse_points(empty_bits, B.RESO)
    assert ids.numel() == 0
    none = torch.empty((0,) + tuple(sp.rows.shape[1:]), dtype=torch.float16, device=dev)
    for white in (False, True):
        rgb, depth, alpha = ops.baked_sparse_half_render(rays, none, degree, empty_index, empty_bits, B.RESO, B.C1, B.C2, step, white_bkgd=white)
        assert (rgb == (1.0 if white else 0.0)).all() and (depth == 0).all() and (alpha == 0).all()


# ---------------------------------------------------------------- 3. skipping stays exact after the rounding

@pytest.mark.parametrize("kind", HR.KINDS, ids=HR.KIND_IDS)
def test_skip_is_exact_after_rounding(dev, bake, common, kind):
    t32 = torch.from_numpy(HR.tiny_sigma(kind)).to(dev)
    plain = _cls(bake, kind).from_tensor(t32, B.C1, B.C2)
    half = plain.half() if kind != "rgba" else _cls(bake, kind).from_tensor(_to_half(bake, t32), B.C1, B.C2)
    assert half.dtype == torch.float16
    on32 = SP.cells_from_bits(plain.occupancy.bits.cpu().numpy(), B.RESO)
    on16 = SP.cells_from_bits(half.occupancy.bits.cpu().numpy(), B.RESO)
    assert on32[2:4, 2:4, 2:4].all() and not on16[2:4, 2:4, 2:4].any()     # the cells inside the block of tiny sigmas
    assert (on32 | ~on16).all() and int(on16.sum()) < int(on32.sum())      # the half grid only drops cells
    assert torch.equal(half.occupancy.bits, half.float().occupancy.bits)
    if kind != "rgba":                                                     # through sigma_bound(): of the widened coefficients
        assert torch.equal(half.sigma_bound(), half.float().sigma_bound())
        assert float(plain.sigma_bound()[3, 3, 3]) > 0.0 and float(half.sigma_bound()[3, 3, 3]) == 0.0
    for setting, (_, _, step) in B.SETTINGS.items():
        rays = common["rays"][setting]
        for kw in KW_SETS:
            a = half.render(rays, step=step, skip=True, **kw)
            assert _equal(a, half.render(rays, step=step, skip=False, **kw)), (setting, kw)
            assert _equal(a, half.float().render(rays, step=step, skip=True, **kw)), (setting, kw)
        assert float(a.alpha.max()) > 0.5


# ---------------------------------------------------------------- 4. against the fp64 restatement, at the fp32 tests' bar

@pytest.mark.parametrize("kind,setting", [("rgba", "n133"), (0, "n40"), (1, "n133"), (2, "n40")], ids=HR.KIND_IDS)
def test_parity_with_the_fp64_restatement_of_the_widened_volume(common, kind, setting):
    step = B.SETTINGS[setting][2]
    rays_np = B.common_rays(setting)
    wide_np = common[kind]["w32"].cpu().numpy()
    r64 = HR.render_ref(kind, rays_np, wide_np, step, dtype=np.float64)
    r32 = HR.render_ref(kind, rays_np, wide_np, step, dtype=np.float32)
    out = common[kind]["half"].render(common["rays"][setting], step=step, skip=False)
    got = tuple(t.cpu().numpy() for t in (out.rgb, out.depth, out.alpha))
    gap, err = B.gaps(r32, r64), B.gaps(got, r64)
    print(f"{kind} {setting}: fp32 - fp64 gap rgb {gap[0]:.3e} depth {gap[1]:.3e} alpha {gap[2]:.3e}; "
          f"half kernel - fp64 rgb {err[0]:.3e} depth {err[1]:.3e} alpha {err[2]:.3e}")
    for name, g, e in zip(("rgb", "depth", "alpha"), gap, err):
        assert 0.0 < g < 1e-4, (name, g)
        assert e <= 4.0 * g, (name, e, 4.0 * g)
    for r in (26, 27, 28, 29, 36):                                         # the misses and the near >= far ray: exactly the background
        assert (got[0][r] == 0.0).all() and got[1][r] == 0.0 and got[2][r] == 0.0, r


# ---------------------------------------------------------------- 5. the bake

class _Stub(torch.nn.Module):
    """net(xyz (1,N,3), coarse=, viewdirs=(1,N,3)) -> (1,N,4): an element-wise function of the point and the direction (the stub
    of tests/test_hip_sparse_baked.py, restated), with one sigma beyond the fp16 range"""
    use_viewdirs = True

    def __init__(self, dev):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))

    def forward(self, xyz, coarse=True, viewdirs=None):
        p, d = xyz[0], viewdirs[0]
        rgb = (0.5 + 0.3 * torch.sin(3.0 * p) + 0.1 * d).clamp(0.0, 1.0)
        sigma = (2.0 + p[:, :1] * d[:, 1:2] + p[:, 2:3] * p[:, 1:2] + d[:, :1] * d[:, 2:3]).clamp_min(0.0)
        sigma = torch.where(p.sum(dim=1, keepdim=True) > 2.5, torch.full_like(sigma, 3e5), sigma)   # the last grid point alone
        return torch.cat((rgb, sigma), dim=1)[None]


class _Plain(torch.nn.Module):
    use_viewdirs = False

    def __init__(self, dev):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))

    def forward(self, xyz, coarse=True, viewdirs=None):
        assert viewdirs is None
        return torch.cat((xyz[0].abs().clamp(0, 1), xyz[0, :, :1] ** 2), dim=1)[None]


def _half_bake_is_to_half_of_the_bake(dev, bake, net, reso, c1, c2):
    """from_model(dtype=float16) holds the bytes of to_half(from_model()) for the three classes -> the three half volumes"""
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    field = torch.zeros(reso, device=dev)
    field[reso[0] - 2:, 1:, 1:] = 1.0
    occ = OccupancyGrid.from_density(field, c1, c2, 0.0, dilate=0)
    made = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                    # fake directions, no view directions, saturation
        for cls, kw in ((bake.BakedVolume, dict()), (bake.BakedSHVolume, dict(degree=2, n_dirs=18)),
                        (bake.SparseBakedVolume, dict(occupancy=occ)), (bake.SparseBakedVolume, dict(occupancy=occ, degree=2, n_dirs=18))):
            v32 = cls.from_model(net, c1, c2, reso, **kw)
            v16 = cls.from_model(net, c1, c2, reso, dtype=torch.float16, **kw)
            again = cls.from_model(net, c1, c2, reso, dtype=torch.float16, eval_batch_size=6, **kw)
            assert v32.dtype == torch.float32 and v16.dtype == torch.float16 and _stored(v16).shape == _stored(v32).shape
            assert torch.equal(_stored(v16), bake.to_half(_stored(v32))) and torch.equal(_stored(again), _stored(v16))
            assert torch.equal(_stored(v32.half()), _stored(v16))
            assert torch.equal(_stored(cls.from_model(net, c1, c2, reso, dtype=torch.float32, **kw)), _stored(v32))
            assert float(_stored(v16).float().abs().max()) > 0.0
            made.append(v16)
    return made


def test_half_bake_of_stub_networks(dev, bake):
    c1, c2 = (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)
    for reso in ((5, 4, 3), (5, 3, 3)):
        for net in (_Stub(dev), _Plain(dev)):
            net.train()
            made = _half_bake_is_to_half_of_the_bake(dev, bake, net, reso, c1, c2)
            assert net.training                                            # the flag is restored
    with pytest.warns(UserWarning, match="saturated"):                     # the stub's sigma of 3e5 at the last point
        bv = bake.BakedVolume.from_model(_Stub(dev), c1, c2, (5, 4, 3), viewdirs=(0.0, 0.0, 1.0), dtype=torch.float16)
    assert float(bv.vol[-1, -1, -1, 3]) == 65504.0 and bool(torch.isfinite(bv.vol).all())
    with pytest.raises(ValueError, match="dtype"):
        bake.BakedVolume.from_model(_Stub(dev), c1, c2, (5, 4, 3), dtype=torch.float64)


def test_half_bake_through_the_model(dev, bake):
    from helpers import scene_for
    from test_api_gpu import build_net
    scene, _ = scene_for("sn64")
    net = build_net(dev, scene)
    assert net.use_viewdirs and net.mlp_fine is not None
    made = _half_bake_is_to_half_of_the_bake(dev, bake, net, (5, 4, 3), (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8))
    rays = torch.tensor([[3.0, 0.1, 0.05, -1.0, 0.0, 0.0, 1.0, 5.0]], device=dev)
    for v in made:                                                         # usable as baked
        assert _equal(v.render(rays), v.float().render(rays))


# ---------------------------------------------------------------- 6. the surface

@pytest.mark.parametrize("kind", HR.KINDS, ids=HR.KIND_IDS)
def test_dtype_surface(dev, ops, bake, common, kind):
    c = common[kind]
    plain, half, wide = c["plain"], c["half"], c["wide"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h = plain.half()
    assert type(h) is type(plain) and h.dtype == torch.float16 and torch.equal(_stored(h), c["h16"])
    assert h.reso == plain.reso and h.c1 == plain.c1 and h.c2 == plain.c2 and h.skip_threshold == plain.skip_threshold
    assert torch.equal(_stored(h.float()), c["w32"]) and torch.equal(_stored(h.float().half()), c["h16"])     # stable
    assert torch.equal(_stored(half.half()), _stored(half)) and torch.equal(_stored(plain.float()), _stored(plain))
    assert half.nbytes * 2 == plain.nbytes == _stored(plain).numel() * 4
    rays, step = common["rays"]["n40"], B.SETTINGS["n40"][2]
    want = half.render(rays, step=step, white_bkgd=True, terminate=1e-2)
    # the state keeps dtype, bytes and renders; an fp32 state loads as before
    for v in (half, plain):
        state = {k: t.cpu() for k, t in v.state_dict().items()}
        key = "vol" if kind == "rgba" else "coef"
        assert state[key].dtype == v.dtype
        back = type(v).from_state_dict(state, device=dev)
        assert back.dtype == v.dtype and torch.equal(_stored(back), _stored(v)) and torch.equal(back.occupancy.bits, v.occupancy.bits)
        assert _equal(back.render(rays, step=step, white_bkgd=True, terminate=1e-2), v.render(rays, step=step, white_bkgd=True, terminate=1e-2))
    # sparse: to_dense keeps the dtype, the state round trip too
    sp = half.sparse()
    full = sp.to_dense()
    assert full.dtype == torch.float16 and tuple(full.shape) == tuple(c["h16"].shape)
    kept = torch.zeros(P_TOTAL, dtype=torch.bool, device=dev)
    kept[sp.ids.long()] = True
    per_point = full.reshape(P_TOTAL, -1)
    assert bool((per_point[~kept] == 0).all()) and torch.equal(per_point[kept], c["h16"].reshape(P_TOTAL, -1)[kept])
    state = {k: t.cpu() for k, t in sp.state_dict().items()}
    assert state["rows"].dtype == torch.float16
    back = bake.SparseBakedVolume.from_state_dict(state, device=dev)
    assert back.dtype == torch.float16 and torch.equal(back.rows, sp.rows) and torch.equal(back.index, sp.index) and back.nbytes == sp.nbytes
    assert _equal(back.render(rays, step=step, white_bkgd=True, terminate=1e-2), want)
    assert plain.sparse().to_dense().dtype == torch.float32
    ps = plain.sparse()                                                    # SparseBakedVolume.half(): rows converted, the rest shared
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sh = ps.half()
        assert torch.equal(sh.rows, bake.to_half(ps.rows))
    assert sh.dtype == torch.float16 and sh.index is ps.index and sh.ids is ps.ids and sh.occupancy is ps.occupancy
    assert torch.equal(sh.half().rows, sh.rows) and torch.equal(ps.float().rows, ps.rows)
    # an fp32 volume built after this change renders the bytes of the fp32 entries called directly
    direct = _march32(ops, kind, c["a32"], rays, step, plain.occupancy.bits, white_bkgd=True, terminate=1e-2)
    assert _equal(plain.render(rays, step=step, white_bkgd=True, terminate=1e-2), direct)
    if kind != "rgba":
        d = (0.3, -0.5, 0.8)
        a, b = half.at_direction(d), half.float().at_direction(d)
        assert isinstance(a, bake.BakedVolume) and a.dtype == torch.float32 and torch.equal(a.vol, b.vol)
        assert torch.equal(a.occupancy.bits, b.occupancy.bits)
