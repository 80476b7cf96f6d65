"""GPU tests (-m gpu) of the occupancy-grid ray culling: pnr_occupancy_build / pnr_occupancy_clip_rays / pnr_philox_noise_ids through
ops.occupancy_build / ops.occupancy_clip_rays / ops.philox_noise_ids, util.occupancy.OccupancyGrid, and the `occupancy=` keyword of
NeRFRenderer.forward / render_views.

Build: the bits equal the numpy restatement (tests/occ_ref.py build_ref) exactly.
Rendering: identities, no tolerance -- a pixel the grid keeps has the bits of the dense render, a pixel it culls is the background.
Clip: a one-sided bracket without exclusions, see test_clip_is_bracketed_by_shrunk_and_grown_cells."""
import numpy as np
import pytest
import torch

import occ_ref as R
from helpers import golden_setup, scene_for
from testdata import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


def _words(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- 1. build

def _build_field(shape, seed, thr):
    """seeded normal values, ~5 % of the points set EQUAL to the threshold, and a NaN, a +inf and a -inf where the grid has room"""
    rs = np.random.RandomState(seed)
    f = rs.standard_normal(shape).astype(np.float32)
    flat = f.reshape(-1)
    idx = rs.choice(flat.size, max(2, flat.size // 20), replace=False)
    flat[idx] = np.float32(thr)
    if flat.size > 8:
        far = rs.choice(np.setdiff1d(np.arange(flat.size), idx), 3, replace=False)
        flat[far] = (np.nan, np.inf, -np.inf)
    return f


@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 6, 7), (3, 4, 35), (9, 9, 9)], ids=lambda s: "x".join(map(str, s)))
def test_build_equals_the_restatement(ops, dev, shape):
    """2x2x2: one cell, dilate 4 reaches beyond the grid; 5x6x7: 120 cells end mid-word; 3x4x35: rows of 34 cells cross the word
    boundaries; 9x9x9: 512 cells = 16 full words.  Threshold 1.8: ~3.6 % of the points above it, so dilation has room to act."""
    thr = 1.8
    for seed in (0, 1):
        field = _build_field(shape, 10 * seed + shape[2], thr)
        if seed == 1:
            field = np.where(np.isfinite(field), np.minimum(field, np.float32(thr)), field).astype(np.float32)  # only == thr and specials
        f = torch.from_numpy(field).to(dev)
        cells = tuple(n - 1 for n in shape)
        for dilate in (0, 1, 2, 4):
            ref = R.build_ref(field, thr, dilate)
            bits, count = ops.occupancy_build(f, thr, dilate)
            assert bits.dtype == torch.int32 and bits.is_cuda and bits.shape == ((ref.size + 31) // 32,) and count.dim() == 0
            got, rest = R.unpack_bits(_words(bits), cells)
            assert np.array_equal(got, ref), (shape, seed, dilate)
            assert not rest.any()                                            # the unused high bits of the last word
            assert np.array_equal(_words(bits), R.pack_bits(ref))
            assert int(count) == int(ref.sum())
            again, count2 = ops.occupancy_build(f, thr, dilate)
            assert _words(again).tobytes() == _words(bits).tobytes() and int(count2) == int(count)
    # every point EQUAL to the threshold but one: the next float above it, then a NaN (the one cell of 2x2x2 turns occupied)
    last = tuple(n - 1 for n in shape)
    for value in (np.nextafter(np.float32(thr), np.float32(np.inf)), np.float32(np.nan)):
        field = np.full(shape, thr, np.float32)
        assert not R.build_ref(field, thr, 4).any()
        field[last[0], 0, last[2]] = value
        for dilate in (0, 4):
            ref = R.build_ref(field, thr, dilate)
            bits, count = ops.occupancy_build(torch.from_numpy(field).to(dev), thr, dilate)
            assert ref[-1, 0, -1] and np.array_equal(_words(bits), R.pack_bits(ref)) and int(count) == int(ref.sum()), (shape, value, dilate)
    # a single point above the threshold in a corner of the 9x9x9 grid: the dilated block, clipped by the grid
    if shape == (9, 9, 9):
        field = np.zeros(shape, np.float32)
        field[0, 8, 3] = 2.0
        for dilate, n in ((0, 2), (1, 2 * 2 * 4), (2, 3 * 3 * 6), (4, 5 * 5 * 8)):
            bits, count = ops.occupancy_build(torch.from_numpy(field).to(dev), thr, dilate)
            assert int(count) == n and np.array_equal(_words(bits), R.pack_bits(R.build_ref(field, thr, dilate))), dilate


def test_build_and_clip_refuse_invalid_arguments(ops, dev):
    lib = ops._lib.load()
    f = torch.zeros((4, 4, 4), device=dev)
    bits = torch.zeros((1,), dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    for d in (-1, 5):
        assert lib.pnr_occupancy_build(p(f), 4, 4, 4, 0.5, d, p(bits), None, None) == -1
    assert lib.pnr_occupancy_build(p(f), 4, 1, 4, 0.5, 1, p(bits), None, None) == -1
    assert lib.pnr_occupancy_build(p(f), 1292, 1292, 1292, 0.5, 1, p(bits), None, None) == -1
    assert lib.pnr_occupancy_build(p(f), 4, 4, 4, float("nan"), 1, p(bits), None, None) == -1
    assert lib.pnr_occupancy_build(p(f), 4, 4, 4, 0.5, 1, p(bits), None, None) == 0      # no count wanted: fine
    torch.cuda.synchronize()
    assert int(bits[0]) == 0
    with pytest.raises(ValueError, match="dilate"):
        ops.occupancy_build(f, 0.5, dilate=5)
    with pytest.raises(ValueError):
        ops.occupancy_build(torch.zeros((4, 1, 4), device=dev), 0.5)
    rays = torch.zeros((3, 8), device=dev)
    with pytest.raises(ValueError, match="bits"):
        ops.occupancy_clip_rays(rays, torch.zeros((2,), dtype=torch.int32, device=dev), (4, 4, 4), (-1,) * 3, (1,) * 3)
    with pytest.raises(ops._lib.PixelNerfHipError, match="pad"):
        ops.occupancy_clip_rays(rays, bits, (4, 4, 4), (-1,) * 3, (1,) * 3, pad=-1.0)
    with pytest.raises(ops._lib.PixelNerfHipError, match="c1 < c2"):
        ops.occupancy_clip_rays(rays, bits, (4, 4, 4), (-1,) * 3, (1, -1, 1))


# ---------------------------------------------------------------- 2. clip

def _clip(ops, dev, rays, occ, pad):
    bits = torch.from_numpy(R.pack_bits(occ).view(np.int32)).to(dev)
    tb, hit = ops.occupancy_clip_rays(torch.from_numpy(rays).to(dev), bits, tuple(n + 1 for n in occ.shape), R.C1, R.C2, pad)
    assert tb.dtype == torch.float32 and hit.dtype == torch.int32 and tb.shape == (len(rays), 2) and hit.shape == (len(rays),)
    return hit.cpu().numpy(), tb.cpu().numpy()


@pytest.mark.parametrize("pad", [0.0, 0.1])
def test_clip_is_bracketed_by_shrunk_and_grown_cells(ops, dev, pad):
    """One-sided, without exclusions.  With delta = 2^-12 and every cell grown (+) or shrunk (-) by delta * h per side, for every
    ray  hit_ref(-delta) => hit_device => hit_ref(+delta),  and for the rays hit on both sides
        t_enter_dev in [t_enter(+delta) - tau, t_enter(-delta) + tau],  t_exit_dev in [t_exit(-delta) - tau, t_exit(+delta) + tau],
    tau = 8 * 2^-24 * max(1, |t|)  (tests/occ_ref.py check_clip; the reference is a brute-force fp64 slab test against every
    occupied cell, not a traversal).

    Why these constants: delta * h is 6e-5 at h = 0.25.  The device forms a plane as c1 + i h and a parameter as
    (plane - o) / d in separately rounded fp32: the rounding of the plane and of `plane - o` is at most 2^-23 * 4, about 5e-7,
    at coordinates up to 4.  Growing a cell shifts its planes by delta * h, which moves t by delta * h / |d_axis| -- the same
    1 / |d_axis| factor by which those two roundings reach t -- so delta absorbs them with two orders of magnitude to spare,
    whatever the direction.  What is left is relative to t itself: the rounding of the quotient, of +- pad and of the clamp to
    [near, far], 2^-24 |t| each: tau covers them.  A traversal can also skip a cell it crosses for a parameter length of the
    order of those roundings (two planes reached at nearly the same t): such a cell is not hit once shrunk by delta.

    The not-vacuous condition (tests/test_occupancy_host.py) is repeated here, on the device's own input, BEFORE comparing: on
    the 4096 sphere rays at most 1 % are ambiguous (hit(+delta) != hit(-delta)) and both classes hold at least 25 %."""
    cases = R.clip_cases(0)
    name, rays, occ = cases[0]
    assert name == "sphere" and len(rays) == 4096 and 0.05 <= occ.mean() <= 0.15
    ambiguous, share = R.vacuity(rays, occ, pad=pad)
    print(f"sphere rays: {100 * ambiguous:.3f} % ambiguous, {100 * share:.1f} % hit")
    assert ambiguous <= 0.01 and 0.25 <= share <= 0.75
    for name, rays, occ in cases:
        hit, tb = _clip(ops, dev, rays, occ, pad)
        R.check_clip(rays, occ, pad, hit, tb, what=f"{name} pad {pad}")
        if name == "full_grid":
            assert hit[:512].mean() > 0.5
        if name in ("empty_grid", "missing"):
            assert not hit.any()
        if name == "inside":
            near_hits = (tb[:64, 0] == rays[:64, 6]) & (hit[:64] == 1)
            assert near_hits.all()                                           # origins inside occupied cells: t_enter = near


def test_clip_keeps_what_it_cannot_classify(ops, dev):
    rays = R.unclassifiable_rays()
    for occ in (R.random_cells(0), np.zeros((8, 8, 8), bool)):
        hit, tb = _clip(ops, dev, rays, occ, 0.1)
        assert hit[:-1].tolist() == [1] * (len(rays) - 1)                    # NaN / inf components, zero direction, near >= far
        assert hit[-1] == 0                                                  # the control: a finite ray far from the box
        assert tb.tobytes() == rays[:, 6:8].tobytes()                        # bounds unchanged, bit for bit (NaN included)


def test_grid_object_clips_any_leading_shape(ops, dev):
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    occ_cells = R.random_cells(0)
    field = np.zeros((9, 9, 9), np.float32)
    grid = OccupancyGrid.from_density(torch.from_numpy(field).to(dev), R.C1, R.C2, 0.5, dilate=0)
    assert grid.occupied_fraction == 0.0 and grid.n_cells == 512
    grid = OccupancyGrid(torch.from_numpy(R.pack_bits(occ_cells).view(np.int32)).to(dev), R.RESO, R.C1, R.C2, 0.5, 0,
                         torch.tensor(int(occ_cells.sum()), dtype=torch.int32, device=dev))
    assert abs(grid.occupied_fraction - occ_cells.mean()) < 1e-12
    rays = torch.from_numpy(R.sphere_rays(0, n=96)).to(dev)
    tb, hit = grid.clip_rays(rays)
    tb3, hit3 = grid.clip_rays(rays.reshape(2, 3, 16, 8))
    assert tb3.shape == (2, 3, 16, 2) and hit3.shape == (2, 3, 16)
    assert torch.equal(tb3.reshape(-1, 2), tb) and torch.equal(hit3.reshape(-1), hit)
    tb1, hit1 = grid.clip_rays(rays[5])
    assert tb1.shape == (2,) and hit1.shape == () and torch.equal(tb1, tb[5]) and int(hit1) == int(hit[5])


# ---------------------------------------------------------------- 3. philox_noise_ids

@pytest.mark.parametrize("counts", [(8, 8, 3), (8, 0, 0), (0, 5, 0), (4, 3, 3)], ids=lambda c: "Kc%d_Kf%d_Kfd%d" % c)
def test_philox_noise_ids_equals_philox_noise(ops, dev, counts):
    """(8, 8, 3): Kc = 8, Kimp = 5, Kfd = 3; the others: a count of 0 in every position"""
    Kc, Kf, Kfd = counts
    seed, R_ = 0x1234_5678_9ABC_DEF0, 300
    whole = ops.philox_noise(R_, Kc, Kf, Kfd, seed, dev)
    same = lambda a, b: a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)  # noqa: E731
    ids = torch.arange(R_, dtype=torch.int64, device=dev)
    assert same(ops.philox_noise_ids(ids, Kc, Kf, Kfd, seed), whole)                         # a contiguous range
    perm = torch.from_numpy(np.random.RandomState(3).permutation(R_)).to(dev)
    rep = torch.tensor([7, 7, 299, 0, 7, 123, 0], dtype=torch.int64, device=dev)
    for pick in (perm, rep):
        got = ops.philox_noise_ids(pick, Kc, Kf, Kfd, seed)
        assert all(torch.equal(got[k], whole[k][pick]) for k in whole) and got.keys() == whole.keys()
    for base in (2 ** 31 - 2, 2 ** 32 - 1, 2 ** 40 + 5):                                     # ids above 2^31 and 2^32
        far = ops.philox_noise(6, Kc, Kf, Kfd, seed, dev, ray_id_offset=base)
        got = ops.philox_noise_ids(base + torch.tensor([3, 0, 5, 5, 1], dtype=torch.int64, device=dev), Kc, Kf, Kfd, seed)
        assert all(torch.equal(got[k], far[k][[3, 0, 5, 5, 1]]) for k in far) and got.keys() == far.keys()
    if Kc > 0:
        assert not torch.equal(ops.philox_noise_ids(ids, Kc, Kf, Kfd, seed + 1)["u1"], whole["u1"])
    empty = ops.philox_noise_ids(ids[:0], Kc, Kf, Kfd, seed)
    assert all(v.shape[0] == 0 for v in empty.values())


# ---------------------------------------------------------------- 4. end to end

W = H = 16
FOCAL, C, Z_NEAR, Z_FAR = 30.0, (8.0, 8.0), 1.2, 4.0
GRID_C1, GRID_C2, GRID_N = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 17


def _ball_grid(dev, radius=0.5, dilate=1):
    """the synthetic field: 1 inside the ball of `radius` around the origin, 0 outside, on 17^3 points over [-1,1]^3"""
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    g = np.linspace(-1.0, 1.0, GRID_N)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    field = (np.sqrt(x * x + y * y + z * z) < radius).astype(np.float32)
    return OccupancyGrid.from_density(torch.from_numpy(field).to(dev), GRID_C1, GRID_C2, 0.5, dilate=dilate)


def _const_grid(dev, value):
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    return OccupancyGrid.from_density(torch.full((GRID_N,) * 3, float(value), device=dev), GRID_C1, GRID_C2, 0.5, dilate=0)


def _poses(dev):
    p = torch.stack([torch.as_tensor(synthetic.pose_spherical(t, -20.0 - 5.0 * i, 2.732)) for i, t in enumerate((40.0, 200.0))])
    return p.reshape(1, 2, 4, 4).float().to(dev)


def _setup(dev, golden="sn64_64_128", precision=None, use_fine=True, **rend_kw):
    """the smallest one-object golden scene (sn64) with the sample counts of `golden`"""
    from pixelnerf_amd.render import NeRFRenderer
    from test_api_gpu import build_net
    g = golden_setup(golden)[0]
    scene, _ = scene_for(str(g["scene"]), int(g["scene_seed"]))
    assert scene["SB"] == 1
    net = build_net(dev, scene, use_fine=use_fine, precision=precision)
    kw = dict(n_coarse=int(g["n_coarse"]), n_fine=int(g["n_fine"]), n_fine_depth=int(g["n_fine_depth"]),
              depth_std=float(g["depth_std"]), white_bkgd=True)
    kw.update(rend_kw)
    return net, NeRFRenderer(**kw).to(dev).eval()


def _views(rend, net, poses, seed, **kw):
    torch.manual_seed(seed)
    return rend.render_views(net, poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C, **kw)


def _assert_kept_pixels_are_dense_and_culled_are_background(out, dense, rend, what):
    hit = out.hit
    assert hit.dtype == torch.bool and hit.shape == dense.depth.shape and out.n_hit == int(hit.sum())
    assert 0 < out.n_hit < hit.numel(), f"{what}: the fixture must have hit and missed pixels ({out.n_hit} of {hit.numel()})"
    assert torch.equal(out.rgb[hit], dense.rgb[hit]), f"{what}: rgb differs at a kept pixel"
    assert torch.equal(out.depth[hit], dense.depth[hit]), f"{what}: depth differs at a kept pixel"
    bg = 1.0 if rend.white_bkgd else 0.0
    assert (out.rgb[~hit] == bg).all() and (out.depth[~hit] == 0).all(), f"{what}: a culled pixel is not the background"


@pytest.fixture(scope="module")
def main_case(dev):
    net, rend = _setup(dev)
    poses = _poses(dev)
    return net, rend, poses, _ball_grid(dev), _views(rend, net, poses, 21)


def test_culled_render_views_equals_the_dense_render_at_every_kept_pixel(ops, dev, main_case):
    """(a) bit-equal at the hit pixels, (b) the background elsewhere, (c) hit = ops.occupancy_clip_rays on util.gen_rays of the
    cameras, (f) views_per_call=1 gives the bits of the single call; the epilogue runs on the full image"""
    from pixelnerf_amd import util
    net, rend, poses, occ, dense = main_case
    assert "hit" not in dense and "n_hit" not in dense
    out = _views(rend, net, poses, 21, occupancy=occ)
    _assert_kept_pixels_are_dense_and_culled_are_background(out, dense, rend, "one call")
    print(f"ball grid: {out.n_hit} of {out.hit.numel()} pixels rendered, {100 * occ.occupied_fraction:.1f} % of the cells occupied")
    rays = util.gen_rays(poses.reshape(-1, 4, 4), W, H, FOCAL, Z_NEAR, Z_FAR, C).reshape(-1, 8)
    _, hit = ops.occupancy_clip_rays(rays, occ.bits, occ.reso, occ.c1, occ.c2)
    assert torch.equal(out.hit.reshape(-1), hit != 0)                                         # (c)
    assert torch.equal(out.depth_norm, ops.eval_epilogue(out.rgb.reshape(2, -1, 3), out.depth.reshape(2, -1), Z_NEAR, Z_FAR)
                       ["depth_norm"].reshape(out.depth.shape))
    one = _views(rend, net, poses, 21, occupancy=occ, views_per_call=1)                       # (f)
    assert torch.equal(one.rgb, out.rgb) and torch.equal(one.depth, out.depth) and torch.equal(one.hit, out.hit)
    assert one.n_hit == out.n_hit
    gt = dense.rgb.clamp(0, 1)
    with_gt = _views(rend, net, poses, 21, occupancy=occ, gt_rgb=gt, want_u8=True)
    assert torch.equal(with_gt.rgb, out.rgb) and with_gt.psnr.shape == (1, 2) and with_gt.rgb_u8.shape == out.rgb.shape
    # the generator advances as for the dense call
    gen = torch.cuda.default_generators[dev.index]
    _views(rend, net, poses, 21)
    want = gen.get_offset()
    _views(rend, net, poses, 21, occupancy=occ)
    assert gen.get_offset() == want
    par = rend.bind_parallel(net, None, simple_output=True).eval()                            # the bound wrapper passes it on
    torch.manual_seed(21)
    got = par.render_views(poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C, occupancy=occ)
    assert torch.equal(got.rgb, out.rgb) and torch.equal(got.hit, out.hit)


@pytest.mark.parametrize("white", [False, True])
def test_culled_forward_fills_coarse_and_fine_with_the_background(ops, dev, main_case, white):
    """(b) every missed ray is exactly the empty-ray value in the coarse and the fine outputs of forward, weights included;
    (h) with a non-zero ray_id_offset the hit rays match the dense forward"""
    from pixelnerf_amd import util
    net, rend0, poses, occ, _ = main_case
    _, rend = _setup(dev, white_bkgd=white)
    rays = util.gen_rays(poses.reshape(-1, 4, 4), W, H, FOCAL, Z_NEAR, Z_FAR, C).reshape(1, -1, 8)
    hit = (ops.occupancy_clip_rays(rays.reshape(-1, 8), occ.bits, occ.reso, occ.c1, occ.c2)[1] != 0)
    assert 0 < int(hit.sum()) < hit.numel()
    for offset in (0, 12345):
        rend.ray_id_offset = offset
        with torch.no_grad():
            torch.manual_seed(5)
            dense = rend(net, rays, want_weights=True)
            torch.manual_seed(5)
            out = rend(net, rays, want_weights=True, occupancy=occ)
        for p, K in (("coarse", rend.n_coarse), ("fine", rend.n_coarse + rend.n_fine)):
            o, d = out[p], dense[p]
            assert o.rgb.shape == d.rgb.shape and o.depth.shape == d.depth.shape and o.weights.shape == (1, hit.numel(), K)
            for key in ("rgb", "depth", "weights"):
                assert torch.equal(o[key][0][hit], d[key][0][hit]), (p, key, offset)
            assert (o.rgb[0][~hit] == (1.0 if white else 0.0)).all() and (o.depth[0][~hit] == 0).all()
            assert (o.weights[0][~hit] == 0).all()
    rend.ray_id_offset = 0
    with torch.no_grad():
        torch.manual_seed(5)
        other = rend(net, rays, occupancy=occ)
    assert not torch.equal(other.fine.rgb[0][hit], out.fine.rgb[0][hit])                      # the offset does select other draws
    # explicit noise is cut to the hit rows
    noise = {k: v.to(dev) for k, v in synthetic.make_noise(hit.numel(), rend.n_coarse, rend.n_fine, rend.n_fine_depth, seed=3).items()}
    with torch.no_grad():
        dense = rend(net, rays, _noise=noise)
        out = rend(net, rays, _noise=noise, occupancy=occ)
    assert torch.equal(out.fine.rgb[0][hit], dense.fine.rgb[0][hit]) and torch.equal(out.coarse.depth[0][hit], dense.coarse.depth[0][hit])


def test_full_grid_is_the_dense_image_and_empty_grid_launches_nothing(ops, dev, main_case):
    """(d) a full grid reproduces the dense image bit for bit; (e) an empty grid returns pure background and the profile hook
    counts zero network launches for it"""
    net, rend, poses, occ, dense = main_case
    full = _views(rend, net, poses, 21, occupancy=_const_grid(dev, 1.0))
    assert full.n_hit == full.hit.numel() and full.hit.all()
    assert torch.equal(full.rgb, dense.rgb) and torch.equal(full.depth, dense.depth) and torch.equal(full.depth_norm, dense.depth_norm)
    empty_grid = _const_grid(dev, 0.0)
    assert empty_grid.occupied_fraction == 0.0
    ops.profile_enable(True)
    try:
        empty = _views(rend, net, poses, 21, occupancy=empty_grid)
        torch.cuda.synchronize()
        assert ops.profile_read()[1] == 0
        _views(rend, net, poses, 21, occupancy=occ)
        torch.cuda.synchronize()
        assert ops.profile_read()[1] > 0                                                      # the hook does count launches
    finally:
        ops.profile_enable(False)
    assert empty.n_hit == 0 and not empty.hit.any()
    assert (empty.rgb == 1.0).all() and (empty.depth == 0).all()


def test_tighten_samples_between_the_first_and_last_occupied_cell(ops, dev, main_case):
    """(g) tighten=True equals forward on the same gathered rays with columns 6 and 7 replaced by hand and the draws of
    philox_noise_ids for their global ids"""
    from pixelnerf_amd import util
    net, rend, poses, occ, dense = main_case
    out = _views(rend, net, poses, 33, occupancy=occ, tighten=True)
    rays = util.gen_rays(poses.reshape(-1, 4, 4), W, H, FOCAL, Z_NEAR, Z_FAR, C).reshape(-1, 8)
    tb, hit = ops.occupancy_clip_rays(rays, occ.bits, occ.reso, occ.c1, occ.c2)
    idx = torch.nonzero(hit).flatten()
    sub = rays[idx].clone()
    sub[:, 6:8] = tb[idx]
    assert (sub[:, 6] > Z_NEAR).all() and (sub[:, 7] < Z_FAR).all() and (sub[:, 6] < sub[:, 7]).all()
    torch.manual_seed(33)
    seed = rend._next_seed(dev)
    noise = ops.philox_noise_ids(idx, rend.n_coarse, rend.n_fine, rend.n_fine_depth, seed)
    with torch.no_grad():
        ref = rend(net, sub[None], _noise=noise)
    assert torch.equal(out.rgb.reshape(-1, 3)[idx], ref.fine.rgb[0]) and torch.equal(out.depth.reshape(-1)[idx], ref.fine.depth[0])
    assert torch.equal(out.hit.reshape(-1), hit != 0)
    assert (out.rgb.reshape(-1, 3)[hit == 0] == 1.0).all()
    plain = _views(rend, net, poses, 33, occupancy=occ)
    assert not torch.equal(plain.rgb[out.hit], out.rgb[out.hit])                              # denser samples: another image


def test_culling_refuses_two_objects_and_gradients(ops, dev, main_case):
    """(i)"""
    from pixelnerf_amd import util
    net, rend, poses, occ, _ = main_case
    rays = util.gen_rays(poses.reshape(-1, 4, 4), W, H, FOCAL, Z_NEAR, Z_FAR, C).reshape(1, -1, 8)
    with torch.no_grad(), pytest.raises(ValueError, match="ONE object"):
        rend(net, rays.reshape(2, -1, 8), occupancy=occ)
    saved = net.num_objs
    try:
        net.num_objs = 2
        with pytest.raises(ValueError, match="ONE object"):
            _views(rend, net, poses, 1, occupancy=occ)
    finally:
        net.num_objs = saved
    need = rays.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference"):
        rend(net, need, occupancy=occ)
    p = next(net.mlp_coarse.parameters())
    was = p.requires_grad
    try:
        p.requires_grad_(True)
        with pytest.raises(NotImplementedError, match="inference"):
            rend(net, rays, occupancy=occ)
        with torch.no_grad():
            rend(net, rays, occupancy=occ)                                                    # under no_grad it is inference
    finally:
        p.requires_grad_(was)


@pytest.mark.parametrize("variant", ["no_fine_network", "f32"])
def test_merge_path_and_exact_fp32_keep_the_identity(ops, dev, variant):
    """(j) mlp_fine is None (the fine pass merges the coarse pass's outputs; the sample counts of the sn64_coarse_only_mlp golden)
    and precision "f32" each pass (a)"""
    if variant == "no_fine_network":
        net, rend = _setup(dev, golden="sn64_coarse_only_mlp", use_fine=False)
        assert net.mlp_fine is None
    else:
        net, rend = _setup(dev, golden="sn64_coarse_only_mlp", precision="f32")
    poses, occ = _poses(dev), _ball_grid(dev)
    dense = _views(rend, net, poses, 9)
    for k in (None, 1):
        out = _views(rend, net, poses, 9, occupancy=occ, views_per_call=k)
        _assert_kept_pixels_are_dense_and_culled_are_background(out, dense, rend, f"{variant} views_per_call={k}")


def test_torch_draws_and_generic_callables_render_the_hit_rays_only(ops, dev, main_case):
    """no bit-equality is promised here (the draws are made for the rendered rays only): shapes, the background, finite values"""
    net, _, poses, occ, _ = main_case

    class Plain(torch.nn.Module):
        use_viewdirs = True

        def forward(self, xyz, coarse=True, viewdirs=None):
            return net(xyz, coarse=coarse, viewdirs=viewdirs)

    _, rend_t = _setup(dev, rng="torch")
    for model, rend in ((net, rend_t), (Plain(), _setup(dev)[1])):
        out = _views(rend, model, poses, 4, occupancy=occ)
        assert 0 < out.n_hit < out.hit.numel() and torch.isfinite(out.rgb).all()
        assert (out.rgb[~out.hit] == 1.0).all() and (out.depth[~out.hit] == 0).all() and (out.depth[out.hit] > 0).all()


# ---------------------------------------------------------------- 5. from_model

def test_from_model_is_the_maximum_of_both_networks_and_recon_is_unchanged(ops, dev, main_case):
    from pixelnerf_amd.util import recon
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    net = main_case[0]
    reso, c1, c2 = [9, 9, 9], [-1, -1, -1], [1, 1, 1]
    xyz, vd = ops.gen_grid_points(c1, c2, reso, device=dev)
    with torch.no_grad():
        sc = net(xyz[None], coarse=True, viewdirs=vd[None])[0, :, 3]
        sf = net(xyz[None], coarse=False, viewdirs=vd[None])[0, :, 3]
    assert not torch.equal(sc, sf)
    field = torch.maximum(sc, sf).view(*reso)
    thr = float(field.median())
    net.train()
    with pytest.warns(UserWarning, match="fake view dirs"):
        occ = OccupancyGrid.from_model(net, c1, c2, reso, thr, dilate=0, eval_batch_size=200)
    assert net.training
    net.eval()
    bits, count = ops.occupancy_build(field, thr, 0)
    assert torch.equal(occ.bits, bits) and int(occ.n_occupied) == int(count) and 0.0 < occ.occupied_fraction <= 1.0
    assert occ.reso == (9, 9, 9) and occ.threshold == thr and occ.dilate == 0
    only_coarse, _ = ops.occupancy_build(sc.view(*reso), thr, 0)
    saved = net.mlp_fine
    try:
        net.mlp_fine = None                                                  # the coarse network's alone
        with pytest.warns(UserWarning):
            assert torch.equal(OccupancyGrid.from_model(net, c1, c2, reso, thr, dilate=0).bits, only_coarse)
    finally:
        net.mlp_fine = saved
    # recon.marching_cubes after the refactor: the mesh of the coarse field in the reference's scaling
    iso = float(sc.median())
    with pytest.warns(UserWarning, match="fake view dirs"):
        v, t = recon.marching_cubes(net, c1, c2, reso, isosurface=iso, as_tensors=True)
        vf, tf = recon.marching_cubes(net, c1, c2, reso, isosurface=iso, as_tensors=True, coarse=False, eval_batch_size=100)
    rv, rt = ops.marching_cubes(sc.view(*reso), iso, c1=np.array(c1, np.float64), scale=2.0 / np.array(reso))
    assert len(v) > 0 and torch.equal(v, rv) and torch.equal(t, rt)
    fv, ft = ops.marching_cubes(sf.view(*reso), iso, c1=np.array(c1, np.float64), scale=2.0 / np.array(reso))
    assert torch.equal(vf, fv) and torch.equal(tf, ft)
