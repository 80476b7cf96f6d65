"""GPU tests (-m gpu) of the per-sample skipping: pnr_occupancy_mark_samples / pnr_compact_samples / pnr_expand_rgbsigma through
ops.occupancy_mark_samples / ops.compact_samples / ops.expand_rgbsigma, OccupancyGrid.mark_samples, and the `skip_empty=` keyword of
NeRFRenderer.forward / render_views.

Mark: equal to the numpy restatement (tests/skip_ref.py) on every sample that is not within 1e-4 cell of a cell plane.
Compaction, expansion: exact.  Rendering: identities without a tolerance -- skip_empty is the dense render of the kept rays with
rgb sigma = 0 at the samples the grid calls empty (A), and with a grid that calls nothing empty it is the dense render (B)."""
import ctypes

import numpy as np
import pytest
import torch

import occ_ref
import skip_ref as S
from helpers import golden_setup, mlp_params
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


def _bits(occ, dev):
    return torch.from_numpy(occ_ref.pack_bits(occ).view(np.int32)).to(dev)


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.contiguous().cpu().numpy().tobytes() == b.contiguous().cpu().numpy().tobytes()


# ---------------------------------------------------------------- 1. mark

def _mark_cases():
    cases = [(f"sphere{seed}",) + S.sphere_case(seed) + (S.C1, S.C2) for seed in (0, 1, 2)]
    cases.append(("random_5x6x7",) + S.random_grid_case(0))
    return cases


@pytest.mark.parametrize("case", _mark_cases(), ids=lambda c: c[0])
def test_mark_equals_the_restatement(ops, dev, case):
    """Every operation of the definition is an individually rounded fp32 operation, so the expected number of mismatches is zero;
    samples within 1e-4 cell of a cell plane (at most 0.5 % of them) are only required to be 0 or 1."""
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    name, rays, z, occ, c1, c2 = case
    reso = tuple(n + 1 for n in occ.shape)
    bits = _bits(occ, dev)
    keep = ops.occupancy_mark_samples(torch.from_numpy(rays).to(dev), torch.from_numpy(z).to(dev), bits, reso, c1, c2)
    assert keep.dtype == torch.uint8 and keep.shape == z.shape and keep.is_cuda
    got = keep.cpu().numpy()
    ref = S.mark_ref(rays, z, occ, c1, c2)
    amb = S.ambiguous(rays, z, occ.shape, c1, c2)
    print(f"mark {name}: kept {got.mean():.4f} (restatement {ref.mean():.4f}), ambiguous {100 * amb.mean():.3f} %, mismatches "
          f"{int((got != ref).sum())} of {got.size}, on unambiguous samples {int(((got != ref) & ~amb).sum())}")
    assert amb.mean() <= 0.005
    assert ((got == 0) | (got == 1)).all()
    assert np.array_equal(got[~amb], ref[~amb])
    if name.startswith("sphere"):
        assert 0.15 <= ref.mean() <= 0.30                                    # (the host test's not-vacuous condition, on this input)
    grid = OccupancyGrid(bits, reso, c1, c2, 0.5, 0, torch.tensor(int(occ.sum()), dtype=torch.int32, device=dev))
    assert torch.equal(grid.mark_samples(torch.from_numpy(rays).to(dev), torch.from_numpy(z).to(dev)), keep)


def test_mark_hand_made_samples(ops, dev):
    """K = 1; an origin inside the box, a zero direction, NaN / inf components (kept), samples before and beyond the box (empty),
    points exactly on the c1 and the c2 faces (the first / the last cell): all exactly representable, so no sample is excluded"""
    rays, z, occ, want = S.hand_case()
    keep = ops.occupancy_mark_samples(torch.from_numpy(rays).to(dev), torch.from_numpy(z).to(dev), _bits(occ, dev), (9, 9, 9), S.C1, S.C2)
    assert keep.shape == (len(rays), 1)
    assert keep.cpu().numpy().reshape(-1).tolist() == want.tolist() == S.mark_ref(rays, z, occ, S.C1, S.C2).reshape(-1).tolist()
    empty = ops.occupancy_mark_samples(torch.zeros((0, 8), device=dev), torch.zeros((0, 3), device=dev), _bits(occ, dev), (9, 9, 9), S.C1, S.C2)
    assert empty.shape == (0, 3)


# ---------------------------------------------------------------- 2. compaction

@pytest.mark.parametrize("shape", S.COMPACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_compaction_is_stable_exact_and_writes_nothing_beyond_the_count(ops, dev, shape):
    """(1,63..65): the wave boundary; (1024,67): an odd K and 268 workgroups, more than one round of the scan covers"""
    R, K = shape
    N = R * K
    lib = ops._lib.load()
    rs = np.random.RandomState(R + K)
    rays = torch.from_numpy(rs.standard_normal((R, 8)).astype(np.float32)).to(dev)
    z = torch.from_numpy(rs.standard_normal((R, K)).astype(np.float32)).to(dev)
    for name, mask in S.keep_patterns(R, K):
        keep = torch.from_numpy(mask).to(dev)
        want = torch.nonzero(keep.reshape(-1)).flatten()
        index, rays_c, z_c, M = ops.compact_samples(keep, rays, z)
        assert isinstance(M, int) and M == want.numel() == int((mask != 0).sum()), name
        assert index.dtype == torch.int32 and index.shape == (M,) and rays_c.shape == (M, 8) and z_c.shape == (M,)
        assert torch.equal(index.long(), want), name                                             # ascending kept ids
        assert _same_bytes(rays_c, rays[want // K]) and _same_bytes(z_c, z.reshape(-1)[want]), name
        # the raw entry on oversized NaN-prefilled buffers: rows >= M stay untouched; a second call gives the same bytes
        pad = 5
        outs = []
        for _ in range(2):
            idx = torch.full((N + pad,), -7, dtype=torch.int32, device=dev)
            rc = torch.full((N + pad, 8), float("nan"), device=dev)
            zc = torch.full((N + pad,), float("nan"), device=dev)
            count = torch.full((), -1, dtype=torch.int32, device=dev)
            nbytes = lib.pnr_compact_samples_workspace_bytes(N)
            assert nbytes == 4 * ((N + 255) // 256)
            ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
            rc_ = lib.pnr_compact_samples(keep.data_ptr(), rays.data_ptr(), z.data_ptr(), R, K, idx.data_ptr(), rc.data_ptr(), zc.data_ptr(),
                                          count.data_ptr(), ws.data_ptr(), nbytes, None)
            assert rc_ == 0, lib.pnr_last_error()
            torch.cuda.synchronize()
            assert int(count) == M, name
            assert (idx[M:] == -7).all() and torch.isnan(rc[M:]).all() and torch.isnan(zc[M:]).all(), name
            outs.append((idx, rc, zc))
        assert torch.equal(outs[0][0][:M], index) and _same_bytes(outs[0][1][:M], rays_c) and _same_bytes(outs[0][2][:M], z_c), name
        assert all(_same_bytes(a, b) for a, b in zip(outs[0], outs[1])), name


# ---------------------------------------------------------------- 3. expand

def test_expand_writes_every_row(ops, dev):
    lib = ops._lib.load()
    N = 1024 * 67
    rs = np.random.RandomState(3)
    for frac in (0.2, 1.0, 0.0):
        index = torch.from_numpy(np.flatnonzero(rs.uniform(size=N) < frac).astype(np.int32)).to(dev)
        M = index.numel()
        part = torch.from_numpy(rs.standard_normal((M, 4)).astype(np.float32)).to(dev)
        out = torch.full((N, 4), float("nan"), device=dev)
        assert lib.pnr_expand_rgbsigma(index.data_ptr() if M else None, part.data_ptr() if M else None, M, N, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
        assert _same_bytes(out[index.long()], part)
        rest = torch.ones(N, dtype=torch.bool, device=dev)
        rest[index.long()] = False
        assert (out[rest] == 0).all() and int(rest.sum()) == N - M
        assert _same_bytes(ops.expand_rgbsigma(index, part if M else None, N), out)
        assert _same_bytes(out.cpu(), torch.from_numpy(S.expand_ref(index.cpu().numpy(), part.cpu().numpy(), N)))
    assert ops.expand_rgbsigma(index[:0], None, 0).shape == (0, 4)


# ---------------------------------------------------------------- 4.-6. rendering

KC, KF, KFD = 64, 32, 16
# The cases that are about the renderer's plumbing (tighten, the public path, a pass that keeps nothing) run at the default
# precision, the one with the pair rule (odd sample counts in the last of them: pairs then straddle rays)
PLUMBING_PRECISION = None
SCENES = {"sn64": ("adv_surface_sn64", 17, 0.5), "dtu_mini": ("adv_surface_dtu", 33, 0.5)}   # golden, ball grid points, ball radius


def _ball_grid(dev, n_points, radius):
    """cells of the n^3-point grid over [-1,1]^3 with a corner within `radius` of the origin (no dilation: S.ball_cells)"""
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    g = np.linspace(-1.0, 1.0, n_points)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    field = (np.sqrt(x * x + y * y + z * z) <= radius).astype(np.float32)
    grid = OccupancyGrid.from_density(torch.from_numpy(field).to(dev), S.C1, S.C2, 0.5, dilate=0)
    assert int(grid.n_occupied) == int(S.ball_cells(n_points, radius).sum())
    return grid


@pytest.fixture(scope="module")
def setup(dev):
    """-> f(scene, precision=None, use_fine=True) = (net with the surface-variant networks, renderer, 256 rays (256,8), noise, ball grid),
    built once per configuration"""
    from pixelnerf_amd.render import NeRFRenderer
    from test_api_gpu import build_net
    cache = {}

    def make(scene_name, precision=None, use_fine=True):
        key = (scene_name, precision, use_fine)
        if key not in cache:
            golden, n_points, radius = SCENES[scene_name]
            g, scene, meta, mc, mf, _, _ = golden_setup(golden)
            assert scene["SB"] == 1
            net = build_net(dev, scene, use_fine=use_fine, precision=precision)
            net.mlp_coarse.load_state_dict(mc)
            if use_fine:
                gain, tau = float(g["sigma_gain"]), float(g["sigma_tau"])
                net.mlp_fine.load_state_dict(mf if mf is not None else synthetic.surface_variant(mlp_params(12), gain, tau))
            for p in net.parameters():
                p.requires_grad_(False)
            rend = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).to(dev).eval()
            rays = synthetic.target_rays(meta, n_rays=256)[0].to(dev)
            noise = {k: v.to(dev) for k, v in synthetic.make_noise(256, KC, KF, KFD, seed=77).items()}
            cache[key] = (net, rend, rays, noise, _ball_grid(dev, n_points, radius))
        return cache[key]
    return make


def _staged_reference(ops, net, rend, rays, noise, occ):
    """the defining property, from the EXISTING staged ops on the same rays and noise: sample_coarse, a DENSE eval_ray_samples,
    rgb sigma := 0 where the grid calls the sample empty, composite, sample_fine, and the same again with the fine network
    -> ({pass: {rgb, depth, weights}}, {pass: (kept, total)})"""
    scene = net.scene()
    Kf = rend.n_fine if rend.using_fine else 0

    def network(coarse, z):
        pk = net.packed(coarse)
        rs = ops.eval_ray_samples(scene, pk, rays, z, net.tables(coarse))
        keep = occ.mark_samples(rays, z)
        return torch.where(keep.unsqueeze(-1) != 0, rs, torch.zeros_like(rs)), (int(keep.sum()), keep.numel())

    with torch.no_grad():
        z_c = ops.sample_coarse(rays, noise["u1"], rend.lindisp)
        rs_c, kept_c = network(True, z_c)
        w_c, rgb_c, d_c = ops.composite(rays, z_c, rs_c, rend.white_bkgd, True)
        out, stats = {"coarse": dict(rgb=rgb_c, depth=d_c, weights=w_c)}, {"coarse": kept_c, "fine": (0, 0)}
        if Kf > 0:
            z_f = ops.sample_fine(rays, w_c, d_c, z_c, noise.get("u2"), noise.get("u3"), noise.get("n4"), rend.depth_std, rend.lindisp)
            rs_f, kept_f = network(False, z_f)
            w_f, rgb_f, d_f = ops.composite(rays, z_f, rs_f, rend.white_bkgd, True)
            out["fine"], stats["fine"] = dict(rgb=rgb_f, depth=d_f, weights=w_f), kept_f
    return out, stats


def _assert_identity_a(ops, net, rend, rays, noise, occ, out, tighten=False, what=""):
    """out = rend(net, rays[None], want_weights=True, occupancy=occ, skip_empty=True[, tighten]) under `noise` (rows of ALL rays):
    the rays the grid keeps are bit-equal to the staged reference, the others are the background; -> last_skip_stats"""
    tb, hit = occ.clip_rays(rays)
    idx = torch.nonzero(hit).flatten()
    sub = rays[idx].clone()
    if tighten:
        sub[:, 6:8] = tb[idx]
    ref, stats = _staged_reference(ops, net, rend, sub, {k: v[idx] for k, v in noise.items()}, occ)
    miss = hit == 0
    assert 0 < idx.numel(), what
    for p in ref:                                                            # (every figure is printed before anything is asserted)
        for key in ("rgb", "depth", "weights"):
            got, want = out[p][key][0][idx], ref[p][key]
            differ = (got != want).reshape(len(idx), -1).any(dim=1)
            print(f"{what}: {p} {key}: {int(differ.sum())} of {len(idx)} rays differ from the staged reference, max abs "
                  f"{float((got - want).abs().max()):.3e}")
    for p in ref:
        for key in ("rgb", "depth", "weights"):
            got = out[p][key][0]
            assert _same_bytes(got[idx], ref[p][key]), f"{what}: {p} {key} differs from the staged reference"
        assert (out[p].rgb[0][miss] == 1.0).all() and (out[p].depth[0][miss] == 0).all() and (out[p].weights[0][miss] == 0).all(), what
    got_stats = rend.last_skip_stats
    print(f"{what}: {idx.numel()} of {len(rays)} rays rendered, kept samples coarse {got_stats['coarse']}, fine {got_stats['fine']}")
    assert got_stats == stats, what
    assert all(type(v) is int for pair in got_stats.values() for v in pair)
    return got_stats


def _share(pair):
    return pair[0] / max(pair[1], 1)


@pytest.mark.parametrize("scene_name,precision,use_fine", [("sn64", None, True), ("sn64", "f16", True), ("dtu_mini", None, True),
                                                           ("dtu_mini", "f16", True), ("sn64", "f32", True), ("sn64", "f16", False)],
                         ids=["sn64-default", "sn64-f16", "dtu3view-default", "dtu3view-f16", "sn64-f32", "sn64-f16-no_fine_network"])
def test_skip_empty_is_the_dense_render_with_sigma_zero_in_empty_cells(ops, dev, setup, scene_name, precision, use_fine):
    """Identity A on a one-view and a three-view scene, 256 rays, 64 + 32 (16 depth) samples, an analytic ball as the grid (the
    identity holds for any grid, so the network does not decide whether the test bites): rgb, depth and weights of both passes are
    bit-equal to the staged reference.  The ball keeps 5-60 % of the samples in both passes.

    The default precision ("f16x3") is the case that bites: eval_split_kernel's last places depend on the parity of a point's
    place in the launch (profiles/occupancy_notes.md), so a plainly compacted list gives other bits (sn64: 38 of 155 rays differ
    in the coarse rgb, max abs 3.2e-6); the renderer keeps whole pairs of the dense launch in the list there."""
    net, rend, rays, noise, occ = setup(scene_name, precision, use_fine)
    assert (net.mlp_fine is not None) == use_fine
    with torch.no_grad():
        out = rend(net, rays[None], want_weights=True, _noise=noise, occupancy=occ, skip_empty=True)
    stats = _assert_identity_a(ops, net, rend, rays, noise, occ, out, what=f"{scene_name} {precision} fine={use_fine}")
    assert 0.05 <= _share(stats["coarse"]) <= 0.60 and 0.05 <= _share(stats["fine"]) <= 0.60
    assert stats["fine"][1] == stats["coarse"][1] // KC * (KC + KF)
    # without the keyword nothing changes: the ray-culled call, which evaluates every sample of a kept ray, differs from it
    with torch.no_grad():
        culled = rend(net, rays[None], want_weights=True, _noise=noise, occupancy=occ)
    assert not torch.equal(culled.coarse.weights, out.coarse.weights)


def test_skip_empty_with_tighten_and_through_the_public_path(ops, dev, setup):
    """tighten=True composes (the staged reference on the tightened rays); and once through everything public: a grid from
    OccupancyGrid.from_model, seeded draws (no explicit noise), the bound wrapper, forward and render_views"""
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    net, rend, rays, noise, occ = setup("sn64", PLUMBING_PRECISION)
    with torch.no_grad():
        out = rend(net, rays[None], want_weights=True, _noise=noise, occupancy=occ, skip_empty=True, tighten=True)
    _assert_identity_a(ops, net, rend, rays, noise, occ, out, tighten=True, what="tighten")
    with pytest.warns(UserWarning, match="fake view dirs"):
        model_grid = OccupancyGrid.from_model(net, S.C1, S.C2, [17, 17, 17], 1.0, dilate=0)
    assert 0.0 < model_grid.occupied_fraction < 1.0
    torch.manual_seed(31)
    with torch.no_grad():
        out = rend(net, rays[None], want_weights=True, occupancy=model_grid, skip_empty=True)
    torch.manual_seed(31)
    seed = rend._next_seed(dev)
    drawn = ops.philox_noise_ids(torch.arange(len(rays), dtype=torch.int64, device=dev), KC, KF, KFD, seed)
    stats = _assert_identity_a(ops, net, rend, rays, drawn, model_grid, out, what="from_model, seeded")
    assert 0 < stats["coarse"][0] < stats["coarse"][1]
    par = rend.bind_parallel(net, None, simple_output=True).eval()
    torch.manual_seed(31)
    with torch.no_grad():
        rgb, depth = par(rays[None], occupancy=model_grid, skip_empty=True)
    assert _same_bytes(rgb, out.fine.rgb) and _same_bytes(depth, out.fine.depth)


W = H = 16
FOCAL, C, Z_NEAR, Z_FAR = 30.0, (8.0, 8.0), 1.2, 4.0


def _poses(dev):
    p = torch.stack([torch.as_tensor(synthetic.pose_spherical(t, -20.0 - 5.0 * i, 2.732)) for i, t in enumerate((40.0, 200.0))])
    return p.reshape(1, 2, 4, 4).float().to(dev)


def test_a_grid_without_empty_cells_gives_the_dense_render(ops, dev, setup):
    """Identity B: every bit set, a box that encloses every sample of every ray (the cameras are 2.73 from the origin, far = 4)"""
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    net, rend, rays, _, _ = setup("sn64")
    full = OccupancyGrid.from_density(torch.ones((5, 5, 5), device=dev), (-4.0,) * 3, (4.0,) * 3, 0.5, dilate=0)
    assert full.occupied_fraction == 1.0
    outs = []
    for kw in ({}, dict(occupancy=full), dict(occupancy=full, skip_empty=True)):
        torch.manual_seed(12)
        with torch.no_grad():
            outs.append(rend(net, rays[None], want_weights=True, **kw))
    for p in ("coarse", "fine"):
        for key in ("rgb", "depth", "weights"):
            assert _same_bytes(outs[2][p][key], outs[0][p][key]) and _same_bytes(outs[2][p][key], outs[1][p][key]), (p, key)
    N = len(rays)
    assert rend.last_skip_stats == {"coarse": (N * KC, N * KC), "fine": (N * (KC + KF), N * (KC + KF))}
    poses = _poses(dev)
    torch.manual_seed(12)
    gt = (rend.render_views(net, poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C).rgb.clamp(0, 1) * 0.9 + 0.05).contiguous()
    views = []
    for kw in ({}, dict(occupancy=full, skip_empty=True), dict(occupancy=full, skip_empty=True, views_per_call=1)):
        torch.manual_seed(12)
        views.append(rend.render_views(net, poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C, gt_rgb=gt, **kw))
    for v in views[1:]:
        assert _same_bytes(v.rgb, views[0].rgb) and _same_bytes(v.depth, views[0].depth)
        assert _same_bytes(v.psnr, views[0].psnr) and _same_bytes(v.ssim, views[0].ssim)
        assert v.n_hit == 2 * H * W
        assert rend.last_skip_stats == {"coarse": (2 * H * W * KC,) * 2, "fine": (2 * H * W * (KC + KF),) * 2}


def test_a_pass_that_keeps_nothing_launches_no_network(ops, dev, setup):
    """3 coarse samples at z = 1.48, 2.41, 3.35 (u1 = 0.3) on rays through a 4x4x4-cell block around the origin, 2.73 away: every
    ray passes through occupied cells, no coarse sample lies in one.  The coarse outputs are the compositing of all-zero rgb sigma,
    the coarse weights are all equal, so the 8 importance samples (u2 = 0.5: the middle bin; u3 in [0.62, 0.67]: z = 2.71 .. 2.76)
    land in the block: the fine pass runs its network, and only it does."""
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    net = setup("sn64", PLUMBING_PRECISION)[0]
    R = 64
    rs = np.random.RandomState(8)
    v = rs.standard_normal((R, 3))
    o = 2.732 * v / np.linalg.norm(v, axis=1, keepdims=True)
    d = rs.uniform(-0.03, 0.03, (R, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = torch.from_numpy(np.concatenate([o, d, np.full((R, 1), 1.2), np.full((R, 1), 4.0)], axis=1).astype(np.float32)).to(dev)
    field = torch.zeros((33, 33, 33), device=dev)
    field[16, 16, 16] = 1.0
    occ = OccupancyGrid.from_density(field, S.C1, S.C2, 0.5, dilate=1)
    assert int(occ.n_occupied) == 64
    rend = NeRFRenderer(n_coarse=3, n_fine=8, n_fine_depth=0, white_bkgd=True).to(dev).eval()
    noise = {"u1": torch.full((R, 3), 0.3, device=dev), "u2": torch.full((R, 8), 0.5, device=dev),
             "u3": torch.linspace(0.62, 0.67, 8, device=dev).repeat(R, 1).contiguous()}
    assert bool((occ.clip_rays(rays)[1] != 0).all())
    ops.profile_enable(True)
    try:
        with torch.no_grad():
            out = rend(net, rays[None], want_weights=True, _noise=noise, occupancy=occ, skip_empty=True)
        torch.cuda.synchronize()
        launches = ops.profile_read()[1]
        stats = rend.last_skip_stats
        print(f"kept samples coarse {stats['coarse']}, fine {stats['fine']}; network launches {launches}")
        assert stats["coarse"] == (0, R * 3)
        assert stats["fine"][1] == R * 11 and stats["fine"][0] >= R * 8
        # the launches of the whole call are those of ONE network call on the fine pass's kept samples
        z_c = ops.sample_coarse(rays, noise["u1"])
        zero = torch.zeros((R, 3, 4), device=dev)
        w_c, rgb_c, d_c = ops.composite(rays, z_c, zero, True, True)
        z_f = ops.sample_fine(rays, w_c, d_c, z_c, noise["u2"], noise["u3"], None, rend.depth_std, False)
        _, rays_k, z_k, M = ops.compact_samples(occ.mark_samples(rays, z_f), rays, z_f)
        assert M == stats["fine"][0]
        ops.profile_enable(True)                                             # (resets the count)
        ops.eval_ray_samples(net.scene(), net.packed(False), rays_k, z_k.unsqueeze(1), net.tables(False))
        torch.cuda.synchronize()
        assert launches == ops.profile_read()[1] > 0
    finally:
        ops.profile_enable(False)
    assert _same_bytes(out.coarse.rgb[0], rgb_c) and _same_bytes(out.coarse.depth[0], d_c) and _same_bytes(out.coarse.weights[0], w_c)
    assert (out.coarse.rgb == 1.0).all() and (out.coarse.depth == 0).all() and (out.coarse.weights == 0).all()
    _assert_identity_a(ops, net, rend, rays, noise, occ, out, what="coarse pass keeps nothing")


# ---------------------------------------------------------------- 7. refusals

def test_skip_empty_refusals(ops, dev, setup):
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.util.conf import default_model_conf
    net, rend, rays, noise, occ = setup("sn64")

    class Plain(torch.nn.Module):
        use_viewdirs = True

        def forward(self, xyz, coarse=True, viewdirs=None):
            return net(xyz, coarse=coarse, viewdirs=viewdirs)

    with torch.no_grad(), pytest.raises(NotImplementedError, match="generic model callable"):
        rend(Plain(), rays[None], occupancy=occ, skip_empty=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="composed"):
        rend.render_views(Plain(), _poses(dev), W, H, FOCAL, Z_NEAR, Z_FAR, c=C, occupancy=occ, skip_empty=True)
    conf = default_model_conf()
    composed = make_model(conf).to(dev).eval()
    composed.use_code_viewdirs = True                                        # outside what the fused kernels implement
    assert not composed.fused_supported()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="composed"):
        rend(composed, rays[None], occupancy=occ, skip_empty=True)
    with pytest.raises(ValueError, match="occupancy"):
        rend(net, rays[None], skip_empty=True)
    p = next(net.mlp_coarse.parameters())
    try:
        p.requires_grad_(True)
        with pytest.raises(NotImplementedError, match="inference"):
            rend(net, rays[None], occupancy=occ, skip_empty=True)
    finally:
        p.requires_grad_(False)
    # the raw entries: -1 on null or bad arguments
    lib = ops._lib.load()
    lo, hi = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    z = torch.zeros((4, 2), device=dev)
    r4 = torch.zeros((4, 8), device=dev)
    keep = torch.zeros((4, 2), dtype=torch.uint8, device=dev)
    bits = torch.zeros((1,), dtype=torch.int32, device=dev)
    a = lambda t: t.data_ptr()  # noqa: E731
    assert lib.pnr_occupancy_mark_samples(a(r4), a(z), 4, 2, a(bits), 4, 4, 4, lo, hi, None, None) == -1
    assert lib.pnr_occupancy_mark_samples(a(r4), a(z), 4, 0, a(bits), 4, 4, 4, lo, hi, a(keep), None) == -1
    assert lib.pnr_occupancy_mark_samples(a(r4), a(z), 4, 2, a(bits), 4, 1, 4, lo, hi, a(keep), None) == -1
    assert lib.pnr_occupancy_mark_samples(a(r4), a(z), 4, 2, a(bits), 4, 4, 4, hi, lo, a(keep), None) == -1
    assert lib.pnr_occupancy_mark_samples(a(r4), a(z), 4, 2, a(bits), 4, 4, 4, lo, hi, a(keep), None) == 0
    idx, rc, zc = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros((8, 8), device=dev), torch.zeros(8, device=dev)
    count, ws = torch.zeros((), dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.uint8, device=dev)
    assert lib.pnr_compact_samples(a(keep), a(r4), a(z), 4, 2, a(idx), a(rc), a(zc), None, a(ws), 4, None) == -1
    assert lib.pnr_compact_samples(a(keep), a(r4), a(z), 4, 2, a(idx), a(rc), a(zc), a(count), a(ws), 0, None) == -1
    assert lib.pnr_compact_samples(a(keep), a(r4), a(z), -1, 2, a(idx), a(rc), a(zc), a(count), a(ws), 4, None) == -1
    assert lib.pnr_compact_samples(a(keep), a(r4), a(z), 4, 2, a(idx), a(rc), a(zc), a(count), a(ws), 4, None) == 0
    out = torch.zeros((8, 4), device=dev)
    assert lib.pnr_expand_rgbsigma(a(idx), a(rc), 2, 8, None, None) == -1
    assert lib.pnr_expand_rgbsigma(None, a(rc), 2, 8, a(out), None) == -1
    assert lib.pnr_expand_rgbsigma(a(idx), a(rc), 9, 8, a(out), None) == -1
    assert lib.pnr_expand_rgbsigma(a(idx), a(rc), 0, 2 ** 31, a(out), None) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="keep"):
        ops.compact_samples(keep[:2], r4, z)
