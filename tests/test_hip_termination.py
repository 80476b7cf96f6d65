"""GPU tests (-m gpu) of early ray termination: pnr_termination_mark through ops.termination_mark, and the `terminate=` /
`terminate_stages=` keywords of NeRFRenderer.forward / render_views.

Mark: the transmittance lies in the restatement's bracket and the keep bytes equal it on every ray whose stop is decided
(tests/termination_ref.py).  Rendering: Identity T without a tolerance -- the terminated fine pass is ops.composite of the dense fine
pass's per-sample outputs with rgb sigma = 0 behind each ray's stop (and in the cells a grid calls empty), and the coarse pass is
the dense call's -- and Bound B against the dense render itself."""
import numpy as np
import pytest
import torch

import termination_ref as T
from test_hip_skip_empty import (C, FOCAL, H, KC, KF, KFD, W, Z_FAR, Z_NEAR, _poses, _same_bytes, dev, ops, setup)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

EPS = 1e-2
STAGES = 4
K = KC + KF
FP32_BAR = 2e-5     # the project's fp32 per-point bar; covers the rounding of a 96-term fp32 sum


# ---------------------------------------------------------------- 1. the mark kernel

@pytest.mark.parametrize("shape", T.MARK_SHAPES, ids=lambda s: "%dx%d" % s)
def test_mark_equals_the_restatement(ops, dev, shape):
    """(3,63) .. (7,65): the 64-lane chunk edge; (64,96): the renderer's shape; (16,200): four chunks, the carried product.
    k_begin at 0, 1, around the chunk edge and at K (where `far` gives the last interval)."""
    R, Kk = shape
    lib = ops._lib.load()
    rays, z, rs, keep_in = T.mark_case(R, Kk)
    d = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    rays_d, z_d, rs_d, in_d = d(rays), d(z), d(rs), d(keep_in)
    begins = sorted({k for k in T.K_BEGINS + (Kk,) if k <= Kk})
    n_stopped, n_amb = 0, 0
    for k0 in begins:
        for k1 in sorted({min(Kk, k0 + 70), Kk}):
            for mask_np, mask_d in ((None, None), (keep_in, in_d)):
                keep, t = ops.termination_mark(rays_d, z_d, rs_d, k0, k1, EPS, keep_in=mask_d)
                assert keep.dtype == torch.uint8 and keep.shape == (R, Kk) and t.shape == (R,) and t.dtype == torch.float32
                want, lo, hi, amb = T.mark_ref(rays, z, rs, k0, k1, EPS, mask_np)
                got, tf = keep.cpu().numpy(), t.cpu().numpy().astype(np.float64)
                inside = (tf >= lo) & (tf <= hi)
                print(f"mark {R}x{Kk} [{k0},{k1}) keep_in={'yes' if mask_np is not None else 'no'}: stopped {int((hi <= EPS).sum())}, "
                      f"ambiguous {int(amb.sum())}, t_front outside its bracket {int((~inside).sum())}, keep mismatches on decided rays "
                      f"{int((got != want)[~amb].sum())}")
                assert inside.all()
                assert amb.mean() <= T.AMBIGUOUS_CAP
                assert ((got == 0) | (got == 1)).all()
                assert np.array_equal(got[~amb], want[~amb])
                if k0 == 0:
                    assert (tf == 1.0).all()
                assert not (hi[-1] <= EPS)                                   # the ray with the NaN sigma stays alive
                n_stopped, n_amb = n_stopped + int((hi <= EPS).sum()), n_amb + int(amb.sum())
                # the raw entry on a 0xFF prefill: every byte is written; a second call gives the same bytes
                outs = []
                for _ in range(2):
                    raw = torch.full((R, Kk), 0xFF, dtype=torch.uint8, device=dev)
                    tr = torch.full((R,), float("nan"), device=dev)
                    rc = lib.pnr_termination_mark(rays_d.data_ptr(), z_d.data_ptr(), rs_d.data_ptr(), R, Kk, k0, k1, EPS,
                                                  None if mask_d is None else mask_d.data_ptr(), raw.data_ptr(), tr.data_ptr(), None)
                    assert rc == 0, lib.pnr_last_error()
                    torch.cuda.synchronize()
                    outs.append((raw, tr))
                assert _same_bytes(outs[0][0], keep) and _same_bytes(outs[0][1], t)
                assert _same_bytes(outs[0][0], outs[1][0]) and _same_bytes(outs[0][1], outs[1][1])
                # t_front is optional
                raw = torch.full((R, Kk), 0xFF, dtype=torch.uint8, device=dev)
                assert lib.pnr_termination_mark(rays_d.data_ptr(), z_d.data_ptr(), rs_d.data_ptr(), R, Kk, k0, k1, EPS,
                                                None if mask_d is None else mask_d.data_ptr(), raw.data_ptr(), None, None) == 0
                assert _same_bytes(raw, keep)
    if R >= 16:
        assert n_stopped > 0                                                 # (both outcomes occur on the larger cases)
    empty = ops.termination_mark(torch.zeros((0, 8), device=dev), torch.zeros((0, 3), device=dev), torch.zeros((0, 3, 4), device=dev), 0, 3, EPS)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


def test_t_front_is_the_compositing_transmittance(ops, dev):
    """t_front in front of sample k equals, bit for bit, what ops.composite uses for sample k: with sigma = +inf at sample k alone
    (alpha = 1) and zero behind, composite's weight k IS that transmittance"""
    R, Kk = 16, 200
    rays, z, rs, _ = T.mark_case(R, Kk)
    rays_d, z_d = torch.from_numpy(rays).to(dev), torch.from_numpy(z).to(dev)
    for k in (1, 63, 64, 65, 130, 199):
        probe = rs.copy()
        probe[:, k:, 3] = 0.0
        probe[:, k, 3] = np.inf
        w = ops.composite(rays_d, z_d, torch.from_numpy(probe).to(dev), False, True)[0]
        t = ops.termination_mark(rays_d, z_d, torch.from_numpy(rs).to(dev), k, Kk, EPS)[1]
        ok = (z[:, k + 1] > z[:, k]) if k + 1 < Kk else np.ones(R, bool)    # (a zero interval gives alpha = NaN: not a probe)
        assert ok.sum() >= R - 1 and _same_bytes(w[:, k][torch.from_numpy(ok).to(dev)], t[torch.from_numpy(ok).to(dev)]), k


# ---------------------------------------------------------------- 2. Identity T

CONFIGS = [("sn64", None, True), ("sn64", "f16", True), ("sn64", "f32", True), ("dtu_mini", None, True), ("dtu_mini", "f16", True),
           ("sn64", "f16", False)]
CONFIG_IDS = ["sn64-default", "sn64-f16", "sn64-f32", "dtu3view-default", "dtu3view-f16", "sn64-f16-no_fine_network"]
NOT_VACUOUS = {"sn64": (0.30, 0.85), "dtu_mini": (0.10, 0.95)}             # rays that stop >=, evaluated share <=


@pytest.fixture(scope="module")
def reference(ops, dev, setup):
    """-> f(scene, precision, use_fine, with_grid) = dict of the staged reference of that configuration, computed once: the rendered
    rays (idx into the 256), the dense coarse pass, the fine samples, the DENSE fine outputs (rgb sigma = 0 where the grid calls a
    sample empty), the restatement's stops on them, and ops.composite of the outputs zeroed behind the stops"""
    cache = {}

    def make(scene_name, precision, use_fine, with_grid):
        key = (scene_name, precision, use_fine, with_grid)
        if key in cache:
            return cache[key]
        net, rend, rays, noise, occ = setup(scene_name, precision, use_fine)
        grid = occ if with_grid else None
        idx = torch.nonzero(occ.clip_rays(rays)[1]).flatten() if with_grid else torch.arange(len(rays), device=dev)
        sub, sub_noise = rays[idx].contiguous(), {k: v[idx].contiguous() for k, v in noise.items()}
        scene = net.scene()

        def network(coarse, z):
            rs = ops.eval_ray_samples(scene, net.packed(coarse), sub, z, net.tables(coarse))
            keep = grid.mark_samples(sub, z) if grid is not None else None
            return (rs if keep is None else torch.where(keep.unsqueeze(-1) != 0, rs, torch.zeros_like(rs))), keep

        with torch.no_grad():
            z_c = ops.sample_coarse(sub, sub_noise["u1"], rend.lindisp)
            rs_c, _ = network(True, z_c)
            w_c, rgb_c, d_c = ops.composite(sub, z_c, rs_c, rend.white_bkgd, True)
            z_f = ops.sample_fine(sub, w_c, d_c, z_c, sub_noise.get("u2"), sub_noise.get("u3"), sub_noise.get("n4"), rend.depth_std, rend.lindisp)
            rs_f, keep_f = network(False, z_f)
            bounds = T.stage_bounds(K, STAGES)
            sub_np, z_np, rs_np = sub.cpu().numpy(), z_f.cpu().numpy(), rs_f.cpu().numpy()
            stop, amb = T.stops(sub_np, z_np, rs_np, bounds, EPS)
            zeroed = torch.from_numpy(T.zero_behind(rs_np, stop)).to(dev)
            w_f, rgb_f, d_f = ops.composite(sub, z_f, zeroed, rend.white_bkgd, True)
            w_d, rgb_d, d_d = ops.composite(sub, z_f, rs_f, rend.white_bkgd, True)
        cache[key] = dict(idx=idx, sub=sub, z_f=z_np, stop=stop, amb=amb, bounds=bounds,
                          coarse=dict(rgb=rgb_c, depth=d_c, weights=w_c), fine=dict(rgb=rgb_f, depth=d_f, weights=w_f),
                          dense_fine=dict(rgb=rgb_d, depth=d_d, weights=w_d),
                          counts=T.counts(stop, bounds, None if keep_f is None else keep_f.cpu().numpy()))
        return cache[key]
    return make


def _grid_kw(occ, with_grid):
    return dict(occupancy=occ, skip_empty=True) if with_grid else {}


@pytest.mark.parametrize("with_grid", [False, True], ids=["no_grid", "ball_grid_skip_empty"])
@pytest.mark.parametrize("scene_name,precision,use_fine", CONFIGS, ids=CONFIG_IDS)
def test_terminate_is_the_dense_fine_pass_with_sigma_zero_behind_the_stop(ops, dev, setup, reference, scene_name, precision, use_fine, with_grid):
    """Identity T, 256 rays, 64 + 32 (16 depth) samples, white background, eps = 1e-2, 4 stages (boundaries 24 / 48 / 72): rgb, depth
    and weights of the fine pass are bit-equal, on every ray whose stop is decided, to the reference built from the existing staged
    ops; the coarse outputs are bit-equal to the same call without `terminate`.  The default precision ("f16x3") is the case that
    bites the pair rule: a stage's compacted list moves a sample to another place of the launch."""
    net, rend, rays, noise, occ = setup(scene_name, precision, use_fine)
    assert (net.mlp_fine is not None) == use_fine
    ref = reference(scene_name, precision, use_fine, with_grid)
    what = f"{scene_name} {precision} fine={use_fine} grid={with_grid}"
    with torch.no_grad():
        out = rend(net, rays[None], want_weights=True, _noise=noise, terminate=EPS, terminate_stages=STAGES, **_grid_kw(occ, with_grid))
        stats, skip_stats = rend.last_terminate_stats, rend.last_skip_stats
        plain = rend(net, rays[None], want_weights=True, _noise=noise, **_grid_kw(occ, with_grid))
    idx, amb, stop, want = ref["idx"], ref["amb"], ref["stop"], ref["counts"]
    sel = torch.from_numpy(~amb).to(dev)
    n = len(idx)
    share, stopped = want["evaluated"] / want["total"], want["stopped_rays"] / n
    print(f"{what}: {n} rays rendered, {want['stopped_rays']} stop ({100 * stopped:.1f} %), evaluated share {share:.4f}, ambiguous "
          f"{int(amb.sum())}; stats {stats}; reference {want}")
    for key in ("rgb", "depth", "weights"):
        got, exp = out.fine[key][0][idx][sel], ref["fine"][key][sel]
        differ = (got != exp).reshape(int(sel.sum()), -1).any(dim=1)
        print(f"{what}: fine {key}: {int(differ.sum())} of {int(sel.sum())} decided rays differ from the reference, max abs "
              f"{float((got - exp).abs().max()):.3e}; coarse {key} equal to the call without terminate: "
              f"{_same_bytes(out.coarse[key], plain.coarse[key])}")
    assert n > 0 and amb.mean() <= T.AMBIGUOUS_CAP
    for key in ("rgb", "depth", "weights"):
        assert _same_bytes(out.fine[key][0][idx][sel], ref["fine"][key][sel]), f"{what}: fine {key} differs from the reference"
        assert _same_bytes(out.coarse[key], plain.coarse[key]), f"{what}: coarse {key} differs from the call without terminate"
        assert _same_bytes(out.coarse[key][0][idx], ref["coarse"][key]), f"{what}: coarse {key} differs from the staged reference"
    if with_grid:
        miss = torch.ones(len(rays), dtype=torch.bool, device=dev)
        miss[idx] = False
        assert (out.fine.rgb[0][miss] == 1.0).all() and (out.fine.depth[0][miss] == 0).all() and (out.fine.weights[0][miss] == 0).all()
    # not vacuous.  The share of rays that stop is required where the CPU oracle states it: without a grid (57 % / 0.70 on sn64,
    # 25 % / 0.88 on dtu_mini).  The ball grid of radius 0.5 sets sigma to 0 outside the ball, so most rays no longer go opaque
    # (sn64: 18 of 155, dtu_mini: 6 of 243 in the restatement); there the stop rule must still fire: at least one ray stops, and the
    # network runs on no more samples than skip_empty alone keeps (on dtu_mini exactly as many: behind the 6 stops the ball is over)
    min_stopped, max_share = NOT_VACUOUS[scene_name]
    assert share <= max_share, what
    if with_grid:
        kept_by_grid = rend.last_skip_stats["fine"][0]                       # (of the call without terminate, just above)
        print(f"{what}: skip_empty alone keeps {kept_by_grid} fine samples, with terminate {stats['evaluated']}")
        assert want["stopped_rays"] >= 1 and stats["evaluated"] <= kept_by_grid, what
    else:
        assert stopped >= min_stopped, what
        assert not _same_bytes(out.fine.weights, plain.fine.weights)         # (with the grid the stops may cut off empty samples only)
    # the counts
    assert all(type(stats[k]) is int for k in ("evaluated", "total", "stopped_rays", "rays"))
    assert all(type(v) is int for pair in stats["stages"] for v in pair) and len(stats["stages"]) == STAGES
    assert stats["rays"] == n and stats["total"] == n * K and stats["evaluated"] == sum(m for m, _ in stats["stages"])
    if not amb.any():
        assert stats == want, what
    if with_grid:
        assert skip_stats["fine"] == (stats["evaluated"], stats["total"])


# ---------------------------------------------------------------- 3. against the dense render itself

def test_against_the_dense_render(ops, dev, setup, reference):
    """No restatement: per ray there is a stage boundary in front of which the weights are the dense render's bytes and behind
    which they are 0; on the rays whose intervals are all non-negative, Bound B."""
    net, rend, rays, noise, _ = setup("sn64", None, True)
    with torch.no_grad():
        dense = rend(net, rays[None], want_weights=True, _noise=noise)
        term = rend(net, rays[None], want_weights=True, _noise=noise, terminate=EPS, terminate_stages=STAGES)
    stats = rend.last_terminate_stats
    wd, wt = dense.fine.weights[0], term.fine.weights[0]
    bounds = T.stage_bounds(K, STAGES)
    same = (wd.view(torch.int32) == wt.view(torch.int32))
    stop = torch.zeros(len(rays), dtype=torch.long, device=dev)
    for b in bounds[1:]:                                                     # the last boundary in front of which every weight is the dense one
        stop = torch.where(same[:, :b].all(dim=1), torch.full_like(stop, b), stop)
    behind = torch.arange(K, device=dev)[None, :] >= stop[:, None]
    differ = (~same).any(dim=1)
    z_f = torch.from_numpy(reference("sn64", None, True, False)["z_f"]).to(dev)
    far = rays[:, 7]
    ok = (torch.diff(torch.cat([z_f, far[:, None]], dim=1), dim=1) >= 0).all(dim=1)
    d_rgb = (dense.fine.rgb[0] - term.fine.rgb[0]).abs().max(dim=1).values
    d_depth = (dense.fine.depth[0] - term.fine.depth[0]).abs()
    print(f"against dense: {int(differ.sum())} of {len(rays)} rays differ, stops at {sorted(set(stop.tolist()))}, weights behind the stop "
          f"non-zero on {int(((wt != 0) & behind).any(dim=1).sum())} rays; rays with all delta >= 0: {int(ok.sum())}, max |d rgb| on them "
          f"{float(d_rgb[ok].max()):.3e}, max |d depth| {float(d_depth[ok].max()):.3e}, on the others {float(d_rgb[~ok].max()) if (~ok).any() else 0:.3e}; "
          f"stats {stats}")
    assert (stop > 0).all()
    assert ((wt == 0) | ~behind).all()
    assert differ.any() and int(differ.sum()) <= stats["stopped_rays"]
    assert (~differ | (stop < K)).all()
    assert ok.sum() >= len(rays) // 2
    assert (d_rgb[ok] <= EPS + FP32_BAR).all()
    assert (d_depth[ok] <= (EPS + FP32_BAR) * far[ok]).all()
    for key in ("rgb", "depth", "weights"):
        assert _same_bytes(dense.coarse[key], term.coarse[key])


# ---------------------------------------------------------------- 4. degenerate and public paths

def test_one_stage_is_the_dense_call(dev, setup):
    net, rend, rays, _, occ = setup("sn64", None, True)
    for kw in ({}, dict(occupancy=occ), dict(occupancy=occ, skip_empty=True)):
        outs = []
        for extra in ({}, dict(terminate=EPS, terminate_stages=1)):
            torch.manual_seed(5)
            with torch.no_grad():
                outs.append(rend(net, rays[None], want_weights=True, **kw, **extra))
        for p in ("coarse", "fine"):
            for key in ("rgb", "depth", "weights"):
                assert _same_bytes(outs[0][p][key], outs[1][p][key]), (sorted(kw), p, key)
        st = rend.last_terminate_stats
        assert st["stopped_rays"] == 0 and st["evaluated"] == st["stages"][0][0] and len(st["stages"]) == 1
        if not kw.get("skip_empty"):
            assert st["evaluated"] == st["total"] == st["rays"] * K


@pytest.mark.parametrize("with_grid", [False, True], ids=["no_grid", "ball_grid_skip_empty"])
def test_render_views_equals_forward_over_the_same_cameras(dev, setup, with_grid):
    """two 16 x 16 views: render_views(terminate=) equals forward(terminate=) on util.gen_rays of the same cameras under the same
    seed (seeded draws, the bound wrapper, views_per_call); PSNR / SSIM are present"""
    from pixelnerf_amd import util
    net, rend, _, _, occ = setup("sn64", None, True)
    kw = dict(terminate=EPS, **_grid_kw(occ, with_grid))
    poses = _poses(dev)
    rays = util.gen_rays(poses.reshape(-1, 4, 4), W, H, FOCAL, Z_NEAR, Z_FAR, C).reshape(1, -1, 8)
    torch.manual_seed(21)
    with torch.no_grad():
        fwd = rend(net, rays, **kw)
    fwd_stats = rend.last_terminate_stats
    torch.manual_seed(21)
    with torch.no_grad():
        dense = rend(net, rays)
    gt = (dense.fine.rgb.reshape(2, H, W, 3).clamp(0, 1) * 0.9 + 0.05).contiguous()
    par = rend.bind_parallel(net, None, simple_output=True).eval()
    for call, extra in ((rend.render_views, (net,)), (par.render_views, ())):
        for vpc in (None, 1):
            torch.manual_seed(21)
            v = call(*extra, poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C, gt_rgb=gt, views_per_call=vpc, **kw)
            assert _same_bytes(v.rgb.reshape(1, -1, 3), fwd.fine.rgb) and _same_bytes(v.depth.reshape(1, -1), fwd.fine.depth), vpc
            assert v.psnr.shape == (1, 2) and v.ssim.shape == (1, 2) and torch.isfinite(v.psnr).all() and torch.isfinite(v.ssim).all()
            assert ("hit" in v) == with_grid
            assert rend.last_terminate_stats == fwd_stats, vpc                # (summed over the groups of views)
    torch.manual_seed(21)
    with torch.no_grad():
        rgb, depth = par(rays, **kw)
    assert _same_bytes(rgb, fwd.fine.rgb) and _same_bytes(depth, fwd.fine.depth)
    assert fwd_stats["stopped_rays"] > 0 and not _same_bytes(fwd.fine.rgb, dense.fine.rgb)
    for key in ("rgb", "depth"):
        assert _same_bytes(fwd.coarse[key], dense.coarse[key]) or with_grid


# ---------------------------------------------------------------- 5. refusals; a stage that keeps nothing

def test_a_stage_that_keeps_nothing_launches_no_network(ops, dev, setup, monkeypatch):
    """The rays of test_hip_skip_empty's last case: 3 coarse samples at z = 1.48, 2.41, 3.35 outside a 4x4x4-cell block around the
    origin, 8 importance samples at z = 2.71 .. 2.76 inside it.  With skip_empty the coarse pass keeps nothing; with the fine
    boundaries at 2 and 10 the first stage (1.48, 2.41) and the last (3.35) keep nothing either, the middle one holds every kept
    sample: ONE network call in all, and the loop went on past the empty stage."""
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.occupancy import OccupancyGrid
    import skip_ref as S
    net = setup("sn64", None, True)[0]
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
    rend = NeRFRenderer(n_coarse=3, n_fine=8, n_fine_depth=0, white_bkgd=True).to(dev).eval()
    noise = {"u1": torch.full((R, 3), 0.3, device=dev), "u2": torch.full((R, 8), 0.5, device=dev),
             "u3": torch.linspace(0.62, 0.67, 8, device=dev).repeat(R, 1).contiguous()}
    calls = []
    real = ops.eval_ray_samples
    monkeypatch.setattr(ops, "eval_ray_samples", lambda *a, **k: (calls.append(a[2].shape[0]), real(*a, **k))[1])
    with torch.no_grad():
        out = rend(net, rays[None], want_weights=True, _noise=noise, occupancy=occ, skip_empty=True, terminate=EPS, terminate_stages=[2, 10])
    st = rend.last_terminate_stats
    print(f"network calls {calls}; stats {st}; skip stats {rend.last_skip_stats}")
    assert rend.last_skip_stats["coarse"] == (0, R * 3)
    assert st["stages"][0] == (0, R * 2) and st["stages"][2] == (0, R * 1) and st["stages"][1][1] == R * 8 and st["stages"][1][0] > 0
    assert st["evaluated"] == st["stages"][1][0] and st["total"] == R * 11 and st["rays"] == R
    assert len(calls) == 1
    monkeypatch.undo()
    with torch.no_grad():
        skip = rend(net, rays[None], want_weights=True, _noise=noise, occupancy=occ, skip_empty=True)
    for p in ("coarse", "fine"):                                             # behind either boundary lie empty samples only: the skip_empty render
        for key in ("rgb", "depth", "weights"):
            assert _same_bytes(out[p][key], skip[p][key]), (p, key)


def test_refusals_on_the_device(ops, dev, setup, monkeypatch):
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import default_model_conf
    net, rend, rays, noise, occ = setup("sn64", None, True)
    rend.last_terminate_stats = None
    calls = []
    real = ops.eval_ray_samples
    monkeypatch.setattr(ops, "eval_ray_samples", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    poses = _poses(dev)

    class Plain(torch.nn.Module):
        use_viewdirs = True

        def forward(self, xyz, coarse=True, viewdirs=None):
            return net(xyz, coarse=coarse, viewdirs=viewdirs)

    for grid_kw in ({}, dict(occupancy=occ), dict(occupancy=occ, skip_empty=True)):
        for eps in (0.0, 1.0, -0.1, float("nan")):
            with torch.no_grad(), pytest.raises(ValueError, match="eps must lie in"):
                rend(net, rays[None], terminate=eps, **grid_kw)
        for stages in (0, [0], [K], [30, 30], [40, 20]):
            with torch.no_grad(), pytest.raises(ValueError, match="terminate_stages"):
                rend(net, rays[None], terminate=EPS, terminate_stages=stages, **grid_kw)
            with pytest.raises(ValueError, match="terminate_stages"):
                rend.render_views(net, poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C, terminate=EPS, terminate_stages=stages, **grid_kw)
        with torch.no_grad(), pytest.raises(ValueError, match="ONE object|ONE, the call has"):
            rend(net, rays.reshape(2, -1, 8), terminate=EPS, **grid_kw)
        p = next(net.mlp_coarse.parameters())
        try:
            p.requires_grad_(True)
            with pytest.raises(NotImplementedError, match="inference"):
                rend(net, rays[None], terminate=EPS, **grid_kw)
        finally:
            p.requires_grad_(False)
        with monkeypatch.context() as m:                                     # a HIP-graph capture in progress (nothing is captured here)
            m.setattr(torch.cuda, "is_current_stream_capturing", lambda *a: True)
            with torch.no_grad(), pytest.raises(NotImplementedError, match="capture"):
                rend(net, rays[None], terminate=EPS, **grid_kw)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="generic model callable"):
            rend(Plain(), rays[None], terminate=EPS, **grid_kw)
        with pytest.raises(NotImplementedError, match="composed"):
            rend.render_views(Plain(), poses, W, H, FOCAL, Z_NEAR, Z_FAR, c=C, terminate=EPS, **grid_kw)
        coarse_only = NeRFRenderer(n_coarse=KC, n_fine=0, white_bkgd=True).to(dev).eval()
        with torch.no_grad(), pytest.raises(NotImplementedError, match="FINE pass"):
            coarse_only(net, rays[None], terminate=EPS, **grid_kw)
        noisy = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, noise_std=1.0, white_bkgd=True).to(dev).train()
        with torch.no_grad(), pytest.raises(NotImplementedError, match="noise_std"):
            noisy(net, rays[None], terminate=EPS, **grid_kw)
        assert coarse_only.last_terminate_stats is None and noisy.last_terminate_stats is None
    composed = make_model(default_model_conf()).to(dev).eval()
    composed.use_code_viewdirs = True                                        # outside what the fused kernels implement
    assert not composed.fused_supported()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="composed"):
        rend(composed, rays[None], terminate=EPS)
    assert rend.last_terminate_stats is None and not calls                   # every refusal came before any network launch
    with pytest.raises(ValueError, match="keep_in"):
        ops.termination_mark(rays, torch.zeros((len(rays), 4), device=dev), torch.zeros((len(rays), 4, 4), device=dev), 0, 4, EPS,
                             keep_in=torch.zeros((2, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="eps"):
        ops.termination_mark(rays, torch.zeros((len(rays), 4), device=dev), torch.zeros((len(rays), 4, 4), device=dev), 0, 4, 1.0)
