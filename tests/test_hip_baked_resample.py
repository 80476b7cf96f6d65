"""GPU tests (-m gpu) of pnr_baked_resample through ops.baked_resample and `volume.resample`, and of what is built on it and on the
visibility: `volume.prune` and util.bake.fit_coarse_to_fine.

The yardstick of the resampling is tests/baked_resample_ref.py (its own checks: tests/test_baked_resample_host.py).  Most of what is
held here is BYTES: the same point count is the identity, a refinement keeps the old points, sparse is dense at the kept ids, half
goes through to_half alone, a 0-step coarse-to-fine run is the hand-written sequence."""
import numpy as np
import pytest
import torch

import baked_grad_ref as G
import baked_resample_ref as RS
import baked_visibility_ref as V
import sparse_baked_ref as SP

pytestmark = pytest.mark.gpu

KINDS = [(kind, half) for kind in RS.KINDS for half in (False, True)]
KIND_IDS = [f"{'rgba' if k is None else f'sh{k}'}_{'fp16' if h else 'fp32'}" for k, h in KINDS]
NON_INTEGER = (((5, 6, 7), (7, 4, 10)), ((6, 5, 9), (9, 7, 4)))   # 7 -> 10 and 9 -> 4 among them


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


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _same(a, b):
    """equal bytes (fp32 as int32 views: -0 is not +0)"""
    view = {torch.float32: torch.int32, torch.float16: torch.int16}.get(a.dtype)
    if view is None:
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _sparse(dev, reso, kind, half):
    """-> (rows, index, ids, bits) on the device: the kept rows of RS.volume under RS.cells"""
    v, cells = RS.volume(reso, kind, half), RS.cells(reso)
    index, ids = SP.sparse_points(cells)
    rows = v.reshape((-1,) + v.shape[3:])[ids]
    return _t(rows, dev), _t(index, dev), _t(ids, dev), _t(SP.bits_from_cells(cells).copy().view(np.int32), dev)


# ---------------------------------------------------------------- 1. the entry: bytes
@pytest.mark.parametrize("kind,half", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("reso", RS.GRIDS)
def test_same_point_count_is_the_identity(dev, ops, reso, kind, half):
    """dense and sparse, on a volume that holds -0: the int32 views are equal; twice the same bytes"""
    v = _t(RS.volume(reso, kind, half), dev)
    assert bool(((v == 0) & torch.signbit(v)).any())
    out = ops.baked_resample(v, kind, reso, reso)
    assert out.dtype == torch.float32 and _same(out, v.float()) and _same(ops.baked_resample(v, kind, reso, reso), out)
    rows, index, ids, _ = _sparse(dev, reso, kind, half)
    assert 0 < rows.shape[0] < reso[0] * reso[1] * reso[2]
    assert _same(ops.baked_resample(rows, kind, reso, reso, index=index, ids_dst=ids), rows.float())


@pytest.mark.parametrize("kind,half", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("m", [2, 3])
def test_refinement_keeps_the_old_points_and_matches_the_restatement(dev, ops, kind, half, m):
    reso = RS.GRIDS[m - 2]
    v = RS.volume(reso, kind, half)
    new = RS.refined(reso, m)
    out = ops.baked_resample(_t(v, dev), kind, reso, new)
    assert tuple(out.shape[:3]) == new and _same(out[::m, ::m, ::m].contiguous(), _t(v, dev).float())
    assert _same(out.cpu(), RS.resample(v, new, torch.float32))           # every fraction k / m: the fp32 restatement's bytes
    # the rows at a list of ids are the dense result at those ids; an id outside the grid gives a row of zeros
    total = new[0] * new[1] * new[2]
    ids = torch.tensor([0, 5, total - 1, total, -1, 17, 2 ** 31 - 1], dtype=torch.int32, device=dev)
    some = ops.baked_resample(_t(v, dev), kind, reso, new, ids_dst=ids)
    inside = (ids >= 0) & (ids < total)
    flat = out.reshape((total,) + tuple(out.shape[3:]))
    assert _same(some[inside], flat[ids[inside].long()]) and not bool(some[~inside].any()) and not bool(torch.signbit(some[~inside]).any())


@pytest.mark.parametrize("kind,half", [(None, False), (1, True), (2, False)])
def test_sparse_source_is_the_dense_resample_of_to_dense(dev, ops, bake, kind, half):
    """the entry with an index, and SparseBakedVolume.resample around it: the rows at the NEW kept ids of the dense resample of
    to_dense(); a child cell is occupied iff its parent was; the dense tensor is never needed"""
    reso, m = RS.GRIDS[0], 2
    rows, index, ids, bits = _sparse(dev, reso, kind, half)
    occ = bake.OccupancyGrid(bits, reso, V.C1, V.C2, 0.5, 1, torch.tensor(int(RS.cells(reso).sum()), dtype=torch.int32, device=dev))
    sparse = bake.SparseBakedVolume(rows, occ, index=index, ids=ids)
    fine = sparse.resample(RS.refined(reso, m))
    assert isinstance(fine, bake.SparseBakedVolume) and fine.reso == RS.refined(reso, m) and fine.dtype == rows.dtype
    assert (fine.c1, fine.c2, fine.occupancy.threshold, fine.occupancy.dilate) == (sparse.c1, sparse.c2, 0.5, 1)
    cells = SP.cells_from_bits(fine.occupancy.bits.cpu().numpy().view(np.uint32), fine.reso)
    parent = np.repeat(np.repeat(np.repeat(RS.cells(reso), m, 0), m, 1), m, 2)
    assert np.array_equal(cells, parent) and int(fine.occupancy.n_occupied) == int(parent.sum()) == 8 * int(RS.cells(reso).sum())
    want_index, want_ids = SP.sparse_points(parent)
    assert np.array_equal(fine.ids.cpu().numpy(), want_ids) and np.array_equal(fine.index.cpu().numpy(), want_index)
    dense = ops.baked_resample(sparse.to_dense(), kind, reso, fine.reso)
    want = dense.reshape((-1,) + tuple(dense.shape[3:]))[fine.ids.long()]
    assert _same(fine.rows, bake.to_half(want) if half else want)
    if not half:   # and the restatement's bytes
        ref = RS.resample(RS.volume(reso, kind), fine.reso, torch.float32, kept=SP.kept_points(RS.cells(reso)))
        assert _same(fine.rows.cpu(), ref.reshape((-1,) + tuple(ref.shape[3:]))[torch.from_numpy(want_ids.astype(np.int64))])
    with pytest.raises(ValueError, match="integer refinements only"):
        sparse.resample((8, 11, 13))


@pytest.mark.parametrize("kind", [None, 2])
def test_half_volume_resamples_through_to_half_alone(dev, bake, kind):
    reso = RS.GRIDS[1]
    stored = _t(RS.volume(reso, kind, True), dev)
    cls = bake.BakedVolume if kind is None else bake.BakedSHVolume
    half = cls(stored, V.C1, V.C2, 0.25)
    for new in (RS.refined(reso, 2), (9, 7, 4)):
        a, b = half.resample(new), half.float().resample(new)
        assert type(a) is cls and a.dtype == torch.float16 and b.dtype == torch.float32 and a.reso == tuple(new) == b.reso
        assert a.skip_threshold == 0.25 and (a.c1, a.c2) == (half.c1, half.c2)
        assert _same(a._stored(), bake.to_half(b._stored()))
        assert _same(a.occupancy.bits, cls(a._stored(), V.C1, V.C2, 0.25).occupancy.bits)     # the skip grid is the new sigma's
    assert half.resample(9).reso == (9, 9, 9)


# ---------------------------------------------------------------- 2. the entry: against the fp64 restatement
@pytest.mark.parametrize("reso,new", NON_INTEGER)
def test_non_integer_ratios_are_within_4_ulp_of_the_fp64_restatement(dev, ops, reso, new):
    """The bar: the value is three nested blends a + f (b - a), each with ONE rounded fraction f = fp32(rem / den) and the rounding
    of its difference, product and sum.  With |a|, |b| <= A = the largest stored magnitude and u = ulp(A): a blend of exact inputs is
    off by about u (f's relative 2^-24 on a term of at most 2 A, half an ulp for each operation on numbers of at most 2 A and A), the
    errors of the inner blends pass through the outer ones with weights that sum to 1, and three levels add up to 4 u at most in
    all but contrived cases.  The fp32 restatement meets it (tests/test_baked_resample_host.py); the kernel performs its operations."""
    worst = 0.0
    for kind in RS.KINDS:
        v = RS.volume(reso, kind)
        got = ops.baked_resample(_t(v, dev), kind, reso, new).cpu()
        ulp = RS.ulp32(np.abs(v).max())
        worst = max(worst, float((got.double() - RS.resample(v, new, torch.float64)).abs().max()) / ulp)
        assert _same(got, RS.resample(v, new, torch.float32))
    print(f"{reso} -> {new}: HIP against fp64 {worst:.2f} ulp of the largest stored magnitude")
    assert worst <= 4.0


def test_render_of_a_volume_refined_by_2_is_the_render_of_the_original(dev, bake):
    """RGBA: the HIP render of the refined volume against the fp64 restatement march of the ORIGINAL volume.  The bar is 10 x the
    error of the HIP render of the original (the parent's code, not the code under test) against the same march, floor 1e-6."""
    vol, rays = G.rgba_volume(0.15), G.case_rays("n150")
    ref = G.march(rays, G._fp32(vol, torch.float64), G.C1, G.C2, 0.03)
    coarse = bake.BakedVolume(_t(vol, dev), G.C1, G.C2)
    fine = coarse.resample(RS.refined(G.RESO, 2))
    assert fine.reso == (17, 15, 13) and _same(fine.vol[::2, ::2, ::2].contiguous(), coarse.vol)
    a, b = coarse.render(_t(rays, dev), step=0.03, skip=False), fine.render(_t(rays, dev), step=0.03, skip=False)
    for name, want in zip(("rgb", "depth", "alpha"), ref):
        err0 = float((a[name].cpu().double() - want).abs().max())
        err = float((b[name].cpu().double() - want).abs().max())
        bar = max(10.0 * err0, 1e-6)
        print(f"{name}: refined {err:.3e}, original {err0:.3e}, ratio {err / max(err0, 1e-30):.2f}, bar {bar:.3e}")
        assert float(want.abs().max()) > 0.1 and err <= bar, (name, err, bar)


# ---------------------------------------------------------------- 3. prune and fit_coarse_to_fine
def _cells(volume):
    return SP.cells_from_bits(volume.occupancy.bits.cpu().numpy().view(np.uint32), volume.reso)


@pytest.mark.parametrize("kind", [None, 1])
def test_prune_never_adds_a_cell_and_renders_the_kept_part_bit_for_bit(dev, bake, kind):
    case = V.BY_NAME["rgba" if kind is None else "sh1_bits"]
    inp = V.inputs(case)
    cls = bake.BakedVolume if kind is None else bake.BakedSHVolume
    vol = cls(_t(inp["stored"], dev), V.C1, V.C2)
    rays = _t(inp["rays"], dev)
    vis = vol.visibility(rays[:6], step=V.STEP)                                # six rays of one camera: much of the volume is unseen
    threshold = float(vis[vis > 0].median())
    pruned = vol.prune(vis, threshold, dilate=0)
    own, kept = _cells(vol), _cells(pruned)
    assert isinstance(pruned, bake.SparseBakedVolume) and pruned.degree == kind
    assert 0 < kept.sum() < own.sum() and not (kept & ~own).any() and int(pruned.occupancy.n_occupied) == int(kept.sum())
    seen = SP.occupied_cells(vis.cpu().numpy(), threshold)
    assert np.array_equal(kept, seen & own)
    wide = vol.prune(vis, threshold, dilate=1)
    assert not (_cells(wide) & ~own).any() and (_cells(wide) | kept == _cells(wide)).all() and _cells(wide).sum() > kept.sum()
    # a sparse volume prunes to the same thing: its (M,) field is scattered first
    sparse = vol.sparse()
    again = sparse.prune(sparse.visibility(rays[:6], step=V.STEP), threshold, dilate=0)
    assert _same(again.rows, pruned.rows) and _same(again.ids, pruned.ids) and _same(again.occupancy.bits, pruned.occupancy.bits)
    # rays all of whose samples in the volume's own cells lie in kept cells, by the fp64 and the fp32 walk: bit for bit
    ok = None
    for dtype in (torch.float64, torch.float32):
        s = V.weights(inp["rays"], inp["stored"], V.C1, V.C2, V.STEP, kind, None, 0.0, dtype)
        at = lambda c: torch.from_numpy(c)[s["idx"][..., 0], s["idx"][..., 1], s["idx"][..., 2]]
        fine = (~s["active"] | ~at(own) | at(kept)).all(dim=1)
        ok = fine if ok is None else ok & fine
    a, b = pruned.render(rays[ok.to(dev)], step=V.STEP), vol.render(rays[ok.to(dev)], step=V.STEP, skip=True)
    assert int((a.alpha > 0).sum()) >= 5 and int((~ok).sum()) >= 5
    assert all(_same(a[k], b[k]) for k in ("rgb", "depth", "alpha"))
    c, d = pruned.render(rays, step=V.STEP), vol.render(rays, step=V.STEP, skip=True)
    assert not _same(c.rgb, d.rgb)                                             # the other rays lost something: pruning did prune


@pytest.fixture(scope="module")
def fit_scene(dev, bake):
    """baked_grad_ref.fit_scene (12^3, RGBA): the start volume, the rays and the HIP render of the known volume as the target"""
    known, start, rays = G.fit_scene(None)
    rays = _t(rays, dev)
    target = bake.BakedVolume(_t(known, dev), G.FIT_C1, G.FIT_C2).render(rays, step=G.FIT_STEP, skip=False).rgb
    return bake.BakedVolume(_t(start, dev), G.FIT_C1, G.FIT_C2), rays, target


def test_zero_step_stages_are_the_hand_written_sequence(dev, bake, fit_scene):
    start, rays, target = fit_scene
    prune = dict(threshold=1e-3, dilate=1)
    got, losses = bake.fit_coarse_to_fine(start, rays, target, [(None, 0), (23, 0), ((23, 45, 23), 0)], prune=prune, step=G.FIT_STEP)
    assert losses == [[], [], []]
    v = start
    v = v.prune(v.visibility(rays, step=G.FIT_STEP, skip=False), 1e-3, 1)
    for reso in ((23, 23, 23), (23, 45, 23)):
        v = v.resample(reso)
        v = v.prune(v.visibility(rays, step=G.FIT_STEP), 1e-3, 1)
    assert isinstance(got, bake.SparseBakedVolume) and got.reso == (23, 45, 23) == v.reso and 0 < got.n_rows < 23 * 45 * 23
    assert _same(got.rows, v.rows) and _same(got.ids, v.ids) and _same(got.index, v.index) and _same(got.occupancy.bits, v.occupancy.bits)
    # without pruning: the dense volume, resampled
    plain, _ = bake.fit_coarse_to_fine(start, rays, target, [(None, 0), (23, 0)])
    assert isinstance(plain, bake.BakedVolume) and _same(plain.vol, start.resample(23).vol)


@pytest.mark.parametrize("prune", [None, dict(threshold=1e-3, dilate=1)], ids=["dense", "pruned"])
def test_every_stage_of_a_coarse_to_fine_fit_lowers_its_loss(dev, bake, fit_scene, prune):
    """No bytes are compared with a host loop: `fit` goes through the stored backward's fp32 atomics, which are not bit-reproducible.
    What is held is what a fit is for: per stage, the mean of the last 10 batch losses lies below the stage's first loss."""
    start, rays, target = fit_scene
    got, losses = bake.fit_coarse_to_fine(start, rays, target, [(None, 15), (23, 40)], prune=prune, step=G.FIT_STEP, lr=2e-2, batch=256,
                                          seed=3)
    assert [len(l) for l in losses] == [15, 40] and got.reso == (23, 23, 23)
    assert isinstance(got, bake.SparseBakedVolume if prune else bake.BakedVolume)
    for k, l in enumerate(losses):
        tail = float(np.mean(l[-10:]))
        print(f"stage {k} ({'pruned' if prune else 'dense'}): first loss {l[0]:.4e}, mean of the last 10 {tail:.4e}")
        assert tail < l[0], (k, l[0], tail)
