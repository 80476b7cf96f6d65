"""GPU tests (-m gpu) of the visibility of a baked volume: pnr_baked_visibility_rays / _views through ops.baked_visibility /
ops.baked_visibility_views and the `visibility` methods of the volume classes.

The yardstick is tests/baked_visibility_ref.py -- baked_grad_ref.march's samples and weights, the maximum per grid point -- in fp64
(its own checks, and the input conditions of these cases: tests/test_baked_visibility_host.py).  Error and bar are the project's
for march quantities: error = max|got - ref64| / max|ref64|, bar = 10 x the error of the fp32 restatement (floor 2e-6, cap 2e-4).
Everything else here is BYTES: a maximum does not depend on order."""
import numpy as np
import pytest
import torch

import baked_ray_grad_ref as RG
import baked_visibility_ref as V
import sparse_baked_ref as SP
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


@pytest.fixture(scope="module")
def bake():
    from pixelnerf_amd.util import bake as _bake
    return _bake


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bits(cells, dev):
    return None if cells is None else torch.from_numpy(SP.bits_from_cells(cells).copy()).to(dev)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _vis(ops, dev, case, rays=None, stored=None, out=None, **kw):
    """ops.baked_visibility on the inputs of a case (rays / stored: others in place of the case's)"""
    inp = V.inputs(case)
    stored = _t(inp["stored"], dev) if stored is None else stored
    rays = inp["rays"] if rays is None else rays
    args = dict(bits=_bits(inp["occupied"], dev), terminate=case.terminate, out=out)
    args.update(kw)
    return ops.baked_visibility(_t(rays, dev), stored, case.kind, V.RESO, V.C1, V.C2, V.STEP, **args)


def _sparse_parts(dev, case):
    """-> (rows, index, ids, kept) of the case's volume under the case's cells"""
    inp = V.inputs(case)
    index, ids = SP.sparse_points(inp["occupied"])
    flat = inp["stored"].reshape((-1,) + inp["stored"].shape[3:])
    return _t(flat[ids], dev), _t(index, dev), ids, SP.kept_points(inp["occupied"])


# ---------------------------------------------------------------- 1. against the fp64 restatement
@pytest.mark.parametrize("name", V.CASE_IDS)
def test_visibility_of_every_case_is_within_its_bar(dev, ops, name):
    """RGBA and degree 0, 1, 2, with and without bits, with and without terminate (the restatement stops where the forward stops);
    150-sample rays (three chunks) next to 60-sample ones; rays that miss, a ray with near >= far"""
    case = V.BY_NAME[name]
    inp, v64, v32, info = V.reference(case)
    got = _vis(ops, dev, case)
    assert got.shape == V.RESO and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    err, err32 = V.error(got.cpu(), v64), V.error(v32.double(), v64)
    bar = V.bar_from(err32)
    seen = float((got > 0).float().mean())
    print(f"{name}: HIP error {err:.3e}, fp32-restatement error {err32:.3e}, bar {bar:.3e}, ratio {err / max(err32, 1e-30):.2f}; seen {seen:.3f}")
    assert seen >= 0.25 and int((info["chunks"] >= 2).sum()) >= 1 and (not case.terminate or int(info["stopped"].sum()) >= 1)
    assert err <= bar, (name, err, bar)
    assert float(got.min()) >= 0.0
    # exactly 0 at the points no walked active sample's cell touches, in either precision of the restatement
    touched32 = {}
    V.visibility(inp["rays"], inp["stored"], V.C1, V.C2, V.STEP, dtype=torch.float32, info=touched32, **inp["kw"])
    untouched = ~(info["touched"] | touched32["touched"])
    assert bool(untouched.any()) and not bool(got.cpu()[untouched].any())


@pytest.mark.parametrize("name", ["rgba_terminate", "sh2_bits_terminate"])
def test_terminate_stops_where_the_forward_stops(dev, ops, name):
    """the field with terminate is the restatement's with the stop, and -- RGBA -- differs from the field without"""
    case = V.BY_NAME[name]
    _, v64, v32, _ = V.reference(case)
    got, free = _vis(ops, dev, case), _vis(ops, dev, case, terminate=0.0)
    assert V.error(got.cpu(), v64) <= V.bar_from(V.error(v32.double(), v64))
    assert bool((free >= got).all()) and (case.kind is not None or not torch.equal(free, got))


# ---------------------------------------------------------------- 2. bytes
@pytest.mark.parametrize("name", ["rgba", "sh1_bits", "sh2_bits_terminate"])
def test_bytes_equal_on_two_calls_under_permutation_and_in_three_batches(dev, ops, name):
    """maximum is commutative and associative exactly: no order of the rays and no split into accumulating calls changes a bit"""
    case = V.BY_NAME[name]
    rays = V.inputs(case)["rays"]
    first = _vis(ops, dev, case)
    assert bool(first.any()) and _same(_vis(ops, dev, case), first)
    perm = np.random.RandomState(5).permutation(rays.shape[0])
    assert _same(_vis(ops, dev, case, rays=rays[perm]), first)
    acc = torch.zeros(V.RESO, device=dev)
    for part in np.array_split(perm, 3):
        assert _vis(ops, dev, case, rays=rays[part], out=acc) is acc
    assert _same(acc, first)


def test_64_copies_of_one_ray_give_the_bytes_of_the_one(dev, ops):
    case = V.BY_NAME["rgba"]
    copies = V.contention_rays(case)
    one = _vis(ops, dev, case, rays=copies[:1])
    assert bool(one.any()) and _same(_vis(ops, dev, case, rays=copies), one)


@pytest.mark.parametrize("name", V.SPARSE_CASES)
def test_sparse_is_the_dense_with_bits_at_ids_and_dense_is_zero_off_ids(dev, ops, name):
    case = V.BY_NAME[name]
    inp = V.inputs(case)
    rows, index, ids, kept = _sparse_parts(dev, case)
    dense = _vis(ops, dev, case)
    sparse = ops.baked_visibility(_t(inp["rays"], dev), rows, case.kind, V.RESO, V.C1, V.C2, V.STEP, bits=_bits(inp["occupied"], dev),
                                  index=index, terminate=case.terminate)
    assert sparse.shape == (len(ids),) and bool(sparse.any())
    assert _same(sparse, dense.reshape(-1)[torch.from_numpy(ids.astype(np.int64)).to(dev)])
    assert not bool(dense.cpu()[~torch.from_numpy(kept)].any())


@pytest.mark.parametrize("name,sparse", [("rgba_bits", False), ("rgba_bits", True), ("sh2", False), ("sh2_bits_terminate", True)])
def test_half_volume_gives_the_bytes_of_its_widened_volume(dev, ops, name, sparse):
    case = V.BY_NAME[name]
    inp = V.inputs(case)
    if sparse:
        rows, index, _, _ = _sparse_parts(dev, case)
        half, kw = rows.half(), dict(index=index)
    else:
        half, kw = _t(inp["stored"], dev).half(), {}
    a = _vis(ops, dev, case, stored=half, **kw)
    b = _vis(ops, dev, case, stored=half.float(), **kw)
    assert bool(a.any()) and _same(a, b)


@pytest.mark.parametrize("name", ["rgba", "sh2"])
def test_views_form_gives_the_bytes_of_the_rays_form_on_gen_rays(dev, ops, name):
    from pixelnerf_amd import util
    case = V.BY_NAME[name]
    stored = _t(V.inputs(case)["stored"], dev)
    poses = torch.stack([synthetic.pose_spherical(*a) for a in RG.VIEW_ANGLES]).float().to(dev)
    v = RG.VIEWS
    W, H, focal, z_near, z_far = (v[k] for k in ("W", "H", "focal", "z_near", "z_far"))
    rays = util.gen_rays(poses, W, H, focal, z_near, z_far).reshape(-1, 8)
    by_rays = ops.baked_visibility(rays, stored, case.kind, V.RESO, V.C1, V.C2, V.STEP)
    by_views = ops.baked_visibility_views(poses, W, H, focal, None, z_near, z_far, stored, case.kind, V.RESO, V.C1, V.C2, V.STEP)
    assert bool(by_rays.any()) and _same(by_views, by_rays)


# ---------------------------------------------------------------- 3. the volume classes
def test_volume_methods_accumulate_and_match_the_ops(dev, ops, bake):
    case = V.BY_NAME["rgba"]
    inp = V.inputs(case)
    vol = bake.BakedVolume(_t(inp["stored"], dev), V.C1, V.C2)
    rays = _t(inp["rays"], dev)
    whole = vol.visibility(rays, step=V.STEP, skip=False)
    assert _same(whole, _vis(ops, dev, case))
    assert _same(vol.visibility(rays, step=V.STEP, skip=True), whole)                  # the skip grid at threshold 0 is exact
    acc = vol.visibility(rays[:30], step=V.STEP)
    assert vol.visibility(rays[30:].reshape(2, -1, 8), step=V.STEP, out=acc) is acc and _same(acc, whole)
    sparse = vol.sparse()
    vs = sparse.visibility(rays, step=V.STEP)
    assert vs.shape == (sparse.n_rows,) and _same(vs, whole.reshape(-1)[sparse.ids.long()])
    assert _same(vol.half().visibility(rays, step=V.STEP), vol.half().float().visibility(rays, step=V.STEP))
    with pytest.raises(ValueError, match="skip=False is not available"):
        sparse.visibility(rays, step=V.STEP, skip=False)
    sh = bake.BakedSHVolume(_t(V.inputs(V.BY_NAME["sh1_bits"])["stored"], dev), V.C1, V.C2)
    assert sh.visibility(rays, step=V.STEP).shape == V.RESO
