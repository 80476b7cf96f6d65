"""
GPU parity (-m gpu): the backward twin of tests/test_hip_stage_sweep.py.  composite_bwd_kernel (ops.composite_backward: d_rgbsigma,
d_z, d_far, white_bkgd, the reduced call forms, pre_activation) and ray_reduce_kernel in its sampling-only form
(ops.sample_bounds_backward: the coarse map, the merged fine set with clamped depth samples, the d_far pass-through), against fp64
torch autograd on the CPU through the oracle's own functions, over ragged shapes (R not a multiple of the 4 waves per block, K on
both sides of the 64-lane chunk, several chunks with carry, K = 1, near == far; one compositing case of haze past 64 chunks, where
the kernel rebuilds the transmittance at a chunk's head instead of reading it from a lane) and two density families: the forward
sweep's hostile one (lognormal(0, 3), 30 % zeros, 10 % negated, one transparent and one opaque ray) and thin shells (3 consecutive
samples of sigma 50..300, nothing elsewhere).

Inputs are drawn in fp32 and cast up; the kernel gets the same fp32 values.  Error per output tensor: max|got - ref64| / max|ref64|
(d_far: over max(max|d_far ref|, max|d_z ref|)).  Bar per case and tensor: 10 x the error of torch's fp32 autograd through the same
oracle functions on the same inputs, floor 2e-6, cap 2e-5 -- measured against the reference, not against the kernel.  Every case
prints both errors.

Measured on the MI355X (worst over the cases; torch fp32 autograd on the CPU in brackets):
  compositing, hostile   d_rgbsigma 1.9e-7 (1.9e-7)   d_z 2.8e-7 (4.3e-7)   d_far 1.1e-7 (7.9e-8)
  compositing, shell     d_rgbsigma 5.9e-8 (5.9e-8)   d_z 4.1e-7 (8.9e-7)   d_far 7.3e-8 (7.3e-8)
  pre_activation         d_rgbsigma 2.7e-7 (2.1e-7)   d_z 9.1e-7 (5.0e-7)   d_far 2.3e-7 (1.0e-7)
  66 chunks of haze      d_rgbsigma 2.9e-7 (2.9e-7)   d_z 1.5e-7 (2.0e-7)
  sampling maps          coarse 3.5e-7 (1.4e-7), lindisp 5.0e-6 (3.5e-6);  fine set 3.4e-7 (1.4e-7), lindisp 5.5e-6 (3.0e-6)
  (lindisp's worst is near 0.5 / far 50, where dz/dnear = z^2 (1 - s) / near^2 spans four decades over the ray)
The kernel this sweep was written against formed the compositing suffix as total - prefix and divided it by 1 - alpha + 1e-10: the same
run gave d_z 2.3e-4 (hostile, R=64 K=64), 4.0e-4 (pre_activation, R=9 K=65), 1.9e-5 (shell, R=9 K=63), d_rgbsigma 5.4e-6, d_far 1.1e-6, and
NaN near / far gradients on the near == far rays -- 24 of the 92 cases failed.
"""
import numpy as np
import pytest
import torch

import composite_bwd_ref as CR

pytestmark = pytest.mark.gpu

NAMES = ("d_rgbsigma", "d_z", "d_far")
LONG_CASE = (2, 4200, 1.2, 4.0)  # K > 64 * 64: the chunks past the 64th rebuild their head transmittance (composite_bwd_kernel)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


def _hip_composite(ops, dev, inp, white, pre_activation=False, **kw):
    args = dict(d_depth=inp["d_depth"].to(dev), d_weights=inp["d_w"].to(dev), want_dz=True, want_dfar=True)
    args.update(kw)
    out = ops.composite_backward(inp["rays"].to(dev), inp["z"].to(dev), inp["rgbsigma"].to(dev), white, inp["d_rgb"].to(dev),
                                 pre_activation=pre_activation, **args)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (out if isinstance(out, tuple) else (out,)))


def _check_composite(ops, dev, case, family, white, pre_activation=False):
    inp = CR.make_inputs(case, family, pre_activation)
    ref64 = CR.autograd_ref(inp, white, torch.float64, pre_activation)
    assert all(bool(torch.isfinite(r).all()) for r in ref64)
    err32 = CR.errors(CR.autograd_ref(inp, white, torch.float32, pre_activation), ref64)
    got = _hip_composite(ops, dev, inp, white, pre_activation)
    err = CR.errors(got, ref64)
    bars = [CR.bar_from(e) for e in err32]
    for n, e, e32, b in zip(NAMES, err, err32, bars):
        print(f"composite {case} {family} white={white} preact={pre_activation} {n}: HIP {e:.2e} torch-fp32 {e32:.2e} bar {b:.1e}")
    for n, g, e, b in zip(NAMES, got, err, bars):
        assert bool(torch.isfinite(g).all()), n
        assert e <= b, f"{n}: {e:.3e} > {b:.1e}"
    return inp, got


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("family", CR.FAMILIES)
@pytest.mark.parametrize("case", CR.CASES, ids=CR.CASE_IDS)
def test_composite_backward_sweep(ops, dev, case, family, white):
    inp, full = _check_composite(ops, dev, case, family, white)
    if family != "hostile" or not white:
        return
    # the reduced call forms == the same slice of the full call with zeros in place of the None
    zd, zw = torch.zeros_like(inp["d_depth"]).to(dev), torch.zeros_like(inp["d_w"]).to(dev)
    for kw, kw0 in (({"d_depth": None}, {"d_depth": zd}), ({"d_weights": None}, {"d_weights": zw}),
                    ({"d_depth": None, "d_weights": None}, {"d_depth": zd, "d_weights": zw})):
        for n, a, b in zip(NAMES, _hip_composite(ops, dev, inp, white, **kw), _hip_composite(ops, dev, inp, white, **kw0)):
            assert torch.equal(a, b), (n, kw)
    no_dz = _hip_composite(ops, dev, inp, white, want_dz=False)
    assert len(no_dz) == 2 and torch.equal(no_dz[0], full[0]) and torch.equal(no_dz[1], full[2])
    no_far = _hip_composite(ops, dev, inp, white, want_dfar=False)
    assert len(no_far) == 2 and torch.equal(no_far[0], full[0]) and torch.equal(no_far[1], full[1])
    only = _hip_composite(ops, dev, inp, white, want_dz=False, want_dfar=False)
    assert len(only) == 1 and torch.equal(only[0], full[0])


@pytest.mark.parametrize("case", CR.CASES, ids=CR.CASE_IDS)
def test_composite_backward_pre_activation(ops, dev, case):
    """raw rgb ~ N(0, 2^2) and the hostile raw sigma; the kernel receives sigmoid / relu of them, the reference differentiates
    through sigmoid / relu in fp64"""
    _check_composite(ops, dev, case, "hostile", True, pre_activation=True)


@pytest.mark.parametrize("white", [False, True])
def test_composite_backward_past_64_chunks(ops, dev, white):
    """66 chunks of haze (one sample of alpha ~ 0.05 in each, T falls to ~0.04 along the ray): every chunk's head transmittance
    matters, the last two come from the rebuilt product"""
    _check_composite(ops, dev, LONG_CASE, "haze", white)


# ------------------------------------------------------------------------------------------------ sampling maps
def _ray_errors(got, ref64):
    den = float(ref64[:, 6:8].abs().max())
    return float((got[:, 6:8].double() - ref64[:, 6:8]).abs().max()) / den


def _check_near_eq_far(got, dz):
    """s cannot be recovered from z: each sample's dz goes half to near, half to far; dn + df = 1 holds for both maps"""
    assert bool(torch.isfinite(got).all())
    total, scale = dz.double().sum(1), dz.double().abs().sum(1)
    assert bool(((got[:, 6].double() + got[:, 7].double() - total).abs() <= 1e-5 * scale).all())
    for col in (6, 7):
        assert bool(((got[:, col].double() - 0.5 * total).abs() <= 1e-5 * scale).all())


@pytest.mark.parametrize("lindisp", [False, True], ids=["lin", "lindisp"])
@pytest.mark.parametrize("case", CR.CASES, ids=CR.CASE_IDS)
def test_sample_bounds_backward_coarse(ops, dev, case, lindisp):
    R, K, near, far = case
    rs = np.random.RandomState(R * 1000 + K)
    rays = CR.rand_rays(rs, R, near, far)
    u1 = torch.from_numpy(rs.uniform(0, 1, (R, K)).astype(np.float32))
    dz = torch.from_numpy(rs.randn(R, K).astype(np.float32))
    d_far = torch.from_numpy(rs.randn(R).astype(np.float32))
    z64, ref64 = CR.coarse_map_ref(rays, u1, dz, K, lindisp, torch.float64)
    assert bool(torch.isfinite(ref64).all())
    z = z64.float()
    got = ops.sample_bounds_backward(rays.to(dev), z.to(dev), dz.to(dev), lindisp).cpu()
    got_far = ops.sample_bounds_backward(rays.to(dev), z.to(dev), dz.to(dev), lindisp, d_far=d_far.to(dev)).cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_far).all())
    assert bool((got[:, :6] == 0).all()) and bool((got_far[:, :6] == 0).all())
    # d_far is added to column 7 unchanged (one fp32 addition in front of the sum)
    assert torch.equal(got_far[:, 6], got[:, 6])
    if near == far:
        _check_near_eq_far(got, dz)
        _check_near_eq_far(got_far - torch.nn.functional.pad(d_far[:, None], (7, 0)), dz)
        return
    _, ref32 = CR.coarse_map_ref(rays, u1, dz, K, lindisp, torch.float32)
    ref_far = ref64.clone()
    ref_far[:, 7] += d_far.double()
    err32, err, err_far = _ray_errors(ref32, ref64), _ray_errors(got, ref64), _ray_errors(got_far, ref_far)
    bar = CR.bar_from(err32)
    print(f"coarse map {case} lindisp={lindisp}: HIP {err:.2e} (+d_far {err_far:.2e}) torch-fp32 {err32:.2e} bar {bar:.1e}")
    assert err <= bar and err_far <= bar, (err, err_far, bar)


KIMP, KFD = 5, 6


@pytest.mark.parametrize("lindisp", [False, True], ids=["lin", "lindisp"])
@pytest.mark.parametrize("case", CR.CASES, ids=CR.CASE_IDS)
def test_sample_bounds_backward_fine(ops, dev, case, lindisp):
    """Kc = the case's K coarse samples, 5 importance samples, 6 depth samples around a depth_c that alternates over the rays
    between near + 0.005, far - 0.005 and mid-span (std 0.01): per ray some clamp at near or far (column 0 is made to) and some stay
    inside (column 1 is made to); |zraw - bound| > 1e-4 so that no tie decides a case.  The set is built and sorted in fp64, the kernel
    gets that z cast to fp32 and the ranks of the fp64 sort: both sides differentiate the same sample set.  near == far runs without
    depth samples (clamped to both bounds at once, a tie by construction) and asserts the half / half split."""
    R, Kc, near, far = case
    Kfd = 0 if near == far else KFD
    rs = np.random.RandomState(R * 1000 + Kc + 1)
    rays = CR.rand_rays(rs, R, near, far)
    u1, u2, u3 = (torch.from_numpy(rs.uniform(0, 1, (R, k)).astype(np.float32)) for k in (Kc, KIMP, KIMP))
    weights = torch.from_numpy(rs.uniform(0.01, 1.0, (R, Kc)).astype(np.float32))
    n4 = rs.randn(R, KFD).astype(np.float32)
    kind = np.arange(R) % 3
    depth_c = np.where(kind == 0, near + 0.005, np.where(kind == 1, far - 0.005, 0.5 * (near + far))).astype(np.float32)
    n4[:, 0] = np.where(kind == 0, -1.5, np.where(kind == 1, 1.5, n4[:, 0]))
    n4[:, 1] = np.where(kind == 0, 0.2, np.where(kind == 1, -0.2, n4[:, 1]))
    zraw = depth_c[:, None].astype(np.float64) + n4.astype(np.float64) * 0.01
    for bound in (near, far):  # push the draws within 1e-4 of a bound 3e-4 further out
        close = np.abs(zraw - bound) <= 1e-4
        n4[close] += np.where(zraw[close] >= bound, 0.03, -0.03).astype(np.float32)
    n4, depth_c = torch.from_numpy(n4), torch.from_numpy(depth_c)
    K = Kc + KIMP + Kfd
    dz = torch.from_numpy(rs.randn(R, K).astype(np.float32))
    d_far = torch.from_numpy(rs.randn(R).astype(np.float32))

    z64, perm, ref64 = CR.fine_map_ref(rays, u1, weights, u2, u3, n4, depth_c, dz, Kc, Kfd, lindisp, torch.float64)
    assert bool(torch.isfinite(ref64).all())
    kw = {}
    if Kfd:
        zr = depth_c.double()[:, None] + n4.double() * 0.01
        assert float((zr - near).abs().min()) > 1e-4 and float((zr - far).abs().min()) > 1e-4
        lo, hi = (zr < near).sum(1), (zr > far).sum(1)
        assert bool(((lo + hi > 0) | (torch.from_numpy(kind) == 2)).all()) and bool((lo + hi < Kfd).all())
        assert R < 2 or (int(lo.sum()) > 0 and int(hi.sum()) > 0)
        ranks = torch.argsort(perm, dim=-1)[:, Kc + KIMP:].to(torch.int32).contiguous()  # sorted positions of the depth samples
        kw = dict(ranks=ranks.to(dev), n4=n4.to(dev), depth_c=depth_c.to(dev), depth_std=0.01)
    z = z64.float()
    got = ops.sample_bounds_backward(rays.to(dev), z.to(dev), dz.to(dev), lindisp, d_far=d_far.to(dev), **kw).cpu()
    assert bool(torch.isfinite(got).all())
    assert bool((got[:, :6] == 0).all())
    if near == far:
        _check_near_eq_far(got - torch.nn.functional.pad(d_far[:, None], (7, 0)), dz)
        return
    _, _, ref32 = CR.fine_map_ref(rays, u1, weights, u2, u3, n4, depth_c, dz, Kc, Kfd, lindisp, torch.float32, perm=perm)
    ref_far = ref64.clone()
    ref_far[:, 7] += d_far.double()
    err32, err = _ray_errors(ref32, ref64), _ray_errors(got, ref_far)
    bar = CR.bar_from(err32)
    print(f"fine set {case} lindisp={lindisp}: HIP {err:.2e} torch-fp32 {err32:.2e} bar {bar:.1e}")
    assert err <= bar, (err, bar)
