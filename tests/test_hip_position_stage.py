"""
GPU stage test (-m gpu) of the third backward block, the geometry chain sample -> world point -> rotated point -> positional code /
projection / bilinear lookup: point_grad (pnr_geom.h), position_bwd_kernel (ops.position_backward, ops.depth_sample_backward),
camera_record_kernel, ray_reduce_kernel in its full form, cam_partial_kernel and cam_final_kernel (ops.camera_backward), and the
latent scatter on the same inputs (ops.latent_scatter: slab, tiled, and -- in a child process, because the form is read from the
environment once per process -- the global-atomic fallback).  The kernels are fed their upstream gradients directly and held to
fp64 torch autograd through tests/position_ref.py.

The bilinear derivative jumps at cell edges and at the border clip; rows within 1e-3 texel of a jump get a zero d_zlat row
(position_ref.edge_mask), so their lookup term is zero whichever cell is differentiated and every other term is smooth.  Error per
tensor: max|got - ref64| / max|ref64|.  Bar per case and tensor: 10 x the error of torch's fp32 autograd through the same chain on
the same inputs, floor 2e-6, cap 2e-4 -- measured against the reference, never against the kernel
(tests/test_position_ref_host.py holds every case's torch-fp32 error below 2e-5, so no bar reaches the cap).  Every test prints
the HIP error, the torch-fp32 error and the bar.

Measured on the MI355X (worst over the cases; torch fp32 autograd on the CPU in brackets):
  position_backward   d_z onto a buffer 3.9e-6 (3.5e-6)   through d_in42 alone 7.5e-6 (9.5e-6)   through d_zlat alone 3.9e-6 (3.4e-6)
  camera_backward     d_rays[:, :6] 1.6e-6 (1.5e-6)   d_poses 2.5e-6 (2.1e-6)   d_focal 2.4e-6 (5.0e-6)   d_c 1.5e-6 (9.0e-7)
                      d_rays[:, 6:8] 2.2e-6 (2.8e-6), lindisp 4.5e-6 (2.1e-6), the same with and without dz_comp / d_far
  depth samples       contrib 1.3e-6 (1.4e-6)   d_rays[:, 6:8] with ranks 7.2e-7 (8.5e-7)   partition 1.0e-6 (1.6e-6)
  dropped records     d_z 3.4e-7 (3.7e-7)   d_rays 1.8e-7 (3.7e-7)   d_poses 4.3e-7 (5.9e-7)   d_focal 5.6e-7 (1.4e-6)   d_c 1.9e-7 (1.0e-6)
  latent scatter      slab 2.2e-6 (2.2e-6)   tiled 3.0e-6 (3.0e-6)   global atomics 3.3e-6 (3.3e-6)
  (the bracket is the torch-fp32 figure of the case with the worst HIP error; the bars were 2e-6 .. 9.5e-5)
position_bwd_kernel used to test its dL/dz with `val == val` only: in test_dropped_records the +inf of d_in42 then reached d_z as an
infinity (d_z: finite False; every pnr_camera_backward output finite).  It takes camera_record_kernel's rule now, __builtin_isfinite.
What the bars catch, from libraries broken on purpose outside the tree: cam_final_kernel summing a per-object intrinsics row from
object 0 -- d_focal 1.0 in mv_mini_24x96_rows, all of tests/test_hip_camera_grad.py still passing (its scenes share one focal / c
row); cam_partial_kernel dropping the last sample of each object -- d_poses 5.4e-3 .. 2.4e-1 in all eight cases, 11 of the 12
end-to-end cases still passing (mv_mini_lindisp f32: c 6.6e-3 against 5e-3).  Coarser damage -- the whole last CAM_CHUNK partial
skipped (d_poses 3.2e-2 .. 4.2e-1 in the five cases with two chunks), code band k = 5 dropped in point_grad (d_z, d_rays
1.3e-1 .. 5.8e-1) -- fails the end-to-end test as well.
"""
import os
import subprocess
import sys

import pytest
import torch

import position_ref as PR

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
CASE_BY_NAME = {c.name: c for c in PR.CASES}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


def _device_inputs(ops, dev, inp):
    sc = ops.make_scene(inp["latent"].to(dev), inp["poses"].to(dev), inp["focal"].to(dev), inp["c"].to(dev), inp["image_shape"],
                        inp["NS"])
    return sc, inp["rays"].to(dev), inp["z"].to(dev), inp["g_in"].to(dev), inp["g_z"].to(dev)


def _report(what, name, err, err32):
    """print HIP error, torch-fp32 error and bar of one tensor, then hold the error to the bar"""
    bar = PR.bar_from(err32)
    print(f"{what} {name}: HIP {err:.2e} torch-fp32 {err32:.2e} bar {bar:.1e}")
    assert err <= bar, f"{what} {name}: {err:.3e} > {bar:.1e}"


def _seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ pnr_position_backward
@pytest.mark.parametrize("case", PR.CASES, ids=PR.CASE_IDS)
def test_position_backward(ops, dev, case):
    """d_z is accumulated: from a non-zero buffer the result is buffer + reference; then each upstream half alone"""
    inp, ref64, ref32 = PR.reference(case)
    sc, rays, z, g_in, g_z = _device_inputs(ops, dev, inp)
    buf = _seeded((inp["R"], inp["K"]), 31)
    got = ops.position_backward(sc, rays, z, g_in, g_z, buf.to(dev).clone()).cpu()
    assert bool(torch.isfinite(got).all())
    den = float(ref64["z"].abs().max())
    err = float((got.double() - (buf.double() + ref64["z"])).abs().max()) / den
    _report(f"position {case.name}", "d_z (buffer + reference)", err, PR.error(ref32["z"], ref64["z"]))
    halves64, halves32 = PR.gradients(inp, F64, halves=True), PR.gradients(inp, F32, halves=True)
    for which, (a, b) in enumerate(((g_in, torch.zeros_like(g_z)), (torch.zeros_like(g_in), g_z))):
        got = ops.position_backward(sc, rays, z, a, b, torch.zeros(inp["R"], inp["K"], device=dev)).cpu()
        _report(f"position {case.name}", "d_z through " + ("d_in42 alone" if which == 0 else "d_zlat alone"),
                PR.error(got, halves64[which]["z"]), PR.error(halves32[which]["z"], halves64[which]["z"]))


# ------------------------------------------------------------------------------------------------ pnr_camera_backward
def _camera(ops, sc, rays, z, g_in, g_z, **kw):
    out = ops.camera_backward(sc, rays, z, g_in, g_z, **kw)
    torch.cuda.synchronize()
    return dict(zip(("rays", "poses", "focal", "c"), (None if t is None else t.cpu() for t in out)))


@pytest.mark.parametrize("case", PR.CASES, ids=PR.CASE_IDS)
def test_camera_backward(ops, dev, case):
    inp, ref64, ref32 = PR.reference(case)
    sc, rays, z, g_in, g_z = _device_inputs(ops, dev, inp)
    R, K = inp["R"], inp["K"]
    dz_comp, d_far = _seeded((R, K), 41), _seeded((R,), 42)
    what = f"camera {case.name}"
    full = _camera(ops, sc, rays, z, g_in, g_z, dz_comp=dz_comp.to(dev), d_far=d_far.to(dev))
    for t in full.values():
        assert bool(torch.isfinite(t).all())
    # origin and direction; the cameras
    _report(what, "d_rays[:, :6]", PR.error(full["rays"][:, :6], ref64["rays"]), PR.error(ref32["rays"], ref64["rays"]))
    for name in ("poses", "focal", "c"):
        assert full[name].shape == inp[name].shape
        _report(what, "d_" + name, PR.error(full[name], ref64[name]), PR.error(ref32[name], ref64[name]))
    # near / far: dL/dz (network term over all views + dz_comp) through the sampling map, d_far added to far
    for lindisp in (False, True):
        for given in (True, False):
            kw = dict(dz_comp=dz_comp.to(dev), d_far=d_far.to(dev)) if given else {}
            got = full if (given and not lindisp) else _camera(ops, sc, rays, z, g_in, g_z, lindisp=lindisp, **kw)
            comp = dz_comp if given else torch.zeros(R, K)
            nf64 = PR.near_far(inp, ref64["z"] + comp.double(), lindisp, F64, d_far if given else None)
            nf32 = PR.near_far(inp, ref32["z"] + comp, lindisp, F32, d_far if given else None)
            assert torch.equal(got["rays"][:, :6], full["rays"][:, :6])
            _report(what, f"d_rays[:, 6:8] lindisp={lindisp} dz_comp/d_far {'given' if given else 'not given'}",
                    PR.error(got["rays"][:, 6:8], nf64), PR.error(nf32, nf64))
    # every want_* subset == the same tensors of the full call, bit for bit; so is a second full call
    names = ("rays", "poses", "focal", "c")
    for bits in range(1, 16):
        want = {n: bool(bits >> i & 1) for i, n in enumerate(names)}
        sub = _camera(ops, sc, rays, z, g_in, g_z, dz_comp=dz_comp.to(dev), d_far=d_far.to(dev),
                      **{"want_" + n: w for n, w in want.items()})
        for n in names:
            assert (sub[n] is None) == (not want[n]), (n, want)
            if want[n]:
                assert torch.equal(sub[n], full[n]), (n, want)


# ------------------------------------------------------------------------------------------------ depth samples
KIMP, KFD, DEPTH_STD = 8, 8, 0.5


def _depth_setup(ops, dev):
    """the merged fine set of PR.DEPTH_CASE from ops.sample_fine: 32 coarse + 8 importance + 8 depth samples.  The seeded coarse
    weights are a bump around the first / the last / the middle bin in turn over the rays, so the coarse depth sum w z lies near
    `near`, near `far` or mid-span, and with depth_std = 0.5 each clamp state holds for a good share of the depth samples."""
    base = PR.make_inputs(PR.DEPTH_CASE)
    R, Kc = base["R"], base["K"]
    gen = torch.Generator().manual_seed(55)
    centre = torch.tensor([0.0, Kc - 1.0, Kc / 2.0])[torch.arange(R) % 3]
    w = torch.exp(-0.5 * (torch.arange(Kc, dtype=F32)[None] - centre[:, None]) ** 2)
    w = w / w.sum(1, keepdim=True)
    depth_c = (w * base["z"]).sum(1)
    u2, u3, n4 = torch.rand(R, KIMP, generator=gen), torch.rand(R, KIMP, generator=gen), torch.randn(R, KFD, generator=gen)
    z_all, ranks = ops.sample_fine(base["rays"].to(dev), w.to(dev), depth_c.to(dev), base["z"].to(dev), u2.to(dev), u3.to(dev),
                                   n4.to(dev), depth_std=DEPTH_STD, want_ranks=True)
    inp = PR.with_samples(base, z_all.cpu(), gen)
    return inp, (ranks.cpu(), n4, depth_c, DEPTH_STD)


def test_depth_samples(ops, dev):
    """pnr_depth_sample_backward's contrib against the header's formula, dz_comp entering at view 0 only, and the partition: the
    dL/dz of a depth sample reaches the coarse depth (live), near or far (clamped) -- exactly one of them"""
    inp, depth = _depth_setup(ops, dev)
    ranks, n4, depth_c, std = depth
    R, K, NS = inp["R"], inp["K"], inp["NS"]
    assert K == 32 + KIMP + KFD and ranks.shape == (R, KFD)
    zd = torch.gather(inp["z"], 1, ranks.long())  # the depth samples sit where ranks says: the clamped z = clamp(depth_c + n4 std)
    near, far = inp["rays"][:, 6:7], inp["rays"][:, 7:8]
    assert torch.allclose(zd, torch.max(torch.min(depth_c[:, None] + n4 * std, far), near), rtol=0, atol=1e-6)
    zraw = depth_c.double()[:, None] + n4.double() * std
    assert float(torch.minimum((zraw - near).abs(), (zraw - far).abs()).min()) > 1e-5  # no tie decides a clamp state
    state = PR.clamp_state(inp["rays"], n4, depth_c, std)
    shares = [float((state == s).double().mean()) for s in (-1, 0, 1)]
    print(f"depth samples: below near {100 * shares[0]:.0f} % live {100 * shares[1]:.0f} % above far {100 * shares[2]:.0f} %; "
          f"masked rows {100 * inp['stats']['masked']:.2f} %")
    assert min(shares) >= 0.10 and inp["stats"]["masked"] <= 0.01

    ref64, ref32 = PR.gradients(inp, F64), PR.gradients(inp, F32)
    assert all(e <= 2e-5 for e in PR.errors(ref32, ref64).values())
    sc, rays, z, g_in, g_z = _device_inputs(ops, dev, inp)
    dz_comp, d_far = _seeded((R, K), 43), _seeded((R,), 44)
    dkw = dict(ranks=ranks.to(dev), n4=n4.to(dev), depth_c=depth_c.to(dev), depth_std=std)
    for comp in (dz_comp, None):
        got = ops.depth_sample_backward(sc, rays, z, dkw["ranks"], dkw["n4"], dkw["depth_c"], std, g_in, g_z,
                                        None if comp is None else comp.to(dev), want_contrib=True).cpu()
        assert got.shape == (NS, R, KFD) and bool(torch.isfinite(got).all())
        c64 = PR.depth_contrib(inp, ref64["z_views"], None if comp is None else comp.double(), depth)
        c32 = PR.depth_contrib(inp, ref32["z_views"], comp, depth)
        _report("depth samples", f"contrib, dz_comp {'given' if comp is not None else 'not given'}", PR.error(got, c64),
                PR.error(c32, c64))
        assert not bool(got[:, state != 0].any())  # a clamped sample sends nothing to the coarse depth, exactly
        if comp is not None:
            contrib = got
    # the clamped ones reach near / far whole (pnr_camera_backward with the same ranks), the others' map is untouched
    cam = _camera(ops, sc, rays, z, g_in, g_z, dz_comp=dz_comp.to(dev), d_far=d_far.to(dev), want_poses=False, want_focal=False,
                  want_c=False, **dkw)["rays"]
    dz64, dz32 = ref64["z"] + dz_comp.double(), ref32["z"] + dz_comp
    nf64, nf32 = PR.near_far(inp, dz64, False, F64, d_far, depth), PR.near_far(inp, dz32, False, F32, d_far, depth)
    err32 = PR.error(nf32, nf64)
    _report("depth samples", "d_rays[:, 6:8] with ranks", PR.error(cam[:, 6:8], nf64), err32)
    # partition (lindisp off: dn + df = 1 on every other sample): d near + d far + sum contrib = sum_k dz + d_far, per ray
    total = cam[:, 6].double() + cam[:, 7].double() + contrib.double().sum(dim=(0, 2))
    want = dz64.sum(1) + d_far.double()
    err = float((total - want).abs().max()) / float(nf64.abs().max())
    ref_total = nf32[:, 0].double() + nf32[:, 1].double() + PR.depth_contrib(inp, ref32["z_views"], dz_comp, depth).double().sum(dim=(0, 2))
    _report("depth samples", "partition: d near + d far + sum contrib vs sum dz", err,
            float((ref_total - want).abs().max()) / float(nf64.abs().max()))


# ------------------------------------------------------------------------------------------------ dropped records
def test_dropped_records(ops, dev):
    """a sample on a source camera's plane, a +inf row and a NaN row of d_in42: both kernels drop the record -- every output is
    finite and equals the reference with those samples' contributions removed"""
    inp, z_views, dropped = PR.hostile_inputs()
    ref64 = PR.reference_without(inp, z_views, dropped, F64)
    ref32 = PR.reference_without(inp, z_views, dropped, F32)
    assert all(bool(torch.isfinite(t).all()) for t in ref64.values())
    sc, rays, z, g_in, g_z = _device_inputs(ops, dev, inp)
    R, K = inp["R"], inp["K"]
    got = {"z": ops.position_backward(sc, rays, z, g_in, g_z, torch.zeros(R, K, device=dev)).cpu()}
    cam = _camera(ops, sc, rays, z, g_in, g_z)
    got.update(rays=cam["rays"][:, :6], poses=cam["poses"], focal=cam["focal"], c=cam["c"])
    got["near / far"] = cam["rays"][:, 6:8]
    ref64["near / far"], ref32["near / far"] = PR.near_far(inp, ref64["z"], False, F64), PR.near_far(inp, ref32["z"], False, F32)
    for name, g in got.items():
        print(f"dropped records d_{name}: finite {bool(torch.isfinite(g).all())}")
    for name, g in got.items():
        assert bool(torch.isfinite(g).all()), name
        _report("dropped records", "d_" + name, PR.error(g, ref64[name]), PR.error(ref32[name], ref64[name]))
    # the depth-sample form takes the same rule: the three samples as "depth samples" of their rays
    P = R * K
    ranks = torch.zeros(R, 1, dtype=torch.int32)
    for row in dropped:
        ranks[(row % P) // K, 0] = (row % P) % K
    depth_c = torch.gather(inp["z"], 1, ranks.long())[:, 0].contiguous()
    contrib = ops.depth_sample_backward(sc, rays, z, ranks.to(dev), torch.zeros(R, 1, device=dev), depth_c.to(dev), 0.01, g_in, g_z,
                                        None, want_contrib=True).cpu()
    assert bool(torch.isfinite(contrib).all())
    c64 = PR.depth_contrib(inp, ref64["z_views"], None, (ranks, torch.zeros(R, 1), depth_c, 0.01))
    c32 = PR.depth_contrib(inp, ref32["z_views"], None, (ranks, torch.zeros(R, 1), depth_c, 0.01))
    _report("dropped records", "contrib", PR.error(contrib, c64), PR.error(c32, c64))


# ------------------------------------------------------------------------------------------------ latent scatter
@pytest.mark.parametrize("case", [CASE_BY_NAME["mv_mini_24x96"], CASE_BY_NAME["dtu_mini_64x24"], PR.GRID_CASE], ids=lambda c: c.name)
def test_latent_scatter(ops, dev, case):
    """ops.latent_scatter with d_zlat = g_z against the reference's d_latent: the slab form (16 x 16, 15 x 20) and the tiled form
    (72 x 80)"""
    inp, ref64, ref32 = PR.reference(case)
    sc, rays, z, _, g_z = _device_inputs(ops, dev, inp)
    assert ops.latent_scatter_single_owner(sc, inp["R"], inp["K"]) == (case.grid is not None)
    NV, _, Hl, Wl = inp["latent"].shape
    out = ops.latent_scatter(sc, rays, z, g_z, torch.zeros(NV, Hl, Wl, 512, device=dev))
    got = out.permute(0, 3, 1, 2).cpu()
    assert bool(torch.isfinite(got).all())
    _report(f"latent scatter {case.name}", "d_latent", PR.error(got, ref64["latent"]), PR.error(ref32["latent"], ref64["latent"]))


def test_latent_scatter_atomic_fallback():
    """latent_scatter_kernel (global fp32 atomics) runs on a large grid only with PIXELNERF_SCATTER_TILED=0, which is read once per
    process: a fresh child process runs PR.CHILD_CASE (72 x 80, SB = 1, NS = 2, P = 207), asserts the form and applies the bar"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "position_scatter_child.py")
    env = dict(os.environ, PIXELNERF_SCATTER_TILED="0")
    res = subprocess.run([sys.executable, child], env=env, timeout=120, capture_output=True, text=True)
    print(res.stdout + res.stderr)
    assert res.returncode >= 0, f"the child died from signal {-res.returncode}"
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "latent scatter (atomic)" in res.stdout
