"""GPU tests (-m gpu) of the on-device structural similarity (pnr_ssim / ops.ssim / ops.eval_epilogue(image_shape=) / util.ssim)
against the numpy fp64 restatement of tests/ssim_ref.py (itself checked against scipy's filter route in tests/test_ssim_host.py).

Tolerance 1e-10 absolute per view: both sides evaluate the same formula in fp64 and differ only in the order of the window sums and
of the mean (a few 1e-14 between two host orders on these very cases); the identical pair must give exactly 1.0, a batch must equal
its single-view calls bit for bit, and two runs must agree bit for bit (fixed-order reduction, no atomics)."""
import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_ssim_matches_the_restatement(ops, dev, name):
    pred, gt = R.cases()[name]
    got = ops.ssim(_t(pred, dev), _t(gt, dev))
    assert got.shape == (1,) and got.dtype == torch.float64 and got.is_cuda
    ref = R.ssim_ref(pred, gt)
    err = abs(float(got[0]) - ref)
    print(f"ssim {name}: device {float(got[0]):.15f}  restatement {ref:.15f}  |diff| {err:.2e}")
    assert err <= BAR
    if name.startswith("identical"):
        assert float(got[0]) == 1.0
    if name.startswith("noise"):
        assert abs(float(got[0])) < 0.05


@pytest.mark.parametrize("size", [(64, 64), (9, 23)])
def test_a_batch_equals_its_single_view_calls_and_runs_repeat(ops, dev, size):
    H, W = size
    pairs = [R.disc_pair(H, W, 500 + v) for v in range(23)]
    pred, gt = _t(np.stack([p for p, _ in pairs]), dev), _t(np.stack([g for _, g in pairs]), dev)
    batch = ops.ssim(pred, gt)
    assert batch.shape == (23,)
    single = torch.cat([ops.ssim(pred[v], gt[v]) for v in range(23)])
    assert torch.equal(batch, single)                       # a view's value does not depend on the launch it shares
    assert torch.equal(ops.ssim(pred, gt), batch)           # bit-identical from run to run
    ref = R.ssim_ref_batch(pred.cpu().numpy(), gt.cpu().numpy())
    assert np.abs(batch.cpu().numpy() - ref).max() <= BAR


@pytest.mark.parametrize("win", [3, 11])
@pytest.mark.parametrize("channels", [1, 3])
def test_window_sizes_channels_and_data_range(ops, dev, win, channels):
    pred, gt = R.disc_pair(40, 52, 31 + win, channels=channels)
    ref = R.ssim_ref(pred, gt, win_size=win)
    got = float(ops.ssim(_t(pred, dev), _t(gt, dev), win_size=win)[0])
    print(f"ssim win {win} channels {channels}: |diff| {abs(got - ref):.2e}")
    assert abs(got - ref) <= BAR
    # doubled images at data_range 2 (exact in fp32): C1, C2 and every moment scale together
    twice = float(ops.ssim(_t(pred * 2.0, dev), _t(gt * 2.0, dev), win_size=win, data_range=2.0)[0])
    assert abs(twice - got) <= BAR and abs(twice - R.ssim_ref(pred * 2.0, gt * 2.0, win, 2.0)) <= BAR
    with pytest.raises(ops._lib.PixelNerfHipError, match="win_size"):
        ops.ssim(_t(pred, dev), _t(gt, dev), win_size=4)


def test_eval_epilogue_adds_ssim_of_the_clamped_image(ops, dev):
    H, W, NV = 30, 44, 3
    rs = np.random.RandomState(12)
    pairs = [R.disc_pair(H, W, 40 + v) for v in range(NV)]
    gt = np.stack([g for _, g in pairs])
    pred = (np.stack([p for p, _ in pairs]) + rs.uniform(-0.3, 0.3, (NV, H, W, 3))).astype(np.float32)  # leaves [0,1] on both sides
    assert pred.min() < 0 and pred.max() > 1
    depth = rs.uniform(0.5, 2.5, (NV, H * W)).astype(np.float32)
    args = (_t(pred.reshape(NV, -1, 3), dev), _t(depth, dev), 0.8, 1.8)
    plain = ops.eval_epilogue(*args, gt_rgb=_t(gt.reshape(NV, -1, 3), dev))
    full = ops.eval_epilogue(*args, gt_rgb=_t(gt.reshape(NV, -1, 3), dev), image_shape=(H, W))
    assert "ssim" not in plain and set(full) == set(plain) | {"ssim"}
    for k in plain:
        assert torch.equal(plain[k], full[k]), k
    assert full["ssim"].shape == (NV,) and full["ssim"].dtype == torch.float64
    ref = R.ssim_ref_batch(np.clip(pred, 0.0, 1.0), gt)
    assert np.abs(full["ssim"].cpu().numpy() - ref).max() <= BAR
    assert np.abs(R.ssim_ref_batch(pred, gt) - ref).max() > 1e-4   # (the unclamped image would give another number)
    assert "ssim" not in ops.eval_epilogue(args[0], image_shape=(H, W))  # nothing to compare with
    with pytest.raises(ValueError):
        ops.eval_epilogue(*args, gt_rgb=_t(gt.reshape(NV, -1, 3), dev), image_shape=(H, W + 1))


def test_util_ssim_shapes(dev):
    from pixelnerf_amd import util
    pairs = [R.disc_pair(20, 28, 70 + v) for v in range(4)]
    pred, gt = _t(np.stack([p for p, _ in pairs]), dev), _t(np.stack([g for _, g in pairs]), dev)
    one = util.ssim(pred[1], gt[1])
    assert one.shape == () and one.dtype == torch.float64
    many = util.ssim(pred, gt)
    assert many.shape == (4,) and float(many[1]) == float(one)
    assert abs(float(one) - R.ssim_ref(pairs[1][0], pairs[1][1])) <= BAR   # the reference's defaults: window 7, data range 1
