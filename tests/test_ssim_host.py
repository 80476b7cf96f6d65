"""Host tests (no GPU) of the on-device SSIM: the numpy restatement the GPU tests compare against is itself checked against
the route scikit-image takes (scipy's uniform filter on the five products, cropped), and the C entry refuses bad arguments on the
host before any HIP call.

Tolerance: two fp64 evaluations of the formula that differ only in summation order (direct 49-term sums here, scipy's running
sums there) differ by a few 1e-14 on these cases; the bar is 1e-12."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref as R
from pixelnerf_amd import _lib, ops


def _scipy_route(pred, gt, win=7, data_range=1.0):
    from scipy.ndimage import uniform_filter
    pred, gt = pred.astype(np.float64), gt.astype(np.float64)
    npx = win * win
    cn, pad = npx / (npx - 1.0), (win - 1) // 2
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vals = []
    for ch in range(pred.shape[2]):
        x, y = pred[..., ch], gt[..., ch]
        ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
        uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        vals.append(s[pad:s.shape[0] - pad, pad:s.shape[1] - pad].mean())
    return float(np.mean(vals))


def test_restatement_matches_the_filter_route():
    pytest.importorskip("scipy")
    for name, (pred, gt) in R.cases().items():
        a, b = R.ssim_ref(pred, gt), _scipy_route(pred, gt)
        print(f"{name}: restatement {a:.15f}  scipy route {b:.15f}  diff {abs(a - b):.2e}")
        assert abs(a - b) <= 1e-12, name
    pred, gt = R.cases()["identical_48x40"]
    assert R.ssim_ref(pred, gt) == 1.0
    n = R.ssim_ref(*R.cases()["noise_64x64"])
    assert abs(n) < 0.05  # independent noise: no structure in common


def test_pnr_ssim_refuses_bad_arguments_on_the_host():
    """PNR_E_INVALID (-1) with the argument named, before any HIP call (on a machine without a GPU a HIP call would fail with
    PNR_E_HIP = -2 instead); the addresses are dummies, never dereferenced"""
    _lib.build_library()
    lib = _lib.load()
    big = 1 << 30
    call = lambda pred=64, gt=64, nv=2, H=32, W=24, ch=3, win=7, dr=1.0, ws=64, nb=big, out=64: lib.pnr_ssim(  # noqa: E731
        pred, gt, nv, H, W, ch, win, dr, ws, nb, out, None)
    for win in (4, 8, 1, 17, 0, -3):  # even, below 3, above 15
        assert call(win=win) == -1 and b"win_size" in lib.pnr_last_error(), win
    assert call(win=9, H=8) == -1 and b"win_size" in lib.pnr_last_error()       # larger than the image
    assert call(win=9, W=7) == -1 and b"win_size" in lib.pnr_last_error()
    for ch in (0, 5, -1):
        assert call(ch=ch) == -1 and b"channels" in lib.pnr_last_error(), ch
    assert call(pred=None) == -1 and b"pred" in lib.pnr_last_error()
    assert call(gt=None) == -1 and b"gt" in lib.pnr_last_error()
    assert call(out=None) == -1 and b"ssim" in lib.pnr_last_error()
    need = lib.pnr_ssim_workspace_bytes(2, 32, 24, 3)
    assert need >= 8 and need % 8 == 0
    assert call(nb=need - 1) == -1 and b"workspace" in lib.pnr_last_error()
    assert call(ws=None) == -1 and b"workspace" in lib.pnr_last_error()
    assert call(nv=-1) == -1
    assert call(dr=0.0) == -1 and b"data_range" in lib.pnr_last_error()
    assert call(nv=0, pred=None, gt=None, out=None, ws=None, nb=0) == 0          # no views: a no-op
    # the workspace is a function of the image, not of the window; it grows linearly with views and channels
    assert lib.pnr_ssim_workspace_bytes(4, 32, 24, 3) == 2 * need
    assert lib.pnr_ssim_workspace_bytes(2, 32, 24, 1) * 3 == need
    assert lib.pnr_ssim_workspace_bytes(0, 32, 24, 3) == 0


def test_abi_revision_stays_12_and_the_header_declares_the_entries(repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"size_t\s+pnr_ssim_workspace_bytes\s*\(", code) and re.search(r"int\s+pnr_ssim\s*\(", code)
    assert "pnr_ssim" in _lib.PROTOTYPES and "pnr_ssim_workspace_bytes" in _lib.PROTOTYPES
    assert _lib._AUX not in _lib.PROTOTYPES["pnr_ssim"][1]
    _lib.build_library()
    lib = _lib.load()
    assert lib.pnr_abi_version() == 12 and hasattr(lib, "pnr_ssim")
    assert ctypes.sizeof(ctypes.c_double) == 8


def test_ssim_operators_refuse_cpu_tensors():
    from pixelnerf_amd import util
    a = torch.rand(2, 16, 16, 3)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.ssim(a, a)
    with pytest.raises(_lib.PixelNerfHipError):
        ops.ssim(a[0], a[0])
    with pytest.raises(_lib.PixelNerfHipError):
        util.ssim(a[0], a[0])
