"""Test helper (not a test): the structural similarity of include/pixelnerf_hip.h `pnr_ssim`, restated in numpy fp64 by direct
summation over every window that lies fully inside the image, and the seeded images the SSIM tests run on."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SIZES = [(64, 64), (128, 128), (300, 400), (7, 7), (9, 23)]  # (H, W): ..., DTU, a single window, a thin odd one


def ssim_ref(pred, gt, win_size=7, data_range=1.0):
    """pred, gt (H,W,C) -> float: mean over windows, then over channels, everything in fp64"""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    assert pred.shape == gt.shape and pred.ndim == 3
    npx = win_size * win_size
    cn = npx / (npx - 1.0)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    per_channel = []
    for ch in range(pred.shape[2]):
        wx = sliding_window_view(pred[..., ch], (win_size, win_size))
        wy = sliding_window_view(gt[..., ch], (win_size, win_size))
        ux, uy = wx.sum(axis=(-2, -1)) / npx, wy.sum(axis=(-2, -1)) / npx
        uxx, uyy, uxy = (wx * wx).sum(axis=(-2, -1)) / npx, (wy * wy).sum(axis=(-2, -1)) / npx, (wx * wy).sum(axis=(-2, -1)) / npx
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        s = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        per_channel.append(s.mean())
    return float(np.mean(per_channel))


def ssim_ref_batch(pred, gt, win_size=7, data_range=1.0):
    return np.array([ssim_ref(p, g, win_size, data_range) for p, g in zip(pred, gt)])


def disc_pair(H, W, seed, channels=3):
    """-> (pred, gt) (H,W,channels) float32 in [0,1].  gt: a shaded disc on a white background, every channel offset; pred = gt +
    0.03 N(0,1), clamped; the upper half of pred is an exact copy of gt (white and flat there: S must be exactly 1)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx, rad = 0.55 * H, 0.5 * W, 0.35 * min(H, W)
    d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) / max(rad, 1.0)
    gt = np.ones((H, W, channels))
    for ch in range(channels):
        shade = 0.25 + 0.1 * ch + 0.5 * np.clip(1.0 - d, 0.0, 1.0) * (0.6 + 0.4 * np.cos(0.3 * xx + ch))
        gt[..., ch] = np.where(d < 1.0, shade, 1.0)
    gt = np.clip(gt, 0.0, 1.0).astype(np.float32)
    pred = np.clip(gt + 0.03 * rs.randn(H, W, channels), 0.0, 1.0).astype(np.float32)
    pred[: H // 2] = gt[: H // 2]
    return pred, gt


def noise_pair(H, W, seed, channels=3):
    """two independent uniform-noise images (SSIM close to 0)"""
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 1, (H, W, channels)).astype(np.float32), rs.uniform(0, 1, (H, W, channels)).astype(np.float32)


def cases():
    """name -> (pred, gt): the sizes above, the noise pair and an identical pair"""
    out = {f"disc_{h}x{w}": disc_pair(h, w, 100 + i) for i, (h, w) in enumerate(SIZES)}
    out["noise_64x64"] = noise_pair(64, 64, 7)
    same = disc_pair(48, 40, 9)[1]
    out["identical_48x40"] = (same, same.copy())
    return out
