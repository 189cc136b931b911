"""float64 numpy restatement of the reference's `ssim` (common/metrics.py:41-68), the yardstick of csrc/ssim.h
(tests/test_gpu_ssim.py); tests/test_ssim_ref_host.py pins it to scipy's gaussian_filter and to hand cases.  No torch, no
scipy, no oracle.

    X = SR, Y = HR, (..., 3, H, W) float32 in either.
    1. X = (X * 255).round().clamp(0, 255) / 255 in float32 (round half to even, true division); Y is not quantised
    2. luma of both = (R c0 + G c1) + B c2 in float32, c = float32([65.738, 129.057, 25.064]) / 256
    3. crop [shave:-shave] on both axes, to float64
    4. skimage.metrics.structural_similarity(win_size=11, gaussian_weights=True, sigma=1.5, data_range=1, K1=.01, K2=.03):
       the window is scipy's gaussian_filter with truncate 3.5 (radius 5), use_sample_covariance stays True (121 / 120),
       and the mean of S leaves out a 5-pixel border.  That border is the filter's radius, so no kept pixel's window
       leaves the cropped image and the filter's `reflect` mode never shows: the "valid" filter below is the same number.
skimage is not a dependency of this project: the steps are transcribed from its source, and their agreement with an
actual skimage run is unmeasured."""
import numpy as np

RADIUS, SIGMA = 5, 1.5
C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
COV_NORM = 121.0 / 120.0


def window():
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w = np.exp(-0.5 / (SIGMA * SIGMA) * k ** 2)
    return w / w.sum()


def quantise(sr):
    """step 1, float32"""
    x = np.asarray(sr, dtype=np.float32)
    return np.clip(np.round(x * np.float32(255)), np.float32(0), np.float32(255)) / np.float32(255)


def luma(img):
    """step 2 on (..., 3, H, W), float32: three rounded products, R + G, then + B"""
    img = np.asarray(img, dtype=np.float32)
    c = np.array([65.738, 129.057, 25.064], dtype=np.float32) / np.float32(256)
    out = (img[..., 0, :, :] * c[0] + img[..., 1, :, :] * c[1]) + img[..., 2, :, :] * c[2]
    assert out.dtype == np.float32
    return out


def _valid(a, w, axis):
    n = a.shape[axis] - 2 * RADIUS
    out = np.zeros_like(np.take(a, range(n), axis=axis))
    for k in range(2 * RADIUS + 1):
        out += w[k] * np.take(a, range(k, k + n), axis=axis)
    return out


def ssim_map(x, y, filt=None):
    """step 4 on two float64 (H', W') images: S at the (H' - 10, W' - 10) pixels the mean keeps.  filt(a) -> the filtered
    image already cut to those pixels (default: the valid separable Gaussian, axis 0 then axis 1)"""
    if filt is None:
        w = window()
        filt = lambda a: _valid(_valid(a, w, 0), w, 1)
    ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_ref(sr, hr, shave=4, filt=None):
    """the reference's value for one image; for more (any leading dims) the per-image values summed"""
    sr, hr = np.asarray(sr), np.asarray(hr)
    assert sr.shape == hr.shape and sr.ndim >= 3 and sr.shape[-3] == 3 and shave >= 1
    h, w = sr.shape[-2:]
    assert h - 2 * shave >= 2 * RADIUS + 1 and w - 2 * shave >= 2 * RADIUS + 1
    x = luma(quantise(sr)).reshape(-1, h, w)[:, shave:-shave, shave:-shave].astype(np.float64)
    y = luma(hr).reshape(-1, h, w)[:, shave:-shave, shave:-shave].astype(np.float64)
    return float(sum(ssim_map(a, b, filt).mean(dtype=np.float64) for a, b in zip(x, y)))
