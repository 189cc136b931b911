"""`psnr` / `psnr_y` / `ssim` of the evaluation loop on the MI355X (reference: common/metrics.py:10-68, called by
utils/estimate.py:102-104,123-129).  Same names and arguments; the return value is a 0-dim device tensor (the per-image
values SUMMED over the batch), computed by csrc/metrics.h and csrc/ssim.h where the SR image already is instead of after
`.to('cpu')`.  `ssim` restates skimage's `structural_similarity` as the reference calls it (float64 from the filter on)
and returns float64.  No CPU fallback."""
from __future__ import annotations

import torch

from . import _lib as L

__all__ = ["psnr", "psnr_y", "ssim"]

_SSIM_TILE, _SSIM_RADIUS = 32, 5         # csrc/ssim.h: ssim::TW == ssim::TH, ssim::R


def _run(sr, hr, shave, luma):
    if not (sr.is_cuda and hr.is_cuda):
        raise L.HotpathError("psnr / psnr_y (MI355X hot path) need CUDA/HIP tensors; there is no CPU fallback")
    if sr.device != hr.device:
        raise L.HotpathError(f"sr on {sr.device}, hr on {hr.device}")
    if sr.shape != hr.shape or sr.dim() < 3:
        raise ValueError(f"sr {tuple(sr.shape)} vs hr {tuple(hr.shape)}")
    if hr.dtype != torch.float32:
        raise NotImplementedError("hr must be float32 (the reference casts sr to hr's dtype; its loaders produce float32)")
    c, h, w = sr.shape[-3:]
    if luma and not (sr.dim() == 4 and sr.shape[1] == 3):
        luma = -1                                    # metrics.py:29 tests shape[1]: anything else skips the luma filter
    s = sr.detach().to(hr.dtype).reshape(-1, c, h, w).contiguous()
    t = hr.detach().reshape(-1, c, h, w).contiguous()
    n = s.shape[0]
    wgs = max(1, min(64, (c * h * w + 4095) // 4096))
    with torch.cuda.device(sr.device):
        partial = torch.empty(n * wgs, dtype=torch.float32, device=sr.device)
        out = torch.empty((), dtype=torch.float32, device=sr.device)
        L.launch("sr_psnr", L.lib().sr_psnr, s.data_ptr(), t.data_ptr(), partial.data_ptr(), out.data_ptr(), n, c, h, w,
                 int(shave) if shave else 0, luma, wgs, L.stream_ptr())
    return out


def psnr(sr, hr, shave=4):
    """common/metrics.py:10-19"""
    return _run(sr, hr, shave, 0)


def psnr_y(sr, hr, shave=4):
    """common/metrics.py:22-38 (including the unused quantised copy: sr is clamped, not quantised)"""
    return _run(sr, hr, shave, 1)


def ssim(X, Y, shave=4):
    """common/metrics.py:41-68 with X = SR, Y = HR: skimage's structural_similarity (11 x 11 Gaussian window, sigma 1.5,
    data_range 1, K1 0.01, K2 0.03, sample covariance) of the float32 lumas of the 8-bit quantised X and of Y, both
    shaved.  Returns a 0-dim float64 tensor on the inputs' device (the reference returns a numpy float64).

    Extension: for more than one image -- (N,3,H,W) or (B,T,3,H,W) -- the result is the per-image values SUMMED, the
    convention of `psnr` here.  The reference has no batch form: its `.squeeze()` would hand skimage a 3-D volume, and its
    video branch has the `ssim` call commented out.

    What makes the reference fail raises ValueError: fewer than 3 dims, a channel count other than 3, shave < 1 (its
    unguarded `shave:-shave` leaves an empty image) and a shaved side below 11 ("win_size exceeds image extent")."""
    if not (X.is_cuda and Y.is_cuda):
        raise L.HotpathError("ssim (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
    if X.device != Y.device:
        raise L.HotpathError(f"X on {X.device}, Y on {Y.device}")
    if X.shape != Y.shape or X.dim() < 3:
        raise ValueError(f"X {tuple(X.shape)} vs Y {tuple(Y.shape)}")
    if Y.dtype != torch.float32:
        raise NotImplementedError("Y must be float32 (the reference casts X to Y's dtype; its loaders produce float32)")
    c, h, w = X.shape[-3:]
    shave = int(shave)
    if c != 3:
        raise ValueError(f"ssim needs 3 channels (the luma weights), got {c}")
    if shave < 1:
        raise ValueError(f"shave {shave} < 1: the reference's [shave:-shave] leaves an empty image")
    if h - 2 * shave < 11 or w - 2 * shave < 11:
        raise ValueError(f"win_size 11 exceeds the shaved image extent {h - 2 * shave} x {w - 2 * shave}")
    s = X.detach().to(Y.dtype).reshape(-1, c, h, w).contiguous()
    t = Y.detach().reshape(-1, c, h, w).contiguous()
    n = s.shape[0]
    tiles = -(-(h - 2 * shave - 2 * _SSIM_RADIUS) // _SSIM_TILE) * -(-(w - 2 * shave - 2 * _SSIM_RADIUS) // _SSIM_TILE)
    with torch.cuda.device(X.device):
        partial = torch.empty(n * tiles, dtype=torch.float64, device=X.device)
        out = torch.empty((), dtype=torch.float64, device=X.device)
        L.launch("sr_ssim", L.lib().sr_ssim, s.data_ptr(), t.data_ptr(), partial.data_ptr(), out.data_ptr(), n, h, w, shave,
                 n * tiles, L.stream_ptr())
    return out
