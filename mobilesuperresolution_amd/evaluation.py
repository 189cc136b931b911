"""What the reference's evaluation loops do per frame between the network and their prints (utils/estimate.py:49-129,
test_video_superresolution_by_patch.py:198-224), on the MI355X where the SR clip already is instead of after `.to('cpu')`:

    clip_metrics(sr, lr, hr, shave=4, align_corners=False) -> (4, B*N) float32, rows
        psnr(sr, hr), psnr_y(sr, hr), psnr(bilinear baseline of lr, hr), Charbonnier mean (the `test loss` term)  PER FRAME
    bilinear_baseline_u8(lr, size, align_corners=False), to_uint8_hwc(img) -> (F, H, W, 3) uint8, what save_image quantises
    clip_variation(lr) -> (2, B*N) float32, rows total_variation, time_variation

The baseline is `interpolate(lr, (H, W), mode='bilinear', align_corners=...)` as ATen computes it in fp32; it is blended in
registers (csrc/eval.h) and never stored in float.  `metrics.psnr` / `psnr_y` return batch sums; these return one value per
frame, which is what the by-patch script records.  No CPU fallback."""
from __future__ import annotations

import torch

from . import _lib as L

__all__ = ["clip_metrics", "bilinear_baseline_u8", "to_uint8_hwc", "clip_variation"]


def _need_device(what, *ts):
    if not all(t.is_cuda for t in ts):
        raise L.HotpathError(f"{what} (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
    for t in ts[1:]:
        if t.device != ts[0].device:
            raise L.HotpathError(f"{what}: tensors on {ts[0].device} and {t.device}")


def _frames(t, what):
    """(B,N,C,H,W) or (N,C,H,W) -> contiguous float32 (F,C,H,W)"""
    if t.dim() not in (4, 5):
        raise ValueError(f"{what} must be (B,N,C,H,W) or (N,C,H,W), got {tuple(t.shape)}")
    return t.detach().to(torch.float32).reshape(-1, *t.shape[-3:]).contiguous()


def _wgs(items):
    return max(1, min(256, (items + 4095) // 4096))


def clip_metrics(sr, lr, hr, shave=4, align_corners=False):
    """Rows psnr, psnr_y, psnr_bilinear, charbonnier of a (4, B*N) float32 device tensor, one column per frame.
    sr, hr (B,N,3,H,W) or (N,3,H,W); lr the same with (h, w) and at least 3 channels, of which the first three are used
    (estimate.py:81-82).  Rows 0-2 shave the border (nan when nothing is left, as `metrics.psnr`); row 3, the mean of
    sqrt((sr - hr)^2 + 1e-12), covers the whole frame as the reference's loss does.  The video branch of the reference
    calls this with shave=4, align_corners=False; its image branch has align_corners=True and shave=scale + 6 for rows 0
    and 2 but shave=scale for psnr_y: two calls there."""
    _need_device("clip_metrics", sr, lr, hr)
    if sr.shape != hr.shape or sr.dim() not in (4, 5) or sr.shape[-3] != 3:
        raise ValueError(f"sr {tuple(sr.shape)} vs hr {tuple(hr.shape)}: need equal (B,N,3,H,W) or (N,3,H,W)")
    if lr.dim() != sr.dim() or lr.shape[:-3] != sr.shape[:-3] or lr.shape[-3] < 3:
        raise ValueError(f"lr {tuple(lr.shape)} does not go with sr {tuple(sr.shape)}: same leading dims, >= 3 channels")
    if hr.dtype != torch.float32:
        raise NotImplementedError("hr must be float32 (the reference casts sr to hr's dtype; its loaders produce float32)")
    s, t, l = _frames(sr, "sr"), _frames(hr, "hr"), _frames(lr, "lr")
    f, _, H, W = s.shape
    wgs = _wgs(H * W)
    with L.device_guard(sr.device):
        partial = torch.empty(f * wgs * 4, dtype=torch.float32, device=sr.device)
        out = torch.empty((4, f), dtype=torch.float32, device=sr.device)
        L.launch("sr_eval_clip", L.lib().sr_eval_clip, s.data_ptr(), l.data_ptr(), t.data_ptr(), partial.data_ptr(), out.data_ptr(),
                 f, H, W, l.shape[2], l.shape[3], l.shape[1], int(shave) if shave else 0, int(bool(align_corners)), wgs,
                 L.stream_ptr())
    return out


def _u8(src, H, W, from_lr, align_corners):
    f, c, h, w = src.shape
    with L.device_guard(src.device):
        out = torch.empty((f, H, W, 3), dtype=torch.uint8, device=src.device)
        L.launch("sr_eval_u8", L.lib().sr_eval_u8, src.data_ptr(), out.data_ptr(), f, H, W, h, w, c, from_lr,
                 int(bool(align_corners)), L.stream_ptr())
    return out


def to_uint8_hwc(img):
    """save_image's quantisation of `img.clamp(0, 1)`: (F,3,H,W) or (B,N,3,H,W) float -> (F,H,W,3) uint8 on device,
    uint8(clamp(x.clamp(0, 1) * 255 + 0.5, 0, 255)): the bytes the reference's PNG holds (estimate.py:84,86)"""
    _need_device("to_uint8_hwc", img)
    if img.dim() not in (4, 5) or img.shape[-3] != 3:
        raise ValueError(f"img must be (F,3,H,W) or (B,N,3,H,W), got {tuple(img.shape)}")
    x = _frames(img, "img")
    return _u8(x, x.shape[2], x.shape[3], 0, False)


def bilinear_baseline_u8(lr, size, align_corners=False):
    """the same bytes for `interpolate(lr, size, mode='bilinear', align_corners=...)[:, :3]` (estimate.py:80-85) without
    the float image: lr (F,C>=3,h,w) or (B,N,C,h,w), size = (H, W) -> (F,H,W,3) uint8 on device"""
    _need_device("bilinear_baseline_u8", lr)
    if lr.dim() not in (4, 5) or lr.shape[-3] < 3:
        raise ValueError(f"lr must be (F,C,h,w) or (B,N,C,h,w) with C >= 3, got {tuple(lr.shape)}")
    H, W = (int(v) for v in size)
    if H <= 0 or W <= 0:
        raise ValueError(f"size {size}")
    return _u8(_frames(lr, "lr"), H, W, 1, align_corners)


def clip_variation(lr):
    """Rows total_variation, time_variation (by_patch.py:43-69) of a (2, B*N) float32 device tensor for lr (B,N,C,h,w);
    (N,C,h,w) is one clip.  time_variation is zero everywhere for N = 1."""
    _need_device("clip_variation", lr)
    if lr.dim() not in (4, 5):
        raise ValueError(f"lr must be (B,N,C,h,w) or (N,C,h,w), got {tuple(lr.shape)}")
    b, n = (lr.shape[0], lr.shape[1]) if lr.dim() == 5 else (1, lr.shape[0])
    x = _frames(lr, "lr")
    _, c, h, w = x.shape
    wgs = _wgs(c * h * w)
    with L.device_guard(lr.device):
        partial = torch.empty(b * n * wgs * 2, dtype=torch.float32, device=lr.device)
        out = torch.empty((2, b * n), dtype=torch.float32, device=lr.device)
        L.launch("sr_eval_variation", L.lib().sr_eval_variation, x.data_ptr(), partial.data_ptr(), out.data_ptr(), b, n, c, h, w,
                 wgs, L.stream_ptr())
    return out
