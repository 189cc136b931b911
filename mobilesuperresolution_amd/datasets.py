"""Device-side training input pipeline.  Reference: datasets/_isr.py:56-121 -- per item the DataLoader
workers open two PNGs, `_sample_patch` (random crop, HR crop at scale times the LR one), `_augment` (row flip, column flip,
axis swap) and torchvision's `to_tensor`; at >10^3 HR-Mpix/s per GPU eight Python workers (datasets/__init__.py:22-26)
cannot keep up.  Here the decoded uint8 images stay resident in HBM (DIV2K train: 800 HR images, ~7 GB; 288 GB per GPU)
and one kernel (csrc/patches.h) cuts, flips, transposes, converts and normalises a whole batch.  The random draws are
made on the host with the reference's own calls in the reference's order, so a seeded `random.Random` yields exactly
the patches the reference's `__getitem__` yields (tests/test_gpu_input.py)."""
from __future__ import annotations

import random as _random

import numpy as np
import torch

from . import _lib as L
from . import packing as PK

__all__ = ["DevicePatchCache", "DeviceClipCache", "DeviceBicubicPatchCache", "bicubic_downscale"]

_CLIP_REC = np.dtype([("ids_off", "<i8"), ("x", "<i4"), ("y", "<i4"), ("flags", "<i4"), ("T", "<i4")])     # sr_clip_rec_t
_CLIP_FRAME = np.dtype([("lr_off", "<i8"), ("hr_off", "<i8"), ("mv_off", "<i8"), ("lr_w", "<i4"), ("hr_w", "<i4")])   # sr_clip_frame_t
_PAD = 16              # bytes after the last frame: csrc/clips.h reads runs with wide loads
_REC = np.dtype([("lr_off", "<i8"), ("hr_off", "<i8"), ("lr_w", "<i4"), ("hr_w", "<i4"), ("x", "<i4"), ("y", "<i4"),
                 ("flags", "<i4"), ("pad", "<i4")])
_BICUBIC_REC = np.dtype([("hr_off", "<i8"), ("hr_w", "<i4"), ("x", "<i4"), ("y", "<i4"), ("flags", "<i4")])      # sr_bicubic_rec_t


def _as_u8(img):
    a = img.cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected H x W x 3 uint8 images (np.asarray(Image.open(...)), _isr.py:82-84), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


class DevicePatchCache:
    """`params` fields as the reference's dataset reads them: lr_patch_size, scale, ignored_boundary_size, num_patches
    (datasets/_isr.py:22-37,66-67).  `__len__` and the `index // num_patches` item mapping are the TRAIN-mode ones."""

    def __init__(self, lr_images, hr_images, lr_patch_size, scale, ignored_boundary_size=0, num_patches=1, device="cuda"):
        if len(lr_images) != len(hr_images) or not len(lr_images):
            raise ValueError("need as many HR as LR images, and at least one")
        self.P, self.scale = int(lr_patch_size), int(scale)
        self.ignored, self.num_patches = int(ignored_boundary_size), int(num_patches)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.HotpathError("DevicePatchCache (MI355X hot path) keeps its cache in HBM; there is no CPU fallback")
        chunks, self.meta, off = [], [], 0
        for lr, hr in zip(lr_images, hr_images):
            lr, hr = _as_u8(lr), _as_u8(hr)
            if hr.shape[0] < lr.shape[0] * self.scale or hr.shape[1] < lr.shape[1] * self.scale:
                raise ValueError(f"HR {hr.shape} smaller than scale x LR {lr.shape}")
            if min(lr.shape[:2]) - self.P + 1 - 2 * self.ignored <= 0:
                raise ValueError(f"LR image {lr.shape} too small for a {self.P} patch with boundary {self.ignored}")
            self.meta.append((off, lr.shape[0], lr.shape[1], off + lr.size, hr.shape[1]))
            chunks += [lr.reshape(-1), hr.reshape(-1)]
            off += lr.size + hr.size
        self.cache = torch.from_numpy(np.concatenate(chunks)).to(self.device)

    def __len__(self):
        return len(self.meta) * self.num_patches

    def draw(self, index, rng=_random):
        """one item's draws, in the reference's call order: randrange (row), randrange (column) -- _isr.py:90-95 -- then three
        `random() < 0.5` -- :113-121"""
        lr_off, h, w, hr_off, hr_w = self.meta[index // self.num_patches]
        x = rng.randrange(self.ignored, h - self.P + 1 - self.ignored)
        y = rng.randrange(self.ignored, w - self.P + 1 - self.ignored)
        flags = (1 if rng.random() < 0.5 else 0) | (2 if rng.random() < 0.5 else 0) | (4 if rng.random() < 0.5 else 0)
        return (lr_off, hr_off, w, hr_w, x, y, flags, 0)

    def batch(self, indices, rng=_random, want_lr=True, want_hr=True):
        """(lr (B,3,P,P), hr (B,3,P s,P s)) float32 in [0,1] on the device, items in the order of `indices`"""
        recs = np.array([self.draw(i, rng) for i in indices], dtype=_REC)
        b = len(recs)
        with torch.cuda.device(self.device):
            dev_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).pin_memory().to(self.device, non_blocking=True)
            lr = torch.empty((b, 3, self.P, self.P), dtype=torch.float32, device=self.device) if want_lr else None
            s = self.P * self.scale
            hr = torch.empty((b, 3, s, s), dtype=torch.float32, device=self.device) if want_hr else None
            L.launch("sr_patch_gather", L.lib().sr_patch_gather, self.cache.data_ptr(), dev_recs.data_ptr(),
                     lr.data_ptr() if lr is not None else None, hr.data_ptr() if hr is not None else None, b, self.P, self.scale,
                     L.stream_ptr())
        return lr, hr


class DeviceClipCache:
    """Video training clips for the trainer's 'basic' and 'basic_mv' models.  Reference: the TRAIN-mode
    `__getitem__` of VideoSuperResolution(Hdf5)Dataset (RGB) and VideoSuperResolutionWithMVHdf5Dataset (MV), datasets/_vsr.py:59-180
    and :314-432, with `train_sample_patch` set.  Every frame is stored once in HBM (LR / HR as uint8, motion vectors as float32,
    converted like the reference's `.float()`); a clip is a list of frame ids, as `lr_files[clip]` is a list of overlapping
    windows of frame files (datasets/reds.py `list_image_files`).  One launch of csrc/clips.h cuts a whole batch.

    lr_frames / hr_frames: H x W x 3 uint8; mv_frames (None: the RGB class): H x W x 2 of any numeric dtype, one per frame;
    clips: one list of frame ids per clip, all of one length T.  Items: (T, 3 or 5, P, P) and (T, 3, P scale, P scale)."""

    def __init__(self, lr_frames, hr_frames, clips, lr_patch_size, scale, ignored_boundary_size=0, num_patches=1, mv_frames=None,
                 device="cuda"):
        self.P, self.scale = int(lr_patch_size), int(scale)
        self.ignored, self.num_patches = int(ignored_boundary_size), int(num_patches)
        self.with_mv = mv_frames is not None
        if len(lr_frames) != len(hr_frames) or (self.with_mv and len(mv_frames) != len(lr_frames)) or not len(lr_frames):
            raise ValueError("need one HR (and MV) frame per LR frame, and at least one frame")
        if self.P <= 0 or self.scale <= 0 or self.ignored < 0 or self.num_patches <= 0:
            raise ValueError("lr_patch_size, scale and num_patches must be positive, ignored_boundary_size not negative")
        lrs, hrs = [_as_u8(f) for f in lr_frames], [_as_u8(f) for f in hr_frames]
        mvs = None
        if self.with_mv:
            mvs = [torch.from_numpy(np.ascontiguousarray(m.cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m))).float()
                   for m in mv_frames]
        clips = [[int(f) for f in c] for c in clips]
        if not clips or any(len(c) != len(clips[0]) for c in clips) or not clips[0]:
            raise ValueError("need at least one clip, all clips of the same (non-zero) number of frames")
        self.T = len(clips[0])
        for k, (lr, hr) in enumerate(zip(lrs, hrs)):
            if hr.shape[0] < lr.shape[0] * self.scale or hr.shape[1] < lr.shape[1] * self.scale:
                raise ValueError(f"frame {k}: HR {hr.shape} smaller than scale x LR {lr.shape}")
            if mvs is not None and tuple(mvs[k].shape) != lr.shape[:2] + (2,):
                raise ValueError(f"frame {k}: motion vectors {tuple(mvs[k].shape)} do not match LR {lr.shape[:2]} x 2")
        self.clip_hw, ids_off = [], []
        for c in clips:
            if any(f < 0 or f >= len(lrs) for f in c):
                raise ValueError(f"clip {c}: frame id out of range")
            if any(lrs[f].shape != lrs[c[0]].shape or hrs[f].shape != hrs[c[0]].shape for f in c):
                raise ValueError(f"clip {c}: frames of different sizes")
            h, w = lrs[c[0]].shape[:2]
            # the RGB class does not draw the row of frames at most 68 high (it crops from row 0): they need P rows only
            rows_ok = h >= self.P if (not self.with_mv and h <= 68) else h - self.P + 1 - 2 * self.ignored > 0
            if not rows_ok or w - self.P + 1 - 2 * self.ignored <= 0:
                raise ValueError(f"clip {c}: LR frames {h} x {w} too small for a {self.P} patch with boundary {self.ignored}")
            ids_off.append(len(self.clip_hw) * self.T)
            self.clip_hw.append((h, w))
        self.ids_off = ids_off
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.HotpathError("DeviceClipCache (MI355X hot path) keeps its cache in HBM; there is no CPU fallback")

        tab = np.zeros(len(lrs), dtype=_CLIP_FRAME)
        off = mv_off = 0
        for k, (lr, hr) in enumerate(zip(lrs, hrs)):
            tab[k] = (off, off + lr.size, mv_off, lr.shape[1], hr.shape[1])
            off += lr.size + hr.size
            mv_off += lr.shape[0] * lr.shape[1] * 2 * 4
        with torch.cuda.device(self.device):
            # frame by frame: REDS train is ~70 GB of uint8, more than a host copy of the whole cache should need
            self.cache = torch.empty(off + _PAD, dtype=torch.uint8, device=self.device)
            self.cache[off:].zero_()
            for k, (lr, hr) in enumerate(zip(lrs, hrs)):
                o = int(tab[k]["lr_off"])
                self.cache[o:o + lr.size].copy_(torch.from_numpy(lr.reshape(-1)))
                self.cache[o + lr.size:o + lr.size + hr.size].copy_(torch.from_numpy(hr.reshape(-1)))
            self.mv_cache = None
            if mvs is not None:
                self.mv_cache = torch.empty(mv_off // 4, dtype=torch.float32, device=self.device)
                for k, m in enumerate(mvs):
                    o = int(tab[k]["mv_off"]) // 4
                    self.mv_cache[o:o + m.numel()].copy_(m.reshape(-1))
            self.frames = torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(self.device)
            self.ids = torch.tensor([f for c in clips for f in c], dtype=torch.int32, device=self.device)

    def __len__(self):
        return len(self.clip_hw) * self.num_patches

    def draw(self, index, rng=_random):
        """one item's draws, in the reference's call order: p1 = random(), p2 = random(), the row x (not drawn -- 0 -- by the RGB
        class for frames at most 68 high), the column y -- _vsr.py:74-84 (RGB), :330-336 (MV); p1 < 0.5 reverses the width,
        p2 < 0.5 the height (`_augment`, :165-180, :415-432).  Returns the item's sr_clip_rec_t fields."""
        c = index // self.num_patches
        h, w = self.clip_hw[c]
        flags = (1 if rng.random() < 0.5 else 0) | (2 if rng.random() < 0.5 else 0)
        if not self.with_mv and h <= 68:
            x = 0
        else:
            x = rng.randrange(self.ignored, h - self.P + 1 - self.ignored)
        y = rng.randrange(self.ignored, w - self.P + 1 - self.ignored)
        return (self.ids_off[c], x, y, flags, self.T)

    def batch(self, indices, rng=_random, want_lr=True, want_hr=True):
        """(lr (B,T,3,P,P) -- (B,T,5,P,P) with motion vectors, the reference's `torch.cat((lr, mv), dim=1)` --, hr (B,T,3,sP,sP))
        float32 on the device, items in the order of `indices`"""
        recs = np.array([self.draw(i, rng) for i in indices], dtype=_CLIP_REC)
        b = len(recs)
        if not want_lr and self.with_mv:
            raise ValueError("the motion vectors travel in the LR tensor: want_lr is needed with mv_frames")
        with L.device_guard(self.device):
            dev_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).pin_memory().to(self.device, non_blocking=True)
            s = self.P * self.scale
            lr = torch.empty((b, self.T, 5 if self.with_mv else 3, self.P, self.P), dtype=torch.float32, device=self.device) if want_lr else None
            hr = torch.empty((b, self.T, 3, s, s), dtype=torch.float32, device=self.device) if want_hr else None
            L.launch("sr_clip_gather", L.lib().sr_clip_gather, self.cache.data_ptr(),
                     self.mv_cache.data_ptr() if self.mv_cache is not None else None, self.frames.data_ptr(), self.ids.data_ptr(),
                     dev_recs.data_ptr(), lr.data_ptr() if lr is not None else None, hr.data_ptr() if hr is not None else None,
                     b, self.T, self.P, self.scale, L.stream_ptr(self.device))
        return lr, hr


# ---- bicubic-on-the-fly: HR-only datasets (ImageSuperResolutionBicubicDataset, datasets/_isr.py:170-222) ----
_BICUBIC_TABLES = {}


def _bicubic_tables_on(length, scale, device):
    """packing.bicubic_tables(length, scale) in device memory, uploaded once per (length, scale, device): (weights, indices, taps)"""
    key = (int(length), int(scale), device.index if device.index is not None else torch.cuda.current_device())
    t = _BICUBIC_TABLES.get(key)
    if t is None:
        w, idx = PK.bicubic_tables(key[0], key[1])
        t = (torch.from_numpy(w.copy()).to(device), torch.from_numpy(idx.copy()).to(device), w.shape[1])
        _BICUBIC_TABLES[key] = t
    return t


def _bicubic_resize(img_u8, scale, want_f32, want_src_f32):
    """one launch of sr_bicubic_resize_u8: (uint8 h x w x 3, float32 (3, h, w) or None, the source as float32 (3, H, W) or None)"""
    if not isinstance(img_u8, torch.Tensor) or not img_u8.is_cuda:
        raise L.HotpathError("bicubic_downscale (MI355X hot path) needs a device tensor; there is no CPU fallback")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3 or not img_u8.numel():
        raise ValueError(f"expected an H x W x 3 uint8 image, got {img_u8.dtype} {tuple(img_u8.shape)}")
    scale = int(scale)
    if scale not in PK.BICUBIC_SCALES:
        raise ValueError(f"bicubic_downscale: scale {scale} not in {PK.BICUBIC_SCALES}")
    img = img_u8.contiguous()
    h, w = img.shape[:2]
    ho, wo = -(-h // scale), -(-w // scale)
    with L.device_guard(img.device):
        wr, ir, tr = _bicubic_tables_on(h, scale, img.device)
        wc, ic, tc = _bicubic_tables_on(w, scale, img.device)
        out = torch.empty((ho, wo, 3), dtype=torch.uint8, device=img.device)
        f32 = torch.empty((3, ho, wo), dtype=torch.float32, device=img.device) if want_f32 else None
        src = torch.empty((3, h, w), dtype=torch.float32, device=img.device) if want_src_f32 else None
        L.launch("sr_bicubic_resize_u8", L.lib().sr_bicubic_resize_u8, img.data_ptr(), out.data_ptr(),
                 f32.data_ptr() if f32 is not None else None, src.data_ptr() if src is not None else None, h, w, scale,
                 wr.data_ptr(), ir.data_ptr(), tr, wc.data_ptr(), ic.data_ptr(), tc, L.stream_ptr(img.device))
    return out, f32, src


def bicubic_downscale(img_u8, scale, return_f32=False):
    """The reference's `imresize(hr, scalar_scale=1 / scale)` (third_party/matlab_imresize/imresize.py) for uint8 input, bit for
    bit, on the device (csrc/bicubic.h): H x W x 3 uint8 -> ceil(H / scale) x ceil(W / scale) x 3 uint8, scale in {2, 3, 4}.
    return_f32: also the same values as `to_tensor` gives them, (3, h, w) float32 = value / 255, from the same launch."""
    out, f32, _ = _bicubic_resize(img_u8, scale, return_f32, False)
    return (out, f32) if return_f32 else out


def bicubic_patch_draw(h, w, side, rng=_random):
    """one TRAIN item's draws for an h x w HR image and an HR crop of `side`, in the reference's call order: randrange (row),
    randrange (column) -- _isr.py:204-205 -- then three `random() < 0.5` -- :112-118.  Returns (x, y, flags)."""
    x = rng.randrange(0, h - side + 1)
    y = rng.randrange(0, w - side + 1)
    flags = (1 if rng.random() < 0.5 else 0) | (2 if rng.random() < 0.5 else 0) | (4 if rng.random() < 0.5 else 0)
    return x, y, flags


class DeviceBicubicPatchCache:
    """HR-only training and evaluation items (the reference's ImageSuperResolutionBicubicDataset, from which Set5, Set14, BSDS100
    and Urban100 derive): only the HR images stay resident, as uint8, and the LR side is made on the device by the
    MATLAB-compatible bicubic downscale.  `__len__` and the `index // num_patches` item mapping are the TRAIN-mode ones.

    TRAIN item (_isr.py:197-214): an HR crop of side S = (lr_patch_size + 2 ignored_boundary_size) scale is resized as a whole,
    the LR patch is the resize without its `ignored_boundary_size` border, the HR patch the crop without scale times that.
    The reference's `[b:-b]` slices are empty for a boundary of 0, so that is refused here."""

    def __init__(self, hr_images, lr_patch_size, scale, ignored_boundary_size, num_patches=1, device="cuda"):
        self.P, self.scale = int(lr_patch_size), int(scale)
        self.ignored, self.num_patches = int(ignored_boundary_size), int(num_patches)
        if self.scale not in PK.BICUBIC_SCALES:
            raise ValueError(f"scale {self.scale} not in {PK.BICUBIC_SCALES}")
        if self.ignored < 1:
            raise ValueError("ignored_boundary_size must be at least 1: the reference's [b:-b] slices are empty for 0")
        if self.P <= 0 or self.num_patches <= 0 or not len(hr_images):
            raise ValueError("lr_patch_size and num_patches must be positive, and at least one image is needed")
        self.S = (self.P + 2 * self.ignored) * self.scale
        hrs = [_as_u8(h) for h in hr_images]
        self.meta, off = [], 0
        for hr in hrs:
            if min(hr.shape[:2]) < self.S:
                raise ValueError(f"HR image {hr.shape} smaller than the {self.S} x {self.S} crop "
                                 f"(({self.P} + 2 x {self.ignored}) x {self.scale})")
            self.meta.append((off, hr.shape[0], hr.shape[1]))
            off += hr.size
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.HotpathError("DeviceBicubicPatchCache (MI355X hot path) keeps its cache in HBM; there is no CPU fallback")
        self.cache = torch.from_numpy(np.concatenate([h.reshape(-1) for h in hrs])).to(self.device)

    def __len__(self):
        return len(self.meta) * self.num_patches

    def draw(self, index, rng=_random):
        """one item's sr_bicubic_rec_t fields; the draws are `bicubic_patch_draw`'s"""
        off, h, w = self.meta[index // self.num_patches]
        x, y, flags = bicubic_patch_draw(h, w, self.S, rng)
        return (off, w, x, y, flags)

    def batch(self, indices, rng=_random, want_lr=True, want_hr=True):
        """(lr (B,3,P,P), hr (B,3,P s,P s)) float32 in [0,1] on the device, items in the order of `indices`, from one launch"""
        recs = np.array([self.draw(i, rng) for i in indices], dtype=_BICUBIC_REC)
        b = len(recs)
        with L.device_guard(self.device):
            wt, it, taps = _bicubic_tables_on(self.S, self.scale, self.device)
            dev_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).pin_memory().to(self.device, non_blocking=True)
            lr = torch.empty((b, 3, self.P, self.P), dtype=torch.float32, device=self.device) if want_lr else None
            s = self.P * self.scale
            hr = torch.empty((b, 3, s, s), dtype=torch.float32, device=self.device) if want_hr else None
            L.launch("sr_bicubic_patch_gather", L.lib().sr_bicubic_patch_gather, self.cache.data_ptr(), dev_recs.data_ptr(),
                     lr.data_ptr() if lr is not None else None, hr.data_ptr() if hr is not None else None, b, self.P, self.scale,
                     self.ignored, wt.data_ptr(), it.data_ptr(), taps, L.stream_ptr(self.device))
        return lr, hr

    def eval_item(self, index):
        """the EVAL-mode item of image `index` (_isr.py:216-221): HR cropped to multiples of the scale, LR its bicubic downscale;
        (lr (1,3,h,w), hr (1,3,h s,w s)) float32 in [0,1], both from one launch (a true division by 255 like `to_tensor`'s:
        torch's own division of a device tensor by a scalar multiplies by the reciprocal, which is one ulp off for some values)"""
        off, h, w = self.meta[index]
        hc, wc = h - h % self.scale, w - w % self.scale
        if not hc or not wc:
            raise ValueError(f"HR image {h} x {w} smaller than the scale {self.scale}")
        hr = self.cache[off:off + h * w * 3].view(h, w, 3)[:hc, :wc]
        _, lr, hr_f32 = _bicubic_resize(hr, self.scale, True, True)
        return lr.unsqueeze(0), hr_f32.unsqueeze(0)
