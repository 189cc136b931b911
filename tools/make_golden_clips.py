#!/usr/bin/env python3
"""Write fixture G16 (tests/golden/g16_clips.npz) by running the REFERENCE's own video training-item path on the CPU:

    SR_REFERENCE_ROOT=<reference checkout> python tools/make_golden_clips.py

`datasets._vsr` is imported from the reference with the absent third-party modules stubbed (oracle/make_golden.py's stubs,
plus torchvision's RandomHorizontalFlip / RandomVerticalFlip at p=1 -- `t.flip(-1)` / `t.flip(-2)`, torchvision's documented
tensor behaviour -- and an empty cv2).  Instances of VideoSuperResolutionHdf5Dataset (RGB) and
VideoSuperResolutionWithMVHdf5Dataset (MV) are made without their `__init__` (it would write h5 files): dict-backed stand-ins
with `.get(path)` take the place of the h5 caches, so the reference's own `_load_item`, `__getitem__`, `_sample_patch` and
`_augment` run unchanged, in TRAIN mode with `train_sample_patch` set, under a seeded `random`.

Stored per configuration: the frames, the clips (frame ids of `lr_files[clip]`, overlapping windows of `image_batch` frames as
datasets/reds.py `list_image_files` builds them), the parameters, every item (LR / HR as uint8 -- `to_tensor` only divides by
255 --, MV as int16) and `random.random()` drawn right after the last item, which pins the number of draws."""
import argparse
import importlib
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SR_REFERENCE_ROOT", "")
OUT = os.path.join(ROOT, "tests", "golden", "g16_clips.npz")

# (scale, lr_patch_size, ignored_boundary_size, num_patches, with_mv, image_batch, sequences as (n_frames, lr_h, lr_w), n_items)
CFGS = [
    (2, 12, 2, 2, 0, 3, [(4, 40, 52), (4, 44, 48)], 24),     # RGB, frames <= 68 high: x = 0, not drawn
    (3, 10, 0, 1, 0, 2, [(3, 70, 36)], 16),                  # RGB, frames > 68 high: x drawn
    (2, 12, 1, 3, 1, 3, [(4, 40, 44)], 24),                  # MV (int16): x drawn whatever the height
]


class _DictCache:
    """stands in for common.io.Hdf5: `.get(path)` returns the stored array"""

    def __init__(self, d):
        self.d = d

    def get(self, key):
        return self.d[key]


def _stubs():
    sys.path.insert(0, ROOT)
    from oracle.make_golden import _absent_third_party_stubs
    _absent_third_party_stubs()
    tt = sys.modules["torchvision.transforms"]

    class RandomHorizontalFlip:
        def __init__(self, p=0.5):
            assert p == 1

        def __call__(self, t):
            return t.flip(-1)

    class RandomVerticalFlip(RandomHorizontalFlip):
        def __call__(self, t):
            return t.flip(-2)

    tt.RandomHorizontalFlip, tt.RandomVerticalFlip = RandomHorizontalFlip, RandomVerticalFlip
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("datasets._vsr"), importlib.import_module("common.modes")


def main():
    if not os.path.isfile(os.path.join(REF, "datasets", "_vsr.py")):
        sys.exit("set SR_REFERENCE_ROOT to a checkout of the reference")
    vsr, modes = _stubs()
    d = {"cfgs": np.array([c[:6] for c in CFGS], dtype=np.int64)}
    for ci, (scale, P, ignored, num_patches, with_mv, image_batch, seqs, n_items) in enumerate(CFGS):
        g = np.random.default_rng(160 + ci)
        lr_c, hr_c, mv_c, lr_files, hr_files, clips = {}, {}, {}, [], [], []
        k = 0
        for si, (n_frames, h, w) in enumerate(seqs):
            first = k
            for f in range(n_frames):
                lr = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
                hr = g.integers(0, 256, (h * scale + (si + ci) % 2, w * scale + si % 2, 3), dtype=np.uint8)   # HR may be a pixel larger
                lr_c[f"lr/{si}/{f:08d}.png"], hr_c[f"hr/{si}/{f:08d}.png"] = lr, hr
                d[f"c{ci}_lr{k}"], d[f"c{ci}_hr{k}"] = lr, hr
                if with_mv:
                    mv = g.integers(-40, 41, (h, w, 2), dtype=np.int16)
                    mv_c[f"lr/{si}/{f:08d}.png"] = mv
                    d[f"c{ci}_mv{k}"] = mv
                k += 1
            for s in range(0, n_frames + 1 - image_batch):                   # list_image_files: range(0, 101 - image_batch)
                lr_files.append([f"lr/{si}/{f:08d}.png" for f in range(s, s + image_batch)])
                hr_files.append([f"hr/{si}/{f:08d}.png" for f in range(s, s + image_batch)])
                clips.append(list(range(first + s, first + s + image_batch)))
        cls = vsr.VideoSuperResolutionWithMVHdf5Dataset if with_mv else vsr.VideoSuperResolutionHdf5Dataset
        ds = cls.__new__(cls)
        ds.mode, ds.lr_files, ds.hr_files, ds.image_batch = modes.TRAIN, lr_files, hr_files, image_batch
        ds.params = argparse.Namespace(scale=scale, lr_patch_size=P, ignored_boundary_size=ignored, num_patches=num_patches,
                                       train_sample_patch=True)
        ds.lr_cache_file, ds.hr_cache_file = _DictCache(lr_c), _DictCache(hr_c)
        if with_mv:
            ds.mv_cache_file = _DictCache(mv_c)
        idx = (list(range(len(ds))) * n_items)[:n_items]
        random.seed(1600 + ci)
        lrs, hrs, mvs = [], [], []
        for i in idx:
            a, b = ds[i]
            assert a.shape == (image_batch, 5 if with_mv else 3, P, P) and b.shape == (image_batch, 3, P * scale, P * scale)
            rgb = a[:, :3]
            lrs.append((rgb * 255).round().to(torch.uint8).numpy())
            hrs.append((b * 255).round().to(torch.uint8).numpy())
            assert torch.equal(torch.from_numpy(lrs[-1]).float().div(255), rgb)
            assert torch.equal(torch.from_numpy(hrs[-1]).float().div(255), b)
            if with_mv:
                mvs.append(a[:, 3:].to(torch.int16).numpy())
                assert torch.equal(torch.from_numpy(mvs[-1]).float(), a[:, 3:])
        d[f"c{ci}_n_frames"] = np.int64(k)
        d[f"c{ci}_clips"] = np.array(clips, dtype=np.int64)
        d[f"c{ci}_idx"] = np.array(idx, dtype=np.int64)
        d[f"c{ci}_seed"] = np.int64(1600 + ci)
        d[f"c{ci}_lr_items"], d[f"c{ci}_hr_items"] = np.stack(lrs), np.stack(hrs)
        if with_mv:
            d[f"c{ci}_mv_items"] = np.stack(mvs)
        d[f"c{ci}_next_random"] = np.float64(random.random())
        print(f"G16 cfg {ci} (scale {scale}, P {P}, ignored {ignored}, num_patches {num_patches}, mv {with_mv}, "
              f"image_batch {image_batch}): {len(clips)} clips, {len(idx)} items")
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
