"""CPU restatement of one video training item, datasets/_vsr.py in TRAIN mode with `train_sample_patch` set: the RGB class
(VideoSuperResolution(Hdf5)Dataset, :59-180) and the MV class (VideoSuperResolutionWithMVHdf5Dataset, :314-432).  numpy only.
Pinned to the reference's own classes by fixture G16 (tools/make_golden_clips.py; tests/test_clip_golden.py), item for item
and draw for draw; the parity tests of mobilesuperresolution_amd.datasets.DeviceClipCache use it for random shapes."""
import numpy as np


def draw(h, w, P, ignored, rng, with_mv):
    """p1, p2, then the LR row x (the RGB class makes no draw for frames at most 68 high: x = 0), then the LR column y"""
    p1 = rng.random()
    p2 = rng.random()
    x = 0 if (not with_mv and h <= 68) else rng.randrange(ignored, h - P + 1 - ignored)
    y = rng.randrange(ignored, w - P + 1 - ignored)
    return p1, p2, x, y


def train_item(lr_frames, hr_frames, clips, index, P, scale, ignored, num_patches, rng, mv_frames=None):
    """one `__getitem__(index)`: (T, 3, P, P) float32 -- (T, 5, P, P) with motion vectors, channels 3, 4 = the MV as float32,
    not scaled -- and (T, 3, sP, sP) float32"""
    clip = clips[index // num_patches]
    h, w = lr_frames[clip[0]].shape[:2]
    p1, p2, x, y = draw(h, w, P, ignored, rng, mv_frames is not None)
    lr = np.stack([lr_frames[f][x:x + P, y:y + P] for f in clip])                                      # T, P, P, 3
    hr = np.stack([hr_frames[f][x * scale:(x + P) * scale, y * scale:(y + P) * scale] for f in clip])
    parts = [lr, hr]
    if mv_frames is not None:
        parts.append(np.stack([np.asarray(mv_frames[f])[x:x + P, y:y + P] for f in clip]))
    if p1 < 0.5:                                                       # RandomHorizontalFlip: reverse the width
        parts = [a[:, :, ::-1] for a in parts]
    if p2 < 0.5:                                                       # RandomVerticalFlip: reverse the height
        parts = [a[:, ::-1] for a in parts]
    lr, hr = (np.ascontiguousarray(a.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255) for a in parts[:2])
    if mv_frames is not None:
        mv = np.ascontiguousarray(parts[2].transpose(0, 3, 1, 2)).astype(np.float32)             # mv.float(), sign kept
        lr = np.concatenate([lr, mv], axis=1)
    return lr, hr
