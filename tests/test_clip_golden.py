"""G16 (tools/make_golden_clips.py: the reference's own VideoSuperResolutionHdf5Dataset / VideoSuperResolutionWithMVHdf5Dataset
`__getitem__` in TRAIN mode) pins the CPU restatement tests/clip_ref.py item for item and draw for draw."""
import os
import random

import numpy as np
import pytest

from tests import clip_ref as CR


def load_g16(golden_dir):
    """per configuration: (params dict, lr frames, hr frames, mv frames or None, clips, indices, seed, expected lr items as
    float32 -- RGB / 255 and the MV channels --, expected hr items, next random())"""
    z = np.load(os.path.join(golden_dir, "g16_clips.npz"))
    out = []
    for ci, (scale, P, ignored, num_patches, with_mv, image_batch) in enumerate(z["cfgs"].tolist()):
        n = int(z[f"c{ci}_n_frames"])
        lrs = [z[f"c{ci}_lr{k}"] for k in range(n)]
        hrs = [z[f"c{ci}_hr{k}"] for k in range(n)]
        mvs = [z[f"c{ci}_mv{k}"] for k in range(n)] if with_mv else None
        exp_lr = z[f"c{ci}_lr_items"].astype(np.float32) / np.float32(255)
        if with_mv:
            exp_lr = np.concatenate([exp_lr, z[f"c{ci}_mv_items"].astype(np.float32)], axis=2)
        exp_hr = z[f"c{ci}_hr_items"].astype(np.float32) / np.float32(255)
        out.append((dict(scale=scale, P=P, ignored=ignored, num_patches=num_patches, with_mv=bool(with_mv), T=image_batch),
                    lrs, hrs, mvs, z[f"c{ci}_clips"].tolist(), z[f"c{ci}_idx"].tolist(), int(z[f"c{ci}_seed"]), exp_lr, exp_hr,
                    float(z[f"c{ci}_next_random"])))
    return out


def test_g16_covers_what_it_should(golden_dir):
    cfgs = load_g16(golden_dir)
    assert {c[0]["with_mv"] for c in cfgs} == {False, True}
    heights = {(c[0]["with_mv"], c[1][0].shape[0] <= 68) for c in cfgs}
    assert (False, True) in heights and (False, False) in heights          # both sides of the RGB class's x = 0 rule
    assert any(c[0]["num_patches"] > 1 for c in cfgs) and any(c[0]["ignored"] > 0 for c in cfgs)
    assert all(len(c[4]) > 1 and len({f for clip in c[4] for f in clip}) < sum(map(len, c[4])) for c in cfgs)   # overlapping windows
    assert any(c[3] is not None and c[3][0].dtype == np.int16 and c[3][0].min() < 0 for c in cfgs)


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_restatement_reproduces_every_g16_item(golden_dir, ci):
    p, lrs, hrs, mvs, clips, idx, seed, exp_lr, exp_hr, nxt = load_g16(golden_dir)[ci]
    rng = random.Random(seed)
    for b, i in enumerate(idx):
        lr, hr = CR.train_item(lrs, hrs, clips, i, p["P"], p["scale"], p["ignored"], p["num_patches"], rng, mvs)
        assert np.array_equal(lr, exp_lr[b]), (ci, b, i)
        assert np.array_equal(hr, exp_hr[b]), (ci, b, i)
    assert rng.random() == nxt


def test_constructor_rejects_bad_inputs_before_touching_a_device():
    """the ValueErrors come from the host-side checks; a valid cache on a non-CUDA device is a HotpathError (no CPU fallback)"""
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.datasets import DeviceClipCache
    g = np.random.default_rng(0)
    lr = [g.integers(0, 256, (40, 48, 3), dtype=np.uint8) for _ in range(3)]
    hr = [g.integers(0, 256, (80, 96, 3), dtype=np.uint8) for _ in range(3)]
    mv = [np.zeros((40, 48, 2), np.int16) for _ in range(3)]
    with pytest.raises(L.HotpathError):
        DeviceClipCache(lr, hr, [[0, 1], [1, 2]], 12, 2, device="cpu")
    with pytest.raises(L.HotpathError):
        DeviceClipCache(lr, hr, [[0, 1], [1, 2]], 12, 2, mv_frames=mv, device="cpu")
    bad_lr = lr[:2] + [g.integers(0, 256, (40, 46, 3), dtype=np.uint8)]
    with pytest.raises(ValueError, match="different sizes"):
        DeviceClipCache(bad_lr, hr, [[1, 2]], 12, 2, device="cpu")
    with pytest.raises(ValueError, match="smaller than scale"):
        DeviceClipCache(lr, hr, [[0, 1]], 12, 3, device="cpu")
    with pytest.raises(ValueError, match="motion vectors"):
        DeviceClipCache(lr, hr, [[0, 1]], 12, 2, mv_frames=mv[:2] + [np.zeros((40, 47, 2), np.int16)], device="cpu")
    with pytest.raises(ValueError, match="too small"):
        DeviceClipCache(lr, hr, [[0, 1]], 48, 2, device="cpu")
    with pytest.raises(ValueError, match="too small"):               # 40 rows, P 38, boundary 2: the MV class draws x
        DeviceClipCache(lr, hr, [[0, 1]], 38, 2, ignored_boundary_size=2, mv_frames=mv, device="cpu")
    with pytest.raises(L.HotpathError):                              # ... the RGB class crops from row 0 (40 <= 68): fine
        DeviceClipCache(lr, hr, [[0, 1]], 38, 2, ignored_boundary_size=2, device="cpu")
