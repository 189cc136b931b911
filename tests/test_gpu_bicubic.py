"""Bicubic-on-the-fly on device (csrc/bicubic.h) against fixture G20 -- the reference's own `imresize` outputs and
ImageSuperResolutionBicubicDataset items, written by tools/make_golden_bicubic.py -- and, at shapes the fixture does not hold,
against the numpy restatement tests/bicubic_ref.py (itself pinned to G20 by tests/test_bicubic_host.py).  No comparison carries a
tolerance: one grey level anywhere is a failure."""
import os
import random

import numpy as np
import pytest
import torch

from tests import bicubic_ref as BR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_bicubic.npz"))


def _hr_images(n, lo, hi, seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (int(g.integers(lo, hi)), int(g.integers(lo, hi)), 3), dtype=np.uint8) for _ in range(n)]


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_downscale_equals_the_reference_imresize(g20, scale):
    """k = 0: 48s x 52s, several tiles both ways and a ragged last tile column; 1: 37 x 50 binary, ragged sizes and the clip;
    2: 4s x 4s, multiple reflections in one partial tile; 3: low amplitude, .5 ties after pass 1 (x2, x4).  The fp32 output of the
    same launch is the uint8 one / 255, exactly, in NCHW."""
    from mobilesuperresolution_amd.datasets import bicubic_downscale
    assert int(g20[f"s{scale}_n_img"]) == 4 and (int(g20[f"s{scale}_ties"]) >= 1 or scale == 3)
    for k in range(4):
        img, exp = torch.from_numpy(g20[f"s{scale}_img{k}"]).cuda(), torch.from_numpy(g20[f"s{scale}_out{k}"])
        out = bicubic_downscale(img, scale)
        assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == tuple(exp.shape)
        assert torch.equal(out.cpu(), exp), (scale, k, int((out.cpu() != exp).sum()))
        out2, f32 = bicubic_downscale(img, scale, return_f32=True)
        assert torch.equal(out2.cpu(), exp), (scale, k)
        assert f32.dtype == torch.float32 and torch.equal(f32.cpu(), exp.permute(2, 0, 1).float().div(255)), (scale, k)


@pytest.mark.parametrize("scale,h,w", [(3, 131, 203), (4, 70, 301), (2, 33, 130)])
def test_downscale_equals_the_restatement_at_odd_sizes(scale, h, w):
    """no multiple of the scale or of the 16 x 32 tile; up to five tile rows and three tile columns"""
    from mobilesuperresolution_amd.datasets import bicubic_downscale
    img = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = bicubic_downscale(torch.from_numpy(img).cuda(), scale)
    assert torch.equal(out.cpu(), torch.from_numpy(BR.downscale(img, scale)))


def test_downscale_refuses_what_it_does_not_support():
    from mobilesuperresolution_amd.datasets import bicubic_downscale
    img = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        bicubic_downscale(img, 5)
    with pytest.raises(ValueError):
        bicubic_downscale(img.float(), 2)


def test_batch_equals_the_reference_dataset_items(g20):
    """every TRAIN item the reference's ImageSuperResolutionBicubicDataset.__getitem__ produced under a seeded `random` comes out
    of DeviceBicubicPatchCache.batch bit for bit -- ignored_boundary_size 1 (centre outputs whose taps reflect at the crop's
    edge) and 2 with num_patches 2, all eight flip / transpose combinations -- and the RNG has made the same draws afterwards"""
    from mobilesuperresolution_amd.datasets import DeviceBicubicPatchCache
    cfgs = g20["cfgs"].tolist()
    assert [c[2] for c in cfgs] == [1, 2] and cfgs[1][3] == 2
    for ci, (scale, P, ig, num_patches) in enumerate(cfgs):
        hrs = [g20[f"c{ci}_hr{k}"] for k in range(int(g20[f"c{ci}_n_img"]))]
        ds = DeviceBicubicPatchCache(hrs, P, scale, ig, num_patches)
        assert len(ds) == len(hrs) * num_patches
        idx = g20[f"c{ci}_idx"].tolist()
        probe = random.Random(int(g20[f"c{ci}_seed"]))
        assert {ds.draw(i, probe)[4] for i in idx} == set(range(8))
        rng = random.Random(int(g20[f"c{ci}_seed"]))
        lr, hr = ds.batch(idx, rng)
        assert torch.equal(lr.cpu(), torch.from_numpy(g20[f"c{ci}_lr_items"]).float().div(255)), ci
        assert torch.equal(hr.cpu(), torch.from_numpy(g20[f"c{ci}_hr_items"]).float().div(255)), ci
        assert rng.random() == float(g20[f"c{ci}_next_random"])


@pytest.mark.parametrize("scale,P,ig,num_patches", [(2, 40, 1, 2), (4, 20, 3, 1), (3, 17, 1, 3)])
def test_batch_equals_the_restatement_draw_for_draw(scale, P, ig, num_patches):
    """fresh seeds and patches of more than one tile (P > 16 rows, P > 32 columns), ragged last tiles"""
    from mobilesuperresolution_amd.datasets import DeviceBicubicPatchCache
    S = (P + 2 * ig) * scale
    hrs = _hr_images(3, S, S + 40, seed=S)
    ds = DeviceBicubicPatchCache(hrs, P, scale, ig, num_patches)
    idx = list(range(len(ds))) * 3
    lr, hr = ds.batch(idx, random.Random(77))
    assert tuple(lr.shape) == (len(idx), 3, P, P) and tuple(hr.shape) == (len(idx), 3, P * scale, P * scale)
    rng = random.Random(77)
    for b, i in enumerate(idx):
        _, _, x, y, flags = ds.draw(i, rng)
        el, eh = BR.train_item(hrs[i // num_patches], x, y, flags, P, scale, ig)
        assert torch.equal(lr[b].cpu(), torch.from_numpy(el).float().div(255)), (b, i, flags)
        assert torch.equal(hr[b].cpu(), torch.from_numpy(eh).float().div(255)), (b, i, flags)


def test_each_output_alone_is_unchanged():
    from mobilesuperresolution_amd.datasets import DeviceBicubicPatchCache
    ds = DeviceBicubicPatchCache(_hr_images(3, 60, 90, seed=4), 12, 4, 1, 2)
    idx = list(range(len(ds)))
    lr, hr = ds.batch(idx, random.Random(5))
    lr_only, none_hr = ds.batch(idx, random.Random(5), want_hr=False)
    none_lr, hr_only = ds.batch(idx, random.Random(5), want_lr=False)
    assert none_hr is None and none_lr is None
    assert torch.equal(lr_only, lr) and torch.equal(hr_only, hr)


def test_eval_item_equals_the_reference_eval_item(g20):
    """EVAL mode: HR cropped to multiples of the scale (37 x 50 is none of 2, 3, 4 in both directions at once), LR its downscale"""
    from mobilesuperresolution_amd.datasets import DeviceBicubicPatchCache
    for scale in (2, 3, 4):
        pad = np.zeros((40, 50, 3), dtype=np.uint8)                     # a second image: the item is cut at its own offset
        ds = DeviceBicubicPatchCache([pad, g20["eval_img"]], 4, scale, 1)
        lr, hr = ds.eval_item(1)
        el, eh = torch.from_numpy(g20[f"eval_s{scale}_lr"]), torch.from_numpy(g20[f"eval_s{scale}_hr"])
        assert lr.dtype == hr.dtype == torch.float32 and lr.is_cuda and hr.is_cuda
        assert torch.equal(lr.cpu(), el.float().div(255).unsqueeze(0)), scale
        assert torch.equal(hr.cpu(), eh.float().div(255).unsqueeze(0)), scale


def test_feeds_the_training_step():
    """batch -> BASIC_MODEL.train_step without leaving the device"""
    import argparse
    from mobilesuperresolution_amd.datasets import DeviceBicubicPatchCache
    from mobilesuperresolution_amd.models import get_model
    ds = DeviceBicubicPatchCache(_hr_images(4, 110, 140, seed=5), 24, 4, 1)
    torch.manual_seed(0)
    ns = argparse.Namespace(model_type="BASIC_MODEL", image_mean=0.5, num_channels=3, scale=4, num_blocks=2, num_residual_units=24,
                            hot_dtype="bf16")
    m = get_model(ns).cuda().train()
    st = m.make_train_state(1e-3)
    lr, hr = ds.batch(range(len(ds)), random.Random(0))
    l0 = m.train_step(lr, hr, st).item()
    for _ in range(20):
        l1 = m.train_step(lr, hr, st).item()
    assert l1 < l0
