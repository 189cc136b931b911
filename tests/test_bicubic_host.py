"""Bicubic-on-the-fly, host side: the tables, the numpy restatement and the draw logic against fixture G20, which
tools/make_golden_bicubic.py wrote from the reference's own `imresize`, `contributions` and ImageSuperResolutionBicubicDataset.
Every comparison is exact."""
import os
import random

import numpy as np
import pytest

from tests import bicubic_ref as BR


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_bicubic.npz"))


def test_tables_equal_the_reference_contributions_bitwise(g20):
    from mobilesuperresolution_amd.packing import bicubic_tables
    keys = g20["table_keys"].tolist()
    assert {s for s, _ in keys} == {2, 3, 4}
    for scale, n in keys:
        w, i = bicubic_tables(n, scale)
        ew, ei = g20[f"tab_s{scale}_n{n}_w"], g20[f"tab_s{scale}_n{n}_i"]
        assert w.dtype == np.float64 and i.dtype == np.int32 and w.shape == ew.shape == i.shape == (-(-n // scale), w.shape[1])
        assert np.array_equal(w.view(np.int64), ew.view(np.int64)), (scale, n)        # bit patterns, not values
        assert np.array_equal(i, ei), (scale, n)
        assert w.shape[1] <= 4 * scale + 2
    assert {s: bicubic_tables(48 * s, s)[0].shape[1] for s in (2, 3, 4)} == {2: 8, 3: 9, 4: 16}


def test_tables_refuse_other_scales():
    from mobilesuperresolution_amd.packing import bicubic_tables
    for scale in (1, 5, 8):
        with pytest.raises(ValueError):
            bicubic_tables(64, scale)


def test_restatement_equals_every_reference_output(g20):
    for scale in g20["scales"].tolist():
        shapes = []
        for k in range(int(g20[f"s{scale}_n_img"])):
            img, exp = g20[f"s{scale}_img{k}"], g20[f"s{scale}_out{k}"]
            shapes.append(img.shape[:2])
            assert np.array_equal(BR.downscale(img, scale), exp), (scale, k)
        assert shapes == [(48 * scale, 52 * scale), (37, 50), (4 * scale, 4 * scale), (16 * scale, 20 * scale)]
        # the low-amplitude image really holds ties that tell round-half-even from round-half-up (x3 has no exact ties)
        ties = BR.half_even_ties(g20[f"s{scale}_img3"], scale)
        assert ties == int(g20[f"s{scale}_ties"])
        assert ties >= 1 or scale == 3
        hr = g20[f"eval_s{scale}_hr"].transpose(1, 2, 0)
        assert hr.shape[:2] == (37 - 37 % scale, 50 - 50 % scale) and np.array_equal(hr, g20["eval_img"][:hr.shape[0], :hr.shape[1]])
        assert np.array_equal(BR.downscale(hr, scale).transpose(2, 0, 1), g20[f"eval_s{scale}_lr"])


def test_draws_consume_the_rng_like_the_reference(g20):
    """`bicubic_patch_draw` (what DeviceBicubicPatchCache.draw calls, usable without a device) returns, item by item, what the
    reference's randrange / random calls returned, leaves the generator where the reference left it, and the draws are the ones
    that make the stored items"""
    from mobilesuperresolution_amd.datasets import bicubic_patch_draw
    for ci, (scale, P, ig, num_patches) in enumerate(g20["cfgs"].tolist()):
        hrs = [g20[f"c{ci}_hr{k}"] for k in range(int(g20[f"c{ci}_n_img"]))]
        S = (P + 2 * ig) * scale
        rng = random.Random(int(g20[f"c{ci}_seed"]))
        seen = set()
        for b, i in enumerate(g20[f"c{ci}_idx"].tolist()):
            hr = hrs[i // num_patches]
            x, y, flags = bicubic_patch_draw(hr.shape[0], hr.shape[1], S, rng)
            ex, ey, r1, r2, r3 = g20[f"c{ci}_draws"][b].tolist()
            assert (x, y) == (ex, ey) and flags == (r1 < 0.5) | (r2 < 0.5) << 1 | (r3 < 0.5) << 2, (ci, b)
            seen.add(flags)
            lr_item, hr_item = BR.train_item(hr, x, y, flags, P, scale, ig)
            assert np.array_equal(lr_item, g20[f"c{ci}_lr_items"][b]) and np.array_equal(hr_item, g20[f"c{ci}_hr_items"][b]), (ci, b)
        assert seen == set(range(8))
        assert rng.random() == float(g20[f"c{ci}_next_random"])
    assert g20["cfgs"][0, 2] == 1 and g20["cfgs"][1, 2] == 2 and g20["cfgs"][1, 3] == 2


def test_cache_refuses_what_the_reference_cannot_do():
    """checked before anything is allocated on a device"""
    from mobilesuperresolution_amd.datasets import DeviceBicubicPatchCache
    img = np.zeros((80, 90, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="ignored_boundary_size"):
        DeviceBicubicPatchCache([img], 8, 4, 0)                       # the reference's [0:-0] slices are empty
    with pytest.raises(ValueError, match="smaller"):
        DeviceBicubicPatchCache([img, img[:39]], 8, 4, 1)             # S = (8 + 2) * 4 = 40 > 39 rows
    with pytest.raises(ValueError, match="smaller"):
        DeviceBicubicPatchCache([img[:, :39]], 8, 4, 1)
    with pytest.raises(ValueError, match="scale"):
        DeviceBicubicPatchCache([img], 8, 5, 1)
    with pytest.raises(ValueError):
        DeviceBicubicPatchCache([img.astype(np.float32)], 8, 4, 1)


def test_downscale_has_no_cpu_fallback():
    import torch
    from mobilesuperresolution_amd import _lib
    from mobilesuperresolution_amd.datasets import DeviceBicubicPatchCache, bicubic_downscale
    with pytest.raises(_lib.HotpathError):
        bicubic_downscale(torch.zeros((8, 8, 3), dtype=torch.uint8), 2)
    with pytest.raises(_lib.HotpathError):
        DeviceBicubicPatchCache([np.zeros((80, 90, 3), dtype=np.uint8)], 8, 4, 1, device="cpu")


def test_entry_points_refuse_unsupported_arguments():
    """the argument checks come before any launch, so they can be called without a device: scale outside {2, 3, 4}, ig < 1, NULL tables"""
    from mobilesuperresolution_amd import _lib, build
    build.build()
    h = _lib.lib()
    one = 0x1000                                                      # never dereferenced on these paths
    assert h.sr_bicubic_resize_u8(one, one, None, None, 8, 8, 5, one, one, 8, one, one, 8, None) == -1
    assert h.sr_bicubic_resize_u8(one, one, None, None, 8, 8, 1, one, one, 8, one, one, 8, None) == -1
    assert h.sr_bicubic_resize_u8(one, one, None, None, 8, 8, 2, None, one, 8, one, one, 8, None) == -2
    assert h.sr_bicubic_resize_u8(one, one, None, None, 8, 8, 2, one, one, 8, one, None, 8, None) == -2
    assert h.sr_bicubic_resize_u8(one, None, None, None, 8, 8, 2, one, one, 8, one, one, 8, None) == -2
    assert h.sr_bicubic_resize_u8(one, one, None, None, 8, 8, 4, one, one, 19, one, one, 16, None) == -2
    assert h.sr_bicubic_patch_gather(one, one, one, one, 4, 8, 6, 1, one, one, 16, None) == -1
    assert h.sr_bicubic_patch_gather(one, one, one, one, 4, 8, 4, 0, one, one, 16, None) == -2
    assert h.sr_bicubic_patch_gather(one, one, one, one, 4, 8, 4, 1, None, one, 16, None) == -2
    assert h.sr_bicubic_patch_gather(one, one, one, one, 4, 8, 4, 1, one, None, 16, None) == -2
    assert h.sr_bicubic_patch_gather(one, one, None, None, 4, 8, 4, 1, one, one, 16, None) == -2
