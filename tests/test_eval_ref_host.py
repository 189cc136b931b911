"""tests/eval_ref.py, the float64 reference tests/test_gpu_eval_clip.py holds csrc/eval.h to, pinned on the CPU: its bilinear
baseline against torch's own `F.interpolate`, its psnr / psnr_y against the reference's values in fixture G9, its 8-bit
quantisation and the two variation statistics against the reference's expressions re-typed in torch -- and the condition
the GPU tests rest on: at most 0.1 % of the baseline samples of every seeded input are ambiguous."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eval_ref as R


@pytest.mark.parametrize("lr_shape,size,shave,align", R.CASES)
@pytest.mark.parametrize("align_override", [False, True])
def test_baseline_matches_torch_cpu_interpolate(lr_shape, size, shave, align, align_override):
    """max-abs <= 2^-20: torch's fp32 blend and the float64 one are both within 2^-21 of the exact blend of the same taps"""
    lr, _, _ = R.make_case(lr_shape, size)
    x = lr.reshape(-1, *lr_shape[-3:])
    exp = F.interpolate(torch.from_numpy(x), size, mode="bilinear", align_corners=align_override).numpy()
    got = R.baseline(x, *size, align_corners=align_override)
    err = np.abs(got - exp.astype(np.float64)).max()
    print(f"\n{lr_shape} -> {size} align_corners={align_override}: max|ref - torch| {err:.3e}")
    assert got.shape == exp.shape and err <= 2.0 ** -20


def test_baseline_non_integer_ratio_of_a_real_dataset_and_extra_channels():
    """NEMO's 240 x 426 -> 1080 x 1920 (a strip of it: the ratios are what matters) and lr with 5 channels: the first three"""
    g = torch.Generator().manual_seed(426)
    x = torch.rand(1, 5, 240, 20, generator=g)
    for align in (False, True):
        exp = F.interpolate(x, (1080, 90), mode="bilinear", align_corners=align)[:, :3].numpy()
        got = R.baseline(x.numpy(), 1080, 90, align_corners=align)
        assert np.abs(got - exp).max() <= 2.0 ** -20
    x = torch.rand(1, 3, 8, 426, generator=g)
    exp = F.interpolate(x, (36, 1920), mode="bilinear").numpy()
    assert np.abs(R.baseline(x.numpy(), 36, 1920) - exp).max() <= 2.0 ** -20


def test_taps_by_hand():
    i0, i1, l0, l1 = R.taps(8, 2, False)                     # x4: src = 0.25 (d + 0.5) - 0.5
    assert i0.tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and i1.tolist() == [1, 1, 1, 1, 1, 1, 1, 1]
    assert l1.tolist() == [0.0, 0.0, 0.125, 0.375, 0.625, 0.875, 0.125, 0.375]
    i0, i1, l0, l1 = R.taps(5, 3, True)                      # src = d / 2
    assert i0.tolist() == [0, 0, 1, 1, 2] and i1.tolist() == [1, 1, 2, 2, 2] and l1.tolist() == [0.0, 0.5, 0.0, 0.5, 0.0]
    i0, i1, l0, l1 = R.taps(1, 7, True)                      # out == 1: scale 0
    assert i0.tolist() == [0] and l0.tolist() == [1.0]
    assert all(a.dtype == np.float32 for a in (l0, l1))


def test_psnr_and_psnr_y_match_the_reference_values_of_g9(golden_dir):
    """G9 holds common/metrics.py's own results (fp32, SUMMED over the batch); 1e-4 dB as tests/test_oracle_golden.py"""
    z = np.load(os.path.join(golden_dir, "g9_metrics.npz"))
    seen_y = 0
    for k in range(int(z["n_cases"])):
        sr, hr, shave = z[f"sr_{k}"], z[f"hr_{k}"], int(z[f"shave_{k}"])
        assert R.psnr(sr, hr, shave).sum() == pytest.approx(float(z[f"psnr_{k}"]), abs=1e-4), k
        if sr.shape[1] == 3:
            assert R.psnr_y(sr, hr, shave).sum() == pytest.approx(float(z[f"psnr_y_{k}"]), abs=1e-4), k
            seen_y += 1
    assert seen_y >= 2
    assert np.isnan(R.psnr(z["sr_0"], z["hr_0"], 20)).all() and np.isnan(R.psnr_y(z["sr_0"], z["hr_0"], 20)).all()


def test_charbonnier_matches_the_reference_expression():
    _, hr, sr = R.make_case((1, 3, 3, 16, 20), (64, 80))
    s, t = torch.from_numpy(sr[0]).double(), torch.from_numpy(hr[0]).double()
    for f in range(3):
        d = torch.add(s[f], -t[f])
        assert R.charbonnier(sr[0], hr[0])[f] == pytest.approx(float(torch.mean(torch.sqrt(d * d + 1e-12))), rel=1e-12)


def test_quant_u8_matches_the_torch_expression():
    g = torch.Generator().manual_seed(8)
    x = torch.cat([torch.rand(4000, generator=g) * 1.2 - 0.1, torch.arange(256.0) / 255, (torch.arange(255.0) + 0.5) / 255,
                   torch.tensor([-1.0, 0.0, 1.0, 2.0, 0.99999994, 0.998, 0.9981])])
    exp = x.clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    assert np.array_equal(R.quant_u8(x.numpy()), exp)
    assert np.array_equal(R.quant_u8(x.double().numpy()), x.double().clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy())
    a = np.arange(24, dtype=np.float32).reshape(1, 3, 2, 4)
    assert R.to_hwc(a).shape == (1, 2, 4, 3) and R.to_hwc(a)[0, 1, 2].tolist() == [6.0, 14.0, 22.0]


def _torch_total_variation(img):
    B, N, C, H, W = img.shape
    img = img.view(B * N, C, H, W)
    img_ = F.pad(img, (0, 1, 0, 1), "replicate")
    img_h = img_[:, :, 1:, :-1]
    img_w = img_[:, :, :-1, 1:]
    return torch.sum(torch.abs(img_h - img) + torch.abs(img_w - img), dim=[-1, -2, -3])


def _torch_time_variation(img):
    B, N, C, H, W = img.shape
    img_1 = img[:, 1:, :, :, :]
    img_0 = img[:, :-1, :, :, :]
    tv_ = torch.sum(torch.abs(img_1 - img_0), dim=[-3, -2, -1])
    tv = torch.zeros((B, N), dtype=img.dtype)
    tv[:, :-1] += tv_
    tv[:, 1:] += tv_
    tv[:, 0] = tv[:, 0] * 2
    tv[:, -1] = tv[:, -1] * 2
    return tv.view(B * N)


@pytest.mark.parametrize("shape", [(2, 35, 3, 5, 6), (1, 1, 3, 60, 107), (1, 2, 3, 9, 11), (2, 3, 4, 7, 5)])
def test_variation_matches_the_by_patch_expressions(shape):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(sum(shape)), dtype=torch.float64)
    np.testing.assert_allclose(R.total_variation(x.numpy()), _torch_total_variation(x).numpy(), rtol=1e-12)
    np.testing.assert_allclose(R.time_variation(x.numpy()), _torch_time_variation(x).numpy(), rtol=1e-12, atol=0)
    if shape[1] == 1:
        assert not R.time_variation(x.numpy()).any()


def test_time_variation_by_hand():
    x = np.zeros((1, 4, 1, 1, 1))
    x[0, :, 0, 0, 0] = [0.0, 1.0, 3.0, 7.0]                  # d = 1, 2, 4
    assert R.time_variation(x).tolist() == [2.0, 3.0, 6.0, 8.0]
    assert R.time_variation(x[:, :2]).tolist() == [2.0, 2.0]


@pytest.mark.parametrize("lr_shape,size,shave,align", R.CASES)
def test_ambiguous_share_of_every_gpu_input_is_small(lr_shape, size, shave, align):
    """the condition of the GPU tests: <= 0.1 % ambiguous baseline samples (expected for uniform lr: 2 M = 0.05 %)"""
    lr, _, _ = R.make_case(lr_shape, size)
    amb = R.ambiguous(R.baseline(lr.reshape(-1, *lr_shape[-3:]), *size, align_corners=align))
    print(f"\n{lr_shape} -> {size}: {amb.sum()} of {amb.size} ambiguous ({100 * amb.mean():.4f} %)")
    assert amb.mean() <= R.AMBIGUOUS_CAP


def test_interval_brackets_the_plain_value_and_widens_only_at_ambiguous_samples():
    lr, hr, _ = R.make_case((1, 3, 3, 16, 20), (64, 80))
    b = R.baseline(lr[0], 64, 80)
    lo, hi, s_lo, s_hi = R.baseline_psnr_interval(b, hr[0], 4)
    mid = R.psnr(b, hr[0], 4)
    assert (s_lo <= s_hi).all() and (lo <= mid + 1e-12).all() and (mid <= hi + 1e-12).all() and (hi - lo < 1e-3).all()
    b2 = (np.floor(b * 255.0) + 0.25) / 255.0                # nowhere near a rounding point: the interval is a point
    lo, hi, s_lo, s_hi = R.baseline_psnr_interval(b2, hr[0], 4)
    assert not R.ambiguous(b2).any() and np.array_equal(s_lo, s_hi) and np.allclose(lo, R.psnr(b2, hr[0], 4), atol=1e-12)
    b3 = (np.floor(b * 255.0) + 0.5) / 255.0                 # every sample on one
    lo, hi, s_lo, s_hi = R.baseline_psnr_interval(b3, hr[0], 4)
    assert R.ambiguous(b3).all() and (s_lo < s_hi).all()
