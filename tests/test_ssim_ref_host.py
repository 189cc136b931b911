"""tests/ssim_ref.py, the float64 restatement of the reference's `ssim` that csrc/ssim.h is held against
(tests/test_gpu_ssim.py), pinned before it is used: its "valid" filter against scipy's gaussian_filter(mode='reflect') on
the full cropped image followed by skimage's 5-pixel crop, and hand cases that need no library."""
import numpy as np
import pytest

from tests import ssim_ref as SR


def _images(shape, seed):
    g = np.random.default_rng(seed)
    hr = g.random(shape, dtype=np.float32)
    sr = (hr + 0.05 * g.standard_normal(shape) + 0.3 * (g.random(shape) > 0.97)).astype(np.float32)   # some leave [0, 1]
    return sr, hr


@pytest.mark.parametrize("hw,shave", [((19, 19), 4), ((60, 85), 4), ((150, 131), 2)])
def test_valid_form_equals_scipy_reflect_filter_and_crop(hw, shave):
    ndi = pytest.importorskip("scipy.ndimage")
    sr, hr = _images((3,) + hw, seed=hw[0] * hw[1])
    r = SR.RADIUS
    got = SR.ssim_ref(sr, hr, shave)
    exp = SR.ssim_ref(sr, hr, shave,
                      filt=lambda a: ndi.gaussian_filter(a, sigma=SR.SIGMA, truncate=3.5, mode="reflect")[r:-r, r:-r])
    print(f"\n{hw} shave {shave}: valid {got:.16f} scipy {exp:.16f} |d| {abs(got - exp):.1e}")
    assert 0.0 < got < 1.0 and abs(got - exp) <= 1e-12


def test_window_is_scipys_gaussian_kernel():
    w = SR.window()
    assert w.shape == (11,) and w.dtype == np.float64 and abs(w.sum() - 1.0) <= 1e-15 and np.array_equal(w, w[::-1])
    assert w[5] / w[4] == pytest.approx(np.exp(0.5 / 2.25), rel=1e-14) and w[5] / w[0] == pytest.approx(np.exp(12.5 / 2.25), rel=1e-14)


def test_identical_images_give_one():
    g = np.random.default_rng(5)
    hr = (g.integers(0, 256, (3, 40, 44)).astype(np.float32) / np.float32(255))        # on the 8-bit grid: sr == quantise(sr)
    assert np.array_equal(SR.quantise(hr), hr)
    assert abs(SR.ssim_ref(hr, hr, 4) - 1.0) <= 1e-12
    assert abs(SR.ssim_ref(np.stack([hr, hr]), np.stack([hr, hr]), 4) - 2.0) <= 2e-12     # more than one image: summed


def test_two_constant_images():
    sr, hr = np.full((3, 30, 34), 100.0 / 255.0, np.float32), np.full((3, 30, 34), 0.7, np.float32)
    a, b = float(SR.luma(SR.quantise(sr))[0, 0]), float(SR.luma(hr)[0, 0])
    got = SR.ssim_ref(sr, hr, 4)
    assert abs(got - (2 * a * b + SR.C1) / (a * a + b * b + SR.C1)) <= 1e-12
    assert abs(got - 0.85282794548016) <= 1e-12


def test_quantisation_rounds_half_to_even_and_clamps():
    k = np.arange(0, 255)
    v = ((k + 0.5) / 255.0).astype(np.float32)
    p = v * np.float32(255)                                  # the float32 product the reference rounds
    tie = p == (k + np.float32(0.5))
    assert tie[k % 2 == 0].any() and tie[k % 2 == 1].any()   # exact ties of both parities are among them
    n = np.where(tie, k + (k % 2), np.where(p > k + 0.5, k + 1, k)).astype(np.float32)
    assert np.array_equal(SR.quantise(v), n / np.float32(255))
    assert SR.quantise(np.float32(0.5 / 255)) == 0.0 and SR.quantise(np.float32(1.5 / 255)) == np.float32(2) / np.float32(255)
    assert np.array_equal(SR.quantise(np.float32([-0.3, -1e-3, 1.0 + 1e-3, 1.7])), np.float32([0, 0, 1, 1]))


def test_luma_is_three_float32_products_added_in_float32():
    g = np.random.default_rng(9)
    img = g.random((3, 8, 8), dtype=np.float32)
    c = [np.float32(65.738) / np.float32(256), np.float32(129.057) / np.float32(256), np.float32(25.064) / np.float32(256)]
    exp = np.float32(np.float32(np.float32(img[0] * c[0]) + np.float32(img[1] * c[1])) + np.float32(img[2] * c[2]))
    assert np.array_equal(SR.luma(img), exp)
    wide = (img[0].astype(np.float64) * c[0] + img[1].astype(np.float64) * c[1] + img[2].astype(np.float64) * c[2])
    assert (SR.luma(img).astype(np.float64) != wide).any()   # and not a wider sum rounded once
