"""`metrics.ssim` (csrc/ssim.h) against tests/ssim_ref.py, the float64 restatement of the reference's `ssim`
(common/metrics.py:41-68) that tests/test_ssim_ref_host.py pins.

Tolerance: 1e-9 absolute per image.  The device path is double from the filter on (a few hundred roundings per pixel and
a mean of values <= 1: ~1e-13), so 1e-9 is margin for the order of the sums only, and 100 times below what one fp32 ulp
of luma or an fp32 filter pass would show.  Shapes: the smallest that reach one output pixel, a ragged thin tile, a batch,
several 32 x 32 tiles with seams on both axes, 5-D and 3-D input."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import ssim_ref as SR

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _n_images(shape):
    return int(np.prod(shape[:-3])) if len(shape) > 3 else 1


def _check(sr, hr, shave, what=""):
    from mobilesuperresolution_amd.metrics import ssim
    got = ssim(sr.cuda(), hr.cuda(), shave=shave)
    exp = SR.ssim_ref(sr.numpy(), hr.numpy(), shave)
    n = _n_images(tuple(sr.shape))
    print(f"\n{what}{tuple(sr.shape)} shave {shave}: device {float(got):.15f} ref {exp:.15f} |d| {abs(float(got) - exp):.2e}")
    assert abs(float(got) - exp) <= TOL * n
    return got


@pytest.mark.parametrize("shape,shave", [((1, 3, 19, 19), 4), ((1, 3, 21, 40), 1), ((2, 3, 60, 85), 4), ((1, 3, 150, 131), 2),
                                         ((2, 2, 3, 30, 34), 4), ((3, 40, 44), 4)])
def test_device_ssim_matches_float64_reference(shape, shave):
    g = torch.Generator().manual_seed(sum(shape))
    hr = torch.rand(shape, generator=g)
    sr = hr + 0.05 * torch.randn(shape, generator=g) + 0.3 * (torch.rand(shape, generator=g) > 0.97)    # some values leave [0, 1]
    _check(sr, hr, shave)


def test_device_ssim_on_a_smooth_image():
    """small variances: uxx - ux^2 cancels, which an fp32 filter would not survive"""
    h, w = 64, 80
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    base = 0.5 + 0.4 * torch.sin(x / 7) * torch.cos(y / 5)
    hr = torch.stack([base, 0.8 * base, 0.6 * base])[None]
    sr = hr + 0.02 * torch.randn(hr.shape, generator=torch.Generator().manual_seed(64))
    _check(sr, hr, 4, "smooth ")


def test_device_ssim_hand_cases():
    from mobilesuperresolution_amd.metrics import ssim
    g = torch.Generator().manual_seed(5)
    hr = torch.randint(0, 256, (1, 3, 40, 44), generator=g).float() / 255          # on the 8-bit grid: quantising changes nothing
    assert abs(float(ssim(hr.cuda(), hr.cuda(), shave=4)) - 1.0) <= TOL
    sr, hr = torch.full((1, 3, 30, 34), 100.0 / 255.0), torch.full((1, 3, 30, 34), 0.7)
    a, b = float(SR.luma(SR.quantise(sr.numpy()))[0, 0, 0]), float(SR.luma(hr.numpy())[0, 0, 0])
    got = float(ssim(sr.cuda(), hr.cuda(), shave=4))
    assert abs(got - (2 * a * b + SR.C1) / (a * a + b * b + SR.C1)) <= TOL
    assert abs(got - 0.85282794548016) <= TOL


def test_device_ssim_quantises_half_way_values_as_the_reference():
    """sr at (k + 0.5) / 255: the fp32 product with 255 is a tie for many k (round half to even), a neighbour for the rest"""
    h, w = 24, 32
    k = (torch.arange(3 * h * w) * 7 % 255).reshape(1, 3, h, w)
    sr = ((k.double() + 0.5) / 255.0).float()
    ties = (sr * 255 == k + 0.5)
    assert ties.any() and (ties & (k % 2 == 1)).any() and (ties & (k % 2 == 0)).any()
    hr = torch.rand(sr.shape, generator=torch.Generator().manual_seed(24))
    _check(sr, hr, 2, "half-way ")


def test_device_ssim_is_deterministic_and_a_float64_scalar_on_device():
    from mobilesuperresolution_amd.metrics import ssim
    g = torch.Generator().manual_seed(11)
    hr = torch.rand((2, 3, 90, 101), generator=g).cuda()
    sr = (hr + 0.05 * torch.randn(hr.shape, generator=g).cuda())
    a, b = ssim(sr, hr, shave=3), ssim(sr, hr, shave=3)
    assert a.dim() == 0 and a.dtype == torch.float64 and a.device == sr.device
    assert torch.equal(a, b)


def test_device_ssim_errors():
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.metrics import ssim
    x = torch.rand(1, 3, 32, 32).cuda()
    with pytest.raises(L.HotpathError):
        ssim(x.cpu(), x.cpu())
    with pytest.raises(L.HotpathError):
        ssim(x, x.cpu())
    with pytest.raises(ValueError):
        ssim(x[0, 0], x[0, 0])                        # fewer than 3 dims
    with pytest.raises(ValueError):
        ssim(x, x[..., :31])                          # shapes differ
    with pytest.raises(ValueError):
        ssim(x[:, :1], x[:, :1])                      # 1 channel
    with pytest.raises(ValueError):
        ssim(torch.cat([x, x], 1), torch.cat([x, x], 1))
    with pytest.raises(ValueError):
        ssim(x, x, shave=0)                           # the reference's [0:-0] is empty
    with pytest.raises(ValueError):
        ssim(x, x, shave=11)                          # 32 - 22 = 10 < win_size
    with pytest.raises(ValueError):
        ssim(x[..., :18], x[..., :18], shave=4)       # one side only
    with pytest.raises(NotImplementedError):
        ssim(x, x.double())
    assert 0.0 < float(ssim(x.half(), x, shave=4)) <= 1.0      # sr is cast to hr's dtype, as in the reference
    # the C entry itself: a cropped side of 10, shave 0, null pointers
    part, out = torch.zeros(4, dtype=torch.float64).cuda(), torch.zeros((), dtype=torch.float64).cuda()
    f, st = L.lib().sr_ssim, L.stream_ptr()
    assert f(x.data_ptr(), x.data_ptr(), part.data_ptr(), out.data_ptr(), 1, 32, 32, 11, 4, st) == -2
    assert f(x.data_ptr(), x.data_ptr(), part.data_ptr(), out.data_ptr(), 1, 32, 18, 4, 4, st) == -2
    assert f(x.data_ptr(), x.data_ptr(), part.data_ptr(), out.data_ptr(), 1, 32, 32, 0, 4, st) == -2
    assert f(x.data_ptr(), x.data_ptr(), part.data_ptr(), out.data_ptr(), 0, 32, 32, 4, 4, st) == -2
    assert f(None, x.data_ptr(), part.data_ptr(), out.data_ptr(), 1, 32, 32, 4, 4, st) == -2
    assert f(x.data_ptr(), x.data_ptr(), None, out.data_ptr(), 1, 32, 32, 4, 4, st) == -2
    assert f(x.data_ptr(), x.data_ptr(), part.data_ptr(), out.data_ptr(), 1, 32, 32, 4, 0, st) == -2   # partial too small
    assert f(x.data_ptr(), x.data_ptr(), part.data_ptr(), out.data_ptr(), 1, 32, 32, 4, 1, st) == 0


def test_three_metrics_of_the_evaluation_loop_without_leaving_the_device(golden_dir):
    """utils/estimate.py:123-128 on the first Set5-shaped image of G13: model output, tiling, psnr, psnr_y and ssim stay on
    the GPU; ssim against the float64 reference on the same sr copied to the host"""
    from oracle.set5_like import SET5_SHAPES, set5_like_hr
    from mobilesuperresolution_amd.inference import tiled_forward
    from mobilesuperresolution_amd.metrics import psnr, psnr_y, ssim
    from mobilesuperresolution_amd.models import get_model
    z = np.load(os.path.join(golden_dir, "g13_set5_shaped.npz"))
    g3 = np.load(os.path.join(golden_dir, "g3_pretrained_x2_8_24.npz"))
    ns = argparse.Namespace(model_type="BASIC_MODEL", image_mean=0.5, num_channels=3, scale=2, num_blocks=8,
                            num_residual_units=24, hot_dtype="fp32")
    m = get_model(ns)
    m.load_state_dict({k[2:]: torch.from_numpy(g3[k]) for k in g3.files if k.startswith("p/")})
    m = m.cuda().eval()
    hw = SET5_SHAPES[0]
    hr = set5_like_hr(0, hw)
    hr = hr[:, :hw[0] - hw[0] % 2, :hw[1] - hw[1] % 2][None].cuda()
    lr = torch.from_numpy(z["lr_x2_0"]).float().cuda()
    sr = tiled_forward(m, lr, tile=64)
    assert abs(float(psnr(sr, hr, shave=2 + 6)) - float(z["psnr_x2_0"])) <= 1e-3
    assert abs(float(psnr_y(sr, hr, shave=2)) - float(z["psnr_y_x2_0"])) <= 1e-3
    got = float(ssim(sr, hr, shave=2))
    exp = SR.ssim_ref(sr.cpu().numpy(), hr.cpu().numpy(), 2)
    print(f"\nG13 image 0 {tuple(sr.shape)}: ssim device {got:.15f} ref {exp:.15f} |d| {abs(got - exp):.2e}")
    assert 0.0 < got < 1.0 and abs(got - exp) <= TOL
