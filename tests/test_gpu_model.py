"""Whole-model parity of the MI355X hot path (BASIC_MODEL through the C ABI) against the reference's
golden vectors: G1 (C1 model fwd + L1 + bwd), G3 (shipped x2 checkpoint), plus PixelShuffle
bit-exactness and the error conventions of the boundary."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

from oracle import wdsr_oracle as O

pytestmark = pytest.mark.gpu


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _ns(**kw):
    ns = argparse.Namespace(model_type="BASIC_MODEL", image_mean=0.5, num_channels=3, scale=4, num_blocks=4,
                            num_residual_units=24, hot_dtype="fp32")
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _model(ns, sd=None):
    from mobilesuperresolution_amd.models import get_model
    m = get_model(ns)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda()


def test_g1_fp32_forward_backward_matches_reference(golden_dir):
    d = _load(golden_dir, "g1_basic_model_c1.npz")
    sd = {k[2:]: v for k, v in d.items() if k.startswith("p/")}
    m = _model(_ns(), sd).train()
    y = m(d["x"].cuda())
    assert y.shape == (1, 3, 192, 192) and y.dtype == torch.float32
    err = (y.detach().cpu() - d["y"]).abs().max().item()
    scale = d["y"].abs().max().item()
    print(f"\nG1 fwd max|diff| {err:.3e} (scale {scale:.2f})")
    assert err <= 2e-5 * scale
    loss = torch.nn.functional.l1_loss(y, d["hr"].cuda())
    assert abs(loss.item() - d["loss"].item()) <= 1e-5 * abs(d["loss"].item())
    loss.backward()
    worst = 0.0
    gflat = m.flat.grad.cpu()
    assert [n for n, _ in m.named_parameters()] == ["flat"]
    for k, (off, shape) in m.layout.entries.items():
        exp = d["g/" + k]
        got = gflat[off:off + exp.numel()].view(shape)
        e = (got - exp).abs().max().item() / max(exp.abs().max().item(), 1e-12)
        worst = max(worst, e)
        assert e <= 2e-4, (k, e)
    print(f"G1 bwd worst relative grad error {worst:.2e}")
    # PSNR parity (north star: <= 1e-3 dB): same weights, same LR input
    ref_psnr = O.psnr_y(d["y"], d["hr"], shave=4).item()
    got_psnr = O.psnr_y(y.detach().cpu(), d["hr"], shave=4).item()
    print(f"psnr_y ref {ref_psnr:.5f} dB, hot path {got_psnr:.5f} dB")
    assert abs(ref_psnr - got_psnr) <= 1e-3


def test_g1_bf16_forward_tolerance(golden_dir):
    d = _load(golden_dir, "g1_basic_model_c1.npz")
    sd = {k[2:]: v for k, v in d.items() if k.startswith("p/")}
    m = _model(_ns(hot_dtype="bf16"), sd).eval()
    with torch.no_grad():
        y = m(d["x"].cuda()).cpu()
    mse = (y - d["y"]).pow(2).mean().item()
    peak = d["y"].abs().max().item()          # this fixture's outputs reach |13|, not [0,1]
    psnr = 10 * math.log10(peak * peak / mse)
    print(f"\nbf16 vs reference output: {psnr:.1f} dB relative to the signal peak {peak:.1f}")
    assert psnr >= 50.0          # tolerance of bf16 storage / bf16 MFMA operands with fp32 accumulation


def test_g3_pretrained_x2_checkpoint(golden_dir):
    d = _load(golden_dir, "g3_pretrained_x2_8_24.npz")
    sd = {k[2:]: v for k, v in d.items() if k.startswith("p/")}
    m = _model(_ns(scale=2, num_blocks=8), sd).eval()
    assert m.scale == 2
    with torch.no_grad():
        y = m(d["x"].cuda()).cpu()
    assert y.shape == d["y"].shape == (1, 3, 80, 112)
    err = (y - d["y"]).abs().max().item()
    print(f"\nG3 (x2, 8 blocks, shipped weights) max|diff| {err:.3e}")
    assert err <= 2e-5 * d["y"].abs().max().item()
    assert abs(O.psnr_y(y, d["y"].clamp(0, 1), shave=2).item()) > 60 or err < 1e-5


@pytest.mark.parametrize("r", [2, 3, 4])
def test_pixel_shuffle_indexing_bit_exact(r):
    """Tail weights that copy feature channel (ch mod F) to conv channel ch: the fused epilogue must then
    equal nn.PixelShuffle applied to that tensor bit for bit (law: models/basic_wdsr_b.py:80-83)."""
    from mobilesuperresolution_amd import hotpath as HP
    f, n, h, w = 24, 2, 13, 29
    co = 3 * r * r
    g = torch.Generator().manual_seed(r)
    feat = torch.randint(-512, 512, (n, h, w, f), generator=g).float() / 8.0     # exact in fp32
    wt = torch.zeros(co, f, 3, 3)
    for ch in range(co):
        wt[ch, ch % f, 1, 1] = 1.0
    src_t = HP.tail_src(wt, torch.zeros(co, 3, 5, 5), torch.zeros(co)).cuda()
    src_h = HP.head_src(torch.zeros(f, 3, 3, 3), torch.zeros(f)).cuda()
    _, blob_t = HP.pack_ends(src_h, src_t, f, r, torch.float32)
    x = torch.rand(n, 3, h, w, generator=g).cuda()
    out = torch.full((n, 3, r * h, r * w), float("nan"), device="cuda")
    HP.tail_fwd(feat.cuda().contiguous(), x, out, blob_t, 0.5, r)
    conv = feat.permute(0, 3, 1, 2)[:, [ch % f for ch in range(co)]]
    assert torch.equal(out.cpu(), torch.nn.functional.pixel_shuffle(conv, r))
    assert torch.equal(out.cpu(), O.pixel_shuffle(conv, r))


def test_full_size_batch_property_and_state_dict_roundtrip():
    """BASELINE C2 shape (16 blocks / 24 units, batch 32, 48x48): batch independence + determinism."""
    torch.manual_seed(0)
    m = _model(_ns(num_blocks=16, hot_dtype="bf16")).eval()
    x = torch.rand(32, 3, 48, 48, device="cuda")
    with torch.no_grad():
        y = m(x)
        y2 = m(x)
        y_half = m(x[16:])
    assert y.shape == (32, 3, 192, 192) and torch.isfinite(y).all()
    assert torch.equal(y, y2) and torch.equal(y[16:], y_half)
    keys = list(m.state_dict().keys())
    assert len(keys) == 153 and "body.15.body.3.weight_v" in keys and "skip.0.weight_g" in keys


def test_boundary_errors():
    from mobilesuperresolution_amd import _lib as L
    m = _model(_ns())
    with pytest.raises(L.HotpathError):
        m.cpu()(torch.rand(1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        _model(_ns(num_residual_units=48))
    with pytest.raises(NotImplementedError):
        from mobilesuperresolution_amd.models import get_model
        get_model(_ns(model_type="Result_Model"))


def test_ddp_rccl_single_rank_step():
    """DistributedDataParallel over RCCL (backend 'nccl') wraps the flat-parameter model and steps, as
    pretrain.py:157,239 does; world_size 1 here (one GPU per box), world 2 semantics are covered on gloo."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        torch.manual_seed(0)
        m = _model(_ns(num_blocks=2, hot_dtype="bf16")).train()
        ref_flat = m.flat.detach().clone()
        ddp = torch.nn.parallel.DistributedDataParallel(m, device_ids=[0], gradient_as_bucket_view=True)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        x = torch.rand(4, 3, 24, 24, device="cuda")
        hr = torch.rand(4, 3, 96, 96, device="cuda")
        losses = []
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.l1_loss(ddp(x), hr)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        assert m.flat.grad is not None and torch.isfinite(m.flat.grad).all()
        assert not torch.equal(m.flat.detach(), ref_flat) and losses[-1] < losses[0]
        assert len(ddp.state_dict()) == 3 * (3 * 2 + 3) and "module.skip.0.weight_v" in ddp.state_dict()
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------
# edge cases and the other BASELINE configs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 12, 24), (1, 13, 25), (3, 48, 48), (1, 37, 91)])
def test_ragged_and_tiny_images_vs_oracle(shape):
    """images smaller than / not a multiple of the 12x24 workgroup tile, batch 1..3"""
    n, h, w = shape
    torch.manual_seed(11)
    ns = _ns(num_blocks=2)
    m = _model(ns).train()
    ref = O.OracleBasicModel(ns)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    x = torch.rand(n, 3, h, w)
    hr = torch.rand(n, 3, 4 * h, 4 * w)
    y = m(x.cuda())
    yr = ref(x)
    assert (y.detach().cpu() - yr.detach()).abs().max().item() <= 2e-5 * yr.abs().max().item()
    torch.nn.functional.l1_loss(y, hr.cuda()).backward()
    torch.nn.functional.l1_loss(yr, hr).backward()
    refg = dict(ref.named_parameters())
    gflat = m.flat.grad.cpu()
    for k, (off, shp) in m.layout.entries.items():
        e = (gflat[off:off + refg[k].numel()].view(shp) - refg[k].grad).abs().max().item()
        assert e <= 3e-4 * max(refg[k].grad.abs().max().item(), 1e-9), (k, e)


def test_c3_shape_f32_units_16_blocks_vs_oracle():
    """BASELINE config C3's per-GPU shape: x4, 16 blocks / 32 units (fp32 parity mode, batch 2)"""
    torch.manual_seed(12)
    ns = _ns(num_blocks=16, num_residual_units=32)
    m = _model(ns).train()
    assert m.layout.total == 324528
    ref = O.OracleBasicModel(ns)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    x = torch.rand(2, 3, 48, 48)
    hr = torch.rand(2, 3, 192, 192)
    y = m(x.cuda())
    yr = ref(x)
    assert (y.detach().cpu() - yr.detach()).abs().max().item() <= 3e-5 * yr.abs().max().item()
    torch.nn.functional.l1_loss(y, hr.cuda()).backward()
    torch.nn.functional.l1_loss(yr, hr).backward()
    refg = dict(ref.named_parameters())
    gflat = m.flat.grad.cpu()
    worst = max(((gflat[off:off + refg[k].numel()].view(shp) - refg[k].grad).abs().max()
                 / refg[k].grad.abs().max().clamp_min(1e-12)).item() for k, (off, shp) in m.layout.entries.items())
    print(f"\nC3 shape worst rel grad err {worst:.2e}")
    assert worst <= 5e-4


def test_training_reduces_loss_bf16_and_matches_oracle_trajectory():
    """10 Adam steps at C1 size: the bf16 hot path follows the fp32 oracle's loss curve (same init, same data)"""
    torch.manual_seed(13)
    ns = _ns(num_blocks=4, hot_dtype="bf16")
    m = _model(ns).train()
    ref = O.OracleBasicModel(ns)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    x = torch.rand(4, 3, 24, 24)
    hr = torch.nn.functional.interpolate(x, scale_factor=4, mode="bilinear")
    o1 = torch.optim.Adam(m.parameters(), lr=1e-3)
    o2 = torch.optim.Adam(ref.parameters(), lr=1e-3)
    l1, l2 = [], []
    for _ in range(10):
        o1.zero_grad(); o2.zero_grad()
        a = torch.nn.functional.l1_loss(m(x.cuda()), hr.cuda()); a.backward(); o1.step(); l1.append(a.item())
        b = torch.nn.functional.l1_loss(ref(x), hr); b.backward(); o2.step(); l2.append(b.item())
    print("\nloss hot/bf16:", [round(v, 4) for v in l1], "\nloss oracle  :", [round(v, 4) for v in l2])
    assert l1[-1] < 0.7 * l1[0]
    assert all(abs(p - q) <= 0.05 * q + 2e-3 for p, q in zip(l1, l2))


def test_linearity_of_backward_at_full_size():
    """size-independent property at the BASELINE C2 shape: gradients are linear in the upstream gradient"""
    torch.manual_seed(14)
    m = _model(_ns(num_blocks=16, hot_dtype="fp32")).train()
    x = torch.rand(32, 3, 48, 48, device="cuda")
    g1 = torch.randn(32, 3, 192, 192, device="cuda")
    g2 = torch.randn(32, 3, 192, 192, device="cuda")

    def grad(g):
        m.zero_grad(set_to_none=True)
        m(x).backward(g)
        return m.flat.grad.clone()
    ga, gb, gc = grad(g1), grad(g2), grad(g1 + 2 * g2)
    err = (gc - (ga + 2 * gb)).abs().max().item() / gc.abs().max().item()
    print(f"\nlinearity rel err {err:.2e}")
    assert err <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nb,units", [((3, 3, 48, 48), 4, 24), ((2, 3, 20, 28), 4, 24), ((1, 3, 7, 9), 4, 24),
                                            ((3, 3, 48, 48), 3, 24),      # odd block count: two-block launch + one single
                                            ((50, 3, 48, 48), 2, 24),     # 400 workgroups: single-block kernels (with saves)
                                            ((3, 3, 48, 48), 3, 32), ((2, 3, 20, 28), 2, 32)])   # 32 units (C3 width)
def test_saved_image_weight_gradients_equal_recompute_path(shape, nb, units, monkeypatch):
    """bf16 / 24 units: the weight-gradient kernels fed by the saved t / dt images (two-block kernels) give the
    gradients of the recompute kernels: the same bf16 products, summed over pixel tiles in a different fp32 order
    (3 partial sums per e-tile instead of 2); db2 is the pixel sum of the bf16-rounded dt image instead of the
    fp32 accumulators (a bf16-rounding-level difference on the 20 conv2 biases per block)."""
    torch.manual_seed(5)
    m = _model(_ns(num_blocks=nb, num_residual_units=units, hot_dtype="bf16")).train()
    with torch.no_grad():
        m.flat.add_(0.02 * torch.randn_like(m.flat))
    x = torch.rand(*shape, device="cuda")
    w = torch.randn(shape[0], 3, 4 * shape[2], 4 * shape[3], device="cuda")

    def grad():
        m.flat.grad = None
        (m(x) * w).sum().backward()
        return m.flat.grad.clone()
    assert m._saves_side_images()
    g_saved = grad()
    monkeypatch.setenv("SR_RECOMPUTE_WGRAD", "1")
    assert not m._saves_side_images()
    g_rec = grad()
    scale = float(g_rec.abs().max())
    assert scale > 0 and torch.isfinite(g_saved).all()
    assert float((g_saved - g_rec).abs().max()) <= 2e-3 * scale
    assert float((g_saved - g_rec).abs().mean()) <= 2e-6 * scale


@pytest.mark.gpu
def test_static_weights_inference_skips_prep_and_matches():
    """opt-in `assume_static_weights`: repeated inference re-uses the packed weights (SR_NET_WEIGHTS_PACKED) and gives
    the same output; a parameter update (version bump) re-packs"""
    torch.manual_seed(9)
    m = _model(_ns(num_blocks=2, hot_dtype="bf16")).eval()
    x = torch.rand(2, 3, 20, 28, device="cuda")
    with torch.no_grad():
        ref = m(x)
        m.assume_static_weights = True
        a, b = m(x), m(x)
        assert torch.equal(a, ref) and torch.equal(b, ref)
        m.flat.mul_(1.01)                                    # in-place update through the parameter: version bump
        c = m(x)
        m.assume_static_weights = False
        d = m(x)
    assert torch.equal(c, d) and not torch.equal(c, ref)


@pytest.mark.gpu
def test_static_weights_two_segment_mode_repacks_after_optimizer_step():
    """with hot_grad_segments = 2 the optimizer steps flat_lo / flat_hi, whose version counters are not the
    master buffer's: the packed-weights key must follow the segments, or an eval forward after a step would run on the
    pre-step weights.  Checked against the one-parameter model carrying the same (stepped) weights."""
    torch.manual_seed(10)
    m2 = _model(_ns(num_blocks=4, hot_dtype="bf16", hot_grad_segments=2))
    m1 = _model(_ns(num_blocks=4, hot_dtype="bf16"))
    x = torch.rand(2, 3, 20, 28, device="cuda")
    hr = torch.rand(2, 3, 80, 112, device="cuda")
    m2.assume_static_weights = True
    m2.eval()
    with torch.no_grad():
        before = m2(x)
        assert torch.equal(m2(x), before)                   # (the shortcut is taken here)
    m2.train()
    opt = torch.optim.Adam(m2.parameters(), lr=1e-2)
    torch.nn.functional.l1_loss(m2(x), hr).backward()
    opt.step()
    m2.eval()
    m1.load_state_dict(m2.state_dict(), strict=True)
    m1.eval()
    with torch.no_grad():
        after, ref = m2(x), m1(x)
    assert not torch.equal(after, before)
    assert torch.equal(after, ref)


def test_large_batch_inference_takes_the_persistent_launches_and_equals_small_batches():
    """eval mode, bf16, 130 patches of 48x48 = 1040 tiles: sr_wdsr_net_forward runs the persistent two-block launches; the
    result equals the same patches pushed through in batches of 10 (per-tile launches), bit for bit"""
    import argparse
    from mobilesuperresolution_amd.models import get_model
    torch.manual_seed(11)
    ns = argparse.Namespace(model_type="BASIC_MODEL", image_mean=0.5, num_channels=3, scale=4, num_blocks=5, num_residual_units=24,
                            hot_dtype="bf16")
    m = get_model(ns).cuda().eval()
    x = torch.rand(130, 3, 48, 48, device="cuda")
    with torch.no_grad():
        big = m(x)
        small = torch.cat([m(x[i:i + 10]) for i in range(0, 130, 10)])
    assert torch.equal(big, small)


def test_large_batch_training_on_the_streaming_kernel_equals_small_batches():
    """256 patches of 48x48 per step: the forward of a training step takes the streaming two-block kernel WITH the saved t images
    (csrc/wdsr_fwd_stream.h, SAVE_T) and the weight gradients read those images.  Batch-split property at full size: output rows and
    the mean-loss gradient equal those of eight steps of 32 patches (per-tile kernels), combined -- outputs bit for bit, the
    gradient to fp32 summation order (bf16 mode)"""
    import argparse
    from mobilesuperresolution_amd.models import get_model
    torch.manual_seed(12)
    ns = argparse.Namespace(model_type="BASIC_MODEL", image_mean=0.5, num_channels=3, scale=4, num_blocks=4, num_residual_units=24,
                            hot_dtype="bf16")
    m = get_model(ns).cuda().train()
    x = torch.rand(256, 3, 48, 48, device="cuda")
    hr = torch.rand(256, 3, 192, 192, device="cuda")
    m.flat.grad = None
    big = m(x)
    torch.nn.functional.l1_loss(big, hr).backward()
    g_big = m.flat.grad.clone()
    g_acc = torch.zeros_like(g_big)
    outs = []
    for i in range(0, 256, 32):
        m.flat.grad = None
        o = m(x[i:i + 32])
        torch.nn.functional.l1_loss(o, hr[i:i + 32]).backward()
        g_acc += m.flat.grad / 8
        outs.append(o.detach())
    assert torch.equal(big.detach(), torch.cat(outs))
    scale = float(g_acc.abs().max())
    assert float((g_big - g_acc).abs().max()) <= 2e-3 * scale and float((g_big - g_acc).norm()) <= 1e-3 * float(g_acc.norm())


def test_32_units_two_blocks_per_forward_launch_equal_one_block_kernels():
    """32 units, bf16 (C3's width): the forward runs two blocks per launch on wdsr_fwd_rs16_kernel (sixteen waves, dense-K 3x3 on
    28-channel t rows); model.one_block32 = True keeps the round-1 one-block kernels.  Same products in another summation order: the
    outputs agree up to one-ulp flips of the bf16 activations, the saved t images feed the same weight-gradient kernels, the
    gradients agree within bf16 tolerance; the fused route also agrees with the fp32 parity mode like the one-block route does"""
    torch.manual_seed(14)
    ns = _ns(num_blocks=6, num_residual_units=32, hot_dtype="bf16")
    m = _model(ns).train()
    g = torch.Generator().manual_seed(15)
    x = torch.rand(3, 3, 40, 52, generator=g).cuda()
    hr = torch.rand(3, 3, 160, 208, generator=g).cuda()
    res = {}
    for key, single in (("pairs", False), ("single", True)):
        m.one_block32 = single
        m.zero_grad(set_to_none=True)
        y = m(x)
        torch.nn.functional.l1_loss(y, hr).backward()
        res[key] = (y.detach().clone(), m.flat.grad.clone())
    m.one_block32 = False
    (yp, gp), (ys, gs) = res["pairs"], res["single"]
    assert torch.isfinite(yp).all() and torch.isfinite(gp).all()
    rel = ((yp - ys).norm() / ys.norm()).item()
    grel = ((gp - gs).norm() / gs.norm()).item()
    print(f"\n32 units, pairs vs one-block kernels: output rel L2 {rel:.2e}, flat gradient rel L2 {grel:.2e}")
    assert rel <= 2e-3 and grel <= 3e-2
    # against the fp32 parity mode on the same parameters
    ns32 = _ns(num_blocks=6, num_residual_units=32)
    a = _model(ns32).train()
    a.load_state_dict(m.state_dict())
    ya = a(x)
    torch.nn.functional.l1_loss(ya, hr).backward()
    assert ((yp - ya.detach()).norm() / ya.detach().norm()).item() <= 2e-2
    assert ((gp - a.flat.grad).norm() / a.flat.grad.norm()).item() <= 6e-2


@pytest.mark.parametrize("units", [24, 32])
def test_overlapped_two_part_backward_equals_one_part(units):
    """the data-parallel step with the gradient all-reduce in two halves (backward_part 1 / 2, pair launches on either side of the
    split) against the one-call step, on a one-rank RCCL group, 24 and 32 units: the same gradients up to the summation order of the
    weight-gradient slabs (a half-depth part spreads its layers over other workgroups)"""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29541"
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        g = torch.Generator().manual_seed(31)
        x = torch.rand(4, 3, 24, 36, generator=g).cuda()
        hr = torch.rand(4, 3, 96, 144, generator=g).cuda()
        flats = []
        for overlap in (True, False):
            torch.manual_seed(2)
            m = _model(_ns(num_blocks=8, num_residual_units=units, hot_dtype="bf16")).train()
            st = m.make_train_state(lr=1e-3)
            for _ in range(2):
                loss = m.train_step(x, hr, st, process_group=dist.group.WORLD, overlap=overlap)
            assert torch.isfinite(loss)
            flats.append(m.flat.detach().clone())
        d = (flats[0] - flats[1]).abs()
        scale = float(flats[1].abs().max())
        assert float((d > 2e-5 * scale + 2e-6).float().mean()) <= 1e-3 and float(d.max()) <= 0.1 * 2 * 1e-3, (float(d.max()), scale)
    finally:
        dist.destroy_process_group()
