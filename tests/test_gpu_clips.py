"""f3 for the video trainer: training clips cut on device (csrc/clips.h, datasets.DeviceClipCache) against items of the
reference's own dataset classes (fixture G16, tools/make_golden_clips.py from datasets/_vsr.py) and against the CPU
restatement tests/clip_ref.py (pinned by G16), draw for draw; then one training step of each video model on a cache batch."""
import random

import numpy as np
import pytest
import torch

from tests import clip_ref as CR
from tests.test_clip_golden import load_g16

pytestmark = pytest.mark.gpu


def _sequences(scale, seqs, with_mv, seed, mv_range=300):
    """frames of `seqs` = [(n_frames, lr_h, lr_w), ...]; HR up to a pixel larger than scale x LR; MV signed int16"""
    g = np.random.default_rng(seed)
    lrs, hrs, mvs, starts = [], [], [], []
    for si, (n, h, w) in enumerate(seqs):
        starts.append(len(lrs))
        for _ in range(n):
            lrs.append(g.integers(0, 256, (h, w, 3), dtype=np.uint8))
            hrs.append(g.integers(0, 256, (h * scale + si % 2, w * scale + (si // 2) % 2, 3), dtype=np.uint8))
            mvs.append(g.integers(-mv_range, mv_range + 1, (h, w, 2), dtype=np.int16))
    return lrs, hrs, (mvs if with_mv else None), starts


def _windows(seqs, starts, T):
    """datasets/reds.py list_image_files: every window of T consecutive frames of every sequence"""
    return [list(range(s + k, s + k + T)) for (n, _, _), s in zip(seqs, starts) for k in range(n + 1 - T)]


def _expected(lrs, hrs, mvs, clips, idx, P, scale, ignored, num_patches, rng):
    items = [CR.train_item(lrs, hrs, clips, i, P, scale, ignored, num_patches, rng, mvs) for i in idx]
    return torch.from_numpy(np.stack([a for a, _ in items])), torch.from_numpy(np.stack([b for _, b in items]))


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_device_clips_equal_reference_dataset_items_g16(golden_dir, ci):
    """every item the reference's __getitem__ produced under a seeded `random` comes out of DeviceClipCache.batch bit for bit,
    and the RNG has made the same number of draws afterwards"""
    from mobilesuperresolution_amd.datasets import DeviceClipCache
    p, lrs, hrs, mvs, clips, idx, seed, exp_lr, exp_hr, nxt = load_g16(golden_dir)[ci]
    ds = DeviceClipCache(lrs, hrs, clips, p["P"], p["scale"], p["ignored"], p["num_patches"], mv_frames=mvs)
    assert len(ds) == len(clips) * p["num_patches"]
    rng = random.Random(seed)
    lr, hr = ds.batch(idx, rng)
    assert lr.shape == exp_lr.shape and hr.shape == exp_hr.shape
    assert torch.equal(lr.cpu(), torch.from_numpy(exp_lr)), ci
    assert torch.equal(hr.cpu(), torch.from_numpy(exp_hr)), ci
    assert rng.random() == nxt


# P = 17 / sP = 51 and 34: rows end in a run shorter than the kernel's four pixels, and the rows are not 16-byte aligned
@pytest.mark.parametrize("scale,P,ignored,num_patches,with_mv,T", [(2, 17, 1, 2, False, 3), (3, 17, 2, 1, True, 4),
                                                                   (4, 16, 0, 3, False, 2), (4, 24, 3, 2, True, 3)])
def test_device_clips_equal_restatement_draw_for_draw(scale, P, ignored, num_patches, with_mv, T):
    from mobilesuperresolution_amd.datasets import DeviceClipCache
    g = np.random.default_rng(scale * 100 + P)
    lo = P + 2 * ignored + 1
    seqs = [(T + 2, int(g.integers(lo, 68)), int(g.integers(lo, 90))), (T + 1, int(g.integers(70, 90)), int(g.integers(lo, 90))),
            (T, int(g.integers(lo, 90)), int(g.integers(lo, 90)))]
    lrs, hrs, mvs, starts = _sequences(scale, seqs, with_mv, seed=P + scale)
    clips = _windows(seqs, starts, T)
    ds = DeviceClipCache(lrs, hrs, clips, P, scale, ignored, num_patches, mv_frames=mvs)
    idx = list(range(len(ds))) * 6
    lr, hr = ds.batch(idx, random.Random(77))
    rng = random.Random(77)
    exp_lr, exp_hr = _expected(lrs, hrs, mvs, clips, idx, P, scale, ignored, num_patches, rng)
    assert lr.shape == (len(idx), T, 5 if with_mv else 3, P, P) and hr.shape == (len(idx), T, 3, P * scale, P * scale)
    assert torch.equal(lr.cpu(), exp_lr)
    assert torch.equal(hr.cpu(), exp_hr)
    probe = random.Random(77)
    flags = {ds.draw(i, probe)[3] for i in idx}
    assert flags == {0, 1, 2, 3}                                            # all four flip combinations occurred
    assert probe.getstate() == rng.getstate()
    assert {h <= 68 for _, h, _ in seqs} == {True, False}                   # both sides of the RGB class's x = 0 rule


def test_repeated_indices_and_overlapping_clips():
    from mobilesuperresolution_amd.datasets import DeviceClipCache
    seqs = [(6, 50, 60), (5, 72, 40)]
    lrs, hrs, mvs, starts = _sequences(3, seqs, True, seed=3)
    clips = _windows(seqs, starts, 4)                                       # windows share frames
    for m in (None, mvs):
        ds = DeviceClipCache(lrs, hrs, clips, 20, 3, 1, 2, mv_frames=m)
        idx = [5, 5, 0, 1, 2, 5, 9, 0, 8]
        lr, hr = ds.batch(idx, random.Random(4))
        exp_lr, exp_hr = _expected(lrs, hrs, m, clips, idx, 20, 3, 1, 2, random.Random(4))
        assert torch.equal(lr.cpu(), exp_lr) and torch.equal(hr.cpu(), exp_hr)


def test_bad_constructor_inputs_raise():
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.datasets import DeviceClipCache
    lrs, hrs, mvs, _ = _sequences(2, [(3, 40, 48)], True, seed=1)
    with pytest.raises(ValueError, match="different sizes"):
        DeviceClipCache(lrs[:2] + [lrs[2][:, :46].copy()], hrs, [[1, 2]], 12, 2)
    with pytest.raises(ValueError, match="smaller than scale"):
        DeviceClipCache(lrs, hrs, [[0, 1]], 12, 3)
    with pytest.raises(ValueError, match="motion vectors"):
        DeviceClipCache(lrs, hrs, [[0, 1]], 12, 2, mv_frames=mvs[:2] + [mvs[2][:39]])
    with pytest.raises(ValueError, match="too small"):
        DeviceClipCache(lrs, hrs, [[0, 1]], 12, 2, ignored_boundary_size=19)
    with pytest.raises(L.HotpathError):
        DeviceClipCache(lrs, hrs, [[0, 1]], 12, 2, device="cpu")


def _step(model, lr, hr, loss_of):
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = loss_of(model, lr, hr)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    opt.step()
    return loss.detach(), grads, {k: v.detach().clone() for k, v in model.state_dict().items()}


def _same_step(make, lr_a, hr_a, lr_b, hr_b, loss_of):
    """the same training step on two equal batches from two equal models.  Not bit for bit: the backward of ATen's bilinear
    `interpolate` (upsample_bilinear2d_backward, a scatter with float atomics) sums in arrival order, so gradients may differ
    in the last bits from run to run; G11's tolerances apply to the gradients, and the Adam step is compared in bulk."""
    torch.manual_seed(0)
    ma = make()
    mb = make()
    mb.load_state_dict(ma.state_dict(), strict=True)
    la, ga, sa = _step(ma.cuda().train(), lr_a, hr_a, loss_of)
    lb, gb, sb = _step(mb.cuda().train(), lr_b, hr_b, loss_of)
    assert torch.equal(la, lb), (la.item(), lb.item())
    assert ga.keys() == gb.keys() and ga
    for k in ga:
        e = (ga[k] - gb[k]).abs().max().item() / max(gb[k].abs().max().item(), 1e-30)
        assert e <= 5e-4, (k, e)
    diff = torch.cat([(sa[k].float() - sb[k].float()).abs().reshape(-1) for k in sb])
    assert (diff <= 1e-4).float().mean().item() >= 0.99


def test_mv_batch_feeds_a_motion_vector_vsr_training_step():
    """the trainer's loop body for 'basic_mv' (train_video_superresolution.py:87): model(lr, hr.shape[3], hr.shape[4]), L1,
    backward, Adam -- on a cache batch and on the restatement's batch copied to the device"""
    from mobilesuperresolution_amd.datasets import DeviceClipCache
    from mobilesuperresolution_amd.models import MotionVectorVSR
    seqs = [(5, 40, 44), (4, 72, 36)]
    lrs, hrs, mvs, starts = _sequences(4, seqs, True, seed=11, mv_range=4)     # flows of a few pixels
    clips = _windows(seqs, starts, 3)
    ds = DeviceClipCache(lrs, hrs, clips, 16, 4, 1, 2, mv_frames=mvs)
    idx = [3, 0, 5]
    lr, hr = ds.batch(idx, random.Random(5))
    elr, ehr = _expected(lrs, hrs, mvs, clips, idx, 16, 4, 1, 2, random.Random(5))
    assert torch.equal(lr.cpu(), elr) and torch.equal(hr.cpu(), ehr)

    def l1(m, x, y):
        return torch.nn.functional.l1_loss(m(x, y.shape[3], y.shape[4]), y)
    _same_step(lambda: MotionVectorVSR(num_feat=20, num_block=2, hot_dtype="fp32"), lr, hr, elr.cuda(), ehr.cuda(), l1)


def test_rgb_batch_feeds_a_basicvsr_training_step():
    """'basic': BasicVSR on 64 x 64 clips (SpyNet's six-level pyramid needs them).  Its forward ends in `out += base` with F
    channels against three and raises in the reference as well (see models/basicvsr_arch.py), with either batch; the step
    therefore trains what the module computes up to there: SpyNet flows and both propagation trunks, L1 on their features"""
    from mobilesuperresolution_amd.datasets import DeviceClipCache
    from mobilesuperresolution_amd.models import BasicVSR
    seqs = [(4, 70, 80), (3, 66, 72)]
    lrs, hrs, _, starts = _sequences(2, seqs, False, seed=12)
    clips = _windows(seqs, starts, 3)
    ds = DeviceClipCache(lrs, hrs, clips, 64, 2)
    idx = [2, 0]
    lr, hr = ds.batch(idx, random.Random(6))
    elr, ehr = _expected(lrs, hrs, None, clips, idx, 64, 2, 0, 1, random.Random(6))
    assert torch.equal(lr.cpu(), elr) and torch.equal(hr.cpu(), ehr)
    with pytest.raises(RuntimeError, match="must match"):
        BasicVSR(num_feat=24, num_block=2, hot_dtype="fp32").cuda()(lr, hr.shape[3], hr.shape[4])

    def feat_l1(m, x, y):
        fb, ff = m.propagation_features(x)
        f = torch.stack(list(fb) + list(ff))
        return torch.nn.functional.l1_loss(f, torch.zeros_like(f))
    _same_step(lambda: BasicVSR(num_feat=24, num_block=2, hot_dtype="fp32"), lr, hr, elr.cuda(), ehr.cuda(), feat_l1)
