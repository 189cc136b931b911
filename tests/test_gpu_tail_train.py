"""sr_tail_train (tail forward + folded loss + tail backward in one launch, csrc/wdsr_ends.h sr_tail_train_kernel) against
the two launches it replaces in the training step, sr_tail_fwd followed by sr_tail_bwd_loss: bit for bit."""
import argparse
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TH, TW = 12, 24                                                # the tail kernels' LR tile


def _tail_inputs(f, n, h, w, seed):
    from mobilesuperresolution_amd import hotpath as HP
    dev = torch.device("cuda", 0)
    tb = HP.ends_tables(f, 4, dev)
    g = torch.Generator().manual_seed(seed)
    src_tail = (torch.randn(tb["tail_size"], generator=g) * 0.05).cuda()
    src_tail[-2], src_tail[-1] = 0.0, 1.0
    blob = HP.pack_tail(src_tail, f, 4, torch.bfloat16)
    feat = torch.randn(n, h, w, f, generator=g).cuda().bfloat16()
    x = torch.rand(n, 3, h, w, generator=g).cuda()
    hr = torch.rand(n, 3, 4 * h, 4 * w, generator=g).cuda()
    return tb, blob, feat, x, hr, g


def _two_launches(tb, blob, feat, x, hr, out, kind, gscale, wgs):
    from mobilesuperresolution_amd import _lib as L
    n, h, w, f = feat.shape
    dfeat = torch.full_like(feat, float("nan"))
    part = torch.zeros(wgs, tb["tail_slab"], device=feat.device)
    lpart = torch.full((wgs,), float("nan"), device=feat.device)
    L.check(L.lib().sr_tail_bwd_loss(out.data_ptr(), hr.data_ptr(), kind, gscale, lpart.data_ptr(), feat.data_ptr(), x.data_ptr(), 0.5,
                                     blob.data_ptr(), dfeat.data_ptr(), part.data_ptr(), wgs, n, h, w, f, 4, 1, L.stream_ptr()), "bwd_loss")
    return dfeat, part, lpart


def _one_launch(tb, blob, feat, x, hr, kind, gscale, wgs):
    from mobilesuperresolution_amd import _lib as L
    n, h, w, f = feat.shape
    dfeat = torch.full_like(feat, float("nan"))
    part = torch.zeros(wgs, tb["tail_slab"], device=feat.device)
    lpart = torch.full((wgs,), float("nan"), device=feat.device)
    L.check(L.lib().sr_tail_train(hr.data_ptr(), kind, gscale, lpart.data_ptr(), feat.data_ptr(), x.data_ptr(), 0.5, blob.data_ptr(),
                                  dfeat.data_ptr(), part.data_ptr(), wgs, n, h, w, f, 4, 1, L.stream_ptr()), "tail_train")
    return dfeat, part, lpart


# (N, H, W, wgs): one tile with every halo pixel outside the image; ragged right and bottom tiles; 2 x 2 tiles whose halo
# pixels belong to neighbours; one workgroup looping over all 12 tiles; an uneven share; idle workgroups
_GRID = [(1, 12, 24, 16), (2, 12, 24, 16), (1, 13, 25, 16), (2, 13, 25, 16), (1, 24, 48, 16), (2, 24, 48, 16),
         (3, 24, 48, 1), (3, 24, 48, 5), (3, 24, 48, 20)]


@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n,h,w,wgs", _GRID)
def test_tail_train_bit_identical_to_forward_then_backward(n, h, w, wgs, kind, f):
    from mobilesuperresolution_amd import hotpath as HP
    tb, blob, feat, x, hr, g = _tail_inputs(f, n, h, w, 100 + 7 * n + h + wgs)
    out = torch.empty(n, 3, 4 * h, 4 * w, device="cuda")
    HP.tail_fwd(feat, x, out, blob, 0.5, 4)
    if kind == 1:
        # exact zeros of sr - hr (sign(0) = 0 and no loss term): a few hundred HR values taken from the two-launch path's own
        # output, at least 100 in LR pixels inside a tile and at least 20 in LR pixels on a tile's border
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        border = ((ys % TH == 0) | (ys % TH == TH - 1) | (ys == h - 1) | (xs % TW == 0) | (xs % TW == TW - 1) | (xs == w - 1))
        pick = torch.zeros(n, h, w, dtype=torch.bool)
        for mask, cnt in ((border, 40), (~border, 120)):
            idx = mask.expand(n, h, w).nonzero()
            sel = idx[torch.randperm(idx.shape[0], generator=g)[:cnt]]
            pick[sel[:, 0], sel[:, 1], sel[:, 2]] = True
        n_border, n_inner = int((pick & border).sum()), int((pick & ~border).sum())
        assert n_inner >= 100 and n_border >= 20, (n_inner, n_border)
        hr_mask = pick.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, None].expand(n, 3, 4 * h, 4 * w).cuda()
        hr = torch.where(hr_mask, out, hr)
        assert int((out == hr).sum()) >= 3 * 16 * (n_inner + n_border)
    gscale = 0.7 / out.numel()
    d_ref, p_ref, l_ref = _two_launches(tb, blob, feat, x, hr, out, kind, gscale, wgs)
    d_new, p_new, l_new = _one_launch(tb, blob, feat, x, hr, kind, gscale, wgs)
    torch.cuda.synchronize()
    assert torch.isfinite(d_ref.float()).all() and torch.isfinite(l_ref).all()
    assert torch.equal(d_new, d_ref)
    # slab columns outside the gather table come from LDS bytes past the 4-channel image rows (never used): compare what
    # the network consumes, slab by slab (as test_gpu_block.test_fused_tail_backward_bit_identical_to_two_launches does)
    used = tb["tail_grad"]
    assert torch.equal(p_new.index_select(1, used), p_ref.index_select(1, used))
    assert torch.equal(l_new, l_ref), (l_new - l_ref).abs().max().item()


def _ns(nb=2, f=24):
    return argparse.Namespace(model_type="BASIC_MODEL", image_mean=0.5, num_channels=3, scale=4, num_blocks=nb,
                              num_residual_units=f, hot_dtype="bf16")


def test_train_step_bit_identical_to_forward_backward_adam_by_hand():
    """model.train_step (the tail in one launch) == sr_wdsr_net_forward + sr_wdsr_net_backward + sr_adam_step of the same build
    (the tail in two launches): loss, parameters and both Adam moments after each of 3 steps"""
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.models import get_model
    from mobilesuperresolution_amd.models import basic_wdsr_b as B
    from mobilesuperresolution_amd.models import loss_fold
    torch.manual_seed(3)
    a = get_model(_ns()).cuda().train()
    b = get_model(_ns()).cuda().train()
    with torch.no_grad():
        b.flat.copy_(a.flat)
    sa, sb = a.make_train_state(), b.make_train_state()
    g = torch.Generator().manual_seed(9)
    for step in range(3):
        x = torch.rand(2, 3, 24, 48, generator=g).cuda()
        hr = torch.rand(2, 3, 96, 192, generator=g).cuda()
        la = a.train_step(x, hr, sa)
        # by hand, on b
        st = b._state(x.device)
        flat = b.flat.detach()
        out, acts, side = b._forward_buffers(x, True)
        grads, gflat, dtsave = B._backward_buffers(acts, flat, side)
        net = st.call_net(x, flat, acts, out=out, grads=grads, gflat=gflat, side=side, dtsave=dtsave, hr=hr, kind=1,
                          gscale=loss_fold.gscale(1.0, out.numel()))
        lb = torch.empty((), dtype=torch.float32, device=x.device)
        scal = sb.next_scalars()
        sp = L.stream_ptr(x.device)
        B._launch_net("sr_wdsr_net_forward", net, 1, sp)
        B._launch_net("sr_wdsr_net_backward", net, sp)
        L.check(L.lib().sr_adam_step(flat.data_ptr(), gflat.data_ptr(), sb.exp_avg.data_ptr(), sb.exp_avg_sq.data_ptr(), flat.numel(),
                                     ctypes.byref(scal), st.loss_part.data_ptr(), st.wgs_tail, 1.0 / out.numel(), lb.data_ptr(), sp),
                "adam")
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (step, la.item(), lb.item())
        assert torch.equal(a.flat.detach(), b.flat.detach()), step
        assert torch.equal(sa.exp_avg, sb.exp_avg) and torch.equal(sa.exp_avg_sq, sb.exp_avg_sq), step
