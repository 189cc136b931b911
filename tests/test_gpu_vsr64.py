"""The 64-feature propagation trunk (ConvResidualBlocks with 24 < F <= 64 on csrc/conv64.h, inference only) on the MI355X:
fixture G17 of the reference's BasicVSR_origin(64, 1), a 30-block REDS-shaped clip against an fp32 ATen restatement, both
directions in one launch, the F = 40 embedding, the ping-pong memory plan and the no-graph guard."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# bf16 route vs the fp32 ATen restatement, 30 blocks at 180 x 320, relative L2 over all features:
# first run 8.9e-3 (forward-time loop) and 1.14e-2 (backward-time loop); the bound leaves ~2x
BF16_L2_30 = 2.5e-2


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _trunks(p, nb, dtype, f=64):
    from mobilesuperresolution_amd.models import ConvResidualBlocks
    out = []
    for name in ("backward_trunk", "forward_trunk"):
        m = ConvResidualBlocks(f + 3, f, nb, hot_dtype=dtype)
        if p is not None:
            m.load_state_dict({k[len(name) + 1:]: v for k, v in p.items() if k.startswith(name + ".")}, strict=True)
        out.append(m.cuda().requires_grad_(False))
    return out


def _rel_max(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("fused", [True, False])
def test_g17_propagation_matches_reference(golden_dir, dtype, fused):
    from mobilesuperresolution_amd.models import flow_warp
    from mobilesuperresolution_amd.models.basicvsr_arch import propagate
    d = _load(golden_dir, "g17_vsr_trunk64.npz")
    p = {k[2:]: v for k, v in d.items() if k.startswith("p/")}
    bt, ft = _trunks(p, 1, dtype)
    fw = flow_warp if fused else (lambda a, b: flow_warp(a, b))      # a wrapped flow_warp takes propagate's unfused loops
    with torch.no_grad():
        ob, of = propagate(d["x"].cuda(), d["flows_forward"].cuda(), d["flows_backward"].cuda(), bt, ft, fw, num_feat=64)
    got_b = torch.stack(ob[::-1], 1).cpu()                             # call order of the backward-time loop: frame n-1 .. 0
    got_f = torch.stack(of, 1).cpu()
    for got, ref in ((got_b, d["feat_backward"]), (got_f, d["feat_forward"])):
        if dtype == "fp32":
            e = _rel_max(got, ref)
            print(f"\nG17 {dtype} fused={fused} rel max-abs {e:.2e}")
            assert e <= 1e-5
        else:
            e = _rel_l2(got, ref)
            print(f"\nG17 {dtype} fused={fused} rel L2 {e:.2e}")
            assert e <= 2e-2


def _aten_trunk(p, prefix, x, nb):
    y = F.leaky_relu(F.conv2d(x, p[prefix + "main.0.weight"], p[prefix + "main.0.bias"], padding=1), 0.1)
    for i in range(nb):
        q = f"{prefix}main.2.{i}."
        t = F.relu(F.conv2d(y, p[q + "conv1.weight"], p[q + "conv1.bias"], padding=1))
        y = y + F.conv2d(t, p[q + "conv2.weight"], p[q + "conv2.bias"], padding=1)
    return y


def _aten_warp(x, flow):
    _, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=x.dtype, device=x.device), torch.arange(w, dtype=x.dtype, device=x.device),
                            indexing="ij")
    vx = 2.0 * (gx + flow[:, 0]) / max(w - 1, 1) - 1.0
    vy = 2.0 * (gy + flow[:, 1]) / max(h - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((vx, vy), 3), mode="bilinear", padding_mode="zeros", align_corners=True)


def _aten_propagate(sd, x, ff, fb, nb):
    """the reference's propagation loops (basicvsr_arch_origin.py:61-82) in fp32 ATen"""
    b, n, _, h, w = x.shape
    out = {}
    for name, flows, order in (("backward", fb, range(n - 1, -1, -1)), ("forward", ff, range(n))):
        feat, res = x.new_zeros(b, 64, h, w), {}
        for k, i in enumerate(order):
            if k:
                feat = _aten_warp(feat, flows[:, i if name == "backward" else i - 1])
            feat = _aten_trunk(sd, name + "_trunk.", torch.cat([x[:, i], feat], 1), nb)
            res[i] = feat
        out[name] = torch.stack([res[i] for i in range(n)], 1)
    return out


@pytest.fixture(scope="module")
def clip30():
    from mobilesuperresolution_amd.models.basicvsr_arch_origin import BasicVSR_origin
    torch.manual_seed(64)
    m = BasicVSR_origin(64, 30)
    g = torch.Generator().manual_seed(65)
    x = torch.rand(1, 5, 3, 180, 320, generator=g).cuda()
    ff = (torch.rand(1, 4, 2, 180, 320, generator=g) * 8 - 4).cuda()
    fb = (torch.rand(1, 4, 2, 180, 320, generator=g) * 8 - 4).cuda()
    sd = {k: v.cuda() for k, v in m.state_dict().items() if "_trunk." in k}
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    with torch.no_grad():
        ref = _aten_propagate(sd, x, ff, fb, 30)
    torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
    return m.state_dict(), x, ff, fb, ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_basicvsr_origin_30_blocks_reds_shape_against_aten(clip30, dtype):
    from mobilesuperresolution_amd.models.basicvsr_arch_origin import BasicVSR_origin
    sd, x, ff, fb, ref = clip30
    m = BasicVSR_origin(64, 30, hot_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    with torch.no_grad():
        ob, of = m.backward_trunk, m.forward_trunk
        from mobilesuperresolution_amd.models import flow_warp
        from mobilesuperresolution_amd.models.basicvsr_arch import propagate
        fb_l, ff_l = propagate(x, ff, fb, ob, of, flow_warp, num_feat=64)
        got = {"backward": torch.stack(fb_l, 1), "forward": torch.stack(ff_l, 1)}
        for name in ("backward", "forward"):
            if dtype == "fp32":
                e = _rel_max(got[name], ref[name])
                print(f"\n30 blocks fp32 {name}: rel max-abs {e:.2e}")
                assert e <= 1e-4
            else:
                e = _rel_l2(got[name], ref[name])
                print(f"\n30 blocks bf16 {name}: rel L2 {e:.2e}")
                assert e <= BF16_L2_30
        out = m(x, 720, 1280, flows=(ff, fb))
    assert out.shape == (1, 5, 3, 720, 1280) and torch.isfinite(out).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_both_directions_in_one_launch_equal_two_calls(dtype):
    from mobilesuperresolution_amd.models.basicvsr_arch import forward_warped_pair
    torch.manual_seed(7)
    bt, ft = _trunks(None, 3, dtype)
    g = torch.Generator().manual_seed(8)
    fr = torch.rand(2, 2, 3, 37, 50, generator=g).cuda()
    fl = (torch.rand(2, 2, 37, 50, generator=g) * 6 - 3).cuda()
    with torch.no_grad():
        sa = sb = sp = None
        for k in range(3):
            fa, sa = bt.forward_warped(fr[k % 2, 0:1], sa, fl[0:1] if k else None)
            fb_, sb = ft.forward_warped(fr[k % 2, 1:2], sb, fl[1:2] if k else None)
            pa, pb, sp = forward_warped_pair(bt, ft, fr[k % 2], sp, fl if k else None)
            assert torch.equal(pa, fa) and torch.equal(pb, fb_) and torch.equal(sp, torch.cat([sa, sb]))
    assert sp.shape == (2, 37, 50, 64) and sp.dtype == bt.hot_dtype


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_f40_equals_f64_with_zero_rows_and_columns(dtype):
    from mobilesuperresolution_amd.models import ConvResidualBlocks
    torch.manual_seed(40)
    m40 = ConvResidualBlocks(43, 40, 2, hot_dtype=dtype)
    sd64 = {}
    for k, v in m40.state_dict().items():
        if k.endswith("bias"):
            z = torch.zeros(64)
            z[:40] = v
        elif k == "main.0.weight":                    # [frame 3 | state 40] -> [frame 3 | state 64]
            z = torch.zeros(64, 67, 3, 3)
            z[:40, :43] = v
        else:
            z = torch.zeros(64, 64, 3, 3)
            z[:40, :40] = v
        sd64[k] = z
    m64 = ConvResidualBlocks(67, 64, 2, hot_dtype=dtype)
    m64.load_state_dict(sd64, strict=True)
    m40, m64 = m40.cuda().requires_grad_(False), m64.cuda().requires_grad_(False)
    g = torch.Generator().manual_seed(41)
    fr = torch.rand(2, 1, 3, 21, 35, generator=g).cuda()
    fl = (torch.rand(1, 2, 21, 35, generator=g) * 4 - 2).cuda()
    with torch.no_grad():
        s40 = s64 = None
        for k in range(2):
            f40, s40 = m40.forward_warped(fr[k], s40, fl if k else None)
            f64, s64 = m64.forward_warped(fr[k], s64, fl if k else None)
            assert torch.equal(f40, f64[:, :40]) and not f64[:, 40:].any() and torch.equal(s40, s64)
        # the plain (unfused) entry: [frame | state] NCHW
        x = torch.cat([fr[0], f40], 1)
        assert torch.equal(m40(x), m64(torch.cat([fr[0], f64], 1))[:, :40])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_plain_64_input_trunk_against_aten(dtype):
    """ConvResidualBlocks(64, 64, n): the 64-channel first conv"""
    from mobilesuperresolution_amd.models import ConvResidualBlocks
    torch.manual_seed(12)
    m = ConvResidualBlocks(64, 64, 2, hot_dtype=dtype).cuda().requires_grad_(False)
    x = torch.randn(2, 64, 33, 17, device="cuda")
    sd = {k: v.cuda() for k, v in m.state_dict().items()}
    prev = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    with torch.no_grad():
        ref = _aten_trunk(sd, "", x, 2)
        y = m(x)
    torch.backends.cudnn.allow_tf32 = prev
    e = _rel_max(y, ref) if dtype == "fp32" else _rel_l2(y, ref)
    assert e <= (1e-5 if dtype == "fp32" else 2e-2), e


def test_propagation_memory_is_the_ping_pong_plan():
    from mobilesuperresolution_amd.models import flow_warp
    from mobilesuperresolution_amd.models.basicvsr_arch import propagate
    torch.manual_seed(3)
    bt, ft = _trunks(None, 30, "bf16")
    n, h, w = 5, 180, 320
    x = torch.rand(1, n, 3, h, w, device="cuda")
    fl = torch.rand(1, n - 1, 2, h, w, device="cuda") * 4 - 2
    with torch.no_grad():
        propagate(x, fl, -fl, bt, ft, flow_warp, num_feat=64)      # packed weights cached, allocator warm
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ob, of = propagate(x, fl, -fl, bt, ft, flow_warp, num_feat=64)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    img = 2 * h * w * 64 * 2                                          # one 64-channel bf16 image pair of a frame step (both directions)
    feat = h * w * 64 * 4                                             # one direction's fp32 feature map
    # kept: 2n feature maps (the result); per step: ping, pong, out, the previous state, 2 feature maps, the frame / flow slices
    bound = 2 * n * feat + 6 * img + 16 * 2 ** 20
    print(f"\npeak {peak / 2 ** 20:.1f} MiB, bound {bound / 2 ** 20:.1f} MiB, a saved-activation route: {61 * img / 2 ** 20:.0f} MiB per step")
    assert peak <= bound < 61 * img


def test_grad_recording_forward_raises_at_f64():
    from mobilesuperresolution_amd.models import ConvResidualBlocks
    from mobilesuperresolution_amd.models.basicvsr_arch import forward_warped_pair
    m = ConvResidualBlocks(67, 64, 1).cuda()
    m2 = ConvResidualBlocks(67, 64, 1).cuda()
    fr = torch.rand(2, 3, 20, 20, device="cuda")
    x = torch.rand(1, 67, 20, 20, device="cuda")
    for call in (lambda: m(x), lambda: m.forward_warped(fr[:1]), lambda: forward_warped_pair(m, m2, fr)):
        with pytest.raises(NotImplementedError, match="no_grad"):
            call()
    with torch.no_grad():
        f, s = m.forward_warped(fr[:1])
    m.requires_grad_(False)
    m2.requires_grad_(False)
    f2, _ = m.forward_warped(fr[:1])                                   # grad mode on, nothing requires grad: runs
    assert torch.equal(f, f2) and not f2.requires_grad
    with pytest.raises(NotImplementedError):
        m.forward_warped(fr[:1].clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        m(x.clone().requires_grad_(True))


@pytest.mark.parametrize("name", ["BasicVSR_origin", "MotionVectorVSR", "BasicVSR"])
def test_default_models_construct_and_propagate(name):
    from mobilesuperresolution_amd import models as M
    from mobilesuperresolution_amd.models import flow_warp
    from mobilesuperresolution_amd.models.basicvsr_arch import propagate
    from mobilesuperresolution_amd.models.basicvsr_arch_origin import BasicVSR_origin
    from mobilesuperresolution_amd.models.mvvsr_arch import MotionVectorVSR
    cls = {"BasicVSR_origin": BasicVSR_origin, "MotionVectorVSR": MotionVectorVSR, "BasicVSR": M.basicvsr_arch.BasicVSR}[name]
    torch.manual_seed(1)
    m = cls(hot_dtype="bf16").cuda().eval()
    assert m.backward_trunk.num_feat == 64 and m.backward_trunk.wide
    x = torch.rand(1, 3, 3, 24, 40, device="cuda")
    fl = torch.rand(1, 2, 2, 24, 40, device="cuda") * 2 - 1
    with torch.no_grad():
        ob, of = propagate(x, fl, -fl, m.backward_trunk, m.forward_trunk, flow_warp, num_feat=64)
        if name == "MotionVectorVSR":
            mv = torch.cat([torch.zeros_like(fl[:, :1]), fl], 1)
            out = m(torch.cat([x, mv], 2), 96, 160)
            assert out.shape == (1, 3, 3, 96, 160) and torch.isfinite(out).all()
    assert len(ob) == len(of) == 3 and all(torch.isfinite(t).all() for t in ob + of) and ob[0].shape == (1, 64, 24, 40)
