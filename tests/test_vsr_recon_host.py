"""CPU checks of the HIP reconstruction of BasicVSR_origin (csrc/vsr_recon.h): fixture G19 against a plain-torch restatement of the
reference's forward, packing.c64_recon_tables (coverage, and lane-level numpy models of the fusion, of the sub-pixel upconvs with
their shuffled store and of conv_last + base against F.conv2d / F.pixel_shuffle / F.interpolate), and the kernel's bilinear x4
base against F.interpolate bit for bit (no GPU)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mobilesuperresolution_amd import packing as P
from tests import mfma_emu as E
from tests.test_trunk64_layout import _emu_conv64, _flow_warp_cpu, _trunk_cpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bf16_bits_to_float(a):
    return torch.from_numpy((a.astype(np.uint32) << 16).view(np.float32).copy())


def load_g19():
    """(frames, flows_forward, flows_backward, {64: (params, out), 24: (params, out)}) -- the 64-feature trunks come from G17"""
    g17 = np.load(os.path.join(GOLDEN, "g17_vsr_trunk64.npz"))
    g19 = np.load(os.path.join(GOLDEN, "g19_vsr_recon.npz"))
    p64 = {k[2:]: torch.from_numpy(g17[k]) for k in g17.files if k.startswith("p/")}
    p64.update({k[2:]: bf16_bits_to_float(g19[k]) for k in g19.files if k.startswith("q/")})
    p24 = {k[4:]: bf16_bits_to_float(g19[k]) for k in g19.files if k.startswith("q24/")}
    x, ff, fb = (torch.from_numpy(g17[k]) for k in ("x", "flows_forward", "flows_backward"))
    return x, ff, fb, {64: (p64, torch.from_numpy(g19["out64"])), 24: (p24, torch.from_numpy(g19["out24"]))}


def recon_cpu(p, feat_b, feat_f, frame):
    """the reference's reconstruction of one frame (basicvsr_arch_origin.py:84-92) in plain torch"""
    out = torch.cat([feat_b, feat_f], 1)
    out = F.leaky_relu(F.conv2d(out, p["fusion.weight"], p["fusion.bias"]), 0.1)
    out = F.leaky_relu(F.pixel_shuffle(F.conv2d(out, p["upconv1.weight"], p["upconv1.bias"], padding=1), 2), 0.1)
    out = F.leaky_relu(F.pixel_shuffle(F.conv2d(out, p["upconv2.weight"], p["upconv2.bias"], padding=1), 2), 0.1)
    out = F.leaky_relu(F.conv2d(out, p["conv_hr.weight"], p["conv_hr.bias"], padding=1), 0.1)
    out = F.conv2d(out, p["conv_last.weight"], p["conv_last.bias"], padding=1)
    return out + F.interpolate(frame, scale_factor=4, mode="bilinear", align_corners=False)


def forward_cpu(p, x, ff, fb, f):
    """the reference's BasicVSR_origin.forward(x, 4h, 4w) with given flows, one block per trunk"""
    b, n, _, h, w = x.shape
    nb = len({k.split(".")[3] for k in p if k.startswith("backward_trunk.main.2.")})
    feats = {}
    for name, flows, order in (("backward", fb, range(n - 1, -1, -1)), ("forward", ff, range(n))):
        feat, res = x.new_zeros(b, f, h, w), {}
        for i in order:
            if res:
                feat = _flow_warp_cpu(feat, flows[:, i if name == "backward" else i - 1].permute(0, 2, 3, 1))
            feat = _trunk_cpu(p, f"{name}_trunk.", torch.cat([x[:, i], feat], 1), nb)
            res[i] = feat
        feats[name] = res
    return torch.stack([recon_cpu(p, feats["backward"][i], feats["forward"][i], x[:, i]) for i in range(n)], 1)


@pytest.mark.parametrize("f", [64, 24])
def test_g19_is_self_consistent_with_a_plain_torch_restatement(f):
    x, ff, fb, models = load_g19()
    p, ref = models[f]
    assert ref.shape == (1, 3, 3, 72, 80)
    assert [k for k, _ in P.c64_recon_shapes(f)] == [k for k in p if "_trunk." not in k]
    for k, shape in P.c64_recon_shapes(f):
        assert tuple(p[k].shape) == shape and torch.equal(p[k], p[k].bfloat16().float()), k
    out = forward_cpu(p, x, ff, fb, f)
    e = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"\nG19 F={f}: restatement vs fixture, rel max-abs {e:.2e}")
    assert e <= 1e-5


# ---- packing.c64_recon_tables ----
@pytest.mark.parametrize("f", [64, 40, 24, 20])
def test_recon_tables_pack_every_parameter_exactly_once(f):
    t = P.c64_recon_tables(f)
    total = sum(int(np.prod(s)) for _, s in P.c64_recon_shapes(f))
    assert t["zero"] == total and t["size"] == total + 1 and t["pack"].max() <= total
    counts = np.bincount(t["pack"], minlength=total + 1)
    assert (counts[:total] == 1).all()                      # every real parameter once; every pad slot is the appended 0
    assert counts[total] == t["pack"].size - total
    sub = 2 * 36 * 512 + 64
    assert t["boff"] == [0, 2 * 8 * 512 + 64, 2 * 8 * 512 + 64 + 4 * sub, 2 * 8 * 512 + 64 + 8 * sub, 2 * 8 * 512 + 64 + 9 * sub]
    assert t["pack"].size == t["boff"][4] + 18 * 512 + 64 and all(o % 8 == 0 for o in t["boff"])
    assert t["off"]["upconv1.weight"] == f * 2 * f + f        # state_dict order: fusion.weight | fusion.bias | upconv1.weight ..


def _params(f, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g, dtype=torch.float64) for k, s in P.c64_recon_shapes(f)}


def _blob(p, f):
    t = P.c64_recon_tables(f)
    flat = np.concatenate([p[k].numpy().reshape(-1) for k, _ in P.c64_recon_shapes(f)] + [[0.0]])
    return flat[t["pack"]], t["boff"]


def _embed(x_nchw, cw):
    """(1, f, H, W) -> the kernels' (H, W, cw) NHWC image, channels >= f zero"""
    _, f, H, W = x_nchw.shape
    y = np.zeros((H, W, cw))
    y[..., :f] = x_nchw[0].permute(1, 2, 0).numpy()
    return y


def _emu_fusion(blob, fb, ff):
    """vr_fusion_kernel, lane by lane: fb, ff (H, W, cw) -> (H, W, 64) before the activation"""
    H, W, cw = fb.shape
    bias = blob[2 * 8 * 512:2 * 8 * 512 + 64]
    y = np.zeros((H, W, 64))
    for ty0 in range(0, H, 16):
        for tx0 in range(0, W, 16):
            for pt in range(8):
                pc = pt * 32 + E.R
                Y, X = ty0 + pc // 16, tx0 + pc % 16
                ok = (Y < H) & (X < W)
                Yc, Xc = np.where(ok, Y, 0), np.where(ok, X, 0)
                for ch in range(2):
                    acc = np.stack([bias[32 * ch + (i & 3) + 8 * (i >> 2) + 4 * E.HH] for i in range(16)], 1)
                    for s in range(8):
                        src = fb if s < 4 else ff
                        q = 2 * (s & 3) + E.HH
                        live = ok & (q * 8 < cw)
                        b = np.stack([np.where(live, src[Yc, Xc, np.minimum(q * 8 + j, cw - 1)], 0.0) for j in range(8)], 1)
                        acc = E.mma16(E.wfrag(blob, ch * 8 + s), b, acc)
                    for i in range(16):
                        co = 32 * ch + (i & 3) + 8 * (i >> 2) + 4 * E.HH
                        y[Y[ok], X[ok], co[ok]] = acc[ok, i]
    return y


@pytest.mark.parametrize("f,cw", [(64, 64), (40, 64), (24, 24), (20, 24)])
def test_packed_fusion_reproduces_conv2d(f, cw):
    p = _params(f, 100 + f)
    blob, boff = _blob(p, f)
    g = torch.Generator().manual_seed(f)
    xb, xf = (torch.randn(1, f, 18, 20, generator=g, dtype=torch.float64) for _ in range(2))
    y = _emu_fusion(blob[boff[0]:boff[1]], _embed(xb, cw), _embed(xf, cw))
    ref = F.conv2d(torch.cat([xb, xf], 1), p["fusion.weight"], p["fusion.bias"])[0].permute(1, 2, 0).numpy()
    assert np.abs(y[..., :f] - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.all(y[..., f:] == 0.0)


def _emu_upconv(blob, x_k):
    """vr_upconv_kernel: four conv64-shaped sub-convs q = 2 dy + dx of x_k (H, W, 64), each stored to pixel (2Y + dy, 2X + dx)"""
    H, W, _ = x_k.shape
    sub = 2 * 36 * 512 + 64
    y = np.zeros((2 * H, 2 * W, 64))
    for q in range(4):
        y[(q >> 1)::2, (q & 1)::2] = _emu_conv64(blob[q * sub:(q + 1) * sub], x_k, 64)
    return y


@pytest.mark.parametrize("f", [64, 24])
@pytest.mark.parametrize("layer", ["upconv1", "upconv2"])
def test_packed_upconv_and_shuffled_store_reproduce_pixel_shuffle_of_conv2d(f, layer):
    p = _params(f, 200 + f)
    blob, boff = _blob(p, f)
    k = 1 if layer == "upconv1" else 2
    g = torch.Generator().manual_seed(f + k)
    x = torch.randn(1, f, 18, 20, generator=g, dtype=torch.float64)
    y = _emu_upconv(blob[boff[k]:boff[k + 1]], _embed(x, 64))
    ref = F.pixel_shuffle(F.conv2d(x, p[layer + ".weight"], p[layer + ".bias"], padding=1), 2)[0].permute(1, 2, 0).numpy()
    co = ref.shape[-1]                                        # f for upconv1, 64 for upconv2
    assert co == (f if layer == "upconv1" else 64) and y.shape[:2] == ref.shape[:2] == (36, 40)
    assert np.abs(y[..., :co] - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.all(y[..., co:] == 0.0)


def test_packed_conv_hr_is_a_conv64_conv():
    p = _params(24, 7)
    blob, boff = _blob(p, 24)
    t = P.c64_tables(64, 64)
    src = np.concatenate([p["conv_hr.weight"].numpy().reshape(-1), p["conv_hr.bias"].numpy(), [0.0]])
    assert np.array_equal(blob[boff[3]:boff[4]], src[t["w"]])


# ---- conv_last on the 16 x 16 x 32 MFMA + the bilinear x4 base ----
def mma32(a, b, acc):
    """v_mfma_f32_16x16x32 conventions of csrc/vsr_recon.h: a, b (64, 8) fragments, lane l: A[row l & 15][k = 8 (l >> 4) + j],
    B[k][col l & 15]; acc (64, 4): reg i = D[row 4 (l >> 4) + i][col l & 15]"""
    A, B = np.zeros((16, 32)), np.zeros((32, 16))
    for j in range(8):
        A[E.LANE & 15, 8 * (E.LANE >> 4) + j] = a[:, j]
        B[8 * (E.LANE >> 4) + j, E.LANE & 15] = b[:, j]
    D = A @ B
    out = acc.copy()
    for i in range(4):
        out[:, i] += D[4 * (E.LANE >> 4) + i, E.LANE & 15]
    return out


def base_taps(d, n):
    """vr_tap: (i0, i1, l0, l1) of output indices d (int array) for a x4 upsample of n samples, in fp32"""
    src = np.float32(0.25) * (d.astype(np.float32) + np.float32(0.5)) - np.float32(0.5)
    src = np.maximum(src, np.float32(0.0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1.0) - l1).astype(np.float32), l1


def _fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in float64, and so is the sum of these operands (weights k / 8)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def base_x4(frame):
    """vr_base on a (C, h, w) float32 array, in the kernel's order: fma(l0y, top, l1y bot), top = fma(l0x, v00, l1x v01)"""
    _, h, w = frame.shape
    y0, y1, ly0, ly1 = base_taps(np.arange(4 * h), h)
    x0, x1, lx0, lx1 = base_taps(np.arange(4 * w), w)
    f = frame.astype(np.float32)
    v00, v01, v10, v11 = f[:, y0][:, :, x0], f[:, y0][:, :, x1], f[:, y1][:, :, x0], f[:, y1][:, :, x1]
    lx0, lx1 = np.broadcast_to(lx0, v00.shape), np.broadcast_to(lx1, v00.shape)
    ly0, ly1 = np.broadcast_to(ly0[:, None], v00.shape), np.broadcast_to(ly1[:, None], v00.shape)
    top = _fma(lx0, v00, (lx1 * v01).astype(np.float32))
    bot = _fma(lx0, v10, (lx1 * v11).astype(np.float32))
    return _fma(ly0, top, (ly1 * bot).astype(np.float32))


def test_base_weights_and_clamping_equal_interpolate_bit_for_bit():
    g = torch.Generator().manual_seed(19)
    fr = torch.rand(1, 3, 18, 20, generator=g)
    ref = F.interpolate(fr, scale_factor=4, mode="bilinear", align_corners=False)[0].numpy()
    got = base_x4(fr[0].numpy())
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    _, _, l0, l1 = base_taps(np.arange(4, 12), 18)
    assert set(l1.tolist()) == {0.125, 0.375, 0.625, 0.875} and np.all(l0 + l1 == 1.0)
    i0, i1, l0, l1 = base_taps(np.array([0, 1, 70, 71]), 18)   # borders: the source index clamps, as ATen's does
    assert i0.tolist() == [0, 0, 17, 17] and i1.tolist() == [1, 1, 17, 17] and l1[0] == 0.0 and l1[1] == 0.0


def _emu_last(blob, x_k, frame):
    """vr_last_kernel: x_k (H, W, 64) -> (3, H, W) = conv_last + bias + base(frame (3, H/4, W/4))"""
    H, W, _ = x_k.shape
    pad = np.zeros((H + 2, W + 2, 64))
    pad[1:-1, 1:-1] = x_k
    bias = blob[18 * 512:18 * 512 + 64]
    base = base_x4(frame).astype(np.float64)
    l16, kq = E.LANE & 15, E.LANE >> 4
    y = np.zeros((3, H, W))
    for ty0 in range(0, H, 16):
        for tx0 in range(0, W, 16):
            tile = np.zeros((34, 34, 64))
            sub = pad[ty0:ty0 + 18, tx0:tx0 + 18]
            tile[:sub.shape[0], :sub.shape[1]] = sub
            for oy in range(16):
                acc = np.stack([np.where((kq == 0) & (i < 3), bias[i], 0.0) for i in range(4)], 1)
                for s in range(18):
                    tap, c = s >> 1, s & 1
                    b = np.stack([tile[oy + tap // 3, l16 + tap % 3, 32 * c + 8 * kq + j] for j in range(8)], 1)
                    acc = mma32(E.wfrag(blob, s), b, acc)
                Y, X = ty0 + oy, tx0 + l16
                if Y >= H:
                    continue
                ok = (kq == 0) & (X < W)
                for c in range(3):
                    y[c, Y, X[ok]] = acc[ok, c] + base[c, Y, X[ok]]
    return y


def test_packed_conv_last_plus_base_reproduces_conv2d_plus_interpolate():
    p = _params(24, 9)
    blob, boff = _blob(p, 24)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(1, 64, 24, 40, generator=g, dtype=torch.float64)
    fr = torch.rand(1, 3, 6, 10, generator=g)
    y = _emu_last(blob[boff[4]:], _embed(x, 64), fr[0].numpy())
    ref = (F.conv2d(x, p["conv_last.weight"], p["conv_last.bias"], padding=1) +
           F.interpolate(fr.double(), scale_factor=4, mode="bilinear", align_corners=False))[0].numpy()
    assert np.abs(y - ref).max() <= 1e-6 * np.abs(ref).max()   # the base is computed in fp32
    assert np.all(blob[boff[4] + 18 * 512 + 3:] == 0.0)
