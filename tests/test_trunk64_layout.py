"""CPU checks of the 64-feature (inference) propagation trunk: flat parameter layout and init = the reference's, checkpoint
round trips, a lane-level numpy model of csrc/conv64.h's k-steps applied to packing.c64_tables' packed blob against
F.conv2d, and fixture G17 against a plain-torch restatement of the reference's propagation loops (no GPU)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mobilesuperresolution_amd import packing as P
from mobilesuperresolution_amd.models import ConvResidualBlocks
from mobilesuperresolution_amd.models.basicvsr_arch import ResidualBlockNoBN
from tests import mfma_emu as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _reference_shaped(nin, f, nb):
    """plain modules with the reference's structure and key names (models/basicvsr_arch.py:108-147)"""
    return nn.Sequential(nn.Conv2d(nin, f, 3, 1, 1), nn.Identity(), nn.Sequential(*[ResidualBlockNoBN(f) for _ in range(nb)]))


@pytest.mark.parametrize("nin,f,nb", [(67, 64, 3), (64, 64, 2), (43, 40, 1)])
def test_flat_layout_is_reference_state_dict_order_and_same_init(nin, f, nb):
    torch.manual_seed(5)
    m = ConvResidualBlocks(nin, f, nb, "bf16")
    torch.manual_seed(5)
    ref = _reference_shaped(nin, f, nb).state_dict(prefix="main.")
    sd = m.state_dict()
    assert m.wide and list(sd.keys()) == list(ref.keys())
    assert [n for n, _ in m.named_parameters()] == ["flat"]
    off = 0
    for k, v in ref.items():
        assert torch.equal(sd[k], v), k
        assert torch.equal(m.flat.detach()[off:off + v.numel()].view(v.shape), v)
        off += v.numel()
    assert off == m.flat.numel()
    st = m.__getstate__()
    assert "_blob" not in st and "flat" not in st            # parameters travel through _parameters, the packed cache never


def test_width_classes():
    assert not ConvResidualBlocks(27, 24, 1).wide and ConvResidualBlocks(27, 24, 1).cin_k == 27
    assert ConvResidualBlocks(28, 25, 1).wide and ConvResidualBlocks(67, 64, 1).cin_k == 80 and ConvResidualBlocks(64, 64, 1).cin_k == 64
    with pytest.raises(NotImplementedError):
        ConvResidualBlocks(68, 65, 1)
    with pytest.raises(NotImplementedError):
        ConvResidualBlocks(66, 64, 1)


def test_checkpoint_round_trip_trunk_and_whole_model():
    src = _reference_shaped(67, 64, 2).state_dict(prefix="main.")
    m = ConvResidualBlocks(67, 64, 2, "fp32")
    assert m.load_state_dict(src, strict=True).missing_keys == []
    for k, v in m.state_dict().items():
        assert torch.equal(v, src[k])
    from mobilesuperresolution_amd.models.basicvsr_arch_origin import BasicVSR_origin
    a, b = BasicVSR_origin(64, 2), BasicVSR_origin(64, 2)
    ck = {k: torch.randn(v.shape) for k, v in a.state_dict().items()}
    trunk_keys = [k[len("backward_trunk."):] for k in ck if k.startswith("backward_trunk.")]
    assert trunk_keys == list(src.keys())                   # the reference's key set of a 2-block trunk
    b.load_state_dict(ck, strict=True)
    for k, v in b.state_dict().items():
        assert torch.equal(v, ck[k]), k


def test_trunk_tables_are_per_conv_tables_at_flat_offsets():
    nin, f, nb = 43, 40, 2
    pack, boff, ci_k = P.c64_trunk_tables(nin, f, nb)
    total = (f * nin * 9 + f) + 2 * nb * (f * f * 9 + f)
    assert ci_k == 80 and pack.max() == total and len(boff) == 1 + 2 * nb
    assert boff[1] - boff[0] == 2 * 45 * 512 + 64 and boff[2] - boff[1] == 2 * 36 * 512 + 64
    used = np.zeros(total + 1, dtype=bool)
    used[pack] = True
    assert used[:total].all()                                # every real parameter is packed; padding -> the appended 0


def _emu_conv64(blob, x_k, ci_k):
    """csrc/conv64.h c64_conv_kernel on one image, lane by lane: x_k (H, W, ci_k) in the kernels' channel order -> (H, W, 64)
    before the activation.  16 x 16 tiles, pixel tile pt = 32 consecutive core pixels, output half ch, k-step s = (tap, chunk c)."""
    H, W, _ = x_k.shape
    cpt, ks = ci_k // 16, 9 * ci_k // 16
    pad = np.zeros((H + 2, W + 2, ci_k))
    pad[1:-1, 1:-1] = x_k
    bias = np.asarray(blob[2 * ks * 512:2 * ks * 512 + 64], dtype=np.float64)
    y = np.zeros((H, W, 64))
    for ty0 in range(0, H, 16):
        for tx0 in range(0, W, 16):
            tile = np.zeros((18 + 16, 18 + 16, ci_k))          # out-of-image reads of partial tiles see zeros
            sub = pad[ty0:ty0 + 18, tx0:tx0 + 18]
            tile[:sub.shape[0], :sub.shape[1]] = sub
            for pt in range(8):
                pc = pt * 32 + E.R
                oy, ox = pc // 16, pc % 16
                for ch in range(2):
                    acc = np.stack([bias[32 * ch + (i & 3) + 8 * (i >> 2) + 4 * E.HH] for i in range(16)], 1)
                    for s in range(ks):
                        tap, c = s // cpt, s % cpt
                        b = np.stack([tile[oy + tap // 3, ox + tap % 3, 16 * c + 8 * E.HH + j] for j in range(8)], 1)
                        acc = E.mma16(E.wfrag(blob, ch * ks + s), b, acc)
                    for i in range(16):
                        co = 32 * ch + (i & 3) + 8 * (i >> 2) + 4 * E.HH
                        Y, X = ty0 + oy, tx0 + ox
                        ok = (Y < H) & (X < W)
                        y[Y[ok], X[ok], co[ok]] = acc[ok, i]
    return y


@pytest.mark.parametrize("f", [64, 40])
@pytest.mark.parametrize("warped_width", [True, False])
def test_packed_blob_reproduces_conv2d(f, warped_width):
    g = torch.Generator().manual_seed(f + warped_width)
    ci = f + 3 if warped_width else f
    H, W = 18, 20
    wt = torch.randn(f, ci, 3, 3, generator=g, dtype=torch.float64)
    bt = torch.randn(f, generator=g, dtype=torch.float64)
    x = torch.randn(1, ci, H, W, generator=g, dtype=torch.float64)
    t = P.c64_tables(ci, f)
    src = np.concatenate([wt.numpy().reshape(-1), bt.numpy(), [0.0]])
    blob = src[t["w"]]
    xn = x[0].permute(1, 2, 0).numpy()
    x_k = np.zeros((H, W, t["ci_k"]))
    if warped_width:                                         # [frame | state] -> [state | frame | 0]
        x_k[..., :f] = xn[..., 3:]
        x_k[..., 64:67] = xn[..., :3]
    else:
        x_k[..., :f] = xn
    y = _emu_conv64(blob, x_k, t["ci_k"])
    ref = F.conv2d(x, wt, bt, padding=1)[0].permute(1, 2, 0).numpy()
    assert np.abs(y[..., :f] - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.all(y[..., f:] == 0.0)                         # embedded rows: exactly zero


def _flow_warp_cpu(x, flow):
    """the reference's flow_warp (bilinear, zeros padding, align_corners=True) in plain torch"""
    _, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=x.dtype), torch.arange(w, dtype=x.dtype), indexing="ij")
    vx = 2.0 * (gx + flow[..., 0]) / max(w - 1, 1) - 1.0
    vy = 2.0 * (gy + flow[..., 1]) / max(h - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((vx, vy), 3), mode="bilinear", padding_mode="zeros", align_corners=True)


def _trunk_cpu(p, prefix, x, nb):
    y = F.leaky_relu(F.conv2d(x, p[f"{prefix}main.0.weight"], p[f"{prefix}main.0.bias"], padding=1), 0.1)
    for i in range(nb):
        q = f"{prefix}main.2.{i}."
        t = F.relu(F.conv2d(y, p[q + "conv1.weight"], p[q + "conv1.bias"], padding=1))
        y = y + F.conv2d(t, p[q + "conv2.weight"], p[q + "conv2.bias"], padding=1)
    return y


def propagate_cpu(d):
    """backward / forward features of the reference's two propagation loops (basicvsr_arch_origin.py:61-82), in call order"""
    p = {k[2:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("p/")}
    x = torch.from_numpy(d["x"])
    fb, ff = torch.from_numpy(d["flows_backward"]), torch.from_numpy(d["flows_forward"])
    b, n, _, h, w = x.shape
    nb = len({k.split(".")[3] for k in p if k.startswith("backward_trunk.main.2.")})
    out = {}
    for name, flows, order in (("backward", fb, range(n - 1, -1, -1)), ("forward", ff, range(n))):
        feat, res = x.new_zeros(b, 64, h, w), []
        for i in order:
            if res:
                feat = _flow_warp_cpu(feat, flows[:, i if name == "backward" else i - 1].permute(0, 2, 3, 1))
            feat = _trunk_cpu(p, f"{name}_trunk.", torch.cat([x[:, i], feat], 1), nb)
            res.append(feat)
        out[name] = torch.stack(res, 1)
    return out


def test_g17_is_self_consistent_with_a_plain_torch_restatement():
    d = dict(np.load(os.path.join(GOLDEN, "g17_vsr_trunk64.npz")))
    assert d["x"].shape == (1, 3, 3, 18, 20) and d["feat_forward"].shape == (1, 3, 64, 18, 20)
    assert not any(k.startswith("p/") and "_trunk." not in k for k in d)       # no reconstruction weights
    out = propagate_cpu(d)
    for name in ("backward", "forward"):
        ref = torch.from_numpy(d[f"feat_{name}"])
        assert (out[name] - ref).abs().max() <= 1e-5 * ref.abs().max(), name
