"""Result_Model (the NAS stage-3 network) on the host: status parser, module tree, seeded init and checkpoints against
fixture G18 (the reference's own Result_Model), the packed weight tables against F.conv2d, and the geometry limits."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mobilesuperresolution_amd import packing as P
from mobilesuperresolution_amd.models import Result_Model
from mobilesuperresolution_amd.models.result_model import parse_status

G18 = os.path.join(os.path.dirname(__file__), "golden", "g18_result_model.npz")
ARCH = {"a": (2, [[27, 16, 3], [27, 27, 5], [27, 9, 7]], 180), "b": (4, [[20, 20, 3], [20, 12, 5], [20, 8, 3]], 181)}


@pytest.fixture(scope="module")
def g18():
    return dict(np.load(G18))


def test_parse_status_last_line(tmp_path):
    f = tmp_path / "block_index.txt"
    f.write_text("([0], [[8, 8, 3]])\n([1, 2, 4], [[27, 16, 3], [27, 27, 5], [27, 9, 7]])\n")
    assert parse_status(str(f)) == [[27, 16, 3], [27, 27, 5], [27, 9, 7]]
    m = Result_Model(2, str(f))
    assert m.IN == 27 and m.F == 32 and m.idx == [[27, 16, 3], [27, 27, 5], [27, 9, 7]]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_keys_shapes_and_seeded_init_match_reference(g18, tag):
    scale, status, seed = ARCH[tag]
    torch.manual_seed(seed)
    m = Result_Model(scale, status=status)
    sd = m.state_dict()
    ref = {k[len(f"{tag}/init/"):]: v for k, v in g18.items() if k.startswith(f"{tag}/init/")}
    assert list(sd) == list(ref) and len(sd) == 18
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k].shape, k
        assert torch.equal(v, torch.from_numpy(ref[k])), k
    if tag == "a":
        assert tuple(sd[f"body.{len(status) + 1}.weight_v"].shape) == (12, 27, 7, 7)       # the last block's k
    assert m.receptive_halo() == max(2, 1 + sum(k // 2 for *_, k in status) + status[-1][2] // 2)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_checkpoint_round_trip(g18, tag, tmp_path):
    scale, status, _ = ARCH[tag]
    m = Result_Model(scale, status=status)
    ref = {k[len(f"{tag}/p/"):]: torch.from_numpy(v) for k, v in g18.items() if k.startswith(f"{tag}/p/")}
    m.load_state_dict(ref, strict=True)
    torch.save(m.state_dict(), tmp_path / "ck.pth")
    m2 = Result_Model(scale, status=status, hot_dtype="bf16")
    m2.load_state_dict(torch.load(tmp_path / "ck.pth"), strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, ref[k]), k


def _unpack(frags, rows, ks):
    """packed fragments [row tile][k-step][lane][8] -> the dense A matrix (rows, 16 ks) the kernel multiplies"""
    nrt = (rows + 31) // 32
    fr = frags.reshape(nrt, ks, 2, 32, 8)                     # lane = 32 hh + r
    return fr.permute(0, 3, 1, 2, 4).reshape(nrt * 32, ks * 16)[:rows]


def _im2col(x, k):
    """x (CI, H, W) -> B (K*K*CI padded to 16, H*W): row tap * CI + ci = x[ci] shifted by the tap (zero padding)"""
    ci, h, w = x.shape
    p = k // 2
    xp = F.pad(x, (p, p, p, p))
    rows = [xp[c, dy:dy + h, dx:dx + w].reshape(-1) for dy in range(k) for dx in range(k) for c in range(ci)]
    b = torch.stack(rows)
    ks = (k * k * ci + 15) // 16
    return torch.cat([b, b.new_zeros(ks * 16 - b.shape[0], h * w)]), ks


@pytest.mark.parametrize("F_,IN,split,k", [(32, 27, 16, 3), (32, 27, 27, 5), (32, 27, 9, 7), (24, 20, 12, 5), (24, 20, 20, 3)])
def test_block_tables_reproduce_conv2d_with_zero_embedding(F_, IN, split, k):
    g = torch.Generator().manual_seed(F_ * 100 + split * 10 + k)
    w = torch.randn(split, split, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(split, generator=g, dtype=torch.float64)
    x = torch.zeros(F_, 7, 9, dtype=torch.float64)
    x[:IN] = torch.randn(IN, 7, 9, generator=g, dtype=torch.float64)
    a = IN - split
    wd = torch.zeros(F_, F_, k, k, dtype=torch.float64)
    wd[a:IN, a:IN] = w
    idx = torch.from_numpy(P.rm_conv_index(F_, F_, k))
    frags = torch.cat([wd.reshape(-1), wd.new_zeros(1)])[idx]
    B, ks = _im2col(x, k)
    A = _unpack(frags, F_, ks)
    b32 = torch.zeros(F_, dtype=torch.float64)
    b32[a:IN] = b
    z = (A @ B + b32[:, None]).view(F_, 7, 9)
    y = x + torch.relu(z)
    ref = x.clone()
    ref[a:IN] = x[a:IN] + torch.relu(F.conv2d(x[None, a:IN], w, b, padding=k // 2)[0])
    assert torch.allclose(y, ref, rtol=0, atol=1e-12)
    assert torch.equal(y[IN:], torch.zeros_like(y[IN:])) and torch.equal(y[:a], x[:a])      # padded / pass-through rows
    # backward-data packs the transposed, flipped weights the same way: conv_k^T
    gy = torch.randn(F_, 7, 9, generator=g, dtype=torch.float64)
    gy[:a] = 0
    gy[IN:] = 0
    At = _unpack(torch.cat([wd.transpose(0, 1).flip(2, 3).reshape(-1), wd.new_zeros(1)])[idx], F_, ks)
    Bt, _ = _im2col(gy, k)
    dx = (At @ Bt).view(F_, 7, 9)
    xr = x[None, a:IN].clone().requires_grad_(True)
    (F.conv2d(xr, w, None, padding=k // 2) * gy[None, a:IN]).sum().backward()
    assert torch.allclose(dx[a:IN], xr.grad[0], rtol=0, atol=1e-10)
    assert torch.equal(dx[:a], torch.zeros_like(dx[:a])) and torch.equal(dx[IN:], torch.zeros_like(dx[IN:]))


@pytest.mark.parametrize("R,k", [(2, 7), (3, 5), (4, 7)])
def test_tail_tables_and_bias_fold(R, k):
    """k x k tail: rows 3 R^2 (one or two row tiles), inputs F with zero columns past IN; the skip + bias go through the 3x3
    tail source with zero 3x3 weights and btot = bt + bs (the 3x3 kernel's `+ mean` slot holds no mean here)"""
    F_, IN, co = 24, 20, 3 * R * R
    g = torch.Generator().manual_seed(R * 10 + k)
    wt = torch.randn(co, IN, k, k, generator=g, dtype=torch.float64)
    wtd = torch.zeros(co, F_, k, k, dtype=torch.float64)
    wtd[:, :IN] = wt
    feat = torch.zeros(F_, 5, 6, dtype=torch.float64)
    feat[:IN] = torch.randn(IN, 5, 6, generator=g, dtype=torch.float64)
    B, ks = _im2col(feat, k)
    A = _unpack(torch.cat([wtd.reshape(-1), wtd.new_zeros(1)])[torch.from_numpy(P.rm_conv_index(co, F_, k))], co, ks)
    ref = F.conv2d(feat[None, :IN], wt, None, padding=k // 2)[0]
    assert torch.allclose((A @ B).view(co, 5, 6), ref, rtol=0, atol=1e-10)
    ot = P.EndsGeom(F_, R).tail_off
    assert ot["b"] == co * F_ * 9 + co * 75 and ot["size"] == ot["b"] + co + 2


@pytest.mark.parametrize("ca,rows,cols,k", [(32, 27, 32, 3), (24, 24, 24, 7), (48, 48, 24, 7), (16, 12, 32, 5)])
def test_wgrad_gather_is_injective(ca, rows, cols, k):
    iw, ib = P.rm_wgrad_index(ca, rows, cols, k)
    assert len(np.unique(iw)) == iw.size and len(np.unique(ib)) == ib.size and not set(iw) & set(ib)
    assert iw.max() < P.rm_wgrad_groups(ca, k) * P.RM_WGRAD_TPG * 1024


def test_unsupported_geometry_raises():
    with pytest.raises(NotImplementedError, match="IN = 40"):
        Result_Model(2, status=[[40, 8, 3]])
    with pytest.raises(NotImplementedError, match="scale 1"):
        Result_Model(1, status=[[16, 8, 3]])
    with pytest.raises(NotImplementedError, match="kernel size 9"):
        Result_Model(2, status=[[16, 8, 9]])
    with pytest.raises(NotImplementedError, match="split"):
        Result_Model(2, status=[[16, 17, 3]])
    with pytest.raises(NotImplementedError, match="widths differ"):
        Result_Model(2, status=[[16, 8, 3], [12, 8, 3]])


def test_forward_needs_a_device():
    from mobilesuperresolution_amd._lib import HotpathError
    m = Result_Model(2, status=[[16, 8, 3]])
    with pytest.raises(HotpathError):
        m(torch.rand(1, 3, 8, 8))


@pytest.mark.parametrize("F_,IN,split,k", [(32, 27, 16, 3), (24, 20, 8, 7), (32, 32, 32, 5)])
def test_direct_block_gathers_equal_the_dense_embedding(F_, IN, split, k):
    g = torch.Generator().manual_seed(split * k)
    w = torch.randn(split, split, k, k, generator=g)
    b = torch.randn(split, generator=g)
    a = IN - split
    wd = torch.zeros(F_, F_, k, k)
    wd[a:IN, a:IN] = w
    src = torch.cat([w.reshape(-1), torch.zeros(1)])
    for tr, dense in ((False, wd), (True, wd.transpose(0, 1).flip(2, 3))):
        ref = torch.cat([dense.reshape(-1), torch.zeros(1)])[torch.from_numpy(P.rm_conv_index(F_, F_, k))]
        assert torch.equal(src[torch.from_numpy(P.rm_block_index(F_, IN, split, k, tr))], ref)
    b32 = torch.cat([b, torch.zeros(1)])[torch.from_numpy(P.rm_block_bias_index(IN, split))]
    assert torch.equal(b32[a:IN], b) and b32[:a].abs().sum() == 0 and b32[IN:].abs().sum() == 0
    iw, ib = P.rm_block_wgrad_index(F_, IN, split, k)
    fw, fb = P.rm_wgrad_index(F_, F_, F_, k)
    assert np.array_equal(iw.reshape(split, split, k * k), fw.reshape(F_, F_, k * k)[a:IN, a:IN]) and np.array_equal(ib, fb[a:IN])
