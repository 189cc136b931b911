"""Host side of the HIP reconstruction backward of BasicVSR_origin (csrc/vsr_recon_bwd.h): the float64 reference of
tests/recon_bwd_ref.py against torch.autograd on the reference formula, packing.c64_recon_bwd_tables (the transposed blob and the
reduce table), and the route rule of models/basicvsr_arch_origin.py.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mobilesuperresolution_amd import packing as P
from tests import recon_bwd_ref as B
from tests.parity_kit import rel_max


def _params(f, g):
    return {k: torch.randn(s, generator=g, dtype=torch.float64) / max(1.0, float(np.prod(s[1:])) ** 0.5) for k, s in P.c64_recon_shapes(f)}


@pytest.mark.parametrize("f", [25, 40])
def test_reference_against_autograd(f):
    g = torch.Generator().manual_seed(5)
    p = {k: v.requires_grad_(True) for k, v in _params(f, g).items()}
    fb = torch.randn(2, f, 3, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    ff = torch.randn(2, f, 3, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    frame = torch.rand(2, 3, 3, 5, generator=g, dtype=torch.float64)
    cot = torch.randn(2, 3, 12, 20, generator=g, dtype=torch.float64)
    out = B.chain_forward(p, fb, ff, frame)[0]
    out.backward(cot)
    with torch.no_grad():
        got = B.chain_backward({k: v.detach() for k, v in p.items()}, fb.detach(), ff.detach(), frame, cot)
    for k, v in p.items():
        assert rel_max(got[k], v.grad) < 1e-12, k
    assert rel_max(got["dfb"], fb.grad) < 1e-12 and rel_max(got["dff"], ff.grad) < 1e-12


def _blob_conv(pack, start, src):
    """a conv64-shaped blob section read back as the (64, 64, 3, 3) weight c64_conv_kernel applies (c64_tables' fragment layout)"""
    fr, r, hh, j = P._grid(2 * 36)
    ch, s = fr // 36, fr % 36
    tap, c = s // 4, s % 4
    w = torch.zeros(64, 64, 9, dtype=torch.float64)
    vals = src[torch.from_numpy(pack[start:start + 2 * 36 * 512])].reshape(fr.shape)
    w[torch.from_numpy(32 * ch + r), torch.from_numpy(16 * c + 8 * hh + j), torch.from_numpy(tap)] = vals
    assert bool((src[torch.from_numpy(pack[start + 2 * 36 * 512:start + 2 * 36 * 512 + 64])] == 0).all())      # zero biases
    return w.view(64, 64, 3, 3)


@pytest.mark.parametrize("f", [25, 40, 64])
def test_transposed_blob_is_the_backward_conv(f):
    """c64_conv_kernel on each section of the blob computes the transposed conv of the layer (of sub-conv q), channels >= F zero"""
    t = P.c64_recon_bwd_tables(f)
    g = torch.Generator().manual_seed(f)
    p = _params(f, g)
    src = torch.cat([p[k].reshape(-1) for k, _ in P.c64_recon_shapes(f)] + [torch.zeros(1, dtype=torch.float64)])
    pack, boff = t["pack"], t["boff"]
    assert pack.max() == t["zero"] and pack.min() >= 0

    def held(name, got, exp):
        real = exp.shape[1]
        assert rel_max(got[:, :real], exp) < 1e-12, name
        assert bool((got[:, real:] == 0).all()), name

    dz = torch.zeros(1, 64, 4, 5, dtype=torch.float64)
    dz[:, :f] = torch.randn(1, f, 4, 5, generator=g, dtype=torch.float64)
    wfu = p["fusion.weight"]
    for k, half in ((0, wfu[:, :f]), (1, wfu[:, f:])):
        held(f"fusion {k}", F.conv2d(dz, _blob_conv(pack, boff[k], src), padding=1), F.conv_transpose2d(dz[:, :f], half))
    for k, key, co_real in ((2, "upconv1", f), (3, "upconv2", 64)):
        w = p[key + ".weight"]
        for q in range(4):
            dq = torch.zeros(1, 64, 4, 5, dtype=torch.float64)
            dq[:, :co_real] = torch.randn(1, co_real, 4, 5, generator=g, dtype=torch.float64)
            got = F.conv2d(dq, _blob_conv(pack, boff[k] + q * P.C64_BWD_CONV_ELEMS, src), padding=1)
            held(f"{key} q={q}", got, F.conv_transpose2d(dq[:, :co_real], w[q::4], padding=1))
    dq = torch.randn(1, 64, 4, 5, generator=g, dtype=torch.float64)
    held("conv_hr", F.conv2d(dq, _blob_conv(pack, boff[4], src), padding=1), F.conv_transpose2d(dq, p["conv_hr.weight"], padding=1))
    last = src[torch.from_numpy(pack[boff[5]:boff[5] + 27 * 64])].view(3, 9, 64)
    assert torch.equal(last, p["conv_last.weight"].reshape(3, 64, 9).permute(0, 2, 1))
    assert pack.size == boff[5] + 27 * 64
    # only real rows and columns: every real weight is named exactly once, nothing else is
    named = pack[pack != t["zero"]]
    n_w = sum(int(np.prod(s)) for k, s in P.c64_recon_shapes(f) if k.endswith("weight"))
    assert named.size == n_w and np.unique(named).size == n_w


@pytest.mark.parametrize("f", [25, 40, 64])
def test_reduce_table_names_every_gradient_element_once(f):
    t = P.c64_recon_bwd_tables(f)
    red = t["reduce"].astype(np.int64)
    assert red.size == t["zero"] == sum(int(np.prod(s)) for _, s in P.c64_recon_shapes(f))
    S, NS = P.C64_RECON_BWD_WSLAB, P.C64_RECON_BWD_NSEC
    assert red.min() >= 0 and red.max() < t["per_wg"] == NS * S + P.C64_RECON_BWD_LAST_SLAB
    # fusion.bias is read from the backward-state section, whose bias tiles the forward-state section repeats: unique otherwise
    assert np.unique(red).size == red.size
    sec, o = red // S, 0
    want = {"fusion.weight": {0, 1}, "fusion.bias": {0}, "upconv1.weight": {2, 3, 4, 5}, "upconv1.bias": {2, 3, 4, 5},
            "upconv2.weight": {6, 7, 8, 9}, "upconv2.bias": {6, 7, 8, 9}, "conv_hr.weight": {10}, "conv_hr.bias": {10},
            "conv_last.weight": {11}, "conv_last.bias": {11}}
    for key, shape in P.c64_recon_shapes(f):
        n = int(np.prod(shape))
        assert set(sec[o:o + n].tolist()) == want[key], key
        o += n
    # a weight-gradient slab is [tile 38][reg 16][lane 64] with output columns in lanes (col + 32 hh): an element of a sub-conv with
    # F real outputs sits in a column < F of its pair of tiles (ob = 0: columns 0..31, ob = 1: 32..63)
    e = red[sec < NS] % S
    tile, lane = e // 1024, e % 64
    col = lane % 32 + 32 * np.where(tile < 36, tile % 2, tile - 36)
    k = sec[sec < NS]
    assert (col[k < 6] < f).all() and (col < 64).all()
    # the upconv sub-conv of output channel o is q = o % 4
    o1 = P.c64_recon_tables(f)["off"]["upconv1.weight"]
    assert (sec[o1:o1 + 4 * f * f * 9].reshape(4 * f, -1) == 2 + (np.arange(4 * f) % 4)[:, None]).all()
    with pytest.raises(ValueError):
        P.c64_recon_bwd_tables(24)


def _model(f=40, nb=1):
    from mobilesuperresolution_amd.models import BasicVSR_origin
    torch.manual_seed(3)
    return BasicVSR_origin(f, nb)


def test_route_rule_names_the_failing_condition():
    from mobilesuperresolution_amd.models import set_wide_training
    x = torch.rand(1, 3, 3, 6, 8)
    ff, fb = torch.zeros(1, 2, 2, 6, 8), torch.zeros(1, 2, 2, 6, 8)
    rule = lambda m, hw=(24, 32), x=x, ff=ff, fb=fb: m._hot_training_route(x, ff, fb, *hw)
    m = _model()
    assert type(m).hot_training is False and m.hot_training is False
    assert rule(m) == (False, "hot_training is not set")                      # the default
    assert len(set_wide_training(m)) == 2 and m.hot_training is False
    assert rule(m) == (False, "hot_training is not set")                      # set_wide_training alone keeps the ATen reconstruction
    m.hot_training = True
    assert m.backward_trunk.hot_training and m.forward_trunk.hot_training
    m.forward_trunk.hot_training = False
    assert rule(m) == (False, "hot_training is not set on both trunks")
    m.hot_training = True
    other, m.forward_trunk = m.forward_trunk, m.backward_trunk
    assert rule(m) == (False, "the trunks are not paired")
    m.forward_trunk = other
    assert rule(m, (25, 32)) == (False, "(height, weight) != (4h, 4w)")
    assert rule(m, x=x.clone().requires_grad_(True)) == (False, "x or a flow requires grad")
    assert rule(m, ff=ff.clone().requires_grad_(True)) == (False, "x or a flow requires grad")
    m.aten_reconstruction = True
    assert rule(m) == (False, "aten_reconstruction is set")
    m.aten_reconstruction = False
    h = m.upconv2.register_forward_hook(lambda *a: None)
    assert rule(m) == (False, "a hook sits on a reconstruction layer")
    h.remove()
    assert rule(m) == (False, "the tensors are not on the GPU")               # every other condition holds: CPU tensors alone
    m.hot_training = False
    assert not m.backward_trunk.hot_training and rule(m) == (False, "hot_training is not set")
    narrow = _model(24, 1)
    narrow.hot_training = True                                                 # changes nothing at F <= 24
    assert rule(narrow) == (False, "num_feat <= 24 trains on the 24-wide route")
