"""Host side of the video trainers' loss fold and of the multi-tensor Adam step (no GPU): the float64 reference of the folded gradient
source, the Adam table builder and the criterion's node lookup (the fold rule itself: tests/test_loss_fold_host.py)."""
import types

import pytest
import torch

from tests import frame_net_ref as FR
from tests import frame_net_train_ref as FT
from tests import multi_frame_ref as MR
from tests import multi_frame_train_ref as MT
from tests import video_fold_ref as V


def _autograd_grad(sr, hr, kind):
    leaf = sr.double().clone().requires_grad_(True)
    d = leaf - hr.double()
    loss = d.abs().mean() if kind == "l1" else torch.sqrt(d * d + V.EPS).mean()
    g, = torch.autograd.grad(loss, leaf)
    return loss.detach(), g


def _same(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("kind", V.KINDS)
def test_single_reference_backward_takes_the_closed_form_loss_gradient(kind):
    case = FR.rounded_case(8, 1, 2, 5, 6)
    x, p = case["x"], case["p"]
    sr = FR.forward(x, p)["out"]
    hr = torch.rand(sr.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    loss, g_auto = _autograd_grad(sr, hr, kind)
    _same(V.loss_value(sr, hr, kind), loss)
    closed = FT.flat_grads(FT.backward(x, p, V.loss_grad(sr, hr, kind))["grads"])
    auto = FT.flat_grads(FT.backward(x, p, g_auto)["grads"])
    assert [k for k, _ in closed] == [k for k, _ in auto] and len(closed) == 2 * 3 + 4
    for (k, a), (_, b) in zip(closed, auto):
        assert a.abs().max() > 0, k
        _same(a, b)


@pytest.mark.parametrize("kind", V.KINDS)
def test_multi_reference_backward_takes_the_closed_form_loss_gradient(kind):
    case = MR.rounded_case(8, 2, 1, 2, 5, 6)
    x, flows, p = case["x"], case["flows"], case["p"]
    sr = MR.forward(x, flows, p)["out"]
    hr = torch.rand(sr.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    loss, g_auto = _autograd_grad(sr, hr, kind)
    _same(V.loss_value(sr, hr, kind), loss)
    closed = MT.flat_grads(MT.backward(x, flows, p, V.loss_grad(sr, hr, kind))["grads"])
    auto = MT.flat_grads(MT.backward(x, flows, p, g_auto)["grads"])
    assert [k for k, _ in closed] == [k for k, _ in auto] and closed
    for (k, a), (_, b) in zip(closed, auto):
        assert a.abs().max() > 0, k
        _same(a, b)


def test_kernel_formula_is_the_closed_form():
    g = torch.Generator().manual_seed(2)
    sr, hr = torch.rand(2, 3, 8, 8, generator=g), torch.rand(2, 3, 8, 8, generator=g)
    hr[0, 0, 0, 0] = sr[0, 0, 0, 0]                                      # d = 0: sign 0, charbonnier 0
    for kind in V.KINDS:
        torch.testing.assert_close(V.kernel_formula_fp32(sr, hr, kind).double(), V.loss_grad(sr, hr, kind), rtol=1e-5, atol=1e-12)
        assert V.loss_grad(sr, hr, kind)[0, 0, 0, 0] == 0


# ---- the Adam table builder ---------------------------------------------------------------------------------------------------------
def _params(sizes, none_at=()):
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
    for i, p in enumerate(ps):
        p.grad = None if i in none_at else torch.zeros_like(p)
    return ps


def _covered(table, chunk):
    """per row: the element ranges of its workgroups, and the table's workgroup count"""
    blocks = 0
    for p, n, blk0 in table:
        assert blk0 == blocks and n == p.numel() and n >= 1
        nblk = -(-n // chunk)
        seen = torch.zeros(n, dtype=torch.int64)
        for j in range(nblk):
            seen[j * chunk:min((j + 1) * chunk, n)] += 1
        assert bool((seen == 1).all())                                  # every element exactly once
        blocks += nblk
    return blocks


def test_adam_tables_cover_every_element_once():
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.training import Adam
    chunk, cap = L.ADAM_MULTI_CHUNK, L.ADAM_MULTI_CAP
    assert (chunk, cap) == (1024, 80)
    sizes = [1, 3, chunk - 1, chunk, chunk + 1]
    ps = _params(sizes)
    tables = Adam._tables(ps)
    assert len(tables) == 1 and [r[0] for r in tables[0]] == ps
    assert [r[2] for r in tables[0]] == [0, 1, 2, 3, 4] and _covered(tables[0], chunk) == 6
    # capacity + 1 tensors make two tables, the second starting again at workgroup 0
    ps = _params([8] * (cap + 1))
    tables = Adam._tables(ps)
    assert [len(t) for t in tables] == [cap, 1] and tables[1][0][2] == 0
    assert [r[0] for t in tables for r in t] == ps and [_covered(t, chunk) for t in tables] == [cap, 1]
    # tensors without a gradient are absent and take no workgroup
    ps = _params([5, chunk + 1, 7, 9], none_at=(1, 3))
    tables = Adam._tables(ps)
    assert len(tables) == 1 and [r[0] for r in tables[0]] == [ps[0], ps[2]] and _covered(tables[0], chunk) == 2
    assert Adam._tables(_params([4, 4], none_at=(0, 1))) == []
    # other capacities and chunks follow the same rule
    tables = Adam._tables(_params([10, 1, 21]), capacity=2, chunk=10)
    assert [[(n, b) for _, n, b in t] for t in tables] == [[(10, 0), (1, 1)], [(21, 0)]]


# ---- the criterion's node lookup -----------------------------------------------------------------------------------------------------
def _fake_node(name, **attrs):
    return type(name, (), attrs)()


def test_network_node_knows_the_video_nodes():
    from mobilesuperresolution_amd import training as TR
    for name in ("_NetFunctionBackward", "_TailFunctionBackward", "_FrameNetTrainBackward", "_MultiFrameTrainBackward"):
        node = _fake_node(name, run_folded=lambda *a: None)
        assert TR._network_node(types.SimpleNamespace(grad_fn=node)) is node, name
        assert TR._network_node(types.SimpleNamespace(grad_fn=_fake_node(name))) is None      # the name without the protocol
    assert TR._network_node(types.SimpleNamespace(grad_fn=_fake_node("MulBackward0", run_folded=None))) is None
    assert TR._network_node(torch.zeros(3)) is None
    assert TR._network_node((torch.zeros(3, requires_grad=True) * 2)) is None


def test_hot_loss_keeps_torch_ops_for_foreign_tensors():
    from mobilesuperresolution_amd import training as TR
    sr = (torch.rand(2, 3, 4, 4) * 1.0).requires_grad_(True) * 2
    hr = torch.rand(2, 3, 4, 4)
    for crit, kind in ((TR.L1Loss(), "l1"), (TR.L1_Charbonnier_loss(), "charbonnier")):
        loss = crit(sr, hr)
        assert type(loss.grad_fn).__name__ != "_FoldedCriterionBackward"
        torch.testing.assert_close(loss.double(), V.loss_value(sr.detach(), hr, kind), rtol=1e-5, atol=0)
