"""training.Adam on many parameter tensors: one sr_adam_step_multi launch per table of up to _lib.ADAM_MULTI_CAP tensors
(csrc/train_step.h adam_step_multi_kernel), parameters and state bit-identical to torch.optim.Adam; a lone tensor keeps sr_adam_step."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETAS = (0.9, 0.99)                                          # the video trainer's


def _count_launches(monkeypatch):
    from mobilesuperresolution_amd import _lib as L
    seen = []
    real = L.launch

    def launch(name, fn, *args):
        seen.append(name)
        return real(name, fn, *args)

    monkeypatch.setattr(L, "launch", launch)
    return seen


def test_many_tensors_step_bit_identically_in_two_launches(monkeypatch):
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.training import Adam
    cap, chunk = L.ADAM_MULTI_CAP, L.ADAM_MULTI_CHUNK
    sizes = [1, 3, 31, chunk + 1] + [8] * (cap - 3) + [8]                # cap + 1 tensors get a gradient, the last one none
    none_at = len(sizes) - 1
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(n, generator=g) for n in sizes]
    mine = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    theirs = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt, ref = Adam(mine, lr=1e-3, betas=BETAS), torch.optim.Adam(theirs, lr=1e-3, betas=BETAS)
    seen = _count_launches(monkeypatch)
    with_grad = len(sizes) - 1
    for step in range(3):
        for i, (p, q) in enumerate(zip(mine, theirs)):
            if i == none_at:
                p.grad = q.grad = None
                continue
            gr = torch.randn(sizes[i], generator=g).to(DEV)
            p.grad, q.grad = gr.clone(), gr.clone()
        del seen[:]
        opt.step()
        assert seen.count("sr_adam_step_multi") == math.ceil(with_grad / cap) == 2 and seen.count("sr_adam_step") == 0
        ref.step()
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(mine, theirs)):
        if i == none_at:
            assert torch.equal(p, init[i].to(DEV)) and len(opt.state[p]) == 0
            continue
        assert torch.equal(p, q), i
        assert torch.equal(opt.state[p]["exp_avg"], ref.state[q]["exp_avg"]), i
        assert torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"]), i
        assert int(opt.state[p]["step"]) == 3


def test_a_single_tensor_keeps_the_single_launch(monkeypatch):
    from mobilesuperresolution_amd.training import Adam
    p = torch.nn.Parameter(torch.randn(1500, generator=torch.Generator().manual_seed(4)).to(DEV))
    q = torch.nn.Parameter(p.detach().clone())
    opt, ref = Adam([p], lr=1e-3, betas=BETAS), torch.optim.Adam([q], lr=1e-3, betas=BETAS)
    seen = _count_launches(monkeypatch)
    p.grad = torch.randn(1500, generator=torch.Generator().manual_seed(5)).to(DEV)
    q.grad = p.grad.clone()
    opt.step()
    ref.step()
    assert seen == ["sr_adam_step"]
    assert torch.equal(p, q)


def test_tensors_that_joined_later_step_with_their_own_count(monkeypatch):
    """a tensor whose first gradient arrives at step 2 has step count 1 there: its bias corrections differ, it goes in its own group"""
    from mobilesuperresolution_amd.training import Adam
    g = torch.Generator().manual_seed(6)
    init = [torch.randn(n, generator=g) for n in (5, 9, 40)]
    mine = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    theirs = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt, ref = Adam(mine, lr=1e-3, betas=BETAS), torch.optim.Adam(theirs, lr=1e-3, betas=BETAS)
    seen = _count_launches(monkeypatch)
    for step in range(2):
        for i, (p, q) in enumerate(zip(mine, theirs)):
            if step == 0 and i == 2:
                continue
            gr = torch.randn(p.numel(), generator=g).to(DEV)
            p.grad, q.grad = gr.clone(), gr.clone()
        del seen[:]
        opt.step()
        ref.step()
        assert sorted(seen) == (["sr_adam_step_multi"] if step == 0 else ["sr_adam_step", "sr_adam_step_multi"])
    assert all(torch.equal(p, q) for p, q in zip(mine, theirs))


def test_bad_tables_are_refused():
    import ctypes
    from mobilesuperresolution_amd import _lib as L
    lib = L.lib()
    t = torch.zeros(8, device=DEV)
    scal = L.AdamScalars(0.1, 0.99, 0.01, 1.0, 1e-8, -1e-3)
    rows = (L.AdamRow * (L.ADAM_MULTI_CAP + 1))()
    for r in rows:
        r.param = r.grad = r.exp_avg = r.exp_avg_sq = t.data_ptr()
        r.n = 8
    s = L.stream_ptr()
    assert lib.sr_adam_step_multi(rows, L.ADAM_MULTI_CAP + 1, ctypes.byref(scal), s) == -2
    assert lib.sr_adam_step_multi(rows, 0, ctypes.byref(scal), s) == -2
    assert lib.sr_adam_step_multi(None, 1, ctypes.byref(scal), s) == -2
    rows[1].n = 0
    assert lib.sr_adam_step_multi(rows, 2, ctypes.byref(scal), s) == -2
    torch.cuda.synchronize()
    assert not bool(t.any())
