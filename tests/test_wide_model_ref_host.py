"""tests/wide_model_ref.py on the CPU: the composed whole-step reference agrees with the code it restates and was built from, and the
cases of tests/test_gpu_wide_batch.py tell clips and halves apart -- every seeded wiring defect moves a tensor more than ten times
outside the bound the GPU suite applies to it, in fp32 and in bf16."""
import time

import pytest
import torch

from tests import recon_bwd_ref as B
from tests import recon_ref as R
from tests import trunk_ref as T
from tests import wide_model_ref as W
from tests.parity_kit import bf16_round, bound, leaf, rel_max

CASES = [(kind, f, nb, b) for kind in W.KINDS for f, nb in W.WIDTHS for b in W.BATCHES]
_cid = lambda c: "%s-F%d-nb%d-b%d" % c


# ---- 1. agreement with existing code ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("f,nb", W.WIDTHS)
def test_float64_equals_the_aten_restatement(kind, f, nb, mode):
    """b = 2, the case of either mode: the output and every gradient group to 1e-12 of the largest element"""
    c, ref, _ = W.reference(kind, f, nb, 2, mode)
    aten = W.aten_step(kind, c["params"], c["x"], c["ff"], c["fb"], c["target"], nb, f, torch.float64)
    assert [k for k, _ in W.tensors(ref)] == [k for k, _ in W.tensors(aten)] == ["out"] + list(W.TRUNKS) + list(W.RECON[kind])
    for (name, got), (_, exp) in zip(W.tensors(ref), W.tensors(aten)):
        assert got.shape == exp.shape and got.dtype == torch.float64, name
        assert rel_max(got, exp) <= 1e-12, (name, rel_max(got, exp))


def test_propagation_is_step_ref_per_half():
    """hot = ident: every step state equals trunk_ref.step_ref (with its own warp) run on each half alone, loop by loop"""
    c = W.case("origin", 40, 1, 3)
    b, n, nb = 3, W.FRAMES, 1
    x, ff, fb = c["x"].double(), c["ff"].double(), c["fb"].double()
    pb, pf = ([c["params"][k].double() for k in W.trunk_keys(tr, nb)] for tr in W.TRUNKS)
    steps = W.propagate(pb, pf, x, ff, fb, nb)
    prev = None
    for k, i in enumerate(range(n - 1, -1, -1)):                       # the backward-time loop of the reference model
        prev = T.step_ref(x[:, i], prev, fb[:, i] if k else None, pb, nb)
        assert torch.equal(steps[k][:b], prev), ("backward", i)
    prev = None
    for i in range(n):
        prev = T.step_ref(x[:, i], prev, ff[:, i - 1] if i else None, pf, nb)
        assert torch.equal(steps[i][b:], prev), ("forward", i)


@pytest.mark.parametrize("hot", [R.ident, bf16_round], ids=["ident", "bf16"])
def test_origin_reconstruction_is_the_chain(hot):
    """hot = ident: forward and backward equal recon_bwd_ref.chain_forward / chain_backward bit for bit; through the autograd node
    too.  With the bf16 hooks the node still returns what origin_recon_backward computes on the stored images."""
    c = W.case("origin", 40, 1, 2)
    g = torch.Generator().manual_seed(3)
    p = {k: c["params"][k].double() for k in W.ORIGIN_RECON}
    fb, ff = (hot(torch.randn(2, 40, 9, 11, generator=g, dtype=torch.float64)) for _ in range(2))
    frame = torch.rand(2, 3, 9, 11, generator=g, dtype=torch.float64)
    cot = torch.randn(2, 3, 36, 44, generator=g, dtype=torch.float64)
    out, *images = W.origin_recon_forward(p, fb, ff, frame, torch.float64, hot)
    exp = W.origin_recon_backward(p, fb, ff, images, cot, torch.float64, hot)
    if hot is R.ident:
        for a, e in zip([out] + images, B.chain_forward(p, fb, ff, frame)):
            assert torch.equal(a, e)
        chain = B.chain_backward(p, fb, ff, frame, cot)
        assert set(chain) == set(exp) and all(torch.equal(exp[k], chain[k]) for k in chain)
    leaves = [leaf(fb), leaf(ff)] + [leaf(p[k]) for k in W.ORIGIN_RECON]
    node = W._OriginRecon.apply(leaves[0], leaves[1], frame, hot, *leaves[2:])
    assert torch.equal(node, out)
    node.backward(cot)
    for name, t in zip(("dfb", "dff") + W.ORIGIN_RECON, leaves):
        assert torch.equal(t.grad, exp[name]), name


@pytest.mark.parametrize("hot", [R.ident, bf16_round], ids=["ident", "bf16"])
def test_mv_reconstruction_is_mv_run(hot):
    c = W.case("mv", 40, 1, 2)
    g = torch.Generator().manual_seed(4)
    ps = [c["params"][k].double() for k in W.MV_RECON]
    fb, ff = (hot(torch.randn(6, 40, 9, 11, generator=g, dtype=torch.float64)) for _ in range(2))
    xs = torch.rand(6, 3, 9, 11, generator=g, dtype=torch.float64)
    cot = torch.randn(6, 3, 36, 44, generator=g, dtype=torch.float64)
    exp = R.mv_run(dict(f=40, b=2, n=3, fb=fb, ff=ff, x=xs, w_fu=ps[0], b_fu=ps[1], w_last=ps[2], b_last=ps[3], g=cot), torch.float64, hot)
    leaves = [leaf(fb), leaf(ff)] + [leaf(t) for t in ps]
    node = W._MvRecon.apply(leaves[0], leaves[1], xs, hot, *leaves[2:])
    assert torch.equal(node, exp["out"])
    node.backward(cot)
    for t, e in zip(leaves, (exp["dc"][:, :40], exp["dc"][:, 40:], exp["dW_fu"], exp["db_fu"], exp["dW_last"], exp["db_last"])):
        assert torch.equal(t.grad, e)


# ---- 2. seeded wiring defects --------------------------------------------------------------------------------------------------------
def test_the_cases_separate_clips_and_halves():
    for kind, f, nb, b in CASES:
        c = W.case(kind, f, nb, b)
        assert all(not torch.equal(c[k][0], c[k][j]) for k in ("x", "mv", "target") for j in range(1, b))
        assert float(c["mv"].abs().median()) >= 1.0                       # flows of a pixel or more
        assert float((c["ff"] - c["ff"].flip(1)).abs().max()) > 1.0


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_masks_of_the_two_case_families(case):
    """the fp32 cases keep every pre-activation in front of a LeakyReLU or ReLU at least W.MARGIN = 0.25 above zero in the float64 step (an fp32
    sum cannot then sign one differently, whatever its order: the stored activations of these cases stay below 5 and a row's sum of
    |w| below 13, so a sum of at most 9 x 67 + 1 products errs by less than 604 x 2^-24 x 65 = 2.4e-3); the bf16 cases have both signs
    in front of every mask"""
    kind, f, nb, b = case
    for positive in (True, False):
        c = W.case(kind, f, nb, b, positive)
        mins = W.pre_minima(kind, c["params"], c["x"], c["ff"], c["fb"], nb)
        assert len(mins) == 2 * (1 + nb) + (4 if kind == "origin" else 1)
        low = min(float(m.min()) for m in mins.values())
        print(f"wide case | {_cid(case)} | positive={positive} | smallest masked pre-activation {low:.3g}")
        if positive:
            assert low >= W.MARGIN - 1e-5, mins                            # the raised biases are stored in float32
        else:                                                              # every mask meets its negative side
            assert all(float(m.min()) < 0 for m in mins.values()), mins


@pytest.mark.parametrize("positive", [True, False], ids=["fp32-cases", "bf16-cases"])
@pytest.mark.parametrize("kind,f,nb", [("origin", 64, 2), ("mv", 40, 1)])
def test_clips_do_not_cancel(kind, f, nb, positive):
    """b = 3: no gradient group is a small difference of large per-clip contributions (two clips with coherent cotangents of opposite
    signs would leave a sum a fraction of its terms, and a relative bound on the sum would then measure the cancellation, not the
    kernel): the clips' largest elements together stay within 2 x the largest element of the sum"""
    c = W.case(kind, f, nb, 3, positive)
    total = W.run(kind, f, nb, 3, positive=positive)[1]
    per = [W.STEP[kind](c["params"], c["x"][k:k + 1], c["ff"][k:k + 1], c["fb"][k:k + 1], c["target"][k:k + 1], nb, f)[1] for k in range(3)]
    for name, t in total.items():
        assert rel_max(sum(p[name] for p in per) / 3, t) < 1e-12, name        # the clips are independent: the sum is the step
        parts = sum(float(p[name].abs().max()) for p in per) / 3
        print(f"wide case | {kind} F={f} positive={positive} | {name} | per-clip maxima / max of the sum {parts / float(t.abs().max()):.2f}")
        assert parts <= 2.0 * float(t.abs().max()), (name, parts, float(t.abs().max()))


@pytest.mark.parametrize("defect", W.DEFECTS)
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_seeded_defect_leaves_the_bound(case, defect):
    """the defect, applied to the float64 reference's own indexing, moves at least one asserted tensor by more than 10 x the bound
    tests/test_gpu_wide_batch.py applies to that tensor, in both modes, each on the case that mode is held on"""
    for mode in ("fp32", "bf16"):
        _, ref, yard = W.reference(*case, mode)
        bad = dict(W.tensors(W.run(*case, defect=defect, positive=W.POSITIVE[mode])))
        ratios = {k: rel_max(bad[k], v) / bound(mode, yard[k]) for k, v in W.tensors(ref)}
        worst = max(ratios, key=ratios.get)
        print(f"wide defect | {_cid(case)} | {defect} | {mode} | {worst} moves by {ratios[worst]:.1f} x its bound")
        assert ratios[worst] > 10.0, (mode, ratios)


# ---- 3. cost -------------------------------------------------------------------------------------------------------------------------
def test_reference_is_cached_and_cheap():
    big = ("origin", 64, 2, 3)
    t0 = time.perf_counter()
    W.run(*big)
    dt = time.perf_counter() - t0
    print(f"wide reference | {_cid(big)} | one float64 step {dt:.2f} s")
    assert dt < 20.0                                                       # a few seconds on a desktop CPU; a guard, not a benchmark
    assert W.reference(*big, "bf16") is W.reference(*big, "bf16") and W.case(*big) is W.case(*big)
