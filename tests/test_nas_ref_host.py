"""tests/nas_ref.py on the host: the float64 block reference against oracle.wdsr_oracle (split_block_forward_body with mg = 1 and
the gate open; nas_block_forward with the global mask and both gates) on random fp32 state dicts -- output and every autograd
gradient -- and the exactness conditions of every exact case the GPU tests use, checked on the float64 reference alone."""
import pytest
import torch

from oracle import wdsr_oracle as O
from tests import nas_ref as R, parity_kit as K


def _state_dict(f, g, ms_scale=0.7):
    sd = {"split.weight": torch.rand(f, 1, 1, 1, generator=g) * ms_scale + 0.2, "alpha": torch.rand(3, generator=g) + 0.5,
          "alpha1": torch.rand(1, generator=g), "alpha2": torch.rand(1, generator=g)}
    for k in R.KS:
        sd[f"body.{k}.0.body.0.weight_v"] = torch.randn(f, 1, k, k, generator=g) / k
        sd[f"body.{k}.0.body.0.weight_g"] = torch.rand(f, 1, 1, 1, generator=g) + 0.5
        sd[f"body.{k}.0.body.0.bias"] = 0.2 * torch.randn(f, generator=g)
        sd[f"body.{k}.0.body.2.weight_v"] = torch.randn(f, f, 1, 1, generator=g) / f ** 0.5
        sd[f"body.{k}.0.body.2.weight_g"] = torch.rand(f, 1, 1, 1, generator=g) + 0.5
        sd[f"body.{k}.0.body.2.bias"] = 0.2 * torch.randn(f, generator=g)
    return sd


def _reference_from_state_dict(x, sd, mask_w, gate):
    """nas_ref.nas_block_ref fed from float64 copies of the oracle's parameters: weight-norm, the straight-through masks, the
    softmax and the straight-through gate are applied here in float64, so autograd reaches the same leaves as the oracle's"""
    f = x.shape[1]
    wn = lambda k, i: O.weight_norm(sd[f"body.{k}.0.body.{i}.weight_v"], sd[f"body.{k}.0.body.{i}.weight_g"])
    wdw = [wn(k, 0) for k in R.KS]
    bdw = torch.stack([sd[f"body.{k}.0.body.0.bias"] for k in R.KS])
    wpw = torch.stack([wn(k, 2) for k in R.KS])
    bpw = torch.stack([sd[f"body.{k}.0.body.2.bias"] for k in R.KS])
    sw = sd["split.weight"]
    ms = (sw - (sw.detach() - O.rounding(sw.detach(), 0))).reshape(f)
    if mask_w is None:
        mg = torch.ones(f, dtype=torch.float64)
    else:
        mg = (mask_w - (mask_w.detach() - O.rounding(mask_w.detach(), 8))).reshape(f)
    if gate is None:
        beta = torch.tensor([0.0, 1.0], dtype=torch.float64)
    else:
        a1, a2 = sd["alpha1"], sd["alpha2"]
        keep = bool(a1 < a2)
        beta = torch.cat([(0.0 if keep else 1.0) + (a1 - a1.detach()), (1.0 if keep else 0.0) + (a2 - a2.detach())])
    p = torch.softmax(sd["alpha"], 0)
    return R.nas_block_ref(x.permute(0, 2, 3, 1), wdw[0], wdw[1], wdw[2], bdw, wpw, bpw, mg, ms, p, beta).permute(0, 3, 1, 2)


def _compare(f, seed, with_model_glue, gate_open):
    g = torch.Generator().manual_seed(seed)
    sd = _state_dict(f, g)
    if with_model_glue:
        sd["alpha1"], sd["alpha2"] = (torch.tensor([0.2]), torch.tensor([0.6])) if gate_open else (torch.tensor([0.6]), torch.tensor([0.2]))
    mask_w = torch.rand(f, 1, 1, 1, generator=g) * 0.7 + 0.25
    x = torch.randn(2, f, 9, 11, generator=g)
    dy = torch.randn(2, f, 9, 11, generator=g)
    lo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo, mo = x.clone().requires_grad_(True), mask_w.clone().requires_grad_(True)
    hi = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xh, mh = x.double().requires_grad_(True), mask_w.double().requires_grad_(True)
    if with_model_glue:
        yo = O.nas_block_forward(xo, {"b." + k: v for k, v in lo.items()}, "b", mo, training=True)
        yh = _reference_from_state_dict(xh, hi, mh, True)
    else:
        yo = O.split_block_forward_body(xo, lo)
        yh = _reference_from_state_dict(xh, hi, None, None)
    yo.backward(dy)
    yh.backward(dy.double())
    pairs = [("y", yo.detach(), yh.detach()), ("dx", xo.grad, xh.grad)]
    if with_model_glue:
        pairs.append(("d mask.weight", mo.grad, mh.grad))
    for k in sd:
        if lo[k].grad is None:
            assert hi[k].grad is None or float(hi[k].grad.abs().max()) == 0.0, k
            continue
        pairs.append(("d " + k, lo[k].grad, hi[k].grad))
    assert len(pairs) >= (2 + 1 + 20 + 2 if with_model_glue else 2 + 20)
    for name, a, b in pairs:
        e = R.rel_max(a, b)
        assert e <= 1e-5, (name, e)


@pytest.mark.parametrize("f", [24, 32])
def test_reference_matches_oracle_split_block(f):
    _compare(f, 400 + f, False, True)


@pytest.mark.parametrize("gate_open", [True, False])
@pytest.mark.parametrize("f", [24, 32])
def test_reference_matches_oracle_nas_block(f, gate_open):
    _compare(f, 500 + f, True, gate_open)


def test_intermediates_are_complete_and_consistent():
    """the option that returns every tensor the reference forms: forward names, their gradients, and gyin as the sum of its terms"""
    case = R.exact_case(24, 1, 6, 6, "random", R.P_MIX)
    y, grads, d = R.block_grads(case, want_inter=True)
    for name in ["xg", "x1", "s", "y"] + [f"{t}{k}" for t in "zvut" for k in range(3)]:
        assert name in d and "d " + name in d, name
    f = 24
    cv = lambda t: t.double().view(1, f, 1, 1)
    gyin = cv(case["mg"]) * case["gy"].double().permute(0, 3, 1, 2) + cv(case["mg"] * case["ms"]) * d["d x1"]
    assert torch.equal(gyin.permute(0, 2, 3, 1), grads[0])
    assert torch.equal(d["y"].permute(0, 2, 3, 1), y)


@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=lambda g: "%dx%dx%d" % g)
def test_exact_conditions_geometries(f, geom):
    for p in ((1.0, 0.0, 0.0), R.P_MIX):
        R.exact_case(f, *geom, "all", p)                  # raises if a condition fails
        R.exact_case(f, *geom, "random", p)


@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("geom", R.CORNER_GEOMETRIES, ids=lambda g: "%dx%dx%d" % g)
def test_exact_conditions_corners(f, geom):
    for masks, p, beta in R.CORNERS:
        R.exact_case(f, *geom, masks, p, beta)


@pytest.mark.parametrize("f", [24, 32])
def test_exact_conditions_tile_loop_cases(f):
    R.exact_case(f, *R.TILE_LOOP_GEOMETRY, "random", R.P_MIX)
    assert R.n_tiles(*R.TILE_LOOP_GEOMETRY) == 12
    m = R.MANY_TILES
    R.exact_case(f, m["n"], m["h"], m["w"], m["masks"], m["p"], (0.0, 1.0), 0, m["gy_density"])
    assert R.n_tiles(m["n"], m["h"], m["w"]) == 260
    assert R.n_tiles(*R.BODY_FUSED) == 8 and R.n_tiles(*R.BODY_SEPARATE) == 9
    R.exact_body_case(f, *R.BODY_FUSED)
    R.exact_body_case(f, *R.BODY_SEPARATE)


def test_check_exact_rejects_a_broken_case():
    """the checker is not vacuous: a zero ReLU argument, a value off the bf16 grid and an overlong sum are each refused"""
    good = R.exact_case(24, 1, 6, 6, "all", R.P_MIX)
    bad = {k: v for k, v in good.items() if k != "ref"}
    bad["bpw"] = torch.zeros_like(good["bpw"])             # pointwise pre-activations now land on 0
    with pytest.raises(ValueError, match="zero ReLU"):
        R.check_exact(bad)
    bad = {k: v for k, v in good.items() if k != "ref"}
    bad["yin"] = good["yin"] * 1.00390625                  # 1 + 2^-8: nine significant bits
    with pytest.raises(ValueError, match="bf16"):
        R.check_exact(bad)
    bad = {k: v for k, v in good.items() if k != "ref"}
    bad["gy"] = good["gy"] + 2.0 ** -9                     # gy itself is fine in bf16; its sums with integers are not
    with pytest.raises(ValueError, match="bf16"):
        R.check_exact(bad)
    K.need_sum("a sum", torch.tensor([2.0 ** 22 - 0.25]), 0.25)
    with pytest.raises(ValueError, match="2\\^24"):
        K.need_sum("a sum", torch.tensor([2.0 ** 22]), 0.25)
    bad = {k: v for k, v in good.items() if k != "ref"}
    bad["wdw7"] = good["wdw7"].clone()
    bad["wdw7"][:, :, :, 6] = 0.0                          # the last window column of the 7 x 7 unobserved
    with pytest.raises(ValueError, match="tap"):
        R.check_exact(bad)


def test_emulation_route_is_the_same_function():
    """the rounding route of the reference (manual backward of the branch tail) with a rounding that does nothing gives what
    plain autograd gives"""
    case = R.rounded_case(24, 1, 6, 6, "bf16")
    y0, g0 = R.block_grads(case)
    y1, g1 = R.block_grads(case, torch.float64, lambda t: t)
    for name, a, b in zip(("y",) + R.GRAD_NAMES, [y1] + g1, [y0] + g0):
        assert R.rel_max(a, b) <= 1e-13, name


def test_emulation_yardsticks_are_sane():
    """the CPU emulations the rounded bounds come from: fp32 within 1e-5 of float64 in every tensor; bf16 y and gyin at a few
    bf16 ulps (2^-9 = 2e-3 relative each), nothing beyond 5e-2"""
    _, _, yard = R.rounded_reference(24, 1, 6, 6, "fp32")
    assert len(yard) == 12 and all(e <= 1e-5 for e in yard), yard
    _, _, yard = R.rounded_reference(24, 1, 6, 6, "bf16")
    assert len(yard) == 12 and all(e <= 5e-2 for e in yard), yard
    assert 1e-3 <= yard[0] <= 1e-2 and 1e-3 <= yard[1] <= 1e-2, yard
