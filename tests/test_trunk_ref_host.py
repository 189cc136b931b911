"""tests/trunk_ref.py on the host: the float64 trunk reference against fixture G7 (made by the reference project's own module, in
fp32) and against oracle.wdsr_oracle's trunk and warp -- output and every autograd gradient -- and the exactness conditions of every
exact case the GPU tests use (the same case lists, imported), checked on the float64 reference alone."""
import os

import numpy as np
import pytest
import torch

from oracle import wdsr_oracle as O
from tests import parity_kit as K, trunk_ref as R

_gid = lambda g: "%dx%dx%d" % g


def test_reference_matches_g7_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "g7_vsr_trunk.npz"))
    d = {k: torch.from_numpy(z[k]) for k in z.files}
    nb = 8
    names = R.param_names(nb)
    assert {"p/" + k for k in names} == {k for k in d if k.startswith("p/")}
    case = dict(nb=nb, params=[d["p/" + k] for k in names], x=d["x"], dy=d["dy"])
    out = R.run_case(case)
    assert R.rel_max(d["y"], out["y"][0]) <= 1e-5
    assert R.rel_max(d["dx"], out["dx"][0]) <= 1e-5
    for k, g in zip(names, out["grads"]):
        assert g.shape == d["g/" + k].shape
        assert R.rel_max(d["g/" + k], g) <= 1e-4, k


@pytest.mark.parametrize("cin,f,nb", [(27, 24, 3), (24, 24, 1), (23, 20, 2), (67, 64, 2)])
def test_reference_matches_oracle_trunk(cin, f, nb):
    case = R.rounded_case(cin, f, nb, 2, 9, 11, "fp32")
    names = R.param_names(nb)
    sd = {k: p.clone().requires_grad_(True) for k, p in zip(names, case["params"])}
    x = case["x"].clone().requires_grad_(True)
    y = O.conv_residual_blocks_forward(x, sd)
    y.backward(case["dy"])
    out = R.run_case(case)
    assert R.rel_max(y.detach(), out["y"][0]) <= 1e-5
    assert R.rel_max(x.grad, out["dx"][0]) <= 1e-5
    for k, g in zip(names, out["grads"]):
        assert R.rel_max(sd[k].grad, g) <= 1e-5, k


def test_step_reference_matches_oracle_warp_and_trunk():
    """the recurrent step in float64 on both sides: off-integer flows, so the warp's cells agree"""
    from tests.warp_ref import off_integer_flow
    g = torch.Generator().manual_seed(5)
    case = R.rounded_case(27, 24, 2, 2, 9, 11, "fp32")
    params = [p.double() for p in case["params"]]
    frame, prev = case["x"][:, :3].double(), torch.randn(2, 24, 9, 11, generator=g).double()
    flow = off_integer_flow((2, 9, 11, 2), 3, gen=g).double()
    want = O.conv_residual_blocks_forward(torch.cat([frame, O.flow_warp(prev, flow)], 1), dict(zip(R.param_names(2), params)))
    assert R.rel_max(R.step_ref(frame, prev, flow.permute(0, 3, 1, 2), params, 2), want) <= 1e-12
    zero = R.step_ref(frame, None, None, params, 2)
    assert torch.equal(zero, R.trunk_ref(torch.cat([frame, torch.zeros_like(prev)], 1), params, 2))


def test_intermediates_are_complete_and_consistent():
    case = R.exact_case(27, 24, 2, 1, 17, 18)
    out = R.run_case(case, want_inter=True)
    d = out["inter"][0]
    for name in ["x", "z0", "a0"] + [f"{t}_{i}" for t in ("z1", "t", "z2") for i in range(2)] + ["a1", "a2"]:
        assert name in d and "d " + name in d, name
    assert torch.equal(d["a2"], out["y"][0]) and torch.equal(d["d x"], out["dx"][0])
    assert torch.equal(d["d a2"], case["dy"].double())
    # the case is not idle: every layer's ReLU is open somewhere and shut somewhere, and gradient reaches every parameter tensor
    for i in range(2):
        frac = float((d[f"t_{i}"] > 0).double().mean())
        assert 0.01 < frac < 0.99, (i, frac)
    assert all(float((g != 0).double().mean()) > 0.02 for g in out["grads"])


# ---- the exactness conditions of every case of tests/test_gpu_trunk_ref.py (raises if one fails) -----------------------------
@pytest.mark.parametrize("trunk", R.TRUNKS, ids=lambda t: "%dto%d" % t)
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_gid)
def test_exact_conditions_geometries(geom, trunk):
    R.exact_case(*trunk, 3, *geom)


@pytest.mark.parametrize("trunk", R.TRUNKS, ids=lambda t: "%dto%d" % t)
def test_exact_conditions_block_counts_and_narrow(trunk):
    for nb in R.BLOCK_COUNTS:
        for geom in R.BLOCK_COUNT_GEOMETRIES:
            R.exact_case(*trunk, nb, *geom)
    for geom in R.NARROW_GEOMETRIES:
        R.exact_case(*R.NARROW, *geom)


@pytest.mark.parametrize("spec", R.STEP_CASES, ids=lambda s: _gid(s[0]))
def test_exact_conditions_recurrent_steps(spec):
    geom, shifts = spec
    case = R.exact_step_case(24, R.STEP_NB, *geom, shifts)
    assert len(case["ref"]["y"]) == 1 + len(shifts)
    w0 = case["params"][0]
    assert bool((w0[:, 3:] != 0).any())                    # the state reaches the first conv
    # every flow is integer-valued and at least one moves the whole state off the image
    n, h, w = geom
    assert all(torch.equal(fl, fl.round()) for fl in case["flows"])
    if len(shifts) > 1:
        assert any(bool((fl[:, 0].abs() >= w).all()) or bool((fl[:, 1].abs() >= h).all()) for fl in case["flows"])


def test_exact_conditions_pairs_and_tile_loop():
    for geom in R.PAIR_CASES:
        ca, cb = R.pair_halves(*geom)
        assert not any(torch.equal(p, q) for p, q in zip(ca["params"], cb["params"]))
    assert R.n_tiles(*R.TILE_LOOP_GEOMETRY) == 12 and R.n_tiles(*R.MANY_TILES) == 80
    R.exact_case(27, 24, 3, *R.TILE_LOOP_GEOMETRY, 0, R.TILE_LOOP_DENSITY)
    n, h, w = R.TILE_LOOP_GEOMETRY
    R.pair_halves(2 * n, h, w, 3, R.TILE_LOOP_DENSITY)
    R.exact_case(27, 24, 3, *R.MANY_TILES, 0, R.MANY_TILES_DENSITY)


@pytest.mark.parametrize("geom", R.SIGN_GEOMETRIES, ids=_gid)
def test_exact_conditions_sign_cases(geom):
    case = R.exact_sign_case(27, 24, *geom)
    z = case["z"]
    assert bool((z > 0).any()) and bool((z < 0).any()) and bool((z == 0).any())
    assert torch.equal(z, z.float().double())


@pytest.mark.parametrize("trunk", R.WIDE_TRUNKS, ids=lambda t: "%dto%dx%d" % t)
def test_exact_conditions_wide(trunk):
    cin, f, nb = trunk
    for geom in R.WIDE_GEOMETRIES:
        R.exact_case(cin, f, nb, *geom, 0, 0.25, True)
    if cin == f + 3:
        for geom in R.WIDE_STEP_GEOMETRIES:
            R.exact_step_case(f, nb, *geom, R.WIDE_STEP_SHIFTS, 0, 0.25, True)
        for seed in (1, 2):
            R.exact_case(cin, f, nb, 1, 17, 18, seed, 0.25, True)


def test_exact_shift_flow_is_a_pure_shift_in_fp32():
    """at every size of the recurrent cases the flows are integers whose fp32 position round trip (IEEE operations, one rounding
    each) returns the integer position, and they equal the requested shift wherever that shift's own round trip is exact"""
    for (n, h, w), shifts in R.STEP_CASES + tuple((g, R.WIDE_STEP_SHIFTS) for g in R.WIDE_STEP_GEOMETRIES):
        for s in shifts:
            flow = R.exact_shift_flow(n, h, w, s)
            assert flow.shape == (n, 2, h, w) and torch.equal(flow, flow.round())
            for k, size in ((0, w), (1, h)):
                if size == 1:
                    continue
                grid = torch.arange(size, dtype=torch.float32).view((1, 1, w) if k == 0 else (1, h, 1))
                pos = grid + flow[:, k]
                v = (2.0 * pos) / torch.full_like(pos, float(size - 1)) - 1.0
                assert torch.equal(((v + 1.0) * 0.5) * float(size - 1), pos)
                assert float((flow[:, k] == float(s[k])).float().mean()) >= 0.5 or abs(s[k]) >= size


def test_check_exact_rejects_a_broken_case():
    """the checker is not vacuous: a value off the bf16 grid, a non-dyadic weight, a non-positive pre-activation, an overlong sum,
    an unobserved tap and equal biases are each refused"""
    good = R.exact_case(27, 24, 2, 1, 17, 18)
    base = lambda: {k: (list(v) if k == "params" else v) for k, v in good.items() if k != "ref"}
    R.check_exact(base())
    bad = base()
    bad["x"] = good["x"] * 1.00390625                      # 1 + 2^-8: nine significant bits
    with pytest.raises(ValueError, match="bf16"):
        R.check_exact(bad)
    bad = base()
    bad["params"][4] = good["params"][4] * 0.3             # not dyadic
    with pytest.raises(ValueError, match="bf16"):
        R.check_exact(bad)
    bad = base()
    bad["dy"] = good["dy"] * 1.0078125                     # gradients off the grid
    with pytest.raises(ValueError, match="bf16"):
        R.check_exact(bad)
    bad = base()
    bad["params"][1] = -good["params"][1]
    with pytest.raises(ValueError, match="strictly positive"):
        R.check_exact(bad)
    bad = base()
    bad["params"][2] = good["params"][2].clone()
    bad["params"][2][:, :, 2, 2] = 0.0
    with pytest.raises(ValueError, match="tap"):
        R.check_exact(bad)
    bad = base()
    bad["params"][3] = good["params"][3].clone()
    bad["params"][3][1] = bad["params"][3][0]
    with pytest.raises(ValueError, match="differ per channel"):
        R.check_exact(bad)
    K.need_sum("a sum", torch.tensor([2.0 ** 22 - 0.25]), torch.tensor([0.25]))
    with pytest.raises(ValueError, match="2\\^24"):
        K.need_sum("a sum", torch.tensor([2.0 ** 22]), torch.tensor([0.25]))


def test_emulation_route_is_the_same_function():
    """the rounding route of the reference with a rounding that does nothing gives what plain autograd gives"""
    case = R.rounded_case(27, 24, 2, 1, 9, 11, "bf16")
    a, b = R.tensors_of(R.run_case(case)), R.tensors_of(R.run_case(case, torch.float64, lambda t: t))
    for name, u, v in zip(R.tensor_names(2), b, a):
        assert R.rel_max(u, v) <= 1e-13, name


@pytest.mark.parametrize("geom", R.ROUNDED_GEOMETRIES, ids=_gid)
def test_emulation_yardsticks_are_sane(geom):
    """the CPU emulations the rounded bounds come from: nonzero and finite in every tensor; fp32 within 1e-5 of float64; bf16 y at
    a few bf16 ulps; the gradients carry ReLU gates that a rounding flips, nothing beyond 0.5"""
    for mode, hi in (("fp32", 1e-5), ("bf16", 0.5)):
        case, ref, yard = R.rounded_reference(27, 24, 3, *geom, mode)
        assert len(yard) == 2 + 2 + 4 * 3
        assert all(0.0 < e <= hi and e == e for e in yard), (mode, yard)
        z = R.run_case(case, want_inter=True)["inter"][0]["z0"]
        assert 0.2 < float((z < 0).double().mean()) < 0.8   # both signs everywhere
    assert 1e-3 <= yard[0] <= 3e-2, yard
