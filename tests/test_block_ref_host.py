"""tests/block_ref.py on the CPU: the float64 block reference against fixture G2 (forward, intermediates, dx and every gradient
through the weight-norm), against oracle.wdsr_oracle.block_forward and against nine shifted copies; the side-image builders; and
the exactness conditions of every exact case the GPU file runs (check_exact raises on none of them, and rejects bad draws)."""
import os

import numpy as np
import pytest
import torch

from oracle import wdsr_oracle as O
from tests import block_ref as R

# max |fixture - reference| / max |reference| measured here ("Block parity"); the bound is 4 x that
G2_MEASURED = {24: dict(y=4.52e-7, h=1.58e-7, t=2.61e-7, dx=2.82e-7, grads=1.30e-6), 32: dict(y=3.28e-7, h=1.97e-7, t=2.10e-7, dx=2.21e-7, grads=1.17e-6)}


def _g2(golden_dir, f):
    z = np.load(os.path.join(golden_dir, f"g2_block_f{f}.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _effective_leaves(d):
    ps = {k[2:]: v.double().clone().requires_grad_(True) for k, v in d.items() if k.startswith("p/")}
    w = [O.weight_norm(ps[f"body.{i}.weight_v"], ps[f"body.{i}.weight_g"]) for i in (0, 2, 3)]
    p = dict(w1=w[0][:, :, 0, 0], w2=w[1][:, :, 0, 0], w3=w[2], b1=ps["body.0.bias"], b2=ps["body.2.bias"], b3=ps["body.3.bias"])
    return ps, p


@pytest.mark.parametrize("f", R.UNITS)
def test_reference_matches_fixture_g2(golden_dir, f):
    """y, h, t, dx and -- chained through the weight-norm by autograd -- the gradient of every parameter of the fixture"""
    d = _g2(golden_dir, f)
    ps, p = _effective_leaves(d)
    r = R.run_block(d["x"], {k: v.detach() for k, v in p.items()}, d["dy"])
    got = dict(y=R.rel_max(d["y"], r["y"]), h=R.rel_max(d["h"], r["h"]), t=R.rel_max(d["t"], r["t"]), dx=R.rel_max(d["dx"], r["dx"]))
    torch.autograd.backward([p[k] for k in R.NAMES], [r["d" + k].reshape(p[k].shape) for k in R.NAMES])
    got["grads"] = max(R.rel_max(d["g/" + k], v.grad) for k, v in ps.items())
    print(f"\nG2 F={f}: " + ", ".join(f"{k} {v:.2e}" for k, v in got.items()))
    for k, v in got.items():
        assert v <= 4 * G2_MEASURED[f][k], (k, v)


@pytest.mark.parametrize("f", R.UNITS)
def test_reference_matches_oracle(golden_dir, f):
    d = _g2(golden_dir, f)
    sd = {k[2:]: v.double() for k, v in d.items() if k.startswith("p/")}
    _, p = _effective_leaves(d)
    y, h, t, _ = O.block_forward(d["x"].double(), sd, return_intermediates=True)
    hh, tt, yy = R.block_forward(d["x"].double(), {k: v.detach() for k, v in p.items()})
    for a, b in ((y, yy), (h, hh), (t, tt)):
        assert R.rel_max(a, b) <= 1e-14


@pytest.mark.parametrize("f", R.UNITS)
def test_dt_is_nine_shifted_copies(f):
    c = R.exact_case(f, 2, 25, 49)
    for blk, p in (("a", c["pa"]), ("b", c["pb"])):
        dy = c["ref"]["b"]["dx_st"] if blk == "a" else c["dyb"].double()
        assert torch.equal(R.dt_by_shifts(dy, p["w3"].double()), c["ref"][blk]["dt"])
    rc = R.rounded_case(f, 1, 13, 25)
    r = R.run_block(rc["x"], rc["pa"], rc["dyb"])
    assert R.rel_max(R.dt_by_shifts(rc["dyb"].double(), rc["pa"]["w3"].double()), r["dt"]) <= 1e-14


def test_tile_image_layout():
    v = torch.arange(2 * 3 * 13 * 25, dtype=torch.float64).reshape(2, 3, 13, 25) + 1
    img = R.tile_image(v, 8, ones_at=3)
    assert img.shape == (2, 4, 288, 8)
    assert img[1, 3, 0, 0] == v[1, 0, 12, 24] and img[0, 1, 24 + 0, 2] == v[0, 2, 1, 24] and img[0, 2, 5, 1] == v[0, 1, 12, 5]
    assert float(img[0, 3, 1:].abs().sum()) == 0 and float(img[..., 4:].abs().sum()) == 0
    assert float(img[..., 3].sum()) == 2 * 13 * 25
    assert torch.equal(R.untile_image(img, 13, 25, 3), v)
    assert R.n_tiles(3, 13, 25) == 12 and R.n_chunks(3, 13, 25) == 14 and R.n_tiles(65, 13, 25) == 260
    assert R.lp_of(24) == 24 and R.lp_of(32) == 32


def test_block_vec_and_split_are_inverse():
    c = R.exact_case(24, 1, 3, 3)
    v = R.block_vec(c["pa"])
    s = R.split_vec(v, 24)
    assert all(torch.equal(s["d" + k], c["pa"][k]) for k in R.NAMES) and s["const"].tolist() == [0.0, 1.0]


@pytest.mark.parametrize("idx", range(len(R.exact_family())), ids=[n for n, _ in R.exact_family()])
def test_every_exact_case_is_exact(idx):
    """check_exact() raises on none of the shipped cases (the generator calls it; here again, on the cached case)"""
    case = R.exact_family()[idx][1]()
    ref = R.check_exact(case)
    for blk in "ab":
        assert torch.equal(ref[blk]["y_st"], R.bf16_round(ref[blk]["y"])) and torch.equal(ref[blk]["dx_st"], R.bf16_round(ref[blk]["dx"]))


def test_some_stored_values_lie_on_bf16_ties():
    """the final y / dx need their single rounding: over the family, stored values lie exactly half way between two bf16 values"""
    ties = {name: thunk()["ref"]["ties"] for name, thunk in R.exact_family() if "(1, 13, 25)" in name or "(2, 25, 49)" in name}
    assert all(v > 0 for v in ties.values()), ties
    for f in R.UNITS:                                       # the tensors stored BETWEEN the blocks: each in its own family
        for store, geom in R.STORE_CASES:
            of = R.exact_case(f, *geom, 0, 0.5, store)["ref"]["ties_of"]
            assert of["ya" if store == R.STORE_YA else "dxb"] > 0, (f, store, geom, of)
    assert R.count_ties(torch.tensor([257.0, 256.0, 258.0, 1.5, 0.0, 3 * 2.0 ** -9 + 2.0])) == 1


def _mutated(field, fn):
    c = R.exact_case(24, 1, 13, 25)
    bad = dict(c, pa={k: v.clone() for k, v in c["pa"].items()})
    del bad["ref"]
    fn(bad["pa"][field])
    return bad


def _first_weight(w):
    return tuple(w.reshape(w.shape[0], -1)[0].nonzero()[0].tolist())


def test_check_exact_rejects_bad_draws():
    def non_dyadic(w):
        w.view(w.shape[0], -1)[0, _first_weight(w)[0]] = 0.3

    def tiny(w):
        w.view(w.shape[0], -1)[0, _first_weight(w)[0]] = 2.0 ** -40

    def repeated_row(w):
        w[1] = w[0]

    def missing_tap(w):
        w[:, :, 0, 2] = 0

    for field, fn, what in (("w1", non_dyadic, "w1 is not its own bf16"), ("w2", non_dyadic, "w2 is not its own bf16"),
                            ("w3", non_dyadic, "w3 is not its own bf16"), ("w1", repeated_row, "w1: two rows are equal"),
                            ("w2", repeated_row, "w2: two rows are equal"), ("w3", repeated_row, "w3: two rows are equal"),
                            ("w3", missing_tap, "w3: a tap is zero in every channel pair")):
        with pytest.raises(ValueError, match="exact case: block a (" + what + ")"):
            R.check_exact(_mutated(field, fn))
    for field in ("w1", "w2", "w3"):                         # 2^-40 is a bf16 value: what rejects it is the lattice (or the operand it makes)
        with pytest.raises(ValueError, match="quanta >= 2\\^24|is not its own bf16"):
            R.check_exact(_mutated(field, tiny))
    R.check_exact({k: v for k, v in R.exact_case(24, 1, 13, 25).items() if k != "ref"})


@pytest.mark.parametrize("f", R.UNITS)
def test_store_families_see_a_dropped_rounding(f):
    """the reference with the store BETWEEN the blocks left out (block b fed the unrounded ya, block a the unrounded dxb) differs
    from the shipped reference downstream -- in yb for the ya family, in dxa and dt_a for the dxb family: a pair kernel that
    handed the next block an unrounded value cannot pass these cases.  (This stands in for the part of the dxb mutation trial
    that no value-only mutation of a bf16 LDS image can make: a rounding that is not there at all.)"""
    for store, geom in R.STORE_CASES:
        case = R.exact_case(f, *geom, 0, 0.5, store)
        ref, raw = case["ref"], R.run_pair(case, store=None)
        if store == R.STORE_YA:
            n = int((R.bf16_round(raw["b"]["y"]) != ref["b"]["y_st"]).sum())
            assert n >= 100 and not torch.equal(raw["b"]["t"], ref["b"]["t"]), (f, geom, n)
        else:
            n = int((R.bf16_round(raw["a"]["dx"]) != ref["a"]["dx_st"]).sum())
            assert n >= 100 and not torch.equal(raw["a"]["dt"], ref["a"]["dt"]), (f, geom, n)


def test_tap_cases_cover_every_tap():
    for f in R.UNITS:
        cases = R.tap_cases(f, *R.TAP_GEOMETRY)
        seen = set()
        for c in cases:
            assert all(int((c["p"]["w3"][fo] != 0).sum()) == 1 for fo in range(f))
            seen |= set(c["taps"])
        assert len(seen) == 9 * R.DIMS[f][2]


def test_large_batches_reach_their_routes():
    for n, h, w in R.PERSIST_BATCHES:
        assert R.n_tiles(n, h, w) >= 768 and R.n_tiles(n, h, w) % 256 != 0
    for n, h, w in R.STREAM_BATCHES:
        assert w == 48 and h % 4 == 0 and h >= 8 and n >= 256 and n * 10 >= (n + 255) // 256 * 256 * 7
    order = R.batch_order(360, R.DISTINCT_IMAGES)
    assert set(order.tolist()) == set(range(R.DISTINCT_IMAGES))
    assert not any(torch.equal(order[:-p], order[p:]) for p in range(1, 40))
    c = R.exact_case(24, R.DISTINCT_IMAGES, 8, 48)
    x, ref = R.replicate(c, order)
    assert x.shape[0] == 360 and torch.equal(ref["b"]["y_st"][7], c["ref"]["b"]["y_st"][order[7]])


@pytest.mark.parametrize("f", R.UNITS)
def test_emulation_brackets_the_reference(f):
    """fp32 emulation within 1e-5 of the float64 reference, bf16 within 3 %; the reference given the emulation's gates and inputs"""
    for mode, lim in (("fp32", 1e-5), ("bf16", 3e-2)):
        _, emu, ref, yard = R.rounded_reference(f, 1, 13, 25, mode)
        for run in ("a", "b"):
            assert all(0 < v < lim for v in yard[run].values()), (mode, run, yard[run])
        assert 0 < yard["b2"]["y_st"] < lim and 0 < yard["a2"]["dx_st"] < lim and 0 < yard["a2"]["dt"] < lim
