"""tests/conv_ref.py on the host: spynet_ref against fixture G15 and rm_block_ref / rm_tail_ref against fixture G18 (both made by
the reference project's own modules, in fp32), conv7_ref against a shift-and-add loop, the mask packing against hand-written
bits, and the exactness conditions of every exact case the GPU tests use (the same case lists, imported), checked on the float64
reference alone."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R, parity_kit as K

_gid = lambda g: "%dx%dx%d" % g

# How far the float64 references lie from the fp32 fixtures, max |fixture - ref| / max |ref|, measured on the CPU; the bounds are
# four times that (the margin covers fp32 reassociation in another torch build).  DESIGN.md keeps both numbers.
G15_MEASURED, G15_BOUND = 3.11e-7, 1.25e-6
G18_MEASURED, G18_BOUND = 1.07e-6, 4.3e-6


# ---- SPyNet ------------------------------------------------------------------------------------------------------------------
def test_spynet_reference_matches_g15_fixture(golden_dir):
    """same seeded default init as the fixture's reference SpyNet (checksums asserted, as the GPU test of G15 does); both pair
    sets, the second of which (40 x 56) takes the resize branch"""
    from mobilesuperresolution_amd.models import SpyNet
    z = np.load(os.path.join(golden_dir, "g15_spynet.npz"))
    d = {k: torch.from_numpy(z[k]) for k in z.files}
    torch.manual_seed(150)
    sd = SpyNet().state_dict()
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(d["w_sum"])) <= 1e-6 * abs(float(d["w_sum"])) + 1e-9
    assert abs(sum(v.double().abs().sum().item() for v in sd.values()) - float(d["w_abs"])) <= 1e-6 * float(d["w_abs"])
    assert set(R.spynet_param_names()) | {"mean", "std"} == set(sd)
    shapes = set()
    for k in range(2):
        flow = R.spynet_ref(d[f"ref_{k}"], d[f"supp_{k}"], sd)
        assert flow.shape == d[f"flow_{k}"].shape and flow.dtype == torch.float64
        err = R.rel_max(d[f"flow_{k}"], flow)
        print(f"conv parity | G15 pair set {k} {tuple(flow.shape)} | fixture (fp32) against spynet_ref (float64): {err:.3e}")
        assert err <= G15_BOUND, (k, err)
        shapes.add(tuple(flow.shape[2:]))
    assert any(h % 32 or w % 32 for h, w in shapes)        # the resize branch is taken


def test_conv7_reference_against_shift_and_add():
    """conv7_ref is F.conv2d; here it is held against 49 shifted copies added up, so the reference does not rest on F.conv2d alone"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(5, 8, 7, 7, generator=g, dtype=torch.float64)
    b = torch.randn(5, generator=g, dtype=torch.float64)
    xp = torch.zeros(2, 8, 9 + 6, 11 + 6, dtype=torch.float64)
    xp[:, :, 3:12, 3:14] = x
    want = b.view(1, 5, 1, 1).expand(2, 5, 9, 11).clone()
    for ky in range(7):
        for kx in range(7):
            want += torch.einsum("oc,nchw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + 9, kx:kx + 11])
    assert R.rel_max(R.conv7_ref(x, w, b, False), want) <= 1e-13
    assert R.rel_max(R.conv7_ref(x, w, b, True), want.clamp_min(0)) <= 1e-13


def test_basic_module_rounding_route_is_the_same_function():
    case = R.chain_rounded_case(1, 9, 11)
    p64 = [p.double() for p in case["params"]]
    a = R.basic_module_ref(case["x"].double(), p64)
    b = R.basic_module_ref(case["x"].double(), p64, lambda t: t)
    assert torch.equal(a, b)
    inter = []
    c = R.basic_module_ref(case["x"].double(), p64, R.bf16_round, inter)
    assert len(inter) == 4 and all(K.is_bf16(t) for t in inter) and 1e-4 < R.rel_max(c, a) < 5e-2


# ---- Result_Model ------------------------------------------------------------------------------------------------------------
def test_mask_packing_against_hand_written_bits():
    pos = torch.zeros(1, 32, 1, 3, dtype=torch.bool)
    pos[0, 0, 0, 0] = pos[0, 5, 0, 0] = True                    # pixel 0: bits 0 and 5
    pos[0, 31, 0, 1] = pos[0, 1, 0, 1] = True                   # pixel 1: bits 31 and 1
    bits = R.pack_mask(pos)
    assert bits.dtype == torch.int64 and bits.tolist() == [[[0b100001, (1 << 31) | 0b10, 0]]]
    # the kernels' words are int32: bit 31 set reads back negative, the tests compare the low 32 bits
    assert int(torch.tensor((1 << 31) | 0b10).to(torch.int32)) < 0
    assert int(torch.tensor((1 << 31) | 0b10).to(torch.int32).long() & 0xFFFFFFFF) == (1 << 31) | 0b10


def test_unshuffle_reference_is_the_inverse_of_pixel_shuffle():
    for r_ in R.RM_TAIL_RS:
        t = torch.arange(2 * 3 * r_ * r_ * 3 * 5, dtype=torch.float64).view(2, 3 * r_ * r_, 3, 5)
        u = R.unshuffle_ref(F.pixel_shuffle(t, r_), r_, R.RM_CP[r_])
        assert u.shape == (2, R.RM_CP[r_], 3, 5) and torch.equal(u[:, :3 * r_ * r_], t) and not bool(u[:, 3 * r_ * r_:].any())
        hr = F.pixel_shuffle(t, r_)
        assert float(u[1, 2 * r_ * r_ + 1 * r_ + (r_ - 1), 2, 4]) == float(hr[1, 2, 2 * r_ + 1, 4 * r_ + r_ - 1])


def _result_model_ref(sd, status, scale, x, hr):
    """Result_Model (models/result_model.py, tools/make_golden_result_model.py) and one backward of its L1 loss in float64, the
    blocks and the tail through rm_block_ref / rm_tail_ref and their own gradients, chained by hand the way the kernel route
    chains them; the head, the skip, the weight norms and the biases of the ends through autograd"""
    lv = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    wn = lambda p: torch._weight_norm(lv[p + ".weight_v"], lv[p + ".weight_g"], 0)
    IN, nb, kl = status[0][0], len(status), status[-1][2]
    xm = x.double() - 0.5
    y0 = F.conv2d(xm, wn("body.0"), lv["body.0.bias"], padding=1)
    acts, ws = [y0.detach()], []
    for i, (_, split, k) in enumerate(status):
        p = f"body.{i + 1}.body.0.body.0"
        ws.append(wn(p))
        acts.append(R.rm_block_ref(acts[-1], ws[-1].detach(), lv[p + ".bias"].detach(), IN - split, IN, k)["y"])
    pt = f"body.{nb + 1}"
    wt = wn(pt)
    base = F.pixel_shuffle(F.conv2d(xm, wn("skip"), lv["skip.bias"], padding=2) + lv[pt + ".bias"].view(1, -1, 1, 1), scale)
    out = R.rm_tail_ref(acts[-1], wt.detach(), base.detach(), scale, kl)["out"]
    loss = (out - hr.double()).abs().mean()
    dout = torch.sign(out - hr.double()) / out.numel()
    t = R.rm_tail_ref(acts[-1], wt.detach(), base.detach(), scale, kl, dout)
    base.backward(dout)
    assert R.rel_max(t["gb"], lv[pt + ".bias"].grad) <= 1e-12
    wt.backward(t["gw"])
    gy = t["dfeat"]
    for i in range(nb - 1, -1, -1):
        _, split, k = status[i]
        p = f"body.{i + 1}.body.0.body.0"
        o = R.rm_block_ref(acts[i], ws[i].detach(), lv[p + ".bias"].detach(), IN - split, IN, k, gy)
        ws[i].backward(o["gw"])
        lv[p + ".bias"].grad = o["gb"]
        gy = o["dx"]
    y0.backward(gy)
    return out, float(loss), {k: v.grad for k, v in lv.items()}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_block_and_tail_references_match_g18_fixture(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "g18_result_model.npz"))
    g = lambda pre: {k[len(f"{tag}/{pre}/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{tag}/{pre}/")}
    params, grads = g("p"), g("g")
    status, scale = z[f"{tag}/status"].tolist(), int(z[f"{tag}/scale"])
    out, loss, got = _result_model_ref(params, status, scale, torch.from_numpy(z[f"{tag}/x"]), torch.from_numpy(z[f"{tag}/hr"]))
    worst = R.rel_max(torch.from_numpy(z[f"{tag}/y"]), out)
    assert abs(loss - float(z[f"{tag}/loss"])) <= 1e-6 * loss
    assert set(got) == set(grads)
    for k, v in grads.items():
        worst = max(worst, R.rel_max(v, got[k]))
    print(f"conv parity | G18 {tag} | fixture (fp32) against the float64 restatement, worst of y and {len(grads)} gradients: {worst:.3e}")
    assert worst <= G18_BOUND, worst


def test_block_reference_window_against_a_plain_restatement():
    """the (F, F) embedding inside rm_block_ref against the window written directly; the gate argument; relu'(0) = 0"""
    case = R.block_rounded_case(24, 20, 12, 5, 1, 7, 9)
    x, w, b, gy = (case[k].double() for k in ("x", "w", "b", "gy"))
    a, IN = 8, 20
    o = R.rm_block_ref(x, w, b, a, IN, 5, gy)
    xs, wl, bl = x[:, a:IN].clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    zs = F.conv2d(xs, wl, bl, padding=2)
    ys = xs + torch.relu(zs)
    ys.backward(gy[:, a:IN])
    assert R.rel_max(o["y"][:, a:IN], ys.detach()) <= 1e-13 and torch.equal(o["y"][:, :a], x[:, :a]) and torch.equal(o["y"][:, IN:], x[:, IN:])
    assert R.rel_max(o["dx"][:, a:IN], xs.grad) <= 1e-13 and torch.equal(o["dx"][:, :a], gy[:, :a])
    assert R.rel_max(o["gw"], wl.grad) <= 1e-13 and R.rel_max(o["gb"], bl.grad) <= 1e-13
    assert torch.equal(o["gw_dense"][a:IN, a:IN], o["gw"]) and not bool(o["gw_dense"][:a].any()) and not bool(o["gw_dense"][IN:].any())
    assert bool(o["gw_dense"][a:IN, :a].any())                  # the pass-through channels reach the dense gradient's columns
    assert torch.equal(o["bits"], R.pack_mask(o["z"] > 0)) and int(o["bits"].max()) < (1 << IN) and int((o["bits"] & ((1 << a) - 1)).max()) == 0
    o2 = R.rm_block_ref(x, w, b, a, IN, 5, gy, o["z"] > 0)
    assert all(R.rel_max(o2[k], o[k]) <= 1e-13 for k in ("y", "dx", "gw", "gb"))
    o3 = R.rm_block_ref(x, w, b, a, IN, 5, gy, torch.zeros_like(o["z"], dtype=torch.bool))
    assert torch.equal(o3["dx"], gy) and not bool(o3["gw"].any())


# ---- the exactness conditions of every case of tests/test_gpu_conv_ref.py (raises if one fails) -------------------------------
@pytest.mark.parametrize("layer", range(5))
def test_exact_conditions_conv7(layer):
    ties = 0
    for geom in R.CONV7_GEOMETRIES:
        ref = R.conv7_exact_case(layer, *geom)["ref"]
        assert ref["quanta"] < 2.0 ** 24
        ties += ref.get("ties", 0)
        if layer < 4:
            assert ref["ties"] >= 1
    assert layer == 4 or ties >= len(R.CONV7_GEOMETRIES)
    if layer == 2:                                             # the figures the exactness argument quotes, 64 -> 32 at 2 x 17 x 65
        case = R.conv7_exact_case(2, 2, 17, 65)
        y64 = case["ref"]["y"]
        y32 = R.conv7_ref(case["x"], case["w"], case["b"], True)
        frac = float((R.bf16_round(y64) != y64).double().mean())
        print(f"conv parity | conv7 64 -> 32 at 2x17x65 | sum |terms| {case['ref']['quanta']:.3g} quanta of 2^24 = {2.0 ** 24:.3g} | "
              f"{100 * frac:.0f} % of the outputs need the bf16 rounding")
        assert torch.equal(y32.double(), y64) and 0.05 < frac < 0.95


@pytest.mark.parametrize("layer", range(5))
def test_tap_identity_sets_cover_every_tap_and_channel(layer):
    cin, cout, relu = R.LAYERS[layer]
    cases = R.conv7_tap_cases(layer, *R.CONV7_TAP_GEOMETRY)
    assert len(cases) == R.conv7_tap_count(layer)
    taps = [t for c in cases for t in c["taps"]]
    assert {(ky, kx) for _, ky, kx in taps} == {(ky, kx) for ky in range(7) for kx in range(7)}
    assert {ci for ci, _, _ in taps} == set(range(cin))
    if cin == 8:                                               # kx = 6 shares its k-step with the zero tap kx = 7
        assert {ci for ci, _, kx in taps if kx == 6} == set(range(8))
        assert {ky for _, ky, kx in taps if kx == 6} == set(range(7))
    case = cases[0]                                            # the output is a shifted copy of one input channel plus the bias
    x, w, b = case["x"].double(), case["w"].double(), case["b"].double()
    xp = F.pad(x, (3, 3, 3, 3))
    n, _, h, wd = x.shape
    for co, (ci, ky, kx) in enumerate(case["taps"]):
        want = w[co, ci, ky, kx] * xp[:, ci, ky:ky + h, kx:kx + wd] + b[co]
        assert torch.equal(case["ref"]["y"][:, co], want.clamp_min(0) if relu else want), (co, ci, ky, kx)


@pytest.mark.parametrize("geom", R.CHAIN_GEOMETRIES, ids=_gid)
def test_exact_conditions_chain(geom):
    case = R.chain_exact_case(*geom)
    assert len(case["ref"]["inter"]) == 4 and all(K.is_bf16(t) for t in case["ref"]["inter"])
    for i in range(5):
        assert torch.unique(case["params"][2 * i].abs()).numel() >= 4          # +-2^k with k all over the place, and 0


@pytest.mark.parametrize("k", R.RM_KS)
def test_exact_conditions_blocks(k):
    for window in R.RM_SWEEP_WINDOWS:
        for geom in R.RM_GEOMETRIES:
            ref = R.block_exact_case(*window, k, *geom)["ref"]
            assert ref["ties"] >= 1 and bool((ref["z"] == 0)[:, window[1] - window[2]:window[1]].any())
    for window in R.RM_WINDOWS:
        for geom in R.RM_WINDOW_GEOMETRIES:
            R.block_exact_case(*window, k, *geom)
    if k in R.RM_LOOP_KS:
        assert R.wgrad_tiles(*R.RM_LOOP_GEOMETRY) == 6 and R.wgrad_tiles(*R.RM_MANY_TILES[0]) == 30
        R.block_exact_case(*R.RM_LOOP_WINDOW, k, *R.RM_LOOP_GEOMETRY)
        R.block_exact_case(*R.RM_LOOP_WINDOW, k, *R.RM_MANY_TILES[0])


@pytest.mark.parametrize("k", R.RM_TAIL_KS)
def test_exact_conditions_tails(k):
    ties = 0
    for f in R.RM_TAIL_FS:
        for r_ in R.RM_TAIL_RS:
            for geom in R.RM_TAIL_GEOMETRIES:
                ref = R.tail_exact_case(f, r_, k, *geom)["ref"]
                ties += ref["ties"]
                assert ref["dconv"].shape[1] == R.RM_CP[r_]
    assert ties >= 1                                           # the tail family's bf16 store (dfeat) meets a tie


def test_check_exact_rejects_a_broken_case():
    """the checker is not vacuous: a value off the bf16 grid, a zero weight, equal biases, an overlong sum, a block whose z
    never vanishes and a tap case whose weight sits elsewhere are each refused"""
    good = R.conv7_exact_case(1, 1, 8, 32)
    base = lambda c: {k: v for k, v in c.items() if k != "ref"}
    R.check_exact(base(good))
    bad = base(good)
    bad["x"] = good["x"] * 1.00390625                           # 1 + 2^-8: nine significant bits
    with pytest.raises(ValueError, match="bf16"):
        R.check_exact(bad)
    bad = base(good)
    bad["w"] = good["w"].clone()
    bad["w"][3, 2, 6, 6] = 0.0
    with pytest.raises(ValueError, match="zero"):
        R.check_exact(bad)
    bad = base(good)
    bad["b"] = good["b"].clone()
    bad["b"][1] = bad["b"][0]
    with pytest.raises(ValueError, match="differ per channel"):
        R.check_exact(bad)
    bad = base(good)
    bad["b"] = good["b"].clone()
    bad["b"][0] = 2.0 ** 22 + 2.0 ** -3
    with pytest.raises(ValueError, match="2\\^24"):
        R.check_exact(bad)
    blk = R.block_exact_case(24, 20, 12, 3, 2, 9, 33)
    bad = base(blk)
    bad["b"] = blk["b"] + 2.0 ** -9
    with pytest.raises(ValueError, match="exactly zero"):
        R.check_exact(bad)
    tap = R.conv7_tap_cases(0, *R.CONV7_TAP_GEOMETRY)[0]
    bad = base(tap)
    bad["w"] = tap["w"].flip(3)
    with pytest.raises(ValueError, match="tap"):
        R.check_exact(bad)
    with pytest.raises(ValueError, match="2\\^24"):
        K.need_sum("a sum", torch.tensor([2.0 ** 22]), torch.tensor([0.25]))


def test_emulation_yardsticks_are_sane():
    """the CPU emulations the rounded bounds come from: nonzero and finite; fp32 within 1e-5 of float64; bf16 stores at a few bf16
    ulps"""
    for mode, lo, hi in (("fp32", 0.0, 1e-5), ("bf16", 1e-4, 3e-2)):
        for kind, key in (("block", (24, 20, 12, 3) + R.RM_ROUNDED_GEOMETRY), ("tail", (24, 3, 5) + R.RM_ROUNDED_GEOMETRY)):
            _, _, yard = R.rounded_reference(kind, mode, *key)
            assert all(lo < e <= hi and e == e for e in yard.values()), (mode, kind, yard)
    _, _, yard = R.rounded_reference("conv7", "bf16", 1, 1, 8, 32)
    assert 1e-4 < yard["y"] <= 1e-2
