"""tests/ends_ref.py on the host: the float64 reference of the WDSR head and tail against oracle.wdsr_oracle's head / tail / skip /
shuffle restatement, against the fixtures G1 (made by the reference project's own module, in fp32) and G4, against the sum of
shifted copies and against torch's own losses -- and the exactness conditions of every exact case the GPU tests use (the same
case lists, imported), checked on the float64 reference alone."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from oracle import wdsr_oracle as O
from tests import ends_ref as R


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _wn_grads(v, g, dw):
    """(d v, d g) of w = g v / ||v|| for a gradient d w of the effective weight"""
    lv, lg = v.double().clone().requires_grad_(True), g.double().clone().requires_grad_(True)
    O.weight_norm(lv, lg).backward(dw)
    return lv.grad, lg.grad


# measured max |fixture - ref| / max |ref| of the G1 comparison below (the fixture is fp32 arithmetic): y 5.6e-7, dx 3.7e-7, the
# gradients of the head / tail / skip parameters at most 3.3e-6; the bound is 4 x the measured value
_G1_MEASURED = {"y": 5.6e-7, "dx": 3.7e-7, "grads": 3.3e-6}


def test_reference_matches_g1_fixture(golden_dir):
    """G1 through head_ref -> the oracle's blocks (float64) -> tail_ref, and backward through loss_ref, tail_grads_ref, the
    blocks' autograd and head_wgrad_ref: output, dx and the gradient of every head / tail / skip parameter"""
    d = _load(golden_dir, "g1_basic_model_c1.npz")
    sd = {k[2:]: v.double() for k, v in d.items() if k.startswith("p/")}
    w = lambda p: O.weight_norm(sd[p + ".weight_v"], sd[p + ".weight_g"])
    x, hr, mean = d["x"].double(), d["hr"].double(), 0.5
    xl = x.clone().requires_grad_(True)
    y0 = R.head_ref(xl, w("head"), sd["head.bias"], mean)
    y0l = y0.detach().clone().requires_grad_(True)
    a = y0l.permute(0, 3, 1, 2)
    for i in range(4):
        a = O.block_forward(a, sd, f"body.{i}.body")
    feat = a.permute(0, 2, 3, 1)
    btot = sd["tail.bias"] + sd["skip.0.bias"] + mean
    y = R.tail_ref(feat.detach(), x, w("tail"), w("skip.0"), btot, mean, 4)
    worst = {"y": R.rel_max(d["y"], y)}
    dout, lsum = R.loss_ref(y, hr, 1, 1.0 / y.numel())
    assert abs(float(lsum) / y.numel() - float(d["loss"])) <= 1e-6 * float(d["loss"])
    g = R.tail_grads_ref(feat.detach(), x, w("tail"), w("skip.0"), btot, mean, 4, dout)
    feat.backward(g["dfeat"])
    dwh, dbh = R.head_wgrad_ref(y0l.grad, x, mean)
    # dx: the head's and the skip's share, through autograd of the two references
    y0.backward(y0l.grad)
    xs = x.clone().requires_grad_(True)
    R.tail_ref(feat.detach(), xs, w("tail"), w("skip.0"), btot, mean, 4).backward(dout)
    worst["dx"] = R.rel_max(d["dx"], xl.grad + xs.grad)
    grads = {"head.bias": dbh, "tail.bias": g["dbtot"], "skip.0.bias": g["dbtot"]}
    for p, dw in (("head", dwh), ("tail", g["dwt"]), ("skip.0", g["dws"])):
        grads[p + ".weight_v"], grads[p + ".weight_g"] = _wn_grads(sd[p + ".weight_v"], sd[p + ".weight_g"], dw)
    worst["grads"] = max(R.rel_max(d["g/" + k], v) for k, v in grads.items())
    print("G1 distances", worst)
    for k, v in worst.items():
        assert v <= 4 * _G1_MEASURED[k], (k, v)


@pytest.mark.parametrize("f,r", [(24, 4), (32, 4), (24, 3), (32, 2)])
def test_reference_matches_oracle_without_blocks(f, r):
    """oracle.basic_model_forward on a state dict with no blocks is head -> tail + skip -> shuffle -> + mean: output and every
    gradient, float64 on both sides"""
    g = torch.Generator().manual_seed(11 * f + r)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    co, mean = 3 * r * r, 0.5
    sd = {}
    for p, shape in (("head", (f, 3, 3, 3)), ("tail", (co, f, 3, 3)), ("skip.0", (co, 3, 5, 5))):
        sd[p + ".weight_v"], sd[p + ".weight_g"], sd[p + ".bias"] = rn(*shape), rn(shape[0], 1, 1, 1), rn(shape[0])
    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    x, dout = rn(2, 3, 7, 9), rn(2, 3, 7 * r, 9 * r)
    want = O.basic_model_forward(x, sd, r, mean)
    want.backward(dout)
    w = lambda p: O.weight_norm(sd[p + ".weight_v"], sd[p + ".weight_g"]).detach()
    y0 = R.head_ref(x, w("head"), sd["head.bias"].detach(), mean)
    btot = (sd["tail.bias"] + sd["skip.0.bias"] + mean).detach()
    assert R.rel_max(R.tail_ref(y0, x, w("tail"), w("skip.0"), btot, mean, r), want.detach()) <= 1e-12
    gr = R.tail_grads_ref(y0, x, w("tail"), w("skip.0"), btot, mean, r, dout)
    dwh, dbh = R.head_wgrad_ref(gr["dfeat"], x, mean)
    assert R.rel_max(dbh, sd["head.bias"].grad) <= 1e-12
    assert R.rel_max(gr["dbtot"], sd["tail.bias"].grad) <= 1e-12 and R.rel_max(gr["dbtot"], sd["skip.0.bias"].grad) <= 1e-12
    for p, dw in (("head", dwh), ("tail", gr["dwt"]), ("skip.0", gr["dws"])):
        dv, dg = _wn_grads(sd[p + ".weight_v"].detach(), sd[p + ".weight_g"].detach(), dw)
        assert R.rel_max(dv, sd[p + ".weight_v"].grad) <= 1e-11 and R.rel_max(dg, sd[p + ".weight_g"].grad) <= 1e-11, p


def test_shuffle_matches_g4_fixture_and_oracle(golden_dir):
    """tail_ref with an identity centre tap and nothing else is PixelShuffle alone: bit for bit the reference project's own
    nn.PixelShuffle (G4) and the oracle's index permutation; unshuffle is its inverse"""
    d = _load(golden_dir, "g4_pixel_shuffle.npz")
    for r in (2, 3, 4):
        xin, want = d[f"x_r{r}"].double(), d[f"y_r{r}"].double()
        co = 3 * r * r
        wt = torch.zeros(co, co, 3, 3, dtype=torch.float64)
        wt[torch.arange(co), torch.arange(co), 1, 1] = 1.0
        got = R.tail_ref(xin.permute(0, 2, 3, 1), torch.zeros(2, 3, 5, 7, dtype=torch.float64), wt,
                         torch.zeros(co, 3, 5, 5, dtype=torch.float64), torch.zeros(co, dtype=torch.float64), 0.0, r)
        assert torch.equal(got, want) and torch.equal(got, O.pixel_shuffle(xin, r))
        assert torch.equal(R.unshuffle(want, r), xin)


@pytest.mark.parametrize("r", [2, 3, 4])
def test_tail_reference_is_the_sum_of_shifted_copies(r):
    """9 + 25 taps, each a shifted copy of one input plane times one weight, written with slices"""
    case = R.rounded_tail_case(24, r, 2, 6, 7)
    feat, x, wt, ws, btot = (case[k].double() for k in ("feat", "x", "wt", "ws", "btot"))
    n, h, w, f = feat.shape
    z = btot.view(1, -1, 1, 1).expand(n, -1, h, w).clone()
    for src, wgt, k in ((feat.permute(0, 3, 1, 2), wt, 3), (x - R.MEAN, ws, 5)):
        p = k // 2
        pad = torch.zeros(n, src.shape[1], h + 2 * p, w + 2 * p, dtype=torch.float64)
        pad[:, :, p:p + h, p:p + w] = src
        for ky in range(k):
            for kx in range(k):
                z += torch.einsum("oc,nchw->nohw", wgt[:, :, ky, kx], pad[:, :, ky:ky + h, kx:kx + w])
    want = torch.empty(n, 3, h * r, w * r, dtype=torch.float64)
    for c in range(3):
        for i in range(r):
            for j in range(r):
                want[:, c, i::r, j::r] = z[:, c * r * r + i * r + j]
    assert R.rel_max(R.tail_ref(feat, x, wt, ws, btot, R.MEAN, r), want) <= 1e-13


def test_loss_reference_matches_torch_losses():
    g = torch.Generator().manual_seed(2)
    sr = torch.randn(2, 3, 8, 12, generator=g, dtype=torch.float64)
    hr = torch.randn(2, 3, 8, 12, generator=g, dtype=torch.float64)
    hr[0, 1, 2:4] = sr[0, 1, 2:4]                             # exact zeros of sr - hr
    up = 0.7
    for kind, fn in ((1, F_.l1_loss), (2, O.charbonnier)):
        s = sr.clone().requires_grad_(True)
        loss = fn(s, hr)
        (up * loss).backward()
        grad, lsum = R.loss_ref(sr, hr, kind, up / sr.numel())
        assert R.rel_max(grad, s.grad) <= 1e-13 and abs(float(lsum) / sr.numel() - float(loss.detach())) <= 1e-13
        assert bool((grad[0, 1, 2:4] == 0).all())


def test_vectors_follow_hotpath_layout():
    """head_vec / tail_vec are hotpath.head_src / tail_src's order (read from packing's offsets), and the splits invert them"""
    from mobilesuperresolution_amd import packing as P
    for f, r in ((24, 4), (32, 3), (24, 2)):
        g = P.EndsGeom(f, r)
        co = g.CO
        wt, ws, b = torch.randn(co, f, 3, 3), torch.randn(co, 3, 5, 5), torch.randn(co)
        v = R.tail_vec(wt, ws, b)
        o = g.tail_off
        assert v.numel() == o["size"] and v[o["zero"]] == 0 and v[o["one"]] == 1
        assert torch.equal(v[o["ws"]:o["b"]], ws.reshape(-1)) and torch.equal(v[o["b"]:o["zero"]], b)
        s = R.split_tail_vec(v, f, r)
        assert torch.equal(s["dwt"], wt) and torch.equal(s["dws"], ws) and torch.equal(s["dbtot"], b)
        wh, bh = torch.randn(f, 3, 3, 3), torch.randn(f)
        v = R.head_vec(wh, bh)
        o = g.head_off
        assert v.numel() == o["size"] and torch.equal(v[o["b"]:o["zero"]], bh) and v[o["one"]] == 1
        s = R.split_head_vec(v, f)
        assert torch.equal(s["dwh"], wh) and torch.equal(s["dbh"], bh)


def test_emulation_rounds_where_the_kernels_round():
    """emulate('fp32') is the float32 graph; emulate('bf16') stores y and dfeat in bf16 and reads bf16 operands; both stay near
    the float64 reference"""
    tc, hc = R.rounded_tail_case(24, 4, 1, 13, 25), R.rounded_head_case(24, 1, 13, 25)
    for case in (tc, hc):
        ref = R.run_case(case)
        for mode, lo, hi in (("fp32", 1e-9, 1e-5), ("bf16", 1e-4, 3e-2)):
            emu = R.emulate(case, mode)
            for k in ref:
                assert emu[k].dtype == torch.float32 and lo <= R.rel_max(emu[k], ref[k]) <= hi, (mode, k, R.rel_max(emu[k], ref[k]))
            if mode == "bf16":
                for k in ("y", "dfeat"):
                    if k in emu:
                        assert torch.equal(emu[k], R.bf16_round(emu[k]))
    sr = R.run_case(tc)["out"].float()
    hr = torch.where(tc["hr_same"], sr, sr + tc["hr_noise"])
    for kind in (1, 2):
        ref, yard = R.rounded_reference(tc, "bf16", sr=sr, hr=hr, kind=kind, gscale=0.7 / sr.numel())
        assert float(ref["loss"]) > 0 and 0 < yard["loss"] < 1e-4 and yard["dfeat"] > 1e-4


# ---- the exactness conditions of every case of tests/test_gpu_ends_ref.py (raises if one fails) -----------------------------
_FAMILY = R.exact_family()


@pytest.mark.parametrize("name,thunk", _FAMILY, ids=[n for n, _ in _FAMILY])
def test_exact_conditions(name, thunk):
    case = thunk()
    ref = case["ref"]
    if "hr" in case:
        zeros = ref["zeros"]
        assert zeros >= 3 * case["R"] ** 2 * 120 if case["loss_kind"] == 1 else zeros == 0


def test_exact_family_has_ties_and_tiles():
    """over the family at least one stored y and one stored dfeat lie exactly on a bf16 tie (nearest-even is then observable)"""
    ties = {"head": 0, "tail": 0}
    for name, thunk in _FAMILY:
        if "many" not in name:
            case = thunk()
            ties[case["kind"]] += case["ref"]["ties"]
    assert ties["head"] > 0 and ties["tail"] > 0, ties
    assert R.n_tiles(*R.TILE_LOOP_GEOMETRY) == 12 and R.n_tiles(*R.MANY_TILES) == 260 and R.n_tiles(2, 25, 49) == 18


def test_tap_sets_cover_every_tap_and_channel():
    for f in R.UNITS:
        for r in (2, 3, 4):
            cases = R.tail_tap_cases(f, r, *R.TAP_GEOMETRY)
            seen = set()
            for c in cases:
                assert len(c["taps"]) == 3 * r * r
                assert int((c["wt"] != 0).sum() + (c["ws"] != 0).sum()) == 3 * r * r
                assert bool(((c["wt"] != 0).sum((1, 2, 3)) + (c["ws"] != 0).sum((1, 2, 3)) == 1).all())
                seen |= set(c["taps"])
            assert len(seen) == 9 * f + 75
        seen = set()
        for c in R.head_tap_cases(f, *R.TAP_GEOMETRY):
            assert bool(((c["wh"] != 0).sum((1, 2, 3)) == 1).all())
            seen |= set(c["taps"])
        assert len(seen) == 27


def _spoiled(case, **changes):
    c = {k: v for k, v in case.items() if k != "ref"}
    for k, fn in changes.items():
        t = c[k].clone()
        fn(t)
        c[k] = t
    return c


def test_check_exact_rejects_spoiled_cases():
    case = R.exact_tail_case(24, 4, 1, 13, 25)
    R.check_exact(_spoiled(case))                             # the copy itself passes

    def non_dyadic(t):
        t[5, 2, 1, 2] = 0.3

    def overflow(t):
        t[5, 2, 1, 2] = 2.0 ** -40                            # its own bf16 rounding, but a quantum 2^37 times finer

    def repeated_row(t):
        t[7] = t[6]

    def missing_tap(t):
        t[:, :, 0, 2] = 0.0

    for key in ("wt", "ws"):
        for fn, word in ((non_dyadic, "bf16"), (overflow, "quanta"), (repeated_row, "rows are equal"), (missing_tap, "tap")):
            with pytest.raises(ValueError, match=word):
                R.check_exact(_spoiled(case, **{key: fn}))
    head = R.exact_head_case(24, 1, 13, 25)
    for fn, word in ((non_dyadic, "bf16"), (overflow, "quanta"), (repeated_row, "rows are equal"), (missing_tap, "tap")):
        with pytest.raises(ValueError, match=word):
            R.check_exact(_spoiled(head, wh=fn))
    with pytest.raises(ValueError, match="x - mean"):
        R.check_exact(_spoiled(case, x=lambda t: t.__setitem__((0, 0, 0, 0), 0.3)))
    with pytest.raises(ValueError, match="odd multiples"):
        R.check_exact(_spoiled(case, btot=lambda t: t.__setitem__(0, 0.25)))
    loss = R.exact_tail_case(24, 4, 1, 13, 25, 0, 0.5, 2)
    with pytest.raises(ValueError, match="sr - hr"):         # d = 0 is not a Charbonnier exact case
        R.check_exact(_spoiled(loss, hr=lambda t: t.__setitem__((0, 0, 0, 0), float(loss["ref"]["out"][0, 0, 0, 0]))))
