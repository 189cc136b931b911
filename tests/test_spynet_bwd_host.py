"""Host side of SpyNet's training route (no GPU): the backward-data gather table against a numpy statement of "rotate, swap, pad";
its fragment order through the lane-level MFMA emulation against a direct convolution; the weight-gradient unpack tables; the
float64 reference of tests/spynet_bwd_ref.py against torch autograd; the route rule of SpyNet.train_route_reason; the seed of the
whole-network GPU test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from tests import mfma_emu as E
from tests import spynet_bwd_ref as B
from tests.parity_kit import bf16_round, rel_max

LAYER_IDS = ["%dto%d" % l[:2] for l in B.LAYERS]


def _rotated(w, cin_t):
    """rotate, swap, pad: wt (cin, cin_t, 7, 7) with wt[ci][co][ky][kx] = w[co][ci][6 - ky][6 - kx], zero for co >= cout"""
    cout, cin = w.shape[:2]
    wt = np.zeros((cin, cin_t, 7, 7), dtype=w.dtype)
    wt[:, :cout] = w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)
    return wt


@pytest.mark.parametrize("layer", range(5), ids=LAYER_IDS)
def test_bwd_tables_are_rotate_swap_pad(layer):
    """conv7_bwd_tables(cin, cout) gathers what conv7_tables(cin_t, cout_t) gathers from the rotated, role-swapped, padded weight"""
    from mobilesuperresolution_amd import packing as P
    cin, cout, _ = B.LAYERS[layer]
    tab = P.conv7_bwd_tables(cin, cout)
    assert (tab["cin"], tab["cout"]) == (max(cout, 8), cin)
    fwd = P.conv7_tables(tab["cin"], tab["cout"])
    assert (tab["mt"], tab["kpr"]) == (fwd["mt"], fwd["kpr"]) and tab["idx"].shape == fwd["idx"].shape
    w = np.arange(1, cout * cin * 49 + 1, dtype=np.float64).reshape(cout, cin, 7, 7)      # every weight its own nonzero value
    got = np.concatenate([w.reshape(-1), [0.0]])[tab["idx"]]
    want = np.concatenate([_rotated(w, tab["cin"]).reshape(-1), [0.0]])[fwd["idx"]]
    assert np.array_equal(got, want)
    assert set(np.unique(got)) - {0.0} == set(np.unique(w))                              # every weight is used


@pytest.mark.parametrize("layer", range(5), ids=LAYER_IDS)
def test_bwd_fragment_order_against_direct_conv(layer):
    """the backward-data k-loop of conv7_fwd_kernel, lane by lane, on the packed table: one image row of 32 pixels"""
    from mobilesuperresolution_amd import packing as P
    cin, cout, _ = B.LAYERS[layer]
    tab = P.conv7_bwd_tables(cin, cout)
    ct, mt, kpr = tab["cin"], tab["mt"], tab["kpr"]
    g = torch.Generator().manual_seed(100 + layer)
    w = torch.randint(-3, 4, (cout, cin, 7, 7), generator=g).double()
    dy = torch.randint(-3, 4, (1, cout, 7, 32), generator=g).double()
    packed = np.concatenate([w.reshape(-1).numpy(), [0.0]])[tab["idx"]]
    xs = np.zeros((7 + 6, 32 + 6 + 2, ct))                                # halo tile NHWC, zero outside, +2 pixels as the kernel
    xs[3:10, 3:35, :cout] = dy[0].permute(1, 2, 0).numpy()
    row = 3                                                               # the output row this wave computes
    acc = [np.zeros((64, 16)) for _ in range(mt)]
    for ky in range(7):
        for s in range(kpr):
            b = np.zeros((64, 8))
            for lane in range(64):
                r, hh = lane & 31, lane >> 5
                off = (2 * s + hh) * 8 if ct == 8 else (s // (ct // 16)) * ct + (s % (ct // 16)) * 16 + hh * 8
                flat = xs[row + ky].reshape(-1)
                b[lane] = flat[r * ct + off:r * ct + off + 8]
            for m in range(mt):
                acc[m] = E.mma16(E.wfrag(packed, (ky * kpr + s) * mt + m), b, acc[m])
    want = B.bwd_data_ref(dy, w)[0, :, row]                               # (cin, 32)
    got = np.zeros((cin, 32))
    for m in range(mt):
        for i in range(16):
            for lane in range(64):
                ch = m * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
                if ch < cin:
                    got[ch, lane & 31] = acc[m][lane, i]
    assert np.array_equal(got, want.numpy())


@pytest.mark.parametrize("layer", range(5), ids=LAYER_IDS)
def test_wgrad_tables_hit_every_real_element_once(layer):
    from mobilesuperresolution_amd import packing as P
    cin, cout, _ = B.LAYERS[layer]
    tab = P.conv7_wgrad_tables(cin, cout)
    n = cout * cin * 49 + cout
    assert tab["sidx"].shape == tab["dst"].shape == (n,)
    assert np.array_equal(np.sort(tab["dst"]), np.arange(n))                             # every flat element written exactly once
    assert np.unique(tab["sidx"]).size == n and tab["sidx"].min() >= 0 and tab["sidx"].max() < tab["slab"]
    # a slab written as the kernel writes it: element (row, col) of tile (rt, ct, tap) carries its own code, padded ones -1
    nrt, nct = (tab["ca"] + 31) // 32, (tab["cb"] + 31) // 32
    ncol = nct * 49 + 1
    assert tab["ntl"] == nrt * ncol and tab["slab"] == tab["ntl"] * 1024
    slab = np.full(tab["slab"], -1.0)
    for t in range(tab["ntl"]):
        rt, col = divmod(t, ncol)
        for i in range(16):
            for lane in range(64):
                co, c = 32 * rt + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5), lane & 31
                if col == nct * 49:
                    val = cout * cin * 49 + co if co < cout else -1.0                  # the bias tile: every column holds db[co]
                else:
                    ci = 32 * (col // 49) + c
                    val = (co * cin + ci) * 49 + col % 49 if co < cout and ci < cin else -1.0
                slab[(t * 16 + i) * 64 + lane] = val
    flat = np.full(n, np.nan)
    flat[tab["dst"]] = slab[tab["sidx"]]
    assert np.array_equal(flat, np.arange(n, dtype=np.float64))                          # each lands at its own place, no padded one


def test_wgrad_workgroups_are_capped_and_even():
    from mobilesuperresolution_amd import packing as P
    assert P.conv7_wgrad_wgs(1, 1, 1) == 1 and P.conv7_wgrad_wgs(2, 33, 40, 5) == 5 and P.conv7_wgrad_wgs(2, 33, 40, 1) == 1
    for n, h, w in ((64, 64, 64), (64, 2, 2), (3, 17, 65), (128, 180, 320)):
        wgs = P.conv7_wgrad_wgs(n, h, w)
        total = n * ((h + 15) // 16) * ((w + 15) // 16)
        assert 1 <= wgs <= min(total, P.CONV7_WGRAD_WGS) and -(-total // wgs) * wgs < total + wgs


def test_reference_against_autograd():
    """the float64 chain reference with no rounding is autograd of the chain (<= 1e-12 relative); one layer likewise"""
    case = B.chain_case(*B.CHAIN_GEOMETRY)
    x = case["x"].double().requires_grad_(True)
    params = [p.double().requires_grad_(True) for p in case["params"]]
    xs, a = [], x
    for l in range(5):
        xs.append(a.detach())
        a = F_.conv2d(a, params[2 * l], params[2 * l + 1], padding=3)
        a = torch.relu(a) if l < 4 else a
    a.backward(case["dflow"].double())
    dinput, grads = B.chain_bwd_ref(case["dflow"], case["params"], xs, rnd=None)
    assert rel_max(dinput, x.grad) <= 1e-12
    for got, p in zip(grads, params):
        assert rel_max(got, p.grad) <= 1e-12
    one = B.rounded_case(2, 2, 9, 33)
    xl, wl = one["x"].double().requires_grad_(True), one["w"].double().requires_grad_(True)
    bl = torch.zeros(wl.shape[0], dtype=torch.float64, requires_grad=True)
    F_.conv2d(xl, wl, bl, padding=3).backward(one["dy"].double())
    assert rel_max(B.bwd_data_ref(one["dy"].double(), wl.detach()), xl.grad) <= 1e-12
    dw, db = B.wgrad_ref(one["dy"].double(), xl.detach())
    assert rel_max(dw, wl.grad) <= 1e-12 and rel_max(db, bl.grad) <= 1e-12


def test_reference_applies_the_rounding_points():
    """chain_bwd_ref with bf16 rounding: every gradient handed down is its own bf16 rounding and carries the saved mask"""
    case = B.chain_case(1, 9, 33)
    inter = []
    B.R.basic_module_ref(case["x"].double(), [p.double() for p in case["params"]], bf16_round, inter)
    xs = [bf16_round(case["x"].double())] + inter
    seen = []
    B.chain_bwd_ref(case["dflow"], case["params"], xs, rnd=lambda t: seen.append(t) or bf16_round(t))
    assert len(seen) == 1 + 5 + 4                          # the flow gradient, five weights, dx_4 .. dx_1
    lay = B.layer_ref(3, bf16_round(case["dflow"].double().repeat(1, 8, 1, 1)), case["params"][6], xs[3], 4)
    assert bool((lay["dx"][xs[3] <= 0] == 0).all()) and bool((lay["tol_dx"] >= 0).all())
    v = torch.tensor([0.0, 1.0, 1.5, 1.9999, 2.0, 0.75, 3e-5], dtype=torch.float64)
    assert torch.equal(B.half_ulp16(v), torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -24], dtype=torch.float64))
    worst = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=torch.float64)               # just under a tie: rounds down by almost half an ulp
    assert float((bf16_round(worst) - worst).abs()) <= float(B.half_ulp16(worst)) < 1.01 * float((bf16_round(worst) - worst).abs())
    for tap in B.tap_cases(4, 1, 4, 5)[-1]["taps"]:
        assert tap[1:] == (3, 0)


def test_route_rule_and_default():
    """every reason string of SpyNet.train_route_reason; the class default is untouched"""
    from mobilesuperresolution_amd.models.spynet_arch import SpyNet
    assert SpyNet.hot_training is False
    net = SpyNet()
    assert "hot_training" not in net.__dict__
    x = torch.rand(1, 3, 64, 64)
    assert net.train_route_reason(x, x) == "hot_training is not set"
    net.hot_training = True
    with torch.no_grad():
        assert net.train_route_reason(x, x) == "grad mode is off"
    for p in net.parameters():
        p.requires_grad_(False)
    assert net.train_route_reason(x, x) == "nothing requires grad"
    assert net.train_route_reason(x.clone().requires_grad_(True), x) == "CPU tensors"
    next(net.parameters()).requires_grad_(True)
    assert net.train_route_reason(x, x) == "CPU tensors"
    assert "hot_training" not in SpyNet().__dict__ and SpyNet.hot_training is False


def test_spynet_seed_keeps_the_flipped_masks_under_the_cap():
    """the whole-network case of tests/test_gpu_spynet_train.py: the reference's own rounded-vs-unrounded run flips at most 1 % of
    any ReLU mask, and its rounding noise is finite and non-zero for all 62 tensors"""
    _, noise, flipped = B.spynet_noise()
    for k, v in sorted(noise.items()):
        print(f"spynet train | noise of the rounded restatement | {k} | {v:.3e}")
    print(f"spynet train | largest flipped fraction of a ReLU mask | {flipped:.4f}")
    assert len(noise) == 62 and all(0 < v < 1 for v in noise.values())
    assert flipped <= B.MASK_CAP
