"""The per-frame video network (models/single_image_model.py) without a GPU: fixture G21 (the reference's own Result_Model on the CPU,
tools/make_golden_frame_net.py) against a seeded build, the ATen route and tests/frame_net_ref.py; the exact cases' own conditions; the
route rule; the packed blob's documented layout."""
import os

import numpy as np
import pytest
import torch

from tests import frame_net_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_single_frame.npz")
SEEDS = {"a": 210, "b": 211}
SIZES = ((48, 80), (50, 77))


@pytest.fixture(scope="module")
def g21():
    return np.load(GOLD)


def _model(g21, tag, **kw):
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    torch.manual_seed(SEEDS[tag])
    return Result_Model(*[int(v) for v in g21[f"{tag}/args"]], **kw)


@pytest.mark.parametrize("tag", sorted(SEEDS))
def test_seeded_build_is_the_references(g21, tag):
    m = _model(g21, tag)
    sd = m.state_dict()
    keys = [str(k) for k in g21[f"{tag}/keys"]]
    assert list(sd.keys()) == keys
    for k in keys:
        ref = g21[f"{tag}/p/{k}"]
        assert tuple(sd[k].shape) == ref.shape and np.array_equal(sd[k].numpy(), ref), k
    c, nb = int(g21[f"{tag}/args"][1]), int(g21[f"{tag}/args"][2])
    assert keys[:3] == ["encoder.bias", "encoder.weight_g", "encoder.weight_v"]
    assert f"body.{nb}.weight_v" in keys and "skip.weight_v" in keys and keys[-2:] == ["shuf.0.weight", "shuf.0.bias"]
    assert sd["body.0.body.0.body.2.weight_v"].shape == (c, c, 3, 3) and sd["shuf.0.weight"].shape == (c, 3, 5, 5)
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    other = Result_Model(*[int(v) for v in g21[f"{tag}/args"]])
    other.load_state_dict({k: torch.from_numpy(g21[f"{tag}/p/{k}"]) for k in keys}, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))


def test_exports():
    from mobilesuperresolution_amd import models
    from mobilesuperresolution_amd.models import single_image_model as S
    assert models.SingleFrameVSR is S.Result_Model and models.Result_Model is not S.Result_Model
    assert {"Result_Model", "Block", "Conv_sep"} <= set(S.__all__)


@pytest.mark.parametrize("tag", sorted(SEEDS))
def test_aten_route_on_cpu_reproduces_g21(g21, tag):
    m = _model(g21, tag)
    x = torch.from_numpy(g21[f"{tag}/x"])
    for hh, ww in SIZES:
        m.zero_grad()
        y = m(x, hh, ww)
        assert m.last_route == "aten" and y.shape == (1, 2, 3, hh, ww)
        torch.testing.assert_close(y.detach(), torch.from_numpy(g21[f"{tag}/y{hh}x{ww}"]), rtol=1e-6, atol=1e-6)
        if (hh, ww) == SIZES[0]:
            y.sum().backward()
            for k, p in m.named_parameters():
                got = p.grad if p.grad is not None else torch.zeros_like(p)
                torch.testing.assert_close(got, torch.from_numpy(g21[f"{tag}/g/{k}"]), rtol=1e-6, atol=1e-6, msg=lambda s: f"{k}: {s}")


@pytest.mark.parametrize("tag", sorted(SEEDS))
def test_float64_reference_reproduces_g21(g21, tag):
    nb = int(g21[f"{tag}/args"][2])
    p = R.effective({str(k): torch.from_numpy(g21[f"{tag}/p/{k}"]) for k in g21[f"{tag}/keys"]}, nb)
    x = torch.from_numpy(g21[f"{tag}/x"])
    for hh, ww in SIZES:
        out = R.forward(x[0], p, (hh, ww))["out"]
        assert R.rel_max(out, torch.from_numpy(g21[f"{tag}/y{hh}x{ww}"])[0]) <= 1e-5


EXACT = [(32, 2, 1) + s for s in R.SIZES] + [(32, 0, 1, 9, 33), (32, 1, 6, 9, 33), (32, 8, 1, 9, 33), (20, 2, 1, 9, 33), (1, 2, 6, 9, 33),
                                             (32, 8, 6, 5, 70), (20, 1, 1, 5, 70), (1, 8, 1, 5, 70), (32, 8, 1, 8, 16), (20, 2, 6, 8, 16),
                                             (1, 1, 1, 8, 16), (32, 0, 1, 8, 16)]


@pytest.mark.parametrize("key", EXACT, ids=lambda k: "c{}-nb{}-n{}-{}x{}".format(*k))
def test_exact_cases_are_exact_and_spoiled_copies_are_not(key):
    case = R.exact_case(*key)
    r = R.check_exact(case)
    assert len(r["y"]) == key[1] and r["D"].shape[-2:] == (4 * key[3] + 1, 4 * key[4] + 1)
    # the case is not trivial: ReLU cuts something and passes something, and the output is not constant
    if key[1] and key[3] * key[4] >= 9:
        t = torch.cat([t.reshape(-1) for t in r["t"]])
        assert bool((t > 0).any()) and bool((t == 0).any())
    assert r["D"].std().item() > 0
    for how in R.SPOILS:
        with pytest.raises(R.NotExact):
            R.check_exact(R.spoil(case, how))


def test_padding_case_counts_taps():
    for c in (1, 32):
        case = R.padding_case(c, 5, 7)
        r = R.check_exact(case)
        assert torch.equal(r["y"][0][0, 0], c * R.tap_counts(5, 7))
    assert R.tap_counts(5, 7)[0, 0] == 4 and R.tap_counts(5, 7)[0, 3] == 6 and R.tap_counts(5, 7)[2, 3] == 9


ROUTES = [
    # (constructor, the call, a word of the expected reason): the model's own limits come first, then the call's
    (dict(args=(4, 32, 1, 3)), dict(grad=True), "autograd"),
    (dict(args=(4, 32, 1, 3)), dict(grad=False), "CPU"),
    (dict(args=(4, 32, 1, 3)), dict(grad=False, size=(25, 31)), "CPU"),
    (dict(args=(4, 32, 1, 3), frozen=True), dict(grad=True), "CPU"),
    (dict(args=(4, 32, 1, 3), frozen=True), dict(grad=True, x_grad=True), "autograd"),
    (dict(args=(2, 32, 1, 3)), dict(grad=False), "scale"),
    (dict(args=(4, 48, 1, 3)), dict(grad=False), "channels"),
    (dict(args=(4, 32, 1, 5)), dict(grad=False), "kernel"),
    (dict(args=(4, 32, 1, 3), hook="fwd"), dict(grad=False), "hook"),
    (dict(args=(4, 32, 1, 3), hook="pre"), dict(grad=False), "hook"),
    (dict(args=(4, 32, 1, 3), aten=True), dict(grad=False), "aten_forward"),
]


@pytest.mark.parametrize("ctor,call,expect", ROUTES)
def test_hot_route_reason_on_cpu(ctor, call, expect):
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    m = Result_Model(*ctor["args"])
    fired = []
    if ctor.get("aten"):
        m.aten_forward = True
    if ctor.get("frozen"):
        m.requires_grad_(False)
    if ctor.get("hook") == "fwd":
        m.body[0].body[0].register_forward_hook(lambda *a: fired.append(1))
    if ctor.get("hook") == "pre":
        m.shuf[0].register_forward_pre_hook(lambda *a: fired.append(1))
    x = torch.rand(1, 2, 3, 6, 8, requires_grad=bool(call.get("x_grad")))
    size = call.get("size", (6 * ctor["args"][0], 8 * ctor["args"][0]))
    with torch.set_grad_enabled(call["grad"]):
        reason = m.hot_route_reason(x, *size)
        assert reason is not None and expect in reason, reason
        y = m(x, *size)
    records = call["grad"] and (not ctor.get("frozen") or bool(call.get("x_grad")))
    assert m.last_route == "aten" and y.shape == (1, 2, 3) + tuple(size) and y.requires_grad == records
    assert len(fired) == (2 if ctor.get("hook") else 0)          # the ATen route calls every module, once per frame
    for bad in (torch.rand(2, 3, 6, 8), torch.rand(1, 2, 4, 6, 8)):
        with pytest.raises(ValueError):
            m(bad)


@pytest.mark.parametrize("channel,nb", [(32, 2), (20, 1), (1, 0)])
def test_fn_tables_round_trip(channel, nb):
    """read the blob back through the layout packing.fn_tables documents"""
    from mobilesuperresolution_amd import packing as P
    layout, offsets = P.fn_tables(channel, nb)
    c, nconv = channel, 2 * nb + 1
    g = torch.Generator().manual_seed(channel * 10 + nb)
    ws = [torch.randn(c, c, 3, 3, generator=g) for _ in range(nconv)]
    bs = [torch.randn(c, generator=g) for _ in range(nconv)]
    up_w, up_b = torch.randn(c, 3, 5, 5, generator=g), torch.randn(3, generator=g)
    src = torch.cat([t.reshape(-1) for wb in zip(ws, bs) for t in wb] + [up_w.reshape(-1), up_b, torch.zeros(1)])
    assert src.numel() == layout["size"] and len(offsets) == nconv + 1
    blob = src[torch.from_numpy(layout["pack"])]
    assert blob.numel() == offsets[-1] + P.FN_UP_ELEMS and offsets == [j * P.FN_CONV_ELEMS for j in range(nconv + 1)]
    for jc in range(nconv):
        frag = blob[offsets[jc]:offsets[jc] + 18 * 512].view(18, 64, 8)
        w32 = torch.zeros(32, 32, 9)
        for s in range(18):
            for lane in range(64):
                for j in range(8):
                    kk = 16 * s + 8 * (lane >> 5) + j
                    w32[lane & 31, kk % 32, kk // 32] = frag[s, lane, j]
        assert torch.equal(w32[:c, :c].reshape(c, c, 3, 3), ws[jc])
        w32[:c, :c] = 0
        assert not w32.any()                               # padded rows and columns
        bias = blob[offsets[jc] + 18 * 512:offsets[jc] + P.FN_CONV_ELEMS]
        assert torch.equal(bias[:c], bs[jc]) and not bias[c:].any()
    up = blob[offsets[-1]:offsets[-1] + 5 * 512].view(5, 64, 8)
    e = torch.zeros(32, 80)
    for eb in range(5):
        for lane in range(64):
            for j in range(8):
                e[8 * (lane >> 4) + j, 16 * eb + (lane & 15)] = up[eb, lane, j]
    assert torch.equal(e[:c, :75].reshape(c, 3, 5, 5), up_w) and not e[c:].any() and not e[:, 75:].any()
    tail = blob[offsets[-1] + 5 * 512:]
    assert torch.equal(tail[:3], up_b) and not tail[3:].any()
    for bad in ((0, 1), (33, 1), (8, -1)):
        with pytest.raises(ValueError):
            P.fn_tables(*bad)
