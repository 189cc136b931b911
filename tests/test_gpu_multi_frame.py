"""The multi-frame video network on the MI355X: csrc/multi_frame.h through sr_mf_net_fwd and models/naive_multi_model_easy.py, both
hot dtypes, against tests/multi_frame_ref.py (float64) and fixture G22.  Outputs and all scratch are NaN-filled before every call.

  exact cases     torch.equal to the float64 reference, stage by stage (the `stages` mask: ENCODER, FIRST, BLOCKS, TAIL) at every
                  tile-edge size; the padding channels of every scratch image stay exactly zero, untouched buffers stay NaN
  warp edges      zero, integer, far, quarter-pixel and inward flows; clip 1 does not see clip 0
  padding of t    conv1 = 0, b1 = 1, conv2 = 1 on block 0: y - e counts 4 / 6 / 9 taps along the border ring
  tail            decode = 0 gives F.interpolate(x, scale_factor=4) of the same device bit for bit
  rounded cases   fp32 route within 8 x the distance of the fp32 ATen route on the same device from float64; bf16 route within 4 x the
                  distance of the reference's bf16 rounding-point variant from float64 (parity_kit.bound); every ratio is printed
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import multi_frame_ref as R
from tests.parity_kit import bound
from tests.test_multi_frame_host import NoFlowNet, sampled, seeded_model

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_multi_frame.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """drop this module's device-resident pack indices and hand the free blocks back when the module is done: tests elsewhere in the
    suite assert exact torch.cuda.memory_allocated() deltas"""
    yield
    import gc
    from mobilesuperresolution_amd import hotpath as HP
    HP._mf_pack_index.cache_clear()
    HP._fn_pack_index.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def nhwc32(t):
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, 32, dtype=torch.float64)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


class Net:
    """a parameter set packed for sr_mf_net_fwd, NaN-filled scratch and output"""

    def __init__(self, case, dtype):
        from mobilesuperresolution_amd import hotpath as HP
        p = case["p"]
        dev = lambda t: t.float().to(DEV)
        self.nb, self.dtype, self.B, self.N = case["nb"], dtype, case["B"], case["N"]
        self.blob = HP.mf_pack([tuple(dev(t) for t in blk) for blk in p["blocks"]], dev(p["dec_w"]), dev(p["dec_b"]), dtype)
        self.head = HP.fn_pack_encoder(dev(p["enc_w"]), dev(p["enc_b"]), dtype)
        b, n, _, h, w = case["x"].shape
        self.x = case["x"].float().reshape(b * n, 3, h, w).to(DEV).contiguous()
        self.flows = case["flows"].float().to(DEV).contiguous() if n > 1 else None
        self.scratch = torch.full((3, b * n, h, w, 32), float("nan"), dtype=dtype, device=DEV)
        self.out = torch.full((b * n, 3, 4 * h, 4 * w), float("nan"), dtype=torch.float32, device=DEV)

    def run(self, stages):
        from mobilesuperresolution_amd import hotpath as HP
        HP.mf_net_fwd(self.x, self.flows, self.blob, self.head, self.scratch, self.out, self.nb, self.B, self.N, stages)
        torch.cuda.synchronize()

    def s(self, i):
        return self.scratch[i].double().cpu()

    def slot(self, i):
        """scratch index of block i's output: 1, 2, 1, .."""
        return 1 + (i % 2)


def _nan(t):
    return bool(torch.isnan(t.float()).all())


def _staged(case, mode):
    """every stage of an exact case, one `stages` bit at a time on the scratch as it stands"""
    from mobilesuperresolution_amd import packing as P
    net, ref = Net(case, DTYPES[mode]), case["ref"]
    net.run(P.MF_ENCODER)
    assert torch.equal(net.s(0), nhwc32(ref["e"])), "e"
    assert _nan(net.scratch[1:]) and _nan(net.out)
    net.run(P.MF_FIRST)
    assert torch.equal(net.s(1), nhwc32(ref["y"][0])), "y0"
    assert _nan(net.scratch[2]) and _nan(net.out) and torch.equal(net.s(0), nhwc32(ref["e"]))
    net.run(P.MF_BLOCKS)
    for i in range(max(0, net.nb - 2), net.nb):                  # the last two block outputs are still in the scratch
        assert torch.equal(net.s(net.slot(i)), nhwc32(ref["y"][i])), f"y{i}"
    assert _nan(net.out) and (net.nb > 1 or _nan(net.scratch[2]))
    net.run(P.MF_TAIL)
    assert torch.equal(net.out.double().cpu(), ref["out"]), "out"
    assert torch.equal(net.s(0), nhwc32(ref["e"]))
    # all stages in one call from NaN scratch give the same bits
    again = Net(case, DTYPES[mode])
    again.run(P.MF_ALL)
    assert torch.equal(again.out, net.out)
    return net


_id = lambda k: "c{}-nb{}-b{}-n{}-{}x{}-{}".format(*k)
EDGES = [(32, 2, 1, 3) + s + ("int",) for s in R.SIZES] + \
        [(32, 1, 2, 3, 9, 33, "int"), (32, 3, 1, 3, 9, 33, "int"), (20, 2, 2, 1, 9, 33, "int"), (1, 3, 1, 1, 9, 33, "int"), (1, 1, 1, 3, 5, 70, "int"),
         (20, 1, 2, 3, 5, 70, "int")]
WARPS = [(32, 1, 1, 2, 9, 33, "zero"), (32, 1, 1, 3, 17, 65, "far"), (20, 1, 1, 2, 17, 65, "far"), (32, 1, 1, 2, 9, 33, "quarter"),
         (20, 1, 2, 2, 17, 65, "quarter"), (32, 1, 1, 2, 5, 17, "quarter"), (32, 1, 1, 2, 9, 33, "inward"), (32, 1, 1, 2, 17, 65, "inward")]


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", EDGES, ids=_id)
def test_tile_edges_exact_per_stage(key, mode):
    _staged(R.exact_case(*key), mode)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", WARPS, ids=_id)
def test_warp_edges_exact(key, mode):
    case = R.exact_case(*key)
    net = _staged(case, mode)
    if key[6] == "zero":
        # the warp is a copy of e_{i-1}, not of e_i: the reference with warp = e_i differs
        ref = case["ref"]
        assert not torch.equal(ref["warp"][1], ref["e"][1]) and torch.equal(ref["warp"][1], ref["e"][0])
        assert torch.equal(net.s(1), nhwc32(ref["y"][0]))


@pytest.mark.parametrize("mode", DTYPES)
def test_clip_1_does_not_see_clip_0(mode):
    """frame 0 of clip 1 takes warp = its own e and flow = 0: the same clip run alone gives the same bits, whatever clip 0 holds"""
    from mobilesuperresolution_amd import packing as P
    case = R.exact_case(32, 2, 2, 3, 9, 33, "int")
    sentinel = dict(case, x=case["x"].clone())
    sentinel["x"][0] = 3.0 - case["x"][0]                       # another clip 0
    alone = dict(case, B=1, x=case["x"][1:], flows=case["flows"][1:])
    outs = []
    for c in (case, sentinel, alone):
        net = Net(c, DTYPES[mode])
        net.run(P.MF_ALL)
        outs.append((net.out[-3:].clone(), net.scratch[1:, -3:].clone()))
    assert torch.equal(outs[0][0].double().cpu(), case["ref"]["out"][-3:])
    for o, s in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(s, outs[0][1])
    assert not torch.equal(sentinel["x"][0], case["x"][0])


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("channel", (1, 32))
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (R.TH, R.TW), (R.TH + 1, R.TW + 1), (2 * R.TH + 1, 2 * R.TW + 1)], ids=lambda s: "{}x{}".format(*s))
def test_t_is_zero_outside_the_image(size, channel, mode):
    from mobilesuperresolution_amd import packing as P
    case = R.padding_case(channel, *size)
    net = Net(case, DTYPES[mode])
    net.run(P.MF_ENCODER | P.MF_FIRST)
    y = net.s(1)
    want = (channel * R.tap_counts(*size)).view(1, size[0], size[1], 1).expand(2, size[0], size[1], channel)
    assert torch.equal(y[..., :channel], want) and not y[..., channel:].any()


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("size", [(1, 1), (3, 3), (R.TH + 1, R.TW + 1), (5, 70)], ids=lambda s: "{}x{}".format(*s))
def test_decode_zero_is_the_devices_own_interpolate(size, mode):
    from mobilesuperresolution_amd import packing as P
    case = dict(R.rounded_case(20, 1, 1, 2, *size))
    p = dict(case["p"])
    p["dec_w"], p["dec_b"] = torch.zeros_like(p["dec_w"]), torch.zeros_like(p["dec_b"])
    case["p"] = p
    net = Net(case, DTYPES[mode])
    net.run(P.MF_ALL)
    want = F.interpolate(net.x, scale_factor=4, mode="bilinear", align_corners=False)
    assert torch.equal(net.out, want)


# ---- rounded cases ---------------------------------------------------------------------------------------------------------------
def _module(case, mode, monkeypatch):
    from mobilesuperresolution_amd.models import naive_multi_model_easy as M
    monkeypatch.setattr(M, "SpyNet", NoFlowNet)
    m = M.Naive_model(4, status=[[case["channel"], case["channel"], 3]] * case["nb"], hot_dtype=mode)
    m.load_state_dict(R.state_dict_of(case["p"]), strict=False)
    return m.to(DEV).eval()


def _hold(tag, mode, got, ref, yard):
    err = R.rel_max(got.detach().double().cpu(), ref)
    tol = bound(mode, yard, slack=0.0)
    print(f"multi frame parity | {tag} | {mode} | yardstick {yard:.3e} | kernel {err:.3e} | ratio {err / yard:.2f} | bound {tol:.3e}")
    assert err <= tol, (tag, mode, err, tol)


def _both_routes(m, x, flows, mode, p, tag, pick=lambda t: t):
    """the HIP route against float64 with the yardstick of its dtype"""
    ref = R.forward(x, flows, p)["out"].view(x.shape[0], x.shape[1], 3, 4 * x.shape[3], 4 * x.shape[4])
    xd, fd = x.float().to(DEV), flows.float().to(DEV)
    m.get_flow = lambda x_: fd
    with torch.no_grad():
        if mode == "fp32":
            m.aten_forward = True
            aten = m(xd)
            m.aten_forward = False
            assert m.last_route == "aten"
            yard = R.rel_max(pick(aten.double().cpu()), pick(ref))
        else:
            yard = R.rel_max(pick(R.forward(x, flows, p, rnd=R.bf16_round)["out"].view(ref.shape)), pick(ref))
        got = m(xd, 4 * x.shape[3], 4 * x.shape[4])
        assert m.hot_route_reason(xd) is None
    assert m.last_route == "hip" and got.shape == ref.shape and got.dtype == torch.float32
    _hold(tag, mode, pick(got), pick(ref), yard)
    return got


ROUNDED = [(32, 8, 2, 3, 9, 33), (20, 2, 1, 2, 17, 65), (32, 1, 1, 1, 17, 65)]


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", ROUNDED, ids=lambda k: "c{}-nb{}-b{}-n{}-{}x{}".format(*k))
def test_rounded(key, mode, monkeypatch):
    case = R.rounded_case(*key)
    m = _module(case, mode, monkeypatch)
    # the float64 reference runs on the effective weights the module really has (fp32 weight norm of the loaded g, v)
    p = R.effective({k: v.cpu() for k, v in m.state_dict().items()}, case["nb"])
    got = _both_routes(m, case["x"].float(), case["flows"].float(), mode, p, "c{}-nb{}-b{}-n{}-{}x{}".format(*key))
    with torch.no_grad():
        assert torch.equal(got, m(case["x"].float().to(DEV)))                          # calls repeat
    with torch.enable_grad():
        y = m(case["x"].float().to(DEV).requires_grad_(True))
    assert m.last_route == "aten" and y.requires_grad


@pytest.fixture(scope="module")
def g22():
    return np.load(GOLD)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("tag", ("a", "b", "c"))
def test_g22_through_the_hip_route(g22, tag, mode, monkeypatch):
    m = seeded_model(g22, tag, monkeypatch, hot_dtype=mode).to(DEV)
    p = R.effective({k: v.cpu() for k, v in m.state_dict().items()}, len(m.idx))
    x, flows = torch.from_numpy(g22[f"{tag}/x"]), torch.from_numpy(g22[f"{tag}/flows"])
    got = _both_routes(m, x, flows, mode, p, f"G22 {tag}")
    # and against the reference's own output (fp32 on the CPU): the fp32 route sits within a few fp32 roundings of it
    want = torch.from_numpy(g22[f"{tag}/y"]).reshape(-1)
    err = R.rel_max(sampled(got.cpu(), g22, tag).reshape(-1), want)
    print(f"multi frame G22 | {tag} | {mode} | rel max-abs to the reference's output {err:.3e}")
    if mode == "fp32":
        assert err <= 1e-5
    # training keeps the ATen route
    m.get_flow = lambda x_: flows.to(DEV)
    y = m(x.to(DEV), 48, 80)
    assert m.last_route == "aten" and y.requires_grad


@pytest.mark.parametrize("mode", DTYPES)
def test_real_flows_and_the_stage_wise_call_agree(mode):
    from mobilesuperresolution_amd import hotpath as HP, packing as P
    from mobilesuperresolution_amd.models import naive_multi_model_easy as M
    torch.manual_seed(7)
    m = M.Naive_model(4, status=[[32, 32, 3]] * 2, hot_dtype=mode).to(DEV).eval()
    x = torch.rand(1, 3, 3, 64, 64, generator=torch.Generator().manual_seed(8)).to(DEV)
    with torch.no_grad():
        y = m(x, 256, 256)
        flows = m.get_flow(x)
    assert m.last_route == "hip" and bool(torch.isfinite(y).all()) and flows.shape == (1, 2, 2, 64, 64)
    blob, head = m._blobs()
    scratch = torch.full((3, 3, 64, 64, 32), float("nan"), dtype=DTYPES[mode], device=DEV)
    out = torch.full((3, 3, 256, 256), float("nan"), dtype=torch.float32, device=DEV)
    for stage in (P.MF_ENCODER, P.MF_FIRST, P.MF_BLOCKS, P.MF_TAIL):
        HP.mf_net_fwd(x[0].contiguous(), flows.contiguous(), blob, head, scratch, out, 2, 1, 3, stage)
    torch.cuda.synchronize()
    assert torch.equal(out, y[0])
    # pickling drops the packed blobs; the copy packs again and agrees
    import pickle
    m2 = pickle.loads(pickle.dumps(m))
    assert not hasattr(m2, "_mf_blobs")
    with torch.no_grad():
        assert torch.equal(m2(x), y)
    x.requires_grad_(True)
    assert "autograd" in m.hot_route_reason(x)


@pytest.mark.parametrize("mode", DTYPES)
def test_unsupported_geometry_is_refused_untouched(mode):
    from mobilesuperresolution_amd import _lib as L
    net = Net(R.exact_case(32, 1, 1, 2, 3, 3, "int"), DTYPES[mode])
    lib, code = L.lib(), L.DTYPE_CODE[DTYPES[mode]]

    def call(b=1, n=2, h=3, w=3, nb=1, dtype=code, stages=15, blob=net.blob.data_ptr(), flows=net.flows.data_ptr()):
        return lib.sr_mf_net_fwd(net.x.data_ptr(), flows, blob, net.head.data_ptr(), net.scratch[0].data_ptr(), net.scratch[1].data_ptr(),
                                 net.scratch[2].data_ptr(), net.out.data_ptr(), nb, b, n, h, w, dtype, stages, L.stream_ptr())

    for kw, rc in ((dict(b=65536), -1), (dict(b=300, n=300), -1), (dict(h=8193), -1), (dict(w=8193), -1), (dict(dtype=7), -1), (dict(nb=1025), -1),
                   (dict(blob=None), -2), (dict(flows=None), -2), (dict(stages=0), -2), (dict(stages=16), -2), (dict(nb=0), -2), (dict(n=0), -2)):
        assert call(**kw) == rc, kw
        torch.cuda.synchronize()
        assert _nan(net.scratch) and _nan(net.out)
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(net.out).any())
