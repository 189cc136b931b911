"""The per-frame video network on the MI355X: csrc/frame_net.h through sr_fn_net_fwd and models/single_image_model.py, both hot
dtypes, against tests/frame_net_ref.py (float64) and fixture G21.  Outputs and all scratch are NaN-filled before every call.

  exact cases     torch.equal to the float64 reference, stage by stage (the `stages` mask) up to D at every tile-edge size and end
                  to end at 8 x 16; the padding channels of every scratch image stay exactly zero
  padding of t    conv1 = 0, b1 = 1, conv2 = 1: y - x counts 4 / 6 / 9 taps along the border ring
  rounded cases   fp32 route within 8 x the distance of the fp32 ATen route on the same device from float64; bf16 route within 4 x the
                  distance of the reference's bf16 rounding-point variant from float64 (the factors of tests/test_gpu_block_ref.py);
                  every ratio is printed
"""
import os

import numpy as np
import pytest
import torch

from tests import frame_net_ref as R
from tests.parity_kit import bound

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_single_frame.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """drop this module's device-resident pack indices (one per (channel, blocks) pair, the larger ones in the allocator's large
    pool) and hand the free blocks back when the module is done: tests elsewhere in the suite assert exact
    torch.cuda.memory_allocated() deltas, which count a reused oversized fragment next to a live block in full"""
    yield
    import gc
    from mobilesuperresolution_amd import hotpath as HP
    HP._fn_pack_index.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def nhwc32(t):
    """(N, C, H, W) float64 -> (N, H, W, 32) with zero padding channels"""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, 32, dtype=torch.float64)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


class Net:
    """a parameter set packed for sr_fn_net_fwd, NaN-filled scratch and outputs"""

    def __init__(self, case, dtype):
        from mobilesuperresolution_amd import hotpath as HP
        p = case["p"]
        dev = lambda t: t.float().to(DEV)
        self.nb, self.dtype = case["nb"], dtype
        self.blob, self.offs = HP.fn_pack([(dev(w), dev(b)) for w, b in p["convs"]], dev(p["up_w"]), dev(p["up_b"]), dtype)
        self.head = HP.fn_pack_encoder(dev(p["enc_w"]), dev(p["enc_b"]), dtype)
        self.x = case["x"].float().to(DEV).contiguous()
        n, _, h, w = self.x.shape
        self.n, self.h, self.w = n, h, w
        self.scratch = torch.full((3, n, h, w, 32), float("nan"), dtype=dtype, device=DEV)
        self.out = torch.full((n, 3, 4 * h, 4 * w), float("nan"), dtype=torch.float32, device=DEV)
        self.d = torch.full((n, 3, 4 * h + 1, 4 * w + 1), float("nan"), dtype=torch.float32, device=DEV)

    def run(self, stages, to_d=False):
        from mobilesuperresolution_amd import hotpath as HP, packing as P
        dst = self.d if to_d else self.out
        HP.fn_net_fwd(self.x, self.blob, self.offs, self.head, self.scratch, dst, dst.stride(0), self.nb,
                      stages | (P.FN_WRITE_D if to_d else 0))
        torch.cuda.synchronize()

    def s(self, i):
        return self.scratch[i].double().cpu()

    def block_slot(self, i):
        """scratch index of block i's output (the blocks alternate 1, 2, 1, ..); f lands in the other one of 1 / 2"""
        return 1 + (i % 2)

    def f_slot(self):
        return 1 if self.nb == 0 or self.block_slot(self.nb - 1) == 2 else 2


def _staged(case, mode):
    """every stage of an exact case, one `stages` bit at a time on the scratch as it stands"""
    from mobilesuperresolution_amd import packing as P
    net, ref = Net(case, DTYPES[mode]), case["ref"]
    net.run(P.FN_ENCODER)
    assert torch.equal(net.s(0), nhwc32(ref["e"])), "e"
    assert bool(torch.isnan(net.scratch[1:].float()).all()) and bool(torch.isnan(net.out).all()) and bool(torch.isnan(net.d).all())
    net.run(P.FN_BLOCKS)
    for i in range(max(0, net.nb - 2), net.nb):                  # the last two block outputs are still in the scratch
        assert torch.equal(net.s(net.block_slot(i)), nhwc32(ref["y"][i])), f"y{i}"
    assert torch.equal(net.s(0), nhwc32(ref["e"]))
    net.run(P.FN_LAST)
    assert torch.equal(net.s(net.f_slot()), nhwc32(ref["f"])), "f"
    assert bool(torch.isnan(net.out).all()) and bool(torch.isnan(net.d).all())
    net.run(P.FN_UP, to_d=True)
    assert torch.equal(net.d.double().cpu(), ref["D"]), "D"
    assert bool(torch.isnan(net.out).all())
    return net


CASES = [(32, 2, 1) + s for s in R.SIZES] + [(32, 0, 1, 9, 33), (32, 1, 6, 9, 33), (32, 8, 1, 9, 33), (20, 2, 1, 9, 33), (1, 2, 6, 9, 33),
                                             (32, 8, 6, 5, 70), (20, 1, 1, 5, 70), (1, 8, 1, 5, 70)]
_id = lambda k: "c{}-nb{}-n{}-{}x{}".format(*k)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", CASES, ids=_id)
def test_tile_edges_exact_per_stage(key, mode):
    _staged(R.exact_case(*key), mode)


E2E = [(32, 8, 1, 8, 16), (20, 2, 6, 8, 16), (1, 1, 1, 8, 16), (32, 0, 1, 8, 16)]


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", E2E, ids=_id)
def test_exact_end_to_end(key, mode):
    from mobilesuperresolution_amd import packing as P
    case = R.exact_case(*key)
    net = _staged(case, mode)
    net.run(P.FN_UP)
    assert torch.equal(net.out.double().cpu(), case["ref"]["out"])
    # all stages in one call from NaN scratch give the same bits
    again = Net(case, DTYPES[mode])
    again.run(P.FN_ALL)
    assert torch.equal(again.out, net.out)
    for i in range(3):
        s = again.scratch[i].float()
        assert bool(torch.isnan(s).all()) or (not bool(torch.isnan(s).any()) and not bool(s[..., key[0]:].any()))


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("channel", (1, 32))
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (R.TH, R.TW), (R.TH + 1, R.TW + 1), (2 * R.TH + 1, 2 * R.TW + 1)], ids=lambda s: "{}x{}".format(*s))
def test_t_is_zero_outside_the_image(size, channel, mode):
    from mobilesuperresolution_amd import packing as P
    case = R.padding_case(channel, *size)
    net = Net(case, DTYPES[mode])
    net.run(P.FN_ENCODER | P.FN_BLOCKS)
    y = net.s(1)
    want = (channel * R.tap_counts(*size)).view(1, size[0], size[1], 1).expand(1, size[0], size[1], channel)
    assert torch.equal(y[..., :channel], want) and not y[..., channel:].any()


# ---- rounded cases ---------------------------------------------------------------------------------------------------------------
def _module(case, mode):
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    m = Result_Model(4, case["channel"], case["nb"], 3, hot_dtype=mode)
    m.load_state_dict(R.state_dict_of(case["p"]), strict=False)
    return m.to(DEV).eval()


def _hold(tag, mode, got, ref, yard):
    err = R.rel_max(got.detach().double().cpu(), ref)
    tol = bound(mode, yard, slack=0.0)                      # (this suite's fp32 bound has no additive term)
    print(f"frame net parity | {tag} | {mode} | yardstick {yard:.3e} | kernel {err:.3e} | ratio {err / yard:.2f} | bound {tol:.3e}")
    assert err <= tol, (tag, mode, err, tol)


ROUNDED = [(32, 8, 2, 17, 33), (20, 2, 1, 9, 40)]


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", ROUNDED, ids=_id)
def test_rounded(key, mode):
    case = R.rounded_case(*key)
    n, h, w = key[2:]
    m = _module(case, mode)
    # the float64 reference runs on the effective weights the module really has (fp32 weight norm of the loaded g, v)
    p = R.effective({k: v.cpu() for k, v in m.state_dict().items()}, case["nb"])
    x = case["x"].float()
    for size in ((4 * h, 4 * w), (4 * h + 3, 4 * w - 5)):
        ref = R.forward(x, p, size)["out"]
        if mode == "fp32":
            m.aten_forward = True
            with torch.no_grad():
                aten = m(x.to(DEV).unsqueeze(0), *size)[0]
            m.aten_forward = False
            assert m.last_route == "aten"
            yard = R.rel_max(aten.double().cpu(), ref)
        else:
            yard = R.rel_max(R.forward(x, p, size, rnd=R.bf16_round)["out"], ref)
        with torch.no_grad():
            got = m(x.to(DEV).unsqueeze(0), *size)[0]
        assert m.last_route == "hip"
        _hold(f"{_id(key)} -> {size[0]}x{size[1]}", mode, got, ref, yard)


# ---- G21 through the module ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g21():
    return np.load(GOLD)


def _g21_model(g21, tag, mode):
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    m = Result_Model(*[int(v) for v in g21[f"{tag}/args"]], hot_dtype=mode)
    m.load_state_dict({str(k): torch.from_numpy(g21[f"{tag}/p/{k}"]) for k in g21[f"{tag}/keys"]}, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("tag", ("a", "b"))
def test_g21_through_the_module(g21, tag, mode):
    m = _g21_model(g21, tag, mode)
    nb = int(g21[f"{tag}/args"][2])
    x = torch.from_numpy(g21[f"{tag}/x"])
    p = R.effective({k: v.cpu() for k, v in m.state_dict().items()}, nb)
    for size in ((48, 80), (50, 77)):
        want = torch.from_numpy(g21[f"{tag}/y{size[0]}x{size[1]}"])
        with torch.no_grad():
            got = m(x.to(DEV), *size)
        assert m.last_route == "hip" and got.shape == want.shape and got.dtype == torch.float32
        if mode == "fp32":
            err = R.rel_max(got.cpu(), want)
            print(f"frame net G21 | {tag} | fp32 | {size} | rel max-abs {err:.3e}")
            assert err <= 1e-5
        else:
            ref = R.forward(x[0], p, size)["out"]
            yard = R.rel_max(R.forward(x[0], p, size, rnd=R.bf16_round)["out"], ref)
            _hold(f"G21 {tag} {size}", mode, got[0], ref, yard)
    m.zero_grad()
    y = m(x.to(DEV), 48, 80)
    assert m.last_route == "aten" and y.requires_grad
    torch.testing.assert_close(y.detach().cpu(), torch.from_numpy(g21[f"{tag}/y48x80"]), rtol=1e-4, atol=1e-5)
    y.sum().backward()
    for k, prm in m.named_parameters():
        want = torch.from_numpy(g21[f"{tag}/g/{k}"])
        got = prm.grad.cpu() if prm.grad is not None else torch.zeros_like(want)
        assert R.rel_max(got, want) <= 1e-4 or float(want.abs().max()) == 0.0, k


@pytest.mark.parametrize("mode", DTYPES)
def test_routes_agree_and_calls_repeat(mode):
    """both routes on one random 1 x 3 x 3 x 20 x 28 clip; two equal HIP calls; a non-contiguous view"""
    case = R.rounded_case(32, 2, 3, 20, 28)
    m = _module(case, mode)
    p = R.effective({k: v.cpu() for k, v in m.state_dict().items()}, case["nb"])
    x = case["x"].float().unsqueeze(0).to(DEV)
    ref = R.forward(case["x"].float(), p)["out"]
    with torch.no_grad():
        a = m(x, 80, 112)
        assert m.last_route == "hip" and m.hot_route_reason(x, 80, 112) is None and m.hot_route_reason(x, 81, 100) is None
        b = m(x, 80, 112)
        m.aten_forward = True
        aten = m(x, 80, 112)
        assert m.last_route == "aten"
        m.aten_forward = False
        wide = torch.rand(1, 3, 5, 20, 30, device=DEV)
        wide[:, :, 1:4, :, 1:29] = x
        view = wide[:, :, 1:4, :, 1:29]
        assert not view.is_contiguous()
        c = m(view, 80, 112)
        cd = m(view, 77, 100)
        dd = m(x, 77, 100)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(cd, dd)
    if mode == "fp32":
        yard = R.rel_max(aten[0].double().cpu(), ref)
    else:
        yard = R.rel_max(R.forward(case["x"].float(), p, rnd=R.bf16_round)["out"], ref)
    _hold("routes 20x28", mode, a[0], ref, yard)
    with torch.enable_grad():
        y = m(x, 80, 112)
    assert m.last_route == "aten" and y.requires_grad
    h = m.encoder.register_forward_hook(lambda *args: None)
    with torch.no_grad():
        assert "hook" in m.hot_route_reason(x, 80, 112)
        m(x, 80, 112)
        assert m.last_route == "aten"
        h.remove()
        m(x, 80, 112)
        assert m.last_route == "hip"


@pytest.mark.parametrize("mode", DTYPES)
def test_unsupported_geometry_is_refused_untouched(mode):
    from mobilesuperresolution_amd import _lib as L
    net = Net(R.exact_case(32, 1, 1, 3, 3), DTYPES[mode])
    lib, code = L.lib(), L.DTYPE_CODE[DTYPES[mode]]

    def call(n=1, h=3, w=3, nb=1, dtype=code, stages=15, blob=net.blob.data_ptr()):
        return lib.sr_fn_net_fwd(net.x.data_ptr(), blob, net.offs, net.head.data_ptr(), net.scratch[0].data_ptr(), net.scratch[1].data_ptr(),
                                 net.scratch[2].data_ptr(), net.out.data_ptr(), net.out.stride(0), nb, n, h, w, dtype, stages, L.stream_ptr())

    for kw, rc in ((dict(n=65536), -1), (dict(h=8193), -1), (dict(w=8193), -1), (dict(dtype=7), -1), (dict(nb=1025), -1),
                   (dict(blob=None), -2), (dict(stages=0), -2), (dict(stages=32), -2), (dict(nb=-1), -2)):
        assert call(**kw) == rc, kw
        torch.cuda.synchronize()
        assert bool(torch.isnan(net.scratch.float()).all()) and bool(torch.isnan(net.out).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(net.out).any())
