"""The HIP training route of the per-frame video network on the MI355X: sr_fn_net_train_fwd / sr_fn_net_bwd (csrc/frame_net.h,
csrc/frame_net_bwd.h, csrc/result_block.h) and models/single_image_model.py with hot_training, both hot dtypes, against
tests/frame_net_train_ref.py (float64) and fixture G21.  Outputs, saved images, scratch, slabs and gradients are NaN-filled (masks:
-1) before every call; every measured ratio is printed.

  route           hot_training sends a graph-recording call down "hip_train", bit-identical to the no_grad HIP output; every excluded
                  condition keeps "aten" and names its reason
  exact cases     per stage through the `stages` mask, torch.equal to the float64 reference: the conv stages from an injected integer
                  df at the kernels' tile edges in both dtypes; the whole chain from an edge-line output gradient where dD is a value
                  of the hot dtype (fp32: power-of-two sizes up to 8 x 16 and 16 x 32; bf16: H W <= 4, see frame_net_train_ref)
  rounded cases   fp32 within 8 x the fp32 ATen route's distance from float64 (same device, TF32 off), bf16 within 4 x the
                  rounding-point reference's (tests/parity_kit.bound)
  G21, determinism, three real optimiser steps, refusals
"""
import os

import numpy as np
import pytest
import torch

from tests import frame_net_ref as R
from tests import frame_net_train_ref as T
from tests.parity_kit import bound, hold_exact, hold_rounded, rel_max

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_single_frame.npz")
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """as tests/test_gpu_frame_net.py: drop the device-resident pack indices and hand the free blocks back"""
    yield
    import gc
    from mobilesuperresolution_amd import hotpath as HP
    HP._fn_pack_index.cache_clear()
    HP._fn_bwd_pack_index.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def nhwc32(t):
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, 32, dtype=torch.float64)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


def mask_bits(t):
    """(N, C, H, W) -> (N, H, W) int64: bit c = t[c] > 0"""
    return ((t > 0).long() << torch.arange(t.shape[1]).view(1, -1, 1, 1)).sum(1)


class TrainNet:
    """a parameter set packed for the two entry points; everything they write starts as NaN"""

    def __init__(self, case, dtype, wgs=0):
        from mobilesuperresolution_amd import hotpath as HP, packing as P
        p = case["p"]
        dev = lambda t: t.float().to(DEV)
        self.nb, self.c, self.dtype = case["nb"], case["channel"], dtype
        self.blob, self.offs, self.bwd_blob = HP.fn_pack([(dev(w), dev(b)) for w, b in p["convs"]], dev(p["up_w"]), dev(p["up_b"]), dtype,
                                                         backward=True)
        self.head = HP.fn_pack_encoder(dev(p["enc_w"]), dev(p["enc_b"]), dtype)
        self.x = case["x"].float().to(DEV).contiguous()
        n, _, h, w = self.x.shape
        self.n, self.h, self.w = n, h, w
        full = lambda shape, dt=dtype: torch.full(shape, NAN, dtype=dt, device=DEV)
        self.acts, self.ts = full((self.nb + 2, n, h, w, 32)), full((self.nb, n, h, w, 32))
        self.masks = torch.full((self.nb, n, h, w), -1, dtype=torch.int32, device=DEV)
        self.out = full((n, 3, 4 * h, 4 * w), torch.float32)
        self.gs = full((4, n, h, w, 32))
        self.wgs = wgs or HP.fn_bwd_wgs(n, h, w)
        self.parts = full((P.fn_bwd_parts(self.nb, self.wgs),), torch.float32)
        self.sizes = P.fn_grad_sizes(self.c, self.nb)
        self.grads = full((sum(self.sizes),), torch.float32)

    def fwd(self, stages=None):
        from mobilesuperresolution_amd import hotpath as HP, packing as P
        HP.fn_net_train_fwd(self.x, self.blob, self.offs, self.head, self.acts, self.ts, self.masks, self.out, self.out.stride(0), self.nb,
                            P.FN_ALL if stages is None else stages)
        torch.cuda.synchronize()

    def bwd(self, g, stages=None):
        from mobilesuperresolution_amd import hotpath as HP, packing as P
        g = g.float().to(DEV).contiguous()
        HP.fn_net_bwd(self.x, g, g.stride(0), self.bwd_blob, self.acts, self.ts, self.masks, self.gs, self.parts, self.wgs, self.grads,
                      self.c, self.nb, P.FN_BWD_ALL if stages is None else stages)
        torch.cuda.synchronize()

    def g(self, i):
        return self.gs[i].double().cpu()

    def dx0_slot(self):
        return 1 if self.nb % 2 == 0 else 3

    def pieces(self):
        """{name: flat gradient} in the grads vector's order: w0, b0, .., up_w, up_b, enc_w, enc_b"""
        names = [f"{k}{j}" for j in range(2 * self.nb + 1) for k in "wb"] + ["up_w", "up_b", "enc_w", "enc_b"]
        return dict(zip(names, self.grads.cpu().split(self.sizes)))

    def grad_rows(self, ref_grads, only=None):
        """(name, got, expected) for the gradient tensors the reference holds (only: a subset of the names)"""
        got = self.pieces()
        return [(k, got[k].double().view(v.shape), v) for k, v in T.flat_grads(ref_grads) if only is None or k in only]

    def nan_except(self, names):
        return all(bool(torch.isnan(p).all()) for k, p in self.pieces().items() if k not in names)

    def conv_slab_padding_is_zero(self):
        from mobilesuperresolution_amd import packing as P
        tap, row, col = np.meshgrid(np.arange(10), np.arange(32), np.arange(32), indexing="ij")
        dead = (row >= self.c) | ((col >= self.c) & (tap < 9))
        idx = torch.from_numpy(P._acc_pos(tap[dead], row[dead], col[dead]).astype(np.int64))
        slabs = self.parts[:(2 * self.nb + 1) * self.wgs * P.FN_CONV_SLAB].view(-1, P.FN_CONV_SLAB).cpu()
        return not bool(slabs[:, idx].any())


def _saved_forward_is_exact(net, ref, channel):
    fw = ref["fw"]
    ys = [fw["e"]] + fw["y"]
    pairs = [(f"x{i}", net.acts[i].double(), nhwc32(ys[i])) for i in range(net.nb + 1)] + [("f", net.acts[net.nb + 1].double(), nhwc32(fw["f"]))]
    pairs += [(f"t{i}", net.ts[i].double(), nhwc32(fw["t"][i])) for i in range(net.nb)]
    pairs += [(f"mask{i}", net.masks[i].long() & 0xFFFFFFFF, mask_bits(fw["t"][i])) for i in range(net.nb)]
    hold_exact("saved forward", pairs)
    if net.h & (net.h - 1) == 0 and net.w & (net.w - 1) == 0:          # the resize is exact at power-of-two sizes only
        assert torch.equal(net.out.double().cpu(), fw["out"])


# ---- exact cases: the conv stages from an injected df ------------------------------------------------------------------------------
SIZES = ((1, 1), (3, 3), (8, 16), (9, 17), (17, 33), (5, 70))
CONV_CASES = [(32, 2, 1) + s for s in SIZES] + [(32, 0, 3, 9, 17), (32, 1, 3, 17, 33), (20, 2, 3, 9, 17), (1, 2, 1, 9, 17), (1, 1, 3, 17, 33),
                                                (20, 0, 1, 5, 70)]
_id = lambda k: "c{}-nb{}-n{}-{}x{}".format(*k)


CONV_RUNS = [(k, 0) for k in CONV_CASES] + [(k, 1) for k in CONV_CASES if k[3:] in ((9, 17), (17, 33))]   # wgs 1: one workgroup, many tiles


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key, wgs", CONV_RUNS, ids=lambda v: _id(v) if isinstance(v, tuple) else f"wgs{v}")
def test_conv_stages_exact_per_stage(key, wgs, mode):
    from mobilesuperresolution_amd import packing as P
    case, df, ref = T.exact_grad_case(*key)
    net = TrainNet(case, DTYPES[mode], wgs)
    net.fwd()
    _saved_forward_is_exact(net, ref, key[0])
    nb = net.nb
    net.gs[0] = nhwc32(df).to(DEV).to(net.dtype)
    g_unused = torch.zeros(net.n, 3, 4 * net.h, 4 * net.w)
    last = (f"w{2 * nb}", f"b{2 * nb}")
    net.bwd(g_unused, P.FN_BWD_LAST)
    hold_exact("last", [("dz", net.g(1), nhwc32(ref["dz"]))] + net.grad_rows(ref["grads"], last))
    assert bool(torch.isnan(net.gs[2:].float()).all()) and net.nan_except(last)
    blocks = tuple(f"{k}{j}" for j in range(2 * nb) for k in "wb")
    net.bwd(g_unused, P.FN_BWD_BLOCKS)
    pairs = []
    if nb:
        pairs = [("dx0", net.g(net.dx0_slot()), nhwc32(ref["dx"][0])), ("dt0", net.g(2), nhwc32(ref["dt"][0]))]
    if nb > 1:
        pairs.append(("dx1", net.g(4 - net.dx0_slot()), nhwc32(ref["dx"][1])))
    hold_exact("blocks", pairs + net.grad_rows(ref["grads"], blocks))
    assert net.nan_except(last + blocks)
    net.bwd(g_unused, P.FN_BWD_ENCODER)
    hold_exact("encoder", [("de", net.g(2), nhwc32(ref["de"]))] + net.grad_rows(ref["grads"]))
    assert net.nan_except(last + blocks + ("enc_w", "enc_b"))      # the upsampler stage never ran
    assert net.conv_slab_padding_is_zero()


# ---- exact cases: the whole chain from an edge-line output gradient ------------------------------------------------------------------
UP_CASES = {"fp32": [(32, 2, 1, 8, 16), (32, 1, 3, 16, 32), (20, 2, 3, 8, 16), (1, 0, 1, 8, 16), (32, 2, 1, 1, 1), (32, 1, 3, 2, 2), (20, 1, 1, 1, 4)],
            "bf16": [(32, 2, 1, 1, 1), (32, 1, 3, 2, 1), (20, 1, 1, 1, 4), (1, 0, 3, 2, 2)]}


@pytest.mark.parametrize("wgs", (0, 1), ids=("wgs-default", "wgs-1"))
@pytest.mark.parametrize("mode, key", [(m, k) for m in DTYPES for k in UP_CASES[m]], ids=lambda v: v if isinstance(v, str) else _id(v))
def test_whole_chain_exact_from_edge_line_gradients(mode, key, wgs):
    from mobilesuperresolution_amd import packing as P
    case, gout, ref = T.exact_up_case(*key, mode == "bf16")
    net = TrainNet(case, DTYPES[mode], wgs)
    net.fwd()
    _saved_forward_is_exact(net, ref, key[0])
    net.bwd(gout, P.FN_BWD_UP)
    rows = {r[0]: r for r in net.grad_rows(ref["grads"])}
    hold_exact("upsampler", [("df", net.g(0), nhwc32(ref["df"])), rows["up_w"], rows["up_b"]])
    assert bool(torch.isnan(net.gs[1:].float()).all())
    fresh = TrainNet(case, DTYPES[mode], wgs)
    fresh.fwd()
    fresh.bwd(gout)
    pairs = [("df", fresh.g(0), nhwc32(ref["df"])), ("de", fresh.g(2), nhwc32(ref["de"]))]
    if fresh.nb:
        pairs.append(("dx0", fresh.g(fresh.dx0_slot()), nhwc32(ref["dx"][0])))
    hold_exact("whole chain", pairs + fresh.grad_rows(ref["grads"]))
    assert len(fresh.grad_rows(ref["grads"])) == len(fresh.sizes) and fresh.conv_slab_padding_is_zero()


# ---- through the module ------------------------------------------------------------------------------------------------------------------
def _module(case, mode, **attrs):
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    m = Result_Model(4, case["channel"], case["nb"], 3, hot_dtype=mode)
    m.load_state_dict(R.state_dict_of(case["p"]), strict=False)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m.to(DEV)


def _param_grads(m):
    return {k: (p.grad.detach().double().cpu() if p.grad is not None else None) for k, p in m.named_parameters()}


@pytest.mark.parametrize("mode", DTYPES)
def test_route(mode):
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    assert all(hasattr(L.lib(), s) for s in ("sr_fn_net_train_fwd", "sr_fn_net_bwd")) and L.lib().sr_abi_version() == 25
    case = R.rounded_case(20, 2, 3, 9, 17)
    m = _module(case, mode, hot_training=True)
    x = case["x"].float().unsqueeze(0).to(DEV)
    assert m.train_route_reason(x, 36, 68) is None
    y = m(x, 36, 68)
    assert m.last_route == "hip_train" and y.requires_grad and y.shape == (1, 3, 3, 36, 68) and y.dtype == torch.float32
    with torch.no_grad():
        plain = m(x, 36, 68)
        assert m.last_route == "hip" and "grad mode" in m.train_route_reason(x, 36, 68)
    assert torch.equal(y.detach(), plain)
    y.sum().backward()
    assert all((p.grad is None) == k.startswith("skip.") for k, p in m.named_parameters())

    def falls_back(word, mm=m, xx=x, size=(36, 68)):
        assert word in mm.train_route_reason(xx, *size), mm.train_route_reason(xx, *size)
        out = mm(xx, *size)
        assert mm.last_route == "aten" and out.requires_grad

    falls_back("(4H, 4W)", size=(37, 68))
    falls_back("requires grad", xx=x.clone().requires_grad_(True))
    falls_back("CPU", mm=_module(case, mode, hot_training=True).cpu(), xx=x.cpu())
    falls_back("hot_training", mm=_module(case, mode))
    falls_back("aten_forward", mm=_module(case, mode, hot_training=True, aten_forward=True))
    frozen = _module(case, mode, hot_training=True)
    frozen.shuf[0].bias.requires_grad_(False)
    falls_back("frozen", mm=frozen)
    hooked = _module(case, mode, hot_training=True)
    hooked.encoder.register_forward_hook(lambda *a: None)
    falls_back("hook", mm=hooked)
    wide = Result_Model(4, 33, 1, 3, hot_dtype=mode).to(DEV)
    wide.hot_training = True
    falls_back("channels", mm=wide)
    k5 = Result_Model(4, 8, 1, 5, hot_dtype=mode).to(DEV)
    k5.hot_training = True
    falls_back("kernel", mm=k5)


ROUNDED = [(32, 2, 3, 17, 33), (20, 1, 1, 9, 40), (1, 2, 1, 9, 17)]


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", ROUNDED, ids=_id)
def test_rounded(key, mode):
    case = R.rounded_case(*key)
    n, h, w = key[2:]
    m = _module(case, mode, hot_training=True)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    p = R.effective(sd, case["nb"])
    x = case["x"].float()
    gout = torch.randn(n, 3, 4 * h, 4 * w, generator=torch.Generator().manual_seed(11)).double()
    ref = T.param_grads(sd, case["nb"], T.backward(x, p, gout)["grads"])

    def run(mm):
        mm.zero_grad()
        (mm(x.to(DEV).unsqueeze(0), 4 * h, 4 * w)[0] * gout.float().to(DEV)).sum().backward()
        return _param_grads(mm)

    if mode == "fp32":
        tf32 = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
        torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
        try:
            yard = run(_module(case, mode))
        finally:
            torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = tf32
    else:
        yard = T.param_grads(sd, case["nb"], T.backward(x, p, gout, rnd=R.bf16_round)["grads"])
    got = run(m)
    assert m.last_route == "hip_train"
    hold_rounded("frame net train", _id(key), mode, [(k, got[k], ref[k], rel_max(yard[k], ref[k])) for k in ref])


@pytest.mark.parametrize("tag", ("a", "b"))
def test_g21_gradients_through_the_module_fp32(tag):
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    g21 = np.load(GOLD)
    m = Result_Model(*[int(v) for v in g21[f"{tag}/args"]], hot_dtype="fp32")
    m.load_state_dict({str(k): torch.from_numpy(g21[f"{tag}/p/{k}"]) for k in g21[f"{tag}/keys"]}, strict=True)
    m = m.to(DEV)
    m.hot_training = True
    y = m(torch.from_numpy(g21[f"{tag}/x"]).to(DEV), 48, 80)
    assert m.last_route == "hip_train"
    torch.testing.assert_close(y.detach().cpu(), torch.from_numpy(g21[f"{tag}/y48x80"]), rtol=1e-4, atol=1e-5)
    y.sum().backward()
    for k, prm in m.named_parameters():
        want = torch.from_numpy(g21[f"{tag}/g/{k}"])
        if k.startswith("skip."):
            assert prm.grad is None
            continue
        err = rel_max(prm.grad.cpu(), want)
        print(f"frame net train G21 | {tag} | {k} | rel max-abs {err:.3e}")
        assert err <= 1e-4, k


@pytest.mark.parametrize("mode", DTYPES)
def test_two_equal_passes_give_equal_gradients(mode):
    case = R.rounded_case(32, 2, 3, 20, 28)
    m = _module(case, mode, hot_training=True)
    x = case["x"].float().unsqueeze(0).to(DEV)
    runs = []
    for _ in range(2):
        m.zero_grad()
        m(x, 80, 112).square().sum().backward()
        runs.append(_param_grads(m))
    assert m.last_route == "hip_train"
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0] if runs[0][k] is not None)


@pytest.mark.parametrize("mode", DTYPES)
def test_three_real_steps(mode):
    from mobilesuperresolution_amd import training
    case = R.rounded_case(32, 2, 6, 16, 16)
    x = case["x"].float().view(2, 3, 3, 16, 16).to(DEV)
    hr = torch.rand(2, 3, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(DEV)

    def train(hot, double=False):
        m = _module(case, mode, hot_training=hot)
        m = m.double() if double else m
        start = {k: v.detach().clone() for k, v in m.named_parameters()}
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        crit, losses = training.L1_Charbonnier_loss(), []
        for _ in range(3):
            opt.zero_grad()
            loss = crit(m(x.double() if double else x, 64, 64), hr.double() if double else hr)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        assert m.last_route == ("hip_train" if hot else "aten")
        return {k: (v.detach() - start[k]).double().cpu() for k, v in m.named_parameters() if not k.startswith("skip.")}, losses

    hip, hip_loss = train(True)
    aten, aten_loss = train(False)
    print(f"frame net train steps | {mode} | loss hip {hip_loss} | aten {aten_loss}")
    if mode == "bf16":
        assert hip_loss[2] < hip_loss[0] and aten_loss[2] < aten_loss[0]
        return
    ref, _ = train(False, double=True)
    flat = lambda d: torch.cat([d[k].reshape(-1) for k in sorted(d)])
    yard, err = rel_max(flat(aten), flat(ref)), rel_max(flat(hip), flat(ref))
    print(f"frame net train steps | fp32 | parameter change | yardstick {yard:.3e} | hip {err:.3e} | ratio {err / yard:.2f}")
    assert err <= bound("fp32", yard)


@pytest.mark.parametrize("mode", DTYPES)
def test_refusals_leave_every_buffer_untouched(mode):
    from mobilesuperresolution_amd import _lib as L
    net = TrainNet(R.exact_case(32, 1, 1, 3, 3), DTYPES[mode])
    lib, code = L.lib(), L.DTYPE_CODE[DTYPES[mode]]
    g = torch.zeros(1, 3, 12, 12, device=DEV)
    ptr = lambda t: t.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t.float()).all()) for t in (net.acts, net.ts, net.out, net.gs, net.parts, net.grads)) and bool((net.masks == -1).all())

    def fwd(n=1, h=3, w=3, nb=1, dtype=code, stages=15, blob=ptr(net.blob), ts=ptr(net.ts), out_is=net.out.stride(0)):
        return lib.sr_fn_net_train_fwd(ptr(net.x), blob, net.offs, ptr(net.head), ptr(net.acts), ts, ptr(net.masks), ptr(net.out), out_is, nb,
                                       n, h, w, dtype, stages, L.stream_ptr())

    def bwd(n=1, h=3, w=3, nb=1, dtype=code, stages=15, blob=ptr(net.bwd_blob), ts=ptr(net.ts), wgs=net.wgs, c=32, g_is=g.stride(0)):
        return lib.sr_fn_net_bwd(ptr(net.x), ptr(g), g_is, blob, ptr(net.acts), ts, ptr(net.masks), ptr(net.gs), ptr(net.parts), wgs,
                                 ptr(net.grads), c, nb, n, h, w, dtype, stages, L.stream_ptr())

    geometry = (dict(n=65536), dict(h=8193), dict(w=8193), dict(dtype=7), dict(nb=1025))
    for kw in geometry:
        assert fwd(**kw) == -1 and bwd(**kw) == -1 and untouched(), kw
    for kw in (dict(blob=None), dict(ts=None), dict(stages=0), dict(stages=16), dict(nb=-1), dict(n=0)):
        assert fwd(**kw) == -2 and bwd(**kw) == -2 and untouched(), kw
    assert fwd(out_is=100) == -2 and untouched()
    for kw in (dict(wgs=0), dict(wgs=1025), dict(c=0), dict(c=33), dict(g_is=100)):
        assert bwd(**kw) == -2 and untouched(), kw
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(net.out).any()) and not bool(torch.isnan(net.grads).any())
