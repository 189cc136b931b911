"""The HIP training route of the multi-frame video network on the MI355X: sr_mf_net_train_fwd / sr_mf_net_bwd (csrc/multi_frame.h,
csrc/multi_frame_bwd.h, csrc/result_block.h) and models/naive_multi_model_easy.py with hot_training, both hot dtypes, against
tests/multi_frame_train_ref.py (float64) and fixture G22.  Outputs, saved images, scratch, slabs and gradients are NaN-filled (masks:
-1) before every call; every measured ratio is printed.

  route           hot_training sends a graph-recording call down "hip_train", bit-identical to the no_grad HIP output, .grad on exactly
                  the trained parameters; the default and every excluded condition keep "aten"
  exact cases     per stage through the `stages` mask, torch.equal to the float64 reference, from a sparse integer output gradient
                  (the un-shuffle is a permutation, so dD is an integer image in both dtypes and no stage needs the rounded cases to
                  stand in for it): tile-edge sizes, C in {32, 20, 1}, 1..3 blocks, every (B, N), all flow kinds, default and 1 workgroup
  the warp kernel converging flows (four outputs per source), far flows (window past radius 7 and past the image), clip independence
  rounded cases   fp32 within 8 x the fp32 ATen route's distance from float64 (same device, TF32 off), bf16 within 4 x the
                  rounding-point reference's (tests/parity_kit.bound)
  G22, determinism, three real optimiser steps with SPyNet's flows, deepcopy / pickle, refusals
"""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from tests import multi_frame_ref as R
from tests import multi_frame_train_ref as T
from tests.parity_kit import bound, hold_exact, hold_rounded, rel_max

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_multi_frame.npz")
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """drop the device-resident pack indices and hand the free blocks back"""
    yield
    import gc
    from mobilesuperresolution_amd import hotpath as HP
    HP._mf_pack_index.cache_clear()
    HP._mf_bwd_pack_index.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def nhwc(t, ch=32):
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, ch, dtype=torch.float64)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


def mask_bits(t):
    """(N, C, H, W) -> (N, H, W) int64: bit c = t[c] > 0"""
    return ((t > 0).long() << torch.arange(t.shape[1]).view(1, -1, 1, 1)).sum(1)


class TrainNet:
    """a parameter set packed for the two entry points; everything they write starts as NaN"""

    def __init__(self, case, dtype, wgs=0, clips=None):
        from mobilesuperresolution_amd import hotpath as HP, packing as P
        p = case["p"]
        dev = lambda t: t.float().to(DEV)
        self.nb, self.c, self.dtype = case["nb"], case["channel"], dtype
        x, flows = case["x"], case["flows"]
        if clips is not None:
            x, flows = x[clips], flows[clips]
        self.B, self.N = x.shape[:2]
        self.blob, self.bwd_blob = HP.mf_pack_train([tuple(dev(t) for t in bk) for bk in p["blocks"]], dev(p["dec_w"]), dev(p["dec_b"]), dtype)
        self.head = HP.fn_pack_encoder(dev(p["enc_w"]), dev(p["enc_b"]), dtype)
        self.x = x.float().reshape(-1, *x.shape[2:]).to(DEV).contiguous()
        self.flows = flows.float().to(DEV).contiguous() if self.N > 1 else None
        self.bound = self.flows.abs().amax().reshape(1) if self.N > 1 else None
        n, _, h, w = self.x.shape
        self.n, self.h, self.w = n, h, w
        full = lambda shape, dt=dtype: torch.full(shape, NAN, dtype=dt, device=DEV)
        self.acts, self.ts, self.wf = full((self.nb + 1, n, h, w, 32)), full((self.nb, n, h, w, 32)), full((2, n, h, w, 32))
        self.masks = torch.full((self.nb, n, h, w), -1, dtype=torch.int32, device=DEV)
        self.out = full((n, 3, 4 * h, 4 * w), torch.float32)
        self.gs = full((6, n, h, w, 32))
        self.wgs = wgs or HP.fn_bwd_wgs(n, h, w)
        self.parts = full((P.mf_bwd_parts(self.nb, self.wgs),), torch.float32)
        self.sizes = P.mf_grad_sizes(self.c, self.nb)
        self.grads = full((sum(self.sizes),), torch.float32)

    def fwd(self, stages=None):
        from mobilesuperresolution_amd import hotpath as HP, packing as P
        HP.mf_net_train_fwd(self.x, self.flows, self.blob, self.head, self.acts, self.ts, self.masks, self.wf, self.out, self.nb, self.B,
                            self.N, P.MF_ALL if stages is None else stages)
        torch.cuda.synchronize()

    def bwd(self, g, stages=None):
        from mobilesuperresolution_amd import hotpath as HP, packing as P
        g = g.float().to(DEV).contiguous()
        HP.mf_net_bwd(self.x, self.flows, self.bound, g, self.bwd_blob, self.acts, self.ts, self.masks, self.wf, self.gs, self.parts,
                      self.wgs, self.grads, self.c, self.nb, self.B, self.N, P.MF_BWD_ALL if stages is None else stages)
        torch.cuda.synchronize()

    def g(self, i):
        return self.gs[i].double().cpu()

    def dD(self):
        return self.gs[4:].reshape(-1)[:self.n * self.h * self.w * 48].view(self.n, self.h, self.w, 48).double().cpu()

    def slot(self, k):
        """gs index of the dy that k blocks (counted from the tail) have produced"""
        return k % 2

    def names(self):
        return [f"blk{i}.{k}" for i in range(self.nb) for k in ("w1", "b1", "w2", "b2")] + ["dec_w", "dec_b", "enc_w", "enc_b"]

    def pieces(self):
        return dict(zip(self.names(), self.grads.cpu().split(self.sizes)))

    def grad_rows(self, ref_grads, only=None):
        got = self.pieces()
        return [(k, got[k].double().view(v.shape), v) for k, v in T.flat_grads(ref_grads) if only is None or k in only]

    def nan_except(self, names):
        return all(bool(torch.isnan(p).all()) for k, p in self.pieces().items() if k not in names)

    def conv_slab_padding_is_zero(self):
        """rows >= C of every conv slab and columns >= C of its tap tiles (the flow group: columns >= 2) are exactly zero"""
        from mobilesuperresolution_amd import packing as P
        nb = self.nb
        slabs = self.parts[:(2 * nb + 3) * self.wgs * P.FN_CONV_SLAB].view(2 * nb + 3, self.wgs, P.FN_CONV_SLAB).cpu()
        tap, row, col = np.meshgrid(np.arange(10), np.arange(32), np.arange(32), indexing="ij")
        for j in range(2 * nb + 2):
            cols = 2 if j == 2 * nb + 1 else self.c
            dead = (row >= self.c) | ((col >= cols) & (tap < 9))
            if bool(slabs[j][:, torch.from_numpy(P._acc_pos(tap[dead], row[dead], col[dead]).astype(np.int64))].any()):
                return False
        tile, row, col = np.meshgrid(np.arange(20), np.arange(32), np.arange(32), indexing="ij")
        dead = ((tile >= 10) & (row >= 16)) | ((col >= self.c) & (tile % 10 < 9))
        return not bool(slabs[2 * nb + 2][:, torch.from_numpy(P._acc_pos(tile[dead], row[dead], col[dead]).astype(np.int64))].any())


def _saved_forward_is_exact(net, ref):
    fw = ref["fw"]
    ys = [fw["e"]] + fw["y"]
    pairs = [(f"act{i}", net.acts[i].double(), nhwc(ys[i])) for i in range(net.nb + 1)]
    pairs += [(f"t{i}", net.ts[i].double(), nhwc(fw["t"][i])) for i in range(net.nb)]
    pairs += [(f"mask{i}", net.masks[i].long() & 0xFFFFFFFF, mask_bits(fw["t"][i])) for i in range(net.nb)]
    pairs += [("warp", net.wf[0].double(), nhwc(fw["warp"])), ("flow", net.wf[1].double(), nhwc(fw["flow"])),
              ("out", net.out.double(), fw["out"])]
    hold_exact("saved forward", pairs)


# ---- exact cases, stage by stage ----------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (3, 3), (8, 16), (9, 17), (17, 33), (5, 70))
_id = lambda k: "c{}-nb{}-b{}-n{}-{}x{}-{}".format(*k)
# (channel, nb, B, N, h, w, flow kind): every size at C = 32 with (B, N) = (1, 3); then the other widths, block counts, (B, N) and kinds
CASES = [(32, 2, 1, 3) + s + ("int",) for s in SIZES] + [
    (32, 1, 1, 1, 9, 17, "zero"), (32, 1, 2, 1, 8, 16, "zero"), (32, 3, 2, 3, 9, 17, "int"), (20, 2, 2, 3, 9, 17, "quarter"),
    (1, 2, 1, 3, 9, 17, "int"), (20, 1, 1, 3, 17, 33, "far"), (32, 2, 1, 3, 17, 33, "quarter"), (20, 3, 1, 3, 9, 17, "inward"),
    (1, 1, 2, 3, 17, 33, "far"), (20, 1, 2, 3, 5, 70, "zero"), (32, 1, 1, 3, 9, 17, "far")]
RUNS = [(k, 0) for k in CASES] + [(k, 1) for k in CASES if k[4:6] in ((9, 17), (17, 33))]      # wgs 1: one workgroup walks every tile


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key, wgs", RUNS, ids=lambda v: _id(v) if isinstance(v, tuple) else f"wgs{v}")
def test_every_stage_exact(key, wgs, mode):
    from mobilesuperresolution_amd import packing as P
    case, gout, ref = T.exact_grad_case(*key, mode == "bf16")
    net = TrainNet(case, DTYPES[mode], wgs)
    net.fwd()
    _saved_forward_is_exact(net, ref)
    nb, gr = net.nb, ref["grads"]
    isnan = lambda *slots: all(bool(torch.isnan(net.gs[s].float()).all()) for s in slots)
    done = ("dec_w", "dec_b")
    net.bwd(gout, P.MF_BWD_TAIL)
    hold_exact("tail", [("dD", net.dD(), nhwc(ref["dD"], 48)), ("dy", net.g(0), nhwc(ref["dy"]))] + net.grad_rows(gr, done))
    assert isnan(1, 2, 3) and net.nan_except(done)
    net.bwd(gout, P.MF_BWD_BLOCKS)
    if nb > 1:
        done += tuple(f"blk{i}.{k}" for i in range(1, nb) for k in ("w1", "b1", "w2", "b2"))
        pairs = [(f"dx{i}", net.g(net.slot(nb - i)), nhwc(ref["dx"][i])) for i in (1, 2) if i < nb]
        hold_exact("blocks", pairs + [("dt1", net.g(2), nhwc(ref["dt"][1]))] + net.grad_rows(gr, done))
    assert isnan(3) and net.nan_except(done)
    net.bwd(gout, P.MF_BWD_FIRST)
    done += tuple(f"blk0.{k}" for k in ("w1", "b1", "w2", "b2"))
    hold_exact("first", [("dt0", net.g(2), nhwc(ref["dt"][0])), ("direct", net.g(net.slot(nb)), nhwc(ref["direct"])),
                         ("dwarp", net.g(3), nhwc(ref["dwarp"]))] + net.grad_rows(gr, done))
    assert net.nan_except(done)
    net.bwd(gout, P.MF_BWD_WARP)
    hold_exact("warp", [("de", net.g(2), nhwc(ref["de"])), ("dwarp", net.g(3), nhwc(ref["dwarp"]))])
    assert net.nan_except(done)
    net.bwd(gout, P.MF_BWD_ENCODER)
    hold_exact("encoder", net.grad_rows(gr))
    assert net.conv_slab_padding_is_zero()
    fresh = TrainNet(case, DTYPES[mode], wgs)                             # and the whole chain in one call
    fresh.fwd()
    fresh.bwd(gout)
    hold_exact("whole chain", [("de", fresh.g(2), nhwc(ref["de"]))] + fresh.grad_rows(gr))
    assert len(fresh.grad_rows(gr)) == len(fresh.sizes)


# ---- the warp kernel on its own stage ---------------------------------------------------------------------------------------------------
def _warp_stage(case, mode, direct, dwarp, flows=None):
    """the WARP stage alone on injected gradient images -> de"""
    from mobilesuperresolution_amd import packing as P
    if flows is not None:
        case = dict(case, flows=flows)
    net = TrainNet(case, DTYPES[mode])
    net.gs[net.slot(net.nb)] = nhwc(direct).to(DEV).to(net.dtype)
    net.gs[3] = nhwc(dwarp).to(DEV).to(net.dtype)
    net.bwd(torch.zeros(net.n, 3, 4 * net.h, 4 * net.w), P.MF_BWD_WARP)
    return net.g(2)


def _ref_de(direct, dwarp, flows, b, n):
    c, h, w = direct.shape[1:]
    de = direct.view(b, n, c, h, w).clone()
    dwv = dwarp.view(b, n, c, h, w)
    de[:, 0] += dwv[:, 0]
    if n > 1:
        de[:, :-1] += T.warp_t(dwv[:, 1:].reshape(-1, c, h, w), flows.reshape(-1, 2, h, w)).view(b, n - 1, c, h, w)
    return de.view(b * n, c, h, w)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("kind, h, w", (("converging", 17, 33), ("converging", 5, 65), ("far", 17, 33), ("far", 40, 24), ("quarter", 17, 33),
                                        ("int", 9, 17), ("int", 1, 1), ("inward", 3, 3)))
def test_warp_backward_is_an_exact_accumulation(kind, h, w, mode):
    b, n, c = 2, 3, 20
    g = torch.Generator().manual_seed(R.seed(0, 29, 41, h, w))
    # converging flows are not settled (that would break the 2 x 2 cells): sizes whose size - 1 is a power of two keep every position exact
    flows = T.converging_flows(b, n, h, w) if kind == "converging" else R.make_flows(kind, b, n, h, w, g)
    assert bool(R.position_ok(flows, h, w).all())
    if kind == "far":
        assert float(flows.abs().max()) > 7 + max(h, w)                     # the window leaves the LDS table and the image
    direct = torch.randint(-2, 3, (b * n, c, h, w), generator=g).double()
    dwarp = torch.randint(-2, 3, (b * n, c, h, w), generator=g).double()
    want = _ref_de(direct, dwarp, flows, b, n)
    lattice = 16 if kind == "quarter" else 1                              # quarter-pixel weights are multiples of 1/16
    assert bool((want * lattice == (want * lattice).round()).all()) and torch.equal(want, want.bfloat16().double())
    if kind == "converging":
        assert float(T.warp_t(torch.ones(1, 1, h, w, dtype=torch.float64), flows[:1, 0]).max()) == 4.0
    case = dict(R.exact_case(c, 1, b, n, h, w, "zero"))
    hold_exact(f"warp {kind}", [("de", _warp_stage(case, mode, direct, dwarp, flows), nhwc(want))])


@pytest.mark.parametrize("mode", DTYPES)
def test_clip_1_gives_the_same_gradient_images_alone_and_behind_clip_0(mode):
    case = R.rounded_case(20, 2, 2, 3, 9, 17)
    gout = torch.randn(6, 3, 36, 68, generator=torch.Generator().manual_seed(8))
    both, alone = TrainNet(case, DTYPES[mode]), TrainNet(case, DTYPES[mode], clips=slice(1, 2))
    # the same window for both runs: the bound is a batch maximum, and a wider window only adds zero-weight candidates
    alone.bound = both.bound
    both.fwd(), alone.fwd()
    both.bwd(gout), alone.bwd(gout[3:])
    assert torch.equal(both.out[3:], alone.out)
    for s in range(4):
        assert torch.equal(both.gs[s][3:], alone.gs[s]), s
    assert torch.equal(both.dD()[3:], alone.dD())


# ---- through the module ------------------------------------------------------------------------------------------------------------------
def _module(case, mode, flows="case", **attrs):
    from mobilesuperresolution_amd.models.naive_multi_model_easy import Naive_model
    m = Naive_model(4, status=[[case["channel"]] * 2 + [3]] * case["nb"], hot_dtype=mode)
    m.load_state_dict(R.state_dict_of(case["p"]), strict=False)
    for k, v in attrs.items():
        setattr(m, k, v)
    m = m.to(DEV)
    if flows == "case":
        fl = case["flows"].float().to(DEV)
        m.get_flow = lambda x_: fl.to(x_.device)
    return m


def _param_grads(m):
    return {k: (p.grad.detach().double().cpu() if p.grad is not None else None) for k, p in m.named_parameters()}


def _trained(k):
    return not (k.startswith("flownet.") or k.startswith("skip.") or ".skip." in k)


@pytest.mark.parametrize("mode", DTYPES)
def test_route(mode):
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.models.naive_multi_model_easy import Naive_model
    assert all(hasattr(L.lib(), s) for s in ("sr_mf_net_train_fwd", "sr_mf_net_bwd")) and L.lib().sr_abi_version() == 25
    case = R.rounded_case(20, 2, 2, 3, 9, 17)
    m = _module(case, mode, hot_training=True)
    x = case["x"].float().to(DEV)
    assert m.train_route_reason(x) is None
    y = m(x, 36, 68)
    assert m.last_route == "hip_train" and y.requires_grad and y.shape == (2, 3, 3, 36, 68) and y.dtype == torch.float32
    with torch.no_grad():
        plain = m(x, 36, 68)
        assert m.last_route == "hip" and "grad mode" in m.train_route_reason(x)
    assert torch.equal(y.detach(), plain)
    y.sum().backward()
    assert all((p.grad is not None) == _trained(k) for k, p in m.named_parameters())
    assert all(p.grad.shape == p.shape and p.grad.dtype == torch.float32 for k, p in m.named_parameters() if _trained(k))
    default = _module(case, mode)
    out = default(x)
    assert default.hot_training is False and default.last_route == "aten" and out.requires_grad

    def falls_back(word, mm=m, xx=x):
        assert word in mm.train_route_reason(xx), mm.train_route_reason(xx)
        out = mm(xx)
        assert mm.last_route == "aten" and out.requires_grad

    falls_back("requires grad", xx=x.clone().requires_grad_(True))
    falls_back("CPU", mm=_module(case, mode, hot_training=True).cpu(), xx=x.cpu())
    falls_back("aten_forward", mm=_module(case, mode, hot_training=True, aten_forward=True))
    frozen = _module(case, mode, hot_training=True)
    frozen.body["1"].body[2].bias.requires_grad_(False)
    falls_back("frozen", mm=frozen)
    hooked = _module(case, mode, hot_training=True)
    hooked.encode.register_forward_hook(lambda *a: None)
    falls_back("hook", mm=hooked)
    skipfrozen = _module(case, mode, hot_training=True)
    skipfrozen.skip.bias.requires_grad_(False)
    skipfrozen(x)
    assert skipfrozen.last_route == "hip_train"
    wide = Naive_model(4, status=[[33, 33, 3]], hot_dtype=mode).to(DEV)
    wide.hot_training = True
    falls_back("channels", mm=wide, xx=x[:, :1])


ROUNDED = [(32, 2, 1, 3, 17, 65), (20, 1, 1, 3, 9, 33), (1, 2, 1, 3, 9, 33), (32, 3, 2, 3, 9, 33)]


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", ROUNDED, ids=lambda k: _id(k + ("rnd",)))
def test_rounded(key, mode):
    case = R.rounded_case(*key)
    b, n, h, w = key[2:]
    m = _module(case, mode, hot_training=True)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if not k.startswith("flownet.")}
    p = R.effective(sd, case["nb"])
    x, flows = case["x"].float(), case["flows"].float()                  # what the device sees
    gout = torch.randn(b * n, 3, 4 * h, 4 * w, generator=torch.Generator().manual_seed(11)).double()
    ref = T.param_grads(sd, case["nb"], T.backward(x, flows, p, gout)["grads"])

    def run(mm):
        mm.zero_grad()
        (mm(x.to(DEV)).view(b * n, 3, 4 * h, 4 * w) * gout.float().to(DEV)).sum().backward()
        return _param_grads(mm)

    if mode == "fp32":
        tf32 = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
        torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
        try:
            yard = run(_module(case, mode))
        finally:
            torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = tf32
    else:
        yard = T.param_grads(sd, case["nb"], T.backward(x, flows, p, gout, rnd=R.bf16_round)["grads"])
    got = run(m)
    assert m.last_route == "hip_train"
    hold_rounded("multi frame train", _id(key + ("rnd",)), mode, [(k, got[k], ref[k], rel_max(yard[k], ref[k])) for k in ref])


@pytest.mark.parametrize("mode", DTYPES)
def test_g22_gradients_through_the_module(mode):
    """model b of G22 (held in full): y.sum().backward() against the reference implementation's own gradients.  fp32: 1e-4 of each
    tensor's largest gradient, the fixture's fp32 noise; bf16: within 4 x the rounding-point reference's distance from them"""
    from mobilesuperresolution_amd.models.naive_multi_model_easy import Naive_model
    g22 = np.load(GOLD)
    m = Naive_model(4, status=g22["b/status"].tolist(), hot_dtype=mode)
    sd = {str(k): torch.from_numpy(g22[f"b/p/{k}"]) for k in g22["b/keys"]}
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV)
    m.hot_training = True
    x, flows = torch.from_numpy(g22["b/x"]), torch.from_numpy(g22["b/flows"])
    m.get_flow = lambda x_: flows.to(DEV)
    y = m(x.to(DEV), 48, 80)
    assert m.last_route == "hip_train"
    if mode == "fp32":
        torch.testing.assert_close(y.detach().cpu(), torch.from_numpy(g22["b/y"]), rtol=1e-4, atol=1e-5)
    y.sum().backward()
    nb = len(m.idx)
    ones = torch.ones(6, 3, 48, 80, dtype=torch.float64)
    yard = T.param_grads(sd, nb, T.backward(x, flows, R.effective(sd, nb), ones, rnd=R.bf16_round)["grads"]) if mode == "bf16" else None
    for k, prm in m.named_parameters():
        if not _trained(k):
            assert prm.grad is None, k
            continue
        want = torch.from_numpy(g22[f"b/g/{k}"])
        err = rel_max(prm.grad.cpu(), want)
        tol = 1e-4 if mode == "fp32" else bound("bf16", rel_max(yard[k], want))
        print(f"multi frame train G22 | b | {mode} | {k} | rel max-abs {err:.3e} | bound {tol:.3e}")
        assert err <= tol, k


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("flows", ("random", "converging"))
def test_two_equal_passes_give_equal_gradients(flows, mode):
    case = R.rounded_case(32, 2, 2, 3, 20, 28)
    if flows == "converging":
        case = dict(case, flows=T.converging_flows(2, 3, 20, 28))
    m = _module(case, mode, hot_training=True)
    x = case["x"].float().to(DEV)
    runs = []
    for _ in range(2):
        m.zero_grad()
        m(x).square().sum().backward()
        runs.append(_param_grads(m))
    assert m.last_route == "hip_train"
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0] if runs[0][k] is not None)
    assert sum(v is not None for v in runs[0].values()) == 4 * 2 + 6


@pytest.mark.parametrize("mode", DTYPES)
def test_three_real_steps(mode):
    """Three Charbonnier + Adam steps on a 2 x 3 x 3 x 36 x 40 clip with the flows of the real get_flow.  (SPyNet's six-level pyramid
    resizes to a multiple of 32 and halves five times, then starts from a flow of half that size: a clip of 32 px or less, 16 x 16
    included, ends at 0 x 0 and cannot pass the flownet on any route, so the clip is the next size up that is no multiple of a tile.)"""
    from mobilesuperresolution_amd import training
    H, W = 36, 40
    case = R.rounded_case(32, 2, 2, 3, H, W)
    x = case["x"].float().to(DEV)
    hr = torch.rand(2, 3, 3, 4 * H, 4 * W, generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        real = _module(case, mode, flows=None).get_flow(x)                 # the real get_flow: SPyNet as constructed, frozen
    assert real.shape == (2, 2, 2, H, W) and bool(torch.isfinite(real).all())

    def train(hot, double=False):
        m = _module(case, mode, flows=None, hot_training=hot)
        m = m.double() if double else m
        m.get_flow = lambda x_: real.to(x_.dtype) if double else real     # the same flows on every route (no gradient either way)
        start = {k: v.detach().clone() for k, v in m.named_parameters()}
        opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
        crit, losses = training.L1_Charbonnier_loss(), []
        for _ in range(3):
            opt.zero_grad()
            loss = crit(m(x.double() if double else x, 4 * H, 4 * W), hr.double() if double else hr)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        assert m.last_route == ("hip_train" if hot else "aten")
        if hot:
            given = m.__dict__.pop("get_flow")                            # a lambda does not pickle; the class's get_flow is back
            twin, back = copy.deepcopy(m), pickle.loads(pickle.dumps(m))
            assert "_mf_blobs" in m.__dict__ and "_mf_blobs" not in back.__dict__ and back.hot_training
            twin.get_flow = m.get_flow = back.get_flow = given
            assert torch.equal(twin(x), m(x)) and torch.equal(back.to(DEV)(x), m(x)) and twin.last_route == back.last_route == "hip_train"
        return {k: (v.detach() - start[k]).double().cpu() for k, v in m.named_parameters() if _trained(k)}, losses

    hip, hip_loss = train(True)
    aten, aten_loss = train(False)
    print(f"multi frame train steps | {mode} | loss hip {hip_loss} | aten {aten_loss}")
    assert hip_loss[2] < hip_loss[0] and aten_loss[2] < aten_loss[0]
    if mode == "bf16":
        return
    ref, _ = train(False, double=True)
    flat = lambda d: torch.cat([d[k].reshape(-1) for k in sorted(d)])
    yard, err = rel_max(flat(aten), flat(ref)), rel_max(flat(hip), flat(ref))
    print(f"multi frame train steps | fp32 | parameter change | yardstick {yard:.3e} | hip {err:.3e} | ratio {err / yard:.2f}")
    assert err <= bound("fp32", yard)


@pytest.mark.parametrize("mode", DTYPES)
def test_refusals_leave_every_buffer_untouched(mode):
    from mobilesuperresolution_amd import _lib as L
    net = TrainNet(R.exact_case(32, 1, 1, 2, 3, 3, "int"), DTYPES[mode])
    lib, code = L.lib(), L.DTYPE_CODE[DTYPES[mode]]
    g = torch.zeros(2, 3, 12, 12, device=DEV)
    ptr = lambda t: t.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t.float()).all()) for t in (net.acts, net.ts, net.wf, net.out, net.gs, net.parts, net.grads)) and \
            bool((net.masks == -1).all())

    def fwd(b=1, n=2, h=3, w=3, nb=1, dtype=code, stages=15, blob=ptr(net.blob), wf=ptr(net.wf), flows=ptr(net.flows)):
        return lib.sr_mf_net_train_fwd(ptr(net.x), flows, blob, ptr(net.head), ptr(net.acts), ptr(net.ts), ptr(net.masks), wf, ptr(net.out),
                                       nb, b, n, h, w, dtype, stages, L.stream_ptr())

    def bwd(b=1, n=2, h=3, w=3, nb=1, dtype=code, stages=31, blob=ptr(net.bwd_blob), wf=ptr(net.wf), flows=ptr(net.flows), wgs=net.wgs,
            c=32, fb=ptr(net.bound)):
        return lib.sr_mf_net_bwd(ptr(net.x), flows, fb, ptr(g), blob, ptr(net.acts), ptr(net.ts), ptr(net.masks), wf, ptr(net.gs),
                                 ptr(net.parts), wgs, ptr(net.grads), c, nb, b, n, h, w, dtype, stages, L.stream_ptr())

    for kw in (dict(b=65536, n=1), dict(b=256, n=256), dict(h=8193), dict(w=8193), dict(dtype=7), dict(nb=1025)):
        assert fwd(**kw) == -1 and bwd(**kw) == -1 and untouched(), kw
    for kw in (dict(blob=None), dict(wf=None), dict(flows=None), dict(stages=0), dict(nb=0), dict(n=0), dict(b=0)):
        assert fwd(**kw) == -2 and bwd(**kw) == -2 and untouched(), kw
    assert fwd(stages=16) == -2 and bwd(stages=32) == -2 and untouched()
    for kw in (dict(wgs=0), dict(wgs=1025), dict(c=0), dict(c=33), dict(fb=None)):
        assert bwd(**kw) == -2 and untouched(), kw
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(net.out).any()) and not bool(torch.isnan(net.grads).any())
