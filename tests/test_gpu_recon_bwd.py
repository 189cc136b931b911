"""The HIP backward of BasicVSR_origin's reconstruction (csrc/vsr_recon_bwd.h, sr_c64_recon_bwd / sr_c64_recon_reduce) against the
float64 reference of tests/recon_bwd_ref.py, stage by stage through `stages`, and the opt-in `hot_training` route of the model.

  exact    dyadic cases on which every sum is exact (recon_bwd_ref.check_exact): bit for bit in fp32 and bf16
  rounded  random data: kernel distance from float64 within parity_kit.bound of the emulation's own distance
  model    BasicVSR_origin(64, 2) / (40, 1) on 1 x 3 x 3 x 18 x 20 with given flows against a float64 ATen restatement
"""
import ctypes
import functools

import pytest
import torch

from tests import recon_bwd_ref as B
from tests import wide_model_ref as TT
from tests.parity_kit import bound, hold_exact, hold_rounded, rel_max

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16")
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
_gid = lambda g: "x".join(str(v) for v in g)
_IMG = {16: ("hr", "hr", "d_hr"), 8: ("up2", None, "d_up2"), 4: ("up1", "up2", "d_up1"), 2: ("fused", "up1", "d_fused")}
_GIN = {8: "d_hr", 4: "d_up2", 2: "d_up1", 1: "d_fused"}


def _nhwc(t, dt):
    """(N, C, H, W) -> (N, H, W, 64) on the GPU in the hot dtype, channels >= C zero"""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, 64, dtype=dt)
    out[..., :c] = t.permute(0, 2, 3, 1).to(dt)
    return out.cuda()


def _nchw(t, c):
    return t[..., :c].permute(0, 3, 1, 2).double().cpu()


def _default_wgs():
    from mobilesuperresolution_amd.models import basicvsr_arch_origin as O
    return O._RECON_BWD_WGS


def run_stage(case, mode, wgs=None, g_parent=False):
    """one stage of sr_c64_recon_bwd on a recon_bwd_ref case, then the slab reduction: dict(dx, dW, db, pad) -- pad = channels >= the
    real count of the stored gradient image(s), which must be exactly zero.  g_parent: the cotangent of stage 16 goes in as slot 1 of a
    NaN-filled (n, 3, 3, 4h, 4w) parent, with that view's batch stride"""
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd import packing as P
    st, f, dt = case["stage"], case["f"], DT[mode]
    wgs = wgs or _default_wgs()
    n = case["x"].shape[0]
    h, w = (case["x"].shape[2] // 4, case["x"].shape[3] // 4) if st in (16, 8) else \
        (case["x"].shape[2] // 2, case["x"].shape[3] // 2) if st == 4 else case["x"].shape[2:]
    t = P.c64_recon_bwd_tables(f)
    shapes = dict(P.c64_recon_shapes(f))
    wname = B.NAMES[st] + ".weight"
    src = torch.cat([(case["w"].reshape(-1).float() if k == wname else torch.zeros(int(torch.Size(s).numel()))) for k, s in shapes.items()]
                    + [torch.zeros(1)])
    blob = src[torch.from_numpy(t["pack"])].to(dt).cuda()
    boff = (ctypes.c_long * 6)(*t["boff"])
    nan = lambda *s: torch.full(s, float("nan"), dtype=dt, device="cuda")
    img = dict(fused=nan(n, h, w, 64), up1=nan(n, 2 * h, 2 * w, 64), up2=nan(n, 4 * h, 4 * w, 64), hr=nan(n, 4 * h, 4 * w, 64),
               d_fused=nan(n, h, w, 64), d_up1=nan(n, 2 * h, 2 * w, 64), d_up2=nan(n, 4 * h, 4 * w, 64), d_hr=nan(n, 4 * h, 4 * w, 64),
               fb=nan(n, h, w, 64), ff=nan(n, h, w, 64), dfb=nan(n, h, w, 64), dff=nan(n, h, w, 64))
    g = torch.zeros(n, 3, 4 * h, 4 * w, device="cuda")
    if st == 16:
        g = case["gin"].float().cuda().contiguous()
        if g_parent:
            parent = torch.full((n, 3, 3, 4 * h, 4 * w), float("nan"), device="cuda")
            parent[:, 1] = g
            g = parent[:, 1]
            assert g.stride(0) == 3 * 48 * h * w
        img["hr"] = _nhwc(case["x"], dt)
    elif st == 1:
        img["fb"], img["ff"] = _nhwc(case["x"][:, :f], dt), _nhwc(case["x"][:, f:], dt)
        img["fused"], img["d_fused"] = _nhwc(case["a"], dt), _nhwc(case["gin"], dt)
    else:
        xk, ak, _ = _IMG[st]
        img[xk] = _nhwc(case["x"], dt)
        if ak:
            img[ak] = _nhwc(case["a"], dt)
        img[_GIN[st]] = _nhwc(case["gin"], dt)
    lib = L.lib()
    parts = torch.zeros(wgs * lib.sr_c64_recon_bwd_slab(), device="cuda")
    table = torch.from_numpy(t["reduce"]).cuda()
    grads = torch.full((table.numel(),), float("nan"), device="cuda")
    sp = L.stream_ptr(torch.device("cuda"))
    p = lambda k: img[k].data_ptr()
    L.launch("sr_c64_recon_bwd", lib.sr_c64_recon_bwd, p("fb"), p("ff"), p("fused"), p("up1"), p("up2"), p("hr"), g.data_ptr(),
             g.stride(0), blob.data_ptr(), boff, p("d_hr"), p("d_up2"), p("d_up1"), p("d_fused"), p("dfb"), p("dff"), parts.data_ptr(),
             wgs, n, h, w, L.DTYPE_CODE[dt], st, sp)
    L.launch("sr_c64_recon_reduce", lib.sr_c64_recon_reduce, parts.data_ptr(), wgs, table.data_ptr(), table.numel(), grads.data_ptr(),
             0, n, h, w, sp)
    torch.cuda.synchronize()
    o, sl = 0, {}
    for k, s in shapes.items():
        sl[k] = grads[o:o + torch.Size(s).numel()].view(s).double().cpu()
        o += torch.Size(s).numel()
    if st == 1:
        dx = torch.cat([_nchw(img["dfb"], f), _nchw(img["dff"], f)], 1)
        pad = torch.cat([img["dfb"][..., f:], img["dff"][..., f:]], -1).float().cpu()
    else:
        real = f if st in (4, 2) else 64
        dx, pad = _nchw(img[_IMG[st][2]], real), img[_IMG[st][2]][..., real:].float().cpu()
    return dict(dx=dx, dW=sl[wname], db=sl[B.NAMES[st] + ".bias"], pad=pad)


def _hold_exact(case, mode, tag, wgs=None):
    exp = B.exact_ref(case, mode)
    got = run_stage(case, mode, wgs)
    hold_exact(tag, [(k, got[k], exp[k]) for k in ("dx", "dW", "db")] + [("pad", got["pad"], torch.zeros_like(got["pad"]))])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stage", B.STAGES)
@pytest.mark.parametrize("geom", B.EXACT, ids=_gid)
def test_stage_exact(geom, stage, mode):
    f, n, h, w = geom
    _hold_exact(B.stage_case(stage, f, n, h, w, mode), mode, (geom, stage, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stage", (16, 8, 4, 2))
def test_tap_coverage(stage, mode):
    """every (tap, sub-pixel q) pair carries a weight of its own"""
    _hold_exact(B.tap_case(stage, mode), mode, ("taps", stage, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wgs", [1, 3, 5, None])
@pytest.mark.parametrize("stage", B.STAGES)
def test_slab_walk(stage, wgs, mode):
    """fewer workgroups than tiles (each walks several), and the default count (more workgroups than tiles at the low resolutions)"""
    _hold_exact(B.stage_case(stage, 64, 2, 9, 21, mode), mode, ("walk", stage, wgs, mode), wgs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f", [64, 40])
def test_rounded(f, mode):
    """every output tensor of every stage on 9 x 21: the kernel's distance from float64 against the emulation's own"""
    rows = []
    for stage in B.STAGES:
        case = B.rounded_case(stage, f, 1, 9, 21, mode)
        ref, yard = B.rounded_reference(case, mode)
        got = run_stage(case, mode)
        assert bool((got["pad"] == 0).all()), stage
        rows += [(f"{B.NAMES[stage]} {k}", got[k], ref[k], yard[k]) for k in ("dx", "dW", "db")]
    hold_rounded("recon bwd parity", f"F={f} {mode}", mode, rows)


def test_two_equal_calls_are_bit_identical():
    case = B.rounded_case(4, 64, 2, 9, 21, "bf16")
    a, b = run_stage(case, "bf16"), run_stage(case, "bf16")
    assert all(torch.equal(a[k], b[k]) for k in ("dx", "dW", "db"))


# ================================================================================================================================
# model level
# ================================================================================================================================
_CLIP = (1, 3, 18, 20)
_RECON = tuple(f"{l}.{p}" for l in ("fusion", "upconv1", "upconv2", "conv_hr", "conv_last") for p in ("weight", "bias"))


@functools.lru_cache(maxsize=None)
def _clip():
    g = torch.Generator().manual_seed(12)
    b, n, h, w = _CLIP
    x = torch.rand(b, n, 3, h, w, generator=g).cuda()
    mv = (1.5 * torch.randn(b, n, 2, h, w, generator=g)).cuda()
    target = torch.rand(b, n, 3, 4 * h, 4 * w, generator=g).cuda()
    return x, mv[:, 1:], -mv[:, 1:], target


def _new_model(f, nb, dtype):
    from mobilesuperresolution_amd.models import BasicVSR_origin
    torch.manual_seed(11)
    return BasicVSR_origin(f, nb, hot_dtype=dtype).cuda()


@functools.lru_cache(maxsize=None)
def _aten_refs(f, nb):
    """{float64, float32}: (output, {name: gradient}) of the ATen restatement on the seeded model's parameters"""
    model = _new_model(f, nb, "fp32")
    x, ff, fb, target = _clip()
    res = {}
    for dt in (torch.float64, torch.float32):
        p = {k: v.detach().to(dt).requires_grad_(True) for k, v in model.state_dict().items() if not k.startswith("spynet.")}
        out = TT._aten_model("origin", p, x.to(dt), ff.to(dt), fb.to(dt), nb, f, (4 * _CLIP[2], 4 * _CLIP[3]))
        TT._charbonnier(out, target.to(dt)).backward()
        grads = {tr + "_trunk": torch.cat([p[k].grad.reshape(-1) for k in p if k.startswith(tr + "_trunk.")]) for tr in ("backward", "forward")}
        grads.update({k: p[k].grad for k in _RECON})
        res[dt] = (out.detach(), grads)
    return res


def _step(model):
    """forward + Charbonnier + backward: (output, {name: gradient}, the C calls by name)"""
    from mobilesuperresolution_amd import _lib as L
    x, ff, fb, target = _clip()
    real, log = L.launch, []

    def counting(name, fn, *a):
        log.append(name)
        return real(name, fn, *a)
    model.zero_grad(set_to_none=True)
    L.launch = counting
    try:
        out = model(x, 4 * _CLIP[2], 4 * _CLIP[3], flows=(ff, fb))
        TT._charbonnier(out, target).backward()
    finally:
        L.launch = real
    grads = {"backward_trunk": model.backward_trunk.flat.grad.clone(), "forward_trunk": model.forward_trunk.flat.grad.clone()}
    sd = dict(model.named_parameters())
    grads.update({k: sd[k].grad.clone() for k in _RECON})
    return out.detach(), grads, log


def _hot_log_ok(log):
    n = _CLIP[1]
    return (log.count("sr_c64_recon_fwd"), log.count("sr_c64_recon_bwd"), log.count("sr_c64_recon_reduce"), log.count("sr_pixel_shuffle")) \
        == (n, n, n, 0)


@pytest.mark.parametrize("f,nb", [(64, 2), (40, 1)])
def test_model_fp32_against_float64(f, nb):
    """the output and every parameter's gradient (both trunks, the ten reconstruction tensors) within 8 x the fp32 ATen
    restatement's own distance from the float64 one; set_wide_training alone keeps the ATen reconstruction"""
    from mobilesuperresolution_amd.models import set_wide_training
    refs = _aten_refs(f, nb)
    (o64, g64), (o32, g32) = refs[torch.float64], refs[torch.float32]
    hot = _new_model(f, nb, "fp32")
    hot.hot_training = True
    out, grads, log = _step(hot)
    assert _hot_log_ok(log), log
    bad = []
    for name, got, r64, r32 in [("out", out, o64, o32)] + [(k, grads[k], g64[k], g32[k]) for k in g64]:
        e, err = rel_max(r32, r64), rel_max(got, r64)
        print(f"origin model parity | F={f} | hot_training | {name} | yardstick {e:.2e} | kernel {err:.2e} | bound {bound('fp32', e):.2e}")
        if not (bool(got.isfinite().all()) and err <= bound("fp32", e)):
            bad.append((name, err, e))
    assert not bad, bad
    wide = _new_model(f, nb, "fp32")
    assert len(set_wide_training(wide)) == 2 and wide.hot_training is False
    _, _, wlog = _step(wide)
    assert "sr_c64_recon_bwd" not in wlog and "sr_c64_recon_fwd" not in wlog and "sr_pixel_shuffle" in wlog, wlog
    with pytest.raises(NotImplementedError, match="hot_training"):
        _step(_new_model(f, nb, "fp32"))


@pytest.mark.parametrize("f,nb", [(64, 2), (40, 1)])
def test_model_bf16_steps_are_bit_identical(f, nb):
    """two equal steps give bit-identical outputs and gradients.  The distances of the bf16 step from float64 are held, per tensor
    and at b in {2, 3}, by tests/test_gpu_wide_batch.py::test_step_against_the_composed_reference against the composed bf16 emulation
    of tests/wide_model_ref.py"""
    hot = _new_model(f, nb, "bf16")
    hot.hot_training = True
    out, grads, log = _step(hot)
    assert _hot_log_ok(log), log
    out2, grads2, log2 = _step(hot)
    assert log2 == log and torch.equal(out, out2)
    for k in grads:
        assert bool(grads[k].isfinite().all()) and float(grads[k].abs().max()) > 0, k
        assert torch.equal(grads[k], grads2[k]), k


def test_model_adam_step_changes_every_parameter():
    from mobilesuperresolution_amd import training
    model = _new_model(40, 1, "bf16")
    model.hot_training = True
    params = [p for k, p in model.named_parameters() if not k.startswith("spynet.")]
    before = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=1e-3)
    x, ff, fb, target = _clip()
    loss = training.L1_Charbonnier_loss()(model(x, 72, 80, flows=(ff, fb)), target)
    opt.zero_grad()
    loss.backward()
    opt.step()
    for p, b in zip(params, before):
        assert bool(p.isfinite().all()) and not torch.equal(p.detach(), b)


@functools.lru_cache(maxsize=None)
def _clips(b):
    """(x, target) of b clips, each with its own data; b = 1 is _clip()'s"""
    if b == 1:
        x, _, _, target = _clip()
        return x, target
    g = torch.Generator().manual_seed(12 + b)
    _, n, h, w = _CLIP
    return torch.rand(b, n, 3, h, w, generator=g).cuda(), torch.rand(b, n, 3, 4 * h, 4 * w, generator=g).cuda()


@pytest.mark.parametrize("b", [1, 2, 3])
def test_state_gradients_land_in_their_halves(b):
    """dsteps of b 3-frame clips: frame i's two state gradients go to step n - 1 - i, first half, and step i, second half, clip by
    clip.  Checked against the ATen route's gradients at the trunk outputs (fp32; channels >= F exactly zero).  Bound 2e-4 of the
    largest element: five layers of fp32 sums of up to 9 x 64 = 576 terms each, 5 x 576 x 2^-24 = 1.7e-4, on both sides of the
    comparison -- layer depth and term count, whatever b"""
    from mobilesuperresolution_amd.models import basicvsr_arch_origin as O
    f, (_, n, h, w) = 40, _CLIP
    model = _new_model(f, 1, "fp32")
    g = torch.Generator().manual_seed(21)
    steps = [torch.zeros(2 * b, h, w, 64).cuda() for _ in range(n)]
    for s in steps:
        s[..., :f] = torch.randn(2 * b, h, w, f, generator=g).cuda()
        s.requires_grad_(True)
    x, target = _clips(b)
    out = O._ReconTrainFunction.apply(model, x, *model._recon_params(), *steps)
    TT._charbonnier(out, target).backward()
    feats = [s.detach().permute(0, 3, 1, 2)[:, :f].contiguous().requires_grad_(True) for s in steps]
    p = {k: v.detach() for k, v in model.state_dict().items()}
    outs = []
    for i in range(n):
        o = B.chain_forward(p, feats[n - 1 - i][:b], feats[i][b:], x[:, i])[0]
        outs.append(o)
    TT._charbonnier(torch.stack(outs, 1), target).backward()
    assert rel_max(out.detach(), torch.stack(outs, 1).detach()) < 1e-5
    for k in range(n):
        got = steps[k].grad
        assert bool((got[..., f:] == 0).all()), k
        exp = feats[k].grad.permute(0, 2, 3, 1)
        for name, lo in (("first half", 0), ("second half", b)):
            for clip in range(b):
                e = rel_max(got[lo + clip][..., :f], exp[lo + clip])
                print(f"origin state gradients | b={b} | step {k} | {name} | clip {clip} | distance {e:.2e}")
                assert e < 2e-4, (k, name, clip, e)
