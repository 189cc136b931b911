"""The flow gradient of the 64-wide training route (ConvResidualBlocks.flow_training; csrc/conv64_bwd.h, c64_warp_dflow_kernel via
sr_c64_warp_dflow and sr_c64_trunk_bwd), fp32 and bf16, against tests/flow_grad_ref.py (plain torch, float64, CPU).

  1  the kernel alone       per element within flow_grad_ref.dflow_bound (derived there from the fp32 arithmetic, not measured): sizes
                            with a size-1 axis and pixel counts that are no multiple of 8 or 32, corners outside the image, samples
                            wholly outside (exactly 0), integer positions, strided views inside NaN-filled parents, determinism
  2  one trunk, two steps   flow.grad against the same steps with the warp in float64 on the CPU and the trunk on the plain HIP route
                            (the construction of tests/test_gpu_warp.py's _fused_run / _fused_ref, with its bounds); every other
                            gradient bit-identical to the run with the flow detached
  3  the paired route       each half's flow gradient equals the single-trunk run of that half, bit for bit
  4  refusals               flag off, one trunk of a pair off, the C entries without state / flow / dx0
  5  BasicVSR_origin        gradients at flow leaves against wide_model_ref's float64 step differentiated in the flows
  6  end to end             SPyNet's parameters receive, bit for bit, what autograd.grad gives from the leaf gradients
"""
import ctypes
import functools

import pytest
import torch

from tests import flow_grad_ref as FG
from tests import warp_ref as WR
from tests import wide_model_ref as W
from tests.parity_kit import bound, hold_exact, rel_max

pytestmark = pytest.mark.gpu

DT = FG.HOT
SIZES = ((1, 1), (1, 5), (5, 1), (7, 9), (17, 19))
_sid = lambda s: "%dx%d" % s


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_reference(n, h, w, f, mode, kind):
    """inputs, float64 reference and bound of a kernel case: computed once, shared, never written to"""
    g, state, flow = FG.kernel_case(n, h, w, f, mode, kind, 100 * h + w + 7 * n + f)
    return g, state, flow, FG.dflow_ref(g, state, flow), FG.dflow_bound(g, state, flow)


def _launch_dflow(g, state, flow, mode, dflow):
    """flow / dflow: (n, 2, h, w) views with a dense (2, h, w) block; their batch strides go to the kernel"""
    from mobilesuperresolution_amd import _lib as L
    n, _, h, w = flow.shape
    assert flow.stride()[1:] == (h * w, w, 1) and dflow.stride()[1:] == (h * w, w, 1)
    L.launch("sr_c64_warp_dflow", L.lib().sr_c64_warp_dflow, g.data_ptr(), state.data_ptr(), flow.data_ptr(), flow.stride(0),
             dflow.data_ptr(), dflow.stride(0), n, h, w, L.DTYPE_CODE[DT[mode]], L.stream_ptr())
    return dflow


def _kernel(g, state, flow, mode):
    out = torch.full(flow.shape, float("nan"), device="cuda")
    return _launch_dflow(g.to(DT[mode]).cuda(), state.to(DT[mode]).cuda(), flow.cuda(), mode, out).cpu()


def _hold_elements(tag, got, ref, tol):
    """per element: |got - ref| <= tol; prints the largest ratio"""
    assert got.shape == ref.shape and bool(got.isfinite().all()), tag
    err = (got.double() - ref).abs()
    live = tol > 0
    ratio = float((err[live] / tol[live]).max()) if bool(live.any()) else 0.0
    print(f"trunk64 dflow parity | {tag} | max |ref| {float(ref.abs().max()):.2e} | max err {float(err.max()):.2e} | largest err / bound {ratio:.3f}")
    assert bool((err <= tol).all()), (tag, ratio)
    return ratio


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [64, 32])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=_sid)
def test_kernel_alone(size, n, f, mode):
    h, w = size
    for kind in ("fractional", "border", "far"):
        g, state, flow, ref, tol = _kernel_reference(n, h, w, f, mode, kind)
        if kind != "far":
            assert FG.fractions_ok(flow)             # fp32 and float64 floor to the same cell
        got = _kernel(g, state, flow, mode)
        _hold_elements(f"{mode} F={f} n={n} {h}x{w} {kind}", got, ref, tol)
        if kind == "far":
            assert int((got != 0).sum()) == 0        # wholly outside: exactly zero
        if w == 1:
            assert int((got[:, 0] != 0).sum()) == 0
        if h == 1:
            assert int((got[:, 1] != 0).sum()) == 0
    if h > 1 and w > 1:                              # the border case does put each corner outside somewhere
        pos = FG.positions(_kernel_reference(n, h, w, f, mode, "border")[2])
        x0, y0 = pos[:, 0].floor(), pos[:, 1].floor()
        assert bool((x0 < 0).any()) and bool((x0 + 1 >= w).any()) and bool((y0 < 0).any()) and bool((y0 + 1 >= h).any())


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [(5, 9), (17, 17)], ids=_sid)
def test_kernel_integer_positions(size, mode):
    """size - 1 a power of two: fp32 positions are exact, so landings on -1, 0, size - 1 and size fall in the reference's cell"""
    h, w = size
    g, state, flow, ref, tol = _kernel_reference(2, h, w, 64, mode, "integer")
    assert torch.equal(flow, flow.round()) and float(ref.abs().max()) > 0
    _hold_elements(f"{mode} {h}x{w} integer", _kernel(g, state, flow, mode), ref, tol)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_kernel_strided_views_and_determinism(mode):
    """flow = channels 1..2 of a 3-channel parent, dflow = channels 2..3 of a 5-channel parent, both NaN-filled: the result equals the
    dense run's bit for bit, everything outside the views stays NaN; two runs give the same bits"""
    n, h, w = 3, 7, 9
    g, state, flow, ref, tol = _kernel_reference(n, h, w, 64, mode, "fractional")
    gd, sd = g.to(DT[mode]).cuda(), state.to(DT[mode]).cuda()
    dense = _launch_dflow(gd, sd, flow.cuda(), mode, torch.full((n, 2, h, w), float("nan"), device="cuda"))
    again = _launch_dflow(gd, sd, flow.cuda(), mode, torch.full((n, 2, h, w), float("nan"), device="cuda"))
    assert bool(dense.isfinite().all()) and torch.equal(dense, again)
    fpar = torch.full((n, 3, h, w), float("nan"), device="cuda")
    fpar[:, 1:] = flow.cuda()
    dpar = torch.full((n, 5, h, w), float("nan"), device="cuda")
    out = _launch_dflow(gd, sd, fpar[:, 1:], mode, dpar[:, 2:4])
    assert out.stride(0) == 5 * h * w and fpar[:, 1:].stride(0) == 3 * h * w
    assert torch.equal(out, dense)
    assert bool(dpar[:, :2].isnan().all()) and bool(dpar[:, 4:].isnan().all()) and bool(fpar[:, 0].isnan().all())
    _hold_elements(f"{mode} strided", out.cpu(), ref, tol)


# ---- 2. one trunk, two recurrent steps -------------------------------------------------------------------------------------------
STEP_GEOM = (2, 12, 20)


def _trunks(f, mode, count=2, nb=2, seed=5):
    from mobilesuperresolution_amd.models import ConvResidualBlocks
    torch.manual_seed(seed)
    out = [ConvResidualBlocks(f + 3, f, nb, hot_dtype=mode).cuda() for _ in range(count)]
    for m in out:
        m.hot_training = True
    return out


def _step_inputs(f, seed=40):
    n, h, w = STEP_GEOM
    g = torch.Generator().manual_seed(seed + f)
    flow = FG.fractional_flow(n, h, w, g)
    f0, f1 = (torch.rand(n, 3, h, w, generator=g) for _ in range(2))
    wy = torch.randn(n, f, h, w, generator=g)
    return f0, f1, flow, wy


def _step_run(m, f0, f1, flow, wy, flow_grad=True):
    """two recurrent steps through forward_warped; the loss is on y1 alone, so d f0 arrives through the state gradient only"""
    m.flat.grad = None
    a0, a1 = f0.cuda().requires_grad_(True), f1.cuda().requires_grad_(True)
    fl = flow.cuda().requires_grad_(flow_grad)
    y0, st = m.forward_warped(a0)
    st.retain_grad()
    y1, _ = m.forward_warped(a1, st, fl)
    (y1 * wy.cuda()).sum().backward()
    return dict(y1=y1.detach(), dflat=m.flat.grad.clone(), df0=a0.grad.clone(), df1=a1.grad.clone(), dstate=st.grad.clone(),
                dflow=fl.grad.clone() if flow_grad else None)


def _step_ref(m, f, f0, f1, flow, wy):
    """the same two steps with the warp in float64 on the CPU (autograd runs through it) and the trunk fed the plain concat"""
    m.flat.grad = None
    n, _, h, w = f0.shape
    a0, a1 = f0.cuda().requires_grad_(True), f1.cuda().requires_grad_(True)
    fl = flow.cuda().requires_grad_(True)
    y0 = m(torch.cat([a0, torch.zeros(n, f, h, w, device="cuda")], 1))
    warped = WR.warp_ref(y0.double().cpu(), fl.double().cpu().permute(0, 2, 3, 1)).float().cuda()
    y1 = m(torch.cat([a1, warped], 1))
    (y1 * wy.cuda()).sum().backward()
    return fl.grad.clone()


def _rel_l2(x, y):
    return ((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [64, 32])
def test_one_trunk_two_steps(f, mode):
    """flow.grad in relative L2 within the bounds tests/test_gpu_warp.py holds the 24-wide route's dflow to in the same construction
    (fp32 2e-5, bf16 3e-2); with the flag on, every other gradient is the detached run's bit for bit"""
    a, b = _trunks(f, mode)
    b.load_state_dict(a.state_dict())
    a.flow_training = True
    f0, f1, flow, wy = _step_inputs(f)
    assert FG.fractions_ok(flow)
    got = _step_run(a, f0, f1, flow, wy)
    ref = _step_ref(b, f, f0, f1, flow, wy)
    tol = {"fp32": 2e-5, "bf16": 3e-2}[mode]
    err = _rel_l2(got["dflow"], ref)
    print(f"trunk64 dflow parity | two steps | {mode} F={f} | rel L2 {err:.2e} | bound {tol:.0e}")
    assert got["dflow"].shape == flow.shape and got["dflow"].dtype == torch.float32 and float(ref.abs().max()) > 0
    assert err <= tol, (f, mode, err)
    det = _step_run(a, f0, f1, flow, wy, flow_grad=False)
    hold_exact(("flow detached or not", f, mode), [(k, got[k], det[k]) for k in ("y1", "dflat", "df0", "df1", "dstate")])
    again = _step_run(a, f0, f1, flow, wy)
    assert torch.equal(again["dflow"], got["dflow"])


# ---- 3. the paired route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_paired_route_equals_the_single_trunks(mode):
    from mobilesuperresolution_amd.models.basicvsr_arch import forward_warped_pair
    f, (n, h, w) = 64, STEP_GEOM
    ma, mb = _trunks(f, mode, seed=9)
    ma.flow_training = mb.flow_training = True
    g = torch.Generator().manual_seed(77)
    frames = torch.rand(2 * n, 3, h, w, generator=g).cuda()
    state = torch.randn(2 * n, h, w, 64, generator=g).to(DT[mode]).cuda()
    flow = FG.fractional_flow(2 * n, h, w, g).cuda()
    dy = torch.randn(2 * n, f, h, w, generator=g).cuda()
    fl = flow.clone().requires_grad_(True)
    fa, fb, _ = forward_warped_pair(ma, mb, frames, state, fl)
    torch.autograd.backward([fa, fb], [dy[:n], dy[n:]])
    assert fl.grad.shape == (2 * n, 2, h, w) and bool(fl.grad.isfinite().all())
    pairs = []
    for name, m, sl in (("a", ma, slice(0, n)), ("b", mb, slice(n, None))):
        one = flow[sl].clone().requires_grad_(True)
        y, _ = m.forward_warped(frames[sl], state[sl], one)
        y.backward(dy[sl])
        assert float(one.grad.abs().max()) > 0
        pairs.append((f"dflow {name}", fl.grad[sl], one.grad))
    hold_exact(("paired", mode), pairs)
    assert not torch.equal(fl.grad[:n], fl.grad[n:])


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_refusals(mode):
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.models.basicvsr_arch import forward_warped_pair
    f, (n, h, w) = 64, (2, 5, 6)
    off, on, on2 = _trunks(f, mode, count=3, nb=0)
    on.flow_training = on2.flow_training = True
    frame = torch.rand(n, 3, h, w, device="cuda")
    state = torch.zeros(n, h, w, 64, dtype=DT[mode], device="cuda")
    flow = torch.zeros(n, 2, h, w, device="cuda")
    with pytest.raises(NotImplementedError, match="flow"):                      # the default: as before
        off.forward_warped(frame, state, flow.clone().requires_grad_(True))
    for pair in ((on, off), (off, on)):
        with pytest.raises(NotImplementedError, match="flow_training"):
            forward_warped_pair(*pair, frame, state, flow.clone().requires_grad_(True))
    fl = flow.clone().requires_grad_(True)
    _, _, st = forward_warped_pair(on, on2, frame, state, fl)
    assert st.grad_fn is not None
    off.hot_training = False                                                   # flow_training alone opts in to nothing
    off.flow_training = True
    with pytest.raises(NotImplementedError, match="hot_training"):
        off.forward_warped(frame, state, flow.clone().requires_grad_(True))
    # the C entries: every argument check comes before the first launch
    lib, code, sp = L.lib(), L.DTYPE_CODE[DT[mode]], L.stream_ptr()
    img = torch.zeros(1, h, w, 64, dtype=DT[mode], device="cuda")
    f1, d1 = torch.zeros(1, 2, h, w, device="cuda"), torch.zeros(1, 2, h, w, device="cuda")
    for g_, s_, fl_, d_ in ((img, None, f1, d1), (img, img, None, d1), (None, img, f1, d1), (img, img, f1, None)):
        with pytest.raises(L.HotpathError, match="bad argument"):
            L.launch("sr_c64_warp_dflow", lib.sr_c64_warp_dflow, *(t.data_ptr() if t is not None else None for t in (g_, s_)),
                     fl_.data_ptr() if fl_ is not None else None, 2 * h * w, d_.data_ptr() if d_ is not None else None, 2 * h * w,
                     1, h, w, code, sp)
    acts, ga, dx0 = torch.zeros_like(img), torch.zeros_like(img), torch.zeros_like(img)
    blob = torch.zeros(1 << 16, dtype=DT[mode], device="cuda")
    boff = (ctypes.c_long * 2)(0, -1)
    fr = torch.zeros(1, 3, h, w, device="cuda")
    for state_, flow_, dx0_ in ((None, None, dx0), (img, None, dx0), (img, f1, None)):
        warp = L.C3Warp(fr.data_ptr(), 3 * h * w, state_.data_ptr() if state_ is not None else None,
                        flow_.data_ptr() if flow_ is not None else None, 2 * h * w, None, None, d1.data_ptr(), 2 * h * w, None)
        with pytest.raises(L.HotpathError, match="bad argument"):
            L.launch("sr_c64_trunk_bwd", lib.sr_c64_trunk_bwd, None, ctypes.byref(warp), acts.data_ptr(), None, ga.data_ptr(), None,
                     blob.data_ptr(), boff, None, dx0_.data_ptr() if dx0_ is not None else None, None, 0, 0, 1, h, w, 80, code, 0, 0, sp)
    for name in ("sr_c64_trunk_fwd", "sr_c64_trunk_train_fwd"):                 # the forwards keep refusing a dflow
        warp = L.C3Warp(fr.data_ptr(), 3 * h * w, img.data_ptr(), f1.data_ptr(), 2 * h * w, None, None, d1.data_ptr(), 2 * h * w, None)
        args = (None, ctypes.byref(warp)) + ((None, None, acts.data_ptr()) if name == "sr_c64_trunk_fwd" else (acts.data_ptr(), None))
        with pytest.raises(L.HotpathError, match="bad argument"):
            L.launch(name, getattr(lib, name), *args, blob.data_ptr(), boff, 0, 1, h, w, 80, code, 0, 0, sp)


# ---- 5. BasicVSR_origin, gradients at flow leaves ----------------------------------------------------------------------------------
def _origin(f, nb, mode, params=None, seed=None):
    from mobilesuperresolution_amd.models import BasicVSR_origin
    if seed is not None:
        torch.manual_seed(seed)
    m = BasicVSR_origin(f, nb, hot_dtype=mode)
    if params is not None:
        sd = m.state_dict()
        for k, v in params.items():
            assert k in sd and sd[k].shape == v.shape, k
            sd[k] = v.clone()
        m.load_state_dict(sd, strict=True)
    m = m.cuda()
    m.hot_training = True
    m.flow_training = True
    return m


def _origin_step(model, c, flow_grad):
    from mobilesuperresolution_amd import _lib as L
    real, log = L.launch, []

    def counting(name, fn, *a):
        log.append(name)
        return real(name, fn, *a)
    model.zero_grad(set_to_none=True)
    ff, fb = c["ff"].cuda().requires_grad_(flow_grad), c["fb"].cuda().requires_grad_(flow_grad)
    size = tuple(c["target"].shape[-2:])
    L.launch = counting
    try:
        out = model(c["x"].cuda(), *size, flows=(ff, fb))
        W._charbonnier(out, c["target"].cuda()).backward()
    finally:
        L.launch = real
    sd = dict(model.named_parameters())
    grads = {tr: getattr(model, tr).flat.grad.detach().clone() for tr in W.TRUNKS}
    grads.update({k: sd[k].grad.detach().clone() for k in W.ORIGIN_RECON})
    return grads, ff.grad, fb.grad, log


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f,nb", FG.MODEL_WIDTHS)
def test_model_flow_leaf_gradients(f, nb, mode):
    """d ff and d fb within parity_kit.bound(mode, e) of the float64 step, e = the composed emulation's own distance (fp32 on the
    positive twins: DESIGN.md section 23); the HIP reconstruction runs; the parameter gradients are the detached run's bit for bit.

    Observed ratios kernel / yardstick are printed per tensor; DESIGN.md section 25 keeps the table."""
    c, ref, yard = FG.model_reference(f, nb, mode)
    model = _origin(f, nb, mode, c["params"])
    n = c["x"].shape[1]
    grads, dff, dfb, log = _origin_step(model, c, True)
    assert (log.count("sr_c64_trunk_train_fwd"), log.count("sr_c64_trunk_bwd"), log.count("sr_c64_recon_fwd"),
            log.count("sr_c64_recon_bwd"), log.count("sr_pixel_shuffle")) == (n, n, n, n, 0), log
    bad = []
    for name, got, r64, e in zip(("d flows_forward", "d flows_backward"), (dff, dfb), ref, yard):
        assert got is not None and got.shape == r64.shape and bool(got.isfinite().all()), name
        err = rel_max(got.cpu(), r64)
        print(f"trunk64 flow leaves | F={f} | {mode} | {name} | yardstick {e:.2e} | kernel {err:.2e} | ratio {err / e:.2f} | "
              f"bound {bound(mode, e):.2e}")
        if not err <= bound(mode, e):
            bad.append((name, err, e))
    assert not bad, bad
    det, none_f, none_b, _ = _origin_step(model, c, False)
    assert none_f is None and none_b is None
    hold_exact(("parameter gradients, flows detached or not", f, mode), [(k, grads[k], det[k]) for k in grads])


# ---- 6. end to end: SPyNet receives the gradient -----------------------------------------------------------------------------------
SPY = 64                                                 # SPyNet's six-level pyramid halves the frame five times and resizes to a multiple of 32: 64 x 64
#                                                          is the smallest frame it takes (the size tests/test_gpu_spynet_train.py uses)


def _spynet_grads(model):
    return [(k, p.grad) for k, p in model.spynet.named_parameters()]


def _hold_spynet(tag, model, run):
    """run(flows) -> loss.  One pass with SPyNet inside the graph; one with the same flows detached and re-attached as leaves, whose
    leaf gradients go through torch.autograd.grad: the parameter gradients agree bit for bit (each parameter sums two terms, one per
    SPyNet call, and SpyNet's backward is deterministic: tests/test_gpu_spynet_train.py)"""
    model.zero_grad(set_to_none=True)
    run(None).backward()
    full = _spynet_grads(model)
    assert len(full) == 60
    for k, gr in full:
        assert gr is not None and bool(torch.isfinite(gr).all()), k
    assert any(bool((gr != 0).any()) for _, gr in full)
    model.zero_grad(set_to_none=True)
    flows = model.get_flow(run.x)
    leaves = [t.detach().requires_grad_(True) for t in flows]
    run(tuple(leaves)).backward()
    assert all(p.grad is None for p in model.spynet.parameters())
    params = [p for _, p in model.spynet.named_parameters()]
    via = torch.autograd.grad(list(flows), params, grad_outputs=[t.grad for t in leaves])
    hold_exact(tag, [(k, gr, v) for (k, gr), v in zip(full, via)])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_origin_end_to_end(mode):
    model = _origin(64, 2, mode, seed=21)
    model.spynet.hot_training = True
    g = torch.Generator().manual_seed(22)
    x = torch.rand(2, 3, 3, SPY, SPY, generator=g).cuda()
    target = torch.rand(2, 3, 3, 4 * SPY, 4 * SPY, generator=g).cuda()

    def run(flows):
        return W._charbonnier(model(x, 4 * SPY, 4 * SPY, flows=flows), target)
    run.x = x
    assert model._hot_training_route(x, *model.get_flow(x), 4 * SPY, 4 * SPY) == (True, "hot")
    _hold_spynet(("origin", mode), model, run)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_basicvsr_propagation_end_to_end(mode):
    from mobilesuperresolution_amd.models import BasicVSR, set_flow_training, set_wide_training
    torch.manual_seed(23)
    model = BasicVSR(64, 2, hot_dtype=mode).cuda()
    model.spynet.hot_training = True
    assert len(set_wide_training(model)) == 2 and len(set_flow_training(model)) == 2
    g = torch.Generator().manual_seed(24)
    x = torch.rand(1, 3, 3, SPY, SPY, generator=g).cuda()
    cot = torch.randn(2, 3, 1, 64, SPY, SPY, generator=g).cuda()

    def run(flows):
        feat_b, feat_f = model.propagation_features(x, flows)
        return sum((a * cot[0, i]).sum() + (b * cot[1, i]).sum() for i, (a, b) in enumerate(zip(feat_b, feat_f)))
    run.x = x
    _hold_spynet(("basicvsr", mode), model, run)
