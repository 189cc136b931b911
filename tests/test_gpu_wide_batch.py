"""The `hot_training` routes of the wide video models (24 < F <= 64) at MORE THAN ONE CLIP and in BOTH dtypes, where the Python glue
that wires the kernels together indexes for real: the paired batch and its halves, the per-clip views of frames, flows and cotangents
and their batch strides.  BasicVSR_origin (given flows) and MotionVectorVSR on b x 3 x 3 x 18 x 20, b in {2, 3}, (F, nb) in {(40, 1),
(64, 2)}, against tests/wide_model_ref.py (plain torch, float64, CPU; tests/test_wide_model_ref_host.py shows that its cases tell
clips and halves apart).

  1. reference      output and every gradient group within parity_kit.bound of the float64 step; the yardstick is the composed
                    emulation's own distance (float32 throughout / float64 with the bf16 rounding points)
  2. clips          the batched forward of clip k equals the same model on clip k alone, bit for bit (no_grad and graph-recording)
  3. state grads    mvvsr_arch._ReconFunction's d state of both halves at b in {2, 3} against mv_recon_ref.backward (BasicVSR_origin's
                    twin is tests/test_gpu_recon_bwd.py::test_state_gradients_land_in_their_halves)
  4. strides        kernel level, exact: every strided operand is slot 1 of a NaN-filled clip-shaped parent, passed with the view's
                    real strides; results bit for bit, the rest of every output parent still NaN
"""
import pytest
import torch

from tests import mv_recon_ref as M
from tests import recon_bwd_ref as B
from tests import recon_ref as R
from tests import trunk_ref as TR
from tests import wide_model_ref as W
from tests.parity_kit import bound, hold_exact, rel_max

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16")
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
SIZE = (4 * W.HEIGHT, 4 * W.WIDTH)


def _model(kind, f, nb, mode, params):
    from mobilesuperresolution_amd.models import BasicVSR_origin, MotionVectorVSR
    m = (BasicVSR_origin if kind == "origin" else MotionVectorVSR)(f, nb, hot_dtype=mode)
    sd = m.state_dict()
    for k, v in params.items():
        assert k in sd and sd[k].shape == v.shape, k
        sd[k] = v.clone()
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    m.hot_training = True
    return m


def _call(model, kind, x, mv):
    if kind == "origin":
        return model(x, *SIZE, flows=(mv[:, 1:], -mv[:, 1:]))
    return model(torch.cat([x, mv], 2), *SIZE)


def _hot_log_ok(kind, log):
    n = W.FRAMES
    trunks = (log.count("sr_c64_trunk_train_fwd"), log.count("sr_c64_trunk_bwd")) == (n, n)
    if kind == "origin":
        return trunks and (log.count("sr_c64_recon_fwd"), log.count("sr_c64_recon_bwd"), log.count("sr_c64_recon_reduce"),
                           log.count("sr_pixel_shuffle")) == (n, n, n, 0)
    return trunks and (log.count("sr_mv_recon_fwd"), log.count("sr_mv_recon_bwd64"), log.count("sr_mv_recon_bwd")) == (1, 1, 0)


def _step(model, kind, nb, c):
    """forward + Charbonnier + backward on the hot route: (output, {group: gradient}, the C calls by name)"""
    from mobilesuperresolution_amd import _lib as L
    real, log = L.launch, []

    def counting(name, fn, *a):
        log.append(name)
        return real(name, fn, *a)
    model.zero_grad(set_to_none=True)
    L.launch = counting
    try:
        out = _call(model, kind, c["x"].cuda(), c["mv"].cuda())
        W._charbonnier(out, c["target"].cuda()).backward()
    finally:
        L.launch = real
    sd = dict(model.named_parameters())
    grads = {tr: getattr(model, tr).flat.grad.detach().cpu() for tr in W.TRUNKS}
    grads.update({k: sd[k].grad.detach().cpu() for k in W.RECON[kind]})
    return out.detach().cpu(), grads, log


# ---- 1. against the composed reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b", W.BATCHES)
@pytest.mark.parametrize("f,nb", W.WIDTHS)
@pytest.mark.parametrize("kind", W.KINDS)
def test_step_against_the_composed_reference(kind, f, nb, b, mode):
    """the output and every gradient group (both trunks flat, every reconstruction tensor) within parity_kit.bound(mode, e) of the
    float64 step, e = the composed emulation's own distance.  The weight gradients sum over every clip, so this also holds the
    batched step's gradients to the sum of the clips'.

    bf16 runs on the cases with both signs in front of every mask, fp32 on the twin cases whose biases keep every masked
    pre-activation of the float64 step at least wide_model_ref.MARGIN = 0.25 above zero: 8 fp32 yardsticks are a few 1e-6, and one
    LeakyReLU mask that an fp32 sum signs differently from float64 moves a gradient by 1e-4."""
    c, ref, yard = W.reference(kind, f, nb, b, mode)
    model = _model(kind, f, nb, mode, c["params"])
    out, grads, log = _step(model, kind, nb, c)
    assert _hot_log_ok(kind, log), log
    bad = []
    for (name, r64), got in zip(W.tensors(ref), [out] + [grads[k] for k in ref[1]]):
        e, err = yard[name], rel_max(got, r64)
        ratio = err / e if e > 0 else float("nan")
        print(f"wide batch parity | {kind} | F={f} | b={b} | {mode} | {name} | yardstick {e:.2e} | kernel {err:.2e} | ratio {ratio:.2f} | "
              f"bound {bound(mode, e):.2e}")
        if not (got.shape == r64.shape and bool(got.isfinite().all()) and err <= bound(mode, e)):
            bad.append((name, err, e))
    assert not bad, bad


# ---- 2. clips do not see each other ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["no_grad", "graph"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f,nb", W.WIDTHS)
@pytest.mark.parametrize("kind", W.KINDS)
def test_clips_do_not_see_each_other(kind, f, nb, mode, graph):
    """b = 3: the batched forward of clip k equals the forward of clip k alone, bit for bit, on the handles route (no_grad) and on the
    training route (a graph is recorded).  No rule of either route picks a forward kernel by batch size."""
    c = W.case(kind, f, nb, 3)
    model = _model(kind, f, nb, mode, c["params"])
    x, mv = c["x"].cuda(), c["mv"].cuda()

    def fwd(xs, ms):
        if graph:
            out = _call(model, kind, xs, ms)
            assert out.grad_fn is not None
            return out.detach()
        with torch.no_grad():
            return _call(model, kind, xs, ms)
    whole = fwd(x, mv)
    assert whole.shape == (3, W.FRAMES, 3) + SIZE and bool(whole.isfinite().all())
    hold_exact((kind, f, mode, graph), [(f"clip {k}", whole[k:k + 1], fwd(x[k:k + 1], mv[k:k + 1]).cpu()) for k in range(3)])


# ---- 3. state gradients of MotionVectorVSR's node -----------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [2, 3])
def test_mv_state_gradients_land_in_their_halves(b):
    """dsteps of a 3-frame clip batch through mvvsr_arch._ReconFunction (fp32, F = 40): frame i's two state gradients go to step
    n - 1 - i, first half, and step i, second half, clip by clip; channels >= F exactly zero.  Against mv_recon_ref.backward in float64.
    Bound 2e-4 of the largest element, the one BasicVSR_origin's twin derives for five layers of 576-term fp32 sums: this chain is
    shallower (the 80-term fusion, the 75-row transposed conv, four blend taps), so it holds a fortiori, at any b."""
    from mobilesuperresolution_amd.models import mvvsr_arch as A
    f, n, h, w = 40, W.FRAMES, W.HEIGHT, W.WIDTH
    c = W.case("mv", f, 1, b)
    model = _model("mv", f, 1, "fp32", c["params"])
    g = torch.Generator().manual_seed(21 + b)
    vals = [torch.randn(2 * b, h, w, f, generator=g) for _ in range(n)]
    steps = []
    for v in vals:
        s = torch.zeros(2 * b, h, w, 64, device="cuda")
        s[..., :f] = v.cuda()
        steps.append(s.requires_grad_(True))
    x_ = torch.cat([c["x"], c["mv"]], 2).cuda()
    out = A._ReconFunction.apply(model, x_, *model._recon_params(), *steps)
    out.retain_grad()
    W._charbonnier(out, c["target"].cuda()).backward()
    nchw = [v.permute(0, 3, 1, 2).double() for v in vals]
    fb = torch.cat([nchw[n - 1 - i][:b] for i in range(n)], 0)                        # frame-major, as mv_recon_ref takes it
    ff = torch.cat([nchw[i][b:] for i in range(n)], 0)
    xs = c["x"].double().transpose(0, 1).reshape(n * b, 3, h, w)
    ps = [c["params"][k].double() for k in W.MV_RECON]
    o64, cc, u, _ = M.forward(fb, ff, xs, *ps)
    # the same function on both sides: the fp32 blend weights are off by up to 4 x 20 ulp of 1 (recon_ref.blend_bound), about 1e-5
    assert rel_max(out.detach().cpu(), o64.view(n, b, 3, *SIZE).transpose(0, 1)) < 1e-4
    # the node's own cotangent on both sides: where a target crosses the output the Charbonnier gradient turns over within 1e-3, so
    # a cotangent taken from the float64 output would differ from the node's by a percent there, which is the loss's doing
    cot = out.grad.cpu().double().transpose(0, 1).reshape(n * b, 3, *SIZE)
    dc = M.backward(cot, cc, u, ps[0], ps[2])["dc"].view(n, b, 2 * f, h, w)
    for i in range(n):
        for name, k, sl, exp in (("first half", n - 1 - i, slice(0, b), dc[i, :, :f]), ("second half", i, slice(b, 2 * b), dc[i, :, f:])):
            got = steps[k].grad[sl].cpu()
            assert bool((got[..., f:] == 0).all()), (i, name)
            for clip in range(b):
                e = rel_max(got[clip, ..., :f], exp[clip].permute(1, 2, 0))
                print(f"mv state gradients | b={b} | frame {i} | step {k} {name} | clip {clip} | distance {e:.2e}")
                assert e < 2e-4, (i, name, clip, e)


# ---- 4. strided entries, kernel level, exact ------------------------------------------------------------------------------------------
def _slot1(t, n_slots=3):
    """t (n, ...) as slot 1 of a NaN-filled (n, n_slots, ...) parent: (parent, the view)"""
    parent = torch.full((t.shape[0], n_slots) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device="cuda")
    parent[:, 1] = t.cuda()
    return parent, parent[:, 1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", [(64, 2, 9, 21), (25, 2, 4, 16)], ids=lambda g: "x".join(map(str, g)))
def test_recon_bwd_strided_cotangent(geom, mode):
    """sr_c64_recon_bwd, stage conv_last (the one that reads g): g is g[:, 1] of a NaN-filled (n, 3, 3, 4h, 4w) parent, g_bs = its real
    batch stride; d_hr, dW and db bit for bit"""
    from tests.test_gpu_recon_bwd import run_stage
    f, n, h, w = geom
    case = B.stage_case(16, f, n, h, w, mode)
    exp = B.exact_ref(case, mode)
    got = run_stage(case, mode, g_parent=True)
    hold_exact(("recon bwd g_bs", geom, mode), [(k, got[k], exp[k]) for k in ("dx", "dW", "db")] + [("pad", got["pad"], torch.zeros_like(got["pad"]))])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", [(25, 2, 2, 4, 16), (64, 2, 3, 16, 32)], ids=lambda g: "x".join(map(str, g)))
def test_mv_recon_strided_clips(geom, mode):
    """sr_mv_recon_fwd at 64 channels (x_bs, x_fs, out strides) and sr_mv_recon_bwd64 (g_bs, g_fs) at b = 2: the frames are [:, :, :3] of
    a NaN-filled (b, n, 5, h, w) parent, as the model passes them (x_fs = 5 h w); output and cotangent are [:, 1:1 + n, :3] of NaN-filled
    (b, n + 2, 4, 4h, 4w) parents, so no clip stride is n frame strides and no frame stride is the dense frame.  out, u, dc and the four
    gradients bit for bit against recon_ref.mv_exact_ref; the rest of the output parent still NaN (asserted in _mv_fwd)"""
    from tests import test_gpu_mv_recon64 as T64
    from tests import test_gpu_recon_ref as T
    case = R.mv_case(*geom)
    inp = T._mv_inputs(case, mode)
    assert inp["cw"] == 64
    ref = R.mv_exact_ref(case, mode)
    tag, b = ("mv strided", geom, mode), case["b"]
    out, u, us = T._mv_fwd(inp, strided=True)
    hold_exact(tag, T._per_frame("out", out, ref["out"], b) + T._per_frame("u", u, ref["u"], b))
    got = T64._mv_bwd64(inp, case, us, mode, via_table=True, g_strided=True)
    hold_exact(tag, T._per_frame("dc", got["dc"], ref["dc"], b) + [(k, got[k], ref[k]) for k in R.MV_GRADS])


@pytest.mark.parametrize("mode", MODES)
def test_recon_fwd_strided_frame_and_output(mode):
    """sr_c64_recon_fwd, conv_last + base at n = 2: the frame is slot 1 of a NaN-filled (n, 3, 3, h, w) parent (frame_bs), which is
    what this test adds; the output in slot 1 of a NaN-filled (n, 3, 3, 4h, 4w) parent (out stride), the other slots still NaN, is
    what tests/test_gpu_recon_ref.py::test_last_exact does already (_run_conv), kept here so that both strides differ from the
    dense ones in one call; bit for bit"""
    from tests import test_gpu_recon_ref as T
    n, h, w = 2, 9, 10
    case = R.conv_case("last", 64, n, 4 * h, 4 * w)
    m = T._vsr_model(64, mode, case)
    dt = DT[mode]
    zeros = lambda: torch.zeros(n, h, w, 64, dtype=dt, device="cuda")
    scratch = (T._nan(n, h, w, 64, dtype=dt), T._nan(n, 2 * h, 2 * w, 64, dtype=dt), T._nan(n, 4 * h, 4 * w, 64, dtype=dt),
               T._nhwc(case["x"], dt, 64))
    _, frame = _slot1(case["frame"])
    big, out = _slot1(torch.full((n, 3, 4 * h, 4 * w), float("nan")))
    assert frame.stride(0) == 3 * 3 * h * w and out.stride(0) == 3 * 48 * h * w
    with torch.no_grad():
        m.reconstruct_hot(zeros(), zeros(), frame, out, scratch, stages=16)
    torch.cuda.synchronize()
    assert T._all_nan(big[:, 0]) and T._all_nan(big[:, 2]), "conv_last wrote outside its slice"
    hold_exact(("recon fwd frame_bs", mode), [("last", big[:, 1].cpu(), R.conv_exact_ref(case, mode))])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f", [64, 40])
def test_trunk_steps_strided_frames_and_flows(f, mode):
    """sr_c64_trunk_train_fwd / sr_c64_trunk_bwd with `warp` at n = 2 (17 x 33, three steps, one flow moves the state off the image):
    every frame and every flow is slot 1 of a NaN-filled clip-shaped parent and goes in as that view (frame_bs, flow_bs); features,
    frame gradients and every entry of flat.grad bit for bit"""
    from tests.test_gpu_trunk64_train import _flat_grads, _module
    geom, shifts = TR.STEP_CASES[1]
    assert geom[0] == 2
    case = TR.exact_step_case(f, 1, *geom, shifts)
    m = _module(f + 3, f, case["params"], mode)
    parents = [_slot1(fr)[0].requires_grad_(True) for fr in case["frames"]]
    flows = [_slot1(fl)[1] for fl in case["flows"]]
    ys, state = [], None
    for k, parent in enumerate(parents):
        frame = parent[:, 1]
        assert frame.stride(0) == 3 * frame[0].numel() and not frame.is_contiguous()
        y, state = m.forward_warped(frame, state, flows[k - 1] if k > 0 else None)
        ys.append(y)
    torch.autograd.backward(ys, [g.cuda() for g in case["dys"]])
    ref, ns = case["ref"], len(parents)
    names = [f"y{k}" for k in range(ns)] + [f"dframe{k}" for k in range(ns)] + TR.tensor_names(1)[2:]
    got = ys + [p.grad[:, 1] for p in parents] + _flat_grads(m)
    hold_exact(("trunk steps strided", f, mode), zip(names, got, ref["y"] + ref["dx"] + ref["grads"]))
