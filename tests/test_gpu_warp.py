"""Warp parity: every hand-written form of the bilinear warp against tests/warp_ref.py (plain torch, float64, CPU), at the edges
of its control flow and indexing.

  standalone csrc/flow_warp.h       forward, dx (atomic scatter), dflow (four channel phases, two shuffles): grid-stride trips,
                                    channel counts that leave phases empty or uneven, taps on and beyond the border, size-1 axes,
                                    many outputs on one source pixel, pure shifts
  gathered first conv, 24-wide      c3_stage_x_warp and the gather-form backward c3_warp_bwd_kernel (csrc/conv3x3.h): every
                                    class of the window radius rw = ceil(flow_bound) + 1 around the LDS limit rw = 7, tiles smaller
                                    than / equal to / one past 16 pixels, border landings, a whole-row window, an explicit bound;
                                    d f0 is the state gradient handed to the previous frame, seen directly
  gather of the 64-wide trunk       csrc/conv64.h, inference

Tolerance of the standalone kernels: none is hard-coded.  Each case runs the reference's own statement of the op (normalise,
F.grid_sample) in fp32 on the CPU; its max-abs distance from the float64 result is the yardstick e_ref of that case and output,
and the kernel must be within 8 e_ref + 1e-6 max|ref| (8: another summation order -- channel phases and shuffles for dflow, atomics
in arbitrary order for dx).  Every case prints e_ref, the kernel's error and their ratio; DESIGN.md keeps the measured table."""
import functools

import pytest
import torch

from tests import warp_ref as WR

pytestmark = pytest.mark.gpu

OUTPUTS = ("y", "dx", "dflow")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """inputs, float64 reference and fp32 yardstick of a standalone case: computed once, shared, never written to"""
    x, flow, dy = WR.standalone_case(name)
    ref = WR.warp_ref_grads(x, flow, dy)
    f32 = WR.warp_ref_grads(x, flow, dy, fn=WR.grid_sample_warp, dtype=torch.float32)
    e_ref = tuple((a.double() - r).abs().max().item() for a, r in zip(f32, ref))
    return x, flow, dy, ref, e_ref


def _hold(name, what, got, ref, e_ref):
    err = (got.double().cpu() - ref).abs().max().item()
    tol = 8 * e_ref + 1e-6 * ref.abs().max().item()
    ratio = err / e_ref if e_ref > 0 else float("nan")
    print(f"warp parity | {name} | {what} | e_ref {e_ref:.2e} | kernel {err:.2e} | ratio {ratio:.2f} | bound {tol:.2e}")
    assert err <= tol, (name, what, err, tol)


def _forward(name):
    from mobilesuperresolution_amd.models import flow_warp
    x, flow, dy, ref, e_ref = _reference(name)
    xg, fg = x.cuda().requires_grad_(True), flow.cuda().requires_grad_(True)
    y = flow_warp(xg, fg)
    _hold(name, "y", y.detach(), ref[0], e_ref[0])
    return xg, fg, y


def _forward_backward(name):
    """forward, backward with both gradients, then with x alone and with the flow alone (dflow == nullptr / dx == nullptr)"""
    from mobilesuperresolution_amd.models import flow_warp
    x, flow, dy, ref, e_ref = _reference(name)
    xg, fg, y = _forward(name)
    y.backward(dy.cuda())
    _hold(name, "dx", xg.grad, ref[1], e_ref[1])
    _hold(name, "dflow", fg.grad, ref[2], e_ref[2])
    x1 = x.cuda().requires_grad_(True)
    flow_warp(x1, flow.cuda()).backward(dy.cuda())
    _hold(name, "dx (x alone)", x1.grad, ref[1], e_ref[1])
    f2 = flow.cuda().requires_grad_(True)
    flow_warp(x.cuda(), f2).backward(dy.cuda())
    _hold(name, "dflow (flow alone)", f2.grad, ref[2], e_ref[2])
    assert torch.equal(f2.grad, fg.grad)             # the flow gradient has a fixed summation order, with or without the scatter
    return xg.grad, fg.grad


@pytest.mark.parametrize("name", ["general-24x16x20-amp3", "general-27x30x41-amp9"])
def test_standalone_general(name):
    _forward_backward(name)


@pytest.mark.parametrize("c", [1, 2, 3, 5, 6])
def test_standalone_channel_phases(c):
    """C = 1, 2, 3 leave whole phases of the wave empty, C = 5, 6 load them unevenly; the plane of 63 pixels is no multiple of 16"""
    _forward_backward(f"phases-C{c}")


@pytest.mark.parametrize("name", ["borders-3x9x17-dyadic", "borders-5x5x33-dyadic"])
def test_standalone_exact_landings_and_borders(name):
    """taps at -1, W - 1 and W, zero weights, one-sided dflow at the border, samples wholly outside"""
    _forward_backward(name)


@pytest.mark.parametrize("name", ["degenerate-H1", "degenerate-W1", "degenerate-1x1"])
def test_standalone_degenerate_sizes(name):
    _, dflow = _forward_backward(name)
    _, _, h, w = WR.STANDALONE_CASES[name][0]
    if w == 1:
        assert (dflow[..., 0] == 0).all()            # exactly: the un-normalisation multiplies by size - 1 = 0
    if h == 1:
        assert (dflow[..., 1] == 0).all()


def test_standalone_grid_stride_forward():
    """131 327 pixels > 8192 workgroups x 16 and no multiple of 16: a second trip of the grid-stride loop"""
    _forward("gridstride-3x257x511")


def test_standalone_grid_stride_backward():
    """the backward's uniform trip count: lanes past the plane's end take part in the second trip's shuffles"""
    _forward_backward("gridstride-5x257x511")


def test_standalone_contention():
    """40 outputs of a row add into the same two source pixels"""
    _forward_backward("contention-4x12x40")


def test_standalone_integer_shift_forward_and_backward():
    """a constant integer flow at a size whose size - 1 is a power of two is a pure shift with zero fill: bit for bit, both ways"""
    name = "shift-3x9x17"
    x, flow, dy, ref, e_ref = _reference(name)
    xg, fg, y = _forward(name)
    exp = torch.zeros_like(x)
    exp[:, :, 1:, :15] = x[:, :, :8, 2:]             # out[y][x] = x[y - 1][x + 2]
    assert torch.equal(y.detach().cpu(), exp)
    y.backward(dy.cuda())
    edx = torch.zeros_like(x)
    edx[:, :, :8, 2:] = dy[:, :, 1:, :15]
    assert torch.equal(xg.grad.cpu(), edx)
    _hold(name, "dflow", fg.grad, ref[2], e_ref[2])


# ---- the warp gathered into the first conv of the 24-wide trunk, and its gather-form backward ----
def _with_bound_class(flow, lo, hi):
    m = flow.abs().max().item()
    assert lo < m <= hi, (m, lo, hi)
    return flow


def _flow_exactly_6(gen):
    """amp 6 off-integer, then one pixel's x displacement set to -6.0 exactly: max|flow| == 6.0.  The pixel is in column 6, so its
    x position is exactly 0 also after the fp32 round trip (2 * 0 / 40 - 1 = -1), and its y position stays off-integer."""
    f = WR.off_integer_flow((2, 30, 41, 2), 6, gen=gen)
    f[1, 13, 6, 0] = -6.0
    assert f.abs().max().item() == 6.0
    return f


FUSED_CASES = {
    # id: (shape (n, h, w), flow maker, expected rw or None)
    "rw1-zero-flow": ((2, 30, 41), lambda g: torch.zeros(2, 30, 41, 2), 1),
    "rw7-flow-in-5-6": ((2, 30, 41), lambda g: _with_bound_class(WR.off_integer_flow((2, 30, 41, 2), 6, gen=g), 5, 6), 7),
    "rw7-flow-exactly-6": ((2, 30, 41), _flow_exactly_6, 7),
    "rw8-flow-in-6-7": ((2, 30, 41), lambda g: _with_bound_class(WR.off_integer_flow((2, 30, 41, 2), 7, gen=g), 6, 7), 8),
    "amp12": ((2, 30, 41), lambda g: WR.off_integer_flow((2, 30, 41, 2), 12, gen=g), None),
    "general-amp3": ((2, 30, 41), lambda g: WR.off_integer_flow((2, 30, 41, 2), 3, gen=g), None),
    "below-one-tile-7x9": ((1, 7, 9), lambda g: WR.off_integer_flow((1, 7, 9, 2), 3, gen=g), None),
    "tiles-exact-16x32": ((1, 16, 32), lambda g: WR.off_integer_flow((1, 16, 32, 2), 3, gen=g), None),
    "borders-17x33-dyadic": ((1, 17, 33), lambda g: WR.dyadic_flow((1, 17, 33, 2), gen=g), None),
    "converging-12x40": ((1, 12, 40), lambda g: WR.converging_flow(12, 40, 17, 0.37), None),
}
FUSED_NAMES = ("y0", "y1", "dflat", "d f0", "d f1", "dflow")


def _fused_inputs(name):
    (n, h, w), mk, rw = FUSED_CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(FUSED_CASES).index(name))
    flow = mk(g)                                                         # (n, h, w, 2)
    assert torch.isfinite(flow).all() and flow.abs().max() <= 4 * max(h, w)
    if rw is not None:                                                   # the radius c3_warp_bwd_kernel derives from max|flow|
        assert int(torch.ceil(flow.abs().max()).item()) + 1 == rw
    f0, f1 = (torch.rand(n, 3, h, w, generator=g) for _ in range(2))
    wy = torch.randn(n, 24, h, w, generator=g)
    return f0, f1, flow, wy


def _fused_run(m, f0, f1, flow, wy, bound=None):
    """two recurrent steps through forward_warped; the loss is on y1 alone, so d f0 arrives through the state gradient only"""
    m.flat.grad = None
    a0, a1 = f0.cuda().requires_grad_(True), f1.cuda().requires_grad_(True)
    fl = flow.permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True)
    y0, st = m.forward_warped(a0)
    y1, _ = m.forward_warped(a1, st, fl, bound)
    (y1 * wy.cuda()).sum().backward()
    return y0.detach(), y1.detach(), m.flat.grad.clone(), a0.grad.clone(), a1.grad.clone(), fl.grad.clone()


def _fused_ref(m, f0, f1, flow, wy):
    """the same two steps with the warp in float64 on the CPU (autograd runs through it) and the trunk fed the plain concat"""
    m.flat.grad = None
    n, _, h, w = f0.shape
    a0, a1 = f0.cuda().requires_grad_(True), f1.cuda().requires_grad_(True)
    fl = flow.permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True)
    y0 = m(torch.cat([a0, torch.zeros(n, 24, h, w, device="cuda")], 1))
    warped = WR.warp_ref(y0.double().cpu(), fl.double().cpu().permute(0, 2, 3, 1)).float().cuda()
    y1 = m(torch.cat([a1, warped], 1))
    (y1 * wy.cuda()).sum().backward()
    return y0.detach(), y1.detach(), m.flat.grad.clone(), a0.grad.clone(), a1.grad.clone(), fl.grad.clone()


def _trunk_pair(dtype):
    from mobilesuperresolution_amd.models import ConvResidualBlocks
    torch.manual_seed(5)
    a = ConvResidualBlocks(27, 24, 2, hot_dtype=dtype).cuda()
    b = ConvResidualBlocks(27, 24, 2, hot_dtype=dtype).cuda()
    b.load_state_dict(a.state_dict())
    return a, b


def _rel_l2(x, y):
    return ((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30)).item()


def _fused_compare(tag, got, ref, tol, flow):
    # d out / d flow is discontinuous across cell boundaries: compare it where the reference's fp32 position round trip (which the
    # kernel reproduces) stays in the cell of exact arithmetic -- everywhere, for every flow but the zero flow
    same = WR.same_cell(flow).permute(0, 3, 1, 2).cuda()
    if "zero-flow" in tag:
        assert same.float().mean().item() > 0.8
    else:
        assert same.all()
    for name, x, y in zip(FUSED_NAMES, got, ref):
        if name == "dflow":
            x, y = x * same, y * same
        err = _rel_l2(x, y)
        print(f"fused warp parity | {tag} | {name} | rel L2 {err:.2e} | bound {tol:.0e}")
        assert err <= tol, (tag, name, err)
    assert ref[3].abs().max().item() > 0             # the witness of dstate is not vacuous


@pytest.mark.parametrize("name", sorted(FUSED_CASES))
def test_fused_prologue_fp32(name):
    a, b = _trunk_pair("fp32")
    f0, f1, flow, wy = _fused_inputs(name)
    _fused_compare(name, _fused_run(a, f0, f1, flow, wy), _fused_ref(b, f0, f1, flow, wy), 2e-5, flow)


def test_fused_prologue_explicit_flow_bound():
    """flow_bound = 2 max|flow| (rw = 13: taps recomputed per candidate) gives what the computed bound gives (rw = 7: taps in LDS)"""
    a, b = _trunk_pair("fp32")
    f0, f1, flow, wy = _fused_inputs("rw7-flow-in-5-6")
    ref = _fused_ref(b, f0, f1, flow, wy)
    own = _fused_run(a, f0, f1, flow, wy)
    wide = _fused_run(a, f0, f1, flow, wy, bound=(2 * flow.abs().max()).cuda())
    _fused_compare("explicit bound vs float64", wide, ref, 2e-5, flow)
    _fused_compare("explicit bound vs computed bound", wide, own, 2e-5, flow)


@pytest.mark.parametrize("name", ["general-amp3", "rw7-flow-in-5-6", "rw7-flow-exactly-6", "rw8-flow-in-6-7"])
def test_fused_prologue_bf16(name):
    a, b = _trunk_pair("bf16")
    f0, f1, flow, wy = _fused_inputs(name)
    _fused_compare("bf16 " + name, _fused_run(a, f0, f1, flow, wy), _fused_ref(b, f0, f1, flow, wy), 3e-2, flow)


# ---- the gather of the 64-wide inference trunk ----
@pytest.mark.parametrize("name", ["borders-17x33-dyadic", "amp9-30x41", "below-one-tile-7x9"])
def test_fused_gather_64_wide(name):
    from mobilesuperresolution_amd.models import ConvResidualBlocks
    shape, mk = {"borders-17x33-dyadic": ((1, 17, 33), lambda s, g: WR.dyadic_flow(s, gen=g)),
                 "amp9-30x41": ((2, 30, 41), lambda s, g: WR.off_integer_flow(s, 9, gen=g)),
                 "below-one-tile-7x9": ((1, 7, 9), lambda s, g: WR.off_integer_flow(s, 3, gen=g))}[name]
    n, h, w = shape
    g = torch.Generator().manual_seed(3000 + h)
    flow = mk((n, h, w, 2), g)
    fr0, fr1 = (torch.rand(n, 3, h, w, generator=g).cuda() for _ in range(2))
    torch.manual_seed(64)
    m = ConvResidualBlocks(67, 64, 1, hot_dtype="fp32").cuda().requires_grad_(False)
    with torch.no_grad():
        y0, st = m.forward_warped(fr0)
        y1, _ = m.forward_warped(fr1, st, flow.permute(0, 3, 1, 2).contiguous().cuda())
        r0 = m(torch.cat([fr0, torch.zeros(n, 64, h, w, device="cuda")], 1))
        r1 = m(torch.cat([fr1, WR.warp_ref(r0.double().cpu(), flow).float().cuda()], 1))
    for what, a, b in (("y0", y0, r0), ("y1", y1, r1)):
        e = ((a - b).abs().max() / b.abs().max()).item()
        print(f"64-wide warp parity | {name} | {what} | rel max-abs {e:.2e} | bound 1e-05")
        assert e <= 1e-5, (name, what, e)            # the fp32 bound of tests/test_gpu_vsr64.py, trunk against ATen
