"""The bilinear warp of the video routes (flow_warp: bilinear, zeros padding, align_corners=True) written out in plain torch,
float64 on the CPU, plus the flow generators of the warp parity tests.  Nothing of the package or of the oracle is used here:
this is the outside reference that csrc/flow_warp.h, the gathered first conv of csrc/conv3x3.h and csrc/conv64.h are held
against.  tests/test_warp_ref_host.py pins it to float64 grid_sample and to fixture G8.

With align_corners=True the reference's normalise / un-normalise pair cancels for a size > 1, so output pixel (y, x) samples
the position (x + fx, y + fy); along an axis of size 1 the un-normalisation multiplies by size - 1 = 0: the position component
is 0 and no gradient reaches that flow component."""
import torch


def warp_ref(x, flow):
    """x (n, c, h, w), flow (n, h, w, 2) with [..., 0] = x displacement, [..., 1] = y displacement, in pixels.  Returns the
    warped (n, c, h, w) in float64; differentiable in x and in flow (the weights carry the flow gradient, floor is constant)."""
    x, flow = x.double(), flow.double()
    n, c, h, w = x.shape
    assert flow.shape == (n, h, w, 2)
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    px = gx + flow[..., 0] if w > 1 else flow[..., 0] * 0.0
    py = gy + flow[..., 1] if h > 1 else flow[..., 1] * 0.0
    fx, fy = px.detach().floor(), py.detach().floor()
    wx, wy = px - fx, py - fy
    x0, y0 = fx.long(), fy.long()
    flat = x.reshape(n, c, h * w)

    def tap(yy, xx):
        valid = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(n, 1, h * w).expand(n, c, h * w)
        return flat.gather(2, idx).reshape(n, c, h, w) * valid.reshape(n, 1, h, w).double()

    wx, wy = wx.unsqueeze(1), wy.unsqueeze(1)
    return (tap(y0, x0) * ((1 - wx) * (1 - wy)) + tap(y0, x0 + 1) * (wx * (1 - wy))
            + tap(y0 + 1, x0) * ((1 - wx) * wy) + tap(y0 + 1, x0 + 1) * (wx * wy))


def grid_sample_warp(x, flow):
    """The reference's own statement of the op (its flow_warp: normalise with max(size - 1, 1), F.grid_sample bilinear / zeros /
    align_corners=True) in the dtype of x: float64 to pin warp_ref, float32 as the yardstick of what the op costs in the
    kernels' precision."""
    _, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=x.dtype), torch.arange(w, dtype=x.dtype), indexing="ij")
    vx = 2.0 * (gx + flow[..., 0]) / max(w - 1, 1) - 1.0
    vy = 2.0 * (gy + flow[..., 1]) / max(h - 1, 1) - 1.0
    return torch.nn.functional.grid_sample(x, torch.stack((vx, vy), dim=3), mode="bilinear", padding_mode="zeros",
                                           align_corners=True)


def off_integer_flow(shape, amp, margin=1.0 / 16, gen=None):
    """float32 flow of `shape` (n, h, w, 2): integer part uniform in [-amp, amp - 1], fractional part uniform in
    [margin, 1 - margin], so |flow| < amp and every sample position stays `margin` away from an integer.  The flow gradient
    is discontinuous at integer positions and the kernels reproduce the reference's fp32 normalise / un-normalise round trip
    (an error of about size * 2^-24 px): off-integer positions keep fp32 and float64 in the same cell."""
    whole = torch.randint(-int(amp), int(amp), shape, generator=gen).float() if amp else torch.zeros(shape)
    frac = margin + (1.0 - 2.0 * margin) * torch.rand(shape, generator=gen)
    return whole + frac


def dyadic_flow(shape, gen=None):
    """float32 flow of `shape` (n, h, w, 2): multiples of 1/4 in +-4 max(h, w).  For sizes with h - 1 and w - 1 powers of two
    only: there the fp32 round trip of the position is exact, so exact landings on -1, 0, W - 1 and W, half-pixel positions and
    samples wholly outside fall in the same cell (floor convention) in fp32 and in float64."""
    _, h, w, _ = shape
    for s in (h - 1, w - 1):
        assert s >= 1 and s & (s - 1) == 0, "dyadic_flow: h - 1 and w - 1 must be powers of two"
    m = 16 * max(h, w)
    return torch.randint(-m, m + 1, shape, generator=gen).float() / 4.0


def converging_flow(h, w, col, frac):
    """float32 flow (1, h, w, 2): every pixel of a row samples position (col + frac, y + frac), i.e. w outputs per row share
    the source pixels col and col + 1."""
    f = torch.empty(1, h, w, 2)
    f[..., 0] = (col + frac - torch.arange(w, dtype=torch.float64)).float().view(1, 1, w)
    f[..., 1] = frac
    return f


def _shift_flow(h, w, fx, fy):
    f = torch.empty(1, h, w, 2)
    f[..., 0], f[..., 1] = fx, fy
    return f


# the input classes of the standalone kernels: id -> ((n, c, h, w), flow of (n, h, w, 2) from a seeded generator)
STANDALONE_CASES = {
    "general-24x16x20-amp3": ((2, 24, 16, 20), lambda s, g: off_integer_flow(s, 3, gen=g)),
    "general-27x30x41-amp9": ((1, 27, 30, 41), lambda s, g: off_integer_flow(s, 9, gen=g)),
    **{f"phases-C{c}": ((2, c, 7, 9), lambda s, g: off_integer_flow(s, 3, gen=g)) for c in (1, 2, 3, 5, 6)},
    "borders-3x9x17-dyadic": ((1, 3, 9, 17), lambda s, g: dyadic_flow(s, gen=g)),
    "borders-5x5x33-dyadic": ((2, 5, 5, 33), lambda s, g: dyadic_flow(s, gen=g)),
    "degenerate-H1": ((1, 5, 1, 13), lambda s, g: off_integer_flow(s, 3, gen=g)),
    "degenerate-W1": ((2, 2, 7, 1), lambda s, g: off_integer_flow(s, 3, gen=g)),
    "degenerate-1x1": ((1, 1, 1, 1), lambda s, g: off_integer_flow(s, 3, gen=g)),
    "gridstride-3x257x511": ((1, 3, 257, 511), lambda s, g: off_integer_flow(s, 4, gen=g)),
    "gridstride-5x257x511": ((1, 5, 257, 511), lambda s, g: off_integer_flow(s, 4, gen=g)),
    "contention-4x12x40": ((1, 4, 12, 40), lambda s, g: converging_flow(12, 40, 17, 0.37)),
    "shift-3x9x17": ((1, 3, 9, 17), lambda s, g: _shift_flow(9, 17, 2.0, -1.0)),
}


def standalone_case(name):
    """(x, flow, dy) in float32 of a standalone case, from a seed that depends on the case alone"""
    shape, mk = STANDALONE_CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(STANDALONE_CASES).index(name))
    n, c, h, w = shape
    x = torch.randn(shape, generator=g)
    flow = mk((n, h, w, 2), g)
    dy = torch.randn(shape, generator=g)
    assert torch.isfinite(flow).all() and flow.abs().max() <= 4 * max(h, w)
    return x, flow, dy


def warp_ref_grads(x, flow, dy, fn=warp_ref, dtype=torch.float64):
    """(y, dx, dflow) of `fn` in `dtype` for the cotangent dy"""
    xd, fd = (t.detach().to(dtype, copy=True).requires_grad_(True) for t in (x, flow))     # copies: the inputs stay as they are
    y = fn(xd, fd)
    y.backward(dy.to(dtype))
    return y.detach(), xd.grad, fd.grad


def same_cell(flow):
    """bool (n, h, w, 2): True where the reference's fp32 normalise / un-normalise round trip leaves the sample position
    component in the cell (floor) that exact arithmetic gives.  d out / d flow[..., k] is discontinuous only across cell
    boundaries of component k, so where this is False fp32 and float64 rightly differ by a one-sided derivative."""
    n, h, w, _ = flow.shape
    out = torch.empty(flow.shape, dtype=torch.bool)
    for k, size in ((0, w), (1, h)):
        view = (1, 1, w) if k == 0 else (1, h, 1)
        g32 = torch.arange(size, dtype=torch.float32).view(view)
        v = 2.0 * (g32 + flow[..., k].float()) / max(size - 1, 1) - 1.0
        p32 = ((v + 1.0) / 2.0) * (size - 1)
        p64 = (g32.double() + flow[..., k].double()) if size > 1 else torch.zeros(flow.shape[:3], dtype=torch.float64)
        out[..., k] = p32.floor().double() == p64.floor()
    return out
