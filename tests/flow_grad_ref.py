"""The flow gradient of the 64-wide training route (ConvResidualBlocks.flow_training; csrc/conv64_bwd.h, c64_warp_dflow_kernel) in
float64 on the CPU, the flows its tests use and the per-element bound they apply.  Plain torch; nothing of the package is used.

  dflow_ref    warp_ref.warp_ref_grads on inputs already rounded to the hot dtype: the cotangent g of the warped state dotted with the
               derivative of the bilinear sample with respect to its position, (n, 2, h, w)
  dflow_bound  what fp32 arithmetic in the kernel's order may differ from that by, per element (derived below, not measured)
  model_step   wide_model_ref's float64 step of BasicVSR_origin with the two flows as LEAVES: wide_model_ref._step detaches them

The bound.  Per output pixel and flow component the kernel forms 64 terms g_c * (d0_c * (1 - w) + d1_c * w) in fp32, with d0 / d1 the
two corner differences along the component's axis and w the weight along the other axis, and adds them: eight per lane in channel
order, then three shuffle levels.  With u = 2^-24:
  * the inputs are exact (already hot-dtype values); every term costs at most 8 roundings (two differences, 1 - w, two products,
    their sum, the product with g, the add), each relative to a partial result bounded by |g_c| (|d0_c| (1 - w) + |d1_c| w), and
    a sum of 64 terms in any order adds at most 63 u of sum |terms|: (8 + 64) u A, A = sum_c |g_c| (|d0_c| (1 - w) + |d1_c| w);
  * w itself comes from the fp32 position: the kernel reproduces the reference's normalise / un-normalise round trip, five
    roundings of quantities no larger than |pos| + size, so |w - w_exact| <= 8 u (|pos| + size) =: dw, which moves a term by at most
    dw |g_c| (|d0_c| + |d1_c|): dw B, B = sum_c |g_c| (|d0_c| + |d1_c|).  This holds while fp32 and float64 agree on the cell, which
    the cases guarantee: fractional parts in [1/16, 15/16], or positions that fp32 represents exactly.
bound = 72 u A + dw B per element; where every corner is outside the image A = B = 0 and the result must be exactly 0."""
import functools

import torch

from tests import wide_model_ref as W
from tests.parity_kit import leaf, rel_max, seed
from tests.warp_ref import warp_ref, warp_ref_grads

U = 2.0 ** -24
HOT = {"fp32": torch.float32, "bf16": torch.bfloat16}


# ---- flows (n, 2, h, w) fp32 --------------------------------------------------------------------------------------------------
def fractional_flow(n, h, w, gen, amp=3):
    """integer part in [-amp, amp - 1], fractional part in [1/8, 7/8]"""
    whole = torch.randint(-amp, amp, (n, 2, h, w), generator=gen).float()
    return whole + 0.125 + 0.75 * torch.rand(n, 2, h, w, generator=gen)


def border_flow(n, h, w, gen):
    """sub-pixel flows, with the first row / column pushed to cell -1 (corners y0 / x0 outside) and the last row / column left in cell
    size - 1 (corners y0 + 1 / x0 + 1 outside): each of the four corners is outside the image somewhere (sizes > 1), three of them at
    the image's corners"""
    f = 0.125 + 0.75 * torch.rand(n, 2, h, w, generator=gen)
    f[:, 0, :, 0] -= 1.0
    f[:, 1, 0, :] -= 1.0
    return f


def far_flow(n, h, w, gen):
    """+-1000 everywhere: every sample lies wholly outside"""
    return 1000.0 * (2.0 * torch.randint(0, 2, (n, 2, h, w), generator=gen).float() - 1.0)


def integer_flow(n, h, w, gen):
    """integers reaching past every border; for sizes with size - 1 a power of two, where fp32 positions are exact"""
    for s in (h - 1, w - 1):
        assert s >= 1 and s & (s - 1) == 0
    return torch.randint(-max(h, w) - 1, max(h, w) + 2, (n, 2, h, w), generator=gen).float()


FLOWS = {"fractional": fractional_flow, "border": border_flow, "far": far_flow}


def positions(flow):
    """float64 sample positions (n, 2, h, w) along the axes whose size is > 1 (0 along an axis of size 1)"""
    n, _, h, w = flow.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    px = gx + flow[:, 0].double() if w > 1 else torch.zeros(n, h, w, dtype=torch.float64)
    py = gy + flow[:, 1].double() if h > 1 else torch.zeros(n, h, w, dtype=torch.float64)
    return torch.stack([px, py], 1)


def fractions_ok(flow, lo=1.0 / 16, hi=15.0 / 16):
    """every position component along an axis of size > 1 has its fractional part in [lo, hi]"""
    _, _, h, w = flow.shape
    pos = positions(flow)
    frac = pos - pos.floor()
    keep = [k for k, s in ((0, w), (1, h)) if s > 1]
    return all(bool(((frac[:, k] >= lo) & (frac[:, k] <= hi)).all()) for k in keep)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def kernel_case(n, h, w, f, mode, kind, seed):
    """g, state (n, h, w, 64) float32 holding hot-dtype values with channels >= f zero, flow (n, 2, h, w) fp32"""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda t: t.to(HOT[mode]).float()
    g, state = torch.zeros(n, h, w, 64), torch.zeros(n, h, w, 64)
    g[..., :f] = rnd(torch.randn(n, h, w, f, generator=gen))
    state[..., :f] = rnd(torch.randn(n, h, w, f, generator=gen))
    flow = integer_flow(n, h, w, gen) if kind == "integer" else FLOWS[kind](n, h, w, gen)
    return g, state, flow


# ---- reference and bound ------------------------------------------------------------------------------------------------------
def dflow_ref(g, state, flow):
    """float64 (n, 2, h, w): g, state NHWC, flow (n, 2, h, w)"""
    _, _, df = warp_ref_grads(state.permute(0, 3, 1, 2), flow.permute(0, 2, 3, 1), g.permute(0, 3, 1, 2))
    return df.permute(0, 3, 1, 2).contiguous()


def _corners(state, flow):
    """the four corner images (n, c, h, w) float64 (zero where outside) and the weights (wx, wy) (n, 1, h, w)"""
    x = state.permute(0, 3, 1, 2).double()
    n, c, h, w = x.shape
    pos = positions(flow)
    x0, y0 = pos[:, 0].floor().long(), pos[:, 1].floor().long()
    wx, wy = (pos[:, 0] - pos[:, 0].floor()).unsqueeze(1), (pos[:, 1] - pos[:, 1].floor()).unsqueeze(1)
    flat = x.reshape(n, c, h * w)

    def tap(yy, xx):
        valid = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(n, 1, h * w).expand(n, c, h * w)
        return flat.gather(2, idx).reshape(n, c, h, w) * valid.reshape(n, 1, h, w).double()
    return tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), wx, wy


def dflow_bound(g, state, flow):
    """float64 (n, 2, h, w): the per-element bound of the module docstring"""
    _, _, h, w = flow.shape
    v00, v01, v10, v11, wx, wy = _corners(state, flow)
    ga = g.permute(0, 3, 1, 2).double().abs()
    dw = 8 * U * (positions(flow).abs().max().item() + max(h, w))
    ax = (ga * ((v01 - v00).abs() * (1 - wy) + (v11 - v10).abs() * wy)).sum(1)
    bx = (ga * ((v01 - v00).abs() + (v11 - v10).abs())).sum(1)
    ay = (ga * ((v10 - v00).abs() * (1 - wx) + (v11 - v01).abs() * wx)).sum(1)
    by = (ga * ((v10 - v00).abs() + (v11 - v01).abs())).sum(1)
    bound = torch.stack([72 * U * ax + dw * bx, 72 * U * ay + dw * by], 1)
    if w == 1:
        bound[:, 0] = 0
    if h == 1:
        bound[:, 1] = 0
    return bound


# ---- the whole step of BasicVSR_origin with flow leaves ---------------------------------------------------------------------------
def model_step(params, x, ff, fb, target, nb, f, dtype=torch.float64, hot=W.R.ident, rnd=None):
    """wide_model_ref._step("origin", ...) with the flows as leaves: (output, {group: gradient}, d ff, d fb)"""
    if rnd is None and hot is not W.R.ident:
        rnd = hot
    p = {k: leaf(params[k], dtype) for k in W.trunk_keys(W.TRUNKS[0], nb) + W.trunk_keys(W.TRUNKS[1], nb) + list(W.ORIGIN_RECON)}
    x, target = x.detach().to(dtype), target.detach().to(dtype)
    ff, fb = leaf(ff, dtype), leaf(fb, dtype)
    b, n, _, h, w = x.shape
    steps = W.propagate([p[k] for k in W.trunk_keys(W.TRUNKS[0], nb)], [p[k] for k in W.trunk_keys(W.TRUNKS[1], nb)], x, ff, fb, nb, rnd)
    recon = [p[k] for k in W.ORIGIN_RECON]
    out = torch.stack([W._OriginRecon.apply(steps[n - 1 - i][:b], steps[i][b:], x[:, i], hot, *recon) for i in range(n)], 1)
    W._charbonnier(out, target).backward()
    return out.detach().contiguous(), W.group_grads("origin", nb, lambda k: p[k].grad), ff.grad, fb.grad


MODEL_GEOM = dict(b=2, n=3, h=16, w=16)
MODEL_WIDTHS = ((64, 2), (32, 2))                        # (F, nb)
# a shift of its own per clip and time step plus sub-pixel noise, as wide_model_ref.case draws them
MODEL_SHIFTS = (((0.0, 0.0), (1.5, -1.0), (-5.0, 3.0)), ((0.0, 0.0), (-4.0, 2.0), (2.0, 1.5)))


@functools.lru_cache(maxsize=None)
def model_case(f, nb, positive=False):
    """wide_model_ref.case("origin", ...) at 16 x 16 -> 64 x 64 (that function is bound to its own 18 x 20 geometry): the same
    recipe for parameters, clips, flows and targets.  Cached: shared, not to be written to."""
    b, n, h, w = (MODEL_GEOM[k] for k in "bnhw")
    g = torch.Generator().manual_seed(seed(24681, 7, f, nb, int(positive)))
    rn = lambda *s: torch.randn(*s, generator=g)
    params = {}
    for tr in W.TRUNKS:
        for k in range(1 + 2 * nb):
            ci = f + 3 if k == 0 else f
            name = W.trunk_keys(tr, nb)[2 * k][:-len(".weight")]
            params[name + ".weight"], params[name + ".bias"] = rn(f, ci, 3, 3) / (3.0 * ci ** 0.5), 0.1 * rn(f)
            if k == 0:
                params[name + ".weight"][:, 3:] *= 2.0
    for name, shape in W.recon_shapes("origin", f).items():
        params[name] = 0.1 * rn(*shape) if name.endswith(".bias") else rn(*shape) / (shape[2] * shape[1] ** 0.5)
    x = torch.rand(b, n, 3, h, w, generator=g)
    mv = torch.tensor(MODEL_SHIFTS, dtype=torch.float32)[:b, :n].view(b, n, 2, 1, 1) + 0.5 * rn(b, n, 2, h, w)
    target = torch.rand(b, n, 3, 4 * h, 4 * w, generator=g) + torch.tensor(W.TARGET_OFFSETS[:b]).view(b, 1, 1, 1, 1)
    if positive:
        for k in params:
            if k.endswith(".weight"):
                params[k] = 0.3 * params[k]
        params = W._raise_biases("origin", params, x, mv[:, 1:], -mv[:, 1:], nb, W.MARGIN)
    return dict(f=f, nb=nb, params=params, x=x, ff=mv[:, 1:].contiguous(), fb=(-mv[:, 1:]).contiguous(), target=target)


@functools.lru_cache(maxsize=None)
def model_reference(f, nb, mode):
    """(case, float64 (d ff, d fb), their yardsticks): the yardstick is the emulation's own rel_max from float64, on the family of
    cases wide_model_ref holds `mode` on (fp32: the positive twins)"""
    c = model_case(f, nb, W.POSITIVE[mode])
    run = lambda dtype, hot: model_step(c["params"], c["x"], c["ff"], c["fb"], c["target"], nb, f, dtype, hot)[2:]
    ref = run(torch.float64, W.R.ident)
    emu = run(*W.MODES[mode])
    return c, ref, tuple(rel_max(e, r) for e, r in zip(emu, ref))


def finite_difference(state, flow, g, idx, eps=1e-6):
    """central difference of sum(g * warp_ref(state, flow)) in flow[idx] (idx into the (n, h, w, 2) layout), float64"""
    x, fl, gd = state.permute(0, 3, 1, 2).double(), flow.permute(0, 2, 3, 1).double().clone(), g.permute(0, 3, 1, 2).double()
    vals = []
    for s in (eps, -eps):
        f2 = fl.clone()
        f2[idx] += s
        vals.append((warp_ref(x, f2) * gd).sum().item())
    return (vals[0] - vals[1]) / (2 * eps)
