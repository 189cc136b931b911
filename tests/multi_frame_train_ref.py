"""Float64 forward AND backward of the multi-frame video network (Naive_model at scale 4, kernel 3, equal widths) on EFFECTIVE
weights, for the HIP training route (sr_mf_net_train_fwd / sr_mf_net_bwd).  Built on tests/multi_frame_ref.py (the forward, the
parameter sets, the flows, the case generators) and tests/parity_kit.py; plain torch on the CPU, written out by hand (no autograd),
nothing here is derived from the kernels.

    backward(x, flows, p, gout, rnd=None) -> dict: the forward's stages (fw) and every gradient the route stores or returns:
        dD, dy (the tail's input gradient), dt[i], dx[i] (block i >= 1's input gradient), direct, dwarp, de and `grads`, a parameter
        set of p's structure (enc_w, enc_b, blocks = [(w1, b1, w2, b2)], dec_w, dec_b).

The chain, as DESIGN 17 states it:  dD = PixelUnshuffle(gout) (the x4 bilinear base has no parameters, the frames get no gradient);
dy = decode^T(dD);  per block nb - 1 .. 1: dt = conv2^T(dy), dx = dy + conv1^T(dt * [t > 0]);  block 0: dt = conv2^T(dy),
direct = dy + conv1_e^T(dt * mask), dwarp = conv1_warp^T(dt * mask) (the flow group has no data gradient: flows get none);
frame n = b N + i:  de_n = direct_n + (i == 0 ? dwarp_n : 0) + (i < N - 1 ? warp^T(dwarp_{n+1}) : 0)  -- frame 0's warp operand IS
e_0, frame n + 1's sampled e_n; warp^T scatters every output pixel's gradient onto its (at most) four taps with the forward's
weights.  Weight gradients contract the conv's input with its (masked) output gradient, bias gradients sum it; block 0's dW1 is one
(C, 2C + 2, 3, 3) tensor over cat(flow, warp, e).

Rounding points (rnd = parity_kit.bf16_round gives the bf16 route's yardstick).  Forward: as multi_frame_ref.forward.  Backward: dD
(stored, and the MFMA operand of dy and of decode's weight gradient), dy, every dt and dx, direct, dwarp and de as they are stored and
fed to the next MFMA; dt * mask is dt's rounding masked, no new rounding; the frames as the encoder's weight gradient stages them.
Accumulations are fp32 on the device and float64 here.

Exact cases: multi_frame_ref.exact_case supplies integer frames, sparse +-1 weights and flows whose forward is exact; the pixel
un-shuffle is a permutation, so a sparse small-integer OUTPUT gradient gives an integer dD in both hot dtypes and the whole backward
chain stays on small dyadic values (integers with integer flows, multiples of 1/16 with quarter-pixel flows): every stage of both
dtypes is held exactly, from the output gradient on.  check_exact_grad() verifies that on the float64 side alone.
"""
import functools

import torch
import torch.nn.functional as F

from tests import multi_frame_ref as M
from tests.parity_kit import is_bf16, is_fp32, lowbit, need_sum, seed

_seed = functools.partial(seed, 0, 29)


def _conv_t(g, w):
    """input gradient of conv2d(., w, padding=1)"""
    return F.conv_transpose2d(g, w, padding=1)


def _conv_w(xin, g):
    """weight gradient of conv2d(xin, w (co, ci, 3, 3), padding=1) for the output gradient g"""
    return torch.nn.grad.conv2d_weight(xin, (g.shape[1], xin.shape[1], 3, 3), g, padding=1)


def warp_t(g, flow):
    """the transpose of multi_frame_ref.warp: g (n, c, h, w) is the gradient at the warp's output, the result the gradient at its
    input -- every output pixel's gradient scattered onto its four taps with the forward's weights (taps outside the image drop)"""
    n, c, h, w = g.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    px = gx + flow[:, 0] if w > 1 else torch.zeros_like(flow[:, 0])
    py = gy + flow[:, 1] if h > 1 else torch.zeros_like(flow[:, 1])
    x0, y0 = px.floor(), py.floor()
    wx, wy = px - x0, py - y0
    out = torch.zeros(n, c, h * w, dtype=torch.float64)
    for dy, dx, wt in ((0, 0, (1 - wx) * (1 - wy)), (0, 1, wx * (1 - wy)), (1, 0, (1 - wx) * wy), (1, 1, wx * wy)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long().view(n, 1, h * w).expand(n, c, h * w)
        out.scatter_add_(2, idx, ((wt * ok).view(n, 1, h, w) * g).reshape(n, c, h * w))
    return out.view(n, c, h, w)


def backward(x, flows, p, gout, rnd=None):
    r = rnd if rnd is not None else (lambda t: t)
    fw = M.forward(x, flows, p, rnd=rnd)
    b, n, _, h, w = x.shape
    nb, c = len(p["blocks"]), p["enc_w"].shape[0]
    blk = [tuple(r(t.double()) for t in bk) for bk in p["blocks"]]
    dD = r(F.pixel_unshuffle(gout.double().reshape(b * n, 3, 4 * h, 4 * w), 4))
    dy = r(_conv_t(dD, r(p["dec_w"].double())))
    g_dec = (_conv_w(fw["y"][-1], dD), dD.sum((0, 2, 3)))
    gb = [None] * nb
    dts, dxs, dy_tail = [None] * nb, [None] * nb, dy
    for i in range(nb - 1, 0, -1):
        w1, _, w2, _ = blk[i]
        dt = r(_conv_t(dy, w2))
        dtm = dt * (fw["t"][i] > 0)
        dx = r(dy + _conv_t(dtm, w1))
        gb[i] = (_conv_w(fw["y"][i - 1], dtm), dtm.sum((0, 2, 3)), _conv_w(fw["t"][i], dy), dy.sum((0, 2, 3)))
        dts[i], dxs[i], dy = dt, dx, dx
    w1, _, w2, _ = blk[0]
    dt = r(_conv_t(dy, w2))
    dtm = dt * (fw["t"][0] > 0)
    direct = r(dy + _conv_t(dtm, w1[:, 2 + c:]))
    dwarp = r(_conv_t(dtm, w1[:, 2:2 + c]))
    gb[0] = (_conv_w(fw["cat"], dtm), dtm.sum((0, 2, 3)), _conv_w(fw["t"][0], dy), dy.sum((0, 2, 3)))
    dts[0] = dt
    de = direct.view(b, n, c, h, w).clone()
    dwv = dwarp.view(b, n, c, h, w)
    de[:, 0] += dwv[:, 0]
    if n > 1:
        back = warp_t(dwv[:, 1:].reshape(b * (n - 1), c, h, w), flows.double().reshape(b * (n - 1), 2, h, w))
        de[:, :-1] += back.view(b, n - 1, c, h, w)
    de = r(de.view(b * n, c, h, w))
    grads = dict(enc_w=_conv_w(r(fw["x"]), de), enc_b=de.sum((0, 2, 3)), blocks=gb, dec_w=g_dec[0], dec_b=g_dec[1])
    return dict(fw=fw, dD=dD, dy=dy_tail, dt=dts, dx=dxs, direct=direct, dwarp=dwarp, de=de, grads=grads)


def flat_grads(g):
    """[(name, tensor)] in the order of sr_mf_net_bwd's grads vector (packing.mf_grad_sizes): blocks, decode, encoder"""
    rows = []
    for i, bk in enumerate(g["blocks"]):
        rows += [(f"blk{i}.w1", bk[0]), (f"blk{i}.b1", bk[1]), (f"blk{i}.w2", bk[2]), (f"blk{i}.b2", bk[3])]
    return rows + [("dec_w", g["dec_w"]), ("dec_b", g["dec_b"]), ("enc_w", g["enc_w"]), ("enc_b", g["enc_b"])]


def param_grads(sd, nb, g):
    """gradients of the EFFECTIVE tensors -> {state_dict key: gradient} through the weight norm w = g v / |v| of encode / decode
    (float64 autograd on the small parameter tensors, as the route leaves it to torch)"""
    out = {}
    for i, bk in enumerate(g["blocks"]):
        out[f"body.{i}.body.0.weight"], out[f"body.{i}.body.0.bias"], out[f"body.{i}.body.2.weight"], out[f"body.{i}.body.2.bias"] = bk
    for prefix, dw, db in (("encode", g["enc_w"], g["enc_b"]), ("decode", g["dec_w"], g["dec_b"])):
        v = sd[prefix + ".weight_v"].double().requires_grad_(True)
        gg = sd[prefix + ".weight_g"].double().requires_grad_(True)
        wgt = v * (gg / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
        out[prefix + ".weight_v"], out[prefix + ".weight_g"] = torch.autograd.grad(wgt, (v, gg), dw)
        out[prefix + ".bias"] = db
    return out


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def images(res):
    """[(name, tensor)]: every gradient image the route stores"""
    imgs = [("dD", res["dD"]), ("dy", res["dy"]), ("direct", res["direct"]), ("dwarp", res["dwarp"]), ("de", res["de"])]
    imgs += [(f"dt{i}", t) for i, t in enumerate(res["dt"])] + [(f"dx{i}", t) for i, t in enumerate(res["dx"]) if t is not None]
    return imgs


def exact_out_grad(bn, h, w, sd=0, count=8):
    """(bn, 3, 4h, 4w) float64: `count` small integers at random places, the four corners always among them"""
    g = torch.Generator().manual_seed(_seed(31, bn, h, w, sd, count))
    out = torch.zeros(bn, 3, 4 * h, 4 * w, dtype=torch.float64)
    vals = torch.tensor([1.0, -1.0, 2.0, -2.0, 3.0], dtype=torch.float64)
    ri = lambda hi: int(torch.randint(hi, (1,), generator=g))
    spots = [(0, 0), (0, 4 * w - 1), (4 * h - 1, 0), (4 * h - 1, 4 * w - 1)] + [(ri(4 * h), ri(4 * w)) for _ in range(count)]
    for k, (yy, xx) in enumerate(spots):
        out[k % bn, ri(3), yy, xx] = vals[ri(5)]
    return out


def check_exact_grad(case, res, hot_is_bf16):
    """raises M.NotExact unless every stored gradient is a value of the hot dtype and every sum (the data gradients', the warp
    transpose's, the weight and bias gradients') is exact in fp32 in any order"""
    ok = is_bf16 if hot_is_bf16 else is_fp32
    M.check_exact(case)                                    # the forward's own conditions: the backward reads its saved images
    imgs = images(res)
    for name, t in imgs:
        if not ok(t):
            raise M.NotExact(f"{name}: not a value of the hot dtype")
    quantum = min(1.0 / 16, min(float(lowbit(t).min()) for _, t in imgs))      # the forward's lattice is 1/16 (multi_frame_ref)
    a = lambda t: t.double().abs()
    fw, p = res["fw"], case["p"]
    nb, c = len(p["blocks"]), p["enc_w"].shape[0]
    b, n, _, h, w = case["x"].shape
    sums = [("dy", _conv_t(a(res["dD"]), a(p["dec_w"]))), ("dW decode", _conv_w(a(fw["y"][-1]), a(res["dD"]))),
            ("dW encoder", _conv_w(a(fw["x"]), a(res["de"])))]
    dy = res["dy"]
    for i in range(nb - 1, -1, -1):
        w1, _, w2, _ = p["blocks"][i]
        dtm = a(res["dt"][i])
        xin = fw["y"][i - 1] if i else fw["cat"]
        sums += [(f"dt{i}", _conv_t(a(dy), a(w2))), (f"dW2 {i}", _conv_w(a(fw["t"][i]), a(dy))), (f"dW1 {i}", _conv_w(a(xin), dtm))]
        if i:
            sums.append((f"dx{i}", a(dy) + _conv_t(dtm, a(w1))))
            dy = res["dx"][i]
        else:
            sums += [("direct", a(dy) + _conv_t(dtm, a(w1[:, 2 + c:]))), ("dwarp", _conv_t(dtm, a(w1[:, 2:2 + c])))]
    des = a(res["direct"]).view(b, n, c, h, w).clone()
    dwv = a(res["dwarp"]).view(b, n, c, h, w)
    des[:, 0] += dwv[:, 0]
    if n > 1:
        des[:, :-1] += warp_t(dwv[:, 1:].reshape(-1, c, h, w), case["flows"].double().reshape(-1, 2, h, w)).view(b, n - 1, c, h, w)
    sums.append(("de", des))
    sums += [(f"db of {name}", a(t).sum((0, 2, 3))) for name, t in imgs]
    try:
        for name, s in sums:
            need_sum(name, s, quantum)
    except ValueError as e:
        raise M.NotExact(str(e)) from None
    return res


@functools.lru_cache(maxsize=None)
def exact_grad_case(channel, nb, b, n, h, w, kind="int", hot_is_bf16=True, sd=0):
    """(forward case, gout, backward result): the first sparse integer output gradient that passes check_exact_grad"""
    case = M.exact_case(channel, nb, b, n, h, w, kind)
    last = None
    for count in (8, 4, 1, 0):
        for k in range(6):
            gout = exact_out_grad(b * n, h, w, sd + 37 * k, count)
            try:
                return case, gout, check_exact_grad(case, backward(case["x"], case["flows"], case["p"], gout), hot_is_bf16)
            except M.NotExact as e:
                last = e
    raise M.NotExact(f"no exact gradient case for {(channel, nb, b, n, h, w, kind)}: {last}")


def spoil_grad(gout, how):
    """a copy of an exact output gradient that check_exact_grad must reject"""
    g = gout.clone()
    if how == "fraction":                                  # nine significant bits: not a bf16 value
        g.view(-1)[0] = 1.0 + 2.0 ** -8
    elif how == "overflow":                                # an fp32 sum that is not exact
        g.view(-1)[0] = 2.0 ** 25
        g.view(-1)[1] = 1.0
    else:
        raise ValueError(how)
    return g


GRAD_SPOILS = ("fraction", "overflow")


def converging_flows(b, n, h, w):
    """integer flows that put every output pixel of a 2 x 2 cell on the cell's top-left source pixel: four outputs per source"""
    f = torch.zeros(b, max(n - 1, 0), 2, h, w, dtype=torch.float64)
    f[:, :, 0] = -(torch.arange(w) % 2).double().view(1, 1, 1, w)
    f[:, :, 1] = -(torch.arange(h) % 2).double().view(1, 1, h, 1)
    return f
