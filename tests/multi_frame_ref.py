"""Float64 reference of the multi-frame video network (models/naive_multi_model_easy.py Naive_model at scale 4, kernel 3, equal block
widths) on EFFECTIVE weights, layer by layer, for csrc/multi_frame.h and sr_mf_net_fwd.  Plain torch on the CPU; nothing here is
derived from the kernels.

A parameter set `p` is a dict: enc_w (C,3,3,3), enc_b (C), blocks = [(w1, b1, w2, b2)] (block 0's w1 is (C, 2C+2, 3, 3) over
cat(flow 2 | warp C | e C), the others (C, C, 3, 3)), dec_w (48,C,3,3), dec_b (48).

    warp(x, flow)                        flow_warp (bilinear, zeros padding, align_corners=True) written out: the sample position of pixel
                                          (y, x) is (x + fx, y + fy) -- the op's normalise / un-normalise round trip is the identity in
                                          real arithmetic (0 on a size-1 axis) --, four taps, a tap outside the image contributes zero
    forward(x, flows, p, rnd=None)       x (B,N,3,H,W), flows (B,N-1,2,H,W) -> dict(e, t0, y=[..], out), frames flattened to B N.
                                          rnd: a rounding applied exactly where the bf16 route stores a value or feeds an MFMA: the
                                          frames as the encoder stages them, every weight and bias, e, the warp result, the flow operand,
                                          each t, each block output.  The decode accumulator, the x4 base (taken from the UNROUNDED fp32
                                          frame) and their sum stay fp32 on the device and unrounded here.
    exact cases                           small-integer frames, sparse +-1 weights, flows on integers or on multiples of 1/4 (then with
                                          frame sizes whose size - 1 is a power of two, so that the position round trip is exact in
                                          fp32): every rounding point is a bf16 value and every fp32 sum is exact in any order, the x4
                                          base is a multiple of 1/64.  Both hot dtypes must then be torch.equal to forward().
                                          check_exact() verifies all of this ON THE FLOAT64 SIDE ALONE and raises NotExact otherwise.
    rounded cases                         random normal data, PyTorch-sized weights, flows uniform in +-3 px.
"""
import functools

import torch
import torch.nn.functional as F

from tests.frame_net_ref import NotExact, SIZES, TH, TW, _need, _need_sum, _sparse, tap_counts   # noqa: F401
from tests.parity_kit import bf16_round, is_bf16, is_fp32, rel_max, seed   # noqa: F401


def effective(sd, nb):
    """state_dict of Naive_model(4, status = nb blocks of [C, C, 3]) -> parameter set in float64 (encode / decode: w = g v / |v|)"""
    d = {k: v.double() for k, v in sd.items()}

    def wn(prefix):
        v, g = d[prefix + ".weight_v"], d[prefix + ".weight_g"]
        return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1)), d[prefix + ".bias"]

    blocks = [(d[f"body.{i}.body.0.weight"], d[f"body.{i}.body.0.bias"], d[f"body.{i}.body.2.weight"], d[f"body.{i}.body.2.bias"])
              for i in range(nb)]
    ew, eb = wn("encode")
    dw, db = wn("decode")
    return dict(enc_w=ew, enc_b=eb, blocks=blocks, dec_w=dw, dec_b=db)


def state_dict_of(p):
    """a parameter set as the trainable part of a state_dict of Naive_model: weight_v = w, weight_g = |w| per output channel"""
    sd = {}
    for name, w, b in (("encode", p["enc_w"], p["enc_b"]), ("decode", p["dec_w"], p["dec_b"])):
        sd[name + ".bias"] = b.float()
        sd[name + ".weight_g"] = w.flatten(1).norm(dim=1).view(-1, 1, 1, 1).float()
        sd[name + ".weight_v"] = w.float()
    for i, (w1, b1, w2, b2) in enumerate(p["blocks"]):
        sd[f"body.{i}.body.0.weight"], sd[f"body.{i}.body.0.bias"] = w1.float(), b1.float()
        sd[f"body.{i}.body.2.weight"], sd[f"body.{i}.body.2.bias"] = w2.float(), b2.float()
    return sd


def warp(x, flow):
    """x (n, c, h, w), flow (n, 2, h, w) with channel 0 = dx, float64"""
    n, c, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")

    def pos(g, size):
        # in real arithmetic the round trip ((2 g / max(size - 1, 1) - 1) + 1) / 2 (size - 1) is g itself, or 0 on a size-1 axis
        return g if size > 1 else torch.zeros_like(g)

    px, py = pos(gx + flow[:, 0], w), pos(gy + flow[:, 1], h)
    x0, y0 = px.floor(), py.floor()
    wx, wy = px - x0, py - y0
    out = torch.zeros_like(x)
    flat = x.reshape(n, c, h * w)
    for dy, dx, wt in ((0, 0, (1 - wx) * (1 - wy)), (0, 1, wx * (1 - wy)), (1, 0, (1 - wx) * wy), (1, 1, wx * wy)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long().view(n, 1, h * w).expand(n, c, h * w)
        out = out + (wt * ok).view(n, 1, h, w) * flat.gather(2, idx).view(n, c, h, w)
    return out


def base_x4(x):
    """F.interpolate(x, scale_factor=4, 'bilinear', align_corners=False) in x's dtype"""
    return F.interpolate(x, scale_factor=4, mode="bilinear", align_corners=False)


def forward(x, flows, p, rnd=None):
    r = rnd if rnd is not None else (lambda t: t)
    b, n, _, h, w = x.shape
    x = x.double()
    frames = x.reshape(b * n, 3, h, w)
    e = r(F.conv2d(r(frames), r(p["enc_w"].double()), r(p["enc_b"].double()), padding=1))
    ev = e.view(b, n, -1, h, w)
    fl = torch.zeros(b, n, 2, h, w, dtype=torch.float64)
    wp = ev.clone()                                           # frame 0 of every clip: warp = e_0, flow = 0
    if n > 1:
        fl[:, 1:] = flows.double()
        wp[:, 1:] = warp(ev[:, :-1].reshape(b * (n - 1), -1, h, w), flows.double().reshape(b * (n - 1), 2, h, w)).view(b, n - 1, -1, h, w)
    cat = torch.cat((r(fl.view(b * n, 2, h, w)), r(wp.view(b * n, -1, h, w)), e), dim=1)
    w1, b1, w2, b2 = p["blocks"][0]
    t0 = r(F.relu(F.conv2d(cat, r(w1.double()), r(b1.double()), padding=1)))
    y = r(F.conv2d(t0, r(w2.double()), r(b2.double()), padding=1) + e)
    ys, ts = [y], [t0]
    for w1, b1, w2, b2 in p["blocks"][1:]:
        t = r(F.relu(F.conv2d(y, r(w1.double()), r(b1.double()), padding=1)))
        y = r(F.conv2d(t, r(w2.double()), r(b2.double()), padding=1) + y)
        ts.append(t)
        ys.append(y)
    dec = F.conv2d(y, r(p["dec_w"].double()), r(p["dec_b"].double()), padding=1)
    base = base_x4(frames)
    out = F.pixel_shuffle(dec, 4) + base
    return dict(x=frames, e=e, flow=fl.view(b * n, 2, h, w), warp=wp.view(b * n, -1, h, w), cat=cat, t=ts, y=ys, dec=dec, base=base, out=out)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def _is_multiple(t, q):
    s = t.double() / q
    return bool((s == s.round()).all())


def check_exact(case):
    """raises NotExact unless the case is exact on both routes, judged on the float64 side alone: every operand a bf16 value on a
    1/16 lattice (flows on 1/4), sample positions whose fp32 round trip is exact, every accumulation below 2^24 quanta of 1/16 (the
    x4 base: of 1/64, added to the decode accumulator in fp32)"""
    x, flows, p = case["x"].double(), case["flows"].double(), case["p"]
    b, n, _, h, w = x.shape
    flat = [("x", x), ("flows", flows), ("enc_w", p["enc_w"]), ("enc_b", p["enc_b"]), ("dec_w", p["dec_w"]), ("dec_b", p["dec_b"])]
    for j, blk in enumerate(p["blocks"]):
        flat += [(f"blk{j}.{i}", t) for i, t in enumerate(blk)]
    for name, t in flat:
        _need(_is_multiple(t, 0.25 if name == "flows" else 1.0), f"{name}: off its lattice")
        _need(is_bf16(t), f"{name}: not a bf16 value")
    if n > 1 and not _is_multiple(flows, 1.0):
        # fractional positions: 2 g / (size - 1) must be exact in fp32, i.e. size - 1 a power of two (the warp section)
        _need((h - 1) & (h - 2) == 0 and (w - 1) & (w - 2) == 0 and h > 1 and w > 1, "quarter flows need size - 1 = 2^k")
    _need(bool((flows.abs() <= 2.0 ** 20).all()), "flow too large for an exact fp32 position")
    _need(bool(position_ok(flows, h, w).all()), "a sample position whose fp32 round trip is not exact")
    r = forward(x, flows, p)
    q = 1.0 / 16
    for name, t in [("e", r["e"]), ("warp", r["warp"]), ("flow", r["flow"])] + [(f"t{i}", t) for i, t in enumerate(r["t"])] + \
                   [(f"y{i}", t) for i, t in enumerate(r["y"])]:
        _need(_is_multiple(t, q), f"{name}: off the 1/16 lattice")
        _need(is_bf16(t), f"{name}: not a bf16 value")

    def abs_sum(xin, wgt, bias, extra=None):
        s = F.conv2d(xin.abs(), wgt.double().abs(), bias.double().abs(), padding=1)
        return s + (extra.abs() if extra is not None else 0)

    _need_sum("encoder", abs_sum(r["x"], p["enc_w"], p["enc_b"]))
    _need_sum("warp", r["e"].abs().max().view(1) * 4, q)
    src, res = r["cat"], r["e"]
    for i, (w1, b1, w2, b2) in enumerate(p["blocks"]):
        _need_sum(f"block {i} conv1", abs_sum(src, w1, b1), q)
        _need_sum(f"block {i} conv2", abs_sum(r["t"][i], w2, b2, res), q)
        src = res = r["y"][i]
    dsum = F.pixel_shuffle(abs_sum(r["y"][-1], p["dec_w"], p["dec_b"]), 4) + r["base"].abs()
    _need_sum("decode + base", dsum, 1.0 / 64)
    _need(_is_multiple(r["base"], 1.0 / 64) and is_fp32(r["out"]), "base: off the 1/64 lattice")
    return r


_seed = functools.partial(seed, 0, 23)
FLOW_KINDS = ("int", "zero", "far", "quarter", "inward")


def position_ok(flows, h, w):
    """bool per flow component: the op's fp32 normalise / un-normalise round trip (2 g / (size - 1) - 1, then ((v + 1) / 2) (size - 1),
    each operation rounded once) returns the sample position g = grid + flow exactly, or g is more than a pixel outside the image (all
    taps are zero whatever the rounding).  Elsewhere fp32 and float64 weigh the taps differently by an ulp.  A size-1 axis has
    position 0 whatever the flow says."""
    ok = torch.ones_like(flows, dtype=torch.bool)
    for k, size in ((0, w), (1, h)):
        if size == 1:
            continue
        grid = torch.arange(size, dtype=torch.float32)
        g = (grid.view(1, -1) if k == 0 else grid.view(-1, 1)) + flows[:, :, k].float()
        v = (2.0 * g) / torch.full_like(g, float(size - 1)) - 1.0       # tensor / tensor: the IEEE quotient
        ok[:, :, k] = (((v + 1.0) * 0.5) * float(size - 1) == g) | (g <= -2.0) | (g >= size + 1.0)
    return ok


def settle_flows(flows, h, w):
    """flows with every component that fails position_ok moved by the smallest whole number of pixels that passes"""
    out = flows.clone()
    for delta in sorted(range(-max(h, w) - 2, max(h, w) + 3), key=abs):
        bad = ~position_ok(out, h, w)
        if not bool(bad.any()):
            return out
        out = torch.where(bad & position_ok(flows + delta, h, w), flows + delta, out)
    assert bool(position_ok(out, h, w).all())
    return out


def make_flows(kind, b, n, h, w, g):
    return settle_flows(_make_flows(kind, b, n, h, w, g), h, w)


def _make_flows(kind, b, n, h, w, g):
    """(b, n - 1, 2, h, w) float64.  int: integers in +-3 (they cross tile borders at every tile edge); zero; far: integers, a third of
    them +-(40 .. 1000) and so far outside the image; quarter: multiples of 1/4 in +-3; inward: 2 px towards the image centre, so a
    halo-ring pixel warped with a clamped flow -- instead of zeroed -- would sample the non-zero interior"""
    shape = (b, max(n - 1, 0), 2, h, w)
    if kind == "zero":
        return torch.zeros(shape, dtype=torch.float64)
    if kind == "int":
        return torch.randint(-3, 4, shape, generator=g).double()
    if kind == "quarter":
        return torch.randint(-12, 13, shape, generator=g).double() / 4
    if kind == "far":
        near = torch.randint(-3, 4, shape, generator=g).double()
        big = torch.tensor([40.0, -40.0, 64.0, -200.0, 1000.0, -1000.0], dtype=torch.float64)[torch.randint(6, shape, generator=g)]
        return torch.where(torch.randint(3, shape, generator=g) == 0, big, near)
    if kind == "inward":
        f = torch.zeros(shape, dtype=torch.float64)
        f[:, :, 0] = torch.where(torch.arange(w) < w / 2, 2.0, -2.0).view(1, 1, 1, w)
        f[:, :, 1] = torch.where(torch.arange(h) < h / 2, 2.0, -2.0).view(1, 1, h, 1)
        return f
    raise ValueError(kind)


def _build_exact(channel, nb, b, n, h, w, kind, sd, nnz):
    g = torch.Generator().manual_seed(_seed(31, channel, nb, b, n, h, w, FLOW_KINDS.index(kind), sd, nnz))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    c = channel
    pm = (1.0, -1.0)
    # far flows reach 1000: with a live flow column t would need more than bf16's eight bits, so that kind leaves the column zero
    w1 = _sparse(c, 2 * c + 2, 3, min(nnz, 9 * c), g, pm)
    if kind == "far":
        w1[:, :2] = 0
    elif c >= 2:
        w1[0, 0, 1, 1], w1[1, 1, 0, 2] = 1.0, -1.0                      # the flow group is live in every other kind
    blocks = [(w1, ri(-1, 2, c), _sparse(c, c, 3, 1, g, pm), ri(-1, 1, c))]
    for _ in range(nb - 1):
        blocks.append((_sparse(c, c, 3, 1, g, pm), ri(-2, 2, c), _sparse(c, c, 3, 1, g, pm), ri(-1, 1, c)))
    p = dict(enc_w=_sparse(c, 3, 3, 2, g, pm), enc_b=ri(-1, 2, c), blocks=blocks, dec_w=_sparse(48, c, 3, min(3, 9 * c), g, (1.0, -1.0, 2.0)),
             dec_b=ri(-3, 3, 48))
    x = ri(0, 1, b, n, 3, h, w)
    return dict(channel=c, nb=nb, B=b, N=n, x=x, flows=make_flows(kind, b, n, h, w, g), p=p, kind=kind)


@functools.lru_cache(maxsize=None)
def exact_case(channel, nb, b, n, h, w, kind="int", sd=0):
    """the first build that passes check_exact; the float64 stages ride along as case['ref']"""
    last = None
    for nnz in (2, 1):
        for k in range(12):
            case = _build_exact(channel, nb, b, n, h, w, kind, sd + 97 * k, nnz)
            try:
                case["ref"] = check_exact(case)
                return case
            except NotExact as e:
                last = e
    raise NotExact(f"no exact case for {(channel, nb, b, n, h, w, kind)}: {last}")


def spoil(case, how):
    """a copy of an exact case that check_exact must reject"""
    p = dict(case["p"])
    out = dict(case, p=p)
    out.pop("ref", None)
    if how == "fraction":
        p["dec_w"] = p["dec_w"].clone()
        p["dec_w"].view(-1)[0] = 0.3
    elif how == "eighth_flow":                              # a flow off the 1/4 lattice
        f = case["flows"].clone()
        f.view(-1)[0] = 0.125
        out["flows"] = f
    elif how == "nine_bits":
        x = case["x"].clone()
        x.view(-1)[0] = 257.0
        out["x"] = x
    elif how == "overflow":
        p["dec_b"] = p["dec_b"].clone()
        p["dec_b"][0] = 2.0 ** 25
    else:
        raise ValueError(how)
    return out


SPOILS = ("fraction", "eighth_flow", "nine_bits", "overflow")


def padding_case(channel, h, w):
    """block 0 with conv1 weights zero and b1 = 1, conv2 weights all one: y - e counts the taps of t inside the image, 4 / 6 / 9 times
    `channel` along the border ring (the encoder is zero, so e = 0; two frames, the second one warped by integer flows)"""
    c = channel
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    blocks = [(z(c, 2 * c + 2, 3, 3), torch.ones(c, dtype=torch.float64), torch.ones(c, c, 3, 3, dtype=torch.float64), z(c))]
    p = dict(enc_w=z(c, 3, 3, 3), enc_b=z(c), blocks=blocks, dec_w=z(48, c, 3, 3), dec_b=z(48))
    g = torch.Generator().manual_seed(_seed(32, c, h, w))
    return dict(channel=c, nb=1, B=1, N=2, x=torch.ones(1, 2, 3, h, w, dtype=torch.float64), flows=make_flows("int", 1, 2, h, w, g), p=p,
                kind="int")


# ---- rounded cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounded_case(channel, nb, b, n, h, w, sd=0):
    g = torch.Generator().manual_seed(_seed(33, channel, nb, b, n, h, w, sd))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = channel
    blocks = []
    for i in range(nb):
        cin = 2 * c + 2 if i == 0 else c
        blocks.append((rn(c, cin, 3, 3) / (3.0 * cin ** 0.5), 0.1 * rn(c), rn(c, c, 3, 3) / (3.0 * c ** 0.5), 0.1 * rn(c)))
    p = dict(enc_w=rn(c, 3, 3, 3) / 27 ** 0.5, enc_b=0.1 * rn(c), blocks=blocks, dec_w=rn(48, c, 3, 3) / (3.0 * c ** 0.5), dec_b=0.1 * rn(48))
    x = torch.rand(b, n, 3, h, w, generator=g, dtype=torch.float64)
    flows = 6.0 * torch.rand(b, max(n - 1, 0), 2, h, w, generator=g, dtype=torch.float64) - 3.0
    return dict(channel=c, nb=nb, B=b, N=n, x=x, flows=flows, p=p)
