"""Float64 reference of the per-frame video network (models/single_image_model.py Result_Model at scale 4, kernel 3) on EFFECTIVE
weights, layer by layer, for csrc/frame_net.h and sr_fn_net_fwd.  Plain torch on the CPU; nothing here is derived from the kernels.

A parameter set `p` is a dict: enc_w (C,3,3,3), enc_b (C), convs = [(w (C,C,3,3), b (C))] * (2 nb + 1) in forward order (block i: 2 i,
2 i + 1; the body's last conv: 2 nb), up_w (C,3,5,5), up_b (3).

    forward(x, p, size=None, rnd=None)   x (N,3,H,W) -> dict(e, t=[..], y=[..], f, D, out): every stage in float64.  rnd: a rounding
                                          applied exactly where the bf16 route stores a value or feeds an MFMA: the frames (the encoder
                                          stages them in the hot dtype), every weight and bias, e, each t, each block output, f.  D and
                                          the resize stay fp32 on the device and unrounded here.
    exact cases                           small-integer frames, weights and biases with one or two non-zeros per weight row, so that
                                          every rounding point is a bf16 value and every fp32 sum is exact in any order: the fp32 and the
                                          bf16 route must then both be torch.equal to forward() up to and including D.  The two-tap
                                          blend after D has the weights (2 d + 1) / (8 H): dyadic only for power-of-two H and W, so the
                                          end-to-end exact cases are 8 x 16 frames; check_exact() verifies all of this and raises
                                          NotExact otherwise.
    rounded cases                         random normal data, PyTorch-sized weights, nothing rounded beforehand.

The conditions named need_* / is_*, the roundings, the seed recipe and the bound of the rounded cases are tests/parity_kit.py's,
shared by all parity suites and pinned by tests/test_parity_kit_host.py.
"""
import functools

import torch
import torch.nn.functional as F

from tests.parity_kit import bf16_round, is_bf16, is_fp32, need_sum, rel_max, seed   # noqa: F401 (bf16_round, rel_max: for the tests)

TH, TW = 8, 32                                           # the block kernel's tile (FnCfg of csrc/frame_net.h)
SIZES = ((1, 1), (3, 3), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1), (5, 70), (8, 16))
E2E_SIZE = (8, 16)


class NotExact(AssertionError):
    pass


def effective(sd, blocks):
    """state_dict of Result_Model(4, C, blocks, 3) -> parameter set in float64 (w = g v / |v| per output channel)"""
    d = {k: v.double() for k, v in sd.items()}

    def wn(prefix):
        v, g = d[prefix + ".weight_v"], d[prefix + ".weight_g"]
        return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1)), d[prefix + ".bias"]

    convs = []
    for i in range(blocks):
        convs += [wn(f"body.{i}.body.0.body.0"), wn(f"body.{i}.body.0.body.2")]
    convs.append(wn(f"body.{blocks}"))
    ew, eb = wn("encoder")
    return dict(enc_w=ew, enc_b=eb, convs=convs, up_w=d["shuf.0.weight"], up_b=d["shuf.0.bias"])


def forward(x, p, size=None, rnd=None):
    r = rnd if rnd is not None else (lambda t: t)
    x = r(x.double())
    e = r(F.conv2d(x, r(p["enc_w"].double()), r(p["enc_b"].double()), padding=1))
    nb = (len(p["convs"]) - 1) // 2
    y, ts, ys = e, [], []
    for i in range(nb):
        (w1, b1), (w2, b2) = p["convs"][2 * i], p["convs"][2 * i + 1]
        t = r(F.relu(F.conv2d(y, r(w1.double()), r(b1.double()), padding=1)))
        y = r(F.conv2d(t, r(w2.double()), r(b2.double()), padding=1) + y)
        ts.append(t)
        ys.append(y)
    wl, bl = p["convs"][2 * nb]
    f = r(F.conv2d(y, r(wl.double()), r(bl.double()), padding=1) + e)
    D = F.conv_transpose2d(f, r(p["up_w"].double()), r(p["up_b"].double()), stride=4)
    h, w = x.shape[-2:]
    size = size if size is not None else (4 * h, 4 * w)
    out = F.interpolate(D, size=size, mode="bilinear")
    return dict(x=x, e=e, t=ts, y=ys, f=f, D=D, out=out)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def _is_int(t):
    return bool((t == t.round()).all())


def _need(cond, msg):
    if not cond:
        raise NotExact(msg)


def _need_sum(name, abs_sum, quantum=1.0):
    """parity_kit.need_sum (sum |terms| < 2^24 quanta), reported as NotExact"""
    try:
        need_sum(name, abs_sum, quantum)
    except ValueError as e:
        raise NotExact(str(e)) from None


def check_exact(case):
    """raises NotExact unless the case is exact on both routes: integers everywhere, every stored tensor a bf16 value, every
    accumulation below 2^24 in absolute sum (integer partial sums of any order are then exact in fp32), and, for power-of-two
    frames, a D small enough that the blend's products and sums are exact too"""
    x, p = case["x"].double(), case["p"]
    flat = [("x", x), ("enc_w", p["enc_w"]), ("enc_b", p["enc_b"]), ("up_w", p["up_w"]), ("up_b", p["up_b"])]
    for j, (w, b) in enumerate(p["convs"]):
        flat += [(f"w{j}", w), (f"b{j}", b)]
    for name, t in flat:
        _need(_is_int(t.double()), f"{name}: not integer")
        _need(is_bf16(t), f"{name}: not a bf16 value")
    r = forward(x, p)
    for name, t in [("e", r["e"]), ("f", r["f"])] + [(f"t{i}", t) for i, t in enumerate(r["t"])] + [(f"y{i}", t) for i, t in enumerate(r["y"])]:
        _need(is_bf16(t), f"{name}: not a bf16 value")

    def abs_sum(xin, w, b, extra=None):
        s = F.conv2d(xin.abs(), w.double().abs(), b.double().abs(), padding=w.shape[-1] // 2)
        return s + (extra.abs() if extra is not None else 0)

    _need_sum("encoder", abs_sum(r["x"], p["enc_w"], p["enc_b"]))
    y = r["e"]
    for i in range(len(r["t"])):
        (w1, b1), (w2, b2) = p["convs"][2 * i], p["convs"][2 * i + 1]
        _need_sum(f"block {i} conv1", abs_sum(y, w1, b1))
        _need_sum(f"block {i} conv2", abs_sum(r["t"][i], w2, b2, y))
        y = r["y"][i]
    wl, bl = p["convs"][-1]
    _need_sum("last conv", abs_sum(y, wl, bl, r["e"]))
    dsum = F.conv_transpose2d(r["f"].abs(), p["up_w"].double().abs(), p["up_b"].double().abs(), stride=4)
    _need_sum("D", dsum)
    h, w = x.shape[-2:]
    if h & (h - 1) == 0 and w & (w - 1) == 0:
        # blend weights are multiples of 1 / (8 h) and 1 / (8 w): the result is an integer multiple of 1 / (64 h w)
        _need_sum("blend", dsum, 1.0 / (64 * h * w))
        _need(is_fp32(r["out"]), "blend: not an fp32 value")
    return r


_seed = functools.partial(seed, 0, 17)


def _sparse(rows, cols, k, nnz, g, vals=(1.0, -1.0, 2.0, -2.0)):
    """(rows, cols, k, k) with `nnz` non-zero taps per row, values from `vals`"""
    w = torch.zeros(rows, cols * k * k, dtype=torch.float64)
    for r in range(rows):
        idx = torch.randperm(cols * k * k, generator=g)[:nnz]
        w[r, idx] = torch.tensor(vals, dtype=torch.float64)[torch.randint(len(vals), (nnz,), generator=g)]
    return w.view(rows, cols, k, k)


def _build_exact(channel, nb, n, h, w, seed, nnz):
    g = torch.Generator().manual_seed(_seed(21, channel, nb, n, h, w, seed, nnz))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    c = channel
    convs = []
    for i in range(2 * nb + 1):
        # conv1 of a block gets biases of both signs (so ReLU cuts some channels and passes others), the rest small ones
        convs.append((_sparse(c, c, 3, min(nnz, 9 * c), g, (1.0, -1.0)), ri(-2, 3, c)))
    p = dict(enc_w=_sparse(c, 3, 3, 2, g), enc_b=ri(-2, 2, c), convs=convs,
             up_w=_sparse(c, 3, 5, 6, g, (1.0, -1.0, 2.0, -2.0, 3.0)), up_b=ri(-3, 3, 3))
    return dict(channel=c, nb=nb, x=ri(0, 3, n, 3, h, w), p=p)


@functools.lru_cache(maxsize=None)
def exact_case(channel, nb, n, h, w, seed=0):
    """the first build (two non-zeros per row, then one) that passes check_exact; the float64 stages ride along as case['ref']"""
    last = None
    for nnz in ((2, 1) if nb <= 2 else (1,)):
        for k in range(12):
            case = _build_exact(channel, nb, n, h, w, seed + 97 * k, nnz)
            try:
                case["ref"] = check_exact(case)
                return case
            except NotExact as e:
                last = e
    raise NotExact(f"no exact case for {(channel, nb, n, h, w)}: {last}")


def spoil(case, how):
    """a copy of an exact case that check_exact must reject"""
    p = dict(case["p"])
    out = dict(case, p=p)
    out.pop("ref", None)
    if how == "fraction":                                   # a weight that is no integer
        w, b = p["convs"][-1]
        w = w.clone()
        w.view(-1)[0] = 0.3
        p["convs"] = list(p["convs"][:-1]) + [(w, b)]
    elif how == "nine_bits":                                # a frame value that bf16 cannot hold
        x = case["x"].clone()
        x.view(-1)[0] = 257.0
        out["x"] = x
    elif how == "overflow":                                 # an accumulation past 2^24
        p["up_b"] = p["up_b"].clone()
        p["up_b"][0] = 2.0 ** 25
    else:
        raise ValueError(how)
    return out


SPOILS = ("fraction", "nine_bits", "overflow")


def padding_case(channel, h, w):
    """conv1 weights zero with b1 = 1, conv2 weights all one: y - x counts the taps of t inside the image, 4 / 6 / 9 times `channel`
    along the border ring (1 block; the encoder is zero, so x = e = 0)"""
    c = channel
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    convs = [(z(c, c, 3, 3), torch.ones(c, dtype=torch.float64)), (torch.ones(c, c, 3, 3, dtype=torch.float64), z(c)), (z(c, c, 3, 3), z(c))]
    p = dict(enc_w=z(c, 3, 3, 3), enc_b=z(c), convs=convs, up_w=z(c, 3, 5, 5), up_b=z(3))
    return dict(channel=c, nb=1, x=torch.ones(1, 3, h, w, dtype=torch.float64), p=p)


def tap_counts(h, w):
    """taps of a zero-padded 3x3 window that fall inside an h x w image"""
    ny = torch.tensor([min(y + 1, h - 1) - max(y - 1, 0) + 1 for y in range(h)], dtype=torch.float64)
    nx = torch.tensor([min(x + 1, w - 1) - max(x - 1, 0) + 1 for x in range(w)], dtype=torch.float64)
    return ny.view(-1, 1) * nx.view(1, -1)


# ---- rounded cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounded_case(channel, nb, n, h, w, seed=0):
    g = torch.Generator().manual_seed(_seed(22, channel, nb, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = channel
    convs = [(rn(c, c, 3, 3) / (3.0 * c ** 0.5), 0.1 * rn(c)) for _ in range(2 * nb + 1)]
    p = dict(enc_w=rn(c, 3, 3, 3) / 27 ** 0.5, enc_b=0.1 * rn(c), convs=convs, up_w=rn(c, 3, 5, 5) / (2.0 * c ** 0.5), up_b=0.1 * rn(3))
    return dict(channel=c, nb=nb, x=torch.rand(n, 3, h, w, generator=g, dtype=torch.float64), p=p)


def state_dict_of(p):
    """a parameter set as a state_dict of Result_Model(4, C, nb, 3): weight_v = w, weight_g = |w| per output channel (the effective
    weight is then w up to rounding); `skip` is left to the caller's model"""
    sd = {}

    def put(prefix, w, b):
        sd[prefix + ".bias"] = b.float()
        sd[prefix + ".weight_g"] = w.flatten(1).norm(dim=1).view(-1, 1, 1, 1).float()
        sd[prefix + ".weight_v"] = w.float()

    nb = (len(p["convs"]) - 1) // 2
    put("encoder", p["enc_w"], p["enc_b"])
    for i in range(nb):
        put(f"body.{i}.body.0.body.0", *p["convs"][2 * i])
        put(f"body.{i}.body.0.body.2", *p["convs"][2 * i + 1])
    put(f"body.{nb}", *p["convs"][2 * nb])
    sd["shuf.0.weight"], sd["shuf.0.bias"] = p["up_w"].float(), p["up_b"].float()
    return sd
