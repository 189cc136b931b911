"""Float64 forward AND backward of the per-frame video network (Result_Model at scale 4, kernel 3) on EFFECTIVE weights, for the HIP
training route (sr_fn_net_train_fwd / sr_fn_net_bwd).  Built on tests/frame_net_ref.py (the forward, the parameter sets, the case
generators); plain torch on the CPU, nothing here is derived from the kernels.

    backward(x, p, gout, rnd=None)   -> dict: the forward's stages (fw) and every gradient the route produces or passes on:
        dD, df, dz (the last conv's input gradient), dt[i], dx[i] (block i's input gradient), de, and `grads`, a parameter set of the
        same structure as p (enc_w, enc_b, convs, up_w, up_b).

The chain, as DESIGN 16 states it:  dD = resize^T(gout);  df = up^T(dD);  dz = last^T(df);  per block, from the last to the first,
dt = conv2^T(dy), dx = dy + conv1^T(dt * [t > 0]);  de = dx_0 + df.  Weight gradients contract the conv's input with its output
gradient, bias gradients sum the output gradient (the upsampler's: sum of gout, since the resize's weights sum to one).

Rounding points (rnd = parity_kit.bf16_round gives the bf16 route's yardstick).  Forward, as frame_net_ref.forward: the frames,
every weight and bias, e, every t, every block output, f.  Backward: dD as the MFMA operand of df and dW_up (db_up sums the
unrounded gout in an fp32 accumulator: modelled as fp32 row sums added row after row, the one tensor no MFMA operand touches); df, dz, every dt and every dx as they are stored and fed to the next MFMA; dt * mask is dt's rounding
masked, no new rounding; de.  Accumulations are fp32 on the device and float64 here.

Exact cases: frame_net_ref.exact_case supplies integer frames and parameters whose forward is exact.  exact_grad_case() adds an
integer df (for the conv stages, both dtypes) whose whole backward chain stays on bf16 values, and exact_out_grad() a sparse
small-integer output gradient on the rows and columns 0, 1, 4H - 2, 4H - 1 and every 4y.  The resize's weights are multiples of
1 / (8H) and 1 / (8W): dD then has log2(64 H W) fraction bits -- an fp32 value at every power-of-two size, a bf16 value only for
H W <= 4, which is why the bf16 upsampler stage is held exactly at 1 x 1, 2 x 2 and 1 x 4 and the fp32 one also at 8 x 16.
"""
import functools

import torch
import torch.nn.functional as F

from tests import frame_net_ref as R
from tests.parity_kit import is_bf16, is_fp32, lowbit, need_sum, seed

_seed = functools.partial(seed, 0, 19)


def _conv_t(g, w):
    """input gradient of conv2d(., w, padding=1)"""
    return F.conv_transpose2d(g, w, padding=1)


def _conv_w(xin, g, k=3):
    """weight gradient of conv2d(xin, w (co, ci, k, k), padding=k // 2) for the output gradient g"""
    return torch.nn.grad.conv2d_weight(xin, (g.shape[1], xin.shape[1], k, k), g, padding=k // 2)


def backward(x, p, gout, rnd=None, df=None):
    """df given: the chain starts there (gout may be None; dD, up_w and up_b gradients are then absent)"""
    r = rnd if rnd is not None else (lambda t: t)
    fw = R.forward(x, p, rnd=rnd)
    nb = len(fw["t"])
    w = [r(wj.double()) for wj, _ in p["convs"]]
    out = dict(fw=fw)
    g_up_w = g_up_b = None
    if df is None:
        gout = gout.double()
        D = fw["D"].detach().requires_grad_(True)
        dD, = torch.autograd.grad(F.interpolate(D, size=gout.shape[-2:], mode="bilinear"), D, gout)
        dDr = r(dD)
        up_w = r(p["up_w"].double())
        df = F.conv2d(dDr, up_w, stride=4)                                     # conv_transpose2d's weight (C, 3, 5, 5) read as (out, in)
        g_up_w = torch.nn.grad.conv2d_weight(dDr, tuple(up_w.shape), fw["f"], stride=4)
        g_up_b = gout.sum((0, 2, 3))
        if rnd is not None:                                                    # an fp32 accumulator taking the rows one after the other
            acc = torch.zeros(3, dtype=torch.float32)
            for row in gout.float().permute(0, 2, 1, 3).reshape(-1, 3, gout.shape[-1]):
                acc = acc + row.sum(-1)                                        # (torch's cumsum would accumulate in float64)
            g_up_b = acc.double()
        out.update(dD=dD)
    df = r(df.double())
    ys = [fw["e"]] + fw["y"]                                                   # block i's input; ys[nb]: the last conv's input
    gc = [None] * (2 * nb + 1)
    dz = r(_conv_t(df, w[2 * nb]))
    gc[2 * nb] = (_conv_w(ys[nb], df), df.sum((0, 2, 3)))
    dy, dts, dxs = dz, [None] * nb, [None] * nb
    for i in range(nb - 1, -1, -1):
        dt = r(_conv_t(dy, w[2 * i + 1]))
        gc[2 * i + 1] = (_conv_w(fw["t"][i], dy), dy.sum((0, 2, 3)))
        dtm = dt * (fw["t"][i] > 0)
        dx = r(dy + _conv_t(dtm, w[2 * i]))
        gc[2 * i] = (_conv_w(ys[i], dtm), dtm.sum((0, 2, 3)))
        dts[i], dxs[i], dy = dt, dx, dx
    de = r(dy + df)
    out.update(df=df, dz=dz, dt=dts, dx=dxs, de=de,
               grads=dict(enc_w=_conv_w(fw["x"], de), enc_b=de.sum((0, 2, 3)), convs=gc, up_w=g_up_w, up_b=g_up_b))
    return out


def flat_grads(g):
    """[(name, tensor)] in the order of sr_fn_net_bwd's grads vector (convs, upsampler, encoder); absent ones left out"""
    rows = []
    for j, (w, b) in enumerate(g["convs"]):
        rows += [(f"w{j}", w), (f"b{j}", b)]
    rows += [("up_w", g["up_w"]), ("up_b", g["up_b"]), ("enc_w", g["enc_w"]), ("enc_b", g["enc_b"])]
    return [(k, v) for k, v in rows if v is not None]


def module_grads(g, nb):
    """a gradient parameter set -> {parameter name of the EFFECTIVE tensor's module prefix: (dw, db)}"""
    d = {"encoder": (g["enc_w"], g["enc_b"]), f"body.{nb}": g["convs"][2 * nb], "shuf.0": (g["up_w"], g["up_b"])}
    for i in range(nb):
        d[f"body.{i}.body.0.body.0"], d[f"body.{i}.body.0.body.2"] = g["convs"][2 * i], g["convs"][2 * i + 1]
    return d


def param_grads(sd, nb, g):
    """gradients of the EFFECTIVE tensors -> {state_dict key: gradient} through the weight norm w = g v / |v| (float64 autograd on
    the small parameter tensors, as the route leaves it to torch)"""
    out = {}
    for prefix, (dw, db) in module_grads(g, nb).items():
        if prefix == "shuf.0":
            out["shuf.0.weight"], out["shuf.0.bias"] = dw, db
            continue
        v = sd[prefix + ".weight_v"].double().requires_grad_(True)
        gg = sd[prefix + ".weight_g"].double().requires_grad_(True)
        wgt = v * (gg / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
        out[prefix + ".weight_v"], out[prefix + ".weight_g"] = torch.autograd.grad(wgt, (v, gg), dw)
        out[prefix + ".bias"] = db
    return out


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def edge_lines(n4):
    """output rows / columns 0, 1, n4 - 2, n4 - 1 and every 4y"""
    return sorted({v for v in (0, 1, n4 - 2, n4 - 1) if 0 <= v < n4} | set(range(0, n4, 4)))


def exact_out_grad(n, h, w, sd=0, count=12):
    """(n, 3, 4h, 4w) float64: `count` small integers on crossings of the edge lines, the four corners always among them"""
    g = torch.Generator().manual_seed(_seed(31, n, h, w, sd, count))
    ys, xs = edge_lines(4 * h), edge_lines(4 * w)
    out = torch.zeros(n, 3, 4 * h, 4 * w, dtype=torch.float64)
    vals = torch.tensor([1.0, -1.0, 2.0, -2.0, 3.0], dtype=torch.float64)
    spots = [(0, 0), (0, xs[-1]), (ys[-1], 0), (ys[-1], xs[-1])]
    for _ in range(count):
        spots.append((ys[int(torch.randint(len(ys), (1,), generator=g))], xs[int(torch.randint(len(xs), (1,), generator=g))]))
    for k, (yy, xx) in enumerate(spots):
        out[k % n, int(torch.randint(3, (1,), generator=g)), yy, xx] = vals[int(torch.randint(5, (1,), generator=g))]
    return out


def _sparse_df(channel, n, h, w, sd, count):
    g = torch.Generator().manual_seed(_seed(32, channel, n, h, w, sd, count))
    df = torch.zeros(n, channel, h, w, dtype=torch.float64)
    ys, xs = sorted({0, h - 1, h // 2}), sorted({0, w - 1, w // 2})
    for k in range(count):
        yy, xx = ys[int(torch.randint(len(ys), (1,), generator=g))], xs[int(torch.randint(len(xs), (1,), generator=g))]
        df[k % n, int(torch.randint(channel, (1,), generator=g)), yy, xx] = float(torch.randint(1, 3, (1,), generator=g)) * (1 - 2 * (k & 1))
    return df


def check_exact_grad(case, res, hot_is_bf16):
    """raises R.NotExact unless every stored gradient is a value of the hot dtype and every weight-gradient sum is exact in fp32"""
    ok = is_bf16 if hot_is_bf16 else is_fp32
    fw = res["fw"]
    imgs = [("df", res["df"]), ("dz", res["dz"]), ("de", res["de"])] + [(f"dt{i}", t) for i, t in enumerate(res["dt"])]
    imgs += [(f"dx{i}", t) for i, t in enumerate(res["dx"])]
    if "dD" in res:
        imgs.append(("dD", res["dD"]))
    for name, t in imgs:
        if not ok(t):
            raise R.NotExact(f"{name}: not a value of the hot dtype")
    quantum = min(1.0, min(float(lowbit(t).min()) for _, t in imgs))     # the gradients' lattice; the forward's is the integers
    a = lambda t: t.double().abs()
    p, nb = case["p"], len(fw["t"])
    ys = [fw["e"]] + fw["y"]
    sums = [("dz", _conv_t(a(res["df"]), a(p["convs"][2 * nb][0]))), ("dW last", _conv_w(a(ys[nb]), a(res["df"]))),
            ("dW encoder", _conv_w(a(fw["x"]), a(res["de"])))]
    if "dD" in res:
        sums += [("df", F.conv2d(a(res["dD"]), a(p["up_w"]), stride=4)),
                 ("dW up", torch.nn.grad.conv2d_weight(a(res["dD"]), tuple(p["up_w"].shape), a(fw["f"]), stride=4))]
    for i in range(nb):
        dy = res["dx"][i + 1] if i + 1 < nb else res["dz"]
        sums += [(f"dt{i}", _conv_t(a(dy), a(p["convs"][2 * i + 1][0]))), (f"dx{i}", a(dy) + _conv_t(a(res["dt"][i]), a(p["convs"][2 * i][0]))),
                 (f"dW2 {i}", _conv_w(a(fw["t"][i]), a(dy))), (f"dW1 {i}", _conv_w(a(ys[i]), a(res["dt"][i])))]
    sums += [(f"db of {name}", a(t).sum((0, 2, 3))) for name, t in imgs]
    try:
        for name, s in sums:
            need_sum(name, s, quantum)
    except ValueError as e:
        raise R.NotExact(str(e)) from None
    return res


@functools.lru_cache(maxsize=None)
def exact_grad_case(channel, nb, n, h, w, sd=0):
    """(forward case, df, backward result): the conv stages' exact case, good for both hot dtypes"""
    case = R.exact_case(channel, nb, n, h, w)
    last = None
    for count in (6, 3, 1):
        for k in range(8):
            df = _sparse_df(channel, n, h, w, sd + 53 * k, count)
            try:
                return case, df, check_exact_grad(case, backward(case["x"], case["p"], None, df=df), True)
            except R.NotExact as e:
                last = e
    raise R.NotExact(f"no exact gradient case for {(channel, nb, n, h, w)}: {last}")


@functools.lru_cache(maxsize=None)
def exact_up_case(channel, nb, n, h, w, hot_is_bf16, sd=0):
    """(forward case, gout, backward result) for the whole chain from an edge-line output gradient; power-of-two h, w"""
    case = R.exact_case(channel, nb, n, h, w)
    last = None
    for count in (12, 6, 2, 0):
        for k in range(6):
            gout = exact_out_grad(n, h, w, sd + 31 * k, count)
            try:
                return case, gout, check_exact_grad(case, backward(case["x"], case["p"], gout), hot_is_bf16)
            except R.NotExact as e:
                last = e
    raise R.NotExact(f"no exact output-gradient case for {(channel, nb, n, h, w)}: {last}")
