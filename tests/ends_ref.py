"""Both ends of the WDSR network -- the head conv (3x3, 3 -> F, on x - mean) and the fused tail (3x3 F -> 3 R^2, plus the 5x5 skip
3 -> 3 R^2 on x - mean, plus the constants, PixelShuffle(R) and the mean), their backward, the loss fold (L1 / Charbonnier) and
the head's weight gradient -- written out in plain torch, float64 on the CPU, plus the case generators of the ends parity tests.
Nothing of the package or of the oracle is used here: this is the outside reference that csrc/wdsr_ends.h is held against
(tests/test_gpu_ends_ref.py).  tests/test_ends_ref_host.py pins it to oracle.wdsr_oracle, to the fixtures G1 and G4 and to
shifted copies, and checks on the CPU that every exact case satisfies its exactness conditions.

Layouts are the entries': the LR image x is (n, 3, h, w) fp32, features and their gradients are NHWC, the HR tensors are
(n, 3, R h, R w) fp32, btot = bt + bs + mean (hotpath.tail_src), and the parameter vectors are hotpath.head_src / tail_src's.

Three families of cases:
  exact     dyadic data on which every operand the kernels hold in the hot dtype is its own bf16 rounding and every reduction
            satisfies sum |terms| < 2^24 quanta, so fp32 accumulation is exact in ANY order: a kernel must return the float64
            reference bit for bit, in fp32 and in bf16, the tensors it stores in the hot dtype (y, dfeat) being the exact value
            rounded once, nearest-even.  check_exact() verifies the conditions on the float64 reference alone and raises
            ValueError if one fails; it also refuses a vacuous case (zeros, unused taps, equal rows, symmetric gradients).
            With the loss fold, hr = sr - d on the REFERENCE's sr, d in {+-1/2, +-1, +-2} and d = 0 at chosen pixels: the kernel's
            own forward has to produce the reference's bits for the zeros to be zeros.  In float32 sqrt(d d + 1e-12) == |d| for
            these d (asserted), so the Charbonnier gradient is +-gscale and its term |d|; d = 0 is L1 only (sqrt(1e-12) is not
            dyadic).
  tap sets  one weight per output channel: the output is a shifted (and shuffled) copy of one input channel plus the constant,
            so a failure names the tap and the HR sub-pixel
  rounded   random normal data, nothing rounded beforehand; the yardstick is emulate(): the same graph in float32 with a
            rounding to bf16 wherever the bf16 kernels round

The conditions named need_* / is_*, the roundings, the seed recipe and the bound of the rounded cases are tests/parity_kit.py's,
shared by all parity suites and pinned by tests/test_parity_kit_host.py.
"""
import functools

import torch
import torch.nn.functional as F_

from tests.parity_kit import (bf16_round, chan_quantum, count_ties, fail, leaf, lowbit, need_bf16, need_biases, need_fp32, need_half_nonzero,
                              need_sum, need_taps, rel_max, seed)

MEAN = 0.5
TH, TW = 12, 24                                             # the ends kernels' LR tile


def n_tiles(n, h, w):
    return n * ((h + TH - 1) // TH) * ((w + TW - 1) // TW)


def unshuffle(d, R):
    """(n, 3, R h, R w) -> (n, 3 R R, h, w): channel c R R + i R + j of LR pixel (y, x) = d[c, y R + i, x R + j]"""
    n, c, hh, ww = d.shape
    return d.reshape(n, c, hh // R, R, ww // R, R).permute(0, 1, 3, 5, 2, 4).reshape(n, c * R * R, hh // R, ww // R)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def head_ref(x, wh, bh, mean):
    """y (n, h, w, F) = conv3x3(x - mean; wh) + bh"""
    return F_.conv2d(x - mean, wh, bh, padding=1).permute(0, 2, 3, 1)


def tail_ref(feat, x, wt, ws, btot, mean, R):
    """out (n, 3, R h, R w) = PixelShuffle_R(conv3x3(feat; wt) + conv5x5(x - mean; ws) + btot), feat NHWC"""
    z = F_.conv2d(feat.permute(0, 3, 1, 2), wt, padding=1) + F_.conv2d(x - mean, ws, padding=2) + btot.view(1, -1, 1, 1)
    return F_.pixel_shuffle(z, R)


def tail_grads_ref(feat, x, wt, ws, btot, mean, R, dout, dtype=torch.float64):
    """dict(dfeat (NHWC), dwt, dws, dbtot) for the cotangent dout: every input a leaf, gradients from autograd"""
    lf, lwt, lws, lb = leaf(feat, dtype), leaf(wt, dtype), leaf(ws, dtype), leaf(btot, dtype)
    tail_ref(lf, x.to(dtype), lwt, lws, lb, mean, R).backward(dout.to(dtype))
    return dict(dfeat=lf.grad, dwt=lwt.grad, dws=lws.grad, dbtot=lb.grad)


def loss_ref(sr, hr, kind, gscale):
    """(d loss / d sr, loss sum) of the folded loss: kind 1 -- L1: sign(sr - hr) gscale with sign(0) = 0, sum |d|;
    kind 2 -- Charbonnier: d / sqrt(d^2 + 1e-12) gscale, sum sqrt(d^2 + 1e-12)"""
    d = sr - hr
    if kind == 1:
        return torch.sign(d) * gscale, d.abs().sum()
    s = torch.sqrt(d * d + 1e-12)
    return d / s * gscale, s.sum()


def head_wgrad_ref(dy0, x, mean, dtype=torch.float64):
    """(d wh (F, 3, 3, 3), d bh (F,)) for the cotangent dy0 (n, h, w, F) of the head's output"""
    f = dy0.shape[-1]
    wh, bh = torch.zeros(f, 3, 3, 3, dtype=dtype, requires_grad=True), torch.zeros(f, dtype=dtype, requires_grad=True)
    head_ref(x.to(dtype), wh, bh, mean).backward(dy0.to(dtype))
    return wh.grad, bh.grad


# ---- the entries' parameter vectors ---------------------------------------------------------------------------------------
def head_vec(wh, bh):
    """hotpath.head_src's order: wh (F, 3, 3, 3) | bh (F) | 0 | 1"""
    return torch.cat([wh.reshape(-1), bh.reshape(-1), wh.new_tensor([0.0, 1.0])])


def tail_vec(wt, ws, btot):
    """hotpath.tail_src's order: wt (CO, F, 3, 3) | ws (CO, 3, 5, 5) | btot (CO) | 0 | 1"""
    return torch.cat([wt.reshape(-1), ws.reshape(-1), btot.reshape(-1), wt.new_tensor([0.0, 1.0])])


def split_head_vec(v, f):
    """a gradient vector of hotpath.head_wgrad -> dict(dwh, dbh, const): const are the two constant slots (zero)"""
    assert v.numel() == 28 * f + 2, (v.numel(), f)
    return dict(dwh=v[:27 * f].reshape(f, 3, 3, 3), dbh=v[27 * f:28 * f], const=v[28 * f:])


def split_tail_vec(v, f, R):
    """a gradient vector of hotpath.tail_wgrad / tail_bwd / tail_bwd_loss -> dict(dwt, dws, dbtot, const)"""
    co = 3 * R * R
    a, b = co * f * 9, co * 75
    assert v.numel() == a + b + co + 2, (v.numel(), f, R)
    return dict(dwt=v[:a].reshape(co, f, 3, 3), dws=v[a:a + b].reshape(co, 3, 5, 5), dbtot=v[a + b:a + b + co], const=v[a + b + co:])


# ---- exactness conditions -------------------------------------------------------------------------------------------------
def _need_weights(name, w, h, w_img, grad=False):
    if not grad:
        if not bool((w != 0).any(0).all()):
            fail(f"{name}: a tap of an input channel is zero in every output channel")
        if torch.unique(w.reshape(w.shape[0], -1), dim=0).shape[0] != w.shape[0]:
            fail(f"{name}: two output-channel rows are equal")
    need_taps(name, w, 3 if not grad else h, 3 if not grad else w_img)


def _need_taps_enter(name, xin, k, h, w_img):
    """every tap the geometry reaches multiplies a nonzero input of every input channel at some output pixel"""
    n, ci = xin.shape[:2]
    ent = torch.nn.grad.conv2d_weight(xin.abs(), (1, ci, k, k), torch.ones(n, 1, h, w_img, dtype=xin.dtype), padding=k // 2)[0] > 0
    off = torch.arange(k) - k // 2
    reach = (off.abs().view(-1, 1) <= h - 1) & (off.abs().view(1, -1) <= w_img - 1)
    if not bool(ent[:, reach].all()):
        fail(f"{name}: a reachable tap of an input channel enters no output")


def _check_conv(tag, xin, w, dz, ref_dw, h, w_img):
    """the backward sums of one conv: xin (n, ci, h, w), dz (n, co, h, w).  Returns (sum |terms| of backward-data, quantum)."""
    k = w.shape[-1]
    qx, qd, qw = chan_quantum(xin), chan_quantum(dz), lowbit(w).amin((2, 3))
    tw = torch.nn.grad.conv2d_weight(xin.abs(), w.shape, dz.abs(), padding=k // 2)
    need_sum(f"d {tag}", tw, qd.view(-1, 1, 1, 1) * qx.view(1, -1, 1, 1))
    need_fp32(f"d {tag}", ref_dw)
    need_half_nonzero(f"d {tag}", ref_dw, tw)
    _need_weights(f"d {tag}", ref_dw, h, w_img, grad=True)
    return F_.conv_transpose2d(dz.abs(), w.abs(), padding=k // 2), (qw * qd.view(-1, 1)).amin(0)


_LOSS_D = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def check_exact(case):
    """Verify the exactness conditions of an exact case (head or tail) on the float64 reference alone; raises ValueError if one
    fails.  Returns the reference: float64 tensors, the hot-dtype stores once exact ('y', 'dfeat') and once rounded to bf16
    ('y_bf16', 'dfeat_bf16'), and 'ties', the number of stored values that lie exactly on a bf16 tie."""
    d64 = lambda k: case[k].double()
    x, mean = d64("x"), case["mean"]
    n, _, h, w = x.shape
    cv = lambda t: t.view(1, -1, 1, 1)
    xm = x - mean
    need_bf16("x - mean", xm)
    qx = chan_quantum(xm)
    if case["kind"] == "head":
        wh, bh, dy0 = d64("wh"), d64("bh"), d64("dy0")
        for name, t in (("wh", wh), ("bh", bh), ("dy0", dy0)):
            need_bf16(name, t)
        _need_weights("wh", wh, h, w)
        _need_taps_enter("head", xm, 3, h, w)
        need_biases("bh", bh)
        y = head_ref(x, wh, bh, mean)
        fwd = F_.conv2d(xm.abs(), wh.abs(), bh.abs(), padding=1)
        need_sum("head forward", fwd, cv(torch.minimum((lowbit(wh).amin((2, 3)) * qx.view(1, -1)).amin(1), lowbit(bh))))
        need_fp32("y", y)
        need_half_nonzero("y", y, fwd.permute(0, 2, 3, 1))
        dwh, dbh = head_wgrad_ref(dy0, x, mean)
        dz = dy0.permute(0, 3, 1, 2)
        _check_conv("wh", xm, wh, dz, dwh, h, w)
        need_sum("d bh", dz.abs().sum((0, 2, 3)), chan_quantum(dz))
        need_fp32("d bh", dbh)
        need_half_nonzero("d bh", dbh, dz.abs().sum((0, 2, 3)))
        return dict(y=y, y_bf16=bf16_round(y), dwh=dwh, dbh=dbh, ties=count_ties(y))
    R = case["R"]
    feat, wt, ws, btot = d64("feat"), d64("wt"), d64("ws"), d64("btot")
    for name, t in (("feat", feat), ("wt", wt), ("ws", ws), ("btot", btot)):
        need_bf16(name, t)
    _need_weights("wt", wt, h, w)
    _need_weights("ws", ws, h, w)
    fn = feat.permute(0, 3, 1, 2)
    _need_taps_enter("tail", fn, 3, h, w)
    _need_taps_enter("skip", xm, 5, h, w)
    odd = btot * 8
    if not (torch.equal(odd, odd.round()) and bool((odd.abs() % 2 == 1).all()) and torch.unique(btot).numel() == btot.numel()):
        fail("btot: the constants must be pairwise different odd multiples of 1/8")
    out = tail_ref(feat, x, wt, ws, btot, mean, R)
    qf = chan_quantum(fn)
    q_out = torch.minimum(torch.minimum((lowbit(wt).amin((2, 3)) * qf.view(1, -1)).amin(1), (lowbit(ws).amin((2, 3)) * qx.view(1, -1)).amin(1)),
                          lowbit(btot))
    fwd = F_.conv2d(fn.abs(), wt.abs(), padding=1) + F_.conv2d(xm.abs(), ws.abs(), btot.abs(), padding=2)
    need_sum("tail forward", fwd, cv(q_out))
    need_fp32("out", out)
    need_half_nonzero("out", out, F_.pixel_shuffle(fwd, R))
    ref = dict(out=out)
    if "hr" in case:
        hr, kind, gscale = d64("hr"), case["loss_kind"], case["gscale"]
        diff = out - hr
        vals = set(diff.unique().tolist())
        if not vals <= set(_LOSS_D) | ({0.0} if kind == 1 else set()):
            fail(f"sr - hr takes the values {sorted(vals)}")
        for v in vals:                                       # in float32, as the kernel forms it: sqrt(d d + 1e-12f) == |d|
            t = torch.tensor(v, dtype=torch.float32)
            if kind == 2 and float(torch.sqrt(t * t + torch.tensor(1e-12, dtype=torch.float32))) != abs(v):
                fail(f"Charbonnier: sqrt(d d + 1e-12) != |d| in float32 at d = {v}")
        if gscale != 2.0 ** round(torch.log2(torch.tensor(gscale)).item()):
            fail("gscale is not a power of two")
        need_fp32("hr", hr)
        dout, lsum = loss_ref(out, hr, 1, gscale)            # +-gscale, 0 at d = 0, for both kinds on these d
        need_sum("loss", lsum.view(1), lowbit(diff).min().view(1))
        need_fp32("loss", lsum.view(1))
        ref.update(dout=dout, loss=lsum, zeros=int((diff == 0).sum()))
    else:
        dout = d64("dout")
    dz = unshuffle(dout, R)
    need_bf16("dconv", dz)
    g = tail_grads_ref(feat, x, wt, ws, btot, mean, R, dout)
    bd, q_in = _check_conv("wt", fn, wt, dz, g["dwt"], h, w)
    need_sum("tail backward data", bd, cv(q_in))
    need_fp32("dfeat", g["dfeat"])
    need_half_nonzero("dfeat", g["dfeat"], bd.permute(0, 2, 3, 1))
    _check_conv("ws", xm, ws, dz, g["dws"], h, w)
    need_sum("d btot", dz.abs().sum((0, 2, 3)), chan_quantum(dz))
    need_fp32("d btot", g["dbtot"])
    need_half_nonzero("d btot", g["dbtot"], dz.abs().sum((0, 2, 3)))
    ref.update(g, dfeat_bf16=bf16_round(g["dfeat"]), ties=count_ties(g["dfeat"]))
    return ref


# ---- exact cases ----------------------------------------------------------------------------------------------------------
_seed = functools.partial(seed, 24680, 7)


def _pow2(shape, lo, hi, g):
    return 2.0 ** torch.randint(lo, hi + 1, shape, generator=g).double()


def _sign(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _tern(shape, density, g):
    t = _sign(shape, g)
    return t * (torch.rand(shape, generator=g) < density).double() if density < 1.0 else t


def _odd_eighths(c, g):
    """c pairwise different odd multiples of 1/8 (|k| <= 2 c - 1 < 2^8: each its own bf16 rounding)"""
    k = torch.arange(-(2 * c - 1), 2 * c, 2)
    return k[torch.randperm(2 * c, generator=g)[:c]].double() / 8


def _first_exact(build, tries=16):
    """the first of build(0), build(1), .. that check_exact() accepts (a tiny image may draw a symmetric or mostly-zero sum)"""
    err = None
    for k in range(tries):
        case = build(k)
        try:
            case["ref"] = check_exact(case)
            return case
        except ValueError as e:
            err = e
    raise err


def zero_pixels(n, h, w, g, n_border=40, n_inner=120):
    """(n, h, w) bool: LR pixels where hr is set to sr exactly -- n_border on a tile's (or the image's) border, n_inner inside,
    chosen as tests/test_gpu_tail_train.py chooses them"""
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    border = ((ys % TH == 0) | (ys % TH == TH - 1) | (ys == h - 1) | (xs % TW == 0) | (xs % TW == TW - 1) | (xs == w - 1))
    pick = torch.zeros(n, h, w, dtype=torch.bool)
    for mask, cnt in ((border, n_border), (~border, n_inner)):
        idx = mask.expand(n, h, w).nonzero()
        sel = idx[torch.randperm(idx.shape[0], generator=g)[:cnt]]
        pick[sel[:, 0], sel[:, 1], sel[:, 2]] = True
    return pick, int((pick & border).sum()), int((pick & ~border).sum())


@functools.lru_cache(maxsize=None)
def exact_tail_case(f, R, n, h, w, seed=0, density=0.5, loss=0):
    """One tail call on dyadic data: weights +-2^k, feat and the un-shuffled cotangent in {-1, 0, 1} times per-channel powers of
    two (`density` of the cotangent nonzero), x on multiples of 1/8 in [0, 1] (mean 0.5), btot pairwise different odd multiples
    of 1/8.  loss = 1 / 2: hr = sr - d instead of a cotangent, gscale = 2^-12, and for L1 zeros of d at >= 100 LR pixels inside
    tiles and >= 20 on tile borders.  Checked by check_exact(); cached: the tensors are shared and must not be written to."""
    co = 3 * R * R
    dense = n * h * w <= 9

    def build(k):
        g = torch.Generator().manual_seed(_seed(1, f, R, n, h, w, seed, loss, k))
        wt = _sign((co, f, 3, 3), g) * _pow2((co, f, 3, 3), -3, 3, g)
        ws = _sign((co, 3, 5, 5), g) * _pow2((co, 3, 5, 5), -3, 3, g)
        btot = _odd_eighths(co, g)
        feat = _tern((n, h, w, f), 1.0 if dense else 0.75, g) * _pow2((f,), -2, 2, g)
        x = torch.randint(0, 9, (n, 3, h, w), generator=g).double() / 8
        case = dict(kind="tail", F=f, R=R, mean=MEAN, feat=feat.float(), x=x.float(), wt=wt.float(), ws=ws.float(), btot=btot.float())
        if loss == 0:
            dz = _tern((n, co, h, w), 1.0 if dense else density, g) * _pow2((co,), -2, 2, g).view(1, -1, 1, 1)
            case["dout"] = F_.pixel_shuffle(dz, R).float()
            return case
        sr = tail_ref(feat, x, wt, ws, btot, MEAN, R)
        d = torch.tensor(_LOSS_D, dtype=torch.float64)[torch.randint(0, len(_LOSS_D), sr.shape, generator=g)]
        if loss == 1:
            pick, nb, ni = zero_pixels(n, h, w, g)
            if ni < 100 or nb < 20:
                fail(f"{ni} zero pixels inside tiles, {nb} on borders")
            d = d * (~pick).repeat_interleave(R, 1).repeat_interleave(R, 2)[:, None].double()
        case.update(hr=(sr - d).float(), loss_kind=loss, gscale=2.0 ** -12)
        return case

    return _first_exact(build)


@functools.lru_cache(maxsize=None)
def exact_head_case(f, n, h, w, seed=0, density=0.5):
    """One head call (forward on x, weight gradient for the cotangent dy0) on dyadic data"""
    dense = n * h * w <= 9

    def build(k):
        g = torch.Generator().manual_seed(_seed(2, f, n, h, w, seed, k))
        wh = _sign((f, 3, 3, 3), g) * _pow2((f, 3, 3, 3), -3, 3, g)
        bh = _odd_eighths(f, g)
        x = torch.randint(0, 9, (n, 3, h, w), generator=g).double() / 8
        dy0 = _tern((n, h, w, f), 1.0 if dense else density, g) * _pow2((f,), -2, 2, g)
        return dict(kind="head", F=f, mean=MEAN, x=x.float(), wh=wh.float(), bh=bh.float(), dy0=dy0.float())

    return _first_exact(build)


# ---- tap-identity sets ------------------------------------------------------------------------------------------------------
def tail_tap_cases(f, R, n, h, w):
    """cases with ONE weight per conv channel, +-2^k: channel ch of set s holds tap number (s CO + ch) mod (9 F + 75) of the list
    [tail (fi, ky, kx) ..., skip (ci, ky, kx) ...], so the sets together cover all 9 F taps of the tail conv and all 75 of the
    skip, each set covers every conv channel c R R + i R + j, and over the sets a tap meets different sub-pixels.  case['taps'][ch] =
    ('tail' | 'skip', input channel, ky, kx); case['ref']['out'] is the float64 reference (a shifted, shuffled copy plus btot)."""
    co = 3 * R * R
    taps = [("tail", fi, ky, kx) for fi in range(f) for ky in range(3) for kx in range(3)]
    taps += [("skip", ci, ky, kx) for ci in range(3) for ky in range(5) for kx in range(5)]
    g = torch.Generator().manual_seed(_seed(3, f, R, n, h, w))
    feat = torch.randint(-8, 9, (n, h, w, f), generator=g).double() * _pow2((f,), -2, 2, g)
    x = torch.randint(0, 9, (n, 3, h, w), generator=g).double() / 8
    cases = []
    for s in range((len(taps) + co - 1) // co):
        wt, ws = torch.zeros(co, f, 3, 3, dtype=torch.float64), torch.zeros(co, 3, 5, 5, dtype=torch.float64)
        val = _sign((co,), g) * _pow2((co,), -3, 3, g)
        mine = []
        for ch in range(co):
            kind, ci, ky, kx = taps[(s * co + ch) % len(taps)]
            (wt if kind == "tail" else ws)[ch, ci, ky, kx] = val[ch]
            mine.append((kind, ci, ky, kx))
        btot = _odd_eighths(co, g)
        case = dict(kind="tail", F=f, R=R, mean=MEAN, feat=feat.float(), x=x.float(), wt=wt.float(), ws=ws.float(), btot=btot.float(), taps=mine)
        case["ref"] = dict(out=tail_ref(feat, x, wt, ws, btot, MEAN, R))
        cases.append(case)
    return cases


def head_tap_cases(f, n, h, w):
    """the same for the head: output channel fo of set s holds tap (s F + fo) mod 27 of [(ci, ky, kx) ...]; two sets cover all 27"""
    taps = [(ci, ky, kx) for ci in range(3) for ky in range(3) for kx in range(3)]
    g = torch.Generator().manual_seed(_seed(4, f, n, h, w))
    x = torch.randint(0, 9, (n, 3, h, w), generator=g).double() / 8
    cases = []
    for s in range(2):
        wh = torch.zeros(f, 3, 3, 3, dtype=torch.float64)
        val = _sign((f,), g) * _pow2((f,), -3, 3, g)
        mine = [taps[(s * f + fo) % 27] for fo in range(f)]
        for fo, (ci, ky, kx) in enumerate(mine):
            wh[fo, ci, ky, kx] = val[fo]
        bh = _odd_eighths(f, g)
        y = head_ref(x, wh, bh, MEAN)
        cases.append(dict(kind="head", F=f, mean=MEAN, x=x.float(), wh=wh.float(), bh=bh.float(), taps=mine, ref=dict(y=y, y_bf16=bf16_round(y))))
    return cases


# ---- the cases of the parity tests: (n, h, w) --------------------------------------------------------------------------------
GEOMETRIES = (
    (1, 1, 1), (1, 1, 30), (1, 30, 1), (1, 2, 3), (1, 3, 3),           # inside the halos (1, 2 and 3 pixels) on both sides
    (1, 11, 23), (1, 12, 24), (1, 13, 25),                              # one tile under / exact / one-pixel slivers
    (1, 12, 25), (1, 13, 24),
    (2, 25, 49),                                                        # 3 x 3 tiles: an interior tile whose halo is all live
    (3, 13, 25),                                                        # 12 tiles, the batch stride
)
UNITS = (24, 32)
SCALE_GEOMETRIES = ((1, 1, 1), (1, 13, 25), (2, 25, 49))                # R = 2 and 3 (R = 3: CO = 27 padded to COP = 32)
TAP_GEOMETRY = (1, 13, 25)
TILE_LOOP_GEOMETRY = (3, 13, 25)                                        # 12 tiles
TILE_LOOP_WGS = (1, 5, 12, 13, None)                                    # None: the entry's default (64 or 256)
MANY_TILES = (65, 13, 25)                                               # 260 tiles > the default 256 workgroups
MANY_TILES_DENSITY = 0.25
LOSS_GEOMETRIES = ((1, 13, 25), (2, 25, 49), (3, 13, 25))
ROUNDED_GEOMETRIES = ((1, 13, 25), (2, 25, 49))


def exact_family():
    """every exact case of the GPU file's parameter lists, as (name, thunk)"""
    fam = []
    for f in UNITS:
        for geom in GEOMETRIES:
            fam.append((f"tail F{f} R4 {geom}", functools.partial(exact_tail_case, f, 4, *geom)))
            fam.append((f"head F{f} {geom}", functools.partial(exact_head_case, f, *geom)))
        for R in (2, 3):
            for geom in SCALE_GEOMETRIES:
                fam.append((f"tail F{f} R{R} {geom}", functools.partial(exact_tail_case, f, R, *geom)))
        fam.append((f"tail F{f} many tiles", functools.partial(exact_tail_case, f, 4, *MANY_TILES, 0, MANY_TILES_DENSITY)))
        fam.append((f"head F{f} many tiles", functools.partial(exact_head_case, f, *MANY_TILES, 0, MANY_TILES_DENSITY)))
        fam.append((f"tail F{f} many tiles loss 1", functools.partial(exact_tail_case, f, 4, *MANY_TILES, 0, 0.5, 1)))
        for kind in (1, 2):
            for geom in LOSS_GEOMETRIES:
                fam.append((f"tail F{f} R4 {geom} loss {kind}", functools.partial(exact_tail_case, f, 4, *geom, 0, 0.5, kind)))
            for R in (2, 3):
                fam.append((f"tail F{f} R{R} {LOSS_GEOMETRIES[0]} loss {kind}",
                            functools.partial(exact_tail_case, f, R, *LOSS_GEOMETRIES[0], 0, 0.5, kind)))
    return fam


# ---- rounded cases ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounded_tail_case(f, R, n, h, w, seed=0):
    """random normal data, PyTorch-default-sized weights; nothing is rounded beforehand: rounding x - mean, feat, the weights and
    the cotangent to bf16 is part of what the bf16 route does, so it belongs to the emulation and to the yardstick"""
    g = torch.Generator().manual_seed(_seed(5, f, R, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    co = 3 * R * R
    return dict(kind="tail", F=f, R=R, mean=MEAN, feat=rn(n, h, w, f), x=0.5 + 0.25 * rn(n, 3, h, w), wt=rn(co, f, 3, 3) / (3.0 * f ** 0.5),
                ws=rn(co, 3, 5, 5) / (5.0 * 3 ** 0.5), btot=0.5 + 0.1 * rn(co), dout=rn(n, 3, R * h, R * w),
                hr_noise=0.1 * rn(n, 3, R * h, R * w), hr_same=torch.rand(n, 3, R * h, R * w, generator=g) < 0.02)


@functools.lru_cache(maxsize=None)
def rounded_head_case(f, n, h, w, seed=0):
    g = torch.Generator().manual_seed(_seed(6, f, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(kind="head", F=f, mean=MEAN, x=0.5 + 0.25 * rn(n, 3, h, w), wh=rn(f, 3, 3, 3) / (3.0 * 3 ** 0.5), bh=0.1 * rn(f),
                dy0=rn(n, h, w, f))


def run_case(case, dtype=torch.float64, rnd=None, sr=None, hr=None, kind=0, gscale=0.0):
    """every tensor the entries produce for `case`, evaluated in `dtype`; rnd: the rounding applied where the bf16 kernels round
    (x - mean, feat, the weights and constants of the blob, the dconv image, the dfeat / y stores, dy0), None for the reference.
    With sr / hr (HR tensors given to the loss fold: sr is an INPUT of sr_tail_bwd_loss) the cotangent is loss_ref(sr, hr)'s and
    'loss' its sum, the terms added left to right in `dtype` when it is not float64."""
    r = rnd if rnd is not None else (lambda t: t)
    c = lambda k: case[k].to(dtype)
    xm = r(c("x") - case["mean"])                           # the kernels subtract in fp32, then round
    zero = torch.zeros((), dtype=dtype)
    if case["kind"] == "head":
        y = r(head_ref(xm, r(c("wh")), r(c("bh")), zero))
        dwh, dbh = head_wgrad_ref(r(c("dy0")), xm, zero, dtype)
        return dict(y=y, dwh=dwh, dbh=dbh)
    R = case["R"]
    feat, wt, ws, btot = r(c("feat")), r(c("wt")), r(c("ws")), r(c("btot"))
    res = dict(out=tail_ref(feat, xm, wt, ws, btot, zero, R))
    if sr is not None:
        dout, lsum = loss_ref(sr.to(dtype), hr.to(dtype), kind, gscale)
        if dtype != torch.float64:
            d = sr.to(dtype) - hr.to(dtype)
            terms = d.abs() if kind == 1 else torch.sqrt(d * d + torch.tensor(1e-12, dtype=dtype))
            lsum = terms.reshape(-1).cumsum(0)[-1]
        res["loss"] = lsum.reshape(1)
    else:
        dout = c("dout")
    g = tail_grads_ref(feat, xm, wt, ws, btot, zero, R, F_.pixel_shuffle(r(unshuffle(dout, R)), R), dtype)
    g["dfeat"] = r(g["dfeat"])
    res.update(g)
    return res


def emulate(case, mode, **loss):
    """the ends in the kernels' precision on the CPU, in float32: 'fp32' -- nothing else; 'bf16' -- with a rounding to bf16 at the
    kernels' rounding points (run_case's rnd); out and the weight-gradient sums stay fp32 as the kernels' slabs do"""
    return run_case(case, torch.float32, bf16_round if mode == "bf16" else None, **loss)


def rounded_reference(case, mode, **loss):
    """(float64 reference, yardstick per tensor): the yardstick is the distance of emulate() from the float64 reference in the
    tests' metric -- computed on the CPU from the reference alone"""
    ref = run_case(case, **loss)
    emu = emulate(case, mode, **loss)
    return ref, {k: rel_max(emu[k], ref[k]) for k in ref}
