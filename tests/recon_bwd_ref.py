"""The backward of BasicVSR_origin's reconstruction written out in plain torch, float64 on the CPU, with the case generators of
tests/test_gpu_recon_bwd.py.  Nothing of the package is used here.  Built on tests/recon_ref.py (fusion_ref, upconv_ref, last_ref,
conv_ref: the forward) and tests/parity_kit.py.

One STAGE per layer, named by its bit of sr_c64_recon_bwd's `stages` (the forward's bits):
  16  conv_last   gin = g (N, 3, 4h, 4w); x = a = hr          dx = d_hr = conv_last^T(g) * lrelu'(hr)
   8  conv_hr     gin = d_hr (masked already); x = up2         dx = d_up2 = conv_hr^T(d_hr)
   4  upconv2     gin = d_up2, a = up2; x = up1                dz = unshuffle(gin * lrelu'(a)); dx = d_up1 = upconv2^T(dz)
   2  upconv1     gin = d_up1, a = up1; x = fused              dx = d_fused
   1  fusion      gin = d_fused, a = fused; x = [fb | ff]      dpre = gin * lrelu'(a); dx = [dfb | dff] = Wfu^T dpre
and dW = sum over pixels of dz (x) x, db = sum of dz, per stage.

Rounding points (`hot`; the identity in fp32): every stored gradient image (d_hr, d_up2, d_up1, d_fused as dx of their stages, the
two state gradients) is rounded once to the hot dtype; dz / dpre is rounded once as it is staged; masks come from the STORED forward
images; all accumulation (taps, channels, the four sub-convs, slabs) is fp32; parameter gradients are fp32.  The kernels' mask is
g * (a > 0 ? 1 : 0.1f), one fp32 product (recon_ref.SLOPE32 in an exact case)."""
import functools

import torch
import torch.nn.functional as F

from tests import recon_ref as R
from tests.parity_kit import bf16_round, lowbit, need_bf16, need_fp32, need_sum, rel_max, seed

_seed = functools.partial(seed, 13579, 7)
STAGES = (16, 8, 4, 2, 1)
NAMES = {16: "conv_last", 8: "conv_hr", 4: "upconv2", 2: "upconv1", 1: "fusion"}
EXACT = ((64, 1, 5, 6), (64, 2, 9, 21), (40, 1, 9, 21), (25, 2, 4, 16), (64, 1, 16, 16), (64, 1, 17, 33))


def mask(g, a, exact=False):
    neg = (g * R.SLOPE32).float().to(g.dtype) if exact else R.SLOPE * g
    return torch.where(a > 0, g, neg)


def stage_shapes(stage, f, n, h, w):
    """(gin, a, x, weight) shapes of a stage on n images of h x w LOW-resolution pixels"""
    if stage == 16:
        return (n, 3, 4 * h, 4 * w), None, (n, 64, 4 * h, 4 * w), (3, 64, 3, 3)
    if stage == 8:
        return (n, 64, 4 * h, 4 * w), None, (n, 64, 4 * h, 4 * w), (64, 64, 3, 3)
    if stage == 4:
        return (n, 64, 4 * h, 4 * w), (n, 64, 4 * h, 4 * w), (n, f, 2 * h, 2 * w), (256, f, 3, 3)
    if stage == 2:
        return (n, f, 2 * h, 2 * w), (n, f, 2 * h, 2 * w), (n, f, h, w), (4 * f, f, 3, 3)
    return (n, f, h, w), (n, f, h, w), (n, 2 * f, h, w), (f, 2 * f, 1, 1)


def stage_run(case, dtype=torch.float64, hot=R.ident, exact=False):
    """one stage in `dtype`: dict(dz, dx, dW, db)"""
    st = case["stage"]
    t = lambda k: case[k].to(dtype)
    w, x, gin = hot(t("w")), t("x"), t("gin")
    if st == 16:
        dx = hot(mask(F.conv_transpose2d(gin, w, padding=1), x, exact))
        return dict(dz=gin, dx=dx, dW=torch.nn.grad.conv2d_weight(x, w.shape, gin, padding=1), db=gin.sum((0, 2, 3)))
    dz = gin if st == 8 else hot(mask(gin, t("a"), exact))
    if st in (4, 2):
        dz = F.pixel_unshuffle(dz, 2)
    pad = 0 if st == 1 else 1
    return dict(dz=dz, dx=hot(F.conv_transpose2d(dz, w, padding=pad)), dW=torch.nn.grad.conv2d_weight(x, w.shape, dz, padding=pad),
                db=dz.sum((0, 2, 3)))


def emulate(case, mode):
    """the yardstick of the rounded cases: the stage in float32, in bf16 mode with the rounding points above"""
    return stage_run(case, torch.float32, R.HOT[mode])


def exact_ref(case, mode):
    return stage_run(case, torch.float64, R.HOT[mode], exact=True)


# ---- the whole reconstruction: forward and the five stages chained (the formula torch.autograd differentiates in the host test) ----
def chain_forward(p, fb, ff, frame):
    """the reference formula (recon_ref's layers); returns (out, fused, up1, up2, hr)"""
    fused = R.fusion_ref(fb, ff, p["fusion.weight"], p["fusion.bias"])
    up1 = R.upconv_ref(fused, p["upconv1.weight"], p["upconv1.bias"])
    up2 = R.upconv_ref(up1, p["upconv2.weight"], p["upconv2.bias"])
    hr = R.lrelu(F.conv2d(up2, p["conv_hr.weight"], p["conv_hr.bias"], padding=1))
    return R.last_ref(hr, p["conv_last.weight"], p["conv_last.bias"], frame), fused, up1, up2, hr


def chain_backward(p, fb, ff, frame, g, dtype=torch.float64, hot=R.ident):
    """the five stages one after the other on the forward's stored images: {parameter name: gradient}, 'dfb', 'dff'"""
    p = {k: v.to(dtype) for k, v in p.items()}
    _, fused, up1, up2, hr = chain_forward(p, fb.to(dtype), ff.to(dtype), frame.to(dtype))
    res, gin = {}, g.to(dtype)
    for st, a, x in ((16, None, hr), (8, None, up2), (4, up2, up1), (2, up1, fused), (1, fused, torch.cat([fb, ff], 1).to(dtype))):
        case = dict(stage=st, gin=gin, x=x, w=p[NAMES[st] + ".weight"])
        if a is not None:
            case["a"] = a
        r = stage_run(case, dtype, hot)
        res[NAMES[st] + ".weight"], res[NAMES[st] + ".bias"], gin = r["dW"], r["db"], r["dx"]
    f = fb.shape[1]
    res["dfb"], res["dff"] = gin[:, :f], gin[:, f:]
    return res


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _sparse_weight(shape, g, nz):
    """+-2^k weights, `nz` per output row, placed so that the rows together use every tap and input channel"""
    co, ci, k, _ = shape
    w = torch.zeros(shape, dtype=torch.float64)
    sg = (torch.randint(0, 2, (co * nz,), generator=g) * 2 - 1).double()
    for i in range(co * nz):
        r = i // nz
        c, tap = (7 * i + 3 + i // ci) % ci, (2 * i + i // 9) % (k * k)
        w[r, c, tap // k, tap % k] = sg[i] * 2.0 ** (i % 3 - 1)
    return w


def check_exact(case, mode, signs=True):
    """the exactness conditions of a stage case on the float64 reference alone (parity_kit.need_sum on every reduction)"""
    r = exact_ref(case, mode)
    st = case["stage"]
    w, x, dz = case["w"].double(), case["x"].double(), r["dz"]
    for k in ("w", "x") + (("gin",) if st != 16 else ()) + (("a",) if "a" in case else ()):
        need_bf16(k, case[k].double())
    need_fp32("dz", dz)
    qz, qw, qx = lowbit(dz).min(), lowbit(w).min(), lowbit(x).min()
    pad = 0 if st == 1 else 1
    need_sum("dx", F.conv_transpose2d(dz.abs(), w.abs(), padding=pad), qz * qw)
    need_sum("dW", torch.nn.grad.conv2d_weight(x.abs(), w.shape, dz.abs(), padding=pad), qz * qx)
    need_sum("db", dz.abs().sum((0, 2, 3)), qz)
    for k in ("dx", "dW", "db"):
        need_fp32(k, r[k])
        if not bool((r[k] != 0).any()):
            raise ValueError(f"exact case: {k} is all zero")
    if signs and mode == "bf16" and "a" in case and not (bool((case["a"] > 0).any()) and bool((case["a"] < 0).any())):
        raise ValueError("exact case: the mask lacks a sign")
    return r


@functools.lru_cache(maxsize=None)
def stage_case(stage, f, n, h, w, mode, sd=0):
    """one exact case of one stage: an integer gradient (a quarter nonzero, {-2 .. 2}), integer forward images, +-2^k weights (two per
    row; conv_last: eight), a power-of-two scale per gradient channel.  fp32: the stored forward image is positive everywhere (the
    product with 0.1f carries 24 bits into the next contraction); bf16: both signs, the negative side is bf16(fp32(0.1f g))."""
    g = torch.Generator().manual_seed(_seed(stage, f, n, h, w, int(mode == "bf16"), sd))
    sg, sa, sx, sw = stage_shapes(stage, f, n, h, w)
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).double()
    gin = ri(sg, -2, 2) * (torch.rand(sg, generator=g) < 0.25).double() * 2.0 ** ri((1, sg[1], 1, 1), -1, 1)
    case = dict(stage=stage, f=f, gin=gin.float(), x=ri(sx, -2, 2).float(), w=_sparse_weight(sw, g, 8 if stage == 16 else 2).float())
    if stage == 16:                                      # hr is both operand and mask
        if mode == "fp32":
            case["x"] = ri(sx, 1, 3).float()
    elif sa is not None:
        a = ri(sa, 1, 3)
        if mode == "bf16":
            a = a * (torch.randint(0, 2, sa, generator=g) * 2 - 1).double()
        case["a"] = a.float()
    check_exact(case, mode)
    return case


def tap_case(stage, mode, h=5, w=6):
    """tap coverage of a 3x3 stage (f = 64): EVERY output row carries all nine taps, tap t on input channel (5 row + 7 t) % ci with
    weight s(q) 2^(t - 4), s(q) = 1, -1, 3, -3 for the sub-conv q = row % 4 of an upconv (1 elsewhere): every (tap, q) pair has a weight
    of its own, so a wrong tap, a wrong flip or a wrong sub-pixel changes the result.  The weights span nine binades, so the mask is
    positive in both modes here (the 0.1f side would not fit 24 bits next to them); stage_case has both signs in bf16."""
    case = dict(stage_case(stage, 64, 1, h, w, mode, sd=1))
    co, ci = case["w"].shape[:2]
    wt = torch.zeros(co, ci, 3, 3, dtype=torch.float64)
    for r in range(co):
        s = (1.0, -1.0, 3.0, -3.0)[r % 4] if stage in (4, 2) else 1.0
        for t in range(9):
            wt[r, (5 * r + 7 * t) % ci, t // 3, t % 3] = s * 2.0 ** (t - 4)
    case["w"] = wt.float()
    if "a" in case:
        case["a"] = case["a"].abs()
    check_exact(case, mode, signs=False)
    return case


def rounded_case(stage, f, n, h, w, mode, sd=0):
    """random normal data; every tensor the kernel holds in the hot dtype is part of the case in that precision"""
    g = torch.Generator().manual_seed(_seed(99, stage, f, n, h, w, sd))
    sg, sa, sx, sw = stage_shapes(stage, f, n, h, w)
    rn = lambda s: torch.randn(s, generator=g)
    hot = R.HOT[mode]
    case = dict(stage=stage, f=f, gin=rn(sg) if stage == 16 else hot(rn(sg)), x=hot(rn(sx)), w=rn(sw) / (sw[1] * sw[2] * sw[3]) ** 0.5)
    if sa is not None:
        case["a"] = hot(rn(sa))
    return case


def rounded_reference(case, mode):
    """(float64 reference, yardstick per tensor).  The data path reads hot-dtype weights: in bf16 mode the weight's rounding is part
    of the case for the reference too (nothing else rounds an operand there)"""
    ref_case = dict(case, w=bf16_round(case["w"])) if mode == "bf16" else case
    ref, emu = stage_run(ref_case), emulate(case, mode)
    return ref, {k: rel_max(emu[k], ref[k]) for k in ("dx", "dW", "db")}
