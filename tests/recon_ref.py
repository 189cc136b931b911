"""The two reconstruction back ends written out in plain torch, float64 on the CPU, with the case generators of the reconstruction
parity tests.  Nothing of the package is used here: this is the outside reference that csrc/vsr_recon.h (BasicVSR_origin: fusion,
upconv + PixelShuffle, conv_last + bilinear base) and csrc/mv_recon.h (MotionVectorVSR: fusion -> ConvTranspose x4 -> resize, forward
and backward) are held against by tests/test_gpu_recon_ref.py.  tests/test_recon_ref_host.py pins the references to fixtures G19 /
G4 / G11 and to ATen, and checks on the CPU that every exact case satisfies its exactness conditions.

  exact     dyadic data (tests/parity_kit.py's recipe: an integer network, then a power-of-two scale per channel of every tensor) on
            which every reduction satisfies sum |terms| < 2^24 quanta of its lattice; check_exact_conv() / check_exact_mv() verify
            this on the float64 reference alone and raise otherwise.  The kernels must return the reference bit for bit.
  rounded   random normal data; the yardstick is emulate_*(): the same reference in float32, in bf16 mode with a rounding at
            every point where the kernels round (below).

LeakyReLU: the kernels compute t > 0 ? t : 0.1f * t, ONE fp32 multiply, then store in the hot dtype.  0.1 is not dyadic, so the
references take the slope as an argument: SLOPE32 = float32(0.1) with the product rounded to fp32 (act_exact) is what the kernels
compute on an exact t, whatever their summation order.

Rounding points of the bf16 route (`hot` below; the identity in fp32): every stored image; u; in the backward dD as it becomes an
MFMA operand (for du and dW_last alike), dpre, and the dc store.

The MotionVectorVSR blend weight (2d + 1) / (8h) and its complement are exact in fp32 only when h is a power of two
(mv_lambda32, pinned by the host tests): out, dD and all gradients are bit-exact only on such images; u never depends on it.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import mv_recon_ref as M
from tests.parity_kit import (bf16_round, chan_quantum, count_ties, fail, lowbit, need_bf16, need_biases, need_fp32, need_sum,
                              need_taps, rel_max, seed)

SLOPE = 0.1
SLOPE32 = float(np.float32(0.1))
_seed = functools.partial(seed, 24680, 11)
ident = lambda t: t
BIG_Q = 2.0 ** 200
HOT = {"fp32": ident, "bf16": bf16_round}


def lrelu(t, slope=SLOPE):
    return torch.where(t > 0, t, slope * t)


def act_exact(t):
    """the kernels' LeakyReLU on an exactly known float64 t: the product with float32(0.1) (exact in float64: 24 x 24 bits), rounded
    once to fp32"""
    return torch.where(t > 0, t, (t * SLOPE32).float().double())


# ---- BasicVSR_origin side: one kernel each -------------------------------------------------------------------------------------
def fusion_ref(fb, ff, w, b, slope=SLOPE):
    return lrelu(F.conv2d(torch.cat([fb, ff], 1), w, b), slope)


def upconv_ref(x, w, b, slope=SLOPE):
    return lrelu(F.pixel_shuffle(F.conv2d(x, w, b, padding=1), 2), slope)


def base_ref(frame):
    return F.interpolate(frame, scale_factor=4, mode="bilinear", align_corners=False)


def last_ref(x, w, b, frame):
    return F.conv2d(x, w, b, padding=1) + base_ref(frame)


def conv_pre(case):
    """the pre-activation (before the shuffle) of a conv case"""
    x = torch.cat([case["fb"], case["ff"]], 1) if case["kind"] == "fusion" else case["x"]
    return F.conv2d(x.double(), case["w"].double(), case["b"].double(), padding=case["w"].shape[-1] // 2)


def conv_exact_ref(case, mode):
    """what the kernel must store, bit for bit: the float64 pre-activation (exact on an exact case), the kernels' own LeakyReLU,
    one rounding to the hot dtype; conv_last adds the base and stores fp32"""
    pre = conv_pre(case)
    if case["kind"] == "last":
        return pre + base_ref(case["frame"].double())
    if case["kind"] != "fusion":
        pre = F.pixel_shuffle(pre, 2)
    return HOT[mode](act_exact(pre))


def conv_ref(case, dtype=torch.float64, hot=ident):
    """the plain operations (slope 0.1) in `dtype`, operands and the stored image rounded by `hot`: the float64 reference of the
    rounded cases (hot = identity) and their yardstick (float32; bf16 rounding in bf16 mode)"""
    t = lambda k: hot(case[k].to(dtype))
    if case["kind"] == "fusion":
        return hot(fusion_ref(t("fb"), t("ff"), t("w"), t("b")))
    if case["kind"] == "last":
        return last_ref(t("x"), t("w"), t("b"), case["frame"].to(dtype))
    return hot(upconv_ref(t("x"), t("w"), t("b")))


_ODD = (1.0, -1.0, 3.0, -3.0, 2.0, -2.0)


def _scaled_biases(ints, exps):
    """ints[k] 2^e, e starting at exps[k] and raised until the value is new: pairwise different, each an odd multiple of a power
    of two.  Returns (biases, the exponents used)."""
    used, out, ex = set(), [], []
    for v, e in zip(ints, exps):
        e = int(e)
        while v * 2.0 ** e in used:
            e += 1
        used.add(v * 2.0 ** e)
        out.append(v * 2.0 ** e)
        ex.append(float(e))
    return torch.tensor(out, dtype=torch.float64), torch.tensor(ex, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def conv_case(kind, f, n, h, w, sd=0):
    """one exact case of one vsr_recon.h kernel.  kind: 'fusion' (1x1, [fb | ff] 2f -> f), 'up1' (3x3, f -> 4f), 'up2' (3x3, f -> 256),
    'last' (3x3, 64 -> 3, + bias + x4 base of an (h/4, w/4) frame; h, w are the conv's size).  Integer network: inputs in {-1, 0, 1},
    weights +-1, two per output row (conv_last: 22) placed so that the rows together use every tap and every input channel -- a
    fusion row reads one backward and one forward channel -- and small odd biases, so that pre-activations of both signs and exact
    zeros occur; every fifth row has its first weight times 2^8 and bias 2, so that its pre-activation is 256 +- 1 + 2: nine
    significant bits, a bf16 tie.  Then a power-of-two scale per channel.  Checked by check_exact_conv() before it is returned."""
    g = torch.Generator().manual_seed(_seed({"fusion": 1, "up1": 2, "up2": 3, "last": 4}[kind], f, n, h, w, sd))
    k = 1 if kind == "fusion" else 3
    ci, co = {"fusion": (2 * f, f), "up1": (f, 4 * f), "up2": (f, 256), "last": (64, 3)}[kind]
    nz = 22 if kind == "last" else 2
    wi = torch.zeros(co, ci, k, k, dtype=torch.float64)
    sg = (torch.randint(0, 2, (co * nz,), generator=g) * 2 - 1).double()
    for i in range(co * nz):
        r, j = divmod(i, nz)
        c, tap = (7 * i + 3) % ci, (2 * i + i // 9) % (k * k)
        if kind == "fusion":
            c = (7 * r + 3) % f if j == 0 else f + (11 * r + 1) % f
        wi[r, c, tap // k, tap % k] = sg[i] * (256.0 if (kind != "last" and j == 0 and r % 5 == 0) else 1.0)
    bi = [2.0 if (kind != "last" and r % 5 == 0) else _ODD[r % 4] for r in range(co)]
    if kind == "last":
        bi = [1.0, -3.0, 5.0]
    sx = 2.0 ** torch.randint(-2, 3, (ci,), generator=g).double()
    b, eo = _scaled_biases(bi, torch.randperm(co, generator=g) % max(8, co // 4) - max(4, co // 8))
    so = 2.0 ** eo
    wt = wi * so.view(-1, 1, 1, 1) / sx.view(1, -1, 1, 1)
    x = torch.randint(-1, 2, (n, ci, h, w), generator=g).double() * sx.view(1, -1, 1, 1)
    case = dict(kind=kind, f=f, w=wt.float(), b=b.float())
    if kind == "fusion":
        case["fb"], case["ff"] = x[:, :f].float(), x[:, f:].float()
    else:
        case["x"] = x.float()
    if kind == "last":
        assert h % 4 == 0 and w % 4 == 0
        case["frame"] = (torch.randint(0, 9, (n, 3, h // 4, w // 4), generator=g).double() / 8.0).float()
    check_exact_conv(case)
    return case


def check_weights(name, w, b, h=3, w_img=3):
    """every tap, every input channel and every output row carry a weight; no two rows are equal; no tap symmetry; biases nonzero
    and pairwise different"""
    if not bool((w != 0).any(0).any(0).all()):
        fail(f"{name}: a tap is zero in every channel pair")
    if not bool((w != 0).any(0).any(1).any(1).all()):
        fail(f"{name}: an input channel carries no weight")
    if not bool((w != 0).any(1).any(1).any(1).all()):
        fail(f"{name}: an output channel carries no weight")
    if torch.unique(w.flatten(1), dim=0).shape[0] != w.shape[0]:
        fail(f"{name}: two output rows are equal")
    if w.shape[-1] > 1:
        need_taps(name, w, h, w_img)
    need_biases(name, b)
    if not bool((w[w != 0].abs() == lowbit(w[w != 0])).all()):
        fail(f"{name}: a weight is not +-2^k")
    if float(w[w != 0].abs().min()) < 2.0 ** -38:
        fail(f"{name}: a weight below 2^-38")


def check_exact_conv(case):
    """the exactness conditions of a conv case, on the float64 reference alone; raises ValueError if one fails.  Returns the number
    of stored values on bf16 ties."""
    kind = case["kind"]
    x = (torch.cat([case["fb"], case["ff"]], 1) if kind == "fusion" else case["x"]).double()
    w, b = case["w"].double(), case["b"].double()
    pad = w.shape[-1] // 2
    check_weights(kind, w, b, x.shape[2], x.shape[3])
    for name, t in (("input", x), ("weight", w), ("bias", b)):
        need_bf16(f"{kind} {name}", t)
    q = torch.minimum((lowbit(w).amin((2, 3)) * chan_quantum(x).view(1, -1)).amin(1), lowbit(b)).view(1, -1, 1, 1)
    mag = F.conv2d(x.abs(), w.abs(), b.abs(), padding=pad)
    need_sum(f"{kind} forward", mag, q)
    pre = conv_pre(case)
    if kind == "last":
        fr = case["frame"].double()
        if not (torch.equal(fr * 8, (fr * 8).round()) and float(fr.min()) >= 0 and float(fr.max()) <= 1):
            fail("frame is not on multiples of 1/8 in [0, 1]")
        base = base_ref(fr)
        need_sum("last + base", mag + base.abs(), torch.minimum(q, torch.tensor(2.0 ** -9, dtype=torch.float64)))
        need_fp32("last + base", pre + base)
        return 0
    need_fp32(f"{kind} pre-activation", pre)
    if x.shape[0] * x.shape[2] * x.shape[3] >= 4 and not (bool((pre > 0).any()) and bool((pre < 0).any()) and bool((pre == 0).any())):
        fail(f"{kind}: the pre-activation lacks a sign or an exact zero")
    return count_ties(act_exact(pre))


# tap-identity sets: ONE weight per output row
def upconv_tap_case(kind, s, h=5, w=6):
    """set s of 9 (f = 64): row co of sub-conv q reads input channel (co + 7 s) % 64 c at tap (s + c // 8 + q) % 9 with weight 2^(q - 1);
    over s = 0..8 every (channel, tap) of each sub-conv occurs once.  Returns (case, table[q][co] = (channel, tap))."""
    g = torch.Generator().manual_seed(_seed(5, s, h, w))
    wt = torch.zeros(256, 64, 3, 3, dtype=torch.float64)
    table = {}
    for q in range(4):
        for co in range(64):
            c = (co + 7 * s) % 64
            tap = (s + c // 8 + q) % 9
            wt[4 * co + q, c, tap // 3, tap % 3] = 2.0 ** (q - 1)
            table[(q, co)] = (c, tap)
    x = torch.randint(-1, 2, (1, 64, h, w), generator=g).double() * (1.0 + torch.arange(64, dtype=torch.float64) % 3).view(1, -1, 1, 1)
    b = torch.zeros(256, dtype=torch.float64)
    return dict(kind=kind, f=64, w=wt.float(), b=b.float(), x=x.float()), table


def upconv_tap_sets_cover():
    """every (sub-conv, tap, channel) occurs in exactly one set"""
    seen = set()
    for s in range(9):
        _, table = upconv_tap_case("up2", s, 1, 1)
        for (q, co), (c, tap) in table.items():
            seen.add((q, c, tap))
    return len(seen) == 4 * 9 * 64


def last_tap_case(s, h=20, w=36):
    """set s of 9: the three rows read ALL 64 channels at ONE tap each -- row o at tap (s + 3 o) % 9 -- with weights +-2^k that differ
    per channel (k = c % 5 - 2, sign by c and o), on an input with one live channel per pixel ((3 y + 5 x + s) % 64): an output pixel
    is one weight times one input, so a wrong tap, channel or row shows at once.  Over s = 0..8 each row sees every tap with every
    channel."""
    wt = torch.zeros(3, 64, 3, 3, dtype=torch.float64)
    c = torch.arange(64)
    for o in range(3):
        tap = (s + 3 * o) % 9
        wt[o, :, tap // 3, tap % 3] = 2.0 ** (c % 5 - 2).double() * (1.0 - 2.0 * ((c // 5 + o) % 2).double())
    x = torch.zeros(1, 64, h, w, dtype=torch.float64)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    x[0, (3 * yy + 5 * xx + s) % 64, yy, xx] = 1.0 + ((yy + xx) % 2).double()
    fr = ((torch.arange(3 * (h // 4) * (w // 4)) * 3 + s) % 9).double().view(1, 3, h // 4, w // 4) / 8.0
    return dict(kind="last", f=64, w=wt.float(), b=torch.tensor([0.5, -0.25, 2.0]), x=x.float(), frame=fr.float())


def rounded_conv_case(kind, f, n, h, w, sd=0):
    g = torch.Generator().manual_seed(_seed(6, {"fusion": 1, "up1": 2, "up2": 3, "last": 4}[kind], f, n, h, w, sd))
    rn = lambda *s: torch.randn(*s, generator=g)
    k = 1 if kind == "fusion" else 3
    ci, co = {"fusion": (2 * f, f), "up1": (f, 4 * f), "up2": (f, 256), "last": (64, 3)}[kind]
    case = dict(kind=kind, f=f, w=rn(co, ci, k, k) / (k * ci ** 0.5), b=0.1 * rn(co))
    if kind == "fusion":
        case["fb"], case["ff"] = rn(n, f, h, w), rn(n, f, h, w)
    else:
        case["x"] = rn(n, ci, h, w)
    if kind == "last":
        case["frame"] = torch.rand(n, 3, h // 4, w // 4, generator=g)
    return case


def rounded_conv_reference(case, mode):
    """(float64 reference, yardstick).  conv_last reads a hot-dtype image and hot-dtype weights, so in bf16 mode its INPUT is part
    of the case: the reference is taken on the rounded operands (nothing else rounds there), the yardstick is float32."""
    if case["kind"] == "last" and mode == "bf16":
        case = dict(case, x=bf16_round(case["x"]), w=bf16_round(case["w"]), b=bf16_round(case["b"]))
        ref = conv_ref(case)
        return ref, rel_max(conv_ref(case, torch.float32), ref), case
    ref = conv_ref(case)
    return ref, rel_max(conv_ref(case, torch.float32, HOT[mode]), ref), case


# ---- MotionVectorVSR side --------------------------------------------------------------------------------------------------------
def mv_lambda32(h, fused=False):
    """csrc/mv_recon.h's mv_lambda for d = 0 .. 4h - 1 in fp32 arithmetic (numpy float32; `fused`: scale (d + 0.5) - 0.5 as one fma)
    -> (lambda, 1 - lambda) as float64 arrays"""
    f32 = np.float32
    d = np.arange(4 * h).astype(f32)
    scale = f32(4 * h + 1) / f32(4 * h)
    if fused:
        t = (scale.astype(np.float64) * (d + f32(0.5)).astype(np.float64) - 0.5).astype(f32)
    else:
        t = (scale * (d + f32(0.5))).astype(f32) - f32(0.5)
    lam = np.clip((t - d).astype(f32), f32(0), f32(1))
    return lam.astype(np.float64), (f32(1) - lam).astype(np.float64)


def is_pow2(v):
    return v & (v - 1) == 0


def _lambdas(h, w, dtype):
    """(ly (4h, 1), 1 - ly, lx (1, 4w), 1 - lx): (2d + 1) / 8h in float64; in float32 as ATen's upsample_bilinear2d and the kernels
    compute them, through the fp32 scale (4h + 1) / 4h (mv_lambda32) -- off by up to 4h ulp on sizes that are no power of two,
    which is part of the precision of the float32 operation and so of the yardstick"""
    if dtype == torch.float64:
        ly, lx = M.lambdas(h).view(-1, 1), M.lambdas(w).view(1, -1)
        return ly, 1 - ly, lx, 1 - lx
    (ly, my), (lx, mx) = mv_lambda32(h), mv_lambda32(w)
    t = lambda a: torch.from_numpy(a).to(dtype)
    return t(ly).view(-1, 1), t(my).view(-1, 1), t(lx).view(1, -1), t(mx).view(1, -1)


def _blend(D, ly, my, lx, mx):
    """M.blend with given weights: columns, then rows"""
    top = mx * D[..., :-1] + lx * D[..., 1:]
    return my * top[..., :-1, :] + ly * top[..., 1:, :]


def _blend_T(g, ly, my, lx, mx):
    """M.blend_T with given weights"""
    cols = F.pad(mx * g, (0, 1)) + F.pad(lx * g, (1, 0))
    return F.pad(my * cols, (0, 0, 0, 1)) + F.pad(ly * cols, (0, 0, 1, 0))


def mv_out_exact(case):
    """whether the blend (and with it out, dD and every gradient) is bit-exact on this case: h and w powers of two (lambda), and in
    a rich case 64 h w <= 2^8 -- a negative u = bf16(fp32(0.1f t)) has eight bits of its own below D's integers, so the 17 bits the
    blend adds at 32 x 64 do not fit; u itself is exact on every case"""
    h, w = case["fb"].shape[-2:]
    return is_pow2(h) and is_pow2(w) and (not case.get("rich") or 64 * h * w <= 256)


def mv_run(case, dtype=torch.float64, hot=ident, slope=SLOPE, exact_act=False, drop=()):
    """forward and (with a cotangent 'g') backward of a MotionVectorVSR reconstruction case in `dtype`.  Tensors are (N, C, h, w)
    with N = frames x clips, frame-major.  hot: the rounding of the hot dtype, applied at the stated rounding points (operands,
    u, dD as an operand, dpre, dc); drop: names among 'dD', 'dpre' whose rounding is left out (the host's dropped-rounding test).
    exact_act: the kernels' LeakyReLU (act_exact) instead of slope * t.  Returns dict(out, u, D, and dc, dW_fu, db_fu, dW_last,
    db_last, dD, du, dpre)."""
    t = lambda k: hot(case[k].to(dtype))
    fb, ff, w_fu, b_fu, w_last, b_last = t("fb"), t("ff"), t("w_fu"), t("b_fu"), t("w_last"), t("b_last")
    c = torch.cat([fb, ff], 1)
    pre = torch.einsum("oi,nihw->nohw", w_fu.reshape(w_fu.shape[0], -1), c) + b_fu.view(1, -1, 1, 1)
    u = hot(act_exact(pre) if exact_act else lrelu(pre, slope))
    D = M.phase_D(u, w_last, b_last)
    lam = _lambdas(D.shape[-2] // 4, D.shape[-1] // 4, dtype)
    res = dict(out=_blend(D, *lam) + M.base(case["x"].to(dtype)), u=u, D=D, pre=pre, c=c)
    if "g" not in case:
        return res
    g = case["g"].to(dtype)
    dD = _blend_T(g, *lam)
    dDh = dD if "dD" in drop else hot(dD)
    dE = M.gather_dE(dDh)
    du = torch.einsum("nohkwl,cokl->nchw", dE, w_last)
    dneg = (du * SLOPE32).float().to(dtype) if exact_act else slope * du
    dpre = torch.where(u > 0, du, dneg)
    if "dpre" not in drop:
        dpre = hot(dpre)
    wf = w_fu.reshape(w_fu.shape[0], -1)
    res.update(dc=hot(torch.einsum("oi,nohw->nihw", wf, dpre)), dW_fu=torch.einsum("nohw,nihw->oi", dpre, c).view_as(w_fu),
               db_fu=dpre.sum((0, 2, 3)), dW_last=torch.einsum("nchw,nohkwl->cokl", u, dE), db_last=g.sum((0, 2, 3)), dD=dD, dDh=dDh,
               du=du, dpre=dpre)
    return res


MV_GRADS = ("dW_fu", "db_fu", "dW_last", "db_last")


def mv_exact_ref(case, mode, drop=()):
    return mv_run(case, torch.float64, HOT[mode], exact_act=True, drop=drop)


def emulate_mv(case, mode):
    """the yardstick of the rounded cases: the reference in float32; bf16 mode rounds the states, the blob's weights and biases and
    every stated rounding point"""
    return mv_run(case, torch.float32, HOT[mode])


# budget of sum |u| |dE| over the clip in quanta: see mv_case
_DW_BUDGET = 2.0 ** 21


@functools.lru_cache(maxsize=None)
def mv_case(f, b, n, h, w, rich=False, backward=True, sd=0, dense=False):
    """one exact case of mv_recon.h on b clips of n frames of h x w: N = n b images, frame-major.

    Integer network.  States in {-1, 0, 1}; a fusion row reads one backward and one forward channel (+-1) and has an odd bias: 3, 5
    or 7 in a plain case, so that the pre-activation is positive (1 .. 9) and u an integer of four bits; conv_last has 2 (2f <= 48)
    or 4 weights +-1 per row (o, ky, kx) over the u channels, biases 1, -3, 5.  D is then an integer of at most 7 bits, times the
    scale of its plane, and with h and w powers of two the blend adds log2(64 h w) <= 17 bits: inside 24.
    rich (bf16 only, small images): biases 1, -1, 3, -3, so both signs and zeros occur -- a negative u is bf16(fp32(0.1f t)), eight
    bits of its own -- and, in a forward-only case, every fifth fusion row has its first weight times 2^8 and bias 2, so that its u is
    a bf16 tie.
    Frames on multiples of 1/8.  Cotangent in {-1, 0, 1} 2^k per plane; its density is a quarter where the weight-gradient sums
    allow it: sum |u| |dE| over the clip is about 9/16 N h w 16 density units against a quantum of 1 / (64 h w), so the density is
    min(1/4, 2^21 / (9 N (h w)^2 64)) (a power of two) -- check_exact_mv() verifies the sums themselves.
    dense: the cotangent is a quarter nonzero whatever the size.  dD, du, dpre, dc and db_last sum per pixel (or few bits) and stay
    bit-exact; dW_last, dW_fu and db_fu, which sum over every pixel of the clip, then leave the 24 bits and are held by grad_bounds()
    (fp32) or the yardstick (bf16) instead -- the sparse twin of the same geometry holds them bit for bit.  A rich dense case
    (bf16, both signs at tile sizes) has u bit-exact, out within blend_bound, and dc bit-exact wherever its two terms fit 24 bits
    together (case['dc_exact'], from the reference alone; at least 90 % of the elements)."""
    g = torch.Generator().manual_seed(_seed(7, f, b, n, h, w, int(rich), sd, int(dense)))
    N, f2 = n * b, 2 * f
    ties = rich and not backward       # (a tie row's 2^8 weight next to a plain one would cost dc's sum 8 bits more than it has)
    wfi = torch.zeros(f2, f2, dtype=torch.float64)
    sg = (torch.randint(0, 2, (f2, 2), generator=g) * 2 - 1).double()
    for r in range(f2):
        wfi[r, (7 * r + 3) % f] = sg[r, 0] * (256.0 if ties and r % 5 == 0 else 1.0)
        wfi[r, f + (11 * r + 1 + r // f) % f] = sg[r, 1]
    bfi = [(2.0 / 256.0 if ties and r % 5 == 0 else _ODD[r % 4]) if rich else 3.0 + 2.0 * (r % 3) for r in range(f2)]
    sx = 2.0 ** torch.randint(-2, 3, (f2,), generator=g).double()
    b_fu, eu = _scaled_biases(bfi, torch.randperm(f2, generator=g) % max(3, f2 // 3) - max(1, f2 // 6))
    tie = torch.tensor([ties and r % 5 == 0 for r in range(f2)])
    su_read = 2.0 ** eu                                  # a tie row's u is 259 / 256: conv_last reads it on the scale of the others
    su = torch.where(tie, su_read / 256.0, su_read)
    nz = 2 if f2 <= 48 else 4
    wli = torch.zeros(f2, 75, dtype=torch.float64)
    sl = (torch.randint(0, 2, (75, nz), generator=g) * 2 - 1).double()
    for r in range(75):
        for j in range(nz):
            i = nz * r + j
            wli[(7 * i + 3 + i // f2) % f2, r] = sl[r, j]
    so = torch.tensor([0.5, 2.0, 1.0], dtype=torch.float64)
    w_last = wli.view(f2, 3, 5, 5) * so.view(1, 3, 1, 1) / su_read.view(-1, 1, 1, 1)
    b_last = torch.tensor([1.0, -3.0, 5.0], dtype=torch.float64) * so
    ci = torch.randint(-1, 2, (N, f2, h, w), generator=g).double()
    cs = ci * sx.view(1, -1, 1, 1)
    case = dict(f=f, b=b, n=n, rich=rich, dense=dense, fb=cs[:, :f].float(), ff=cs[:, f:].float(),
                x=(torch.randint(0, 9, (N, 3, h, w), generator=g).double() / 8.0).float(),
                w_fu=(wfi * su.view(-1, 1) / sx.view(1, -1)).view(f2, f2, 1, 1).float(), b_fu=b_fu.float(), w_last=w_last.float(),
                b_last=b_last.float())
    if backward:
        dens = 0.25 if dense else min(0.25, 2.0 ** np.floor(np.log2(_DW_BUDGET / (9.0 * N * (h * w) ** 2 * 64.0))))
        gi = torch.randint(-1, 2, (N, 3, 4 * h, 4 * w), generator=g).double() * (torch.rand(N, 3, 4 * h, 4 * w, generator=g) < dens * 1.5).double()
        case["g"] = (gi * torch.tensor([1.0, 0.5, 4.0], dtype=torch.float64).view(1, 3, 1, 1)).float()
        case["density"] = float((gi != 0).double().mean())
    case["ties"] = check_exact_mv(case, "bf16" if rich else "both")
    return case


def _q_rows(wq, qin):
    """(rows,) lattice of sum_k w[row, k] in[k]: wq (rows, k) = lowbit of the weights (2^200 where zero), qin (k,)"""
    return (wq * qin.view(1, -1)).amin(1)


def _elem_exact(wf, x):
    """per element of sum_o wf[o, i] x[n, o, y, x]: whether sum |terms| < 2^24 quanta of the element's OWN lattice (the smallest
    low bit among its terms)"""
    n, _, h, w = x.shape
    q = torch.full((n, wf.shape[1], h, w), BIG_Q, dtype=torch.float64)
    mag = torch.zeros_like(q)
    for o, i in (wf != 0).nonzero().tolist():
        term = wf[o, i] * x[:, o]
        q[:, i] = torch.minimum(q[:, i], lowbit(term))
        mag[:, i] += term.abs()
    return mag / q < 2.0 ** 24


def grad_bounds(case, ref):
    """fp32, per element: what each gradient may differ from the float64 reference, from MAGNITUDES (|g|, |W|, |u|, |c| through the
    same sums, LeakyReLU slope taken as 1), as tests/test_gpu_mv_recon.py's edge test derives it.  A blend weight is off by up to
    4 max(h, w) ulp of 1 ABSOLUTELY on sizes that are no power of two (0 on powers of two), and every tap of dD carries two of
    them: lam = 2 * 4 max(h, w) 2^-23 against the plain sum of |g| over the four taps.  On top, a sum of n terms in fp32 is off by
    at most n 2^-24 times the sum of the magnitudes, whatever its order: n = 8 (dD: four taps, products and sums) + 96 (du: 75 rows
    padded to 96) + 2 (dpre) + 64 (dc: 48 channels padded to 64) for dc; 8 + 96 + 2 + P for dW_fu and db_fu, 8 + P for dW_last, with
    P = N x (h, w rounded up to 8 x 16 tiles) pixels + 1024 slabs; 16 N h w + 256 + 1024 for db_last (no blend weight in it)."""
    h, w = case["fb"].shape[-2:]
    N = case["fb"].shape[0]
    lam = 0.0 if (is_pow2(h) and is_pow2(w)) else 8 * max(h, w) * 2.0 ** -23
    P = N * (-(-h // 8) * 8) * (-(-w // 16) * 16) + 1024
    g = case["g"].double().abs()
    box = F.pad(g, (0, 1)) + F.pad(g, (1, 0))
    dDm = F.pad(box, (0, 0, 0, 1)) + F.pad(box, (0, 0, 1, 0))
    dEm = M.gather_dE(dDm)
    wl, wf = case["w_last"].double().abs(), case["w_fu"].double().abs().flatten(1)
    dum = torch.einsum("nohkwl,cokl->nchw", dEm, wl)
    u2 = 2.0 ** -24
    return dict(dc=(lam + 170 * u2) * torch.einsum("oi,nohw->nihw", wf, dum),
                dW_fu=(lam + (106 + P) * u2) * torch.einsum("nohw,nihw->oi", dum, ref["c"].abs()).view_as(case["w_fu"]),
                db_fu=(lam + (106 + P) * u2) * dum.sum((0, 2, 3)),
                dW_last=(lam + (8 + P) * u2) * torch.einsum("nchw,nohkwl->cokl", ref["u"].abs(), dEm),
                db_last=(16 * N * h * w + 1280) * u2 * g.sum((0, 2, 3)))


def check_exact_mv(case, modes="both"):
    """the exactness conditions of an mv_recon.h case on the float64 reference alone, in each mode it is meant for; raises
    ValueError if one fails.  Returns {mode: {rounding point: number of values on bf16 ties}}."""
    f2 = case["w_fu"].shape[0]
    h, w = case["fb"].shape[-2:]
    pow2, lam_ok = mv_out_exact(case), is_pow2(h) and is_pow2(w)
    w_fu, b_fu, w_last, b_last = (case[k].double() for k in ("w_fu", "b_fu", "w_last", "b_last"))
    wf = w_fu.view(f2, f2)
    check_weights("fusion", w_fu, b_fu)
    check_weights("conv_last", w_last.permute(1, 2, 3, 0).reshape(75, f2, 1, 1), torch.arange(1.0, 76.0))
    need_taps("conv_last", w_last)
    need_biases("conv_last", b_last)
    half = wf != 0
    if not bool((half[:, :f2 // 2].sum(1) == 1).all() and (half[:, f2 // 2:].sum(1) == 1).all()):
        fail("a fusion row does not read one backward and one forward channel")
    for k in ("fb", "ff", "w_fu", "b_fu", "w_last", "b_last"):
        need_bf16(k, case[k].double())
    xf = case["x"].double()
    if not (torch.equal(xf * 8, (xf * 8).round()) and float(xf.min()) >= 0 and float(xf.max()) <= 1):
        fail("frames are not on multiples of 1/8 in [0, 1]")
    ties = {}
    cv = lambda t: t.view(1, -1, 1, 1)
    tiny = torch.tensor(2.0 ** -9, dtype=torch.float64)
    for mode in (("fp32", "bf16") if modes == "both" else (modes,)):
        r = mv_exact_ref(case, mode)
        c, u, pre = r["c"], r["u"], r["pre"]
        qc = chan_quantum(c)
        need_sum("fusion", torch.einsum("oi,nihw->nohw", wf.abs(), c.abs()) + cv(b_fu.abs()), cv(torch.minimum(_q_rows(lowbit(wf), qc), lowbit(b_fu))))
        need_fp32("pre", pre)
        if mode == "fp32" and not bool((pre > 0).all()):
            fail("fp32: a fusion pre-activation is not positive (0.1f t carries 24 bits into the next contraction)")
        if mode == "bf16" and case.get("rich") and c.shape[0] * h * w >= 4 and not (bool((pre < 0).any()) and bool((pre > 0).any()) and bool((pre == 0).any())):
            fail("rich case lacks a sign or an exact zero")
        need_fp32("u", u)
        qu = chan_quantum(u)
        wl = w_last.reshape(f2, 75)
        qE = _q_rows(lowbit(wl).t(), qu)                                     # (75,)
        Eabs = torch.einsum("nchw,cr->nrhw", u.abs(), wl.abs())
        need_sum("E", Eabs, cv(qE))
        qD = torch.minimum(qE.view(3, 25).amin(1), lowbit(b_last))          # (3,)
        Dabs = M.phase_D(u.abs(), w_last.abs(), b_last.abs())
        need_sum("D", Dabs, cv(qD))
        need_fp32("D", r["D"])
        t = dict(u=count_ties(act_exact(pre)))
        if pow2:
            lx = M.lambdas(w).view(1, -1)
            ly = M.lambdas(h).view(-1, 1)
            rows_abs = (1 - lx) * Dabs[..., :-1] + lx * Dabs[..., 1:]
            need_sum("blend columns", rows_abs, cv(qD) / (8 * w))
            need_fp32("blend columns", (1 - lx) * r["D"][..., :-1] + lx * r["D"][..., 1:])
            need_sum("blend rows", (1 - ly) * rows_abs[..., :-1, :] + ly * rows_abs[..., 1:, :], cv(qD) / (64 * h * w))
            bl = M.blend(r["D"])
            need_fp32("blend", bl)
            need_sum("out", M.blend(Dabs) + M.base(xf), torch.minimum(cv(qD) / (64 * h * w), tiny))
            need_fp32("out", r["out"])
        if "g" in case and lam_ok:
            g = case["g"].double()
            qg = chan_quantum(g)
            need_sum("dD", M.blend_T(g.abs()), cv(qg) / (64 * h * w))
            need_fp32("dD", r["dD"])
            need_sum("db_last", g.abs().sum((0, 2, 3)), qg)
            dDh = r["dDh"]
            qd = chan_quantum(dDh)                                           # (3,)
            dEabs = M.gather_dE(dDh.abs())
            q_du = _q_rows(lowbit(wl), qd.repeat_interleave(25))             # (f2,)
            need_sum("du", torch.einsum("nohkwl,cokl->nchw", dEabs, w_last.abs()), cv(q_du))
            need_fp32("du", r["du"])
            dpre = r["dpre"]
            qp = chan_quantum(dpre)
            if case.get("rich") and not pow2:
                case["dc_exact"] = _elem_exact(wf, dpre)
                if float(case["dc_exact"].double().mean()) < 0.9:
                    fail("dc: fewer than 90 % of the elements sum exactly")
            else:
                need_sum("dc", torch.einsum("oi,nohw->nihw", wf.abs(), dpre.abs()), cv(_q_rows(lowbit(wf).t(), qp)))
                need_fp32("dc", r["dc"])
            if not case.get("dense"):
                need_sum("dW_fu", torch.einsum("nohw,nihw->oi", dpre.abs(), c.abs()), qp.view(-1, 1) * qc.view(1, -1))
                need_sum("db_fu", dpre.abs().sum((0, 2, 3)), qp)
                need_sum("dW_last", torch.einsum("nchw,nohkwl->cokl", u.abs(), dEabs), qu.view(-1, 1, 1, 1) * qd.view(1, 3, 1, 1))
                for k in MV_GRADS:
                    need_fp32(k, r[k])
            if not all(bool((r[k] != 0).any()) for k in ("dc",) + MV_GRADS):
                fail("a gradient is all zero")
            t.update(dD=count_ties(r["dD"]), dpre=count_ties(torch.where(u > 0, r["du"], (r["du"] * SLOPE32).float().double())),
                     dc=count_ties(torch.einsum("oi,nohw->nihw", wf, dpre)))
        ties[mode] = t
    return ties


@functools.lru_cache(maxsize=None)
def mv_tap_case(s, f=20, h=16, w=32):
    """tap-identity set s of 2 (F = 20: 40 u channels, 75 rows): identity fusion with bias 0 on positive one-hot states, so u IS the
    state; u channel k carries conv_last row r = 40 s + k (r < 75) alone, weight 2^(k % 3); bias 0.  Channel k is 1 or 2 where
    (y + 2x + k) % 3 != 0 and on the whole of LR rows 7 and h - 1 and columns 15 and w - 1 (the last before the 8 x 16 tile seam and the
    last of the image), zero elsewhere, so D's [i = 0], [j = 0] and [i = j = 0] neighbour terms -- across a seam and into image row
    4h / column 4w -- are each one placed copy of one tap for EVERY row (tests/test_recon_ref_host.py asserts it)."""
    f2 = 2 * f
    w_last = torch.zeros(f2, 75, dtype=torch.float64)
    rows = {}
    for k in range(f2):
        r = f2 * s + k
        if r < 75:
            w_last[k, r] = 2.0 ** (k % 3)
            rows[k] = r
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    c = torch.zeros(1, f2, h, w, dtype=torch.float64)
    for k in range(f2):
        live = (((yy + 2 * xx + k) % 3) != 0) | (yy == 7) | (yy == h - 1) | (xx == 15) | (xx == w - 1)
        c[0, k] = live.double() * (1.0 + (yy + xx + k) % 2)
    g = torch.Generator().manual_seed(_seed(8, s, h, w))
    gi = torch.randint(-1, 2, (1, 3, 4 * h, 4 * w), generator=g).double() * (torch.rand(1, 3, 4 * h, 4 * w, generator=g) < 0.02).double()
    case = dict(f=f, b=1, n=1, fb=c[:, :f].float(), ff=c[:, f:].float(), x=torch.zeros(1, 3, h, w),
                w_fu=torch.eye(f2).view(f2, f2, 1, 1), b_fu=torch.zeros(f2), w_last=w_last.view(f2, 3, 5, 5).float(), b_last=torch.zeros(3),
                g=gi.float(), rows=rows)
    return case


def name_mv_tap(case, got, exp):
    """the (o, ky, kx) and phase (i, j) of the first wrong output pixel of a tap-identity case"""
    ne = ((got != exp) | (got != got)).nonzero()
    if ne.numel() == 0:
        return None
    n, o, Y, X = ne[0].tolist()
    return f"plane o={o} pixel ({Y}, {X}): D phase (i, j) = ({Y % 4}, {X % 4}) or its neighbour; rows of plane o: taps (ky, kx) = " \
           f"({Y % 4} | 4 if i = 0, {X % 4} | 4 if j = 0); got {got[n, o, Y, X].item()} expected {exp[n, o, Y, X].item()}"


def mv_rounded_case(f, b, n, h, w, sd=0):
    g = torch.Generator().manual_seed(_seed(9, f, b, n, h, w, sd))
    rn = lambda *s: torch.randn(*s, generator=g)
    N, f2 = n * b, 2 * f
    return dict(f=f, b=b, n=n, fb=rn(N, f, h, w), ff=rn(N, f, h, w), x=torch.rand(N, 3, h, w, generator=g), w_fu=rn(f2, f2, 1, 1) / f2 ** 0.5,
                b_fu=0.1 * rn(f2), w_last=rn(f2, 3, 5, 5) / f2 ** 0.5, b_last=0.1 * rn(3), g=rn(N, 3, 4 * h, 4 * w))


MV_TENSORS = ("out", "u", "dc") + MV_GRADS


def mv_rounded_reference(case, mode):
    """(float64 reference dict, yardstick per tensor name)"""
    ref = mv_run(case)
    emu = emulate_mv(case, mode)
    return ref, {k: rel_max(emu[k], ref[k]) for k in MV_TENSORS}


def blend_bound(D, h, w):
    """per output element, what the fp32 blend may differ from the float64 blend of an EXACT D (non-power-of-two sizes): each of
    the two lambdas is off by at most 4 max(h, w) ulp of 1 (2^-23; tests/test_gpu_mv_recon.py derives it: the fp32 scale (4h + 1) /
    4h is off by half an ulp, multiplied by up to 4h), absolutely, and so is its complement; each tap value passes through two
    products and two sums, each rounded once (2^-24 relative to a magnitude below the sum of the four taps), and the base adds one
    more rounding of the result.  With S = |D00| + |D01| + |D10| + |D11| of the element:
        |got - ref| <= (2 * 4 max(h, w) 2^-23 + 6 * 2^-24) S + 2^-24 |out|
    What this leaves for structural errors: at 25 x 49 the bound is about 4.7e-5 S, with S up to 4 x 127 quanta of D about 0.024
    quanta, while ONE quantum misplaced at the smallest blend weight 1 / (8 x 49) moves the output by 0.0026 quanta only -- such a
    corner case can hide; a wrong tap or pixel typically moves an element by a good fraction of a quantum, ten to a thousand times
    the bound, and u is held bit for bit beside it."""
    a = D.abs()
    S = a[..., :-1, :-1] + a[..., :-1, 1:] + a[..., 1:, :-1] + a[..., 1:, 1:]
    return (8 * max(h, w) * 2.0 ** -23 + 6 * 2.0 ** -24) * S


# ---- geometries ----------------------------------------------------------------------------------------------------------------
VSR_GEOMETRIES = ((1, 1, 1), (1, 1, 17), (1, 17, 1), (1, 3, 3), (1, 15, 15), (1, 16, 16), (1, 17, 17), (1, 16, 17), (1, 17, 16),
                  (2, 33, 35), (3, 17, 17))
LAST_GEOMETRIES = ((1, 1, 1), (1, 1, 9), (1, 9, 1), (1, 4, 4), (1, 4, 5), (1, 5, 4), (1, 5, 5), (2, 9, 10))     # low-resolution sizes
MV_EXACT = ((1, 1, 1), (1, 2, 2), (1, 1, 32), (1, 32, 1), (1, 4, 8), (1, 8, 16), (1, 16, 16), (1, 8, 32), (2, 16, 32), (1, 32, 64))
MV_RICH = ((1, 1, 1), (1, 2, 2), (2, 2, 2), (1, 1, 4))               # both signs, forward and backward: mv_out_exact
MV_RICH_TILES = ((1, 8, 16), (1, 16, 16), (2, 16, 32))                # both signs, dense cotangent, tile-sized: dc_exact
MV_RICH_FORWARD = ((1, 1, 1), (1, 2, 2), (1, 4, 8), (1, 8, 16), (2, 16, 32), (1, 9, 17))   # u exact; out exact or within blend_bound
MV_BOUNDED = ((1, 7, 15), (1, 8, 17), (1, 9, 16), (1, 9, 17), (1, 12, 16), (1, 18, 20), (2, 25, 49))
MV_WIDTHS = (20, 24, 40, 64)
MV_CHUNKS = (17, 33)
MV_WALK = (2, 3, 16, 32)
MV_WALK_WGS = (1, 5, 23, 24, 25, 128)
MV_ROUNDED = ((1, 18, 20), (1, 16, 32), (2, 25, 49))
VSR_ROUNDED = ((1, 17, 17), (2, 33, 35))
