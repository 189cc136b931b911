"""The NAS supernet block written out in plain torch on the CPU, plus the case generators of the NAS block parity tests.
Nothing of the package or of the oracle is used here: this is the outside reference that csrc/nas_block.h, csrc/nas_dw_lc.h
and csrc/nas_bwd_fused.h are held against.  tests/test_nas_ref_host.py pins it to oracle.wdsr_oracle (which G6 / G10 pin to
the reference project) and checks on the CPU that every exact case satisfies its exactness conditions.

  y = beta1 (mg yin) + beta2 (mg yin + ms sum_k p_k relu(pw_k(relu(dw_k(ms mg yin) + bd_k)) + bp_k)),   k = 3x3, 5x5, 7x7

(include/sr_hotpath.h; the gate written out as oracle.nas_block_forward has it).  Every input is a leaf -- mg, ms, p and beta
included -- so autograd yields the eleven gradients of _NasBlockFunction.backward.  Activations are NHWC as the kernels take
them.

Two families of cases:
  exact     dyadic data on which every intermediate is its own bf16 rounding and every reduction satisfies
            sum |terms| < 2^24 quanta, so fp32 accumulation is exact in ANY order: a kernel must return the float64 reference bit
            for bit, in fp32 and in bf16, whatever its summation order or rounding points (check_exact() verifies the
            conditions on the float64 reference alone and raises if one fails);
  rounded   random normal data; the bound comes from an emulation of the kernels' precision on the CPU (emulate()).

The conditions named need_* / is_*, the roundings, the seed recipe and the bound of the rounded cases are tests/parity_kit.py's,
shared by all parity suites and pinned by tests/test_parity_kit_host.py.
"""
import functools

import torch
import torch.nn.functional as F_

from tests.parity_kit import RoundBackward, RoundForward, bf16_round, fail, need_bf16, need_fp32, need_sum, rel_max

KS = (3, 5, 7)
GRAD_NAMES = ("gyin", "g_wdw3", "g_wdw5", "g_wdw7", "g_bdw", "g_wpw", "g_bpw", "g_mg", "g_ms", "g_p", "g_beta")
PARAM_NAMES = ("wdw3", "wdw5", "wdw7", "bdw", "wpw", "bpw", "mg", "ms", "p", "beta")
TILE_H, TILE_W = 12, 24


def n_tiles(n, h, w):
    return n * ((h + TILE_H - 1) // TILE_H) * ((w + TILE_W - 1) // TILE_W)


class _BranchTailRounded(torch.autograd.Function):
    """beta2 ms p_k relu(pw_k(v) + bp_k) with the backward as the bf16 kernels arrange it: the matrix cores take bf16 operands, so
    the factor c_k[co] = p_k beta2 ms[co] of the upstream gradient gu = c_k gy 1(u > 0) cannot ride on fp32 values; the kernels
    fold it into the backward weights, rounded once -- GZ = (rnd(Wpw^T diag(c_k))) (gy 1(u > 0)) -- and apply it to the weight
    and bias sums in fp32 afterwards.  (Rounding gu instead would cost the same one rounding per term.)"""

    @staticmethod
    def forward(ctx, v, w, b, pk, b2, ms, rnd):
        u = F_.conv2d(v, w, b)
        r = torch.relu(u)
        ctx.save_for_backward(v, w, u, r, pk, b2, ms)
        ctx.rnd = rnd
        return (pk * b2 * ms).view(1, -1, 1, 1) * r

    @staticmethod
    def backward(ctx, g):
        v, w, u, r, pk, b2, ms = ctx.saved_tensors
        f = ms.numel()
        c = pk * b2 * ms
        m = g * (u > 0)
        gv = F_.conv_transpose2d(m, ctx.rnd(w * c.view(f, 1, 1, 1)))
        gw = c.view(f, 1, 1, 1) * torch.einsum("nohw,nihw->oi", m, v).view(f, f, 1, 1)
        gb = (c.view(1, f, 1, 1) * m).sum((0, 2, 3))                     # (the kernels scale partial sums, then add them)
        rr = (g * r).sum((0, 2, 3))                                      # r_k[c] = sum gy relu(u_k)
        q = (ms * rr).sum()
        return gv, gw, gb, b2 * q, pk * q, b2 * pk * rr, None


def nas_block_ref(yin, wdw3, wdw5, wdw7, bdw, wpw, bpw, mg, ms, p, beta, rnd=None, inter=None):
    """yin (n, h, w, f); wdwk (f, 1, k, k); bdw, bpw (3, f); wpw (3, f, f, 1, 1); mg, ms (f,); p (3,); beta (2,): all of one
    dtype (float64 for the reference).  Returns y (n, h, w, f).  rnd: None for the reference; else the rounding applied
    where the bf16 kernels round -- V, y and (on the way back) GZ, the tensors include/sr_hotpath.h stores in the activation
    type, and the scaled backward weights of _BranchTailRounded.  inter (reference only): a dict that receives every
    intermediate tensor formed here (NCHW), each with its gradient retained."""
    assert rnd is None or inter is None
    f = yin.shape[3]
    keep = {}
    cv = lambda t: t.view(1, f, 1, 1)
    xg = yin.permute(0, 3, 1, 2) * cv(mg)                               # global mask
    x1 = xg * cv(ms)                                                    # masked input of the three branches
    keep["xg"], keep["x1"] = xg, x1
    s = None
    for k, (ks, wd) in enumerate(zip(KS, (wdw3, wdw5, wdw7))):
        z = F_.conv2d(x1, wd, bdw[k], padding=ks // 2, groups=f)        # depthwise pre-activation; its gradient is GZ_k
        keep[f"z{k}"] = z
        if rnd is not None:
            v = RoundForward.apply(torch.relu(RoundBackward.apply(z, rnd)), rnd)
            t = _BranchTailRounded.apply(v, wpw[k], bpw[k], p[k], beta[1], ms, rnd)
        else:
            v = torch.relu(z)
            u = F_.conv2d(v, wpw[k], bpw[k])                            # pointwise pre-activation
            t = p[k] * torch.relu(u)
            keep[f"v{k}"], keep[f"u{k}"], keep[f"t{k}"] = v, u, t
        s = t if s is None else s + t
    keep["s"] = s
    if rnd is not None:
        y = RoundForward.apply((beta[0] + beta[1]) * xg + s, rnd)      # (s carries beta2 ms here)
    else:
        y = beta[0] * xg + beta[1] * (xg + cv(ms) * s)
    keep["y"] = y
    if inter is not None:
        for name, t in keep.items():
            if t.requires_grad:
                t.retain_grad()
            inter[name] = t
    return y.permute(0, 2, 3, 1)


def nas_body_ref(y0, WDW3, WDW5, WDW7, BDW, WPW, BPW, mg, MS, P, BETA, rnd=None, inter=None):
    """nb blocks one after the other, inputs stacked over blocks as _NasBodyFunction takes them (mg is shared);
    inter: a list that receives one dict of intermediates per block"""
    y = y0
    for b in range(WDW3.shape[0]):
        d = None
        if inter is not None:
            d = {}
            inter.append(d)
        y = nas_block_ref(y, WDW3[b], WDW5[b], WDW7[b], BDW[b], WPW[b], BPW[b], mg, MS[b], P[b], BETA[b], rnd, d)
    return y


def _leaves(case, dtype):
    return [case[k].detach().to(dtype, copy=True).requires_grad_(True) for k in ("yin",) + PARAM_NAMES]


def block_grads(case, dtype=torch.float64, rnd=None, want_inter=False):
    """(y, the eleven gradients in GRAD_NAMES order[, intermediates]) of a case dict (yin, gy and PARAM_NAMES) in `dtype`.
    With want_inter the dict holds every forward intermediate and, under 'd <name>', its gradient; and the terms of gyin."""
    body = case["wdw3"].dim() == 5
    leaves = _leaves(case, dtype)
    inter = ([] if body else {}) if want_inter else None
    y = (nas_body_ref if body else nas_block_ref)(*leaves, rnd=rnd, inter=inter)
    y.backward(case["gy"].to(dtype))
    grads = [t.grad for t in leaves]
    if rnd is not None:
        grads[0] = rnd(grads[0])                                         # gyin is stored in the activation type
    if not want_inter:
        return y.detach(), grads
    out = []
    for b, d in enumerate(inter if body else [inter]):
        o = {}
        for name, t in d.items():
            o[name] = t.detach()
            if t.grad is not None:
                o["d " + name] = t.grad
        out.append(o)
    return y.detach(), grads, (out if body else out[0])


def emulate(case, mode):
    """the formula in the kernels' precision on the CPU: 'fp32' -- float32 throughout; 'bf16' -- float32 with a rounding
    to bf16 at V, y, GZ and gyin, the tensors include/sr_hotpath.h stores in bf16, and at the scaled backward weights
    (_BranchTailRounded)"""
    return block_grads(case, torch.float32, bf16_round if mode == "bf16" else None)


# ---- exact cases ---------------------------------------------------------------------------------------------------------
def _masks(kind, f, g):
    one = torch.ones(f)
    if kind == "all":
        return one.clone(), one.clone()
    if kind == "random":
        mg, ms = (torch.randint(0, 2, (f,), generator=g).float() for _ in range(2))
        mg[f - 1], ms[f - 1], mg[0], ms[1] = 1.0, 1.0, 1.0, 1.0          # never empty, the last channel is live
        return mg, ms
    if kind == "ms0":
        return one.clone(), torch.zeros(f)
    if kind == "mg0":
        return torch.zeros(f), one.clone()
    if kind == "live-first":                                            # one live branch channel, every skip channel
        ms = torch.zeros(f)
        ms[0] = 1.0
        return one.clone(), ms
    if kind == "live-last":                                             # one live channel in all: the last, next to the padding
        m = torch.zeros(f)
        m[f - 1] = 1.0
        return m.clone(), m.clone()
    raise KeyError(kind)


MASK_KINDS = ("all", "random", "ms0", "mg0", "live-first", "live-last")


def _sparse_stencil(f, ks, nt, values, g, shift):
    """(f, 1, ks, ks): nt nonzero taps per channel, placed so that the channels together cover every tap"""
    w = torch.zeros(f, ks * ks)
    perm = torch.randperm(ks * ks, generator=g)
    assert f * nt >= ks * ks
    for c in range(f):
        for j in range(nt):
            i = c * nt + j
            w[c, perm[(i + shift) % (ks * ks)]] = values[int(torch.randint(0, len(values), (1,), generator=g))]
    return w.view(f, 1, ks, ks)


def _sparse_pointwise(f, offsets, values, g):
    """(f, f, 1, 1): row co reads the input channels co + offsets (mod f); supports differ from row to row"""
    w = torch.zeros(f, f)
    for co in range(f):
        for o in offsets:
            w[co, (co + o) % f] = values[int(torch.randint(0, len(values), (1,), generator=g))]
    return w.view(f, f, 1, 1)


def _odd_multiples(shape, unit, g):
    return (2 * torch.randint(-2, 2, shape, generator=g).float() + 1) * unit      # -3, -1, 1, 3 units


def _exact_block_params(f, g, first, chain):
    """weights in {-1, 0, 1, 2} (sparse), depthwise biases on odd multiples of 1/2.  The depthwise outputs then lie on the 1/2
    lattice off zero, so a pointwise pre-activation stays off zero with a bias on odd multiples of 1/4.  chain: blocks that
    feed one another have to stay on ONE lattice -- even pointwise weights (and even depthwise weights after the first block)
    with every bias on odd multiples of 1/2 keep all pre-activations on odd multiples of 1/2."""
    dwv = (-1.0, 1.0, 1.0, -1.0, 2.0) if first else (-2.0, 2.0)
    pwv = (-2.0, 2.0) if chain else (-1.0, 1.0, 2.0)
    wdw = [_sparse_stencil(f, ks, nt, dwv, g, shift) for ks, nt, shift in ((3, 2, 0), (5, 2, 3), (7, 3, 11))]
    bdw = _odd_multiples((3, f), 0.5, g)
    wpw = torch.stack([_sparse_pointwise(f, offs, pwv, g) for offs in ((1, 7), (2, 11), (3, 5))])
    bpw = _odd_multiples((3, f), 0.5 if chain else 0.25, g)
    return wdw, bdw, wpw, bpw


@functools.lru_cache(maxsize=None)
def exact_case(f, n, h, w, masks="all", p=(1.0, 0.0, 0.0), beta=(0.0, 1.0), seed=0, gy_density=1.0):
    """One block on dyadic data; checked by check_exact() before it is returned (raises if a condition fails).
    Cached: the tensors are shared and must not be written to."""
    g = torch.Generator().manual_seed(77000 + 1000 * seed + 13 * f + 7 * h + w + 3 * n)
    wdw, bdw, wpw, bpw = _exact_block_params(f, g, True, False)
    mg, ms = _masks(masks, f, g)
    yin = torch.randint(-1, 2, (n, h, w, f), generator=g).float()
    gy = torch.randint(-2, 3, (n, h, w, f), generator=g).float()
    if gy_density < 1.0:
        gy = gy * (torch.rand(n, h, w, f, generator=g) < gy_density).float()
    case = dict(yin=yin, gy=gy, wdw3=wdw[0], wdw5=wdw[1], wdw7=wdw[2], bdw=bdw, wpw=wpw, bpw=bpw, mg=mg, ms=ms,
                p=torch.tensor(p), beta=torch.tensor(beta))
    case["ref"] = check_exact(case)
    return case


@functools.lru_cache(maxsize=None)
def exact_body_case(f, n, h, w, nb=3, seed=0):
    """nb blocks in a row on dyadic data.  Every block after the first reads what the one before wrote, so the lattice must not
    get finer from block to block: one-hot p (a different branch in each block), even pointwise weights and, after the first
    block, even depthwise weights keep every pre-activation on odd multiples of 1/2."""
    g = torch.Generator().manual_seed(99000 + 1000 * seed + 13 * f + 7 * h + w + 3 * n)
    blocks = [_exact_block_params(f, g, b == 0, True) for b in range(nb)]
    MS = torch.stack([_masks("random", f, g)[1] * (torch.arange(f) % 3 != b % 3).float() for b in range(nb)])
    MS[:, f - 1] = 1.0
    P = torch.stack([torch.eye(3)[(2 * b) % 3] for b in range(nb)])
    case = dict(yin=torch.randint(-1, 2, (n, h, w, f), generator=g).float(),
                gy=torch.randint(-2, 3, (n, h, w, f), generator=g).float(),
                wdw3=torch.stack([b[0][0] for b in blocks]), wdw5=torch.stack([b[0][1] for b in blocks]),
                wdw7=torch.stack([b[0][2] for b in blocks]), bdw=torch.stack([b[1] for b in blocks]),
                wpw=torch.stack([b[2] for b in blocks]), bpw=torch.stack([b[3] for b in blocks]),
                mg=torch.ones(f), ms=MS, p=P, beta=torch.tensor([[0.0, 1.0]] * nb))
    case["ref"] = check_exact(case)
    return case


def _quantum(t):
    """largest power of two 2^-e (0 <= e <= 16) that every entry of t is a multiple of: ONE quantum for the whole tensor, at most 1
    (also for zeros) -- coarser tensors are held to the finer lattice, so this is not parity_kit.lowbit(t).min()"""
    for e in range(17):
        s = t * float(2 ** e)
        if torch.equal(s, s.round()):
            return 2.0 ** -e
    raise ValueError("not dyadic within 2^-16")


def _check_block(tag, c, d, gy_in):
    """the conditions of one block: c its parameters (float64), d its intermediates and their gradients, gy_in the gradient at
    its output"""
    f = c["mg"].numel()
    cv = lambda t: t.view(1, f, 1, 1)
    # (1) every intermediate the kernels form is its own bf16 rounding
    terms = dict(d)
    terms["gyin skip term"] = (c["beta"][0] + c["beta"][1]) * cv(c["mg"]) * gy_in
    terms["gyin branch term"] = cv(c["mg"] * c["ms"]) * d["d x1"]
    for k in range(3):
        terms[f"scaled backward weight {k}"] = c["wpw"][k] * c["p"][k] * c["beta"][1] * c["ms"].view(f, 1, 1, 1)
    for name, t in terms.items():
        need_bf16(tag + name, t)
    # (2) no ReLU argument is exactly 0
    for k in range(3):
        for nm in (f"z{k}", f"u{k}"):
            if bool((d[nm] == 0).any()):
                fail(f"{tag}{nm} has a zero ReLU argument")
    # (3) every reduction: sum |terms| < 2^24 quanta
    x1a, gya = d["x1"].abs(), gy_in.abs()
    for k, ks in enumerate(KS):
        wd, wp = c[f"wdw{ks}"], c["wpw"][k]
        q = min(_quantum(d["x1"]), _quantum(c["bdw"][k]))
        need_sum(f"{tag}stencil {ks}", F_.conv2d(x1a, wd.abs(), c["bdw"][k].abs(), padding=ks // 2, groups=f), q)
        q = min(_quantum(d[f"v{k}"]), _quantum(c["bpw"][k]))
        need_sum(f"{tag}pointwise {ks}", F_.conv2d(d[f"v{k}"].abs(), wp.abs(), c["bpw"][k].abs()), q)
        gu, gz, v = d[f"d u{k}"], d[f"d z{k}"], d[f"v{k}"]
        m = gy_in * (d[f"u{k}"] > 0)                                    # what the pointwise backward contracts: gy 1(u > 0)
        need_sum(f"{tag}pointwise backward {ks}", F_.conv2d(m.abs(), terms[f"scaled backward weight {k}"].abs().transpose(0, 1)),
                   _quantum(terms[f"scaled backward weight {k}"]) * _quantum(m))
        need_sum(f"{tag}flipped stencil {ks}", F_.conv_transpose2d(gz.abs(), wd.abs(), padding=ks // 2, groups=f), _quantum(gz))
        need_sum(f"{tag}d wpw {ks}", torch.einsum("nohw,nihw->oi", m.abs(), v.abs()), _quantum(m) * _quantum(v))
        need_sum(f"{tag}d wpw {ks} scaled", torch.einsum("nohw,nihw->oi", gu.abs(), v.abs()), _quantum(gu) * _quantum(v))
        need_sum(f"{tag}d bpw {ks}", m.abs().sum((0, 2, 3)), _quantum(m))
        need_sum(f"{tag}d bpw {ks} scaled", gu.abs().sum((0, 2, 3)), _quantum(gu))
        need_sum(f"{tag}d wdw {ks}", gz.abs().sum((0, 2, 3)) * x1a.max(), _quantum(gz) * _quantum(d["x1"]))   # (upper bound)
        need_sum(f"{tag}d bdw {ks}", gz.abs().sum((0, 2, 3)), _quantum(gz))
        r = gya * torch.relu(d[f"u{k}"])                                 # r_k[c] = sum gy relu(u_k); q_k = sum_c ms[c] r_k[c]
        need_sum(f"{tag}r {ks}", r.sum(), _quantum(gy_in) * _quantum(d[f"u{k}"]) * _quantum(c["p"]))
    gbr = d["d x1"]                                                     # g_br = sum_k dw_k^T(GZ_k)
    gx = gy_in * (c["beta"][0] + c["beta"][1]) + cv(c["ms"]) * gbr
    need_sum(f"{tag}sA", (gbr * d["xg"]).abs().sum(), _quantum(gbr) * _quantum(d["xg"]))
    need_sum(f"{tag}sB", (gx * d["xg"]).abs().sum(), _quantum(gx) * _quantum(d["xg"]))
    ta = sum(c["p"][k] * (gya * torch.relu(d[f"u{k}"])).sum() for k in range(3))
    need_sum(f"{tag}g_beta", (gya * d["xg"].abs()).sum() + ta, _quantum(gy_in) * _quantum(d["xg"]) * _quantum(d["s"]))
    # (4) the weights: each of the 83 taps nonzero in some channel; every pointwise row reads >= 2 input channels, no two rows equal
    for ks in KS:
        if not bool((c[f"wdw{ks}"] != 0).any(0).all()):
            fail(f"{tag}a tap of the {ks}x{ks} is zero in every channel")
    for k in range(3):
        w2 = c["wpw"][k].view(f, f)
        if int((w2 != 0).sum(1).min()) < 2 or torch.unique(w2, dim=0).shape[0] != f:
            fail(f"{tag}pointwise rows of branch {k} are not distinct two-channel rows")


def check_exact(case):
    """Verify the exactness conditions of an exact case on the float64 reference alone; raises ValueError if one fails.
    Returns (y, gradients) of the float64 reference."""
    y, grads, inter = block_grads(case, torch.float64, None, want_inter=True)
    body = isinstance(inter, list)
    c64 = {k: v.double() for k, v in case.items() if k != "ref"}
    if not body:
        _check_block("", c64, inter, c64["gy"].permute(0, 3, 1, 2))
    else:
        for b, d in enumerate(inter):
            cb = {k: (c64[k][b] if k != "mg" else c64[k]) for k in PARAM_NAMES}
            _check_block(f"block {b}: ", cb, d, d["d y"])
    for name, t in zip(("y",) + GRAD_NAMES, [y] + grads):
        need_fp32(name, t)
    for name, t in (("y", y), ("gyin", grads[0])):
        need_bf16(name, t)
    return y, grads


# the cases of the parity tests (tile 12 x 24, halo 3, half-row unit 12 columns, pixels in pairs): (n, h, w)
P_MIX = (0.5, 0.25, 0.25)
GEOMETRIES = (
    (1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 3, 3), (1, 6, 6),              # inside the 7 x 7 window
    (1, 12, 24), (1, 11, 23), (1, 13, 25),                              # exactly one tile, one under, one-pixel sliver tiles
    (1, 12, 11), (1, 12, 12), (1, 12, 13),                              # around the half-row unit, odd and even width
    (2, 25, 49),                                                        # 3 x 3 tiles: an interior tile whose halo is all neighbours
    (3, 13, 25),                                                        # the batch stride
)
CORNER_GEOMETRIES = ((1, 13, 25), (1, 6, 6))
CORNERS = tuple((m, P_MIX, (0.0, 1.0)) for m in MASK_KINDS) + (         # (masks, p, beta)
    ("random", (1.0, 0.0, 0.0), (0.0, 1.0)), ("random", (0.0, 1.0, 0.0), (0.0, 1.0)), ("random", (0.0, 0.0, 1.0), (0.0, 1.0)),
    ("random", P_MIX, (1.0, 0.0)), ("all", (0.0, 0.0, 1.0), (1.0, 0.0)))
TILE_LOOP_GEOMETRY = (3, 13, 25)                                         # 12 tiles
MANY_TILES = dict(n=65, h=13, w=25, masks="all", p=P_MIX, gy_density=0.25)   # 260 tiles > 256 workgroups; sparse gy: g_p / g_beta sum
BODY_FUSED, BODY_SEPARATE = (2, 13, 25), (1, 25, 49)                     # 8 and 9 tiles
ROUNDED_GEOMETRIES = ((1, 13, 25), (2, 25, 49), (1, 6, 6))


# ---- rounded cases -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounded_case(f, n, h, w, mode, seed=0):
    """random normal data, random 0/1 masks, p = softmax of a random alpha, open gate.  mode 'bf16': yin, gy, the stencil weights and
    the pointwise weights are rounded to bf16 (the lane = channel kernel rounds the stencil weights itself, so the reference
    reads the same values).  Cached: shared, not to be written to."""
    g = torch.Generator().manual_seed(55000 + 1000 * seed + 13 * f + 7 * h + w + 3 * n)
    rn = lambda *s: torch.randn(*s, generator=g)
    mg, ms = _masks("random", f, g)
    case = dict(yin=rn(n, h, w, f), gy=rn(n, h, w, f), wdw3=rn(f, 1, 3, 3) / 3, wdw5=rn(f, 1, 5, 5) / 5, wdw7=rn(f, 1, 7, 7) / 7,
                bdw=0.2 * rn(3, f), wpw=rn(3, f, f, 1, 1) / f ** 0.5, bpw=0.2 * rn(3, f), mg=mg, ms=ms,
                p=torch.softmax(rn(3), 0), beta=torch.tensor([0.0, 1.0]))
    if mode == "bf16":
        for k in ("yin", "gy", "wdw3", "wdw5", "wdw7", "wpw"):
            case[k] = bf16_round(case[k])
    return case


@functools.lru_cache(maxsize=None)
def rounded_reference(f, n, h, w, mode, seed=0):
    """(case, float64 reference (y, grads), yardstick per tensor): the yardstick is the distance of the CPU emulation of the
    kernels' precision from the float64 reference, in the tests' metric -- computed from the reference alone"""
    case = rounded_case(f, n, h, w, mode, seed)
    y, grads = block_grads(case)
    ye, ge = emulate(case, mode)
    yard = [rel_max(a, b) for a, b in zip([ye] + ge, [y] + grads)]
    return case, (y, grads), yard
