"""Float64 reference of the parameter-plumbing kernels and the generators of their test cases: wn_src_kernel, pack_all_kernel,
unpack_all_kernel, wn_bwd_kernel (csrc/wdsr_prep.h), nas_mask_grads_kernel (csrc/nas_block.h), loss_sum_kernel and the loss fold of
adam_step_kernel (csrc/train_step.h), restated from their contracts in include/sr_hotpath.h.  Plain torch on the CPU, nothing of the
package.  Everything is table-driven like the kernels:

  chan_tab  int[n_chan][4] = {v_off, g_off, K, dst_off}     w = g v / |v| of flat[v_off .. v_off + K) into src[dst_off ..]
  bias_tab  int[n_bias][3] = {src_a, src_b | -1, dst}        src[dst] = flat[src_a] + flat[src_b] + bias_const[i]
  pack seg  {idx, src_off, src_stride, n, reps, as_float}    out[rep n + i] = src[src_off + rep src_stride + idx[i]], fp32 or hot dtype
  unpack seg {partial, sidx, dst, dst_off, dst_stride, slab, wgs, n, reps}
                                                             dsrc[dst_off + rep dst_stride + dst[i]] = sum_w partial[rep][w][sidx[i]]

EXACT cases (tests/parity_kit.py): a correct kernel returns them bit for bit.
  sums          dyadic data, sum |terms| < 2^24 quanta (need_sum), so fp32 addition is exact in any order; the slabs of one element
                differ pairwise, so a slab dropped, counted twice or taken for another one changes the sum
  weight norm   integer rows with an integer Euclidean norm: Kronecker products of (1,2,2), (2,3,6), (1,4,8) (norms 3, 7, 9), signs
                and positions permuted, padded with zeros, a nonzero in every 64-stride of a lane; g = n d with a dyadic d, so
                g / n = d and w = d v.  Backward: dw = c v + perp, perp built pairwise as t (b, -a) on the nonzeros of v and free on
                its zeros, so v.dw = c n^2, dot / ss = c, dv = d perp, dg = c n -- exact with or without FMA contraction, also with
                the whole row scaled by 2^+-30
  bf16 packing  values that reach the pack through bias rows (src_b = -1, bias_const = 0) lie exactly half way between two bf16
                neighbours, with both parities of the kept bit; expected: src.bfloat16()
ROUNDED cases are weight norm on standard-normal data; the yardstick is the same restatement evaluated in fp32.
"""
import functools
import math

import torch

from tests import parity_kit as K

_seed = functools.partial(K.seed, 97531, 13)
NAN = float("nan")
BF = torch.bfloat16
TRIPLES = ((1, 2, 2), (2, 3, 6), (1, 4, 8))                  # Euclidean norms 3, 7, 9
UNPACK_Q, UNPACK_JMAX = 16, 4                                # csrc/wdsr_prep.h: slab groups per block, elements per thread
JUNK = 99.0                                                  # flat / dsrc entries no table names (inputs nobody may read or change)


def unpack_j(wgs):
    return 1 if wgs > 4 * UNPACK_Q else UNPACK_JMAX


# ---- the six operations ------------------------------------------------------------------------------------------------------
def _sum(x, order=None):
    """sum of a vector; order (lanes, reverse): `lanes` strided partial sums folded by halves, elementwise adds in x's dtype only"""
    if order is None:
        return x.sum()
    lanes, rev = order
    x = x.flip(0) if rev else x
    x = torch.cat([x, x.new_zeros((-x.numel()) % lanes)]).view(-1, lanes)
    acc = x[0].clone()
    for row in x[1:]:
        acc = acc + row
    while lanes > 1:
        lanes //= 2
        acc = acc[:lanes] + acc[lanes:2 * lanes]
    return acc[0]


def wn_forward(flat, src, chan_tab, bias_tab, bias_const, dtype=torch.float64, order=None, defect=None):
    """wn_src_kernel: `src` with the table rows written (everything else as it was)"""
    f, out = flat.to(dtype), src.to(dtype).clone()
    for v_off, g_off, k, dst in chan_tab.tolist():
        v = f[v_off:v_off + k]
        out[dst:dst + k] = v * (f[g_off] / _sum(v * v, order).sqrt())
    if len(bias_tab):
        a, b, d = bias_tab.long().unbind(1)
        val = f[a]
        if defect != "src_b":
            val = val + torch.where(b >= 0, f[b.clamp_min(0)], torch.zeros_like(val))
        if defect != "bias_const":
            val = val + bias_const.to(dtype)
        out[d] = val
    return out


def wn_backward(flat, dsrc, gflat, chan_tab, bias_tab, dtype=torch.float64, order=None, defect=None):
    """wn_bwd_kernel: dv = (g / n) (dw - v (v.dw) / n^2), dg = (v.dw) / n, biases copied through to src_a and src_b"""
    f, d, out = flat.to(dtype), dsrc.to(dtype), gflat.to(dtype).clone()
    for v_off, g_off, k, dst in chan_tab.tolist():
        v, dw = f[v_off:v_off + k], d[dst:dst + k]
        ss, dot = _sum(v * v, order), _sum(v * dw, order)
        n = ss.sqrt()
        out[v_off:v_off + k] = (f[g_off] / n) * (dw - v * (dot / ss))
        out[g_off] = dot / ss if defect == "dot_ss" else dot / n
    if len(bias_tab):
        a, b, dst = bias_tab.long().unbind(1)
        out[a] = d[dst]
        if defect != "src_b":
            out[b[b >= 0]] = d[dst[b >= 0]]
    return out


def bf16_truncate(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _chunk_of(reps, n, e):
    """(reps, n): the workgroup of its segment that serves element i of repetition rep"""
    per = (n + e - 1) // e
    return torch.arange(reps).view(-1, 1) * per + (torch.arange(n) // e).view(1, -1), reps * per


def pack(src, segs, hot, defect=None):
    """pack_all_kernel: per segment the (reps * n,) blob, fp32 (as_float) or `hot`; src: the fp32 source.  Elements a seeded defect
    leaves unwritten are NaN."""
    outs, shift = [], 0
    for k, s in enumerate(segs):
        idx = s["idx"].long()
        rows = torch.stack([src[s["src_off"] + r * s["src_stride"] + idx] for r in range(s["reps"])]).float()
        dt = torch.float32 if s["as_float"] else hot
        o = bf16_truncate(rows) if (defect == "truncate" and dt == BF) else rows.to(dt)
        chunk, nblk = _chunk_of(s["reps"], s["n"], 256)
        if defect == "last_element":
            o[-1, -1] = NAN
        if defect == "block0" and k:
            o[chunk < shift] = NAN
        shift = nblk
        outs.append(o.reshape(-1))
    return outs


def unpack(dsrc, segs, dtype=torch.float64, defect=None):
    """unpack_all_kernel: `dsrc` with every segment's slab sums scattered into it"""
    out, shift = dsrc.to(dtype).clone(), 0
    for k, s in enumerate(segs):
        p = s["partial"].to(dtype).view(s["reps"], s["wgs"], s["slab"])
        tot = p.sum(1)
        if defect == "drop_last_slab":
            tot = tot - p[:, -1]
        if defect == "slab0_twice":
            tot = tot + p[:, 0]
        val = tot[:, s["sidx"].long()]
        chunk, nblk = _chunk_of(s["reps"], s["n"], 64 * unpack_j(s["wgs"]))
        written = torch.ones_like(chunk, dtype=torch.bool)
        if defect == "last_element":
            written[-1, -1] = False
        if defect == "block0" and k:
            written &= chunk >= shift
        shift = nblk
        for r in range(s["reps"]):
            pos = s["dst_off"] + r * s["dst_stride"] + s["dst"].long()
            out[pos[written[r]]] = val[r][written[r]]
    return out


def mask_grads(dsrc, ds, off_r, off_sxy, off_sA, off_sB, ms, p, beta, dtype=torch.float64):
    """nas_mask_grads_kernel: g_p[nb][3] | g_beta[nb][2] | g_ms[nb][F] | g_mg[F] from the sums in rows of `ds` floats"""
    nb, f = ms.shape
    d, ms, p, beta = dsrc.to(dtype)[:nb * ds].view(nb, ds), ms.to(dtype), p.to(dtype), beta.to(dtype)
    r, sxy = d[:, off_r:off_r + 3 * f].reshape(nb, 3, f), d[:, off_sxy]
    sa, sb = d[:, off_sA:off_sA + f], d[:, off_sB:off_sB + f]
    q = (r * ms.view(nb, 1, f)).sum(2)
    g_p = beta[:, 1:2] * q
    g_beta = torch.stack([sxy, sxy + (p * q).sum(1)], dim=1)
    g_ms = sa + beta[:, 1:2] * (p.view(nb, 3, 1) * r).sum(1)
    return torch.cat([g_p.reshape(-1), g_beta.reshape(-1), g_ms.reshape(-1), sb.sum(0)])


def loss_value(loss_part, loss_scale):
    """loss_sum_kernel / the fold of adam_step_kernel: the float64 product, rounded once to fp32; loss_scale: the fp32 scalar"""
    return (loss_part.double().sum() * torch.tensor(loss_scale, dtype=torch.float32).double()).float()


# ---- generators: tables ------------------------------------------------------------------------------------------------------
def _ri(g, lo, hi, shape=None):
    """random integers of [lo, hi): a tensor of `shape`, or one Python int"""
    t = torch.randint(lo, hi, shape or (1,), generator=g)
    return t if shape else int(t)


def _nonzero_int(g, lo, hi, shape):
    """integers of [-hi, -lo] and [lo, hi]"""
    return _ri(g, lo, hi + 1, shape) * (2 * _ri(g, 0, 2, shape) - 1)


def _place(g, sizes, gap=3):
    """scrambled, non-overlapping offsets of blocks of the given sizes with up to `gap` unnamed entries around them -> (offsets, total)"""
    offs, pos = [0] * len(sizes), _ri(g, 1, gap + 1)
    for i in torch.randperm(len(sizes), generator=g).tolist():
        offs[i] = pos
        pos += sizes[i] + _ri(g, 0, gap + 1)
    return offs, pos + 1


def int_norm_row(g, k):
    """(v, perp, n): an integer row of k entries with the integer norm n, a nonzero in each of its 64-strides, and an integer perp
    orthogonal to it term by term (pairs t (b, -a) on the nonzeros, free values on the zeros)"""
    m = 1
    while 3 ** (m + 1) <= k and m < 5:
        m += 1
    if m > 1 and 3 ** (m - 1) >= (k + 63) // 64 and _ri(g, 0, 2):
        m -= 1
    vec, n = torch.ones(1, dtype=torch.int64), 1
    for j in range(m):
        t = TRIPLES[_ri(g, 0, 3) if m <= 3 else 0]
        vec = torch.kron(vec, torch.tensor(t)[torch.randperm(3, generator=g)])
        n *= math.isqrt(sum(x * x for x in t))
    vec = vec * (2 * _ri(g, 0, 2, (vec.numel(),)) - 1)
    chunks = (k + 63) // 64
    first = [64 * c + _ri(g, 0, min(64, k - 64 * c)) for c in range(chunks)]
    rest = [i for i in torch.randperm(k, generator=g).tolist() if i not in first]
    pos = torch.tensor((first + rest)[:vec.numel()])
    v, perp = torch.zeros(k, dtype=torch.int64), _nonzero_int(g, 1, 8, (k,))
    v[pos] = vec
    perp[pos] = 0
    for a, b in zip(pos[0::2].tolist(), pos[1::2].tolist()):
        t = int(_nonzero_int(g, 1, 3, (1,)))
        perp[a], perp[b] = t * v[b], -t * v[a]
    return v.double(), perp.double(), n


def tie_value(g, parity):
    """a value exactly half way between two bf16 neighbours whose kept (eighth) mantissa bit has the given parity"""
    m9 = 256 + 4 * _ri(g, 0, 64) + 2 * parity + 1
    return float((2 * _ri(g, 0, 2) - 1) * m9) * 2.0 ** _ri(g, -11, -4)


def wn_table(key, ks, n_chan, n_bias, exact, scale_exp=0, reps=1, src_off=0):
    """One weight-norm table with its data.  Channel c has K = ks[c % len(ks)].  The source is `reps` rows of `stride` floats from
    src_off on; block j of the table (a channel's row or one bias) lives in row j % reps, the same places of the other rows hold
    preset inputs (like the mask columns sr_nas_scalars writes), the rest is unnamed.  Returns a dict: flat, chan_tab, bias_tab,
    bias_const, src0 (the source before the call: NaN where unnamed), named (bool: what the kernel writes), covered (places of a row
    a gather may read), dw (the source-shaped upstream gradient of the backward: NaN where unnamed), gnamed (bool over flat: what the
    backward writes)."""
    g = torch.Generator().manual_seed(_seed(1, *key, n_chan, n_bias, int(exact), scale_exp, reps, src_off))
    kk = [ks[c % len(ks)] for c in range(n_chan)]
    has_b = [i % 3 == 1 for i in range(n_bias)]
    fsizes = [k for k in kk] + [1] * n_chan + [1] * n_bias + [1] * sum(has_b)
    foff, n_flat = _place(g, fsizes)
    roff, row = _place(g, kk + [1] * n_bias)
    stride = row + 5
    flat = torch.full((n_flat,), JUNK, dtype=torch.float64)
    size = src_off + reps * stride
    src0, dw = torch.full((size,), NAN, dtype=torch.float64), torch.full((size,), NAN, dtype=torch.float64)
    named, covered = torch.zeros(size, dtype=torch.bool), torch.zeros(row, dtype=torch.bool)
    gnamed = torch.zeros(n_flat, dtype=torch.bool)
    s = 2.0 ** scale_exp
    chan_tab, bias_tab, bias_const = [], [], []
    for j, (rel, n_el) in enumerate(zip(roff, kk + [1] * n_bias)):
        covered[rel:rel + n_el] = True
        for r in range(reps):
            if r != j % reps:
                src0[src_off + r * stride + rel:src_off + r * stride + rel + n_el] = _nonzero_int(g, 1, 64, (n_el,)).double() / 8
    for c, k in enumerate(kk):
        v_off, g_off, dst = foff[c], foff[n_chan + c], src_off + (c % reps) * stride + roff[c]
        if exact:
            v, perp, n = int_norm_row(g, k)
            d, cc = float(_nonzero_int(g, 1, 12, (1,))) / 4, float(_nonzero_int(g, 1, 4, (1,)))
            flat[v_off:v_off + k], flat[g_off] = v * s, n * s * d
            dw[dst:dst + k] = (cc * v + perp) * s
        else:
            flat[v_off:v_off + k] = torch.randn(k, generator=g).float().double()
            flat[g_off] = torch.randn(1, generator=g).float().double()
            dw[dst:dst + k] = torch.randn(k, generator=g).float().double()
        chan_tab.append([v_off, g_off, k, dst])
        named[dst:dst + k] = True
        gnamed[v_off:v_off + k] = True
        gnamed[g_off] = True
    nb_seen = 0
    for i in range(n_bias):
        j = n_chan + i
        a, dst = foff[2 * n_chan + i], src_off + (j % reps) * stride + roff[j]
        b = -1
        if has_b[i]:
            b = foff[2 * n_chan + n_bias + nb_seen]
            nb_seen += 1
        if exact:
            tie = i % 3 == 0
            flat[a] = tie_value(g, (i // 3) % 2) if tie else float(_nonzero_int(g, 1, 256, (1,))) / 16
            if b >= 0:
                flat[b] = float(_nonzero_int(g, 1, 256, (1,))) / 16
            bias_const.append(0.0 if tie else float(_nonzero_int(g, 1, 64, (1,))) / 32)
            dw[dst] = float(_nonzero_int(g, 1, 4096, (1,))) / 64
        else:
            flat[a] = float(torch.randn(1, generator=g).float())
            if b >= 0:
                flat[b] = float(torch.randn(1, generator=g).float())
            bias_const.append(float(torch.randn(1, generator=g).float()) if i % 2 else 0.0)
            dw[dst] = float(torch.randn(1, generator=g).float())
        bias_tab.append([a, b, dst])
        named[dst] = True
        gnamed[a] = True
        if b >= 0:
            gnamed[b] = True
    return dict(flat=flat, chan_tab=torch.tensor(chan_tab, dtype=torch.int32).view(-1, 4),
                bias_tab=torch.tensor(bias_tab, dtype=torch.int32).view(-1, 3), bias_const=torch.tensor(bias_const, dtype=torch.float64),
                src0=src0, named=named, covered=covered.nonzero().view(-1), dw=dw, gnamed=gnamed, row=row, stride=stride,
                src_off=src_off, reps=reps, exact=exact, scale_exp=scale_exp)


def _lattice(name, terms):
    """need_sum over the last dimension of `terms`, on the lattice of its finest term"""
    return K.need_sum(name, terms.abs().sum(-1), K.lowbit(terms).amin(-1))


def check_table(t):
    """the conditions of an exact weight-norm table (forward and backward), raises ValueError"""
    f = t["flat"]
    K.need_fp32("flat", f)
    K.need_fp32("dw", t["dw"][t["named"]])
    K.need_fp32("bias_const", t["bias_const"])
    for v_off, g_off, k, dst in t["chan_tab"].tolist():
        v, dw, g = f[v_off:v_off + k], t["dw"][dst:dst + k], f[g_off]
        q = K.lowbit(v).min()
        ss, dot = (v * v).sum(), (v * dw).sum()
        _lattice("ss", v * v)
        _lattice("dot", v * dw)
        n = ss.sqrt()
        if n * n != ss or n / q != torch.floor(n / q) or n == 0:
            K.fail(f"row at {v_off}: the norm {float(n)} is no integer of the row's lattice")
        d, c = g / n, dot / ss
        if d * n != g or abs(float(d)) > 64 or K.lowbit(d.view(1)).item() < 2.0 ** -4 or d == 0:
            K.fail(f"row at {v_off}: g / n = {float(d)} is no small dyadic number")
        if c != torch.floor(c) or c * ss != dot or c == 0 or dot != c * n * n:
            K.fail(f"row at {v_off}: dot / ss = {float(c)} is no integer")
        perp = dw - c * v
        if float((perp * v).abs().sum()) != 0.0 and float((perp * v).sum()) != 0.0:
            K.fail(f"row at {v_off}: perp is not orthogonal to v")
        if not torch.equal((g / n) * (dw - v * (dot / ss)), d * perp) or dot / n != c * n:
            K.fail(f"row at {v_off}: dv / dg identities")
        K.need_fp32("w", d * v)
        K.need_fp32("dv", d * perp)
        K.need_fp32("dg", (c * n).view(1))
        K.need_half_nonzero("dv", d * perp)
        for c0 in range(0, k, 64):
            if k > 64 and not bool((v[c0:c0 + 64] != 0).any()):
                K.fail(f"row at {v_off}: no nonzero in the 64-stride at {c0}")
    if len(t["bias_tab"]):
        a, b, _ = t["bias_tab"].long().unbind(1)
        terms = torch.stack([f[a], torch.where(b >= 0, f[b.clamp_min(0)], torch.zeros_like(f[a])), t["bias_const"]], dim=1)
        _lattice("bias rows", terms)
        K.need_half_nonzero("bias rows", terms.sum(1))
        ties = K.bf16_ties(terms.sum(1)) & (b < 0) & (t["bias_const"] == 0)
        if len(a) >= 4:
            kept = (torch.frexp(terms.sum(1))[0].abs() * 256).floor() % 2
            if not (bool((ties & (kept == 0)).any()) and bool((ties & (kept == 1)).any())):
                K.fail("bias rows: bf16 ties of both parities of the kept bit are missing")
    # fp32 on the CPU in two summation orders == float64, bit for bit
    src64 = wn_forward(f, t["src0"], t["chan_tab"], t["bias_tab"], t["bias_const"])
    g0 = torch.full_like(f, NAN)
    g64 = wn_backward(f, t["dw"], g0, t["chan_tab"], t["bias_tab"])
    for order in ((64, False), (16, True)):
        s32 = wn_forward(f, t["src0"], t["chan_tab"], t["bias_tab"], t["bias_const"], torch.float32, order)
        g32 = wn_backward(f, t["dw"], g0, t["chan_tab"], t["bias_tab"], torch.float32, order)
        if not (torch.equal(s32[t["named"]].double(), src64[t["named"]]) and torch.equal(g32[t["gnamed"]].double(), g64[t["gnamed"]])):
            K.fail(f"fp32 evaluation in order {order} differs from float64")
    K.need_half_nonzero("gflat", g64[t["gnamed"]])


# the weight-norm tables of the exact cases: (ks, n_chan, n_bias, scale_exp); K, n_chan and n_bias at their edges
TABLES = (((9,), 1, 0, 0), ((25, 27), 3, 1, 0), ((49, 63), 4, 255, 0), ((64, 65), 5, 256, 0), ((216, 288), 9, 257, 0),
          ((27, 65, 216), 5, 4, 30), ((9, 64, 288), 3, 7, -30))
# pack segments per case: (n, reps, as_float); reps 3 reads three source rows src_stride apart
PACK_SEGS = (((1, 1, 1),), ((255, 3, 0), (256, 1, 1)), ((257, 1, 0), (513, 3, 1), (1, 3, 0)),
             ((513, 1, 0), (255, 1, 0), (256, 3, 1), (257, 3, 0)), ((256, 3, 0), (1, 1, 1), (513, 1, 0), (255, 3, 1)),
             ((257, 3, 0), (255, 1, 1)), ((513, 3, 0), (1, 1, 0), (256, 1, 1)))
PACK_CASES = tuple(range(len(TABLES)))


@functools.lru_cache(maxsize=None)
def pack_case(i, exact=True):
    """table i with its gathers: dict(table, segs); a segment is dict(idx, src_off, src_stride, n, reps, as_float)"""
    ks, n_chan, n_bias, e = TABLES[i]
    reps = max(s[1] for s in PACK_SEGS[i])
    t = wn_table((2, i), ks, n_chan, n_bias, exact, e, reps, src_off=0 if i % 2 == 0 else 7)
    g = torch.Generator().manual_seed(_seed(3, i, int(exact)))
    bias_rel = t["bias_tab"][:, 2].long() - t["src_off"] - ((n_chan + torch.arange(n_bias)) % reps) * t["stride"]
    segs = []
    for n, r, as_float in PACK_SEGS[i]:
        idx = t["covered"][torch.randint(0, len(t["covered"]), (n,), generator=g)]
        m = min(n, n_bias)
        idx[:m] = bias_rel[torch.randperm(n_bias, generator=g)[:m]]          # the bias rows (the bf16 ties among them) first
        segs.append(dict(idx=idx.int(), src_off=t["src_off"], src_stride=t["stride"], n=n, reps=r, as_float=as_float))
    return dict(table=t, segs=segs)


def pack_expected(case, hot, defect=None):
    """(src, blobs): the float64 source after wn_src_kernel and what pack_all_kernel makes of its fp32 rounding"""
    t = case["table"]
    src = wn_forward(t["flat"], t["src0"], t["chan_tab"], t["bias_tab"], t["bias_const"],
                     defect=defect if defect in ("src_b", "bias_const") else None)
    return src, pack(src.float(), case["segs"], hot, defect)


def check_pack(case):
    check_table(case["table"])
    src, _ = pack_expected(case, BF)
    for s in case["segs"]:
        got = torch.stack([src[s["src_off"] + r * s["src_stride"] + s["idx"].long()] for r in range(s["reps"])])
        if bool(got.isnan().any()):
            K.fail("a gather reads an unnamed source entry")
        K.need_fp32("gathered", got)


# ---- generators: slabs -------------------------------------------------------------------------------------------------------
# unpack segments per case: (wgs, n, reps, dst_stride_zero, chained); every wgs of both bodies, every n, J = 1 and J = 4 mixed
UNPACK_SEGS = (((1, 1, 1, 1, 0),), ((15, 63, 3, 0, 0), (65, 64, 1, 1, 1)), ((16, 65, 1, 0, 0), (240, 255, 3, 0, 0), (17, 256, 1, 1, 0)),
               ((49, 257, 3, 0, 0), (241, 1, 1, 0, 0), (64, 63, 1, 0, 1), (256, 64, 3, 0, 0)),
               ((257, 65, 1, 1, 0), (300, 255, 1, 0, 0), (64, 257, 1, 0, 1), (1, 256, 3, 0, 0)),
               ((17, 1, 3, 0, 0), (65, 257, 1, 0, 0)), ((64, 257, 3, 0, 0), (300, 255, 1, 1, 0), (49, 256, 3, 0, 0), (241, 65, 3, 0, 0)))
GRADS_CASES = tuple(range(len(TABLES)))
LARGEST_MIXED = 6


def distinct_slabs(g, reps, wgs, slab, quantum):
    """(reps, wgs, slab): per element, nonzero multiples of `quantum` that differ pairwise over the slabs"""
    mag = torch.argsort(torch.rand(reps, slab, 2 * wgs + 2, generator=g), dim=2)[:, :, :wgs] + 1
    sign = 2 * torch.randint(0, 2, mag.shape, generator=g) - 1
    return (mag * sign).double().transpose(1, 2).contiguous() * quantum


@functools.lru_cache(maxsize=None)
def grads_case(i, exact=True):
    """table i with its slab segments: dict(table, segs, dsrc0, dnamed).  dsrc is the table's source row (the upstream gradient the
    weight-norm backward reads; a `chained` segment writes part of it from slabs, the rest is preset) followed by one region per
    segment; dsrc0 holds NaN wherever neither a preset input nor nothing at all belongs, dnamed marks what the slab kernel writes."""
    ks, n_chan, n_bias, e = TABLES[i]
    t = wn_table((4, i), ks, n_chan, n_bias, exact, e)
    g = torch.Generator().manual_seed(_seed(5, i, int(exact)))
    wn_pos = t["named"].nonzero().view(-1)
    regions, size = [], t["dw"].numel()
    for wgs, n, reps, zero, chained in UNPACK_SEGS[i]:
        span = n + 1 + n // 3
        stride = 0 if zero else span + 4
        regions.append((size + 2, span, stride))
        size += 2 + (span if zero else reps * stride)
    dsrc0 = torch.full((size,), NAN, dtype=torch.float64)
    dsrc0[:t["dw"].numel()] = t["dw"]
    dnamed = torch.zeros(size, dtype=torch.bool)
    segs = []
    for (wgs, n, reps, zero, chained), (off, span, stride) in zip(UNPACK_SEGS[i], regions):
        slab = n + 3 + n // 4
        sidx = torch.randperm(slab, generator=g)[:n]
        quantum = 2.0 ** -_ri(g, 0, 5)
        part = distinct_slabs(g, reps, wgs, slab, quantum)
        if chained and exact and e == 0 and len(wn_pos) >= n:                      # slabs whose sum is the dw the weight-norm backward reads
            assert reps == 1
            dst, off = wn_pos[torch.randperm(len(wn_pos), generator=g)[:n]], 0
            target = t["dw"][dst]
            assert wgs > 2
            for j, col in enumerate(sidx.tolist()):                       # the last slab closes the sum; slab 0 moves out of the
                step = 2 * wgs + 3                                        # others' range until the last one equals none of them
                while True:
                    last = target[j] - part[0, :-1, col].sum()
                    if last != 0 and not bool((part[0, :-1, col] == last).any()):
                        break
                    part[0, 0, col], step = step * quantum, step + 1
                part[0, -1, col] = last
            dsrc0[dst] = NAN
        else:
            dst = torch.randperm(span, generator=g)[:n]
        for r in range(reps):
            dnamed[off + r * stride + dst] = True
        segs.append(dict(partial=part.reshape(-1), sidx=sidx.int(), dst=dst.int(), dst_off=off, dst_stride=stride, slab=slab, wgs=wgs,
                         n=n, reps=reps))
    return dict(table=t, segs=segs, dsrc0=dsrc0, dnamed=dnamed)


def grads_expected(case, defect=None):
    """(dsrc, gflat) in float64; gflat starts as NaN, so what no table row names stays NaN"""
    t = case["table"]
    dsrc = unpack(case["dsrc0"], case["segs"], defect=defect if defect in ("drop_last_slab", "slab0_twice", "last_element", "block0") else None)
    gflat = wn_backward(t["flat"], dsrc, torch.full_like(t["flat"], NAN), t["chan_tab"], t["bias_tab"],
                        defect=defect if defect in ("src_b", "dot_ss") else None)
    return dsrc, gflat


def check_slabs(seg):
    p = seg["partial"].view(seg["reps"], seg["wgs"], seg["slab"])[:, :, seg["sidx"].long()]
    K.need_fp32("slabs", p)
    _lattice("slab sums", p.transpose(1, 2))
    K.need_half_nonzero("slab sums", p.sum(1))
    if bool((p == 0).any()):
        K.fail("a slab value is zero: dropping it would not show")
    srt = p.sort(dim=1).values
    if seg["wgs"] > 1 and bool((srt[:, 1:] == srt[:, :-1]).any()):
        K.fail("two equal slabs of one element")
    for name in ("sidx", "dst"):
        if torch.unique(seg[name]).numel() != seg["n"]:
            K.fail(f"{name} names an entry twice")


def check_grads(case):
    check_table(case["table"])
    for s in case["segs"]:
        check_slabs(s)
    dsrc, gflat = grads_expected(case)
    if not torch.equal(dsrc[:case["table"]["dw"].numel()].nan_to_num(1e300), case["table"]["dw"].nan_to_num(1e300)):
        K.fail("a chained segment does not sum to the table's dw")
    if bool(dsrc[case["dnamed"]].isnan().any()) or bool(gflat[case["table"]["gnamed"]].isnan().any()):
        K.fail("a named entry is not written")


# ---- generators: rounded weight norm -----------------------------------------------------------------------------------------
ROUNDED_CASES = tuple(range(5))


def rounded_rows(case_pack, case_grads):
    """(label, named mask picker, float64 reference, yardstick) of the three tensors the rounded rule is applied to: the effective
    weights (and bias rows), all dv, all dg; the yardstick is the same restatement in fp32"""
    tp, tg = case_pack["table"], case_grads["table"]
    src64 = wn_forward(tp["flat"], tp["src0"], tp["chan_tab"], tp["bias_tab"], tp["bias_const"])
    src32 = wn_forward(tp["flat"], tp["src0"], tp["chan_tab"], tp["bias_tab"], tp["bias_const"], torch.float32)
    d64, g64 = grads_expected(case_grads)
    g32 = wn_backward(tg["flat"], d64, torch.full_like(tg["flat"], NAN), tg["chan_tab"], tg["bias_tab"], torch.float32)
    is_g = torch.zeros_like(tg["gnamed"])
    is_g[tg["chan_tab"][:, 1].long()] = True
    is_v = torch.zeros_like(tg["gnamed"])
    for v_off, _, k, _ in tg["chan_tab"].tolist():
        is_v[v_off:v_off + k] = True
    return dict(w=(tp["named"], src64, K.rel_max(src32[tp["named"]], src64[tp["named"]])),
                dv=(is_v, g64, K.rel_max(g32[is_v], g64[is_v])), dg=(is_g, g64, K.rel_max(g32[is_g], g64[is_g])))


# ---- generators: mask gradients and loss sums --------------------------------------------------------------------------------
MASK_CASES = ((1, 8), (3, 24), (16, 32), (342, 24), (1024, 8))


@functools.lru_cache(maxsize=None)
def mask_case(nb, f):
    """dict(dsrc (nb * ds), ds, off (r, sxy, sA, sB in a scrambled order, ds wider than they are), ms, p, beta)"""
    g = torch.Generator().manual_seed(_seed(6, nb, f))
    (off_r, off_sxy, off_sa, off_sb), ds = _place(g, [3 * f, 1, f, f])
    ds += 3
    d = torch.full((nb, ds), JUNK, dtype=torch.float64)
    d[:, off_r:off_r + 3 * f] = torch.randint(-4, 5, (nb, 3 * f), generator=g).double() / 4
    d[:, off_sxy] = _nonzero_int(g, 1, 16, (nb,)).double() / 8
    d[:, off_sa:off_sa + f] = torch.randint(-16, 17, (nb, f), generator=g).double() / 8
    d[:, off_sb:off_sb + f] = torch.randint(-16, 17, (nb, f), generator=g).double() / 8
    return dict(dsrc=d.reshape(-1), ds=ds, off=(off_r, off_sxy, off_sa, off_sb), ms=torch.randint(0, 3, (nb, f), generator=g).double(),
                p=_nonzero_int(g, 1, 3, (nb, 3)).double() / 2, beta=_nonzero_int(g, 1, 3, (nb, 2)).double() / 2)


def mask_expected(c):
    return mask_grads(c["dsrc"], c["ds"], *c["off"], c["ms"], c["p"], c["beta"])


def check_mask(c):
    nb, f = c["ms"].shape
    d = c["dsrc"].view(nb, c["ds"])
    off_r, off_sxy, off_sa, off_sb = c["off"]
    for name in ("dsrc", "ms", "p", "beta"):
        K.need_fp32(name, c[name])
    r = d[:, off_r:off_r + 3 * f].reshape(nb, 3, f)
    b2 = c["beta"][:, 1].view(nb, 1, 1)
    qt = r * c["ms"].view(nb, 1, f)                                     # terms of q_k
    _lattice("g_p", b2 * qt)
    _lattice("g_beta", torch.cat([d[:, off_sxy].view(nb, 1), (c["p"].view(nb, 3, 1) * qt).reshape(nb, -1)], dim=1))
    gms = torch.cat([(b2 * c["p"].view(nb, 3, 1) * r).transpose(1, 2), d[:, off_sa:off_sa + f].view(nb, f, 1)], dim=2)
    _lattice("g_ms", gms)
    _lattice("g_mg", d[:, off_sb:off_sb + f].t())
    out = mask_expected(c)
    K.need_fp32("out", out)
    for name, lo, hi in (("g_p", 0, 3 * nb), ("g_beta", 3 * nb, 5 * nb), ("g_ms", 5 * nb, 5 * nb + nb * f), ("g_mg", 5 * nb + nb * f, out.numel())):
        K.need_half_nonzero(name, out[lo:hi])


LOSS_SIZES = (1, 63, 64, 65, 129, 1000)
LOSS_SCALES = {"pow2": 2.0 ** -7, "third": float(torch.tensor(1.0 / 3.0, dtype=torch.float32))}


@functools.lru_cache(maxsize=None)
def loss_case(n_loss):
    """(n_loss,) distinct nonzero dyadic partial sums"""
    g = torch.Generator().manual_seed(_seed(7, n_loss))
    return distinct_slabs(g, 1, n_loss, 1, 2.0 ** -6).view(-1)


def check_loss(part):
    K.need_fp32("loss_part", part)
    _lattice("loss", part)
    if part.sum() == 0 or torch.unique(part).numel() != part.numel() or bool((part == 0).any()):
        K.fail("loss partial sums must be nonzero, differ pairwise and sum to a nonzero value")


def check_exact(case):
    """the conditions of any exact case of this module (a pack, gradient or mask case, or a vector of loss partial sums); raises
    ValueError when the case does not meet them"""
    if torch.is_tensor(case):
        return check_loss(case)
    if "dsrc0" in case:
        return check_grads(case)
    return check_pack(case) if "segs" in case else check_mask(case)
