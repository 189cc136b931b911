"""The WDSR-B residual block -- h = relu(conv1x1(x; W1, b1)), t = conv1x1(h; W2, b2), y = conv3x3(t; W3, b3, pad 1) + x -- its
backward and a chain of two blocks, written out in plain torch on EFFECTIVE weights, float64 on the CPU, plus the case generators
of the block parity tests.  Nothing of the package or of the oracle is used here: this is the outside reference that
csrc/wdsr_block.h, wdsr_fwd_rs.h, wdsr_fwd_stream.h, wdsr_bwd_rs.h, wdsr_bwd_pair_lds.h and wdsr_wgrad_rs.h are held against
(tests/test_gpu_block_ref.py).  tests/test_block_ref_host.py pins it to fixture G2, to oracle.wdsr_oracle and to shifted copies,
and checks on the CPU that every exact case satisfies its exactness conditions.

Layouts: the reference works on (n, C, h, w); the entries take NHWC (nhwc() / nchw()).  A block's parameters are a dict
w1 (E, F), w2 (L, E), w3 (F, L, 3, 3), b1 (E), b2 (L), b3 (F); block_vec() is hotpath.block_src's vector w1 | w2 | w3 | b1 | b2 |
b3 | 0 | 1.  The saved side images are tile-local, [n][tiles][288][LP] over 12 x 24 tiles (tile_image()).

A case is always a CHAIN of two blocks a -> b: x -> ya -> yb forward, dyb -> dxb -> dxa backward.  The tensors between the blocks
are stored in the hot dtype and read back, so the reference rounds them there (bf16, nearest even): block b's input is
bf16(ya) and block a's cotangent is bf16(dxb).  Every single-block entry is run on either block with exactly these tensors.

Three families of cases:
  exact     dyadic data on which every operand a matrix core or a store sees in the hot dtype is its own bf16 rounding and every
            reduction satisfies sum |terms| < 2^24 quanta, so fp32 accumulation is exact in ANY order: a kernel must return the
            float64 reference bit for bit, in fp32 and in bf16, the final y / dx being the exact value rounded once.
            check_exact() verifies the conditions on the float64 reference alone and raises ValueError if one fails; it also
            refuses a vacuous case (zeros, unused taps or channels, equal rows, symmetric taps).
  tap sets  one 3x3 weight per output channel: y - x - b3 is a shifted copy of one t channel, so a failure names the tap
  rounded   random normal data, nothing rounded beforehand; the yardstick is emulate(): the same graph in float32 with a
            rounding to bf16 wherever the bf16 kernels round

How an exact case is built (trunk_ref.py's recipe).  An INTEGER chain is drawn first: W1 two weights +-1 per row (the rows are
pairwise different pairs of input channels and together use every input channel), W2 and W3 one weight +-1 per (input channel)
resp. per (tap, input channel), dealt out over the rows (7 or 8 per row: every input channel and all nine taps are used, no two
rows are equal), x and dy in {-1, 0, 1}.  b1 is FITTED to the data: minus one of the values the channel's W1 x takes, so that
every case has pre-activations of both signs and pre-activations that are exactly 0 (the gate is 0 there, forward and backward);
block b sees the larger integers of ya and takes a high quantile, which keeps its h -- and with it t -- within 8 significant
bits.  b2 and b3 are odd integers.  Then every channel of every tensor gets its own power-of-two scale (x, ya, yb share one set
because of the residual), which turns the weights into +-2^k and makes the biases of a vector pairwise different, while every dot
product still sums terms of ONE lattice.

The conditions named need_* / is_*, the roundings, the seed recipe and the bound of the rounded cases are tests/parity_kit.py's,
shared by all parity suites and pinned by tests/test_parity_kit_host.py.
"""
import functools

import torch
import torch.nn.functional as F_

from tests.parity_kit import (RoundBackward, RoundForward, bf16_round, chan_quantum, count_ties, fail, leaf, lowbit, need_bf16, need_biases,
                              need_fp32, need_half_nonzero, need_sum, need_taps, rel_max, seed)

DIMS = {24: (24, 144, 20), 32: (32, 192, 26)}
TH, TW, NPX = 12, 24, 288                                    # the block kernels' tile; pixels per tile
A8_CHUNK = 256                                               # pixels per chunk of wdsr_wgrad_a8_kernel's stream
NAMES = ("w1", "w2", "w3", "b1", "b2", "b3")
GRADS = tuple("d" + k for k in NAMES)


def lp_of(f):
    """channels per pixel of the saved images: L real + the ones channel, padded to a multiple of 8"""
    return (DIMS[f][2] + 1 + 7) // 8 * 8


def tiles_of(h, w):
    return ((h + TH - 1) // TH) * ((w + TW - 1) // TW)


def n_tiles(n, h, w):
    return n * tiles_of(h, w)


def n_chunks(n, h, w):
    return (n_tiles(n, h, w) * NPX + A8_CHUNK - 1) // A8_CHUNK


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def block_vec(p):
    """hotpath.block_src's order: w1 | w2 | w3 | b1 | b2 | b3 | 0 | 1"""
    return torch.cat([p[k].reshape(-1) for k in NAMES] + [p["w1"].new_tensor([0.0, 1.0])])


def split_vec(v, f):
    """a gradient vector of hotpath.block_wgrad's layout -> dict(dw1 .. db3, const): const are the two constant slots (zero)"""
    _, e, l = DIMS[f]
    shapes = dict(w1=(e, f), w2=(l, e), w3=(f, l, 3, 3), b1=(e,), b2=(l,), b3=(f,))
    out, o = {}, 0
    for k in NAMES:
        n = 1
        for s in shapes[k]:
            n *= s
        out["d" + k] = v[o:o + n].reshape(shapes[k])
        o += n
    assert v.numel() == o + 2, (v.numel(), o)
    out["const"] = v[o:]
    return out


def tile_image(v, lp, ones_at=None):
    """(n, C, h, w) -> the tile-local side image (n, tiles, 288, lp): pixel (Y, X) of tile (Y // 12, X // 24), row-major tiles,
    sits at row (Y % 12) 24 + X % 24; zeros in the channels C .. lp - 1 and outside the image.  ones_at: a channel that holds 1
    inside the image (the saved t images carry the ones channel that gives db3 at channel L)."""
    n, c, h, w = v.shape
    th, tw = (h + TH - 1) // TH, (w + TW - 1) // TW
    full = v.new_zeros(n, th * TH, tw * TW, lp)
    full[:, :h, :w, :c] = v.permute(0, 2, 3, 1)
    if ones_at is not None:
        full[:, :h, :w, ones_at] = 1
    return full.view(n, th, TH, tw, TW, lp).permute(0, 1, 3, 2, 4, 5).reshape(n, th * tw, NPX, lp).contiguous()


def untile_image(img, h, w, c):
    """inverse of tile_image on the pixels inside the image: (n, tiles, 288, lp) -> (n, c, h, w)"""
    n, _, _, lp = img.shape
    th, tw = (h + TH - 1) // TH, (w + TW - 1) // TW
    full = img.view(n, th, tw, TH, TW, lp).permute(0, 1, 3, 2, 4, 5).reshape(n, th * TH, tw * TW, lp)
    return full[:, :h, :w, :c].permute(0, 3, 1, 2).contiguous()


# ---- the reference ---------------------------------------------------------------------------------------------------------
def block_forward(x, p):
    """(h, t, y) of one block: x (n, F, h, w), p the effective weights, all of one dtype"""
    h = torch.relu(F_.conv2d(x, p["w1"][:, :, None, None], p["b1"]))
    t = F_.conv2d(h, p["w2"][:, :, None, None], p["b2"])
    return h, t, F_.conv2d(t, p["w3"], p["b3"], padding=1) + x


def run_block(x, p, dy, dtype=torch.float64, rnd=None, gate=None, fold_b1=True):
    """forward and backward of one block in `dtype`, every input a leaf, gradients from autograd: dict(z, h, t, y, dt = conv3x3^T(dy),
    dpre = 1(z > 0) W2^T dt, dx, dw1 .. db3).
    rnd: None for the reference; else the rounding applied where the bf16 kernels round: x, the weights of the blob with the
    biases folded into it (b3 always; b1 when fold_b1, i.e. at 24 units -- b2 and an unfolded b1 stay fp32 accumulator initial
    values), h, t, dy, dt and dpre.  The caller rounds the stores y and dx.
    gate: a bool tensor used INSTEAD of z > 0 (the rounded cases hand the float64 reference the gate of the kernels' own z, so
    that a pre-activation next to zero whose sign rounding flips is not counted as an error of the backward kernels)."""
    rf = (lambda t: RoundForward.apply(t, rnd)) if rnd is not None else (lambda t: t)
    rb = (lambda t: RoundBackward.apply(t, rnd)) if rnd is not None else (lambda t: t)
    lx = leaf(x, dtype)
    lp = {k: leaf(p[k], dtype) for k in NAMES}
    q = {k: rf(lp[k]) if (k[0] == "w" or k == "b3" or (k == "b1" and fold_b1)) else lp[k] for k in NAMES}
    xin = rf(lx)
    z = rb(F_.conv2d(xin, q["w1"][:, :, None, None], q["b1"]))
    on = (z.detach() > 0) if gate is None else gate
    h = rf(z * on.to(dtype))
    t = rb(rf(F_.conv2d(h, q["w2"][:, :, None, None], q["b2"])))
    y = F_.conv2d(t, q["w3"], q["b3"], padding=1) + xin
    keep = dict(z=z, h=h, t=t)
    for v in keep.values():
        v.retain_grad()
    cot = dy.to(dtype)
    y.backward(rnd(cot) if rnd is not None else cot)
    out = {k: v.detach() for k, v in keep.items()}
    out.update(y=y.detach(), dt=t.grad, dpre=z.grad, dx=lx.grad)
    out.update({"d" + k: lp[k].grad for k in NAMES})
    return out


def run_pair(case, dtype=torch.float64, rnd=None, store=bf16_round, gates=None):
    """the chain a -> b of a case: dict(a=run_block(..), b=run_block(..)) with, per block, 'y_st' and 'dx_st' = the stored tensors
    (store(y), store(dx)); block b reads a's y_st and block a's cotangent is b's dx_st.  store = None: nothing is rounded in
    between (the fp32 kernels).  gates: (gate a, gate b) as in run_block."""
    st = store if store is not None else (lambda t: t)
    fold = case["F"] % 16 != 0
    ga, gb = gates if gates is not None else (None, None)
    ya_st = st(run_block(case["x"], case["pa"], torch.zeros_like(case["x"]), dtype, rnd, ga, fold)["y"])
    b = run_block(ya_st, case["pb"], case["dyb"], dtype, rnd, gb, fold)
    b["y_st"], b["dx_st"] = st(b["y"]), st(b["dx"])
    a = run_block(case["x"], case["pa"], b["dx_st"], dtype, rnd, ga, fold)
    a["y_st"], a["dx_st"] = st(a["y"]), st(a["dx"])
    assert torch.equal(a["y_st"], ya_st)
    return dict(a=a, b=b)


def dt_by_shifts(dy, w3):
    """dt = conv3x3^T(dy) as nine shifted copies added up: dt[l, Y, X] = sum_{ky, kx, f} w3[f, l, ky, kx] dy[f, Y - ky + 1, X - kx + 1]"""
    n, f, h, w = dy.shape
    pad = F_.pad(dy, (1, 1, 1, 1))
    out = dy.new_zeros(n, w3.shape[1], h, w)
    for ky in range(3):
        for kx in range(3):
            sh = pad[:, :, 2 - ky:2 - ky + h, 2 - kx:2 - kx + w]
            out += torch.einsum("fl,nfyx->nlyx", w3[:, :, ky, kx], sh)
    return out


# ---- exactness conditions -------------------------------------------------------------------------------------------------
def _need_rows(name, w):
    """every input channel (and tap) carries a weight, every row does, no two rows are equal"""
    flat = w.reshape(w.shape[0], -1)
    if torch.unique(flat, dim=0).shape[0] != flat.shape[0]:
        fail(f"{name}: two rows are equal")
    if not bool((flat != 0).any(0).all()):
        fail(f"{name}: an input channel or a tap of one carries no weight in any row")
    if not bool((flat != 0).any(1).all()):
        fail(f"{name}: a row carries no weight")


def _check_conv(tag, xin, w, b, dz, dw, db, extra=None):
    """one conv (1x1 given as (co, ci, 1, 1), or 3x3): xin its input, dz the gradient at its output; extra: a tensor added to the
    output in the same accumulator (the residual).  Forward, backward-data (returns sum |terms| and the quantum per input channel:
    the caller may add the skip term) and the weight / bias sums."""
    cv = lambda t: t.view(1, -1, 1, 1)
    pad = w.shape[-1] // 2
    qx, qw, qd = chan_quantum(xin), lowbit(w).amin((2, 3)), chan_quantum(dz)
    q_out = torch.minimum((qw * qx.view(1, -1)).amin(1), lowbit(b))
    fwd = F_.conv2d(xin.abs(), w.abs(), b.abs(), padding=pad)
    if extra is not None:
        fwd, q_out = fwd + extra.abs(), torch.minimum(q_out, chan_quantum(extra))
    need_sum(f"{tag} forward", fwd, cv(q_out))
    tw, tb = torch.nn.grad.conv2d_weight(xin.abs(), w.shape, dz.abs(), padding=pad), dz.abs().sum((0, 2, 3))
    need_sum(f"d {tag} weight", tw, qd.view(-1, 1, 1, 1) * qx.view(1, -1, 1, 1))
    need_sum(f"d {tag} bias", tb, qd)
    need_half_nonzero(f"d {tag} weight", dw.reshape(tw.shape), tw)
    need_half_nonzero(f"d {tag} bias", db, tb)
    return F_.conv_transpose2d(dz.abs(), w.abs(), padding=pad), (qw * qd.view(-1, 1)).amin(0)


def _check_block(tag, x, p, dy, r, thin=False):
    """the conditions of one block on its reference r = run_block(x, p, dy)"""
    cv = lambda t: t.view(1, -1, 1, 1)
    w1, w2, w3 = p["w1"].double(), p["w2"].double(), p["w3"].double()
    for k in NAMES:                                          # (b1 rides in the bf16 blob at 24 units, b3 always; b2 is asked the same)
        need_bf16(f"{tag} {k}", p[k])
    _need_rows(f"{tag} w1", w1)                              # (the structure of the draw first, then the operands it makes)
    _need_rows(f"{tag} w2", w2)
    if not thin:                                             # (block a of the STORE_DXB family: one 3x3 weight per output channel)
        if not bool((w3 != 0).any(0).any(0).all()):
            fail(f"{tag} w3: a tap is zero in every channel pair")
        _need_rows(f"{tag} w3", w3)
        need_taps(f"{tag} w3", w3)
    for k in ("b1", "b2", "b3"):
        need_biases(f"{tag} {k}", p[k].double())
    for name, t in (("x", x), ("dy", dy), ("h", r["h"]), ("t", r["t"]), ("dt", r["dt"]), ("dpre", r["dpre"])):
        need_bf16(f"{tag} {name}", t)
    z = r["z"]
    if not (bool((z > 0).any()) and bool((z < 0).any()) and bool((z == 0).any())):
        fail(f"{tag}: the pre-activation lacks a sign or an exact zero")
    if bool((r["h"][z == 0] != 0).any()) or bool((r["dpre"][z == 0] != 0).any()):
        fail(f"{tag}: the gate is not 0 at z == 0")
    bd1, q1 = _check_conv(f"{tag} conv1", x, w1[:, :, None, None], p["b1"].double(), r["dpre"], r["dw1"], r["db1"])
    need_sum(f"{tag} dx", bd1 + dy.abs(), cv(torch.minimum(q1, chan_quantum(dy))))
    bd2, q2 = _check_conv(f"{tag} conv2", r["h"], w2[:, :, None, None], p["b2"].double(), r["dt"], r["dw2"], r["db2"])
    need_sum(f"{tag} dh", bd2, cv(q2))
    bd3, q3 = _check_conv(f"{tag} conv3", r["t"], w3, p["b3"].double(), dy, r["dw3"], r["db3"], extra=x)
    need_sum(f"{tag} dt", bd3, cv(q3))
    for k in ("y", "dx") + GRADS:
        need_fp32(f"{tag} {k}", r[k])
    for k in ("y", "dx", "t", "dt"):
        need_half_nonzero(f"{tag} {k}", r[k])
    need_taps(f"{tag} dw3", r["dw3"], *x.shape[2:])


def check_exact(case):
    """Verify the exactness conditions of an exact case on the float64 reference alone; raises ValueError if one fails.  Returns
    the reference run_pair(case) plus 'ties': how many stored values (ya, yb, dxb, dxa before their rounding) lie exactly on a
    bf16 tie."""
    ref = run_pair(case)
    x, dyb = case["x"].double(), case["dyb"].double()
    store = case.get("store", 0)
    _check_block("block a", x, case["pa"], ref["b"]["dx_st"], ref["a"], thin=store == STORE_DXB)
    _check_block("block b", ref["a"]["y_st"], case["pb"], dyb, ref["b"])
    ref["ties_of"] = dict(ya=count_ties(ref["a"]["y"]), yb=count_ties(ref["b"]["y"]), dxb=count_ties(ref["b"]["dx"]), dxa=count_ties(ref["a"]["dx"]))
    ref["ties"] = sum(ref["ties_of"].values())
    for key, name in ((STORE_YA, "ya"), (STORE_DXB, "dxb")):
        if store == key and ref["ties_of"][name] == 0:
            fail(f"no value of {name} lies on a bf16 tie")
    return ref


# ---- exact cases ----------------------------------------------------------------------------------------------------------
_seed = functools.partial(seed, 13579, 7)


def _sign(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _tern(shape, density, g):
    t = _sign(shape, g)
    return t * (torch.rand(shape, generator=g) < density).double() if density < 1.0 else t


def _pair_rows(rows, cols, g):
    """(rows, cols): two weights +-1 per row at the columns (r % cols, r % cols + 1 + r // cols): pairwise different unordered pairs
    (rows <= cols (cols // 2 - 1)), every column used; the rows are then shuffled"""
    assert rows // cols + 1 < cols // 2
    w = torch.zeros(rows, cols, dtype=torch.float64)
    sg = _sign((rows, 2), g)
    for r in range(rows):
        c1 = r % cols
        w[r, c1], w[r, (c1 + 1 + r // cols) % cols] = sg[r, 0], sg[r, 1]
    return w[torch.randperm(rows, generator=g)]


def _dealt_rows(rows, cols, g):
    """(rows, cols): every column carries ONE weight +-1, the columns dealt out over the rows in a random order"""
    w = torch.zeros(rows, cols, dtype=torch.float64)
    perm = torch.randperm(cols, generator=g)
    w[torch.arange(cols) % rows, perm] = _sign((cols,), g)
    return w


_ODD = (1.0, -1.0, 3.0, -3.0, 5.0, -5.0, 7.0, -7.0, 9.0, -9.0, 11.0, -11.0)


def _scales_for(ints, g, lo=-4, hi=4):
    """per channel a power-of-two exponent such that ints 2^e are pairwise different (the range widens where it has to)"""
    used, out = set(), []
    for v in ints.tolist():
        e = int(torch.randint(lo, hi + 1, (1,), generator=g))
        k = 0
        while v * 2.0 ** e in used:
            k += 1
            e = (hi + (k + 1) // 2) if k % 2 else (lo - k // 2)
        used.add(v * 2.0 ** e)
        out.append(float(e))
    return 2.0 ** torch.tensor(out, dtype=torch.float64)


def _odd_for(scale, g):
    """per channel an odd integer such that the scaled values are pairwise different"""
    used, out = set(), []
    for s in scale.tolist():
        k = int(torch.randint(0, 4, (1,), generator=g))
        while _ODD[k] * s in used:
            k += 1
        used.add(_ODD[k] * s)
        out.append(_ODD[k])
    return torch.tensor(out, dtype=torch.float64)


STORE_YA, STORE_DXB = 1, 2                                   # exact_case's `store`: the family whose ya resp. dxb is really rounded


def _thin_w3(f, l, g):
    """(F, L, 3, 3) with ONE weight +-1 per output channel f, at t channel f mod L and a random tap: dt[l] is then a single term
    w dy[f] for every l >= F - L (one output channel reads it), and that product of two bf16 values is a bf16 value"""
    w3 = torch.zeros(f, l, 3, 3, dtype=torch.float64)
    tap = torch.randint(0, 9, (f,), generator=g)
    sg = _sign((f,), g)
    for fo in range(f):
        w3[fo, fo % l, int(tap[fo]) // 3, int(tap[fo]) % 3] = sg[fo]
    return w3


def _int_block(f, x_int, g, quantile, store=0):
    """one integer block fitted to its integer input x_int (n, F, h, w); quantile: block b (its 3x3 weights are +-1, +-2, +-4:
    the chain's last stores, yb and -- through dt -- dxa, then pass 2^8 quanta and are really rounded).  Block b's h is at most 64
    quanta whatever its input is.  store = STORE_YA: block a's 3x3 weights are +-2, +-4, +-8, so ya passes 2^8 quanta.
    store = STORE_DXB: block b's W1 columns F - L .. L - 1 are +-8, +-16, so dxb passes 2^8 quanta in these channels, and block
    a's 3x3 is _thin_w3: its dt stays a bf16 value although its cotangent is large."""
    _, e, l = DIMS[f]
    w1 = _pair_rows(e, f, g)
    if quantile is not None and store == STORE_DXB:
        w1[:, f - l:l] *= 2.0 ** torch.randint(3, 5, (e, 2 * l - f), generator=g).double()
    pre = torch.einsum("ef,nfyx->neyx", w1, x_int)
    b1 = torch.zeros(e, dtype=torch.float64)
    for c in range(e):
        vals = pre[:, c].reshape(-1).sort().values
        if quantile is None:
            v = float(vals[int(torch.randint(0, vals.numel(), (1,), generator=g))])
        else:
            q = quantile[0] + (quantile[1] - quantile[0]) * float(torch.rand(1, generator=g))
            v = max(float(vals[min(int(q * vals.numel()), vals.numel() - 1)]), float(vals[-1]) - 64.0)
        v -= (0.0, 0.0, 1.0, -1.0, 2.0)[int(torch.randint(0, 5, (1,), generator=g))]       # (z = 0 at some pixel for two draws in five)
        v = float(bf16_round(torch.tensor(v, dtype=torch.float64)))                        # (block b behind a large ya: b1 stays a bf16 value)
        b1[c] = -v if v != 0 else float(_sign((1,), g))
    w2 = _dealt_rows(l, e, g)
    w3 = _dealt_rows(f, 9 * l, g).view(f, l, 3, 3)
    if quantile is not None:
        w3 = w3 * 2.0 ** torch.randint(0, 3, w3.shape, generator=g).double()
    elif store == STORE_YA:
        w3 = w3 * 2.0 ** torch.randint(1, 4, w3.shape, generator=g).double()
    elif store == STORE_DXB:
        w3 = _thin_w3(f, l, g)
    return dict(w1=w1, w2=w2, w3=w3, b1=b1)


def _scaled(ip, sx, sh, st):
    """the integer block on the channel scales sx (stream), sh (h), st (t)"""
    return dict(w1=ip["w1"] * sh.view(-1, 1) / sx.view(1, -1), w2=ip["w2"] * st.view(-1, 1) / sh.view(1, -1),
                w3=ip["w3"] * sx.view(-1, 1, 1, 1) / st.view(1, -1, 1, 1), b1=ip["b1"] * sh, b2=ip["b2"] * st, b3=ip["b3"] * sx)


def _first_exact(build, tries=12):
    """the first of build(0), build(1), .. that check_exact() accepts (a tiny image may draw a mostly-zero tensor)"""
    err = None
    for k in range(tries):
        case = build(k)
        try:
            case["ref"] = check_exact(case)
            return case
        except ValueError as e_:
            err = e_
    raise err


@functools.lru_cache(maxsize=None)
def exact_case(f, n, h, w, seed=0, density=0.5, store=0):
    """One chain of two blocks on dyadic data (module docstring); `density` of the cotangent dyb is nonzero.  store: 0, or the
    family in which the tensor stored BETWEEN the blocks is really rounded (_int_block): STORE_YA (with a sparse cotangent, which
    keeps block a's dt within 8 bits under its larger 3x3 weights) or STORE_DXB; check_exact() then asks for ties in that tensor.
    Checked by check_exact(); cached: the tensors are shared and must not be written to."""
    l = DIMS[f][2]
    if store == STORE_YA:
        density = 0.25

    def build(k):
        g = torch.Generator().manual_seed(_seed(1, f, n, h, w, seed, k, store))
        x_int = torch.randint(-1, 2, (n, f, h, w), generator=g).double()
        if n * h * w <= 9:
            x_int = _sign((n, f, h, w), g)
        sx = 2.0 ** torch.randint(-3, 4, (f,), generator=g).double()
        ips, cur = [], x_int
        for blk in range(2):
            ip = _int_block(f, cur, g, None if blk == 0 else (0.75, 0.95), store)
            st = 2.0 ** torch.randint(-4, 5, (l,), generator=g).double()
            ip["b2"], ip["b3"] = _odd_for(st, g), _odd_for(sx, g)
            ip["sh"], ip["st"] = _scales_for(ip["b1"], g), st
            ips.append(ip)
            y = block_forward(cur, ip)[2]
            cur = bf16_round(y)
        pa, pb = (_scaled(ip, sx, ip["sh"], ip["st"]) for ip in ips)
        dy_int = _tern((n, f, h, w), 1.0 if n * h * w <= 9 else density, g)
        cv = sx.view(1, -1, 1, 1)
        return dict(F=f, store=store, x=(x_int * cv).float(), dyb=(dy_int / cv).float(), pa={k_: v.float() for k_, v in pa.items()},
                    pb={k_: v.float() for k_, v in pb.items()})

    return _first_exact(build)


def tap_cases(f, n, h, w):
    """cases whose 3x3 conv has ONE weight +-2^k per output channel: channel fo of set s holds tap number (s F + fo) mod 9 L of the
    list [(l, ky, kx) ...], so the sets together cover all 9 L taps.  Everything else is a block of exact_case.  Per case:
    'taps'[fo] = (l, ky, kx), 'p' the parameters, 'x', and 'ref' = dict(t, y, y_bf16)."""
    l = DIMS[f][2]
    base = exact_case(f, n, h, w)
    taps = [(li, ky, kx) for li in range(l) for ky in range(3) for kx in range(3)]
    g = torch.Generator().manual_seed(_seed(2, f, n, h, w))
    cases = []
    for s in range((len(taps) + f - 1) // f):
        p = {k: v.clone() for k, v in base["pa"].items()}
        w3 = torch.zeros(f, l, 3, 3)
        mine = [taps[(s * f + fo) % len(taps)] for fo in range(f)]
        val = _sign((f,), g) * 2.0 ** torch.randint(-3, 4, (f,), generator=g).double()
        for fo, (li, ky, kx) in enumerate(mine):
            w3[fo, li, ky, kx] = val[fo]
        p["w3"] = w3
        _, t, y = block_forward(base["x"].double(), {k: v.double() for k, v in p.items()})
        cases.append(dict(F=f, x=base["x"], p=p, taps=mine, ref=dict(t=t, y=y, y_bf16=bf16_round(y))))
    return cases


def replicate(case, order):
    """a large batch made of the images of `case` in the given order (LongTensor of image indices): (x, reference of the pair per
    image gathered the same way) -- the float64 reference is computed once per distinct image.  Forward tensors only."""
    ref = case["ref"]
    pick = lambda t: t.index_select(0, order)
    return pick(case["x"]), {blk: {k: pick(ref[blk][k]) for k in ("t", "y", "y_st")} for blk in "ab"}


def batch_order(n_total, n_distinct, seed=0):
    """image indices of a large batch: every distinct image occurs, in a non-periodic order"""
    g = torch.Generator().manual_seed(_seed(3, n_total, n_distinct, seed))
    order = torch.randint(0, n_distinct, (n_total,), generator=g)
    order[:n_distinct] = torch.randperm(n_distinct, generator=g)
    return order


# ---- the cases of the parity tests: (n, h, w) --------------------------------------------------------------------------------
UNITS = (24, 32)
GEOMETRIES = (
    (1, 1, 1), (1, 1, 30), (1, 30, 1), (1, 3, 3),                      # inside the halos (1 and 2 pixels) on both sides
    (1, 11, 23), (1, 12, 24), (1, 13, 25),                              # one tile under / exact / one-pixel slivers
    (1, 12, 25), (1, 13, 24),
    (2, 25, 49),                                                        # 3 x 3 tiles: an interior tile whose halo is all live
    (3, 13, 25),                                                        # 12 tiles, 14 chunks, the batch stride
)
TAP_GEOMETRY = (1, 13, 25)
TILE_LOOP_GEOMETRY = (3, 13, 25)
TILE_LOOP_WGS = (1, 5, 12, 13, 14, 15, None)                            # None: hotpath.block_wgrad's default
MANY_TILES = (65, 13, 25)                                               # 260 tiles
MANY_TILES_DENSITY = 0.25
MANY_TILES_WGS = (16, 64)
PERSIST_BATCHES = ((193, 13, 25), (770, 5, 7))                          # 772 / 770 tiles: >= 768, not a multiple of 256
STREAM_BATCHES = ((256, 8, 48), (360, 20, 48))                          # one round; two rounds, the second ragged
DISTINCT_IMAGES = 5
ROUNDED_GEOMETRIES = ((1, 13, 25), (2, 25, 49))
STORE_CASES = ((1, (1, 13, 25)), (2, (1, 13, 25)), (2, (2, 25, 49)))     # (STORE_YA / STORE_DXB, geometry)


def exact_family():
    """every exact case of the GPU file's parameter lists, as (name, thunk)"""
    fam = []
    for f in UNITS:
        for geom in GEOMETRIES:
            fam.append((f"F{f} {geom}", functools.partial(exact_case, f, *geom)))
        fam.append((f"F{f} many tiles", functools.partial(exact_case, f, *MANY_TILES, 0, MANY_TILES_DENSITY)))
        for store, geom in STORE_CASES:
            fam.append((f"F{f} {geom} {'ya' if store == STORE_YA else 'dxb'} rounded", functools.partial(exact_case, f, *geom, 0, 0.5, store)))
    for _, hh, ww in PERSIST_BATCHES + STREAM_BATCHES:
        fam.append((f"F24 distinct images {hh}x{ww}", functools.partial(exact_case, 24, DISTINCT_IMAGES, hh, ww)))
    return fam


# ---- rounded cases ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounded_case(f, n, h, w, seed=0):
    """random normal data, PyTorch-default-sized weights; nothing is rounded beforehand: rounding the inputs and the weights to
    bf16 is part of what the bf16 route does, so it belongs to the emulation and to the yardstick.  Two independent blocks: a on
    (x, dya), b on (xb, dyb); the pair entries run a -> b forward on x and b -> a backward on (x, xb, dyb)."""
    _, e, l = DIMS[f]                                        # (e: the expand width of w1 / w2 below)
    g = torch.Generator().manual_seed(_seed(4, f, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    mk = lambda: dict(w1=rn(e, f) / f ** 0.5, w2=rn(l, e) / e ** 0.5, w3=rn(f, l, 3, 3) / (3.0 * l ** 0.5), b1=0.1 * rn(e), b2=0.1 * rn(l),
                      b3=0.1 * rn(f))
    return dict(F=f, x=rn(n, f, h, w), xb=rn(n, f, h, w), dya=rn(n, f, h, w), dyb=rn(n, f, h, w), pa=mk(), pb=mk())


COMPARED = ("t", "dt", "y_st", "dx_st") + GRADS
RUNS = ("a", "b", "b2", "a2")                               # single blocks; block b behind a (forward); block a behind b (backward)


def _runs(case, dtype, rnd, gates=None, inter=None):
    """the four runs of a rounded case: a (x, dya), b (xb, dyb), b2 = block b on the STORED output of a, a2 = block a with the
    STORED dx of b as its cotangent.  inter: the stored tensors to chain on (the emulation's, for the reference: every block is
    compared on the inputs the kernels really see); gates: per run, as in run_block."""
    st = rnd if rnd is not None else (lambda t: t)
    fold = case["F"] % 16 != 0
    gt = gates if gates is not None else {}
    out = {}

    def one(key, x, p, dy):
        r = run_block(x, p, dy, dtype, rnd, gt.get(key), fold)
        r["y_st"], r["dx_st"] = st(r["y"]), st(r["dx"])
        out[key] = r

    one("a", case["x"], case["pa"], case["dya"])
    one("b", case["xb"], case["pb"], case["dyb"])
    src = inter if inter is not None else out
    one("b2", src["a"]["y_st"], case["pb"], torch.zeros_like(case["dyb"]))
    one("a2", case["x"], case["pa"], src["b"]["dx_st"])
    return out


def emulate(case, mode):
    """the blocks in the kernels' precision on the CPU, in float32: 'fp32' -- nothing else; 'bf16' -- with a rounding to bf16 at
    the kernels' rounding points (run_block's rnd) and at the stores of y and dx"""
    return _runs(case, torch.float32, bf16_round if mode == "bf16" else None)


@functools.lru_cache(maxsize=None)
def rounded_reference(f, n, h, w, mode):
    """(case, emulation, float64 reference, yardstick[run][tensor]).  The reference gets the emulation's gates and chains on the
    emulation's stored tensors.  The yardstick is the distance of emulate() from that reference in the tests' metric -- computed
    on the CPU alone."""
    case = rounded_case(f, n, h, w)
    emu = emulate(case, mode)
    ref = _runs(case, torch.float64, None, {k: emu[k]["z"] > 0 for k in RUNS}, emu)
    yard = {k: {v: rel_max(emu[k][v], ref[k][v]) for v in COMPARED} for k in RUNS}
    return case, emu, ref, yard
