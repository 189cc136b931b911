"""Host-side index tables that lay weights out as MFMA operand fragments.

The HIP kernels never see a (Cout, Cin, kh, kw) tensor.  They read "packed
fragments": for fragment #i, lane l = 0..63 and element j = 0..7 the value at
``packed[(i*64 + l)*8 + j]``.  This module builds, once per layer geometry, the
int64 tables ``idx`` such that ``packed = src[idx]`` where ``src`` is the
layer's canonical parameter vector (effective weight after weight-norm, then
biases, then the constants 0.0 and 1.0).  A single torch gather therefore does
zero padding, bias folding, k-order permutation and transposition at once, and
its autograd transpose scatters packed gradients back.

Fragment / accumulator lane maps (wave64, r = l & 31, hh = l >> 5), see
csrc/sr_common.h:
  natural k of element j in k-step s :  16 s + 8 hh + j
  chained k (operand = previous accumulator): 16 s + 8 (j>>2) + 4 hh + (j&3)
  accumulator reg i -> row (i&3) + 8 (i>>2) + 4 hh, column r
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, NamedTuple

import numpy as np

LANES = 64


def _grid(nfrag: int):
    """(s, r, hh, j) index arrays of shape (nfrag, 64, 8)."""
    s = np.arange(nfrag).reshape(-1, 1, 1)
    lane = np.arange(LANES).reshape(1, -1, 1)
    j = np.arange(8).reshape(1, 1, -1)
    s, lane, j = np.broadcast_arrays(s, lane, j)
    return s, lane & 31, lane >> 5, j


def k_natural(s, hh, j):
    return 16 * s + 8 * hh + j


def k_chained(s, hh, j):
    return 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)


def acc_row(i, hh):
    return (i & 3) + 8 * (i >> 2) + 4 * hh


def cinit_index(rows_src: np.ndarray, zero: int) -> np.ndarray:
    """C-init table float[2][16] for one 32-row tile: entry (hh, i) = src[rows_src[row]]
    (rows_src has 32 entries; use `zero` for rows without a bias)."""
    hh = np.arange(2).reshape(2, 1)
    i = np.arange(16).reshape(1, 16)
    return rows_src[acc_row(i, hh)].reshape(-1)


@dataclass(frozen=True)
class BlockGeom:
    """WDSR-B residual block geometry (models/basic_wdsr_b.py:98-140 in the reference):
    1x1 F->E, ReLU, 1x1 E->L, 3x3 L->F, + identity."""
    F: int
    E: int
    L: int

    @property
    def KX(self):            # x channels held in LDS (16-multiple; spare slots carry the ones channel)
        return self.F if self.F % 16 == 0 else (self.F // 16 + 1) * 16

    @property
    def fold_b1(self):       # bias of conv1 rides on the spare "ones" input channel
        return self.F % 16 != 0

    @property
    def KS1(self):
        return self.KX // 16

    @property
    def NET(self):           # 32-row tiles over the expand dimension
        return (self.E + 31) // 32

    @property
    def KS2(self):
        return (self.E + 15) // 16

    @property
    def LP(self):            # t channels held in LDS: L real + 1 ones channel, padded to 8
        return ((self.L + 1 + 7) // 8) * 8

    @property
    def CPT(self):           # 8-channel chunks per tap
        return self.LP // 8

    @property
    def FC(self):
        return self.F // 8

    @property
    def KS3(self):
        return (9 * self.CPT + self.FC + 1) // 2

    # canonical per-block source vector: w1 | w2 | w3 | b1 | b2 | b3 | 0 | 1
    @property
    def off(self) -> Dict[str, int]:
        F, E, L = self.F, self.E, self.L
        o, d = 0, {}
        for name, n in (("w1", E * F), ("w2", L * E), ("w3", F * L * 9), ("b1", E), ("b2", L), ("b3", F),
                        ("zero", 1), ("one", 1)):
            d[name] = o
            o += n
        d["size"] = o
        return d


def _sel(cond, a, b):
    return np.where(cond, a, b)


@lru_cache(maxsize=None)
def block_fwd_tables(F: int, E: int, L: int):
    """Tables for wdsr_block_fwd_kernel.  Returns dict(w=idx of packed weight blob,
    cinit=idx of float C-init tables, plus fragment counts)."""
    g = BlockGeom(F, E, L)
    o = g.off
    Z, ONE = o["zero"], o["one"]
    assert g.L < 32 and g.F <= 32 and F % 8 == 0

    # W1 as A operand: rows e (tile et), k natural over x channels (+ ones channel carrying b1)
    s, r, hh, j = _grid(g.NET * g.KS1)
    et, ks = s // g.KS1, s % g.KS1
    e = 32 * et + r
    k = k_natural(ks, hh, j)
    w1 = np.full(s.shape, Z, dtype=np.int64)
    ok = e < E
    w1 = _sel(ok & (k < F), o["w1"] + np.minimum(e, E - 1) * F + np.minimum(k, F - 1), w1)
    if g.fold_b1:
        w1 = _sel(ok & (k == F), o["b1"] + np.minimum(e, E - 1), w1)

    # W2 as A operand: rows l, k = e in chained order (k-step 2*et+s covers rows 16 s.. of h-tile et)
    s, r, hh, j = _grid(g.KS2)
    e = k_chained(s, hh, j)
    w2 = _sel((r < L) & (e < E), o["w2"] + np.minimum(r, L - 1) * E + np.minimum(e, E - 1), Z)

    # W3 as A operand: rows f_out, k = chunks q = 2s + hh; q < 9*CPT: (tap, 8 channels of t),
    # then FC chunks of x carrying the identity (residual).  t channel L is the ones channel -> b3
    # at the centre tap.
    s, r, hh, j = _grid(g.KS3)
    q = 2 * s + hh
    tap, c = q // g.CPT, q % g.CPT
    l = 8 * c + j
    is_tap = q < 9 * g.CPT
    w3 = np.full(s.shape, Z, dtype=np.int64)
    rf = np.minimum(r, F - 1)
    w3 = _sel(is_tap & (r < F) & (l < L),
              o["w3"] + (rf * L + np.minimum(l, L - 1)) * 9 + np.minimum(tap, 8), w3)
    w3 = _sel(is_tap & (r < F) & (l == L) & (tap == 4), o["b3"] + rf, w3)
    fin = 8 * (q - 9 * g.CPT) + j
    w3 = _sel((~is_tap) & (r < F) & (fin == r), ONE, w3)

    w = np.concatenate([w1.reshape(-1), w2.reshape(-1), w3.reshape(-1)])

    # C-init tables: [b2c (ones at row L)] + [b1c per e-tile when b1 is not folded]
    rows = np.full(32, Z, dtype=np.int64)
    rows[:L] = o["b2"] + np.arange(L)
    rows[L] = ONE
    cin = [cinit_index(rows, Z)]
    if not g.fold_b1:
        for t in range(g.NET):
            rows = np.full(32, Z, dtype=np.int64)
            ee = 32 * t + np.arange(32)
            rows[ee < E] = o["b1"] + ee[ee < E]
            cin.append(cinit_index(rows, Z))
    return dict(w=w, cinit=np.concatenate(cin), n_w1=g.NET * g.KS1, n_w2=g.KS2, n_w3=g.KS3, geom=g)


@lru_cache(maxsize=None)
def block_tables(F: int, E: int, L: int):
    """Tables for all residual-block kernels (forward, backward-data, weight-gradient).

    Blob sections (in 512-element fragments), forward first so wdsr_block_fwd_kernel's offsets hold:
      W1 | W2 | W3 | W3T | W2T | W1T | ID | W2N | W3D
    C-init floats: b2c[32] | b1c[NET][32] (only when b1 is not folded) | b1n[NET*32] (same condition).
    """
    fwd = block_fwd_tables(F, E, L)
    g = fwd["geom"]
    o = g.off
    Z, ONE = o["zero"], o["one"]
    KS3B = (9 * g.FC + 1) // 2
    KSI = (g.FC + 1) // 2

    # W3T as A operand of dt^T[l, px] = sum_{u, f} W3[f, l, 8-u] dy[px + u - 1, f]: rows l, chunk q = 2s+hh
    # -> read offset u = q // FC (row-major 3x3 into the halo'd dy tile), channels f = 8 (q % FC) + j.
    s, r, hh, j = _grid(KS3B)
    q = 2 * s + hh
    u, c = q // g.FC, q % g.FC
    f = 8 * c + j
    w3t = _sel((q < 9 * g.FC) & (r < L),
               o["w3"] + (np.minimum(f, F - 1) * L + np.minimum(r, L - 1)) * 9 + (8 - np.minimum(u, 8)), Z)

    # W2T as A operand of dh^T[e, px] = sum_l W2[l, e] dt^T[l, px]: rows e (tile et), k = l chained (2 k-steps)
    s, r, hh, j = _grid(g.NET * 2)
    et, ks = s // 2, s % 2
    e = 32 * et + r
    l = k_chained(ks, hh, j)
    w2t = _sel((e < E) & (l < L), o["w2"] + np.minimum(l, L - 1) * E + np.minimum(e, E - 1), Z)

    # W1T as A operand of dx^T[f, px] += sum_e W1[e, f] dpre^T[e, px]: rows f, k = e chained (k-step 2et+s)
    s, r, hh, j = _grid(g.KS2)
    e = k_chained(s, hh, j)
    w1t = _sel((r < F) & (e < E), o["w1"] + np.minimum(e, E - 1) * F + np.minimum(r, F - 1), Z)

    # identity over the FC chunks of dy (gradient of the skip connection)
    s, r, hh, j = _grid(KSI)
    q = 2 * s + hh
    ident = _sel((q < g.FC) & (r < F) & (8 * q + j == r), ONE, Z)

    # W2N as B operand of dh[px, e] = sum_l dt[px, l] W2[l, e]: columns e (tile et), k = l natural
    s, r, hh, j = _grid(g.NET * 2)
    et, ks = s // 2, s % 2
    e = 32 * et + r
    l = k_natural(ks, hh, j)
    w2n = _sel((e < E) & (l < L), o["w2"] + np.minimum(l, L - 1) * E + np.minimum(e, E - 1), Z)

    # W3D ("dense K", round 3): the 3x3 conv as ONE contraction over (window row ky, row chunk rc): the three taps of a window
    # row are 3 L contiguous elements of the t image (L real channels per pixel), cut into 4-channel chunks rc = 0 .. 3 L / 4 - 1;
    # k-step s = 4 ky + q gives lane half hh the chunks rc = 8 hh + 2 q + (j >> 2), i.e. 16 contiguous bytes at (window row
    # base) + 64 hh + 16 q: the same compile-time offset for both halves.  At L = 20 a row has 15 chunks: rc = 15 (the next
    # pixel's first chunk) gets zero weights, except in the last row where the kernel reads a "ones" chunk there whose first
    # slot carries b3.  12 k-steps where the 8-channel chunks of W3 (LP = 24 with the ones channel, plus the identity chunks
    # of the residual) need 15: the residual is the accumulator's initial value instead (csrc/wdsr_fwd_rs.h, rw_phase_b).
    # General form (round 3, 32 units): TD = L rounded up to a multiple of 4 (channels >= L of a pixel get zero weights), LCD = TD / 4
    # chunks per tap, KPR = ceil((3 LCD + 1) / 4) k-steps per window row, lane half hh of k-step q reads the chunk slots
    # 2 KPR hh + 2 q + (j >> 2); the ones chunk is slot 3 LCD of the last row (BlockCfg::TD / LCD / KPR / HALF in csrc/wdsr_block.h).
    w3d = None
    TD = (L + 3) // 4 * 4
    LCD = TD // 4
    KPR = (3 * LCD + 1 + 3) // 4
    HALF = 2 * KPR
    if 3 * LCD >= HALF and (3 * LCD - HALF) % 2 == 1:
        KS3D = 3 * KPR
        s, r, hh, j = _grid(KS3D)
        ky, q = s // KPR, s % KPR
        rc = HALF * hh + 2 * q + (j >> 2)
        jj = j & 3
        tap, l = 3 * ky + np.minimum(rc, 3 * LCD - 1) // LCD, 4 * (rc % LCD) + jj
        rf = np.minimum(r, F - 1)
        w3d = _sel((rc < 3 * LCD) & (l < L) & (r < F), o["w3"] + (rf * L + np.minimum(l, L - 1)) * 9 + np.minimum(tap, 8), Z)
        w3d = _sel((rc == 3 * LCD) & (ky == 2) & (jj == 0) & (r < F), o["b3"] + rf, w3d)
    else:
        KS3D = 0

    w = np.concatenate([fwd["w"]] + [a.reshape(-1) for a in (w3t, w2t, w1t, ident, w2n)] + ([w3d.reshape(-1)] if w3d is not None else []))
    cin = [fwd["cinit"]]
    if not g.fold_b1:
        ee = np.arange(g.NET * 32)
        cin.append(np.where(ee < E, o["b1"] + np.minimum(ee, E - 1), Z))
    sec, off = {}, 0
    for name, n in (("W1", g.NET * g.KS1), ("W2", g.KS2), ("W3", g.KS3), ("W3T", KS3B), ("W2T", g.NET * 2),
                    ("W1T", g.KS2), ("ID", KSI), ("W2N", g.NET * 2), ("W3D", KS3D)):
        sec[name] = off
        off += n
    assert off * 512 == w.size
    return dict(w=w, cinit=np.concatenate(cin), sec=sec, nfrag=off, geom=g, KS3B=KS3B, KSI=KSI, KS3D=KS3D)


# ---- accumulator-layout slabs written by the weight-gradient kernels -> canonical gradients ----
def _acc_pos(tile, row, col):
    """offset of element (row, col) of 32x32 accumulator tile #tile in a [tile][reg 16][lane 64] slab
    (lane-contiguous so the in-workgroup LDS reduction is bank-conflict free)"""
    hh = (row >> 2) & 1
    i = (row & 3) + 4 * (row >> 3)
    return (tile * 16 + i) * 64 + col + 32 * hh


@lru_cache(maxsize=None)
def block_grad_tables(F: int, E: int, L: int):
    """Gather tables: canonical gradient vector (same layout as BlockGeom.off, without the two
    constants) = slab[idx].  Slab A (wgrad12): dW1T tiles [f rows, e cols] x NET, then dW2 tiles
    [l rows, e cols] x NET, then db1[NET*32], db2[32].  Slab B (wgrad3): 9 tiles [l rows, f cols]
    indexed by read offset u (tap = 8 - u); the ones channel l = L at the centre carries db3."""
    g = BlockGeom(F, E, L)
    NET = g.NET
    e, f = np.meshgrid(np.arange(E), np.arange(F), indexing="ij")
    w1 = _acc_pos(e // 32, f, e % 32)
    l, e2 = np.meshgrid(np.arange(L), np.arange(E), indexing="ij")
    w2 = _acc_pos(NET + e2 // 32, l, e2 % 32)
    base = 2 * NET * 1024
    b1 = base + np.arange(E)
    b2 = base + NET * 32 + np.arange(L)
    slab_a = base + NET * 32 + 32
    f3, l3, tap = np.meshgrid(np.arange(F), np.arange(L), np.arange(9), indexing="ij")
    w3 = _acc_pos(8 - tap, l3, f3)
    b3 = _acc_pos(np.full(F, 4), np.full(F, L), np.arange(F))
    return dict(a=np.concatenate([w1.reshape(-1), w2.reshape(-1), b1, b2]), a_size=slab_a,
                a_order=("w1", "w2", "b1", "b2"),
                b=np.concatenate([w3.reshape(-1), b3]), b_size=9 * 1024, b_order=("w3", "b3"), geom=g)


# =====================================================================================
# head (3x3, 3 -> F) and tail (3x3 F -> 3r^2) + skip (5x5, 3 -> 3r^2) + PixelShuffle(r)
# reference: models/basic_wdsr_b.py:32-42 (head), :55-64 (tail), :66-78 (skip), :80-92 (shuffle, mean)
# =====================================================================================
# The LR image is staged in LDS as [pixel][4]: 3 colours minus the mean, and a ones channel that
# carries the bias.  A fragment chunk (8 elements) is two horizontally adjacent pixels.

@dataclass(frozen=True)
class EndsGeom:
    F: int
    R: int                      # upscale factor

    @property
    def CO(self):               # conv channels before the shuffle
        return 3 * self.R * self.R

    @property
    def NT(self):
        return (self.CO + 31) // 32

    @property
    def COP(self):              # dconv channels held in LDS
        return (self.CO + 7) // 8 * 8

    @property
    def CC(self):
        return self.COP // 8

    @property
    def FC(self):
        return self.F // 8

    @property
    def KST(self):              # k-steps of the fused tail+skip product
        return (9 * self.FC + 15 + 1) // 2

    @property
    def KSTB(self):             # k-steps of tail backward-data
        return (9 * self.CC + 1) // 2

    @property
    def tail_off(self):         # canonical tail source: wt | ws | btot | 0 | 1
        CO, F = self.CO, self.F
        o, d = 0, {}
        for name, n in (("wt", CO * F * 9), ("ws", CO * 3 * 25), ("b", CO), ("zero", 1), ("one", 1)):
            d[name] = o
            o += n
        d["size"] = o
        return d

    @property
    def head_off(self):         # canonical head source: wh | bh | 0 | 1
        F = self.F
        return {"wh": 0, "b": F * 27, "zero": F * 27 + F, "one": F * 27 + F + 1, "size": F * 27 + F + 2}


@lru_cache(maxsize=None)
def ends_tables(F: int, R: int):
    g = EndsGeom(F, R)
    CO, FC, CC = g.CO, g.FC, g.CC
    ot, oh = g.tail_off, g.head_off

    # ---- head: rows f, chunks q = 2s+hh < 6: ky = q//2, m = q%2 -> kx = 2m + (j>>2), ci = j&3 ----
    s, r, hh, j = _grid(3)
    q = 2 * s + hh
    ky, m = q // 2, q % 2
    kx, ci = 2 * m + (j >> 2), j & 3
    ok = (r < F) & (kx < 3)
    rf = np.minimum(r, F - 1)
    head = np.full(s.shape, oh["zero"], dtype=np.int64)
    head = _sel(ok & (ci < 3), oh["wh"] + ((rf * 3 + np.minimum(ci, 2)) * 3 + ky) * 3 + np.minimum(kx, 2), head)
    head = _sel(ok & (ci == 3) & (ky == 1) & (kx == 1), oh["b"] + rf, head)

    # ---- tail + skip: rows ch (NT tiles); chunks q < 9 FC: tail (tap, 8 feature channels);
    #      then 15 image chunks: ky = q'//3, m = q'%3 -> kx = 2m + (j>>2), ci = j&3 ----
    s, r, hh, j = _grid(g.NT * g.KST)
    ti, ks = s // g.KST, s % g.KST
    ch = 32 * ti + r
    chc = np.minimum(ch, CO - 1)
    q = 2 * ks + hh
    tail = np.full(s.shape, ot["zero"], dtype=np.int64)
    is_t = q < 9 * FC
    tap, c = q // FC, q % FC
    f = 8 * c + j
    tail = _sel(is_t & (ch < CO), ot["wt"] + (chc * F + np.minimum(f, F - 1)) * 9 + np.minimum(tap, 8), tail)
    qs = q - 9 * FC
    ky, m = qs // 3, qs % 3
    kx, ci = 2 * m + (j >> 2), j & 3
    is_s = (~is_t) & (qs < 15) & (ch < CO) & (kx < 5)
    tail = _sel(is_s & (ci < 3),
                ot["ws"] + ((chc * 3 + np.minimum(ci, 2)) * 5 + np.clip(ky, 0, 4)) * 5 + np.minimum(kx, 4), tail)
    tail = _sel(is_s & (ci == 3) & (ky == 2) & (kx == 2), ot["b"] + chc, tail)

    # ---- tail backward-data: rows f, chunks q < 9 CC: read offset u = q // CC, channels 8 (q%CC)+j;
    #      dfeat[px, f] = sum_{u, ch} Wt[ch, f, 8-u] dconv[px + u - 1, ch] ----
    s, r, hh, j = _grid(g.KSTB)
    q = 2 * s + hh
    u, c = q // CC, q % CC
    ch = 8 * c + j
    tbd = _sel((q < 9 * CC) & (r < F) & (ch < CO),
               ot["wt"] + (np.minimum(ch, CO - 1) * F + np.minimum(r, F - 1)) * 9 + (8 - np.minimum(u, 8)),
               ot["zero"])

    tail_w = np.concatenate([tail.reshape(-1), tbd.reshape(-1)])
    return dict(head=head.reshape(-1), tail=tail_w, geom=g, n_head=3, n_tail=g.NT * g.KST, n_tbd=g.KSTB)


@lru_cache(maxsize=None)
def ends_grad_tables(F: int, R: int):
    """Gather tables for the slabs of the tail / head weight-gradient kernels.
    Tail slab: tiles [(tap * NT + ti)] (rows ch, cols f) for the 9 taps, then [(ky * NT + ti)] (rows ch,
    cols (kx, ci) = 4 kx + ci) for the 5 skip rows.  Head slab: 3 tiles [ky] (rows f, cols 4 kx + ci).
    The bias is the ones-channel column at the centre tap."""
    g = EndsGeom(F, R)
    CO, NT = g.CO, g.NT
    ch, f, tap = np.meshgrid(np.arange(CO), np.arange(F), np.arange(9), indexing="ij")
    wt = _acc_pos(tap * NT + ch // 32, ch % 32, f)
    base = 9 * NT
    ch, ci, ky, kx = np.meshgrid(np.arange(CO), np.arange(3), np.arange(5), np.arange(5), indexing="ij")
    ws = _acc_pos(base + ky * NT + ch // 32, ch % 32, 4 * kx + ci)
    chb = np.arange(CO)
    bt = _acc_pos(base + 2 * NT + chb // 32, chb % 32, 4 * 2 + 3)
    tail = np.concatenate([wt.reshape(-1), ws.reshape(-1), bt])
    fh, ci, ky, kx = np.meshgrid(np.arange(F), np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    wh = _acc_pos(ky, fh, 4 * kx + ci)
    bh = _acc_pos(np.full(F, 1), np.arange(F), np.full(F, 4 * 1 + 3))
    head = np.concatenate([wh.reshape(-1), bh])
    return dict(tail=tail, tail_size=(9 * NT + 5 * NT) * 1024, head=head, head_size=3 * 1024, geom=g)


# =====================================================================================
# BasicVSR trunk 3x3 convs (models/basicvsr_arch.py:108-147): CI_real in {24, 27} -> 24, plain bias
# canonical source: w (24, CI_real, 3, 3) | b (24) | 0 | 1
# =====================================================================================
@lru_cache(maxsize=None)
def c3_tables(ci_real: int):
    CO = 24
    n_w = CO * ci_real * 9
    o = {"w": 0, "b": n_w, "zero": n_w + CO, "one": n_w + CO + 1, "size": n_w + CO + 2}
    # forward: rows co, chunks q = 2s+hh < 36: tap = q // 4, c = q % 4, ci = 8c + j (ones channel = ci_real)
    s, r, hh, j = _grid(18)
    q = 2 * s + hh
    tap, c = q // 4, q % 4
    ci = 8 * c + j
    rc = np.minimum(r, CO - 1)
    fw = np.full(s.shape, o["zero"], dtype=np.int64)
    fw = _sel((r < CO) & (ci < ci_real), o["w"] + (rc * ci_real + np.minimum(ci, ci_real - 1)) * 9 + tap, fw)
    fw = _sel((r < CO) & (ci == ci_real) & (tap == 4), o["b"] + rc, fw)
    # backward-data: rows ci, chunks q < 27: u = q // 3, c = q % 3, co = 8c + j, weight tap 8 - u
    s, r, hh, j = _grid(14)
    q = 2 * s + hh
    u, c = q // 3, q % 3
    co = 8 * c + j
    bw = _sel((q < 27) & (r < ci_real),
              o["w"] + (co * ci_real + np.minimum(r, ci_real - 1)) * 9 + (8 - np.minimum(u, 8)), o["zero"])
    w = np.concatenate([fw.reshape(-1), bw.reshape(-1)])
    # gradient gather: dW[co, ci, tap] = tile[8 - tap](row ci, col co); db[co] = tile[4](row ci_real, col co)
    co_, ci_, tap_ = np.meshgrid(np.arange(CO), np.arange(ci_real), np.arange(9), indexing="ij")
    gw = _acc_pos(8 - tap_, ci_, co_)
    gb = _acc_pos(np.full(CO, 4), np.full(CO, ci_real), np.arange(CO))
    return dict(w=w, grad=np.concatenate([gw.reshape(-1), gb]), off=o)


# =====================================================================================
# 64-feature propagation trunk, inference (csrc/conv64.h).  Canonical source per conv: w (f, ci_real, 3, 3) | b (f) | 0.
# Kernel input channel kk of the first conv of a (f + 3 -> f) trunk: kk < 64 = state channel kk (reference channel 3 + kk),
# 64..66 = frame (reference 0..2); 24 < f < 64 is embedded with zero rows (co >= f) and columns (state kk >= f).
# =====================================================================================
C64_CO = 64


def c64_ci_kernel(ci_real: int, f: int = C64_CO) -> int:
    """input width of a conv as the kernels see it: 80 for the (f + 3)-channel concat, 64 otherwise"""
    if ci_real == f + 3:
        return 80
    if ci_real == f:
        return 64
    raise ValueError(f"conv64: input width {ci_real} is neither {f} nor {f + 3}")


@lru_cache(maxsize=None)
def c64_tables(ci_real: int, f: int = C64_CO):
    """One conv's packed forward weights as an index vector into its canonical source (`off`): 2 x KS fragments in
    (output half ch, k-step s) order -- lane (r, hh), element j = W[co = 32 ch + r, ci(kk = 16 c + 8 hh + j), tap] with tap =
    s // (CI / 16), c = s % (CI / 16) -- then the 64 biases."""
    if not 24 < f <= C64_CO:
        raise ValueError(f"conv64: {f} output features (24 < F <= 64)")
    ci_k = c64_ci_kernel(ci_real, f)
    cpt, ks = ci_k // 16, 9 * ci_k // 16
    n_w = f * ci_real * 9
    o = {"w": 0, "b": n_w, "zero": n_w + f, "size": n_w + f + 1}
    fr, r, hh, j = _grid(2 * ks)
    ch, s = fr // ks, fr % ks
    tap, c = s // cpt, s % cpt
    kk = 16 * c + 8 * hh + j
    co = 32 * ch + r
    if ci_k == 80:
        ci = np.where(kk < f, 3 + kk, np.where((kk >= 64) & (kk < 67), kk - 64, -1))
    else:
        ci = np.where(kk < f, kk, -1)
    ok = (co < f) & (ci >= 0)
    w = _sel(ok, o["w"] + (np.minimum(co, f - 1) * ci_real + np.maximum(ci, 0)) * 9 + tap, o["zero"])
    cb = np.arange(C64_CO)
    b = np.where(cb < f, o["b"] + np.minimum(cb, f - 1), o["zero"])
    return dict(w=np.concatenate([w.reshape(-1), b]).astype(np.int64), off=o, ci_k=ci_k, ks=ks)


@lru_cache(maxsize=None)
def c64_trunk_tables(cin: int, f: int, nb: int):
    """A whole trunk over its flat parameter (conv k = weight | bias, contiguous, in state_dict order; the style of
    models/basicvsr_arch.py _trunk_tables): `blob = cat(flat, [0])[pack]` packs every conv at once, conv k from element
    `boff[k]`.  Returns (pack int64, boff list, ci_k of the first conv)."""
    first, rest = c64_tables(cin, f), c64_tables(f, f)
    total = (f * cin * 9 + f) + 2 * nb * (f * f * 9 + f)
    pack, boff, foff, npk = [], [], 0, 0
    for k in range(1 + 2 * nb):
        t = first if k == 0 else rest
        nreal = t["off"]["zero"]
        idx = np.where(t["w"] < nreal, t["w"] + foff, total)
        boff.append(npk)
        npk += len(idx)
        pack.append(idx)
        foff += nreal
    assert foff == total
    return np.concatenate(pack), boff, first["ci_k"]


# =====================================================================================
# 64-feature propagation trunk, backward of the training route (csrc/conv64_bwd.h).  Backward-data of a 3x3 stride-1 pad-1 conv IS
# that conv with the taps flipped and in / out transposed, so the backward blob is laid out exactly like a forward conv
# (c64_tables: 2 x 36 fragments | 64 biases, all zero) and c64_conv_kernel runs it.  The first conv of an (f + 3 -> f) trunk has 80
# kernel inputs, i.e. 80 backward outputs: two 64-output convs, the state half (kernel channels 0..63) and the frame half (kernel
# channels 64..66 in rows 0..2, zero rows behind).
# Weight-gradient slab of one workgroup (c64_wgrad_kernel): [tile][reg 16][lane 64]; tile = u NT + 2 cb + ob for tap 8 - u, input
# block cb, output block ob; NT = 6 at 80 kernel inputs (db = the row of the ones channel 80 in the centre tap), NT = 4 at 64 (db =
# row 0 of the two extra tiles 36, 37).
# =====================================================================================
C64_BWD_CONV_ELEMS = 2 * 36 * 512 + C64_CO


def c64_wgrad_slab(ci_k: int) -> int:
    """floats per weight-gradient slab of a conv with ci_k kernel input channels"""
    return (54 if ci_k == 80 else 38) * 1024


def _c64_kernel_channel(ci, ci_real: int, f: int):
    """kernel input channel of the reference input channel ci (see c64_tables)"""
    if ci_real == f + 3:
        return np.where(ci < 3, 64 + ci, ci - 3)
    return ci


@lru_cache(maxsize=None)
def c64_bwd_tables(ci_real: int, f: int = C64_CO):
    """One conv's backward tables over its canonical source w (f, ci_real, 3, 3) | b (f) | 0 (c64_tables' `off`):
      w     index vector of the backward blob: one 64 -> 64 conv per half (`halves`: 1, or 2 = state half | frame half), element
            (output row o, input kk, tap) = W[co = kk, ci(o), 8 - tap], zero where o or kk is padding; the 64 biases are zero
      grad  per canonical element (dW in (co, ci, tap) order, then db): its position in the weight-gradient slab
      slab  floats per slab."""
    if not 24 < f <= C64_CO:
        raise ValueError(f"conv64: {f} output features (24 < F <= 64)")
    ci_k = c64_ci_kernel(ci_real, f)
    n_w = f * ci_real * 9
    o = {"w": 0, "b": n_w, "zero": n_w + f, "size": n_w + f + 1}
    fr, r, hh, j = _grid(2 * 36)
    ch, s = fr // 36, fr % 36
    tap, c = s // 4, s % 4
    kk = 16 * c + 8 * hh + j                                   # backward input = forward output channel co
    row = 32 * ch + r                                          # backward output = forward kernel input channel
    halves = []
    for half in range(2 if ci_k == 80 else 1):
        if ci_k == 80 and half == 0:
            ci = np.where(row < f, 3 + row, -1)
        elif ci_k == 80:
            ci = np.where(row < 3, row, -1)
        else:
            ci = np.where(row < f, row, -1)
        ok = (kk < f) & (ci >= 0)
        w = _sel(ok, o["w"] + (np.minimum(kk, f - 1) * ci_real + np.maximum(ci, 0)) * 9 + (8 - tap), o["zero"])
        halves.append(np.concatenate([w.reshape(-1), np.full(C64_CO, o["zero"], dtype=np.int64)]))
    nt = 6 if ci_k == 80 else 4
    co_, ci_, tap_ = np.meshgrid(np.arange(f), np.arange(ci_real), np.arange(9), indexing="ij")
    kc = _c64_kernel_channel(ci_, ci_real, f)
    gw = _acc_pos((8 - tap_) * nt + 2 * (kc // 32) + co_ // 32, kc % 32, co_ % 32)
    cb = np.arange(f)
    gb = _acc_pos(4 * nt + 4 + cb // 32, np.full(f, 16), cb % 32) if ci_k == 80 else _acc_pos(36 + cb // 32, np.zeros(f, dtype=np.int64), cb % 32)
    return dict(w=np.concatenate(halves).astype(np.int64), halves=len(halves), grad=np.concatenate([gw.reshape(-1), gb]).astype(np.int64),
                slab=c64_wgrad_slab(ci_k), off=o, ci_k=ci_k)


@lru_cache(maxsize=None)
def c64_trunk_bwd_tables(cin: int, f: int, nb: int):
    """A whole trunk's backward tables over its flat parameter (the style of c64_trunk_tables):
      pack    `bwd_blob = cat(flat, [0])[pack]`
      boff    2 + 2 nb element offsets: conv k at boff[k] (conv 0: its state / plain-input half), boff[1 + 2 nb] = conv 0's frame half
              (-1 when the first conv has 64 kernel inputs)
      unpack  (sidx0, dst0, sidx1, dst1) int32, in the role of models.basicvsr_arch._unpack_tables: element dst[i] of a conv's
              weight | bias block of the flat gradient = sum over slabs of entry sidx[i] (sorted by slab position: coalesced reads);
              only real parameter entries appear
      ci_k, slab0, slab1, n0, n1."""
    first, rest = c64_bwd_tables(cin, f), c64_bwd_tables(f, f)
    total = (f * cin * 9 + f) + 2 * nb * (f * f * 9 + f)
    pack, boff, foff, npk, frame_off = [], [], 0, 0, -1
    for k in range(1 + 2 * nb):
        t = first if k == 0 else rest
        nreal = t["off"]["zero"]
        idx = np.where(t["w"] < nreal, t["w"] + foff, total)
        boff.append(npk)
        if k == 0 and t["halves"] == 2:
            frame_off = npk + C64_BWD_CONV_ELEMS
        npk += len(idx)
        pack.append(idx)
        foff += nreal
    assert foff == total

    def mk(t):
        g = t["grad"]
        order = np.argsort(g, kind="stable")
        return g[order].astype(np.int32), order.astype(np.int32)
    return dict(pack=np.concatenate(pack), boff=boff + [frame_off], unpack=mk(first) + mk(rest), ci_k=first["ci_k"],
                slab0=first["slab"], slab1=rest["slab"], n0=len(first["grad"]), n1=len(rest["grad"]))


# =====================================================================================
# Reconstruction of BasicVSR_origin, inference (csrc/vsr_recon.h).  Canonical source: the ten reconstruction parameters in
# state_dict order (fusion, upconv1, upconv2, conv_hr, conv_last: weight | bias each), flattened one behind the other, | 0.
# Every layer runs 64 channels wide; num_feat < 64 is embedded with zero rows and columns.
# =====================================================================================
C64_RECON_LAYERS = ("fusion", "upconv1", "upconv2", "conv_hr", "conv_last")
C64_RECON_KS_FUSION = 8                                # 1x1 over 128 kernel channels: backward state 0..63 | forward state 64..127
C64_RECON_KS_LAST = 18                                 # 9 taps x 2 chunks of 32 channels (16 x 16 x 32 MFMA)


def c64_recon_shapes(f: int):
    """(key, shape) of the reconstruction parameters of BasicVSR_origin(num_feat = f) in state_dict order"""
    return (("fusion.weight", (f, 2 * f, 1, 1)), ("fusion.bias", (f,)), ("upconv1.weight", (4 * f, f, 3, 3)),
            ("upconv1.bias", (4 * f,)), ("upconv2.weight", (256, f, 3, 3)), ("upconv2.bias", (256,)),
            ("conv_hr.weight", (64, 64, 3, 3)), ("conv_hr.bias", (64,)), ("conv_last.weight", (3, 64, 3, 3)),
            ("conv_last.bias", (3,)))


@lru_cache(maxsize=None)
def c64_recon_tables(f: int):
    """The five reconstruction layers as ONE index vector into the canonical source: `blob = cat(flat, [0])[pack]`, layer k
    (C64_RECON_LAYERS order) from element boff[k].
      fusion    2 x 8 fragments (output half ch, k-step s) of the 32 x 32 x 16 MFMA: lane (r, hh), element j =
                W[co = 32 ch + r, kk = 16 s + 8 hh + j]; kk < 64 = backward feature kk, else forward feature kk - 64; | 64 biases
      upconv1/2 four sub-pixel convs q = 2 dy + dx, each laid out as a conv64 conv (c64_tables: 2 x 36 fragments | 64 biases)
                whose output channel c is the layer's output channel 4 c + q (PixelShuffle(2): channel 4 c + 2 dy + dx of
                pixel (Y, X) -> channel c of pixel (2 Y + dy, 2 X + dx))
      conv_hr   one conv64 conv
      conv_last 18 fragments of the 16 x 16 x 32 MFMA: lane l, element j = W[co = l & 15, ci = 32 c + 8 (l >> 4) + j, tap],
                k-step s = 2 tap + c; rows co >= 3 are zero; | 3 biases | 61 zeros"""
    if not 1 <= f <= C64_CO:
        raise ValueError(f"vsr_recon: {f} features (1 <= F <= 64)")
    off, total = {}, 0
    for key, shape in c64_recon_shapes(f):
        off[key] = total
        total += int(np.prod(shape))
    zero = total
    pack, boff, npk = [], [], 0

    def add(idx):
        nonlocal npk
        npk += idx.size
        pack.append(idx.reshape(-1).astype(np.int64))

    def conv3(key, co_of, co_real, ci_real):
        """one conv64-shaped conv: output row co (0..63) = the layer's output channel co_of(co), real when co < co_real"""
        fr, r, hh, j = _grid(2 * 36)
        ch, s = fr // 36, fr % 36
        tap, c = s // 4, s % 4
        ci, co = 16 * c + 8 * hh + j, 32 * ch + r
        ok = (co < co_real) & (ci < ci_real)
        w = _sel(ok, off[key + ".weight"] + (co_of(np.minimum(co, co_real - 1)) * ci_real + np.minimum(ci, ci_real - 1)) * 9 + tap, zero)
        cb = np.arange(C64_CO)
        b = np.where(cb < co_real, off[key + ".bias"] + co_of(np.minimum(cb, co_real - 1)), zero)
        add(w)
        add(b)

    boff.append(npk)                                               # fusion
    fr, r, hh, j = _grid(2 * C64_RECON_KS_FUSION)
    ch, s = fr // C64_RECON_KS_FUSION, fr % C64_RECON_KS_FUSION
    kk, co = 16 * s + 8 * hh + j, 32 * ch + r
    col = np.where(kk < 64, kk, f + kk - 64)                       # column of fusion.weight (f, 2 f)
    ok = (co < f) & ((kk & 63) < f)
    add(_sel(ok, off["fusion.weight"] + np.minimum(co, f - 1) * 2 * f + np.minimum(col, 2 * f - 1), zero))
    cb = np.arange(C64_CO)
    add(np.where(cb < f, off["fusion.bias"] + np.minimum(cb, f - 1), zero))
    # upconv1 (4 f real outputs: f per sub-pixel), upconv2 (256 outputs)
    for key, co_real in (("upconv1", f), ("upconv2", 64)):
        boff.append(npk)
        for q in range(4):
            conv3(key, lambda c, q=q: 4 * c + q, co_real, f)
    boff.append(npk)
    conv3("conv_hr", lambda c: c, 64, 64)
    boff.append(npk)                                               # conv_last
    s = np.arange(C64_RECON_KS_LAST).reshape(-1, 1, 1)
    lane = np.arange(LANES).reshape(1, -1, 1)
    j = np.arange(8).reshape(1, 1, -1)
    s, lane, j = np.broadcast_arrays(s, lane, j)
    tap, c, co = s // 2, s % 2, lane & 15
    ci = 32 * c + 8 * (lane >> 4) + j
    add(_sel(co < 3, off["conv_last.weight"] + (np.minimum(co, 2) * 64 + ci) * 9 + tap, zero))
    add(np.where(cb < 3, off["conv_last.bias"] + np.minimum(cb, 2), zero))
    assert len(boff) == 5
    return dict(pack=np.concatenate(pack), boff=boff, off=off, zero=zero, size=total + 1)


# =====================================================================================
# Reconstruction of BasicVSR_origin, backward of the opt-in training route (csrc/vsr_recon_bwd.h; 24 < f <= 64).  Same canonical
# source as c64_recon_tables.  Weight-gradient slabs of one call: NSEC = 11 sections of `wgs` c64_wgrad_kernel slabs (WSLAB floats:
# fusion against the backward state | against the forward state | upconv1 q = 0..3 | upconv2 q = 0..3 | conv_hr), then `wgs` slabs
# of conv_last (LAST_SLAB floats: dW [co][tap][ci] | db [3] | zeros).
# =====================================================================================
C64_RECON_BWD_NSEC = 11
C64_RECON_BWD_WSLAB = 38 * 1024
C64_RECON_BWD_LAST_SLAB = 27 * 64 + 64


@lru_cache(maxsize=None)
def c64_recon_bwd_tables(f: int):
    """pack    `bwd_blob = cat(flat, [0])[pack]`, six sections from boff[k]: fusion^T towards the backward state and towards the
              forward state (each a conv64-shaped backward blob, c64_bwd_tables' construction, whose centre tap alone is nonzero: the
              1x1 conv), upconv1^T and upconv2^T (four sub-conv blobs each: output row o = the layer's input channel, input kk = the
              sub-conv's output channel, i.e. the layer's channel 4 kk + q, taps flipped), conv_hr^T, and conv_last as [co][tap][ci]
      reduce  int32, one entry per element of the ten gradients in state_dict order: k * WSLAB + e = element e of section k's slab
              (k = NSEC: conv_last's slab).  Only real rows and columns appear; padding in `pack` points at the zero slot."""
    if not 24 < f <= C64_CO:
        raise ValueError(f"vsr_recon backward: {f} features (24 < F <= 64)")
    fwd = c64_recon_tables(f)
    off, zero = fwd["off"], fwd["zero"]
    pack, boff, npk = [], [], 0

    def add(idx):
        nonlocal npk
        npk += idx.size
        pack.append(idx.reshape(-1).astype(np.int64))

    def conv3t(key, co_of, co_real, ci_real, ci_total, ci0=0, one_by_one=False):
        fr, r, hh, j = _grid(2 * 36)
        ch, s = fr // 36, fr % 36
        tap, c = s // 4, s % 4
        kk, row = 16 * c + 8 * hh + j, 32 * ch + r             # backward input = forward output; backward output = forward input
        ok = (kk < co_real) & (row < ci_real)
        elem = co_of(np.minimum(kk, co_real - 1)) * ci_total + ci0 + np.minimum(row, ci_real - 1)
        if one_by_one:
            ok = ok & (tap == 4)
            idx = off[key + ".weight"] + elem
        else:
            idx = off[key + ".weight"] + elem * 9 + (8 - tap)
        add(_sel(ok, idx, zero))
        add(np.full(C64_CO, zero, dtype=np.int64))

    ident = lambda c: c
    boff.append(npk)
    conv3t("fusion", ident, f, f, 2 * f, 0, True)
    boff.append(npk)
    conv3t("fusion", ident, f, f, 2 * f, f, True)
    for key, co_real in (("upconv1", f), ("upconv2", 64)):
        boff.append(npk)
        for q in range(4):
            conv3t(key, lambda c, q=q: 4 * c + q, co_real, f, f)
    boff.append(npk)
    conv3t("conv_hr", ident, 64, 64, 64)
    boff.append(npk)
    k, ci = np.meshgrid(np.arange(27), np.arange(64), indexing="ij")
    add(off["conv_last.weight"] + ((k // 9) * 64 + ci) * 9 + k % 9)
    assert len(boff) == 6 and all(b % 8 == 0 for b in boff)

    S = C64_RECON_BWD_WSLAB

    def wpos(sec, co, ci, tap):
        return sec * S + _acc_pos((8 - tap) * 4 + 2 * (ci // 32) + co // 32, ci % 32, co % 32)

    def bpos(sec, co):
        return sec * S + _acc_pos(36 + co // 32, np.zeros_like(co), co % 32)

    red = []
    co, c = np.meshgrid(np.arange(f), np.arange(2 * f), indexing="ij")
    red.append(np.where(c < f, wpos(0, co, np.minimum(c, f - 1), 4), wpos(1, co, np.maximum(c - f, 0), 4)))
    red.append(bpos(0, np.arange(f)))
    for key, sec0, nout in (("upconv1", 2, 4 * f), ("upconv2", 6, 256)):
        o, ci, tap = np.meshgrid(np.arange(nout), np.arange(f), np.arange(9), indexing="ij")
        red.append(wpos(sec0 + o % 4, o // 4, ci, tap))
        o = np.arange(nout)
        red.append(bpos(sec0 + o % 4, o // 4))
    co, ci, tap = np.meshgrid(np.arange(64), np.arange(64), np.arange(9), indexing="ij")
    red.append(wpos(10, co, ci, tap))
    red.append(bpos(10, np.arange(64)))
    co, ci, tap = np.meshgrid(np.arange(3), np.arange(64), np.arange(9), indexing="ij")
    red.append(C64_RECON_BWD_NSEC * S + (co * 9 + tap) * 64 + ci)
    red.append(C64_RECON_BWD_NSEC * S + 27 * 64 + np.arange(3))
    reduce = np.concatenate([r.reshape(-1) for r in red]).astype(np.int32)
    assert reduce.size == zero
    return dict(pack=np.concatenate(pack), boff=boff, reduce=reduce, off=off, zero=zero, size=zero + 1,
                per_wg=C64_RECON_BWD_NSEC * S + C64_RECON_BWD_LAST_SLAB)


# =====================================================================================
# reconstruction of MotionVectorVSR (csrc/mv_recon.h): fusion 1x1 (2F -> 2F) and conv_last = ConvTranspose2d(2F, 3, 5, stride 4)
# =====================================================================================
def mv_recon_cw(f: int) -> int:
    """channels per pixel of the trunks' state images: the 24-wide route up to F = 24, the 64-wide one above"""
    if not 1 <= f <= 64:
        raise ValueError(f"mv_recon: {f} features (1 <= F <= 64)")
    return 24 if f <= 24 else 64


def mv_recon_geom(cw: int):
    """element offsets of the blob's sections (MVCfg of csrc/mv_recon.h): kp = the padded channel count 2 cw -> multiple of 32"""
    kp = (2 * cw + 31) // 32 * 32
    ks, mb = kp // 32, kp // 16
    g = dict(kp=kp, ks=ks, mb=mb, wfu=0, bfu=mb * ks * 512)
    g["wl"] = g["bfu"] + kp
    g["bl"] = g["wl"] + 5 * ks * 512
    g["fwd_elems"] = g["bl"] + 8
    g["wlb"] = g["fwd_elems"]
    g["wfut"] = g["wlb"] + mb * 3 * 512
    g["all_elems"] = g["wfut"] + mb * ks * 512
    return g


@lru_cache(maxsize=None)
def mv_recon_tables(f: int, cw: int):
    """The reconstruction of MotionVectorVSR(num_feat = f) as ONE index vector into the canonical source
    `src = cat(fusion.weight (2f, 2f), fusion.bias (2f), conv_last.weight (2f, 3, 5, 5), conv_last.bias (3), [0])`:
    `blob = src[pack]`.  Kernel channels: cat channel c sits at kc = c (c < f: backward state) or cw + c - f (forward state) of the
    2 cw state channels; fusion's output channel c (= conv_last's input channel c) sits at c.  Everything else is zero padding.
    Fragments of the 16 x 16 x 32 MFMA, 512 elements each: lane l, element j = A[row = 16 m + (l & 15)][k = 32 s + 8 (l >> 4) + j].
      wfu   mb x ks fragments (m, s): A[oc][kc] = fusion.weight[oc, c(kc)]            | bfu: kp biases
      wl    5 x ks fragments (eb, s): A[r][uc] = conv_last.weight[uc, o, ky, kx], r = 25 o + 5 ky + kx < 75    | bl: 3 biases + 5 zeros
    and, for the backward (cw = 24 only; absent at cw = 64):
      wlb   mb x 3 fragments (m, s):  A[uc][r] = conv_last.weight[uc, o, ky, kx]   (k = r, 75 padded to 96)
      wfut  mb x ks fragments (m, s): A[kc][oc] = fusion.weight[oc, c(kc)]"""
    if cw != mv_recon_cw(f):
        raise ValueError(f"mv_recon: {f} features run on the {mv_recon_cw(f)}-channel route, not {cw}")
    g = mv_recon_geom(cw)
    kp, ks, mb = g["kp"], g["ks"], g["mb"]
    f2 = 2 * f
    off = {"fusion.weight": 0, "fusion.bias": f2 * f2, "conv_last.weight": f2 * f2 + f2, "conv_last.bias": f2 * f2 + f2 + f2 * 75}
    zero = off["conv_last.bias"] + 3

    def frags(nm, nk):
        fr = np.arange(nm * nk).reshape(-1, 1, 1)
        lane = np.arange(LANES).reshape(1, -1, 1)
        j = np.arange(8).reshape(1, 1, -1)
        fr, lane, j = np.broadcast_arrays(fr, lane, j)
        return 16 * (fr // nk) + (lane & 15), 32 * (fr % nk) + 8 * (lane >> 4) + j

    def cat_of(kc):                                   # kernel channel -> (real?, cat channel)
        ok = ((kc < cw) & (kc < f)) | ((kc >= cw) & (kc < cw + f))
        return ok, np.where(kc < cw, kc, f + kc - cw)

    def wfu(oc, kc):
        ok, c = cat_of(kc)
        ok = ok & (oc < f2)
        return _sel(ok, off["fusion.weight"] + np.minimum(oc, f2 - 1) * f2 + np.clip(c, 0, f2 - 1), zero)

    def wl(r, uc):
        ok = (r < 75) & (uc < f2)
        return _sel(ok, off["conv_last.weight"] + np.minimum(uc, f2 - 1) * 75 + np.minimum(r, 74), zero)

    pack = []
    row, k = frags(mb, ks)
    pack.append(wfu(row, k))
    cb = np.arange(kp)
    pack.append(np.where(cb < f2, off["fusion.bias"] + np.minimum(cb, f2 - 1), zero))
    row, k = frags(5, ks)
    pack.append(wl(row, k))
    cb = np.arange(8)
    pack.append(np.where(cb < 3, off["conv_last.bias"] + np.minimum(cb, 2), zero))
    if cw == 24:
        row, k = frags(mb, 3)
        pack.append(wl(k, row))
        row, k = frags(mb, ks)
        pack.append(wfu(k, row))
    pack = np.concatenate([p.reshape(-1).astype(np.int64) for p in pack])
    assert pack.size == (g["all_elems"] if cw == 24 else g["fwd_elems"])
    return dict(pack=pack, geom=g, off=off, zero=zero, size=zero + 1)


MV_SLAB64 = dict(wl=0, wfu=128 * 80, bfu=128 * 80 + 128 * 128, bl=128 * 80 + 128 * 128 + 128, size=128 * 80 + 128 * 128 + 128 + 16)


@lru_cache(maxsize=None)
def mv_recon_bwd_tables(f: int):
    """The backward of the reconstruction at cw = 64 (24 < f <= 64; mv_recon_bwd64_kernel), a blob of its own beside
    mv_recon_tables(f, 64), which stays the forward's.  Index vectors into the same canonical source `src` (mv_recon_tables):
      pack    wlb | wfut, `blob = src[pack]`, fragments as in mv_recon_tables (lane l, element j = A[16 m + (l & 15)][32 s + 8 (l >> 4) + j]):
              wlb   8 x 3 fragments (m, s): A[uc][r] = conv_last.weight[uc, o, ky, kx], r = 25 o + 5 ky + kx (k = r, 75 padded to 96)
              wfut  8 x 4 fragments (m, s): A[kc][oc] = fusion.weight[oc, c(kc)], kc = c (c < f) or 64 + c - f
      reduce  the slab element (MV_SLAB64: dW_last [128][80] | dW_fu [128][128] | db_fu [128] | db_last [3]) of every element of
              grads = dW_fu (2f, 2f) | db_fu (2f) | dW_last (2f, 3, 5, 5) | db_last (3): real rows and columns only
    Padding rows and columns of `pack` point at the zero slot `zero`."""
    if not 24 < f <= 64:
        raise ValueError(f"mv_recon backward at 64 channels: {f} features (24 < F <= 64)")
    cw, kp, ks, mb, ksb = 64, 128, 4, 8, 3
    f2 = 2 * f
    off = {"fusion.weight": 0, "fusion.bias": f2 * f2, "conv_last.weight": f2 * f2 + f2, "conv_last.bias": f2 * f2 + f2 + f2 * 75}
    zero = off["conv_last.bias"] + 3

    def frags(nm, nk):
        fr = np.arange(nm * nk).reshape(-1, 1, 1)
        lane = np.arange(LANES).reshape(1, -1, 1)
        j = np.arange(8).reshape(1, 1, -1)
        fr, lane, j = np.broadcast_arrays(fr, lane, j)
        return 16 * (fr // nk) + (lane & 15), 32 * (fr % nk) + 8 * (lane >> 4) + j

    uc, r = frags(mb, ksb)
    wlb = _sel((r < 75) & (uc < f2), off["conv_last.weight"] + np.minimum(uc, f2 - 1) * 75 + np.minimum(r, 74), zero)
    kc, oc = frags(mb, ks)
    real = (kc < f) | ((kc >= cw) & (kc < cw + f))
    c = np.clip(np.where(kc < cw, kc, f + kc - cw), 0, f2 - 1)
    wfut = _sel(real & (oc < f2), off["fusion.weight"] + np.minimum(oc, f2 - 1) * f2 + c, zero)
    pack = np.concatenate([p.reshape(-1).astype(np.int64) for p in (wlb, wfut)])
    assert pack.size == mb * ksb * 512 + mb * ks * 512
    S = MV_SLAB64
    row, ic = np.divmod(np.arange(f2 * f2), f2)
    uc, r = np.divmod(np.arange(f2 * 75), 75)
    reduce = np.concatenate([S["wfu"] + row * 128 + np.where(ic < f, ic, cw + ic - f), S["bfu"] + np.arange(f2),
                             S["wl"] + uc * 80 + r, S["bl"] + np.arange(3)]).astype(np.int64)
    return dict(pack=pack, reduce=reduce, wlb=0, wfut=mb * ksb * 512, off=off, zero=zero, size=zero + 1, slab=S["size"])


# =====================================================================================
# NAS supernet block (models/wdsr_b.py:375-496): canonical source per block
#   wdw3 (F,9) | wdw5 (F,25) | wdw7 (F,49) | bdw (3,F) | wpw (3,F,F) | bpw (3,F) | mg (F) | ms (F) | m1 (F) | 0 | 1
# =====================================================================================
@lru_cache(maxsize=None)
def nas_tables(F: int):
    o, off = {}, 0
    for name, n in (("wdw3", F * 9), ("wdw5", F * 25), ("wdw7", F * 49), ("bdw", 3 * F), ("wpw", 3 * F * F),
                    ("bpw", 3 * F), ("mg", F), ("ms", F), ("m1", F), ("zero", 1), ("one", 1)):
        o[name] = off
        off += n
    o["size"] = off
    Z = o["zero"]
    ch = np.arange(32)
    chc = np.minimum(ch, F - 1)
    dwp = []
    for key, kk in (("wdw3", 9), ("wdw5", 25), ("wdw7", 49)):
        tap = np.arange(kk).reshape(-1, 1)
        dwp.append(np.where(ch < F, o[key] + chc * kk + tap, Z).reshape(-1))       # [tap][32]
    for k in range(3):
        dwp.append(np.where(ch < F, o["bdw"] + k * F + chc, Z))
    for key in ("m1", "mg", "ms"):
        dwp.append(np.where(ch < F, o[key] + chc, Z))
    dwp = np.concatenate(dwp)
    assert dwp.size == (83 + 3 + 3) * 32
    # pointwise fragments: forward (rows co, k = ci natural), backward (rows ci, k = co chained)
    fw, bw = [], []
    for k in range(3):
        s, r, hh, j = _grid(2)
        ci = k_natural(s, hh, j)
        fw.append(_sel((r < F) & (ci < F), o["wpw"] + (k * F + np.minimum(r, F - 1)) * F + np.minimum(ci, F - 1), Z))
        co = k_chained(s, hh, j)
        bw.append(_sel((r < F) & (co < F), o["wpw"] + (k * F + np.minimum(co, F - 1)) * F + np.minimum(r, F - 1), Z))
    frags = np.concatenate([a.reshape(-1) for a in fw + bw])
    tabs = []
    for k in range(3):
        rows = np.where(ch < F, o["bpw"] + k * F + chc, Z)
        tabs.append(cinit_index(rows, Z))
    for key in ("ms", "mg"):
        tabs.append(cinit_index(np.where(ch < F, o[key] + chc, Z), Z))
    tabs = np.concatenate(tabs)
    # gradient gathers
    co_, ci_ = np.meshgrid(np.arange(F), np.arange(F), indexing="ij")
    g_wpw = np.stack([k * 1088 + _acc_pos(0, co_, ci_) for k in range(3)]).reshape(-1)
    g_bpw = np.stack([k * 1088 + 1024 + np.arange(F) for k in range(3)]).reshape(-1)
    g_r = np.stack([k * 1088 + 1056 + np.arange(F) for k in range(3)]).reshape(-1)
    tb = (0, 9, 34)
    g_wdw = [np.stack([(tb[i] + np.arange(kk)) * 32 + c for c in range(F)]).reshape(-1) for i, kk in enumerate((9, 25, 49))]
    g_bdw = np.stack([(83 + k) * 32 + np.arange(F) for k in range(3)]).reshape(-1)
    return dict(off=o, dwp=dwp, frags=frags, tabs=tabs, g_wpw=g_wpw, g_bpw=g_bpw, g_r=g_r, g_wdw=g_wdw, g_bdw=g_bdw,
                g_sA=86 * 32 + np.arange(F), g_sB=87 * 32 + np.arange(F), pw_slab=3 * 1088 + 4, dw_slab=88 * 32, sxy=3 * 1088)


def nas_prep_tables(F: int, nb: int, layout, blocks=None):
    """Tables for the native parameter plumbing of the supernet body (csrc/wdsr_prep.h through sr_param_pack / sr_param_grads).
    `layout`: NAS_MODEL._layout = (key suffix, offset in the flat parameter, count, (nb, ...) shape) per kind, stacked over
    blocks.  Source row of block b = nas_tables(F)['off'] columns; gradient row = the same columns followed by the extra sums
    r[3][F] | sxy | sA[F] | sB[F] the mask / gate gradients are made of.
    `blocks`: the blocks that run, in order (eval drops skipped blocks; default all `nb`): row j of the source / gradient
    buffers belongs to block blocks[j].
    Returns chan_tab int32[nb * 6F][4] = {v_off, g_off, K, dst}, bias_tab int32[nb * 6F][3] = {flat index, -1, dst},
    the two slab scatters (sidx, dst) and the row sizes."""
    t = nas_tables(F)
    o = t["off"]
    size = o["size"]
    lay = {name: (off, n, shape) for name, off, n, shape in layout}
    ex = dict(r=size, sxy=size + 3 * F, sA=size + 3 * F + 1, sB=size + 4 * F + 1)
    ds = size + 5 * F + 1
    chan, bias = [], []
    c = np.arange(F)
    for row, b in enumerate(range(nb) if blocks is None else blocks):
        for ki, k in enumerate((3, 5, 7)):
            for j, (K, dst0) in ((0, (k * k, o[f"wdw{k}"])), (2, (F, o["wpw"] + ki * F * F))):
                ov, _n, _s = lay[f"body.{k}.0.body.{j}.weight_v"]
                og, _n, _s = lay[f"body.{k}.0.body.{j}.weight_g"]
                chan.append(np.stack([ov + (b * F + c) * K, og + b * F + c, np.full(F, K), row * size + dst0 + c * K], axis=1))
                ob, _n, _s = lay[f"body.{k}.0.body.{j}.bias"]
                bias.append(np.stack([ob + b * F + c, np.full(F, -1), row * size + o["bdw" if j == 0 else "bpw"] + ki * F + c], axis=1))
    chan_tab = np.concatenate(chan).astype(np.int32)
    bias_tab = np.concatenate(bias).astype(np.int32)
    # the weight-norm backward reads d(src) at the same dst offsets but in rows of `ds` columns
    chan_bwd, bias_bwd = chan_tab.copy(), bias_tab.copy()
    chan_bwd[:, 3] = (chan_tab[:, 3] // size) * ds + chan_tab[:, 3] % size
    bias_bwd[:, 2] = (bias_tab[:, 2] // size) * ds + bias_tab[:, 2] % size
    pw_sidx = np.concatenate([t["g_wpw"], t["g_bpw"], t["g_r"], [t["sxy"]]])
    pw_dst = np.concatenate([o["wpw"] + np.arange(3 * F * F), o["bpw"] + np.arange(3 * F), ex["r"] + np.arange(3 * F), [ex["sxy"]]])
    dw_sidx = np.concatenate(list(t["g_wdw"]) + [t["g_bdw"], t["g_sA"], t["g_sB"]])
    dw_dst = np.concatenate([o["wdw3"] + np.arange(9 * F), o["wdw5"] + np.arange(25 * F), o["wdw7"] + np.arange(49 * F),
                             o["bdw"] + np.arange(3 * F), ex["sA"] + np.arange(F), ex["sB"] + np.arange(F)])
    # pairs in slab order: neighbouring threads of the scatter kernel then read neighbouring slab entries
    op, od = np.argsort(pw_sidx, kind="stable"), np.argsort(dw_sidx, kind="stable")
    pw_sidx, pw_dst, dw_sidx, dw_dst = pw_sidx[op], pw_dst[op], dw_sidx[od], dw_dst[od]
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return dict(chan_tab=chan_tab, bias_tab=bias_tab, chan_bwd=i32(chan_bwd), bias_bwd=i32(bias_bwd), pw_sidx=i32(pw_sidx),
                pw_dst=i32(pw_dst), dw_sidx=i32(dw_sidx), dw_dst=i32(dw_dst), size=size, ds=ds, extra=ex, off=o)



# =====================================================================================
# SPyNet's 7x7 convolutions (reference: models/spynet_arch.py:17-22) -> csrc/spynet_conv.h
# =====================================================================================
@lru_cache(maxsize=None)
def conv7_tables(cin: int, cout: int):
    """Gather table for one 7x7 layer: packed = src[idx] with src = weight (cout, cin, 7, 7).reshape(-1) | 0.0, laid out as the
    kernel consumes it: [ky][k-step][32-row tile][lane][8].  k-step s (cin >= 16) = (tap kx = s // (cin/16), channels
    16 (s % (cin/16)) + 8 hh + j); cin = 8: two adjacent taps per k-step, kx = 2 s + hh (kx = 7: zero), channel j."""
    assert cin == 8 or cin % 16 == 0
    mt = (cout + 31) // 32
    kpr = 4 if cin == 8 else 7 * (cin // 16)
    zero = cout * cin * 49
    ky = np.arange(7).reshape(7, 1, 1, 1, 1)
    s = np.arange(kpr).reshape(1, kpr, 1, 1, 1)
    m = np.arange(mt).reshape(1, 1, mt, 1, 1)
    lane = np.arange(64).reshape(1, 1, 1, 64, 1)
    j = np.arange(8).reshape(1, 1, 1, 1, 8)
    ky, s, m, lane, j = np.broadcast_arrays(ky, s, m, lane, j)
    r, hh = lane & 31, lane >> 5
    co = 32 * m + r
    if cin == 8:
        kx, ci = 2 * s + hh, j
    else:
        cc = cin // 16
        kx, ci = s // cc, 16 * (s % cc) + 8 * hh + j
    ok = (co < cout) & (kx < 7)
    idx = np.where(ok, ((np.minimum(co, cout - 1) * cin + ci) * 7 + ky) * 7 + np.minimum(kx, 6), zero)
    return dict(idx=idx.reshape(-1).astype(np.int64), mt=mt, kpr=kpr)


@lru_cache(maxsize=None)
def conv7_bwd_tables(cin: int, cout: int):
    """Gather table of the backward-data operand of the 7x7 layer cin -> cout: the input gradient is the 7x7 / pad 3 convolution
    of dy with wt[ci][co][ky][kx] = w[co][ci][6 - ky][6 - kx] (rotated by 180 degrees, channel roles swapped), i.e. the layer
    cin_t = max(cout, 8) -> cout_t = cin in conv7_tables' fragment order.  packed = src[idx] with src = weight (cout, cin, 7,
    7).reshape(-1) | 0.0; the channels cout .. cin_t - 1 of the last layer's padded two-channel gradient gather the zero."""
    cin_t, cout_t = max(cout, 8), cin
    assert cin_t == 8 or cin_t % 16 == 0
    mt = (cout_t + 31) // 32
    kpr = 4 if cin_t == 8 else 7 * (cin_t // 16)
    zero = cout * cin * 49
    ky = np.arange(7).reshape(7, 1, 1, 1, 1)
    s = np.arange(kpr).reshape(1, kpr, 1, 1, 1)
    m = np.arange(mt).reshape(1, 1, mt, 1, 1)
    lane = np.arange(64).reshape(1, 1, 1, 64, 1)
    j = np.arange(8).reshape(1, 1, 1, 1, 8)
    ky, s, m, lane, j = np.broadcast_arrays(ky, s, m, lane, j)
    r, hh = lane & 31, lane >> 5
    row = 32 * m + r                                    # output channel of the transposed layer = input channel of the forward
    if cin_t == 8:
        kx, c = 2 * s + hh, j
    else:
        cc = cin_t // 16
        kx, c = s // cc, 16 * (s % cc) + 8 * hh + j     # contraction channel = output channel of the forward
    ok = (row < cout_t) & (kx < 7) & (c < cout)
    idx = np.where(ok, ((np.minimum(c, cout - 1) * cin + np.minimum(row, cin - 1)) * 7 + (6 - ky)) * 7 + (6 - np.minimum(kx, 6)), zero)
    return dict(idx=idx.reshape(-1).astype(np.int64), mt=mt, kpr=kpr, cin=cin_t, cout=cout_t)


@lru_cache(maxsize=None)
def conv7_wgrad_tables(cin: int, cout: int):
    """Slab -> flat-gradient tables of conv7_wgrad_kernel for the layer cin -> cout: gflat[dst[i]] = sum over slabs of
    slab[sidx[i]], gflat = dW (cout, cin, 7, 7).reshape(-1) | db (cout).  Tile (row tile rt, column tile ct, tap) =
    rt ncol + 49 ct + tap with ncol = 49 nct + 1; tile rt ncol + 49 nct is the bias tile (column 0 is read).  Only real
    elements are listed: the zero-padded rows (cout .. 32 nrt - 1) and columns (cin .. 32 nct - 1) are never read."""
    ca, cb = max(cout, 8), cin
    nrt, nct = (ca + 31) // 32, (cb + 31) // 32
    ncol = nct * 49 + 1
    ntl = nrt * ncol
    co, ci, tap = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(49), indexing="ij")
    sw = _acc_pos((co // 32) * ncol + (ci // 32) * 49 + tap, co % 32, ci % 32)
    dw = (co * cin + ci) * 49 + tap
    cb_ = np.arange(cout)
    sb = _acc_pos((cb_ // 32) * ncol + nct * 49, cb_ % 32, np.zeros(cout, dtype=np.int64))
    db = cout * cin * 49 + cb_
    i32 = lambda a: np.ascontiguousarray(a.reshape(-1), dtype=np.int32)
    return dict(sidx=i32(np.concatenate([sw.reshape(-1), sb])), dst=i32(np.concatenate([dw.reshape(-1), db])), ntl=ntl,
                slab=ntl * 1024, ng=(ntl + 31) // 32, ca=ca, cb=cb)


CONV7_WGRAD_WGS = 32                # cap of the weight-gradient workgroups per layer (slabs the reduction sums)


def conv7_wgrad_wgs(n: int, h: int, w: int, cap: int = CONV7_WGRAD_WGS) -> int:
    """workgroups of a conv7 weight-gradient launch: every workgroup walks the same number of 16 x 16 pixel tiles (up to one)"""
    total = n * ((h + 15) // 16) * ((w + 15) // 16)
    per = -(-total // cap)
    return -(-total // per)


# =====================================================================================
# Searched network (Result_Model, csrc/result_block.h): dense k x k convs on NHWC rows of CI channels
# =====================================================================================
RM_WGRAD_TPG = 32                   # accumulator tiles per tile group of rm_wgrad_kernel (8 waves x 4)


def rm_cp(R: int) -> int:
    """channels of the un-shuffled HR gradient image (3 R^2 padded to a multiple of 16)"""
    return {2: 16, 3: 32, 4: 48}[R]


@lru_cache(maxsize=None)
def rm_conv_index(rows: int, ci: int, k: int) -> np.ndarray:
    """gather index: packed fragments [row tile][k-step][lane 64][8] of a (rows, ci, k, k) weight, read from
    w.reshape(-1) with a zero appended at position rows * ci * k * k.  Lane (r, hh), element j of k-step s holds
    W[32 t + r][ci = kk % ci][tap = kk // ci] with kk = 16 s + 8 hh + j; zero past the last row or the last tap."""
    nrt, ks = (rows + 31) // 32, (k * k * ci + 15) // 16
    t, s, lane, j = np.meshgrid(np.arange(nrt), np.arange(ks), np.arange(64), np.arange(8), indexing="ij")
    row = 32 * t + (lane & 31)
    kk = 16 * s + 8 * (lane >> 5) + j
    tap, c = kk // ci, kk % ci
    ok = (row < rows) & (tap < k * k)
    idx = (np.minimum(row, rows - 1) * ci + c) * (k * k) + np.minimum(tap, k * k - 1)
    return np.where(ok, idx, rows * ci * k * k).reshape(-1).astype(np.int64)


def rm_wgrad_groups(ca: int, k: int) -> int:
    ntl = (ca + 31) // 32 * (k * k + 1)
    return (ntl + RM_WGRAD_TPG - 1) // RM_WGRAD_TPG


@lru_cache(maxsize=None)
def rm_wgrad_index(ca: int, rows: int, cols: int, k: int):
    """gather index of the summed rm_wgrad slab (tile t at t * 1024, accumulator layout): (weight gradient (rows, cols, k, k),
    bias gradient (rows)).  Tile (row tile rt, tap) = rt (k^2 + 1) + tap; tap k^2 is the bias (every column holds the sum)."""
    ntap = k * k + 1
    co, c, tap = np.meshgrid(np.arange(rows), np.arange(cols), np.arange(k * k), indexing="ij")
    w = _acc_pos((co // 32) * ntap + tap, co % 32, c)
    b = _acc_pos((np.arange(rows) // 32) * ntap + k * k, np.arange(rows) % 32, np.zeros(rows, dtype=np.int64))
    return w.reshape(-1).astype(np.int64), b.astype(np.int64)


@lru_cache(maxsize=None)
def rm_block_index(F: int, IN: int, split: int, k: int, transposed: bool) -> np.ndarray:
    """rm_conv_index(F, F, k) composed with the window embedding: gathers the packed fragments of block [IN, split, k] straight
    from w.reshape(-1) of the (split, split, k, k) weight plus a zero at split^2 k^2.  transposed: the backward-data operand
    (W^T with both taps flipped)."""
    a, kk = IN - split, k * k
    d = rm_conv_index(F, F, k)
    zero = split * split * kk
    row, c, tap = d // kk // F, d // kk % F, d % kk
    live = (d < F * F * kk) & (row >= a) & (row < IN) & (c >= a) & (c < IN)
    if transposed:
        src = ((c - a) * split + (row - a)) * kk + (kk - 1 - tap)
    else:
        src = ((row - a) * split + (c - a)) * kk + tap
    return np.where(live, src, zero).astype(np.int64)


@lru_cache(maxsize=None)
def rm_block_bias_index(IN: int, split: int) -> np.ndarray:
    """bias float[32] of block [IN, split, k] from cat(b, 0): channel c < 32 holds b[c - (IN - split)] inside the window"""
    a, c = IN - split, np.arange(32)
    return np.where((c >= a) & (c < IN), c - a, split).astype(np.int64)


@lru_cache(maxsize=None)
def rm_block_wgrad_index(F: int, IN: int, split: int, k: int):
    """rm_wgrad_index(F, F, F, k) restricted to the window: (weight (split, split, k, k), bias (split)) gathers"""
    a = IN - split
    iw, ib = rm_wgrad_index(F, F, F, k)
    return np.ascontiguousarray(iw.reshape(F, F, k * k)[a:IN, a:IN].reshape(-1)), np.ascontiguousarray(ib[a:IN])


# ---- bicubic downscale (csrc/bicubic.h): the weights and source indices of one pass of MATLAB's imresize ----
BICUBIC_SCALES = (2, 3, 4)


def _cubic(x: np.ndarray) -> np.ndarray:
    """Keys' cubic convolution kernel (a = -0.5), support [-2, 2]; the two pieces are masked and added, as MATLAB's `cubic` does"""
    a1 = np.abs(x)
    a2 = a1 * a1
    a3 = a2 * a1
    inner = (1.5 * a3 - 2.5 * a2 + 1) * (a1 <= 1)
    outer = (-0.5 * a3 + 2.5 * a2 - 4 * a1 + 2) * ((1 < a1) & (a1 <= 2))
    return inner + outer


@lru_cache(maxsize=256)
def bicubic_tables(in_len: int, scale: int):
    """(weights float64 [out_len, taps], indices int32 [out_len, taps]) of one pass of the MATLAB-compatible antialiased bicubic
    downscale by the integer `scale` (third_party/matlab_imresize/imresize.py `contributions` with the cubic kernel of width 4,
    bit for bit: same float64 operations in the same order), out_len = ceil(in_len / scale):
    output o (1-based x) sits at u = x / s + 0.5 (1 - 1 / s) in the source, s = 1 / scale; the kernel is stretched to
    s * cubic(s * d), width 4 / s; the leftmost candidate tap is floor(u - width / 2), there are ceil(width) + 2 candidates;
    each row of weights is normalised by its sum; indices past either end are reflected symmetrically (period 2 in_len, so a
    source shorter than the support reflects more than once); candidate columns whose weight is zero in every row are dropped.
    The arrays are cached: do not write to them."""
    in_len, scale = int(in_len), int(scale)
    if scale not in BICUBIC_SCALES:
        raise ValueError(f"bicubic_tables: scale {scale} not in {BICUBIC_SCALES}")
    if in_len < 1:
        raise ValueError("bicubic_tables: need a positive source length")
    s = 1.0 / scale
    out_len = -(-in_len // scale)
    width = 4.0 / s
    x = np.arange(1, out_len + 1).astype(np.float64)
    u = x / s + 0.5 * (1 - 1 / s)
    left = np.floor(u - width / 2)
    ntaps = int(np.ceil(width)) + 2
    taps = (left[:, None] + np.arange(ntaps) - 1).astype(np.int32)        # 0-based source positions, before reflection
    w = s * _cubic(s * (u[:, None] - taps - 1))
    w = w / w.sum(axis=1)[:, None]
    mirror = np.concatenate((np.arange(in_len), np.arange(in_len - 1, -1, -1))).astype(np.int32)
    idx = mirror[np.mod(taps, 2 * in_len)]
    keep = np.any(w, axis=0)
    w, idx = np.ascontiguousarray(w[:, keep]), np.ascontiguousarray(idx[:, keep])
    w.setflags(write=False)
    idx.setflags(write=False)
    return w, idx


# =====================================================================================
# per-frame video network (models/single_image_model.py, csrc/frame_net.h): 2 nb + 1 weight-normed 3x3 convs C -> C on
# 32-channel NHWC activations and ConvTranspose2d(C, 3, 5, stride 4)
# =====================================================================================
FN_C, FN_TH, FN_TW = 32, 8, 32            # activation channels; the block kernel's tile (FnCfg)
FN_CONV_ELEMS = 18 * 512 + 32             # one conv: 18 fragments + 32 biases
FN_UP_ELEMS = 5 * 512 + 8
FN_ENCODER, FN_BLOCKS, FN_LAST, FN_UP, FN_WRITE_D, FN_ALL = 1, 2, 4, 8, 16, 15


@lru_cache(maxsize=None)
def fn_tables(channel: int, nb: int):
    """(layout, offsets) of the packed blob of Result_Model(4, channel, nb, 3): `blob = src[layout["pack"]]` with the canonical source
    `src = cat(w_0 (C,C,3,3), b_0 (C), .., w_2nb, b_2nb, shuf.0.weight (C,3,5,5), shuf.0.bias (3), [0])` of EFFECTIVE weights, convs in
    forward order (block i: 2 i and 2 i + 1, the body's last conv: 2 nb).  offsets[j] = element offset of conv j, offsets[2 nb + 1] =
    the upsampler's.
      conv   18 fragments of the 32 x 32 x 16 MFMA: lane l, element j of fragment s = W[row = l & 31][ci = kk % 32][tap = kk // 32],
             kk = 16 s + 8 (l >> 5) + j, tap = 3 ky + kx; then the 32 biases.  Rows and ci >= C are zero.
      up     5 fragments of the 16 x 16 x 32 MFMA: lane l, element j of fragment eb = shuf.0.weight[c = 8 (l >> 4) + j][o, ky, kx] at
             E row r = 16 eb + (l & 15) = 25 o + 5 ky + kx (< 75); then the 3 biases and 5 zeros."""
    if not 1 <= channel <= FN_C or nb < 0:
        raise ValueError(f"fn_tables: {channel} channels, {nb} blocks (1 <= channel <= 32, blocks >= 0)")
    C, nconv = channel, 2 * nb + 1
    per = C * C * 9 + C
    up_w = nconv * per
    up_b = up_w + C * 75
    zero = up_b + 3
    d = rm_conv_index(FN_C, FN_C, 3)
    row, c, tap = d // 9 // FN_C, d // 9 % FN_C, d % 9
    live = (d < FN_C * FN_C * 9) & (row < C) & (c < C)
    wrel = np.where(live, (np.minimum(row, C - 1) * C + np.minimum(c, C - 1)) * 9 + tap, -1)
    ch = np.arange(FN_C)
    brel = np.where(ch < C, C * C * 9 + np.minimum(ch, C - 1), -1)
    rel = np.concatenate([wrel, brel])
    pack = [np.where(rel >= 0, j * per + rel, zero) for j in range(nconv)]
    fr = np.arange(5).reshape(-1, 1, 1)
    lane = np.arange(LANES).reshape(1, -1, 1)
    j = np.arange(8).reshape(1, 1, -1)
    fr, lane, j = np.broadcast_arrays(fr, lane, j)
    r, uc = 16 * fr + (lane & 15), 8 * (lane >> 4) + j
    pack.append(np.where((r < 75) & (uc < C), up_w + np.minimum(uc, C - 1) * 75 + np.minimum(r, 74), zero).reshape(-1))
    cb = np.arange(8)
    pack.append(np.where(cb < 3, up_b + np.minimum(cb, 2), zero))
    pack = np.concatenate([p.astype(np.int64) for p in pack])
    offsets = [jj * FN_CONV_ELEMS for jj in range(nconv + 1)]
    assert pack.size == offsets[-1] + FN_UP_ELEMS
    return dict(pack=pack, size=zero + 1, zero=zero, per=per, up_w=up_w, up_b=up_b), offsets


FN_MAX_OUT = 32768                        # largest output height / width of the sized upsampler kernels (SR_FN_MAX_OUT)


class ResizeAxis(NamedTuple):
    """resize_axis' answer: per output d the two taps i0, i1 (int32) and the weight lam of i1 (fp32); per input i the outputs
    lo[i] .. hi[i] (int32) whose first tap it is"""
    i0: np.ndarray
    i1: np.ndarray
    lam: np.ndarray
    lo: np.ndarray
    hi: np.ndarray


@lru_cache(maxsize=64)
def resize_axis(n_in: int, n_out: int) -> ResizeAxis:
    """THE arithmetic of F.interpolate(.., size, mode='bilinear') (align_corners False, no scale factor) along one axis of n_in samples
    resized to n_out, as ATen's fp32 kernels do it: the sized upsampler kernels (csrc/frame_net.h, csrc/frame_net_bwd.h) read these
    tables and compute none of it themselves, and so does every reference of theirs.

        scale = float32(n_in) / float32(n_out);  src = max(scale * (d + 0.5) - 0.5, 0);  i0 = min(trunc(src), n_in - 1)
        lam = clip(src - i0, 0, 1);  i1 = min(i0 + 1, n_in - 1);          out[d] = (1 - lam[d]) in[i0[d]] + lam[d] in[i1[d]]

    Every operation is a numpy fp32 operation of its own, rounded once, never contracted: lam is ill-conditioned (one ulp of src near
    index 1000 moves it by 1e-4, and so does fusing the multiply and the subtraction into an FMA), so it is computed in ONE place.
    i0 is non-decreasing; the adjoint form for a gather backward is, per input i, the contiguous range lo[i] .. hi[i] of outputs with
    i0 == i: lo[i] = #{d: i0[d] < i}, hi[i] = #{d: i0[d] <= i} - 1, empty when hi[i] = lo[i] - 1.  The ranges partition 0 .. n_out - 1.
    The arrays are shared (cached) and read-only."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_axis: {n_in} -> {n_out} samples (both >= 1)")
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    d = np.arange(n_out, dtype=np.float32)
    src = np.maximum(scale * (d + f32(0.5)) - f32(0.5), f32(0.0))
    i0 = np.minimum(np.trunc(src).astype(np.int32), np.int32(n_in - 1))
    lam = np.clip(src - i0.astype(np.float32), f32(0.0), f32(1.0))
    i1 = np.minimum(i0 + np.int32(1), np.int32(n_in - 1))
    i = np.arange(n_in)
    lo = np.searchsorted(i0, i, side="left").astype(np.int32)
    hi = (np.searchsorted(i0, i, side="right") - 1).astype(np.int32)
    assert src.dtype == np.float32 and lam.dtype == np.float32 and i0.dtype == np.int32 and i1.dtype == np.int32
    out = ResizeAxis(i0, i1, lam, lo, hi)
    for a in out:
        a.setflags(write=False)
    return out


def fn_resize_tables(n_in: int, n_out: int):
    """resize_axis(n_in, n_out) as the sized kernels' two tables: int32 i0 [n_out] | lo [n_in] | hi [n_in], fp32 lam [n_out]"""
    ax = resize_axis(n_in, n_out)
    return np.concatenate([ax.i0, ax.lo, ax.hi]), ax.lam


FN_BWD_UP, FN_BWD_LAST, FN_BWD_BLOCKS, FN_BWD_ENCODER, FN_BWD_ALL = 1, 2, 4, 8, 15
FN_BWD_CONV_ELEMS = 18 * 512              # one conv's backward-data operand
FN_BWD_UP_ELEMS = 2 * 3 * 512             # the upsampler's: 32 channel rows x 96 (75 real) E rows
FN_CONV_SLAB, FN_UP_SLAB, FN_HEAD_SLAB = 32 * 1024, 32 * 80 + 16, 3 * 1024     # floats per workgroup (FnBwdCfg)


@lru_cache(maxsize=None)
def fn_bwd_tables(channel: int, nb: int) -> np.ndarray:
    """The backward blob of Result_Model(4, channel, nb, 3) as one index vector into fn_tables' canonical source: `blob = src[pack]`.
      conv j at j * FN_BWD_CONV_ELEMS: rm_conv_frags' layout (rm_block_index, transposed) of the backward-data operand
             Wt[ci][co][tap] = W[co][ci][8 - tap], rows and columns >= C zero;
      up     at (2 nb + 1) * FN_BWD_CONV_ELEMS: 2 x 3 fragments (m, s) of the 16 x 16 x 32 MFMA, lane l, element j =
             shuf.0.weight[c = 16 m + (l & 15)][r = 32 s + 8 (l >> 4) + j], r = 25 o + 5 ky + kx < 75 (mv_recon_tables' wlb)."""
    layout, _ = fn_tables(channel, nb)
    C, zero, per = channel, layout["zero"], layout["per"]
    rel = rm_block_index(FN_C, C, C, 3, True)
    pack = [np.where(rel < C * C * 9, j * per + rel, zero) for j in range(2 * nb + 1)]
    fr = np.arange(6).reshape(-1, 1, 1)
    lane = np.arange(LANES).reshape(1, -1, 1)
    j = np.arange(8).reshape(1, 1, -1)
    fr, lane, j = np.broadcast_arrays(fr, lane, j)
    c, r = 16 * (fr // 3) + (lane & 15), 32 * (fr % 3) + 8 * (lane >> 4) + j
    pack.append(np.where((r < 75) & (c < C), layout["up_w"] + np.minimum(c, C - 1) * 75 + np.minimum(r, 74), zero).reshape(-1))
    pack = np.concatenate([p.astype(np.int64) for p in pack])
    assert pack.size == (2 * nb + 1) * FN_BWD_CONV_ELEMS + FN_BWD_UP_ELEMS
    return pack


def fn_bwd_parts(nb: int, wgs: int) -> int:
    """floats of sr_fn_net_bwd's workgroup slabs"""
    return wgs * ((2 * nb + 1) * FN_CONV_SLAB + FN_UP_SLAB + FN_HEAD_SLAB)


def fn_grad_sizes(channel: int, nb: int):
    """element counts of sr_fn_net_bwd's grads vector, in its order: (w, b) per conv, the upsampler's (w, b), the encoder's (w, b)"""
    C = channel
    return [C * C * 9, C] * (2 * nb + 1) + [C * 75, 3, C * 27, C]


# =====================================================================================
# multi-frame video network (models/naive_multi_model_easy.py, csrc/multi_frame.h): block 0 reads cat(flow 2 | warp C | e C), blocks
# 1.. are C -> C, decode is a 3x3 conv C -> 48; activations as above
# =====================================================================================
MF_KF = 5                                                  # k-steps of block 0's flow group (9 taps x 8 elements, 2 live)
MF_C1_ELEMS = (2 * 18 + MF_KF) * 512 + 32                  # block 0 conv1: e group, warp group, flow group, 32 biases
MF_FIRST_ELEMS = MF_C1_ELEMS + FN_CONV_ELEMS
MF_DEC_ELEMS = 2 * 18 * 512 + 64
MF_ENCODER, MF_FIRST, MF_BLOCKS, MF_TAIL, MF_ALL = 1, 2, 4, 8, 15


@lru_cache(maxsize=None)
def mf_tables(channel: int, nb: int):
    """(layout, offsets) of the packed blob of Naive_model(4, status = nb blocks of [C, C, 3]): `blob = src[layout["pack"]]` with the
    canonical source `src = cat(w1_0 (C,2C+2,3,3), b1_0 (C), w2_0 (C,C,3,3), b2_0 (C), [w1_i, b1_i, w2_i, b2_i for blocks 1..],
    decode weight (48,C,3,3), decode bias (48), [0])`, the decode weight EFFECTIVE (weight-normed).  offsets[i] = element offset of
    block i (its second conv right behind the first), offsets[nb] = the decode conv's.
      block 0 conv1   K in three groups, walked one after the other by mf_first_kernel: e (input channels 2 + C + ci), warp (2 + ci), each
                      18 fragments laid out as an fn conv (kk = 16 s + 8 (l >> 5) + j, tap = kk // 32, ci = kk % 32), then flow: 5
                      fragments, lane l, element j of fragment s = W[row l & 31][input channel j < 2][tap 2 s + (l >> 5) < 9]; then
                      the 32 biases.  (The order is (group, tap, ci): the kernel keeps conv1's accumulators in registers across groups.)
      other convs     fn_tables' conv layout
      decode          2 row tiles x 18 fragments (rows 32 t + (l & 31) < 48), then 64 biases (48 live)"""
    if not 1 <= channel <= FN_C or nb < 1:
        raise ValueError(f"mf_tables: {channel} channels, {nb} blocks (1 <= channel <= 32, blocks >= 1)")
    C, cin0 = channel, 2 * channel + 2
    w1_0 = 0
    b1_0 = w1_0 + C * cin0 * 9
    w2_0 = b1_0 + C
    per = C * C * 9 + C
    rest = w2_0 + per                                      # blocks 1..: conv j (j = 0: block 1 conv1) at rest + j * per
    dec_w = rest + 2 * (nb - 1) * per
    dec_b = dec_w + 48 * C * 9
    zero = dec_b + 48
    d = rm_conv_index(FN_C, FN_C, 3)
    row, c, tap = d // 9 // FN_C, d // 9 % FN_C, d % 9
    live = (d < FN_C * FN_C * 9) & (row < C) & (c < C)
    rowc, cc = np.minimum(row, C - 1), np.minimum(c, C - 1)
    ch = np.arange(FN_C)
    bias = lambda at: np.where(ch < C, at + np.minimum(ch, C - 1), zero)
    pack = [np.where(live, w1_0 + (rowc * cin0 + 2 + C + cc) * 9 + tap, zero),          # e
            np.where(live, w1_0 + (rowc * cin0 + 2 + cc) * 9 + tap, zero)]              # warp
    s, lane, j = np.meshgrid(np.arange(MF_KF), np.arange(LANES), np.arange(8), indexing="ij")
    frow, ftap = lane & 31, 2 * s + (lane >> 5)
    flive = (frow < C) & (j < 2) & (ftap < 9)
    pack.append(np.where(flive, w1_0 + (np.minimum(frow, C - 1) * cin0 + np.minimum(j, 1)) * 9 + np.minimum(ftap, 8), zero).reshape(-1))
    pack.append(bias(b1_0))
    conv = lambda at: [np.where(live, at + (rowc * C + cc) * 9 + tap, zero), bias(at + C * C * 9)]
    pack += conv(w2_0)
    for jj in range(2 * (nb - 1)):
        pack += conv(rest + jj * per)
    dd = rm_conv_index(48, FN_C, 3)
    drow, dc, dtap = dd // 9 // FN_C, dd // 9 % FN_C, dd % 9
    dlive = (dd < 48 * FN_C * 9) & (dc < C)
    pack.append(np.where(dlive, dec_w + (np.minimum(drow, 47) * C + np.minimum(dc, C - 1)) * 9 + dtap, zero))
    ch64 = np.arange(64)
    pack.append(np.where(ch64 < 48, dec_b + np.minimum(ch64, 47), zero))
    pack = np.concatenate([p.astype(np.int64) for p in pack])
    offsets = [0] + [MF_FIRST_ELEMS + 2 * FN_CONV_ELEMS * i for i in range(nb)]
    assert pack.size == offsets[-1] + MF_DEC_ELEMS
    return dict(pack=pack, size=zero + 1, zero=zero, w1_0=w1_0, b1_0=b1_0, w2_0=w2_0, per=per, rest=rest, dec_w=dec_w, dec_b=dec_b), offsets


MF_BWD_TAIL, MF_BWD_BLOCKS, MF_BWD_FIRST, MF_BWD_WARP, MF_BWD_ENCODER, MF_BWD_ALL = 1, 2, 4, 8, 16, 31
MF_BWD_DEC_ELEMS = 27 * 512               # decode's backward-data operand: 32 rows x (9 taps x 48 gradient channels)


def mf_bwd_offsets(nb: int):
    """element offsets in the backward blob: (block i's conv1 -- block 0: its e group, the warp group and conv2 right behind it --
    for i < nb, then the decode conv's)"""
    return [0] + [(3 + 2 * (i - 1)) * FN_BWD_CONV_ELEMS for i in range(1, nb)] + [(2 * nb + 1) * FN_BWD_CONV_ELEMS]


@lru_cache(maxsize=None)
def mf_bwd_tables(channel: int, nb: int) -> np.ndarray:
    """The backward blob of Naive_model(4, status = nb blocks of [C, C, 3]) as one index vector into mf_tables' canonical source:
    `blob = src[pack]`.  Every conv is rm_conv_kernel's fragment layout (rm_conv_index) of the backward-data operand
    Wt[ci][co][tap] = W[co][ci][8 - tap], rows and columns >= C zero:
      block 0   [e group: ci = input channel 2 + C + ci][warp group: 2 + ci][conv2], 18 fragments each (the flow group has no
                backward-data operand: no flow gradient is produced)
      blocks 1..  [conv1][conv2]
      decode    27 fragments, 32 rows (feature channels) x k = tap * 48 + gradient channel (48 -> 32)"""
    layout, _ = mf_tables(channel, nb)
    C, cin0, zero, per = channel, 2 * channel + 2, layout["zero"], layout["per"]
    d = rm_conv_index(FN_C, FN_C, 3)
    row, c, tap = d // 9 // FN_C, d // 9 % FN_C, d % 9           # Wt's row = the forward's input channel, column = its output channel
    live = (d < FN_C * FN_C * 9) & (row < C) & (c < C)
    rowc, cc = np.minimum(row, C - 1), np.minimum(c, C - 1)
    group = lambda goff: np.where(live, layout["w1_0"] + (cc * cin0 + goff + rowc) * 9 + (8 - tap), zero)
    conv = lambda at: np.where(live, at + (cc * C + rowc) * 9 + (8 - tap), zero)
    pack = [group(2 + C), group(2), conv(layout["w2_0"])]
    for jj in range(2 * (nb - 1)):
        pack.append(conv(layout["rest"] + jj * per))
    dd = rm_conv_index(FN_C, 48, 3)
    drow, dc, dtap = dd // 9 // 48, dd // 9 % 48, dd % 9
    dlive = (dd < FN_C * 48 * 9) & (drow < C)
    pack.append(np.where(dlive, layout["dec_w"] + (dc * C + np.minimum(drow, C - 1)) * 9 + (8 - dtap), zero))
    pack = np.concatenate([p.astype(np.int64) for p in pack])
    assert pack.size == mf_bwd_offsets(nb)[-1] + MF_BWD_DEC_ELEMS
    return pack


def mf_bwd_parts(nb: int, wgs: int) -> int:
    """floats of sr_mf_net_bwd's workgroup slabs: 2 nb + 3 conv slabs (2 i: block i's conv1 -- block 0: the e group --, 2 i + 1: its
    conv2, 2 nb: block 0's warp group, 2 nb + 1: its flow group, 2 nb + 2: decode) and the encoder's"""
    return wgs * ((2 * nb + 3) * FN_CONV_SLAB + FN_HEAD_SLAB)


def mf_grad_sizes(channel: int, nb: int):
    """element counts of sr_mf_net_bwd's grads vector, in its order (mf_tables' canonical source, then the encoder): per block
    (w1, b1, w2, b2), decode (w, b), encoder (w, b)"""
    C = channel
    return [C * (2 * C + 2) * 9, C, C * C * 9, C] + [C * C * 9, C] * (2 * (nb - 1)) + [48 * C * 9, 48, C * 27, C]


@lru_cache(maxsize=None)
def clip_step_layout(net: str, channel: int, nb: int):
    """The fp32 source vector of the video networks' one-call training step (sr_fn_net_train_step: net "fn", sr_mf_net_train_step: "mf"):
    the network's canonical source (fn_tables / mf_tables: every effective tensor but the encoder's, then [0]) followed by the encoder's
    effective weight (C, 3, 3, 3), its bias (C) and [1].  The pieces of the flat gradient vector (fn_grad_sizes / mf_grad_sizes) lie in the
    same order, so piece i of the gradient is piece i of the source; the two constants sit between and behind them.
      size, zero, one          length of the source and where its two constants are
      sizes, grad_off, src_off per piece of the gradient vector: elements, offset in the gradient vector, offset in the source
      head                     the encoder's head blob (sr_head_fwd at 32 rows: ends_tables(32, 4)["head"] over wh (32,3,3,3) | bh (32) |
                               0 | 1) as an index vector into THIS source, rows >= C reading the zero"""
    layout, _ = fn_tables(channel, nb) if net == "fn" else mf_tables(channel, nb)
    sizes = fn_grad_sizes(channel, nb) if net == "fn" else mf_grad_sizes(channel, nb)
    C, zero = channel, layout["zero"]
    grad_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    assert grad_off[-2] == zero, (grad_off[-2], zero)                # the encoder's pieces are the last two
    src_off = grad_off.copy()
    src_off[-2:] += 1
    enc_w, enc_b = int(src_off[-2]), int(src_off[-1])
    one = enc_b + C
    h = np.asarray(ends_tables(FN_C, 4)["head"]).astype(np.int64)
    nw = FN_C * 27
    row, k, ch = np.minimum(h, nw - 1) // 27, np.minimum(h, nw - 1) % 27, np.clip(h - nw, 0, FN_C - 1)
    head = np.where(h < nw, np.where(row < C, enc_w + np.minimum(row, C - 1) * 27 + k, zero),
                    np.where(h < nw + FN_C, np.where(ch < C, enc_b + np.minimum(ch, C - 1), zero), np.where(h == nw + FN_C, zero, one)))
    assert h.max() <= nw + FN_C + 1
    head = head.astype(np.int64)
    head.setflags(write=False)
    return dict(size=one + 1, zero=zero, one=one, sizes=list(sizes), grad_off=[int(v) for v in grad_off], src_off=[int(v) for v in src_off],
                head=head)


@lru_cache(maxsize=None)
def mf_grad_sources(channel: int, nb: int):
    """(slab, offset) per element of the grads vector: the element is the sum over workgroups of float `offset` of slab number `slab`
    (mf_bwd_parts' numbering; 2 nb + 3: the encoder's).  Conv slabs hold 32 x 32 accumulator tiles (_acc_pos): tile = tap, tile 9 = the
    bias (column 0); decode: tile 10 (co // 32) + tap; block 0's conv1 draws input channels 0, 1 from the flow group's slab, 2 .. C + 1
    from the warp group's and C + 2 .. 2 C + 1 from the e group's (cat(flow, warp, e)), its bias from the e group's; the encoder
    (sr_head_wgrad's slab): tile ky, column 4 kx + ci, bias at tile 1, column 7."""
    C, cin0 = channel, 2 * channel + 2
    slabs, offs = [], []

    def add(slab, off):
        off = np.asarray(off).reshape(-1)
        slabs.append(np.broadcast_to(np.asarray(slab), off.shape).reshape(-1) if np.ndim(slab) == 0 else np.asarray(slab).reshape(-1))
        offs.append(off)

    co, cin, tap = np.meshgrid(np.arange(C), np.arange(cin0), np.arange(9), indexing="ij")
    ci = np.where(cin < 2, cin, np.where(cin < 2 + C, cin - 2, cin - 2 - C))
    add(np.where(cin < 2, 2 * nb + 1, np.where(cin < 2 + C, 2 * nb, 0)), _acc_pos(tap, co, ci))
    add(0, _acc_pos(np.full(C, 9), np.arange(C), np.zeros(C, dtype=np.int64)))
    co, ci, tap = np.meshgrid(np.arange(C), np.arange(C), np.arange(9), indexing="ij")
    for j in range(1, 2 * nb):
        add(j, _acc_pos(tap, co, ci))
        add(j, _acc_pos(np.full(C, 9), np.arange(C), np.zeros(C, dtype=np.int64)))
    co, ci, tap = np.meshgrid(np.arange(48), np.arange(C), np.arange(9), indexing="ij")
    add(2 * nb + 2, _acc_pos((co // 32) * 10 + tap, co % 32, ci))
    co = np.arange(48)
    add(2 * nb + 2, _acc_pos((co // 32) * 10 + 9, co % 32, np.zeros(48, dtype=np.int64)))
    co, ci, ky, kx = np.meshgrid(np.arange(C), np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    add(2 * nb + 3, _acc_pos(ky, co, 4 * kx + ci))
    add(2 * nb + 3, _acc_pos(np.ones(C, dtype=np.int64), np.arange(C), np.full(C, 7)))
    return np.concatenate(slabs).astype(np.int64), np.concatenate(offs).astype(np.int64)
