"""CPU checks of the opt-in training route of the 64-wide propagation trunks (no GPU): packing.c64_bwd_tables' backward blob run
through the lane-level model of c64_conv_kernel against F.conv_transpose2d, the weight-gradient slab -> flat-gradient tables
against slabs laid out as csrc/conv64_bwd.h writes them, and the route rule."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mobilesuperresolution_amd import packing as P
from mobilesuperresolution_amd import models
from mobilesuperresolution_amd.models import ConvResidualBlocks
from mobilesuperresolution_amd.models import basicvsr_arch as A
from tests import mfma_emu as E

CONVS = [(64, 64), (67, 64), (43, 40), (40, 40)]


def _emu_conv64(blob, x_k):
    """c64_conv_kernel at 64 kernel inputs on one image of at most one 16 x 16 tile, lane by lane (the fragment layout of
    tests/mfma_emu.py; tests/test_trunk64_layout.py holds the forward tables the same way): x_k (H, W, 64) -> (H, W, 64)"""
    H, W, _ = x_k.shape
    assert H <= 16 and W <= 16
    tile = np.zeros((34, 34, 64))
    tile[1:H + 1, 1:W + 1] = x_k
    bias = np.asarray(blob[72 * 512:72 * 512 + 64], dtype=np.float64)
    y = np.zeros((H, W, 64))
    for pt in range(8):
        pc = pt * 32 + E.R
        oy, ox = pc // 16, pc % 16
        if oy.min() >= H:
            continue
        for ch in range(2):
            acc = np.stack([bias[32 * ch + (i & 3) + 8 * (i >> 2) + 4 * E.HH] for i in range(16)], 1)
            for s in range(36):
                tap, c = s // 4, s % 4
                b = np.stack([tile[oy + tap // 3, ox + tap % 3, 16 * c + 8 * E.HH + j] for j in range(8)], 1)
                acc = E.mma16(E.wfrag(blob, ch * 36 + s), b, acc)
            for i in range(16):
                co = 32 * ch + (i & 3) + 8 * (i >> 2) + 4 * E.HH
                ok = (oy < H) & (ox < W)
                y[oy[ok], ox[ok], co[ok]] = acc[ok, i]
    return y


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).double()


@pytest.mark.parametrize("cin,f", CONVS, ids=lambda v: str(v))
def test_backward_blob_is_conv_transpose(cin, f):
    """integer data, so every sum is exact in float64 whatever its order: the conv the blob describes IS conv_transpose2d"""
    g = torch.Generator().manual_seed(cin * 100 + f)
    H, W = 5, 7
    wt, bt, dz = _ints(g, f, cin, 3, 3), _ints(g, f), _ints(g, 1, f, H, W)
    t = P.c64_bwd_tables(cin, f)
    assert t["halves"] == (2 if cin == f + 3 else 1) and len(t["w"]) == t["halves"] * P.C64_BWD_CONV_ELEMS
    blob = np.concatenate([wt.numpy().reshape(-1), bt.numpy(), [0.0]])[t["w"]]
    assert np.all(blob.reshape(t["halves"], -1)[:, 72 * 512:] == 0.0)          # zero bias
    dz_k = np.zeros((H, W, 64))
    dz_k[..., :f] = dz[0].permute(1, 2, 0).numpy()
    ref = F.conv_transpose2d(dz, wt, padding=1)[0].permute(1, 2, 0).numpy()    # (H, W, cin)
    y0 = _emu_conv64(blob[:P.C64_BWD_CONV_ELEMS], dz_k)
    if cin == f + 3:
        y1 = _emu_conv64(blob[P.C64_BWD_CONV_ELEMS:], dz_k)
        assert np.array_equal(y0[..., :f], ref[..., 3:]) and np.array_equal(y1[..., :3], ref[..., :3])
        assert np.all(y1[..., 3:] == 0.0)
    else:
        assert np.array_equal(y0[..., :f], ref)
    assert np.all(y0[..., f:] == 0.0)                                          # padded rows: exactly zero


def _slab_of(dw, db, cin, f):
    """one workgroup's slab as c64_wgrad_kernel writes it, from a given (dW, db): tile u NT + 2 cb + ob = the accumulator of tap
    8 - u, rows = kernel input channels 32 cb .., columns = output channels 32 ob ..; register i of lane (r, hh) = element
    (row (i & 3) + 8 (i >> 2) + 4 hh, column r) (csrc/sr_common.h); [tile][reg][lane].  Unwritten entries are NaN."""
    ci_k = P.c64_ci_kernel(cin, f)
    nt, ncb = (6, 3) if ci_k == 80 else (4, 2)
    mats = np.zeros((9, 32 * ncb, 64))                        # [u][kernel ci][co]
    for ci in range(cin):
        kc = (64 + ci if ci < 3 else ci - 3) if ci_k == 80 else ci
        mats[:, kc, :f] = dw[:, ci].reshape(f, 9).T[::-1]     # u = 8 - tap
    if ci_k == 80:
        mats[4, 80, :f] = db                                  # the ones channel at the centre tap
    slab = np.full(P.c64_wgrad_slab(ci_k), np.nan)
    lane = np.arange(64)
    r, hh = lane & 31, lane >> 5

    def put(tile, m):                                         # m: 32 x 32 accumulator
        for i in range(16):
            slab[(tile * 16 + i) * 64 + lane] = m[(i & 3) + 8 * (i >> 2) + 4 * hh, r]
    for u in range(9):
        for cb in range(ncb):
            for ob in range(2):
                put(u * nt + 2 * cb + ob, mats[u, 32 * cb:32 * cb + 32, 32 * ob:32 * ob + 32])
    if ci_k == 64:
        for ob in range(2):
            m = np.zeros((32, 32))
            m[0, :] = np.concatenate([db, np.zeros(64 - f)])[32 * ob:32 * ob + 32]
            put(36 + ob, m)
    return slab


@pytest.mark.parametrize("cin,f", CONVS, ids=lambda v: str(v))
def test_gradient_tables_pick_each_real_entry_once(cin, f):
    nb = 1
    t = P.c64_trunk_bwd_tables(cin, f, nb)
    n0, n1 = f * cin * 9 + f, f * f * 9 + f
    assert (t["n0"], t["n1"]) == (n0, n1) and t["slab0"] == P.c64_wgrad_slab(t["ci_k"]) and t["slab1"] == P.c64_wgrad_slab(64)
    assert len(t["boff"]) == 2 + 2 * nb and (t["boff"][-1] >= 0) == (cin == f + 3)
    g = torch.Generator().manual_seed(7)
    for (sidx, dst), ci, n, slab_n in ((t["unpack"][:2], cin, n0, t["slab0"]), (t["unpack"][2:], f, n1, t["slab1"])):
        assert sidx.dtype == dst.dtype == np.int32 and len(sidx) == len(dst) == n
        assert np.array_equal(np.sort(dst), np.arange(n))                       # every real element exactly once
        assert len(np.unique(sidx)) == n and sidx.min() >= 0 and sidx.max() < slab_n and np.all(np.diff(sidx) > 0)
        dw, db = torch.randn(f, ci, 3, 3, generator=g, dtype=torch.float64).numpy(), torch.randn(f, generator=g, dtype=torch.float64).numpy()
        slab = _slab_of(dw, db, ci, f)
        flat = np.empty(n)
        flat[dst] = slab[sidx]                                                  # the reduction of one slab
        assert np.array_equal(flat[:n - f].reshape(f, ci, 3, 3), dw)            # NaN anywhere = an unwritten or padded entry
        assert np.array_equal(flat[n - f:], db)                                 # db lands on the bias entries
        idx = np.arange(slab_n, dtype=np.float64)                               # a slab filled with its own indices
        flat[dst] = idx[sidx]
        assert len(np.unique(flat)) == n and np.array_equal(flat, P.c64_bwd_tables(ci, f)["grad"])    # one entry each, its own


def test_no_padded_row_or_column_of_the_embed_is_referenced():
    cin, f = 43, 40
    t = P.c64_bwd_tables(cin, f)
    pos = t["grad"]
    tile, rem = pos // 1024, pos % 1024
    i, lane = rem // 64, rem % 64
    row, col = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5), lane & 31
    u, q = tile // 6, tile % 6
    kc, co = 32 * (q // 2) + row, 32 * (q % 2) + col
    assert np.all(co < f)
    assert np.all((kc < f) | ((kc >= 64) & (kc < 67)) | ((kc == 80) & (u == 4)))
    pack = P.c64_trunk_bwd_tables(cin, f, 2)["pack"]
    total = (f * cin * 9 + f) + 4 * (f * f * 9 + f)
    used = np.zeros(total + 1, dtype=bool)
    used[pack] = True
    w_only = np.ones(total, dtype=bool)                                         # biases are not part of a backward blob
    off = 0
    for k in range(5):
        nw = f * (cin if k == 0 else f) * 9
        w_only[off + nw:off + nw + f] = False
        off += nw + f
    assert np.array_equal(used[:total], w_only)


def test_route_rule_and_helper():
    wide, narrow = ConvResidualBlocks(67, 64, 1), ConvResidualBlocks(27, 24, 1)
    assert ConvResidualBlocks.hot_training is False and wide.hot_training is False and "hot_training" not in wide.__dict__
    holder = nn.ModuleDict({"a": wide, "b": narrow, "c": nn.Sequential(ConvResidualBlocks(40, 40, 0))})
    got = models.set_wide_training(holder)
    assert models.set_wide_training is A.set_wide_training and "set_wide_training" in models.__all__
    assert got == [wide, holder["c"][0]] and wide.hot_training is True and holder["c"][0].hot_training is True
    assert "hot_training" not in narrow.__dict__                                # only wide trunks are touched
    models.set_wide_training(holder, False)
    assert wide.hot_training is False
    assert "no_grad" in A._NO_GRAPH_MSG and "hot_training" in A._NO_GRAPH_MSG
    x = torch.zeros(1, 67, 4, 4)                                                # the rule itself needs no GPU
    with pytest.raises(NotImplementedError, match="no_grad"):
        A._wide_route((wide,), True, x)
    wide.hot_training = True
    assert A._wide_route((wide,), True, x) is True
    with pytest.raises(NotImplementedError, match="no_grad"):                   # a pair needs both
        A._wide_route((wide, ConvResidualBlocks(67, 64, 1)), True, x)
    with torch.no_grad():
        assert A._wide_route((wide,), True, x) is False
    assert A.WGRAD64_WGS >= 1 and A._wgrad64_wgs(3, 32, 32) == min(12, A.WGRAD64_WGS)


def test_wgrad_workgroups_follow_the_module_constant(monkeypatch):
    monkeypatch.setattr(A, "WGRAD64_WGS", 5)
    assert A._wgrad64_wgs(3, 32, 32) == 4                                       # 12 tiles, 3 per workgroup
    monkeypatch.setattr(A, "WGRAD64_WGS", 1)
    assert A._wgrad64_wgs(3, 32, 32) == 1 and A._wgrad64_wgs(6, 32, 32, 3) == 2    # paired: clamped to one per trunk
    monkeypatch.setattr(A, "WGRAD64_WGS", 13)
    assert A._wgrad64_wgs(3, 32, 32) == 12
