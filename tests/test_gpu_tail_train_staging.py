"""sr_tail_train's staging (csrc/wdsr_ends.h sr_tail_train_kernel: feat staged once on its 2-px halo, x - mean once on its
3-px halo, the backward phases reading their narrower windows as views into those images; one weight staging burst and no
tile loop when every workgroup has at most one tile) against sr_tail_fwd + sr_tail_bwd_loss through the C ABI, bit for bit:
dfeat, the reduced tail slabs and loss_part, no element left out.

Shapes are the smallest at which the addressing can go wrong: one tile whose halo is all outside the image, interior tile
seams in both directions, ragged right and bottom tiles, and both launch forms -- every workgroup with at most one tile
(N tiles <= workgroups, idle workgroups included) and the tile loop (N tiles > workgroups: all tiles on one workgroup, an
uneven share, 2 wgs + 1 tiles), where the forward's weights are staged again per tile.

Inputs are seeded and bf16-representable, so every product of the forward is exact in fp32 and the SR image of the kernels
differs from the float64 oracle (tests/ends_ref.py tail_ref) only by fp32 accumulation, at most K 2^-24 sum |terms|.  hr is
the oracle's SR image moved by 0.05 .. 0.5 either way: the CPU check below holds that bound under a quarter of the smallest
|sr - hr|, so no sr - hr of the kernels is zero or changes sign between the two paths' (identical) forwards -- the L1 sign is
discontinuous there, and such a tie would make the comparison depend on nothing this file is about."""
import functools

import pytest
import torch

from tests import ends_ref as R

TH, TW = 12, 24                                                # the tail kernels' LR tile (EndsCfg::TH, TW)

# (N, H, W, workgroups)
_ONE_TILE_PER_WG = [
    (1, TH, TW, 1),                                            # one tile exactly: every side is an image edge
    (1, TH, TW, 3),                                            # ... and two workgroups without a tile
    (1, 2 * TH, 2 * TW, 4),                                    # 2 x 2 tiles: seams in both directions
    (1, TH + 5, TW + 7, 4),                                    # partial right and bottom tiles
    (2, TH + 5, TW + 7, 8),                                    # ... second image of a batch
]
_TILE_LOOP = [
    (1, 2 * TH, 2 * TW, 1),                                    # all four tiles on one workgroup
    (1, TH + 5, TW + 7, 3),                                    # partial tiles, uneven share
    (5, TH, TW, 2),                                            # N tiles = 2 wgs + 1
]
_GRID = _ONE_TILE_PER_WG + _TILE_LOOP


def _bf16_exact(t):
    return t.bfloat16().float()


@functools.lru_cache(maxsize=None)
def _inputs(f, n, h, w):
    """CPU tensors: src_tail (tail_src order), feat (n, h, w, f), x, hr -- and the CPU check that no sr - hr is near zero"""
    g = torch.Generator().manual_seed(9000 + 131 * f + 17 * n + 3 * h + w)
    co = 48
    src = _bf16_exact(torch.randn(co * f * 9 + co * 75 + co + 2, generator=g) * 0.05)
    src[-2], src[-1] = 0.0, 1.0
    feat = _bf16_exact(torch.randn(n, h, w, f, generator=g))
    x = torch.randint(0, 65, (n, 3, h, w), generator=g).float() / 64          # x - 0.5 is a multiple of 1/64: bf16-exact
    assert torch.equal(_bf16_exact(x - R.MEAN), x - R.MEAN)
    v = R.split_tail_vec(src.double(), f, 4)
    sr = R.tail_ref(feat.double(), x.double(), v["dwt"], v["dws"], v["dbtot"], R.MEAN, 4)
    mag = R.tail_ref(feat.double().abs(), (x.double() - R.MEAN).abs() + R.MEAN, v["dwt"].abs(), v["dws"].abs(), v["dbtot"].abs(), R.MEAN, 4)
    off = (0.05 + 0.45 * torch.rand(sr.shape, generator=g).double()) * (torch.randint(0, 2, sr.shape, generator=g) * 2 - 1)
    hr = (sr + off).float()
    # the oracle's check: fp32 accumulation of the K = 9 f + 75 + 1 exact products per value stays far inside |sr - hr|
    bound = float(((9 * f + 76) * 2.0 ** -24 * mag).max())
    gap = float((sr - hr.double()).abs().min())
    assert gap >= 0.04 and bound < gap / 4, (gap, bound)
    return src, feat, x, hr


@pytest.mark.parametrize("f", [24, 32])
def test_seeded_inputs_have_no_tie(f):
    """the CPU half: every shape's inputs pass the oracle's margin check (no GPU needed)"""
    for n, h, w, _ in _GRID:
        _inputs(f, n, h, w)


def _buffers(tb, feat, wgs):
    return (torch.full_like(feat, float("nan")), torch.full((wgs, tb["tail_slab"]), float("nan"), device=feat.device),
            torch.full((wgs,), float("nan"), device=feat.device))


@pytest.mark.gpu
@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n,h,w,wgs", _GRID)
def test_tail_train_staging_bit_identical(n, h, w, wgs, kind, f):
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd import hotpath as HP
    tiles = R.n_tiles(n, h, w)
    assert (tiles <= wgs) == ((n, h, w, wgs) in _ONE_TILE_PER_WG)
    src, feat, x, hr = _inputs(f, n, h, w)
    dev = torch.device("cuda", 0)
    tb = HP.ends_tables(f, 4, dev)
    blob = HP.pack_tail(src.to(dev), f, 4, torch.bfloat16)
    feat, x, hr = feat.to(dev).bfloat16(), x.to(dev), hr.to(dev)
    gscale = 0.7 / hr.numel()
    lib, sp = L.lib(), L.stream_ptr()

    out = torch.full_like(hr, float("nan"))
    L.check(lib.sr_tail_fwd(feat.data_ptr(), x.data_ptr(), out.data_ptr(), blob.data_ptr(), 0.5, n, h, w, f, 4, 1, sp), "sr_tail_fwd")
    d_ref, p_ref, l_ref = _buffers(tb, feat, wgs)
    L.check(lib.sr_tail_bwd_loss(out.data_ptr(), hr.data_ptr(), kind, gscale, l_ref.data_ptr(), feat.data_ptr(), x.data_ptr(), 0.5,
                                 blob.data_ptr(), d_ref.data_ptr(), p_ref.data_ptr(), wgs, n, h, w, f, 4, 1, sp), "sr_tail_bwd_loss")
    d_new, p_new, l_new = _buffers(tb, feat, wgs)
    L.check(lib.sr_tail_train(hr.data_ptr(), kind, gscale, l_new.data_ptr(), feat.data_ptr(), x.data_ptr(), 0.5, blob.data_ptr(),
                              d_new.data_ptr(), p_new.data_ptr(), wgs, n, h, w, f, 4, 1, sp), "sr_tail_train")
    torch.cuda.synchronize()
    assert int((out == hr).sum()) == 0 and torch.isfinite(out).all()
    assert torch.isfinite(d_ref.float()).all() and torch.isfinite(l_ref).all()
    assert torch.equal(d_new, d_ref)
    assert torch.equal(l_new, l_ref), (l_new - l_ref).abs().max().item()
    # the slab columns the network gathers (the others hold products with LDS bytes past an image row and are never read),
    # slab by slab and reduced over the workgroups as the network's gradient vector is formed
    used = tb["tail_grad"]
    s_new, s_ref = p_new.index_select(1, used), p_ref.index_select(1, used)
    assert torch.isfinite(s_ref).all()
    assert torch.equal(s_new, s_ref)
    assert torch.equal(s_new.sum(0), s_ref.sum(0))
    assert s_ref.abs().sum() > 0 and d_ref.float().abs().sum() > 0 and l_ref[:min(wgs, tiles)].min() > 0
