"""The 8-wave weight-gradient kernels of the 24-unit bf16 path (csrc/wdsr_wgrad_rs.h: wdsr_wgrad_a8_kernel -- dW1, db1, dW2, db2 --
and wdsr_wgrad_b8_kernel -- dW3, db3) through sr_wdsr_block_wgrad_saved, at the smallest shapes that reach each piece of their
staging index logic:

  1 x 12x24, 1 layer, 1 workgroup     one full tile of 288 pixels: two a8 chunks, the second partial (288 = 256 + 32)
  3 x 13x25, 2 layers, 2 workgroups   partial tiles in both axes (zero-filled outside the image); a8 chunks straddle a tile and
                                      roll from the last tile of an image into the next image; layer strides; 12 tiles for 2
                                      workgroups in b8, 14 chunks in a8
  2 x 24x48, 1 layer, 16 workgroups   8 tiles / 9 chunks: b8 workgroups without a tile, a8 workgroups with one chunk and no
                                      second buffer
  3 x 13x25, 1 layer, 5 workgroups    14 chunks and 12 tiles, neither a multiple of 5

The inputs are random normal (tests/block_ref.py's rounded cases); the saved t and dt images are the emulation's, i.e. what the
forward and backward-data kernels hand over, rounded where they round.  The reduced gradients are compared with the float64
reference in the metric and with the bound of tests/test_gpu_block_ref.py's rounded cases: max |got - ref| / max |ref| within
4 x the same metric of block_ref.emulate().  Partial buffers are pre-filled with NaN, so an unwritten gathered entry shows.
"""
import pytest
import torch

from tests import block_ref as R
from tests.parity_kit import bound

pytestmark = pytest.mark.gpu

F = 24
BF = torch.bfloat16
NAN = float("nan")
BLOCKS = "ab"                                               # layer i of a call is block BLOCKS[i] of the rounded case
GAP = 40                                                    # elements between two layers' tensors (filled with NaN)
CASES = ((1, 12, 24, 1, 1), (3, 13, 25, 2, 2), (2, 24, 48, 1, 16), (3, 13, 25, 1, 5))
_cid = lambda c: "%dx%dx%d-layers%d-wgs%d" % c


def _p(t):
    return t.data_ptr()


def _layered(tensors, gap, dtype):
    """[layers] tensors -> one NaN-filled buffer with `gap` elements between them: (buffer, layer stride in elements)"""
    stride = tensors[0].numel() + gap
    buf = torch.full((len(tensors), stride), NAN, device="cuda", dtype=dtype)
    for i, t in enumerate(tensors):
        buf[i, :t.numel()] = t.reshape(-1).to(device="cuda", dtype=dtype)
    return buf, stride


def _inputs(n, h, w, layers):
    from mobilesuperresolution_amd import hotpath as HP
    case, emu, ref, yard = R.rounded_reference(F, n, h, w, "bf16")
    l, lp = R.DIMS[F][2], R.lp_of(F)
    src = torch.stack([R.block_vec(case["pa"]), R.block_vec(case["pb"])]).cuda()
    blob, cinit = HP.pack_blocks(src, F, BF)
    blk = BLOCKS[:layers]
    xs = [R.nhwc(case["x" if b == "a" else "xb"]) for b in blk]
    dys = [R.nhwc(case["dy" + b]) for b in blk]
    ts = [R.tile_image(emu[b]["t"], lp, ones_at=l) for b in blk]
    dts = [R.tile_image(emu[b]["dt"], lp) for b in blk]
    idx = [BLOCKS.index(b) for b in blk]
    bufs = dict(x=_layered(xs, GAP, BF), dy=_layered(dys, GAP, BF), t=_layered(ts, 8 * GAP, BF), dt=_layered(dts, 8 * GAP, BF),
                blob=_layered([blob[k] for k in idx], 8 * GAP, BF), cinit=_layered([cinit[k] for k in idx], GAP, torch.float32))
    return bufs, HP.tables(F, src.device), ref, yard


def _call(bufs, tb, n, h, w, layers, wgs, fill):
    from mobilesuperresolution_amd import _lib as L
    pa = torch.full((layers, wgs, tb["slab_a"]), fill, device="cuda")
    pb = torch.full((layers, wgs, tb["slab_b"]), fill, device="cuda")
    assert bufs["t"][1] == bufs["dt"][1]
    L.check(L.lib().sr_wdsr_block_wgrad_saved(_p(bufs["x"][0]), _p(bufs["dy"][0]), _p(bufs["t"][0]), _p(bufs["dt"][0]), _p(bufs["blob"][0]),
                                              _p(bufs["cinit"][0]), _p(pa), _p(pb), layers, wgs, n, h, w, F, L.DTYPE_CODE[BF], bufs["x"][1],
                                              bufs["dy"][1], bufs["t"][1], bufs["blob"][1], bufs["cinit"][1], L.stream_ptr()),
            "sr_wdsr_block_wgrad_saved")
    torch.cuda.synchronize()
    return pa, pb


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_reduced_gradients_against_float64(case):
    n, h, w, layers, wgs = case
    bufs, tb, ref, yard = _inputs(n, h, w, layers)
    pa, pb = _call(bufs, tb, n, h, w, layers, wgs, NAN)
    vec = torch.cat([pa.sum(1), pb.sum(1)], dim=1).index_select(1, tb["grad"]).cpu()
    bad = []
    for i in range(layers):
        b = BLOCKS[i]
        s = R.split_vec(torch.cat([vec[i], torch.zeros(2)]), F)
        for k in R.GRADS:
            e_ref = yard[b][k]
            err = R.rel_max(s[k].float(), ref[b][k])
            tol = bound("bf16", e_ref)
            print(f"wgrad8 | {_cid(case)} | layer {i} (block {b}) {k} | yardstick {e_ref:.2e} | kernel {err:.2e} | bound {tol:.2e}")
            if not err <= tol:
                bad.append((i, k, err, tol))
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", CASES[1:3], ids=_cid)
def test_partial_buffers_are_deterministic(case):
    """two calls on the same inputs: the partial slabs -- every workgroup's, idle ones included -- are equal bit for bit"""
    n, h, w, layers, wgs = case
    bufs, tb, _, _ = _inputs(n, h, w, layers)
    pa1, pb1 = _call(bufs, tb, n, h, w, layers, wgs, 0.0)
    pa2, pb2 = _call(bufs, tb, n, h, w, layers, wgs, 0.0)
    assert torch.equal(pa1, pa2) and torch.equal(pb1, pb2)
