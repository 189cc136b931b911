"""Thin host layer over the C ABI: packs parameters into MFMA fragment blobs (one torch gather per
layer family) and enqueues the HIP kernels on torch's current stream.  No arithmetic of the SR path
happens in PyTorch here; torch is used for device memory, streams and the gather/sum plumbing."""
from __future__ import annotations

import ctypes
from functools import lru_cache
from typing import Tuple

import numpy as np
import torch

from . import _lib as L
from . import packing as P


KernelTimer, set_timer, _launch = L.KernelTimer, L.set_timer, L.launch



@lru_cache(maxsize=None)
def const01(device: torch.device, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """the [0, 1] constant slots of a canonical source vector, uploaded once per device
    (Tensor.new_tensor is a synchronous host-to-device copy: it drains the GPU queue on every call)"""
    return torch.tensor([0.0, 1.0], dtype=dtype, device=device)

def block_dims(F: int) -> Tuple[int, int, int]:
    """(F, E, L) of the reference Block: expand 6, linear 0.84 (models/basic_wdsr_b.py:105-106)."""
    return F, int(F * 6), int(F * 0.84)


@lru_cache(maxsize=None)
def _dev_tables(F: int, device_index: int):
    f, e, l = block_dims(F)
    tab = P.block_tables(f, e, l)
    gt = P.block_grad_tables(f, e, l)
    dev = torch.device("cuda", device_index)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g = tab["geom"]
    o = g.off
    # canonical gradient vector order = w1 | w2 | w3 | b1 | b2 | b3 (src layout without constants)
    E_, L_ = g.E, g.L
    n_w1, n_w2, n_w3 = E_ * f, L_ * E_, f * L_ * 9
    ga, gb = gt["a"], gt["b"]
    # slab A order: w1, w2, b1, b2 ; slab B order: w3, b3  -> positions inside cat(slabA, slabB)
    a_w1, a_w2 = ga[:n_w1], ga[n_w1:n_w1 + n_w2]
    a_b1, a_b2 = ga[n_w1 + n_w2:n_w1 + n_w2 + E_], ga[n_w1 + n_w2 + E_:]
    b_w3, b_b3 = gb[:n_w3] + gt["a_size"], gb[n_w3:] + gt["a_size"]
    grad_idx = np.concatenate([a_w1, a_w2, b_w3, a_b1, a_b2, b_b3])
    assert grad_idx.size == o["zero"]
    return dict(w=t(tab["w"]), cinit=t(tab["cinit"]), grad=t(grad_idx), geom=g, nfrag=tab["nfrag"],
                slab_a=gt["a_size"], slab_b=gt["b_size"], src_size=o["size"])


def tables(F: int, device: torch.device):
    return _dev_tables(F, device.index if device.index is not None else torch.cuda.current_device())


def block_src(w1: torch.Tensor, w2: torch.Tensor, w3: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
              b3: torch.Tensor) -> torch.Tensor:
    """Canonical per-block source vectors [NB, S] from stacked effective weights/biases
    (w1 [NB,E,F], w2 [NB,L,E], w3 [NB,F,L,3,3], b* [NB,...]); differentiable."""
    nb = w1.shape[0]
    const = const01(w1.device, w1.dtype).expand(nb, 2)
    return torch.cat([w1.reshape(nb, -1), w2.reshape(nb, -1), w3.reshape(nb, -1), b1, b2, b3, const], dim=1)


def pack_blocks(src_all: torch.Tensor, F: int, dtype: torch.dtype):
    """src_all [NB, S] fp32 -> (blob [NB, nfrag*512] dtype, cinit [NB, C] fp32)."""
    tb = tables(F, src_all.device)
    assert src_all.shape[1] == tb["src_size"], (src_all.shape, tb["src_size"])
    s = src_all.detach().float()
    blob = s.index_select(1, tb["w"]).to(dtype).contiguous()
    cinit = s.index_select(1, tb["cinit"]).contiguous()
    return blob, cinit


def block_fwd(x: torch.Tensor, y: torch.Tensor, blob_i: torch.Tensor, cinit_i: torch.Tensor):
    n, h, w, f = x.shape
    _launch("sr_wdsr_block_fwd", L.lib().sr_wdsr_block_fwd, L.ptr(x), L.ptr(y), L.ptr(blob_i), L.ptr(cinit_i), n, h, w, f,
                                      L.DTYPE_CODE[x.dtype], L.stream_ptr())


def block_bwd_data(x: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor, blob_i: torch.Tensor,
                   cinit_i: torch.Tensor):
    n, h, w, f = x.shape
    _launch("sr_wdsr_block_bwd_data", L.lib().sr_wdsr_block_bwd_data, L.ptr(x), L.ptr(dy), L.ptr(dx), L.ptr(blob_i), L.ptr(cinit_i),
                                           n, h, w, f, L.DTYPE_CODE[x.dtype], L.stream_ptr())


def block_wgrad(xs: torch.Tensor, dys: torch.Tensor, blob: torch.Tensor, cinit: torch.Tensor,
                wgs_per_layer: int = 16) -> torch.Tensor:
    """xs, dys: [NB, N, H, W, F] (block inputs / output gradients); blob [NB, .], cinit [NB, .].
    Returns d_src [NB, S] (zeros at the two constant slots), fp32."""
    nb, n, h, w, f = xs.shape
    tb = tables(f, xs.device)
    pa = torch.empty((nb, wgs_per_layer, tb["slab_a"]), dtype=torch.float32, device=xs.device)
    pb = torch.empty((nb, wgs_per_layer, tb["slab_b"]), dtype=torch.float32, device=xs.device)
    assert xs.is_contiguous() and dys.is_contiguous() and blob.is_contiguous() and cinit.is_contiguous()
    _launch("sr_wdsr_block_wgrad", L.lib().sr_wdsr_block_wgrad, L.ptr(xs), L.ptr(dys), L.ptr(blob), L.ptr(cinit), L.ptr(pa), L.ptr(pb),
                                        nb, wgs_per_layer, n, h, w, f, L.DTYPE_CODE[xs.dtype],
                                        xs.stride(0), dys.stride(0), blob.stride(0), cinit.stride(0),
                                        L.stream_ptr())
    slab = torch.cat([pa.sum(1), pb.sum(1)], dim=1)
    g = slab.index_select(1, tb["grad"])
    return torch.cat([g, g.new_zeros(nb, 2)], dim=1)


# =====================================================================================
# head / tail (+ skip + PixelShuffle)
# =====================================================================================
@lru_cache(maxsize=None)
def _dev_ends_tables(F: int, R: int, device_index: int):
    tab = P.ends_tables(F, R)
    gt = P.ends_grad_tables(F, R)
    dev = torch.device("cuda", device_index)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g = tab["geom"]
    return dict(head=t(tab["head"]), tail=t(tab["tail"]), head_grad=t(gt["head"]), tail_grad=t(gt["tail"]),
                tail_slab=gt["tail_size"], head_slab=gt["head_size"], geom=g,
                head_size=g.head_off["size"], tail_size=g.tail_off["size"])


def ends_tables(F: int, R: int, device: torch.device):
    return _dev_ends_tables(F, R, device.index if device.index is not None else torch.cuda.current_device())


def head_src(wh: torch.Tensor, bh: torch.Tensor) -> torch.Tensor:
    """canonical head source: wh (F,3,3,3) | bh (F) | 0 | 1"""
    return torch.cat([wh.reshape(-1), bh, const01(wh.device, wh.dtype)])


def tail_src(wt: torch.Tensor, ws: torch.Tensor, btot: torch.Tensor) -> torch.Tensor:
    """canonical tail source: wt (CO,F,3,3) | ws (CO,3,5,5) | bt + bs + mean (CO) | 0 | 1"""
    return torch.cat([wt.reshape(-1), ws.reshape(-1), btot, const01(wt.device, wt.dtype)])


def pack_ends(src_head: torch.Tensor, src_tail: torch.Tensor, F: int, R: int, dtype: torch.dtype):
    tb = ends_tables(F, R, src_head.device)
    assert src_head.numel() == tb["head_size"] and src_tail.numel() == tb["tail_size"]
    bh = src_head.detach().float().index_select(0, tb["head"]).to(dtype).contiguous()
    bt = src_tail.detach().float().index_select(0, tb["tail"]).to(dtype).contiguous()
    return bh, bt


def pack_head(src_head: torch.Tensor, F: int, dtype: torch.dtype):
    tb = ends_tables(F, 4, src_head.device)
    return src_head.detach().float().index_select(0, tb["head"]).to(dtype).contiguous()


def pack_tail(src_tail: torch.Tensor, F: int, R: int, dtype: torch.dtype):
    tb = ends_tables(F, R, src_tail.device)
    assert src_tail.numel() == tb["tail_size"]
    return src_tail.detach().float().index_select(0, tb["tail"]).to(dtype).contiguous()


def head_fwd(x: torch.Tensor, y: torch.Tensor, blob: torch.Tensor, mean: float):
    n, _, h, w = x.shape
    _launch("sr_head_fwd", L.lib().sr_head_fwd, L.ptr(x), L.ptr(y), L.ptr(blob), mean, n, h, w, y.shape[-1],
                                L.DTYPE_CODE[y.dtype], L.stream_ptr())


def tail_fwd(feat: torch.Tensor, x: torch.Tensor, out: torch.Tensor, blob: torch.Tensor, mean: float, R: int):
    n, h, w, f = feat.shape
    _launch("sr_tail_fwd", L.lib().sr_tail_fwd, L.ptr(feat), L.ptr(x), L.ptr(out), L.ptr(blob), mean, n, h, w, f, R,
                                L.DTYPE_CODE[feat.dtype], L.stream_ptr())


def tail_bwd_data(dout: torch.Tensor, dfeat: torch.Tensor, blob: torch.Tensor, R: int):
    n, h, w, f = dfeat.shape
    _launch("sr_tail_bwd_data", L.lib().sr_tail_bwd_data, L.ptr(dout), L.ptr(dfeat), L.ptr(blob), n, h, w, f, R,
                                     L.DTYPE_CODE[dfeat.dtype], L.stream_ptr())


def tail_wgrad(dout: torch.Tensor, feat: torch.Tensor, x: torch.Tensor, mean: float, R: int,
               wgs: int = 64) -> torch.Tensor:
    """returns d_src_tail (zeros at the constant slots)"""
    n, h, w, f = feat.shape
    tb = ends_tables(f, R, feat.device)
    part = torch.empty((wgs, tb["tail_slab"]), dtype=torch.float32, device=feat.device)
    _launch("sr_tail_wgrad", L.lib().sr_tail_wgrad, L.ptr(dout), L.ptr(feat), L.ptr(x), mean, L.ptr(part), wgs, n, h, w, f, R,
                                  L.DTYPE_CODE[feat.dtype], L.stream_ptr())
    g = part.sum(0).index_select(0, tb["tail_grad"])
    return torch.cat([g, g.new_zeros(2)])


def _tail_grad_vector(part: torch.Tensor, tb) -> torch.Tensor:
    g = part.sum(0).index_select(0, tb["tail_grad"])
    return torch.cat([g, g.new_zeros(2)])


def tail_bwd(dout: torch.Tensor, feat: torch.Tensor, x: torch.Tensor, blob: torch.Tensor, mean: float, R: int, wgs: int = 256):
    """tail_bwd_data + tail_wgrad in ONE launch (bf16: the gradient image is un-shuffled once for both): (dfeat, d_src_tail)"""
    n, h, w, f = feat.shape
    tb = ends_tables(f, R, feat.device)
    part = torch.empty((wgs, tb["tail_slab"]), dtype=torch.float32, device=feat.device)
    dfeat = torch.empty_like(feat)
    _launch("sr_tail_bwd", L.lib().sr_tail_bwd, L.ptr(dout), L.ptr(feat), L.ptr(x), mean, L.ptr(blob), L.ptr(dfeat), L.ptr(part), wgs,
            n, h, w, f, R, L.DTYPE_CODE[feat.dtype], L.stream_ptr())
    return dfeat, _tail_grad_vector(part, tb)


def tail_bwd_loss(out: torch.Tensor, hr: torch.Tensor, kind: int, gscale: float, feat: torch.Tensor, x: torch.Tensor,
                  blob: torch.Tensor, mean: float, R: int, wgs: int = 256):
    """the same with d(loss)/d(out) FORMED in the kernel from out and hr (kind 1: L1, 2: Charbonnier; gscale = upstream / numel):
    (dfeat, d_src_tail, per-workgroup loss sums)"""
    n, h, w, f = feat.shape
    tb = ends_tables(f, R, feat.device)
    part = torch.empty((wgs, tb["tail_slab"]), dtype=torch.float32, device=feat.device)
    loss_part = torch.empty(wgs, dtype=torch.float32, device=feat.device)
    dfeat = torch.empty_like(feat)
    _launch("sr_tail_bwd_loss", L.lib().sr_tail_bwd_loss, L.ptr(out), L.ptr(hr), kind, gscale, L.ptr(loss_part), L.ptr(feat), L.ptr(x),
            mean, L.ptr(blob), L.ptr(dfeat), L.ptr(part), wgs, n, h, w, f, R, L.DTYPE_CODE[feat.dtype], L.stream_ptr())
    return dfeat, _tail_grad_vector(part, tb), loss_part


def head_wgrad(dy0: torch.Tensor, x: torch.Tensor, mean: float, wgs: int = 64) -> torch.Tensor:
    n, h, w, f = dy0.shape
    tb = ends_tables(f, 4, dy0.device)
    part = torch.empty((wgs, tb["head_slab"]), dtype=torch.float32, device=dy0.device)
    _launch("sr_head_wgrad", L.lib().sr_head_wgrad, L.ptr(dy0), L.ptr(x), mean, L.ptr(part), wgs, n, h, w, f,
                                  L.DTYPE_CODE[dy0.dtype], L.stream_ptr())
    g = part.sum(0).index_select(0, tb["head_grad"])
    return torch.cat([g, g.new_zeros(2)])


# =====================================================================================
# searched network (Result_Model): csrc/result_block.h
# =====================================================================================
@lru_cache(maxsize=None)
def _dev_index(kind: str, args: tuple, device_index: int):
    dev = torch.device("cuda", device_index)
    if kind == "conv":
        return torch.from_numpy(P.rm_conv_index(*args)).to(dev)
    if kind == "block":
        return torch.from_numpy(P.rm_block_index(*args)).to(dev)
    if kind == "bias":
        return torch.from_numpy(P.rm_block_bias_index(*args)).to(dev)
    w, b = P.rm_block_wgrad_index(*args) if kind == "block_wgrad" else P.rm_wgrad_index(*args)
    return torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)


def _dev_idx(t: torch.Tensor) -> int:
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def rm_pack(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """(rows, ci, k, k) fp32 weight -> packed MFMA fragments for rm_conv_kernel"""
    rows, ci, k, _ = w.shape
    idx = _dev_index("conv", (rows, ci, k), _dev_idx(w))
    src = torch.cat([w.detach().float().reshape(-1), w.new_zeros(1)])
    return src.index_select(0, idx).to(dtype).contiguous()


def rm_pack_block(w: torch.Tensor, F: int, IN: int, dtype: torch.dtype, transposed: bool = False) -> torch.Tensor:
    """(split, split, k, k) block weight -> packed fragments of its F-channel embedding (transposed: backward-data)"""
    split, _, k, _ = w.shape
    idx = _dev_index("block", (F, IN, split, k, transposed), _dev_idx(w))
    return torch.cat([w.detach().float().reshape(-1), w.new_zeros(1)]).index_select(0, idx).to(dtype)


def rm_bias32(b: torch.Tensor, IN: int) -> torch.Tensor:
    idx = _dev_index("bias", (IN, b.shape[0]), _dev_idx(b))
    return torch.cat([b.detach().float(), b.new_zeros(1)]).index_select(0, idx)


def rm_block_fwd(x: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, wp: torch.Tensor, bias32: torch.Tensor, k: int):
    n, h, w, f = x.shape
    _launch("sr_rm_block_fwd", L.lib().sr_rm_block_fwd, L.ptr(x), L.ptr(y), L.ptr(mask), L.ptr(wp), L.ptr(bias32), n, h, w, f, k,
            L.DTYPE_CODE[x.dtype], L.stream_ptr())


def rm_block_bwd_data(dy: torch.Tensor, mask: torch.Tensor, dx: torch.Tensor, wpt: torch.Tensor, k: int):
    n, h, w, f = dy.shape
    _launch("sr_rm_block_bwd_data", L.lib().sr_rm_block_bwd_data, L.ptr(dy), L.ptr(mask), L.ptr(dx), L.ptr(wpt), n, h, w, f, k,
            L.DTYPE_CODE[dy.dtype], L.stream_ptr())


def rm_wgrad(g: torch.Tensor, mask, xin: torch.Tensor, rows: int, cols: int, k: int, wgs: int = 0):
    """(weight gradient (rows, cols, k, k), bias gradient (rows)) of the conv that maps xin to g (times mask: a block)"""
    n, h, w, ca = g.shape
    cb = xin.shape[-1]
    if wgs <= 0:
        wgs = max(1, min(256, n * ((h + 15) // 16) * ((w + 15) // 16)))
    ng = P.rm_wgrad_groups(ca, k)
    part = torch.empty((ng, wgs, P.RM_WGRAD_TPG * 1024), dtype=torch.float32, device=g.device)
    _launch("sr_rm_wgrad", L.lib().sr_rm_wgrad, L.ptr(g), L.ptr(mask) if mask is not None else None, L.ptr(xin), L.ptr(part), wgs,
            n, h, w, ca, cb, k, L.DTYPE_CODE[g.dtype], L.stream_ptr())
    slab = part.sum(1).reshape(-1)
    iw, ib = _dev_index("wgrad", (ca, rows, cols, k), _dev_idx(g))
    return slab.index_select(0, iw).view(rows, cols, k, k), slab.index_select(0, ib)


def rm_block_wgrad(dy: torch.Tensor, mask: torch.Tensor, x: torch.Tensor, IN: int, split: int, k: int, wgs: int = 0):
    """(weight gradient (split, split, k, k), bias gradient (split)) of block [IN, split, k]"""
    n, h, w, f = dy.shape
    if wgs <= 0:
        wgs = max(1, min(256, n * ((h + 15) // 16) * ((w + 15) // 16)))
    ng = P.rm_wgrad_groups(f, k)
    part = torch.empty((ng, wgs, P.RM_WGRAD_TPG * 1024), dtype=torch.float32, device=dy.device)
    _launch("sr_rm_wgrad", L.lib().sr_rm_wgrad, L.ptr(dy), L.ptr(mask), L.ptr(x), L.ptr(part), wgs, n, h, w, f, f, k,
            L.DTYPE_CODE[dy.dtype], L.stream_ptr())
    slab = part.sum(1).reshape(-1)
    iw, ib = _dev_index("block_wgrad", (f, IN, split, k), _dev_idx(dy))
    return slab.index_select(0, iw).view(split, split, k, k), slab.index_select(0, ib)


def rm_tail_fwd(feat: torch.Tensor, out: torch.Tensor, wp: torch.Tensor, R: int, k: int):
    n, h, w, f = feat.shape
    _launch("sr_rm_tail_fwd", L.lib().sr_rm_tail_fwd, L.ptr(feat), L.ptr(out), L.ptr(wp), n, h, w, f, R, k,
            L.DTYPE_CODE[feat.dtype], L.stream_ptr())


def rm_unshuffle(dout: torch.Tensor, R: int, dtype: torch.dtype) -> torch.Tensor:
    n, _, hr, wr = dout.shape
    h, w = hr // R, wr // R
    dconv = torch.empty((n, h, w, P.rm_cp(R)), dtype=dtype, device=dout.device)
    _launch("sr_rm_unshuffle", L.lib().sr_rm_unshuffle, L.ptr(dout), L.ptr(dconv), n, h, w, R, L.DTYPE_CODE[dtype], L.stream_ptr())
    return dconv


def rm_tail_bwd_data(dconv: torch.Tensor, dfeat: torch.Tensor, wpt: torch.Tensor, R: int, k: int):
    n, h, w, f = dfeat.shape
    _launch("sr_rm_tail_bwd_data", L.lib().sr_rm_tail_bwd_data, L.ptr(dconv), L.ptr(dfeat), L.ptr(wpt), n, h, w, f, R, k,
            L.DTYPE_CODE[dfeat.dtype], L.stream_ptr())


# =====================================================================================
# per-frame video network (models/single_image_model.py): csrc/frame_net.h
# =====================================================================================
@lru_cache(maxsize=None)
def _fn_pack_index(channel: int, nb: int, device_index: int):
    layout, offsets = P.fn_tables(channel, nb)
    return torch.from_numpy(layout["pack"]).to(torch.device("cuda", device_index)), (ctypes.c_long * len(offsets))(*offsets)


@lru_cache(maxsize=None)
def _fn_bwd_pack_index(channel: int, nb: int, device_index: int):
    return torch.from_numpy(P.fn_bwd_tables(channel, nb)).to(torch.device("cuda", device_index))


def fn_pack(convs, up_w: torch.Tensor, up_b: torch.Tensor, dtype: torch.dtype, backward: bool = False):
    """convs: the 2 nb + 1 (effective weight (C, C, 3, 3), bias (C)) pairs in forward order; up_w (C, 3, 5, 5), up_b (3) ->
    (blob in `dtype`, host array of per-conv offsets) as sr_fn_net_fwd reads them; backward: and, third, the transposed, flipped
    weights as sr_fn_net_bwd reads them (packing.fn_bwd_tables), gathered from the same source vector"""
    channel, nb = up_w.shape[0], (len(convs) - 1) // 2
    idx, offs = _fn_pack_index(channel, nb, _dev_idx(up_w))
    parts = [t.detach().float().reshape(-1) for wb in convs for t in wb] + [up_w.detach().float().reshape(-1), up_b.detach().float(),
                                                                          up_w.new_zeros(1, dtype=torch.float32)]
    src = torch.cat(parts)
    blob = src.index_select(0, idx).to(dtype).contiguous()
    if not backward:
        return blob, offs
    return blob, offs, src.index_select(0, _fn_bwd_pack_index(channel, nb, _dev_idx(up_w))).to(dtype).contiguous()


def fn_pack_encoder(w: torch.Tensor, b: torch.Tensor, dtype: torch.dtype):
    """the encoder (C, 3, 3, 3), (C) as sr_head_fwd's 32-row head blob (rows >= C zero)"""
    wp = w.new_zeros((P.FN_C, 3, 3, 3), dtype=torch.float32)
    wp[:w.shape[0]] = w.detach().float()
    bp = w.new_zeros(P.FN_C, dtype=torch.float32)
    bp[:w.shape[0]] = b.detach().float()
    return pack_head(head_src(wp, bp), P.FN_C, dtype)


def fn_net_fwd(frames: torch.Tensor, blob: torch.Tensor, offs, head_blob: torch.Tensor, scratch, out: torch.Tensor, out_is: int,
               nb: int, stages: int = P.FN_ALL):
    """frames (N, 3, H, W) fp32 -> out (image stride out_is floats); scratch: three (N, H, W, 32) images in the blob's dtype"""
    n, _, h, w = frames.shape
    _launch("sr_fn_net_fwd", L.lib().sr_fn_net_fwd, L.ptr(frames), L.ptr(blob), offs, L.ptr(head_blob), L.ptr(scratch[0]),
            L.ptr(scratch[1]), L.ptr(scratch[2]), out.data_ptr(), out_is, nb, n, h, w, L.DTYPE_CODE[blob.dtype], stages,
            L.stream_ptr(frames.device))


def fn_net_train_fwd(frames: torch.Tensor, blob: torch.Tensor, offs, head_blob: torch.Tensor, acts: torch.Tensor, ts: torch.Tensor,
                     masks: torch.Tensor, out: torch.Tensor, out_is: int, nb: int, stages: int = P.FN_ALL):
    """fn_net_fwd that keeps acts (nb + 2, N, H, W, 32), ts (nb, N, H, W, 32) in the blob's dtype and masks (nb, N, H, W) int32"""
    n, _, h, w = frames.shape
    _launch("sr_fn_net_train_fwd", L.lib().sr_fn_net_train_fwd, L.ptr(frames), L.ptr(blob), offs, L.ptr(head_blob), L.ptr(acts),
            L.ptr(ts) if nb else None, L.ptr(masks) if nb else None, out.data_ptr(), out_is, nb, n, h, w, L.DTYPE_CODE[blob.dtype],
            stages, L.stream_ptr(frames.device))


def fn_bwd_wgs(n: int, h: int, w: int) -> int:
    """default workgroup count of the weight-gradient launches: one per 16 x 16 tile up to 128"""
    return max(1, min(128, n * ((h + 15) // 16) * ((w + 15) // 16)))


def _fn_bwd(name, frames, grad_args, bwd_blob, acts, ts, masks, gs, parts, wgs, grads, channel, nb, stages):
    """sr_fn_net_bwd / sr_fn_net_bwd_loss / sr_fn_net_bwd_sized: they differ in grad_args, where the output gradient comes from and
    how it is laid out (up to and including g_is, the sized one's resize behind it)"""
    n, _, h, w = frames.shape
    _launch(name, getattr(L.lib(), name), L.ptr(frames), *grad_args, L.ptr(bwd_blob), L.ptr(acts), L.ptr(ts) if nb else None,
            L.ptr(masks) if nb else None, L.ptr(gs), L.ptr(parts), wgs, L.ptr(grads), channel, nb, n, h, w, L.DTYPE_CODE[bwd_blob.dtype],
            stages, L.stream_ptr(frames.device))


def fn_net_bwd(frames: torch.Tensor, g: torch.Tensor, g_is: int, bwd_blob: torch.Tensor, acts: torch.Tensor, ts: torch.Tensor,
               masks: torch.Tensor, gs: torch.Tensor, parts: torch.Tensor, wgs: int, grads: torch.Tensor, channel: int, nb: int,
               stages: int = P.FN_BWD_ALL):
    """g: d(loss)/d(out) fp32 (image stride g_is floats); gs: (4, N, H, W, 32) gradient scratch; parts: packing.fn_bwd_parts(nb, wgs)
    floats; grads: the flat fp32 gradient vector in packing.fn_grad_sizes' order"""
    _fn_bwd("sr_fn_net_bwd", frames, (g.data_ptr(), g_is), bwd_blob, acts, ts, masks, gs, parts, wgs, grads, channel, nb, stages)


def fn_resize(h: int, w: int, oh: int, ow: int, device) -> tuple:
    """The sized entry points' resize argument for H x W frames and an (oh, ow) output: (oh, ow, ty, ly, tx, lx) with
    packing.fn_resize_tables(4 h + 1, oh) and (4 w + 1, ow) on `device`.  The caller keeps it (Result_Model caches it per size)."""
    if not (1 <= oh <= P.FN_MAX_OUT and 1 <= ow <= P.FN_MAX_OUT):
        raise ValueError(f"fn_resize: output size {(oh, ow)} (1 .. {P.FN_MAX_OUT} each)")
    tabs = [torch.from_numpy(t.copy()).to(device) for t in P.fn_resize_tables(4 * h + 1, oh) + P.fn_resize_tables(4 * w + 1, ow)]
    return (oh, ow) + tuple(tabs)


def _rz_args(rz):
    return (rz[0], rz[1]) + tuple(L.ptr(t) for t in rz[2:])


def fn_net_fwd_sized(frames: torch.Tensor, blob: torch.Tensor, offs, head_blob: torch.Tensor, scratch, out: torch.Tensor, out_is: int,
                     rz: tuple, nb: int, stages: int = P.FN_ALL):
    """fn_net_fwd with the resize to rz's (oh, ow) inside the upsampler kernel (rz: fn_resize); out (N, 3, oh, ow) fp32"""
    n, _, h, w = frames.shape
    _launch("sr_fn_net_fwd_sized", L.lib().sr_fn_net_fwd_sized, L.ptr(frames), L.ptr(blob), offs, L.ptr(head_blob), L.ptr(scratch[0]),
            L.ptr(scratch[1]), L.ptr(scratch[2]), out.data_ptr(), out_is, *_rz_args(rz), nb, n, h, w, L.DTYPE_CODE[blob.dtype], stages,
            L.stream_ptr(frames.device))


def fn_net_train_fwd_sized(frames: torch.Tensor, blob: torch.Tensor, offs, head_blob: torch.Tensor, acts: torch.Tensor, ts: torch.Tensor,
                           masks: torch.Tensor, out: torch.Tensor, out_is: int, rz: tuple, nb: int, stages: int = P.FN_ALL):
    """fn_net_train_fwd with the resize to rz's (oh, ow) inside the upsampler kernel"""
    n, _, h, w = frames.shape
    _launch("sr_fn_net_train_fwd_sized", L.lib().sr_fn_net_train_fwd_sized, L.ptr(frames), L.ptr(blob), offs, L.ptr(head_blob),
            L.ptr(acts), L.ptr(ts) if nb else None, L.ptr(masks) if nb else None, out.data_ptr(), out_is, *_rz_args(rz), nb, n, h, w,
            L.DTYPE_CODE[blob.dtype], stages, L.stream_ptr(frames.device))


def fn_net_bwd_sized(frames: torch.Tensor, g: torch.Tensor, g_is: int, rz: tuple, bwd_blob: torch.Tensor, acts: torch.Tensor,
                     ts: torch.Tensor, masks: torch.Tensor, gs: torch.Tensor, parts: torch.Tensor, wgs: int, grads: torch.Tensor,
                     channel: int, nb: int, stages: int = P.FN_BWD_ALL):
    """fn_net_bwd from g = d(loss)/d(out) of the sized forward, fp32 (N, 3, oh, ow) with image stride g_is"""
    _fn_bwd("sr_fn_net_bwd_sized", frames, (g.data_ptr(), g_is) + _rz_args(rz), bwd_blob, acts, ts, masks, gs, parts, wgs, grads,
            channel, nb, stages)


LOSS_KINDS = {"l1": 1, "charbonnier": 2}


def scale_by(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """x * scale with the product formed in fp32 (sr_scale_by): a folded loss's parked gradient times the loss gradient that autograd
    hands over as a device scalar"""
    y = torch.empty_like(x)
    s = scale.detach().float().reshape(1)
    _launch("sr_scale_by", L.lib().sr_scale_by, L.ptr(y), L.ptr(x), x.numel(), L.ptr(s), L.DTYPE_CODE[x.dtype], L.stream_ptr(x.device))
    return y


def fn_loss_wgs(n: int, h: int, w: int, wgs: int) -> int:
    """workgroups of sr_fn_net_bwd_loss's first stage = entries of its loss_part: one per 8 x 16 LR tile up to wgs"""
    return min(n * ((h + 7) // 8) * ((w + 15) // 16), wgs)


def fn_net_bwd_loss(frames: torch.Tensor, sr: torch.Tensor, hr: torch.Tensor, kind: int, gscale: float, g_is: int,
                    bwd_blob: torch.Tensor, acts: torch.Tensor, ts: torch.Tensor, masks: torch.Tensor, gs: torch.Tensor,
                    parts: torch.Tensor, wgs: int, grads: torch.Tensor, channel: int, nb: int) -> torch.Tensor:
    """fn_net_bwd with d(loss)/d(out) FORMED in the upsampler's backward from sr (the network's output) and hr, both contiguous fp32
    with image stride g_is (kind 1: L1, 2: Charbonnier; gscale = upstream / numel).  Returns the per-workgroup loss sums."""
    n, _, h, w = frames.shape
    if sr.dtype != torch.float32 or hr.dtype != torch.float32 or sr.numel() != n * g_is or hr.numel() != n * g_is or g_is != 48 * h * w:
        raise ValueError("fn_net_bwd_loss: sr and hr contiguous fp32 (N, 3, 4H, 4W)")
    loss_part = torch.empty(fn_loss_wgs(n, h, w, wgs), dtype=torch.float32, device=frames.device)
    _fn_bwd("sr_fn_net_bwd_loss", frames, (L.ptr(sr), L.ptr(hr), kind, gscale, L.ptr(loss_part), g_is), bwd_blob, acts, ts, masks, gs,
            parts, wgs, grads, channel, nb, P.FN_BWD_ALL)
    return loss_part


def fn_net_bwd_loss_sized(frames: torch.Tensor, sr: torch.Tensor, hr: torch.Tensor, kind: int, gscale: float, g_is: int, rz: tuple,
                          bwd_blob: torch.Tensor, acts: torch.Tensor, ts: torch.Tensor, masks: torch.Tensor, gs: torch.Tensor,
                          parts: torch.Tensor, wgs: int, grads: torch.Tensor, channel: int, nb: int) -> torch.Tensor:
    """fn_net_bwd_loss behind the sized forward: sr and hr contiguous fp32 (N, 3, oh, ow) of rz (fn_resize), image stride g_is.
    Returns the per-workgroup loss sums, every one written (0 where a workgroup's tiles own no output)."""
    n, _, h, w = frames.shape
    if sr.dtype != torch.float32 or hr.dtype != torch.float32 or sr.numel() != n * g_is or hr.numel() != n * g_is \
            or g_is != 3 * rz[0] * rz[1]:
        raise ValueError("fn_net_bwd_loss_sized: sr and hr contiguous fp32 (N, 3, oh, ow)")
    loss_part = torch.empty(fn_loss_wgs(n, h, w, wgs), dtype=torch.float32, device=frames.device)
    _fn_bwd("sr_fn_net_bwd_loss_sized", frames, (L.ptr(sr), L.ptr(hr), kind, gscale, L.ptr(loss_part), g_is) + _rz_args(rz), bwd_blob,
            acts, ts, masks, gs, parts, wgs, grads, channel, nb, P.FN_BWD_ALL)
    return loss_part


# =====================================================================================
# multi-frame video network (models/naive_multi_model_easy.py): csrc/multi_frame.h
# =====================================================================================
@lru_cache(maxsize=None)
def _mf_pack_index(channel: int, nb: int, device_index: int):
    layout, _ = P.mf_tables(channel, nb)
    return torch.from_numpy(layout["pack"]).to(torch.device("cuda", device_index))


def _mf_src(blocks, dec_w: torch.Tensor, dec_b: torch.Tensor) -> torch.Tensor:
    """the fp32 source vector packing.mf_tables and mf_bwd_tables index: the blocks' tensors, decode's, one zero"""
    parts = [t.detach().float().reshape(-1) for blk in blocks for t in blk] + [dec_w.detach().float().reshape(-1), dec_b.detach().float(),
                                                                             dec_w.new_zeros(1, dtype=torch.float32)]
    return torch.cat(parts)


def mf_pack(blocks, dec_w: torch.Tensor, dec_b: torch.Tensor, dtype: torch.dtype):
    """blocks: per block (w1, b1, w2, b2), block 0's w1 (C, 2C + 2, 3, 3) over cat(flow, warp, e), the others (C, C, 3, 3); dec_w
    (48, C, 3, 3) effective, dec_b (48) -> the blob in `dtype` as sr_mf_net_fwd reads it"""
    idx = _mf_pack_index(dec_w.shape[1], len(blocks), _dev_idx(dec_w))
    return _mf_src(blocks, dec_w, dec_b).index_select(0, idx).to(dtype).contiguous()


def _mf_check(frames, flows, B, N, who):
    bn, _, h, w = frames.shape
    if bn != B * N or (N > 1 and (flows is None or tuple(flows.shape) != (B, N - 1, 2, h, w) or flows.dtype != torch.float32
                                  or not flows.is_contiguous())):
        raise ValueError(f"{who}: frames (B N, 3, H, W) and contiguous fp32 flows (B, N - 1, 2, H, W)")
    return h, w


def mf_net_fwd(frames: torch.Tensor, flows, blob: torch.Tensor, head_blob: torch.Tensor, scratch, out: torch.Tensor, nb: int, B: int,
               N: int, stages: int = P.MF_ALL):
    """frames (B N, 3, H, W) fp32, flows (B, N - 1, 2, H, W) fp32 contiguous (None when N == 1) -> out (B N, 3, 4H, 4W) fp32; scratch:
    three (B N, H, W, 32) images in the blob's dtype"""
    h, w = _mf_check(frames, flows, B, N, "mf_net_fwd")
    _launch("sr_mf_net_fwd", L.lib().sr_mf_net_fwd, L.ptr(frames), L.ptr(flows) if N > 1 else None, L.ptr(blob), L.ptr(head_blob),
            L.ptr(scratch[0]), L.ptr(scratch[1]), L.ptr(scratch[2]), out.data_ptr(), nb, B, N, h, w, L.DTYPE_CODE[blob.dtype], stages,
            L.stream_ptr(frames.device))


# ---- the training route: csrc/multi_frame.h (forward that saves), csrc/multi_frame_bwd.h ----
@lru_cache(maxsize=None)
def _mf_bwd_pack_index(channel: int, nb: int, device_index: int):
    return torch.from_numpy(P.mf_bwd_tables(channel, nb)).to(torch.device("cuda", device_index))


def mf_pack_train(blocks, dec_w: torch.Tensor, dec_b: torch.Tensor, dtype: torch.dtype):
    """mf_pack and, second, the transposed, tap-flipped operands as sr_mf_net_bwd reads them (packing.mf_bwd_tables), gathered from
    the same source vector"""
    channel, nb = dec_w.shape[1], len(blocks)
    dev = _dev_idx(dec_w)
    src = _mf_src(blocks, dec_w, dec_b)
    return (src.index_select(0, _mf_pack_index(channel, nb, dev)).to(dtype).contiguous(),
            src.index_select(0, _mf_bwd_pack_index(channel, nb, dev)).to(dtype).contiguous())


def mf_net_train_fwd(frames: torch.Tensor, flows, blob: torch.Tensor, head_blob: torch.Tensor, acts: torch.Tensor, ts: torch.Tensor,
                     masks: torch.Tensor, wf: torch.Tensor, out: torch.Tensor, nb: int, B: int, N: int, stages: int = P.MF_ALL):
    """mf_net_fwd that keeps acts (nb + 1, B N, H, W, 32), ts (nb, ..), wf (2, ..: the warp operand, the flow image) in the blob's dtype
    and masks (nb, B N, H, W) int32"""
    h, w = _mf_check(frames, flows, B, N, "mf_net_train_fwd")
    _launch("sr_mf_net_train_fwd", L.lib().sr_mf_net_train_fwd, L.ptr(frames), L.ptr(flows) if N > 1 else None, L.ptr(blob),
            L.ptr(head_blob), L.ptr(acts), L.ptr(ts), L.ptr(masks), L.ptr(wf), out.data_ptr(), nb, B, N, h, w, L.DTYPE_CODE[blob.dtype],
            stages, L.stream_ptr(frames.device))


def _mf_bwd(name, frames, flows, flow_bound, grad_args, bwd_blob, acts, ts, masks, wf, gs, parts, wgs, grads, channel, nb, B, N, h, w,
            stages):
    """sr_mf_net_bwd / sr_mf_net_bwd_loss: they differ in grad_args, where the output gradient comes from"""
    _launch(name, getattr(L.lib(), name), L.ptr(frames), L.ptr(flows) if N > 1 else None, L.ptr(flow_bound) if N > 1 else None, *grad_args,
            L.ptr(bwd_blob), L.ptr(acts), L.ptr(ts), L.ptr(masks), L.ptr(wf), L.ptr(gs), L.ptr(parts), wgs, L.ptr(grads), channel, nb, B, N,
            h, w, L.DTYPE_CODE[bwd_blob.dtype], stages, L.stream_ptr(frames.device))


def mf_net_bwd(frames: torch.Tensor, flows, flow_bound, g: torch.Tensor, bwd_blob: torch.Tensor, acts: torch.Tensor, ts: torch.Tensor,
               masks: torch.Tensor, wf: torch.Tensor, gs: torch.Tensor, parts: torch.Tensor, wgs: int, grads: torch.Tensor, channel: int,
               nb: int, B: int, N: int, stages: int = P.MF_BWD_ALL):
    """g: d(loss)/d(out), contiguous fp32 (B N, 3, 4H, 4W); flow_bound: device scalar >= max |flow| (None when N == 1); gs: (6, B N, H,
    W, 32) gradient scratch; parts: packing.mf_bwd_parts(nb, wgs) floats; grads: the flat fp32 vector in packing.mf_grad_sizes' order"""
    h, w = _mf_check(frames, flows, B, N, "mf_net_bwd")
    if g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != B * N * 48 * h * w:
        raise ValueError("mf_net_bwd: g contiguous fp32 (B N, 3, 4H, 4W)")
    _mf_bwd("sr_mf_net_bwd", frames, flows, flow_bound, (g.data_ptr(),), bwd_blob, acts, ts, masks, wf, gs, parts, wgs, grads, channel, nb,
            B, N, h, w, stages)


def mf_loss_wgs(bn: int, h: int, w: int, wgs: int) -> int:
    """workgroups of sr_mf_net_bwd_loss's first stage = entries of its loss_part: one per 8 x 32 LR tile up to wgs"""
    return min(bn * ((h + 7) // 8) * ((w + 31) // 32), wgs)


def mf_net_bwd_loss(frames: torch.Tensor, flows, flow_bound, sr: torch.Tensor, hr: torch.Tensor, kind: int, gscale: float,
                    bwd_blob: torch.Tensor, acts: torch.Tensor, ts: torch.Tensor, masks: torch.Tensor, wf: torch.Tensor, gs: torch.Tensor,
                    parts: torch.Tensor, wgs: int, grads: torch.Tensor, channel: int, nb: int, B: int, N: int) -> torch.Tensor:
    """mf_net_bwd with d(loss)/d(out) FORMED in the tail backward's first stage from sr (the network's output) and hr, contiguous fp32
    (B N, 3, 4H, 4W) (kind 1: L1, 2: Charbonnier; gscale = upstream / numel).  Returns the per-workgroup loss sums."""
    h, w = _mf_check(frames, flows, B, N, "mf_net_bwd_loss")
    numel = B * N * 48 * h * w
    if sr.dtype != torch.float32 or hr.dtype != torch.float32 or sr.numel() != numel or hr.numel() != numel:
        raise ValueError("mf_net_bwd_loss: sr and hr contiguous fp32 (B N, 3, 4H, 4W)")
    loss_part = torch.empty(mf_loss_wgs(B * N, h, w, wgs), dtype=torch.float32, device=frames.device)
    _mf_bwd("sr_mf_net_bwd_loss", frames, flows, flow_bound, (L.ptr(sr), L.ptr(hr), kind, gscale, L.ptr(loss_part)), bwd_blob, acts, ts,
            masks, wf, gs, parts, wgs, grads, channel, nb, B, N, h, w, P.MF_BWD_ALL)
    return loss_part


# =====================================================================================
# the video networks' one-call training step: csrc/clip_param_step.h around the training entry points above
# =====================================================================================
def fn_net_train_step(step, frames: torch.Tensor, hr: torch.Tensor, kind: int, offs, acts: torch.Tensor, ts: torch.Tensor,
                      masks: torch.Tensor, out: torch.Tensor, gs: torch.Tensor, parts: torch.Tensor, wgs: int, grads: torch.Tensor,
                      loss_part: torch.Tensor, channel: int, nb: int, dtype: torch.dtype):
    """step: an _lib.ClipStep (models/clip_train.train_step fills it); the rest as fn_net_train_fwd and fn_net_bwd_loss, hr contiguous fp32
    (N, 3, 4H, 4W); loss_part: at least fn_loss_wgs(n, h, w, wgs) floats"""
    n, _, h, w = frames.shape
    if hr.dtype != torch.float32 or hr.numel() != n * 48 * h * w or loss_part.numel() < fn_loss_wgs(n, h, w, wgs):
        raise ValueError("fn_net_train_step: hr contiguous fp32 (N, 3, 4H, 4W), loss_part of fn_loss_wgs floats")
    _launch("sr_fn_net_train_step", L.lib().sr_fn_net_train_step, ctypes.byref(step), L.ptr(frames), L.ptr(hr), kind, offs, L.ptr(acts),
            L.ptr(ts) if nb else None, L.ptr(masks) if nb else None, L.ptr(out), L.ptr(gs), L.ptr(parts), wgs, L.ptr(grads), L.ptr(loss_part),
            channel, nb, n, h, w, L.DTYPE_CODE[dtype], L.stream_ptr(frames.device))


def fn_net_train_step_sized(step, frames: torch.Tensor, hr: torch.Tensor, kind: int, offs, acts: torch.Tensor, ts: torch.Tensor,
                            masks: torch.Tensor, out: torch.Tensor, rz: tuple, gs: torch.Tensor, parts: torch.Tensor, wgs: int,
                            grads: torch.Tensor, loss_part: torch.Tensor, channel: int, nb: int, dtype: torch.dtype):
    """fn_net_train_step at rz's (oh, ow) (fn_resize): hr and out contiguous fp32 (N, 3, oh, ow); loss_part as there"""
    n, _, h, w = frames.shape
    numel = n * 3 * rz[0] * rz[1]
    if hr.dtype != torch.float32 or hr.numel() != numel or out.numel() != numel or loss_part.numel() < fn_loss_wgs(n, h, w, wgs):
        raise ValueError("fn_net_train_step_sized: hr and out contiguous fp32 (N, 3, oh, ow), loss_part of fn_loss_wgs floats")
    _launch("sr_fn_net_train_step_sized", L.lib().sr_fn_net_train_step_sized, ctypes.byref(step), L.ptr(frames), L.ptr(hr), kind, offs,
            L.ptr(acts), L.ptr(ts) if nb else None, L.ptr(masks) if nb else None, L.ptr(out), *_rz_args(rz), L.ptr(gs), L.ptr(parts), wgs,
            L.ptr(grads), L.ptr(loss_part), channel, nb, n, h, w, L.DTYPE_CODE[dtype], L.stream_ptr(frames.device))


def mf_net_train_step(step, frames: torch.Tensor, flows, flow_bound, hr: torch.Tensor, kind: int, acts: torch.Tensor, ts: torch.Tensor,
                      masks: torch.Tensor, wf: torch.Tensor, out: torch.Tensor, gs: torch.Tensor, parts: torch.Tensor, wgs: int,
                      grads: torch.Tensor, loss_part: torch.Tensor, channel: int, nb: int, B: int, N: int, dtype: torch.dtype):
    """step: an _lib.ClipStep; the rest as mf_net_train_fwd and mf_net_bwd_loss, hr contiguous fp32 (B N, 3, 4H, 4W); loss_part: at least
    mf_loss_wgs(B N, h, w, wgs) floats"""
    h, w = _mf_check(frames, flows, B, N, "mf_net_train_step")
    if hr.dtype != torch.float32 or hr.numel() != B * N * 48 * h * w or loss_part.numel() < mf_loss_wgs(B * N, h, w, wgs):
        raise ValueError("mf_net_train_step: hr contiguous fp32 (B N, 3, 4H, 4W), loss_part of mf_loss_wgs floats")
    _launch("sr_mf_net_train_step", L.lib().sr_mf_net_train_step, ctypes.byref(step), L.ptr(frames), L.ptr(flows) if N > 1 else None,
            L.ptr(flow_bound) if N > 1 else None, L.ptr(hr), kind, L.ptr(acts), L.ptr(ts), L.ptr(masks), L.ptr(wf), L.ptr(out), L.ptr(gs),
            L.ptr(parts), wgs, L.ptr(grads), L.ptr(loss_part), channel, nb, B, N, h, w, L.DTYPE_CODE[dtype], L.stream_ptr(frames.device))
