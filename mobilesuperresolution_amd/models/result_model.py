"""The searched network of the NAS stage-3 trainer (reference: pretrain_simplified_model.py:31-141, `Result_Model`, `Block`,
`Conv_sep(seperate=False)`) on the MI355X hot path.

Same constructor (`Result_Model(scale, filename)`; `status=[[IN, split, k], ...]` in place of the file), module tree,
state_dict keys, parameter shapes and initialisation order as the reference, so its checkpoints load and a seeded build
draws the same numbers:

    body.0                       weight-normed 3x3 head conv, 3 -> IN
    body.{i}.body.0.body.0       block i: weight-normed k x k conv, split -> split, on the LAST `split` channels
    body.{nb+1}                  tail conv, IN -> 3 scale^2, with the LAST block's kernel size (the reference's loop variable)
    skip                         weight-normed 5x5 conv, 3 -> 3 scale^2

forward(x) = PixelShuffle(tail(blocks(head(x - 0.5))) + skip(x - 0.5)) -- no + 0.5 at the end, unlike BASIC_MODEL.

The network runs as one autograd.Function whose forward and backward are chains of C calls (csrc/result_block.h for the
blocks and the 5x5 / 7x7 tail, csrc/wdsr_ends.h for the head, the skip and the 3x3 tail).  Activations are NHWC in F = 24
(IN <= 24) or 32 channels, the IN real channels first and the rest exactly zero.  The weight norm of the parameters stays
an ATen op in front of the Function, as for NAS_MODEL's head and tail.  No CPU fallback.
"""
from __future__ import annotations

import ast

import torch
import torch.nn as nn

from .. import _lib as L
from .. import hotpath as HP
from .. import packing as P

__all__ = ["Result_Model", "parse_status"]

_MEAN = 0.5


def parse_status(filename: str):
    """`status` of the last line of a block_index.txt (reference: Result_Model.file_reader, with ast.literal_eval for eval)"""
    with open(filename, "r") as f:
        return ast.literal_eval(f.readlines()[-1].replace("\n", ""))[1]


class _WNConv2d(nn.Module):
    """torch.nn.utils.weight_norm(nn.Conv2d(cin, cout, k)): bias, weight_g, weight_v in that order, the conv's own init"""

    def __init__(self, cin, cout, k):
        super().__init__()
        conv = nn.Conv2d(cin, cout, k, padding=k // 2)
        v = conv.weight.detach().clone()
        self.bias = nn.Parameter(conv.bias.detach().clone())
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
        self.weight_v = nn.Parameter(v)
        self.kernel_size = k

    def weight(self):
        return torch._weight_norm(self.weight_v, self.weight_g, 0)


class Conv_sep(nn.Module):
    """Conv_sep(seperate=False): weight-normed dense k x k conv + ReLU (keys body.0.*)"""

    def __init__(self, input_dim, output_dim, kernal_size, seperate=False):
        super().__init__()
        if seperate:
            raise NotImplementedError("Result_Model hot path: Conv_sep(seperate=True) (depthwise) blocks are not supported")
        self.seperate, self.kernel_size = seperate, kernal_size
        self.body = nn.ModuleList([_WNConv2d(input_dim, output_dim, kernal_size), nn.ReLU(inplace=True)])


class Block(nn.Module):
    """x[:, IN - split:] += ReLU(conv_k(x[:, IN - split:]))"""

    def __init__(self, IN, split, kernel_size):
        super().__init__()
        self.split, self.IN, self.conv_channel = IN - split, IN, split
        self.body = nn.ModuleList([Conv_sep(split, split, kernel_size)])


class _ResultNet(torch.autograd.Function):
    """the whole network: x -> sr, and d(sr) -> d(every conv's weight and bias)"""

    @staticmethod
    def forward(ctx, x, plan, dt, *ts):
        F_, IN, R, status = plan["F"], plan["IN"], plan["scale"], plan["status"]
        dev = x.device
        n, _, h, w = x.shape
        wh, bh = ts[0], ts[1]
        whp = wh.new_zeros((F_, 3, 3, 3))
        whp[:IN] = wh
        bhp = bh.new_zeros(F_)
        bhp[:IN] = bh
        HP_head = HP.pack_head(HP.head_src(whp.detach(), bhp.detach()), F_, dt)
        y = torch.empty((n, h, w, F_), dtype=dt, device=dev)
        HP.head_fwd(x, y, HP_head, _MEAN)
        acts, masks, wblk = [y], [], []
        for i, (_, split, k) in enumerate(status):
            wb, bb = ts[2 + 2 * i], ts[3 + 2 * i]
            yn = torch.empty_like(y)
            m = torch.empty((n, h, w), dtype=torch.int32, device=dev)
            HP.rm_block_fwd(acts[-1], yn, m, HP.rm_pack_block(wb, F_, IN, dt), HP.rm_bias32(bb, IN), k)
            acts.append(yn)
            masks.append(m)
            wblk.append(wb.detach())
        wt, bt, ws, bs = ts[-4:]
        kl = status[-1][2]
        co = 3 * R * R
        btot = (bt + bs).detach()
        wt3 = wt.new_zeros((co, F_, 3, 3))
        if kl == 3:
            wt3[:, :IN] = wt.detach()
        blob_t = HP.pack_tail(HP.tail_src(wt3, ws.detach(), btot), F_, R, dt)
        out = torch.empty((n, 3, R * h, R * w), dtype=torch.float32, device=dev)
        HP.tail_fwd(acts[-1], x, out, blob_t, _MEAN, R)
        wtd = None
        if kl != 3:
            wtd = wt.new_zeros((co, F_, kl, kl))
            wtd[:, :IN] = wt.detach()
            HP.rm_tail_fwd(acts[-1], out, HP.rm_pack(wtd, dt), R, kl)
        ctx.plan, ctx.dt, ctx.wblk, ctx.wtd, ctx.blob_t = plan, dt, wblk, wtd, blob_t
        ctx.save_for_backward(x, *acts, *masks)
        return out

    @staticmethod
    def backward(ctx, dout):
        plan, dt = ctx.plan, ctx.dt
        F_, IN, R, status = plan["F"], plan["IN"], plan["scale"], plan["status"]
        nb = len(status)
        saved = ctx.saved_tensors
        x, acts, masks = saved[0], saved[1:nb + 2], saved[nb + 2:]
        with torch.cuda.device(x.device):
            dout = dout.contiguous().float()
            feat = acts[-1]
            co, kl = 3 * R * R, status[-1][2]
            ot = P.EndsGeom(F_, R).tail_off
            if kl == 3:
                if dt == torch.bfloat16:
                    dfeat, g = HP.tail_bwd(dout, feat, x, ctx.blob_t, _MEAN, R)
                else:
                    dfeat = torch.empty_like(feat)
                    HP.tail_bwd_data(dout, dfeat, ctx.blob_t, R)
                    g = HP.tail_wgrad(dout, feat, x, _MEAN, R)
                g_wt = g[ot["wt"]:ot["wt"] + co * F_ * 9].view(co, F_, 3, 3)[:, :IN]
            else:
                g = HP.tail_wgrad(dout, feat, x, _MEAN, R)          # skip and bias; its 3x3 part belongs to zero weights
                dconv = HP.rm_unshuffle(dout, R, dt)
                cp = P.rm_cp(R)
                wtt = ctx.wtd.new_zeros((F_, cp, kl, kl))
                wtt[:, :co] = ctx.wtd.transpose(0, 1).flip(2, 3)
                dfeat = torch.empty_like(feat)
                HP.rm_tail_bwd_data(dconv, dfeat, HP.rm_pack(wtt, dt), R, kl)
                g_wt, _ = HP.rm_wgrad(dconv, None, feat, co, F_, kl)
                g_wt = g_wt[:, :IN]
            g_ws = g[ot["ws"]:ot["ws"] + co * 75].view(co, 3, 5, 5)
            g_b = g[ot["b"]:ot["b"] + co]
            grads = [None] * (2 * nb)
            dy = dfeat
            for i in range(nb - 1, -1, -1):
                _, split, k = status[i]
                gw, gb = HP.rm_block_wgrad(dy, masks[i], acts[i], IN, split, k)
                grads[2 * i], grads[2 * i + 1] = gw, gb
                dx = torch.empty_like(dy)
                HP.rm_block_bwd_data(dy, masks[i], dx, HP.rm_pack_block(ctx.wblk[i], F_, IN, dt, transposed=True), k)
                dy = dx
            gh = HP.head_wgrad(dy, x, _MEAN)
            oh = P.EndsGeom(F_, R).head_off
            g_wh = gh[oh["wh"]:oh["wh"] + F_ * 27].view(F_, 3, 3, 3)[:IN].contiguous()
            g_bh = gh[oh["b"]:oh["b"] + F_][:IN].contiguous()
        return (None, None, None, g_wh, g_bh, *grads, g_wt.contiguous(), g_b, g_ws.contiguous(), g_b)


class Result_Model(nn.Module):
    """pretrain_simplified_model.Result_Model(scale, filename) on the MI355X hot path.  `status` may replace `filename`;
    `hot_dtype` ("bf16" / "fp32", default $SR_HOT_DTYPE or fp32) selects the storage and MFMA type."""

    MAX_IN = 32

    def __init__(self, scale, filename=None, hot_dtype=None, status=None):
        super().__init__()
        if (filename is None) == (status is None):
            raise ValueError("Result_Model needs exactly one of filename and status")
        self.image_mean = _MEAN
        self.scale = scale
        self.idx = [list(b) for b in (parse_status(filename) if filename is not None else status)]
        self._check_geometry(scale, self.idx)
        self.IN = self.idx[0][0]
        self.hot_dtype = L.hot_dtype(hot_dtype)
        self.F = 24 if self.IN <= 24 else 32
        num_outputs = scale * scale * 3
        body = [_WNConv2d(3, self.IN, 3)]
        for IN, split, k in self.idx:
            body.append(Block(IN, split, k))
        body.append(_WNConv2d(self.IN, num_outputs, self.idx[-1][2]))      # the last block's kernel size, as the reference
        self.body = nn.ModuleList(body)
        self.skip = _WNConv2d(3, num_outputs, 5)
        self._plan = {"F": self.F, "IN": self.IN, "scale": scale, "status": tuple(tuple(b) for b in self.idx)}

    @classmethod
    def _check_geometry(cls, scale, status):
        if scale not in (2, 3, 4):
            raise NotImplementedError(f"Result_Model hot path: scale {scale} (supported: 2, 3, 4)")
        if not status:
            raise NotImplementedError("Result_Model hot path: at least one block")
        IN = status[0][0]
        if not 1 <= IN <= cls.MAX_IN:
            raise NotImplementedError(f"Result_Model hot path: searched width IN = {IN} (supported: 1 <= IN <= {cls.MAX_IN})")
        for b in status:
            if len(b) != 3:
                raise NotImplementedError(f"Result_Model hot path: block entry {b!r} is not [IN, split, k]")
            if b[0] != IN:
                raise NotImplementedError(f"Result_Model hot path: block widths differ ({b[0]} != {IN})")
            if not 1 <= b[1] <= IN:
                raise NotImplementedError(f"Result_Model hot path: split {b[1]} (supported: 1 <= split <= IN = {IN})")
            if b[2] not in (3, 5, 7):
                raise NotImplementedError(f"Result_Model hot path: kernel size {b[2]} (supported: 3, 5, 7)")

    def receptive_halo(self) -> int:
        """LR pixels of context an output pixel needs on each side (inference.tiled_forward)"""
        return max(2, 1 + sum(k // 2 for _, _, k in self.idx) + self.idx[-1][2] // 2)

    def _tensors(self):
        out = [self.body[0].weight(), self.body[0].bias]
        for blk in self.body[1:-1]:
            conv = blk.body[0].body[0]
            out += [conv.weight(), conv.bias]
        tail = self.body[-1]
        return out + [tail.weight(), tail.bias, self.skip.weight(), self.skip.bias]

    def forward(self, x):
        if not x.is_cuda or not self.skip.weight_v.is_cuda:
            raise L.HotpathError("Result_Model (MI355X hot path) needs the model and its input on a HIP device; there is no CPU fallback")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected N x 3 x H x W, got {tuple(x.shape)}")
        if x.shape[0] > 65535:
            raise NotImplementedError(f"Result_Model hot path: batch {x.shape[0]} (supported: <= 65535)")
        with torch.cuda.device(x.device):
            return _ResultNet.apply(x.contiguous().float(), self._plan, self.hot_dtype, *self._tensors())
