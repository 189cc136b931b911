"""NAS supernet (NAS_MODEL, MyAggregationLayer / Split_Block, Conv_sep, ConditionFunction) on the MI355X hot path.

Mirrors reference models/wdsr_b.py: same class names, constructor fields (`params.width_search`,
`params.pretrained`, ...), `forward(x) -> (sr, speed_accu)`, search-control methods (`get_current_blocks`,
`get_block_status`, `get_width_from_block_idx`, `length_grad`, `mask_grad`, `kernel_grad`, ...) and
state_dict keys (`body.{i}.{alpha,beta,alpha1,beta1,alpha2,beta2,split.weight,body.{3,5,7}.0.body.{0,2}.*}`,
`mask.weight`, `head.*`, `tail.*`, `skip.*`, `speed_estimator.estimator.fc*`).

Per block, everything between the block's input and output -- global mask, split mask, the three
depthwise-separable branches, softmax mixing, the hard skip/keep gate -- runs in csrc/nas_block.h
(4 kernels forward+backward).  The scalar glue (softmax over 3 alphas, the straight-through masks and
gate, the closed-form latency head of speed_models/speed_estimator.py:57-76) stays in PyTorch.
Head and tail reuse the kernels of BASIC_MODEL.  No CPU / ATen fallback.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict, namedtuple
from functools import lru_cache

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.nn.init as init

from .. import _lib as L
from .. import hotpath as HP
from .. import packing as P
from . import loss_fold as LF
from .ops import BinaryConv2d, rounding

ModelOutput = namedtuple("ModelOutput", "sr speed_accu speed_curr")

__all__ = ["NAS_MODEL", "ModelOutput", "MyAggregationLayer", "Split_Block", "Conv_sep", "ConditionFunction"]

@lru_cache(maxsize=None)
def _const(device: torch.device, values: tuple) -> torch.Tensor:
    """small fp32 constant on `device`, uploaded once (Tensor.new_tensor is a synchronous host-to-device copy)"""
    return torch.tensor(values, dtype=torch.float32, device=device)


def _on_tensor_device(fn):
    """Run an autograd.Function's forward / backward with the FIRST CUDA tensor argument's device current: the kernels take raw
    pointers and `L.stream_ptr()` returns the current device's stream, so a block used standalone on a GPU that is not the
    current one would otherwise launch on the wrong device's stream (NAS_MODEL.forward holds the same guard)."""
    import functools

    @functools.wraps(fn)
    def wrapped(ctx, *args):
        dev = next((a.device for a in args if isinstance(a, torch.Tensor) and a.is_cuda), None)
        if dev is None:
            dev = next((t.device for t in getattr(ctx, "saved_tensors", ()) if t.is_cuda), None)
        if dev is None:
            return fn(ctx, *args)
        with torch.cuda.device(dev):
            return fn(ctx, *args)
    return wrapped



class _WNConv(nn.Module):
    """parameters of torch.nn.utils.weight_norm(nn.Conv2d(...)): bias, weight_g, weight_v.
    g_init None = weight_norm's own initialisation (g = ||v||, i.e. w = v)."""

    def __init__(self, cin, cout, k, groups=1, g_init=None, zero_bias=False):
        super().__init__()
        conv = nn.Conv2d(cin, cout, k, groups=groups)
        v = conv.weight.detach().clone()
        self.bias = nn.Parameter(torch.zeros(cout) if zero_bias else conv.bias.detach().clone())
        g = v.flatten(1).norm(dim=1).view(-1, 1, 1, 1) if g_init is None else torch.full((cout, 1, 1, 1), float(g_init))
        self.weight_g = nn.Parameter(g)
        self.weight_v = nn.Parameter(v)

    def weight(self):
        return torch._weight_norm(self.weight_v, self.weight_g, 0)      # what nn.utils.weight_norm computes (one fused op)


class Conv_sep(nn.Module):
    """reference wdsr_b.py:375-402 with seperate=True: wn depthwise kxk -> ReLU -> wn 1x1 (keys body.0 / body.2)"""

    def __init__(self, input_dim, output_dim, kernal_size, weight_norm=None, seperate=True):
        super().__init__()
        if not seperate or input_dim != output_dim:
            raise NotImplementedError("hot path supports Conv_sep(seperate=True, input_dim == output_dim)")
        self.seperate, self.kernel_size = seperate, kernal_size
        self.body = nn.ModuleList([_WNConv(input_dim, input_dim, kernal_size, groups=input_dim), nn.Identity(),
                                   _WNConv(input_dim, output_dim, 1)])


class ConditionFunction(torch.autograd.Function):
    """hard gate (reference wdsr_b.py:594-616): (1,0) if alpha1 >= alpha2 else (0,1); straight-through to alpha."""

    @staticmethod
    def forward(ctx, alpha1, alpha2, beta1, beta2):
        with torch.no_grad():                       # same values as the reference's host-side if/else, no host sync
            b1 = (alpha1 >= alpha2).to(beta1.dtype).reshape(1)
            beta1.data = b1
            beta2.data = 1.0 - b1
        return beta1, beta2

    @staticmethod
    def backward(ctx, g1, g2):
        return g1, g2, None, None


@lru_cache(maxsize=None)
def _nas_dev_tables(Fch: int, device_index: int):
    t = P.nas_tables(Fch)
    dev = torch.device("cuda", device_index)
    out = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in t.items()
           if k != "g_wdw" and k != "off"}
    out["g_wdw"] = [torch.from_numpy(a).to(dev) for a in t["g_wdw"]]
    out["off"] = t["off"]
    return out


class _NasBlockFunction(torch.autograd.Function):
    """y = mg*yin + beta2 * ms * sum_k p_k relu(pw_k(relu(dw_k(mg*ms*yin)))) on csrc/nas_block.h"""

    @staticmethod
    @_on_tensor_device
    def forward(ctx, yin, wdw3, wdw5, wdw7, bdw, wpw, bpw, mg, ms, p, beta):
        n, h, w, f = yin.shape
        dev, dt = yin.device, yin.dtype
        tb = _nas_dev_tables(f, dev.index if dev.index is not None else torch.cuda.current_device())
        src = torch.cat([t.detach().float().reshape(-1) for t in (wdw3, wdw5, wdw7, bdw, wpw, bpw, mg, ms, mg * ms)]
                        + [_const(yin.device, (0.0, 1.0))])
        assert src.numel() == tb["off"]["size"]
        dwp = src.index_select(0, tb["dwp"]).contiguous()
        frags = src.index_select(0, tb["frags"]).to(dt).contiguous()
        tabs = src.index_select(0, tb["tabs"]).contiguous()
        scal = torch.cat([p.detach().float().reshape(-1), beta.detach().float().reshape(-1)[1:2]]).contiguous()
        code = L.DTYPE_CODE[dt]
        V = torch.empty((3, n, h, w, f), dtype=dt, device=dev)
        y = torch.empty_like(yin)
        st = L.stream_ptr
        L.launch("sr_nas_dw_fwd", L.lib().sr_nas_dw_fwd, yin.data_ptr(), V.data_ptr(), dwp.data_ptr(), n, h, w, f, code, st())
        L.launch("sr_nas_pw_fwd", L.lib().sr_nas_pw_fwd, yin.data_ptr(), V.data_ptr(), y.data_ptr(), frags.data_ptr(),
                 tabs.data_ptr(), scal.data_ptr(), n, h, w, f, code, st())
        ctx.save_for_backward(yin, V, dwp, frags, tabs, scal, mg.detach().float(), ms.detach().float(), p.detach().float(),
                              beta.detach().float())
        return y

    @staticmethod
    @_on_tensor_device
    def backward(ctx, gy):
        yin, V, dwp, frags, tabs, scal, mg, ms, p, beta = ctx.saved_tensors
        n, h, w, f = yin.shape
        dev, dt = yin.device, yin.dtype
        tb = _nas_dev_tables(f, dev.index if dev.index is not None else torch.cuda.current_device())
        code = L.DTYPE_CODE[dt]
        gy = gy.contiguous()
        wgs = int(os.environ.get("SR_NAS_WGS", 256))
        GZ = torch.empty_like(V)
        part_pw = torch.empty((wgs, tb["pw_slab"]), dtype=torch.float32, device=dev)
        part_dw = torch.empty((wgs, tb["dw_slab"]), dtype=torch.float32, device=dev)
        gyin = torch.empty_like(yin)
        st = L.stream_ptr
        L.launch("sr_nas_pw_bwd", L.lib().sr_nas_pw_bwd, yin.data_ptr(), V.data_ptr(), gy.data_ptr(), GZ.data_ptr(),
                 frags.data_ptr(), tabs.data_ptr(), scal.data_ptr(), part_pw.data_ptr(), wgs, n, h, w, f, code, st())
        L.launch("sr_nas_dw_bwd", L.lib().sr_nas_dw_bwd, yin.data_ptr(), GZ.data_ptr(), gy.data_ptr(), gyin.data_ptr(),
                 dwp.data_ptr(), part_dw.data_ptr(), wgs, n, h, w, f, code, st())
        L.launch("sr_nas_dw_wgrad", L.lib().sr_nas_dw_wgrad, yin.data_ptr(), GZ.data_ptr(), dwp.data_ptr(), part_dw.data_ptr(),
                 wgs, n, h, w, f, code, st())
        spw, sdw = part_pw.sum(0), part_dw.sum(0)
        g_wpw = spw.index_select(0, tb["g_wpw"]).view(3, f, f, 1, 1)
        g_bpw = spw.index_select(0, tb["g_bpw"]).view(3, f)
        r = spw.index_select(0, tb["g_r"]).view(3, f)                  # r_k[c] = sum gy[c] relu(u_k)[c]
        sxy = spw[tb["sxy"]]
        g_wdw = [sdw.index_select(0, tb["g_wdw"][i]).view(f, 1, k, k) for i, k in enumerate((3, 5, 7))]
        g_bdw = sdw.index_select(0, tb["g_bdw"]).view(3, f)
        sA, sB = sdw.index_select(0, tb["g_sA"]), sdw.index_select(0, tb["g_sB"])
        b2 = beta[1]
        q = (r * ms.view(1, f)).sum(1)                                  # q_k = sum_c ms[c] r_k[c]
        g_p = b2 * q
        g_beta = torch.stack([sxy, sxy + (p * q).sum()])
        g_ms = sA + b2 * (p.view(3, 1) * r).sum(0)
        g_mg = sB
        return gyin, g_wdw[0], g_wdw[1], g_wdw[2], g_bdw, g_wpw, g_bpw, g_mg, g_ms, g_p, g_beta


class _NasBodyFunction(torch.autograd.Function):
    """Every block of the supernet body in one autograd node: per block the same two forward / two backward kernels
    as _NasBlockFunction, but the parameter tables of all blocks are packed by a handful of batched ops (one cat,
    three gathers) and all gradients are gathered at once, instead of ~170 small launches per block.
    Inputs are stacked over blocks: WDWk (nb, F, 1, k, k), BDW / BPW (nb, 3, F), WPW (nb, 3, F, F, 1, 1), mg (F,),
    MS (nb, F), P (nb, 3), BETA (nb, 2); split = (forward, backward) flags of sr_nas_body_fwd / _bwd."""

    @staticmethod
    @_on_tensor_device
    def forward(ctx, y0, WDW3, WDW5, WDW7, BDW, WPW, BPW, mg, MS, P, BETA, split=(0, 0)):
        n, h, w, f = y0.shape
        nb = WDW3.shape[0]
        dev, dt = y0.device, y0.dtype
        tb = _nas_dev_tables(f, dev.index if dev.index is not None else torch.cuda.current_device())
        mgf, MSf = mg.detach().float(), MS.detach().float()
        src = torch.cat([WDW3.detach().float().reshape(nb, -1), WDW5.detach().float().reshape(nb, -1),
                         WDW7.detach().float().reshape(nb, -1), BDW.detach().float().reshape(nb, -1),
                         WPW.detach().float().reshape(nb, -1), BPW.detach().float().reshape(nb, -1),
                         mgf.reshape(1, f).expand(nb, f), MSf, mgf.reshape(1, f) * MSf,
                         _const(dev, (0.0, 1.0)).reshape(1, 2).expand(nb, 2)], dim=1)
        assert src.shape[1] == tb["off"]["size"]
        dwp = src.index_select(1, tb["dwp"])
        frags = src.index_select(1, tb["frags"]).to(dt)
        tabs = src.index_select(1, tb["tabs"])
        scal = torch.cat([P.detach().float(), BETA.detach().float()[:, 1:2]], dim=1).contiguous()
        code = L.DTYPE_CODE[dt]
        ys = torch.empty((nb + 1, n, h, w, f), dtype=dt, device=dev)
        ys[0] = y0
        V = torch.empty((nb, 3, n, h, w, f), dtype=dt, device=dev)
        L.launch("sr_nas_body_fwd", L.lib().sr_nas_body_fwd, ys.data_ptr(), V.data_ptr(), dwp.data_ptr(),
                 dwp.stride(0) * dwp.element_size(), frags.data_ptr(), frags.stride(0) * frags.element_size(), tabs.data_ptr(),
                 tabs.stride(0) * tabs.element_size(), scal.data_ptr(), scal.stride(0) * scal.element_size(), nb, n, h, w, f, code,
                 split[0], L.stream_ptr())                    # every block from ONE C call
        ctx.split_bwd = split[1]
        ctx.save_for_backward(ys, V, dwp, frags, tabs, scal, MSf, P.detach().float(), BETA.detach().float())
        return ys[nb]

    @staticmethod
    @_on_tensor_device
    def backward(ctx, gy):
        ys, V, dwp, frags, tabs, scal, MS, P, BETA = ctx.saved_tensors
        nb, n, h, w, f = V.shape[0], V.shape[2], V.shape[3], V.shape[4], V.shape[5]
        dev, dt = ys.device, ys.dtype
        tb = _nas_dev_tables(f, dev.index if dev.index is not None else torch.cuda.current_device())
        code = L.DTYPE_CODE[dt]
        wgs = int(os.environ.get("SR_NAS_WGS", 256))
        GZ = torch.empty_like(V[0])
        part_pw = torch.empty((nb, wgs, tb["pw_slab"]), dtype=torch.float32, device=dev)
        part_dw = torch.empty((nb, wgs, tb["dw_slab"]), dtype=torch.float32, device=dev)
        g = gy.contiguous()
        gbuf = [torch.empty_like(g), torch.empty_like(g)]
        import ctypes
        g_in = ctypes.c_void_p()
        L.launch("sr_nas_body_bwd", L.lib().sr_nas_body_bwd, ys.data_ptr(), V.data_ptr(), g.data_ptr(), gbuf[0].data_ptr(),
                 gbuf[1].data_ptr(), GZ.data_ptr(), dwp.data_ptr(), dwp.stride(0) * dwp.element_size(), frags.data_ptr(),
                 frags.stride(0) * frags.element_size(), tabs.data_ptr(), tabs.stride(0) * tabs.element_size(), scal.data_ptr(),
                 scal.stride(0) * scal.element_size(), part_pw.data_ptr(), part_pw.stride(0) * 4, part_dw.data_ptr(),
                 part_dw.stride(0) * 4, wgs, nb, n, h, w, f, code, ctx.split_bwd, ctypes.byref(g_in), L.stream_ptr())
        g = gbuf[0] if g_in.value == gbuf[0].data_ptr() else gbuf[1]
        spw, sdw = part_pw.sum(1), part_dw.sum(1)                                      # (nb, slab)
        g_wpw = spw.index_select(1, tb["g_wpw"]).view(nb, 3, f, f, 1, 1)
        g_bpw = spw.index_select(1, tb["g_bpw"]).view(nb, 3, f)
        r = spw.index_select(1, tb["g_r"]).view(nb, 3, f)                             # r_k[c] = sum gy[c] relu(u_k)[c]
        sxy = spw[:, tb["sxy"]]
        g_wdw = [sdw.index_select(1, tb["g_wdw"][i]).view(nb, f, 1, k, k) for i, k in enumerate((3, 5, 7))]
        g_bdw = sdw.index_select(1, tb["g_bdw"]).view(nb, 3, f)
        sA, sB = sdw.index_select(1, tb["g_sA"]), sdw.index_select(1, tb["g_sB"])      # (nb, F)
        b2 = BETA[:, 1]                                                                # (nb,)
        q = (r * MS.view(nb, 1, f)).sum(2)                                             # q_k = sum_c ms[c] r_k[c]
        g_p = b2.view(nb, 1) * q
        g_beta = torch.stack([sxy, sxy + (P * q).sum(1)], dim=1)
        g_ms = sA + b2.view(nb, 1) * (P.view(nb, 3, 1) * r).sum(1)
        g_mg = sB.sum(0)
        return g, g_wdw[0], g_wdw[1], g_wdw[2], g_bdw, g_wpw, g_bpw, g_mg, g_ms, g_p, g_beta, None


_PREP_CACHE = {}


def _nas_prep_dev_tables(Fch: int, nb: int, layout, device_index: int, blocks=None):
    """packing.nas_prep_tables on the device (cached per geometry, set of running blocks and device)"""
    key = (Fch, nb, layout, device_index, blocks)
    t = _PREP_CACHE.get(key)
    if t is None:
        if len(_PREP_CACHE) > 64:                       # (a search visits few block subsets; bound the cache anyway)
            _PREP_CACHE.clear()
        h = P.nas_prep_tables(Fch, nb, layout, blocks)
        base = P.nas_tables(Fch)
        dev = torch.device("cuda", device_index)
        t = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in h.items()}
        for k in ("dwp", "frags", "tabs"):
            t[k] = torch.from_numpy(np.ascontiguousarray(base[k], dtype=np.int32)).to(dev)
        t["bias_const"] = torch.zeros(h["bias_tab"].shape[0], dtype=torch.float32, device=dev)
        t["pw_slab"], t["dw_slab"] = base["pw_slab"], base["dw_slab"]
        _PREP_CACHE[key] = t
    return t


class _NasBodyNative(torch.autograd.Function):
    """_NasBodyFunction with the parameter plumbing native as well: weight-norm of the six convs of every block, the
    gathers into the kernels' operand tables, and on the way back the slab sums, the scatter into d(source) and the
    weight-norm backward straight into a gradient laid out like the flat parameter -- two launches each way
    (sr_param_pack / sr_param_grads, the kernels BASIC_MODEL's net calls use) instead of ~70 small torch launches.
    Inputs: flat (the body parameter), mg (F,), MS (nb, F), P (nb, 3), BETA (nb, 2), layout / frozen of the model."""

    @staticmethod
    @_on_tensor_device
    def forward(ctx, y0, flat, mg, MS, P_, BETA, layout, frozen, src_pre=None, scal_pre=None, nb_total=None, blocks=None,
                split=(0, 0)):
        n, h, w, f = y0.shape
        nb = MS.shape[0]
        dev, dt = y0.device, y0.dtype
        nbt = nb if nb_total is None else nb_total      # blocks of the model; `nb` of them (`blocks`) run
        tb = _nas_prep_dev_tables(f, nbt, layout, dev.index if dev.index is not None else torch.cuda.current_device(), blocks)
        o, size = tb["off"], tb["size"]
        mgf, MSf = mg.detach().float(), MS.detach().float()
        flatd = flat.detach()
        if src_pre is not None:                         # mask columns already written by sr_nas_scalars
            src = src_pre
        else:
            src = torch.empty((nb, size), dtype=torch.float32, device=dev)
            src[:, o["mg"]:o["zero"]] = torch.cat([mgf.reshape(1, f).expand(nb, f), MSf, mgf.reshape(1, f) * MSf], dim=1)
            src[:, o["zero"]:] = _const(dev, (0.0, 1.0))
        code = L.DTYPE_CODE[dt]
        dwp = torch.empty((nb, tb["dwp"].numel()), dtype=torch.float32, device=dev)
        frags = torch.empty((nb, tb["frags"].numel()), dtype=dt, device=dev)
        tabs = torch.empty((nb, tb["tabs"].numel()), dtype=torch.float32, device=dev)
        segs = (L.PackSeg * 3)(L.PackSeg(tb["dwp"].data_ptr(), dwp.data_ptr(), 0, size, dwp.shape[1], nb, 1),
                               L.PackSeg(tb["frags"].data_ptr(), frags.data_ptr(), 0, size, frags.shape[1], nb, 0),
                               L.PackSeg(tb["tabs"].data_ptr(), tabs.data_ptr(), 0, size, tabs.shape[1], nb, 1))
        L.launch("sr_param_pack", L.lib().sr_param_pack, flatd.data_ptr(), src.data_ptr(), tb["chan_tab"].data_ptr(),
                 tb["chan_tab"].shape[0], tb["bias_tab"].data_ptr(), tb["bias_const"].data_ptr(), tb["bias_tab"].shape[0], segs, 3,
                 code, L.stream_ptr())
        scal = scal_pre if scal_pre is not None else torch.cat([P_.detach().float(), BETA.detach().float()[:, 1:2]], dim=1).contiguous()
        ys = torch.empty((nb + 1, n, h, w, f), dtype=dt, device=dev)
        ys[0] = y0
        V = torch.empty((nb, 3, n, h, w, f), dtype=dt, device=dev)
        L.launch("sr_nas_body_fwd", L.lib().sr_nas_body_fwd, ys.data_ptr(), V.data_ptr(), dwp.data_ptr(),
                 dwp.stride(0) * dwp.element_size(), frags.data_ptr(), frags.stride(0) * frags.element_size(), tabs.data_ptr(),
                 tabs.stride(0) * tabs.element_size(), scal.data_ptr(), scal.stride(0) * scal.element_size(), nb, n, h, w, f, code,
                 split[0], L.stream_ptr())
        ctx.layout, ctx.frozen, ctx.nbt, ctx.blocks, ctx.split_bwd = layout, frozen, nbt, blocks, split[1]
        # the parameter values the weight-norm backward needs are the ones of THIS forward: keep a snapshot only if the
        # caller may write the parameter in place before backward (forward() itself rewrites beta1 / beta2, which no table names)
        ctx.save_for_backward(ys, V, dwp, frags, tabs, scal, MSf.contiguous(), P_.detach().float().contiguous(),
                              BETA.detach().float().contiguous(), flat)      # (eval: BETA is an expanded constant)
        return ys[nb]

    @staticmethod
    @_on_tensor_device
    def backward(ctx, gy):
        ys, V, dwp, frags, tabs, scal, MS, P_, BETA, flat = ctx.saved_tensors
        nb, n, h, w, f = V.shape[0], V.shape[2], V.shape[3], V.shape[4], V.shape[5]
        dev, dt = ys.device, ys.dtype
        tb = _nas_prep_dev_tables(f, ctx.nbt, ctx.layout, dev.index if dev.index is not None else torch.cuda.current_device(), ctx.blocks)
        code = L.DTYPE_CODE[dt]
        wgs = int(os.environ.get("SR_NAS_WGS", 256))
        GZ = torch.empty_like(V[0])
        part_pw = torch.empty((nb, wgs, tb["pw_slab"]), dtype=torch.float32, device=dev)
        part_dw = torch.empty((nb, wgs, tb["dw_slab"]), dtype=torch.float32, device=dev)
        g = gy.contiguous()
        gbuf = [torch.empty_like(g), torch.empty_like(g)]
        import ctypes
        g_in = ctypes.c_void_p()
        L.launch("sr_nas_body_bwd", L.lib().sr_nas_body_bwd, ys.data_ptr(), V.data_ptr(), g.data_ptr(), gbuf[0].data_ptr(),
                 gbuf[1].data_ptr(), GZ.data_ptr(), dwp.data_ptr(), dwp.stride(0) * dwp.element_size(), frags.data_ptr(),
                 frags.stride(0) * frags.element_size(), tabs.data_ptr(), tabs.stride(0) * tabs.element_size(), scal.data_ptr(),
                 scal.stride(0) * scal.element_size(), part_pw.data_ptr(), part_pw.stride(0) * 4, part_dw.data_ptr(),
                 part_dw.stride(0) * 4, wgs, nb, n, h, w, f, code, ctx.split_bwd, ctypes.byref(g_in), L.stream_ptr())
        g = gbuf[0] if g_in.value == gbuf[0].data_ptr() else gbuf[1]
        ds, ex = tb["ds"], tb["extra"]
        dsrc = torch.empty((nb, ds), dtype=torch.float32, device=dev)
        gflat = torch.zeros_like(flat)
        flatd = flat.detach()
        segs = (L.UnpackSeg * 2)(
            L.UnpackSeg(part_pw.data_ptr(), tb["pw_sidx"].data_ptr(), tb["pw_dst"].data_ptr(), 0, ds, tb["pw_slab"], wgs,
                        tb["pw_sidx"].numel(), nb),
            L.UnpackSeg(part_dw.data_ptr(), tb["dw_sidx"].data_ptr(), tb["dw_dst"].data_ptr(), 0, ds, tb["dw_slab"], wgs,
                        tb["dw_sidx"].numel(), nb))
        L.launch("sr_param_grads", L.lib().sr_param_grads, flatd.data_ptr(), dsrc.data_ptr(), gflat.data_ptr(),
                 tb["chan_bwd"].data_ptr(), tb["chan_bwd"].shape[0], tb["bias_bwd"].data_ptr(), tb["bias_bwd"].shape[0], segs, 2,
                 L.stream_ptr())
        for name, o_, n_, _shape in ctx.layout:                                        # kernel_grad(False) & co: frozen kinds
            if name in ctx.frozen and name.startswith("body."):
                gflat[o_:o_ + n_].zero_()
        # q_k = sum_c ms[c] r_k[c]; g_p = beta2 q; g_beta = (sxy, sxy + sum_k p_k q_k); g_ms = sA + beta2 sum_k p_k r_k;
        # g_mg = sum_b sB -- one launch over the extra columns of d(source)
        mgr = torch.empty(nb * (5 + f) + f, dtype=torch.float32, device=dev)
        L.launch("sr_nas_mask_grads", L.lib().sr_nas_mask_grads, dsrc.data_ptr(), ds, ex["r"], ex["sxy"], ex["sA"], ex["sB"],
                 MS.data_ptr(), P_.data_ptr(), BETA.data_ptr(), nb, f, mgr.data_ptr(), L.stream_ptr())
        g_p, g_beta = mgr[:3 * nb].view(nb, 3), mgr[3 * nb:5 * nb].view(nb, 2)
        g_ms, g_mg = mgr[5 * nb:5 * nb + nb * f].view(nb, f), mgr[5 * nb + nb * f:]
        return g, gflat, g_mg, g_ms, g_p, g_beta, None, None, None, None, None, None, None


class _GateFunction(torch.autograd.Function):
    """ConditionFunction over all blocks at once: (1,0) where alpha1 >= alpha2 else (0,1); straight-through."""

    @staticmethod
    def forward(ctx, A1, A2):
        b1 = (A1 >= A2).to(A1.dtype)
        return torch.stack([b1, 1.0 - b1], dim=1)                                      # (nb, 2)

    @staticmethod
    def backward(ctx, g):
        return g[:, 0], g[:, 1]


class _GateValues(torch.autograd.Function):
    """_GateFunction whose values came from sr_nas_scalars"""

    @staticmethod
    def forward(ctx, A1, A2, values):
        return values.clone()

    @staticmethod
    def backward(ctx, g):
        return g[:, 0], g[:, 1], None


class Split_Block(nn.Module):
    """reference wdsr_b.py:405-501 (block_type 'normal', seperate_type True)"""

    def __init__(self, num_residual_units, kernel_size=3, weight_norm=None, res_scale=1, width_search=False,
                 block_type="normal", seperate_type=True):
        super().__init__()
        if block_type != "normal" or not seperate_type:
            raise NotImplementedError("hot path supports Split_Block(block_type='normal', seperate_type=True)")
        self.num_residual_units = num_residual_units
        self.alpha = nn.Parameter(torch.ones(3))
        init.uniform_(self.alpha, 0.5, 1.5)
        self.beta = nn.Parameter(torch.zeros(3))
        self.split = BinaryConv2d(num_residual_units, num_residual_units, groups=num_residual_units, least_channel=0)
        self.kernel_list = ["3", "5", "7"]
        self.body = nn.ModuleDict()
        for k in self.kernel_list:
            self.body[k] = nn.Sequential(Conv_sep(num_residual_units, num_residual_units, int(k)), nn.Identity())

    def _branch_params(self):
        wdw = [self.body[k][0].body[0].weight() for k in self.kernel_list]
        bdw = torch.stack([self.body[k][0].body[0].bias for k in self.kernel_list])
        wpw = torch.stack([self.body[k][0].body[2].weight() for k in self.kernel_list])
        bpw = torch.stack([self.body[k][0].body[2].bias for k in self.kernel_list])
        return wdw, bdw, wpw, bpw

    def _run(self, yin, mg, beta):
        """yin NHWC hot tensor; mg (F,) global-mask values (ones outside NAS_MODEL); beta (2,) gate"""
        wdw, bdw, wpw, bpw = self._branch_params()
        p = F.softmax(self.alpha, dim=0)                      # implicit dim 0 in the reference (:487)
        return _NasBlockFunction.apply(yin, wdw[0], wdw[1], wdw[2], bdw, wpw, bpw, mg, self.split.effective(), p, beta)

    def forward_body(self, x):
        """NCHW fp32 in / out, as the reference's forward_body (:482-496)"""
        if not x.is_cuda:
            raise L.HotpathError("Split_Block (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
        dt = getattr(self, "hot_dtype", torch.float32)
        yin = x.permute(0, 2, 3, 1).to(dt).contiguous()
        y = self._run(yin, x.new_ones(self.num_residual_units), _const(x.device, (0.0, 1.0)))
        return y.permute(0, 3, 1, 2).float()

    def forward(self, x):
        return self.forward_body(x)


class MyAggregationLayer(Split_Block):
    """reference wdsr_b.py:503-554: Split_Block + hard skip/keep gate (alpha1/alpha2, beta1/beta2)"""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.alpha1 = nn.Parameter(torch.empty(1))
        self.beta1 = nn.Parameter(torch.zeros(1))
        init.uniform_(self.alpha1, 0, 0.2)
        self.alpha2 = nn.Parameter(torch.empty(1))
        self.beta2 = nn.Parameter(torch.ones(1))
        init.uniform_(self.alpha2, 0.8, 1)

    def _skipped(self) -> bool:
        """eval-time gate alpha1 >= alpha2 as a host bool, read back once per parameter version"""
        key = (self.alpha1.data_ptr(), self.alpha1._version, self.alpha2.data_ptr(), self.alpha2._version)
        if getattr(self, "_skip_key", None) != key:
            self._skip_val, self._skip_key = bool(self.alpha1 >= self.alpha2), key
        return self._skip_val

    def forward(self, y, mg, speed_curr, speed_accu):
        """y: NHWC hot tensor BEFORE the global mask; mg: (F,) effective global mask (applied in-kernel).
        Returns (y_out NHWC, speed_accu) with the reference's train / eval semantics (:517-546)."""
        if self.training:
            beta1, beta2 = ConditionFunction.apply(self.alpha1, self.alpha2, self.beta1, self.beta2)
            self.beta1.data, self.beta2.data = beta1.detach(), beta2.detach()
            out = self._run(y, mg, torch.cat([beta1, beta2]))
            return out, beta2 * speed_curr + speed_accu
        if self._skipped():
            out = (y.float() * mg.view(1, 1, 1, -1)).to(y.dtype)          # skipped block: only the global mask
        else:
            out = self._run(y, mg, _const(y.device, (0.0, 1.0)))
        return out, speed_accu + self.beta2 * speed_curr


class _SpeedMLP(nn.Module):
    """parameter holder of speed_models/SpeedModel.py:9-39 (6-layer MLP); loaded-but-unused at this commit"""

    def __init__(self, num_feat=3):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = nn.Linear(num_feat, 32), nn.Linear(32, 64), nn.Linear(64, 128)
        self.fc6, self.fc7, self.fc8 = nn.Linear(128, 64), nn.Linear(64, 32), nn.Linear(32, 1)
        for p in self.parameters():
            p.requires_grad = False


class BlockBSpeedEstimator(nn.Module):
    """latency head, host/PyTorch scalars (speed_models/speed_estimator.py): the closed form used at this commit"""

    def __init__(self, type):
        super().__init__()
        self.estimator = _SpeedMLP(3)
        self.type = type

    @torch.no_grad()
    def estimateByMyMask(self, module, block_mask):
        """sum_k (c_split + 0.2 c_mask) k^2 alpha_k / 40, alpha RAW (speed_estimator.py:57-76); both channel counts
        use rounding() with its default least_channel=8 (get_unmask_number, :79-83)."""
        c_mask = getattr(block_mask, "_c_mask_cached", None)          # NAS_MODEL.forward computes it once per call
        if c_mask is None:
            c_mask = rounding(block_mask.weight.detach()).sum()
        c_split = rounding(module.split.weight.detach()).sum()
        k2 = _const(module.alpha.device, (9.0, 25.0, 49.0))
        return ((c_split + 0.2 * c_mask) * k2 * module.alpha.detach() / 40).sum().reshape(1)

    @torch.no_grad()
    def estimateByChannelNum(self, x):
        return (x[1] + 0.2 * x[0]) * (x[2] * x[2]) / 40


def get_ori_speed(num_blocks=4, num_residual_units=12):
    """speed_models/helpers.py:5-15"""
    return float(num_blocks * (num_residual_units + 0.2 * num_residual_units) * 49 / 40)


class _HeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, f, dt, mean):
        blob = HP.pack_head(HP.head_src(w, b), f, dt)
        n, _, h, wd = x.shape
        y = torch.empty((n, h, wd, f), dtype=dt, device=x.device)
        HP.head_fwd(x, y, blob, mean)
        ctx.save_for_backward(x)
        ctx.mean, ctx.shape_w = mean, w.shape
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        g = HP.head_wgrad(gy.contiguous(), x, ctx.mean)
        nw = int(np.prod(ctx.shape_w))
        return None, g[:nw].view(ctx.shape_w), g[nw:nw + ctx.shape_w[0]], None, None, None


class _TailFunction(torch.autograd.Function):
    """tail conv + skip conv + PixelShuffle (reference wdsr_b.py:118-123).  A criterion of mobilesuperresolution_amd.training applied
    to this node's output folds the loss into the tail-backward kernel (models/loss_fold.py; `run_folded`): no d(loss)/d(out) tensor,
    none of the seven small ATen loss kernels."""

    @staticmethod
    def forward(ctx, feat, x, wt, ws, btot, r, mean):
        n, h, w, f = feat.shape
        blob = HP.pack_tail(HP.tail_src(wt, ws, btot), f, r, feat.dtype)
        out = torch.empty((n, 3, r * h, r * w), dtype=torch.float32, device=feat.device)
        HP.tail_fwd(feat, x, out, blob, mean, r)
        ctx.save_for_backward(feat, x, blob)
        ctx.r, ctx.mean, ctx.shapes = r, mean, (wt.shape, ws.shape)
        LF.arm(ctx, out)
        return out

    @staticmethod
    def run_folded(node, sr, hr, kind, gscale):
        """the tail's backward with d(loss)/d(out) formed in the kernel -> ((dfeat, g), the loss sums)"""
        feat, x, blob = node.saved_tensors
        dfeat, g, loss_part = HP.tail_bwd_loss(sr, hr, kind, gscale, feat, x, blob, node.mean, node.r)
        return (dfeat, g), loss_part

    @staticmethod
    def _split(ctx, dfeat, g):
        nt, ns = int(np.prod(ctx.shapes[0])), int(np.prod(ctx.shapes[1]))
        co = ctx.shapes[0][0]
        return dfeat, None, g[:nt].view(ctx.shapes[0]), g[nt:nt + ns].view(ctx.shapes[1]), g[nt + ns:nt + ns + co], None, None

    @staticmethod
    @_on_tensor_device
    def backward(ctx, dout):
        feat, x, blob = ctx.saved_tensors
        ctx.ran = True
        folded, only_token = LF.take_folded(ctx, dout)
        if only_token:
            return _TailFunction._split(ctx, *folded)
        dout = dout.contiguous().float()
        if feat.dtype == torch.bfloat16:
            dfeat, g = HP.tail_bwd(dout, feat, x, blob, ctx.mean, ctx.r)
        else:
            dfeat = torch.empty_like(feat)
            HP.tail_bwd_data(dout, dfeat, blob, ctx.r)
            g = HP.tail_wgrad(dout, feat, x, ctx.mean, ctx.r)
        if folded is not None:
            dfeat, g = dfeat + folded[0], g + folded[1]
        return _TailFunction._split(ctx, dfeat, g)


def _body_kinds(f: int):
    """(reference key suffix, per-block shape) of every tensor a MyAggregationLayer owns, in the reference's state_dict order
    (wdsr_b.py:419-431,375-402,505-515)"""
    kinds = [("alpha", (3,)), ("beta", (3,)), ("alpha1", (1,)), ("beta1", (1,)), ("alpha2", (1,)), ("beta2", (1,)),
             ("split.weight", (f, 1, 1, 1))]
    for k in (3, 5, 7):
        kinds += [(f"body.{k}.0.body.0.bias", (f,)), (f"body.{k}.0.body.0.weight_g", (f, 1, 1, 1)),
                  (f"body.{k}.0.body.0.weight_v", (f, 1, k, k)), (f"body.{k}.0.body.2.bias", (f,)),
                  (f"body.{k}.0.body.2.weight_g", (f, 1, 1, 1)), (f"body.{k}.0.body.2.weight_v", (f, f, 1, 1))]
    return kinds


class _SplitFlat(torch.autograd.Function):
    """flat body parameter -> one (nb, ...) tensor per kind.  Forward is ONE copy (the kinds are slices of it: later in-place
    writes into the parameter -- forward() rewrites beta1 / beta2 like the reference, :534 -- cannot disturb what autograd
    saved); backward is one fill plus a copy per kind that received a gradient (with the native plumbing of the convs
    that is the four mask / gate kinds).  `frozen`: kinds whose gradient is zeroed (length_grad / mask_grad / kernel_grad(False))."""

    @staticmethod
    def forward(ctx, flat, layout, frozen):
        ctx.layout, ctx.frozen = layout, frozen
        ctx.set_materialize_grads(False)               # kinds nothing used arrive as None, not as 20-odd zero fills
        snap = flat.detach().clone()
        outs = tuple(snap[o:o + n].view(shape) for (_, o, n, shape) in layout)
        ctx.mark_non_differentiable(*[t for t, (name, *_r) in zip(outs, layout) if name in frozen])
        return outs

    @staticmethod
    def backward(ctx, *grads):
        dev = next((g.device for g in grads if g is not None), None)
        if dev is None:
            return None, None, None
        total = ctx.layout[-1][1] + ctx.layout[-1][2]
        out = torch.zeros(total, dtype=torch.float32, device=dev)          # one fill, then only the kinds that have a gradient
        for g, (name, o, n, shape) in zip(grads, ctx.layout):
            if g is not None and name not in ctx.frozen:
                out[o:o + n] = g.reshape(-1)
        return out, None, None


class _Holder:
    """attribute bag of a block view"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _BlockView:
    """`model.body[i]` of the reference, as views into the flat body parameter: .alpha, .beta, .alpha1, .beta1, .alpha2,
    .beta2, .split.weight, .body['3'][0].body[0].{bias, weight_g, weight_v} ...  Reads and in-place writes (under no_grad)
    go straight to the parameter."""

    def __init__(self, model, i):
        self._m, self._i = model, i

    def _t(self, suffix):
        return self._m.kind(suffix)[self._i]

    def __getattr__(self, name):
        if name in ("alpha", "beta", "alpha1", "beta1", "alpha2", "beta2"):
            return self._t(name)
        if name == "split":
            return _Holder(weight=self._t("split.weight"))
        if name == "body":
            return {str(k): [_Holder(body=[_Holder(**{n: self._t(f"body.{k}.0.body.0.{n}") for n in ("bias", "weight_g", "weight_v")}),
                                           None,
                                           _Holder(**{n: self._t(f"body.{k}.0.body.2.{n}") for n in ("bias", "weight_g", "weight_v")})])]
                    for k in (3, 5, 7)}
        raise AttributeError(name)

    def _skipped(self) -> bool:
        return bool(self._m._skip_flags()[self._i])


class NAS_MODEL(nn.Module):
    """Parameters: head / tail / skip (weight-normalised convs, 3 tensors each), mask.weight, and ONE flat fp32 parameter
    `flat` that holds every tensor of the 16 search blocks, stacked over blocks kind by kind.  With one tensor per
    reference key (25 per block, 400 at C5) a training step spent most of its 5.4 ms in autograd's per-tensor
    bookkeeping, `cat` / `stack` backward splits and a 362-tensor Adam; the reference keys live on as views
    (`state_dict()` / `load_state_dict()` / `named_reference_tensors()` / `body[i].alpha1` ...)."""

    def __init__(self, params):
        super().__init__()
        self.image_mean = float(params.image_mean)
        self.scale = int(params.scale)
        self.num_blocks = int(params.num_blocks)
        self.num_residual_units = f = int(params.num_residual_units)
        self.remain_blocks = params.num_blocks
        self.width_search = bool(params.width_search)
        self.idx_kernel = [3, 5, 7]
        nin = int(params.num_channels)
        if nin != 3 or f not in (24, 32) or self.scale not in (2, 3, 4):
            raise NotImplementedError("MI355X hot path supports num_channels=3, num_residual_units in {24,32}, "
                                      f"scale in {{2,3,4}} (got {nin}, {f}, {self.scale})")
        if not self.width_search:
            # the reference's forward dereferences self.mask, which exists only with width_search (wdsr_b.py:74-77,116)
            raise NotImplementedError("NAS_MODEL(width_search=False) cannot run in the reference either "
                                      "(forward uses self.mask); construct it with width_search=True")
        self.hot_dtype = L.hot_dtype(getattr(params, "hot_dtype", None))
        # bf16 body: True runs a block's forward (resp. backward) as its separate kernels instead of the fused launch -- the
        # fp32 route's kernels, which the parity tests compare the fused ones against
        self.split_body_fwd = self.split_body_bwd = False
        nout = self.scale * self.scale * nin
        nb = self.num_blocks
        self.head = _WNConv(nin, f, 3, g_init=1.0, zero_bias=True)
        self.speed_estimator = BlockBSpeedEstimator("mask" if params.width_search else "channel").eval()
        # the reference's constructor calls, in the reference's order (same RNG draws), then laid out kind by kind
        blocks = [MyAggregationLayer(num_residual_units=f, kernel_size=3, res_scale=1 / math.sqrt(nb), width_search=True)
                  for _ in range(nb)]
        self._layout, off, vals = [], 0, []
        for suffix, shape in _body_kinds(f):
            n = nb * int(np.prod(shape))
            self._layout.append((suffix, off, n, (nb,) + tuple(shape)))
            vals.append(torch.stack([dict(b.named_parameters())[suffix].detach() for b in blocks]).reshape(-1).float())
            off += n
        self._layout = tuple(self._layout)
        self._kind_index = {name: i for i, (name, *_r) in enumerate(self._layout)}
        self.flat = nn.Parameter(torch.cat(vals))
        self._frozen = frozenset()
        self.body = [_BlockView(self, i) for i in range(nb)]          # views, not modules: nothing to register
        self.mask = BinaryConv2d(in_channels=f, out_channels=f, groups=f)
        self.tail = _WNConv(f, nout, 3, g_init=1.0, zero_bias=True)
        self.skip = _WNConv(nin, nout, 5, g_init=1.0, zero_bias=True)        # bare conv in NAS_MODEL: keys skip.*
        self.shuf = nn.Sequential()
        if getattr(params, "pretrained", False):
            self.load_pretrained(getattr(params, "pretrained_path", None))

    # ---- the reference's tensors as views ----
    def kind(self, suffix, source=None):
        """(nb, ...) view of one kind (e.g. 'alpha1', 'body.5.0.body.2.weight_v') over the flat parameter, or over any
        tensor laid out like it (its gradient)"""
        _, o, n, shape = self._layout[self._kind_index[suffix]]
        base = self.flat.detach() if source is None else source
        return base[o:o + n].view(shape)

    def named_reference_tensors(self, grads=False):
        """(reference state_dict key, tensor) in the reference's order: head.*, speed_estimator.*, body.{i}.*, mask.weight,
        tail.*, skip.*.  grads=True: the gradients instead (None where there is none)."""
        def own(prefix, mod):
            for n, p in mod.named_parameters():
                yield prefix + n, (p.grad if grads else p.detach())
        yield from own("head.", self.head)
        yield from own("speed_estimator.", self.speed_estimator)
        g = self.flat.grad
        for i in range(self.num_blocks):
            for suffix, *_r in self._layout:
                if grads:
                    yield f"body.{i}.{suffix}", (None if g is None else self.kind(suffix, g)[i])
                else:
                    yield f"body.{i}.{suffix}", self.kind(suffix)[i]
        yield "mask.weight", (self.mask.weight.grad if grads else self.mask.weight.detach())
        yield from own("tail.", self.tail)
        yield from own("skip.", self.skip)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        if destination is None:
            destination = OrderedDict()
        for k, v in self.named_reference_tensors():
            destination[prefix + k] = v
        return destination

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        mine = dict(self.named_reference_tensors())
        with torch.no_grad():
            for k, view in mine.items():
                key = prefix + k
                if key not in state_dict:
                    missing_keys.append(key)
                    continue
                src = state_dict[key]
                if tuple(src.shape) != tuple(view.shape):
                    error_msgs.append(f"size mismatch for {key}: checkpoint {tuple(src.shape)} vs model {tuple(view.shape)}")
                    continue
                view.copy_(src)
        for key in list(state_dict):
            if key.startswith(prefix) and key[len(prefix):] not in mine and key != prefix + "flat":
                unexpected_keys.append(key)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        missing, unexpected, errors = [], [], []
        self._load_from_state_dict(dict(state_dict), "", {}, strict, missing, unexpected, errors)
        if errors or (strict and (missing or unexpected)):
            raise RuntimeError("Error(s) in loading state_dict for NAS_MODEL:\n\t" +
                               "\n\t".join(errors + ([f"Missing key(s): {missing}"] if strict and missing else []) +
                                           ([f"Unexpected key(s): {unexpected}"] if strict and unexpected else [])))
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    @torch.no_grad()
    def load_pretrained(self, path=None):
        """reference wdsr_b.py:235-250: POSITIONAL copy -- walk the parameters in registration order and take the
        checkpoint's next tensor whenever the shapes agree (so a BASIC_MODEL checkpoint fills the head and nothing the
        search blocks own).  The walk is over the reference's tensors (named_reference_tensors), not over this class's
        flat parameter.  The reference reads `models/pretrained_weights/wdsr_b_x{scale}_{blocks}_{units}.pt` beside its
        own file; the same relative location is the default here, `path` (or params.pretrained_path) names the file
        otherwise.  Loaded with weights_only=True: nothing in the file is executed."""
        import os
        if path is None:
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pretrained_weights",
                                f"wdsr_b_x{self.scale}_{self.num_blocks}_{self.num_residual_units}.pt")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"--pretrained: no checkpoint at {path}; copy the reference's models/pretrained_weights/ "
                                    "there or pass params.pretrained_path")
        state_dict = torch.load(path, map_location="cpu", weights_only=True)
        items = iter(state_dict.items())
        try:
            _, load_param = next(items)
        except StopIteration:
            return 0
        taken = 0
        for _, view in self.named_reference_tensors():
            if view.size() == load_param.size():
                view.copy_(load_param.to(device=view.device, dtype=view.dtype))
                taken += 1
                try:
                    _, load_param = next(items)
                except StopIteration:
                    pass                              # (the reference keeps comparing against the last tensor, :247-250)
        return taken

    def gradless_parameters(self):
        """The reference registers `beta` (unused, wdsr_b.py:422) and `beta1` / `beta2` (ConditionFunction.backward returns
        None for them, :611-616) as requires_grad parameters that never receive a gradient: DistributedDataParallel
        without find_unused_parameters raises on its second iteration over them (SURVEY 8, C5 hazard).  Here they are
        slices of the flat parameter, whose gradient is simply zero there -- Adam leaves them alone, forward() rewrites
        beta1 / beta2 -- so there is nothing left to freeze."""
        return []

    def freeze_gradless_parameters(self):
        return []

    def forward(self, x):
        if not x.is_cuda:
            raise L.HotpathError("NAS_MODEL (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
        if x.device != self.flat.device:
            raise L.HotpathError(f"input on {x.device}, parameters on {self.flat.device}")
        with torch.cuda.device(x.device):
            return self._forward(x)

    def _forward(self, x):
        x = x.contiguous().float()
        f, dt = self.num_residual_units, self.hot_dtype
        y = _HeadFunction.apply(x, self.head.weight(), self.head.bias, f, dt, self.image_mean)
        sc = (self._scalars() if self.mask.least_channel == 8 and (self.num_blocks + 1) * self.num_residual_units <= 4096
              and not os.environ.get("SR_NAS_TORCH_PREP") else None)
        # once: the mask's value and the latency head's count
        mask_hard = sc["mask_hard"] if sc is not None else rounding(self.mask.weight.detach(), self.mask.least_channel)
        mg = self.mask.effective(mask_hard)
        y, speed_accu = self._body(y, mg, mask_hard, sc)
        # y = self.mask(y) before the tail (:118-119): the mask's value is exactly 0 / 1 per channel, so it is applied to the
        # tail conv's INPUT-channel weights (one op on 10 k weights, exact) instead of to the activations (three passes over
        # the feature map each way); the straight-through gradient reaches mask.weight through the product's autograd
        wt = self.tail.weight() * mg.view(1, -1, 1, 1)
        btot = self.tail.bias + self.skip.bias + self.image_mean
        out = _TailFunction.apply(y, x, wt, self.skip.weight(), btot, self.scale, self.image_mean)
        return out, speed_accu

    def _scalars(self):
        """0/1 masks, gates and latency terms of this step from one launch (csrc/nas_block.h nas_scalars_kernel): views
        mask_hard (F,1,1,1), ms_hard (nb, F), speed_curr (nb,), gates (nb, 2) of one buffer"""
        nb, f = self.num_blocks, self.num_residual_units
        fl = self.flat.detach()
        off = P.nas_tables(f)["off"]
        out = torch.empty(f + 1 + nb * (f + 4), dtype=torch.float32, device=fl.device)
        # the operand-source rows of the body (their mask columns are written here, the weights by sr_param_pack) and the
        # per-block kernel scalars softmax(alpha) | gate2
        src = torch.empty((nb, off["size"]), dtype=torch.float32, device=fl.device)
        scal = torch.empty((nb, 4), dtype=torch.float32, device=fl.device)
        with torch.cuda.device(fl.device):
            L.launch("sr_nas_scalars", L.lib().sr_nas_scalars, self.mask.weight.detach().data_ptr(),
                     self.kind("split.weight", fl).data_ptr(), self.kind("alpha", fl).data_ptr(), self.kind("alpha1", fl).data_ptr(),
                     self.kind("alpha2", fl).data_ptr(), nb, f, out.data_ptr(), src.data_ptr(), src.stride(0), off["mg"],
                     scal.data_ptr(), L.stream_ptr(fl.device))
        o = f + 1
        return dict(mask_hard=out[:f].view(f, 1, 1, 1), ms_hard=out[o:o + nb * f].view(nb, f),
                    speed_curr=out[o + nb * (f + 1):o + nb * (f + 2)], gates=out[o + nb * (f + 2):].view(nb, 2), src=src, scal=scal)

    def _skip_flags(self):
        """eval-time gates alpha1 >= alpha2 of all blocks as host bools, read back once per parameter version"""
        key = (self.flat.data_ptr(), self.flat._version)
        if getattr(self, "_skip_key", None) != key:
            self._skip_val = (self.kind("alpha1") >= self.kind("alpha2")).reshape(-1).tolist()
            self._skip_key = key
        return self._skip_val

    def _body(self, y, mg, mask_hard=None, sc=None):
        """All MyAggregationLayer blocks (reference wdsr_b.py:111-117 with :517-546 per block) through ONE autograd node:
        weight-norm, masks, gates, softmax and the latency terms are a few batched ops over the stacked kinds.
        Returns (y NHWC, speed_accu (1,))."""
        nball, f = self.num_blocks, self.num_residual_units
        K = dict(zip((name for name, *_r in self._layout), _SplitFlat.apply(self.flat, self._layout, self._frozen)))
        dev = y.device
        skipped = [] if self.training else self._skip_flags()
        idx = [i for i in range(nball) if not (skipped and skipped[i])]   # eval: a skipped block only applies the (idempotent 0/1) global mask
        # latency head, reference speed_estimator.py:57-76 (raw alpha, rounding() with its default least_channel = 8)
        if sc is not None:
            speed_curr = sc["speed_curr"]
        else:
            with torch.no_grad():
                c_mask = (rounding(self.mask.weight.detach()) if mask_hard is None or self.mask.least_channel != 8 else mask_hard).sum()
                W = K["split.weight"].detach().view(nball, -1)                                           # (NB, F)
                hard = (W >= 0.5).float()
                top8 = ((W.unsqueeze(1) > W.unsqueeze(2)).sum(2) < 8).float()  # W >= 8th largest of its row (ties kept), as rounding()
                c_split = torch.where(hard.sum(1, keepdim=True) >= 8, hard, top8).sum(1)
                A = K["alpha"].detach()                                                                  # (NB, 3)
                speed_curr = ((c_split + 0.2 * c_mask).view(-1, 1) * _const(dev, (9.0, 25.0, 49.0)).view(1, 3) * A / 40).sum(1)
        if self.training:
            if sc is not None:
                gates = _GateValues.apply(K["alpha1"].view(-1), K["alpha2"].view(-1), sc["gates"])
            else:
                gates = _GateFunction.apply(K["alpha1"].view(-1), K["alpha2"].view(-1))
            gd = gates.detach()
            self.kind("beta1", self.flat.data).copy_(gd[:, 0:1])                                     # reference :521-523,:534
            self.kind("beta2", self.flat.data).copy_(gd[:, 1:2])
            speed_accu = (gates[:, 1] * speed_curr).sum().reshape(1)
        else:
            gates = None
            speed_accu = (K["beta2"].view(-1) * speed_curr).sum().reshape(1)
        if not idx:
            return y, speed_accu
        nbk = len(idx)
        if nbk != nball:
            it = torch.tensor(idx, device=dev)
            K = {k: v.index_select(0, it) for k, v in K.items()}

        SW = K["split.weight"].view(nbk, -1)                                                         # (nb, F)
        SWd = SW.detach()
        hard = sc["ms_hard"] if sc is not None and nbk == nball else (SWd >= 0.5).float()
        MS = SW - (SWd - hard)                                   # BinaryConv2d(least_channel=0): value 0/1, gradient 1
        P = F.softmax(K["alpha"], dim=1)
        if self.training:
            BETA = gates
        else:
            BETA = _const(dev, (0.0, 1.0)).view(1, 2).expand(nbk, 2)
        if not os.environ.get("SR_NAS_TORCH_PREP"):
            # weight-norm / packing / gradient gathers native too (two launches each way); eval: only the blocks that run
            pre = (sc["src"], sc["scal"] if self.training else None) if sc is not None and nbk == nball else (None, None)
            return _NasBodyNative.apply(y, self.flat, mg, MS, P, BETA, self._layout, self._frozen, *pre, nball,
                                        None if nbk == nball else tuple(idx), self._body_split()), speed_accu

        def wn(k, j):                                # weight-normalised conv j (0 depthwise, 2 pointwise) of branch k
            v, g = K[f"body.{k}.0.body.{j}.weight_v"], K[f"body.{k}.0.body.{j}.weight_g"]
            return torch._weight_norm(v.reshape(nbk * f, *v.shape[2:]), g.reshape(nbk * f, 1, 1, 1), 0).view(v.shape)
        WDW = [wn(k, 0) for k in (3, 5, 7)]
        WPW = torch.stack([wn(k, 2) for k in (3, 5, 7)], dim=1)                                      # (nb, 3, F, F, 1, 1)
        BDW = torch.stack([K[f"body.{k}.0.body.0.bias"] for k in (3, 5, 7)], dim=1)                  # (nb, 3, F)
        BPW = torch.stack([K[f"body.{k}.0.body.2.bias"] for k in (3, 5, 7)], dim=1)
        y = _NasBodyFunction.apply(y, WDW[0], WDW[1], WDW[2], BDW, WPW, BPW, mg, MS, P, BETA, self._body_split())
        return y, speed_accu

    def _body_split(self):
        return int(self.split_body_fwd), int(self.split_body_bwd)

    # ---- search-control surface used by search.py:83-87,292,331-337,374-380 ----
    @torch.no_grad()
    def get_current_blocks(self):
        return int((self.kind("alpha1") < self.kind("alpha2")).sum())

    @torch.no_grad()
    def get_block_status(self):
        a = F.softmax(torch.stack([self.kind("alpha1"), self.kind("alpha2")], dim=0), dim=0)
        return [i for i, keep in enumerate((a[0] < a[1]).reshape(-1).tolist()) if keep]

    @torch.no_grad()
    def get_width_from_block_idx(self, remain_block_idx):
        all_width = []
        for idx, m in enumerate(self.body):
            if idx in remain_block_idx:
                width = [int(rounding(self.mask.weight).sum()),
                         int((rounding(self.mask.weight) * rounding(m.split.weight)).sum())]
                _, max_index = torch.max(m.alpha, 0)
                width.append(self.idx_kernel[max_index])
                all_width.append(width)
        return all_width

    @torch.no_grad()
    def get_alpha_grad(self):
        g = self.flat.grad
        return (None, None) if g is None else (self.kind("alpha1", g)[0], self.kind("alpha2", g)[0])

    @torch.no_grad()
    def get_alpha(self):
        return self.kind("alpha1")[0], self.kind("alpha2")[0]

    def _set_frozen(self, names, frozen):
        cur = set(self._frozen)
        cur = (cur | set(names)) if frozen else (cur - set(names))
        self._frozen = frozenset(cur)

    @torch.no_grad()
    def length_grad(self, flag=False):
        """reference :573-577 toggles requires_grad of alpha1 / alpha2 / beta1 / beta2 of every block; here the kinds'
        gradient slices are zeroed instead (a fresh Adam, as search.py builds after every toggle, then never moves them)"""
        self._set_frozen(("alpha1", "alpha2", "beta1", "beta2"), not flag)

    @torch.no_grad()
    def mask_grad(self, flag=False):
        self._set_frozen(("split.weight",), not flag)
        self.mask.weight.requires_grad = flag

    @torch.no_grad()
    def kernel_grad(self, flag=False):
        a = self.kind("alpha", self.flat.data)
        a.copy_(F.one_hot(a.argmax(dim=1), 3).to(a.dtype))
        self._set_frozen(("alpha",), not flag)

    @torch.no_grad()
    def get_mask_grad(self):
        return self.mask.weight.grad

    @torch.no_grad()
    def get_mask_weight(self):
        return self.mask.weight.data
