"""SpyNet and flow_warp on the MI355X hot path (reference: models/spynet_arch.py -- the vendored, BasicSR-derived copy of the
mmedit functions the BasicVSR variants call at basicvsr_arch.py:24,74,85 / basicvsr_arch_origin.py:25).

`flow_warp` (:98-129): bilinear / zeros / align_corners=True in HIP (csrc/flow_warp.h), forward and backward.

`SpyNet` (:28-96): same constructor, parameter names (`basic_module.{level}.basic_module.{0,2,4,6,8}.{weight,bias}`, buffers
`mean`, `std`) and `forward(ref, supp)`.  The five 7x7 convolutions of every pyramid level -- where SPyNet's arithmetic is, 2.6
GFLOP per 64 x 64 frame pair -- run as implicit-GEMM MFMA kernels (csrc/spynet_conv.h, bf16 operands, fp32 accumulation, one
launch per layer, NHWC between layers); the pyramid's glue between them (average pooling, the x2 bilinear flow upsampling, the
border-padded warp of the 3-channel support image, normalisation, concatenation: a few KB to a few MB per level) is torch
tensor plumbing.

By default SpyNet is inference only: the reference's trainer keeps it out of the optimizer
(train_video_superresolution.py:160-163), so `forward` runs under no_grad and returns a flow without history.  Fine-tuning is
opt-in: with `SpyNet.hot_training = True` a call that would record a graph (grad mode on and a SpyNet parameter or an input
requiring grad) runs every BasicModule call as one autograd.Function -- the forward kernels as they are, with the bf16 layer
inputs kept, and the backward of the five convolutions in HIP (sr_conv7_module_bwd: backward-data on the rotated, role-swapped
weights with the saved ReLU mask, weight and bias gradients by partial slabs and one reduction, no float atomics).  The
pyramid's glue stays torch code and autograd differentiates it as it is.  `SpyNet.train_route_reason(ref, supp)` says why a call
would not take that route; a refused call keeps the default (a flow without history), which is documented and not an error."""
from __future__ import annotations

import ctypes
import math
from functools import lru_cache

import torch
from torch import nn as nn
from torch.nn import functional as F

from .. import _lib as L
from .. import packing as P

__all__ = ["flow_warp", "SpyNet", "BasicModule"]


class _FlowWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flow):
        n, c, h, w = x.shape
        with torch.cuda.device(x.device):
            out = torch.empty_like(x)
            L.launch("sr_flow_warp_fwd", L.lib().sr_flow_warp_fwd, x.data_ptr(), flow.data_ptr(), out.data_ptr(), n, c, h, w,
                     L.stream_ptr())
        ctx.save_for_backward(x, flow)
        return out

    @staticmethod
    def backward(ctx, g):
        x, flow = ctx.saved_tensors
        n, c, h, w = x.shape
        with torch.cuda.device(x.device):
            g = g.contiguous().float()
            dx = torch.zeros_like(x) if ctx.needs_input_grad[0] else None
            df = torch.empty_like(flow) if ctx.needs_input_grad[1] else None
            L.launch("sr_flow_warp_bwd", L.lib().sr_flow_warp_bwd, x.data_ptr(), flow.data_ptr(), g.data_ptr(),
                     dx.data_ptr() if dx is not None else None, df.data_ptr() if df is not None else None, n, c, h, w,
                     L.stream_ptr())
        return dx, df


def flow_warp(x, flow, interp_mode="bilinear", padding_mode="zeros", align_corners=True):
    """x: (n, c, h, w); flow: (n, h, w, 2).  Only the reference's defaults are on the hot path."""
    if (interp_mode, padding_mode, align_corners) != ("bilinear", "zeros", True):
        raise NotImplementedError("hot path flow_warp supports bilinear / zeros / align_corners=True only")
    if not x.is_cuda:
        raise L.HotpathError("flow_warp (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
    if x.device != flow.device:
        raise L.HotpathError(f"x on {x.device}, flow on {flow.device}")
    assert x.shape[-2:] == flow.shape[1:3]
    return _FlowWarp.apply(x.contiguous().float(), flow.contiguous().float())


def _border_warp(x, flow_nchw):
    """flow_warp(x, flow.permute(0, 2, 3, 1), padding_mode='border') of spynet_arch.py:73-75 on a 3-channel pyramid image (glue:
    torch's grid_sample, as the reference calls it)"""
    n, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(0, h, device=x.device, dtype=x.dtype), torch.arange(0, w, device=x.device, dtype=x.dtype),
                            indexing="ij")
    vx = 2.0 * (gx + flow_nchw[:, 0]) / max(w - 1, 1) - 1.0
    vy = 2.0 * (gy + flow_nchw[:, 1]) / max(h - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((vx, vy), dim=3), mode="bilinear", padding_mode="border", align_corners=True)


_LAYERS = ((8, 32, True), (32, 64, True), (64, 32, True), (32, 16, True), (16, 2, False))


@lru_cache(maxsize=None)
def _bwd_tables(device_index):
    """per layer: (conv7_bwd_tables' gather index, the weight gradient's sidx, dst) on the device"""
    dev = torch.device("cuda", device_index)
    out = []
    for cin, cout, _ in _LAYERS:
        wg = P.conv7_wgrad_tables(cin, cout)
        out.append((torch.from_numpy(P.conv7_bwd_tables(cin, cout)["idx"]).to(dev), torch.from_numpy(wg["sidx"]).to(dev),
                    torch.from_numpy(wg["dst"]).to(dev)))
    return tuple(out)


def _conv7_chain(x, packed, n, h, w, dev):
    """the five forward launches on x (n, h, w, 8) bf16: [x_0 = x, x_1 .. x_4 (bf16 layer inputs), y (n, h, w, 2) fp32]"""
    xs = [x]
    for (cin, cout, relu), (wp, bias) in zip(_LAYERS, packed):
        last = cout == 2
        y = torch.empty((n, h, w, cout), dtype=torch.float32 if last else torch.bfloat16, device=dev)
        L.launch("sr_conv7_fwd", L.lib().sr_conv7_fwd, xs[-1].data_ptr(), wp.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, w, cin,
                 cout, 1 if relu else 0, 1 if last else 0, L.stream_ptr(dev))
        xs.append(y)
    return xs


class _BasicModuleFunction(torch.autograd.Function):
    """one BasicModule call on the training route: forward = the inference launches with the bf16 layer inputs kept; backward =
    sr_conv7_module_bwd.  Inputs: the 8-channel NCHW fp32 image, the module, its ten parameters (weight, bias per layer)."""

    @staticmethod
    def forward(ctx, inp, mod, *params):
        n, _, h, w = inp.shape
        dev = inp.device
        with torch.cuda.device(dev):
            xs = _conv7_chain(inp.detach().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16), mod._pack(dev), n, h, w, dev)
        ctx.xs, ctx.weights, ctx.geom = xs[:5], [p.detach() for p in params[0::2]], (n, h, w)
        return xs[5].permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dflow):
        n, h, w = ctx.geom
        dev = dflow.device
        with torch.cuda.device(dev):
            tabs = _bwd_tables(dev.index if dev.index is not None else torch.cuda.current_device())
            g4 = torch.zeros((n, h, w, 8), dtype=torch.bfloat16, device=dev)      # the flow gradient, rounded once, 2 -> 8 channels
            g4[..., :2] = dflow.permute(0, 2, 3, 1)
            g = [torch.empty((n, h, w, cout), dtype=torch.bfloat16, device=dev) for _, cout, _ in _LAYERS[:4]] + [g4]
            dx0 = torch.empty((n, h, w, 8), dtype=torch.float32, device=dev)
            wts = [torch.cat([wt.float().reshape(-1), wt.new_zeros(1, dtype=torch.float32)]).index_select(0, t[0]).to(torch.bfloat16)
                   for wt, t in zip(ctx.weights, tabs)]
            gflat = [torch.empty(cout * cin * 49 + cout, dtype=torch.float32, device=dev) for cin, cout, _ in _LAYERS]
            wgs = P.conv7_wgrad_wgs(n, h, w)
            partial = torch.empty(wgs * max(P.conv7_wgrad_tables(cin, cout)["slab"] for cin, cout, _ in _LAYERS), dtype=torch.float32,
                                  device=dev)
            m = L.Conv7ModuleBwd()
            for l in range(5):
                m.x[l], m.g[l], m.wpacked_t[l] = ctx.xs[l].data_ptr(), g[l].data_ptr(), wts[l].data_ptr()
                m.sidx[l], m.dst[l], m.gflat[l] = tabs[l][1].data_ptr(), tabs[l][2].data_ptr(), gflat[l].data_ptr()
            m.partial, m.dx0 = partial.data_ptr(), dx0.data_ptr()
            L.launch("sr_conv7_module_bwd", L.lib().sr_conv7_module_bwd, ctypes.byref(m), wgs, n, h, w, L.stream_ptr(dev))
        grads = []
        for (cin, cout, _), gf in zip(_LAYERS, gflat):
            grads += [gf[:cout * cin * 49].view(cout, cin, 7, 7), gf[cout * cin * 49:]]
        return (dx0.permute(0, 3, 1, 2), None, *grads)


class BasicModule(nn.Module):
    """spynet_arch.py:10-25: Conv 7x7 8 -> 32 -> 64 -> 32 -> 16 -> 2, ReLU between; keys basic_module.{0,2,4,6,8}.*"""

    def __init__(self):
        super().__init__()
        self.basic_module = nn.Sequential(
            nn.Conv2d(8, 32, 7, 1, 3), nn.ReLU(inplace=False), nn.Conv2d(32, 64, 7, 1, 3), nn.ReLU(inplace=False),
            nn.Conv2d(64, 32, 7, 1, 3), nn.ReLU(inplace=False), nn.Conv2d(32, 16, 7, 1, 3), nn.ReLU(inplace=False),
            nn.Conv2d(16, 2, 7, 1, 3))
        self._packed = None

    def _pack(self, dev):
        """the five layers' weights as MFMA fragments (bf16) + padded biases; re-made when a parameter changed"""
        convs = [self.basic_module[i] for i in (0, 2, 4, 6, 8)]
        key = tuple((c.weight.data_ptr(), c.weight._version, c.bias._version) for c in convs) + (str(dev),)
        if self._packed is None or self._packed[0] != key:
            out = []
            for c, (cin, cout, _) in zip(convs, _LAYERS):
                tab = P.conv7_tables(cin, cout)
                src = torch.cat([c.weight.detach().float().reshape(-1), torch.zeros(1, device=dev)])
                idx = torch.from_numpy(tab["idx"]).to(dev)
                bias = torch.zeros(tab["mt"] * 32, device=dev)
                bias[:cout] = c.bias.detach().float()
                out.append((src.index_select(0, idx).to(torch.bfloat16).contiguous(), bias))
            self._packed = (key, out)
        return self._packed[1]

    def forward(self, tensor_input):
        """(N, 8, H, W) fp32 -> (N, 2, H, W) fp32"""
        if not tensor_input.is_cuda:
            raise L.HotpathError("SpyNet (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
        n, _, h, w = tensor_input.shape
        dev = tensor_input.device
        packed = self._pack(dev)
        x = tensor_input.detach().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
        with torch.cuda.device(dev):
            x = _conv7_chain(x, packed, n, h, w, dev)[5]
        return x.permute(0, 3, 1, 2)

    def forward_train(self, tensor_input):
        """the same values with history: (N, 8, H, W) fp32 -> (N, 2, H, W) fp32 through _BasicModuleFunction"""
        if not tensor_input.is_cuda:
            raise L.HotpathError("SpyNet (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
        convs = [self.basic_module[i] for i in (0, 2, 4, 6, 8)]
        return _BasicModuleFunction.apply(tensor_input.float(), self, *[p for c in convs for p in (c.weight, c.bias)])


class SpyNet(nn.Module):
    """spynet_arch.py:28-96.  `hot_training` (class default False): see the module docstring and train_route_reason()."""

    hot_training = False

    def __init__(self, load_path=None):
        super().__init__()
        self.basic_module = nn.ModuleList([BasicModule() for _ in range(6)])
        if load_path:
            self.load_state_dict(torch.load(load_path, map_location="cpu", weights_only=True)["params"])
        self.register_buffer("mean", torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))

    def preprocess(self, tensor_input):
        return (tensor_input - self.mean) / self.std

    def process(self, ref, supp, train=False):
        ref = [self.preprocess(ref)]
        supp = [self.preprocess(supp)]
        for _ in range(5):
            ref.insert(0, F.avg_pool2d(input=ref[0], kernel_size=2, stride=2, count_include_pad=False))
            supp.insert(0, F.avg_pool2d(input=supp[0], kernel_size=2, stride=2, count_include_pad=False))
        flow = ref[0].new_zeros([ref[0].size(0), 2, int(math.floor(ref[0].size(2) / 2.0)), int(math.floor(ref[0].size(3) / 2.0))])
        for level in range(len(ref)):
            up = F.interpolate(input=flow, scale_factor=2, mode="bilinear", align_corners=True) * 2.0
            if up.size(2) != ref[level].size(2):
                up = F.pad(input=up, pad=[0, 0, 0, 1], mode="replicate")
            if up.size(3) != ref[level].size(3):
                up = F.pad(input=up, pad=[0, 1, 0, 0], mode="replicate")
            module = self.basic_module[level].forward_train if train else self.basic_module[level]
            flow = module(torch.cat([ref[level], _border_warp(supp[level], up), up], 1)) + up
        return flow

    def train_route_reason(self, ref, supp):
        """None when this call runs on the HIP training route (a flow with history), else a short reason why it keeps the
        default: a flow without history, computed under no_grad"""
        if not self.hot_training:
            return "hot_training is not set"
        if not torch.is_grad_enabled():
            return "grad mode is off"
        if not (ref.requires_grad or supp.requires_grad or any(p.requires_grad for p in self.parameters())):
            return "nothing requires grad"
        if not (ref.is_cuda and supp.is_cuda):
            return "CPU tensors"
        return None

    def forward(self, ref, supp):
        if self.train_route_reason(ref, supp) is None:
            return self._forward(ref, supp, True)
        with torch.no_grad():
            return self._forward(ref, supp, False)

    def _forward(self, ref, supp, train):
        assert ref.size() == supp.size()
        h, w = ref.size(2), ref.size(3)
        w_floor = math.floor(math.ceil(w / 32.0) * 32.0)
        h_floor = math.floor(math.ceil(h / 32.0) * 32.0)
        ref = F.interpolate(input=ref, size=(h_floor, w_floor), mode="bilinear", align_corners=False)
        supp = F.interpolate(input=supp, size=(h_floor, w_floor), mode="bilinear", align_corners=False)
        flow = F.interpolate(input=self.process(ref, supp, train), size=(h, w), mode="bilinear", align_corners=False)
        if train:                                          # the same two products, out of place
            return flow * flow.new_tensor([float(w) / float(w_floor), float(h) / float(h_floor)]).view(1, 2, 1, 1)
        flow[:, 0, :, :] *= float(w) / float(w_floor)
        flow[:, 1, :, :] *= float(h) / float(h_floor)
        return flow
