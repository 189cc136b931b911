"""MotionVectorVSR on the MI355X hot path (reference: models/mvvsr_arch.py:11-109; the trainer's 'basic_mv' model,
train_video_superresolution.py:251 constructs `MotionVectorVSR(num_feat=20, num_block=8, spynet_path=...)`).

Same constructor, forward signature `forward(x_, height, weight)` and state_dict keys (`backward_trunk.main.*`,
`forward_trunk.main.*`, `fusion.*`, `upconv1.*`, `upconv2.*`, `conv_hr.*`, `conv_last.*`).  The two recurrent propagation loops
(flow_warp -> concat -> ConvResidualBlocks trunk, mvvsr_arch.py:72-93) run in HIP (csrc/conv3x3.h, csrc/conv64.h).

The reconstruction behind them (:95-105: cat -> 1x1 fusion -> LeakyReLU -> ConvTranspose2d(2F, 3, 5, stride 4) -> bilinear resize ->
+ bilinear base) has two routes.  The HIP route (csrc/mv_recon.h) takes a call whose tensors are on the GPU, whose output size is
(4h, 4w), whose trunks run on the fused route (paired, when a graph is recorded), whose input does not require grad, with no hook on `fusion`, `conv_last` or
the trunks, and with `MotionVectorVSR.aten_reconstruction` unset.  Under no_grad it reads the trunks' NHWC state handles
(sr_mv_recon_fwd, any F <= 64); when a graph is recorded (F <= 24, or 24 < F <= 64 with `hot_training` set) ONE autograd.Function
spans the n per-step state tensors and the four parameters: sr_mv_recon_fwd saves the fused activation u, sr_mv_recon_bwd (F <= 24)
or sr_mv_recon_bwd64 (24 < F <= 64) returns the state gradients in the layout the trunk's backward consumes and the parameter
gradients through fixed-order slab sums -- no ATen convolution, no atomic, two runs agree bit for bit.  Every other call keeps the
reference's ATen loop, line for line.

`hot_training` (class default False; the convention of the two video networks) matters at 24 < F <= 64 only: setting it on a model
opts the two wide trunks in as well (set_wide_training(model, on)) and sends a graph-recording call that meets the conditions above
through the HIP reconstruction.  set_wide_training(model) alone keeps the HIP trunks with the ATen reconstruction.

`upconv1/2`, `conv_hr` and `pixel_shuffle` are constructed and never used, as in the reference.  SPyNet is out of scope: the
reference constructs it and never calls it in this model (flows are the motion vectors in channels 3..4 of the input, :63-67);
`spynet.*` keys of a reference checkpoint are accepted and ignored."""
from __future__ import annotations

import torch
from torch import nn as nn
from torch.nn import functional as F

from functools import lru_cache

from .. import _lib as L
from .. import packing as P
from .basicvsr_arch import ConvResidualBlocks, _fusable, _records_graph, paired, propagate, set_wide_training
from .spynet_arch import flow_warp

__all__ = ["MotionVectorVSR"]


@lru_cache(maxsize=None)
def _recon_pack(num_feat: int, device_index: int):
    """packing.mv_recon_tables on the device: (pack index, state channels per pixel)"""
    cw = P.mv_recon_cw(num_feat)
    return torch.from_numpy(P.mv_recon_tables(num_feat, cw)["pack"]).to(torch.device("cuda", device_index)), cw


_BWD_WGS = 128                                       # workgroups (= fp32 slabs) of sr_mv_recon_bwd per 16 frames
_BWD64_WGS = 256                                     # of sr_mv_recon_bwd64: one workgroup per CU (130 KB of LDS each)


@lru_cache(maxsize=None)
def _recon_bwd_pack(num_feat: int, device_index: int):
    """packing.mv_recon_bwd_tables' pack index on the device"""
    return torch.from_numpy(P.mv_recon_bwd_tables(num_feat)["pack"]).to(torch.device("cuda", device_index))


def _ptrs(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _frames(x_):
    """the (b, n, 5, h, w) input as sr_mv_recon_fwd reads its RGB planes: fp32 with a dense (3, h, w) block per frame"""
    _, _, _, h, w = x_.shape
    x_ = x_.detach()
    if x_.dtype != torch.float32 or x_.stride()[2:] != (h * w, w, 1):
        x_ = x_.float().contiguous()
    return x_


def _recon_fwd(mod, fb, ff, x_, u_save=None):
    """sr_mv_recon_fwd over the clip: fb / ff = per-frame (b, h, w, cw) state images"""
    b, n, _, h, w = x_.shape
    dt, dev = mod.backward_trunk.hot_dtype, x_.device
    blob, cw = mod._recon_blob(dt)
    for t in fb + ff:
        if t.shape != (b, h, w, cw) or t.dtype != dt or not t.is_contiguous():
            raise ValueError("MotionVectorVSR reconstruction: the trunks' (b, h, w, cw) state images in the hot dtype")
    xs = _frames(x_)
    out = torch.empty((b, n, 3, 4 * h, 4 * w), dtype=torch.float32, device=dev)
    L.launch("sr_mv_recon_fwd", L.lib().sr_mv_recon_fwd, _ptrs(fb), _ptrs(ff), cw, xs.data_ptr(), xs.stride(0), xs.stride(1),
             blob.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1), u_save.data_ptr() if u_save is not None else None,
             n, b, h, w, L.DTYPE_CODE[dt], L.stream_ptr(dev))
    return out


class _ReconFunction(torch.autograd.Function):
    """the whole clip's reconstruction as one node: inputs = the n per-step state tensors of propagate(step_states=True) and the
    four parameters; saved = the fused activation u (one 48- or 128-channel hot-dtype image per frame)"""

    @staticmethod
    def forward(ctx, mod, x_, w_fu, b_fu, w_last, b_last, *steps):
        b, n, _, h, w = x_.shape
        dt = mod.backward_trunk.hot_dtype
        cw = P.mv_recon_cw(mod.num_feat)
        if len(steps) != n or any(s.shape != (2 * b, h, w, cw) for s in steps):
            if cw == 24:
                raise ValueError("MotionVectorVSR reconstruction with a backward: the n (2b, h, w, 24) step states of the 24-wide trunks")
            raise ValueError("MotionVectorVSR reconstruction with a backward: the n (2b, h, w, 64) step states of the 64-wide trunks")
        with torch.cuda.device(x_.device):
            steps = [s.detach() for s in steps]
            fb = [steps[n - 1 - i][:b] for i in range(n)]
            ff = [steps[i][b:] for i in range(n)]
            u = torch.empty((n, b, h, w, 2 * cw), dtype=dt, device=x_.device)
            out = _recon_fwd(mod, fb, ff, x_, u)
        # plain attributes, not save_for_backward, as _TrunkWarpFunction keeps its activations: `steps` are views of the trunk
        # Function's `acts` (and the next step's state input), which nothing on the hot path writes in place; autograd's version
        # check therefore does not cover them
        ctx.mod, ctx.geom, ctx.u, ctx.steps = mod, (b, n, h, w), u, steps
        ctx.blob = mod._recon_blob(dt)[0] if cw == 24 else mod._recon_bwd_blob(dt)
        return out

    @staticmethod
    def backward(ctx, g):
        mod, (b, n, h, w), u, steps = ctx.mod, ctx.geom, ctx.u, ctx.steps
        dt, dev, f = mod.backward_trunk.hot_dtype, u.device, mod.num_feat
        with torch.cuda.device(dev):
            g = g.contiguous().float()
            fb = [steps[n - 1 - i][:b] for i in range(n)]
            ff = [steps[i][b:] for i in range(n)]
            dsteps = [torch.empty_like(s) for s in steps]
            dfb = [dsteps[n - 1 - i][:b] for i in range(n)]
            dff = [dsteps[i][b:] for i in range(n)]
            lib = L.lib()
            if f <= 24:
                name, fn, wgs, slab = "sr_mv_recon_bwd", lib.sr_mv_recon_bwd, _BWD_WGS, lib.sr_mv_recon_slab()
            else:
                name, fn, wgs, slab = "sr_mv_recon_bwd64", lib.sr_mv_recon_bwd64, _BWD64_WGS, lib.sr_mv_recon_slab64()
            parts = torch.empty((-(-n // 16) * wgs, slab), dtype=torch.float32, device=dev)
            f2 = 2 * f
            grads = torch.empty(f2 * f2 + f2 + f2 * 75 + 3, dtype=torch.float32, device=dev)
            L.launch(name, fn, _ptrs(fb), _ptrs(ff), u.data_ptr(), g.data_ptr(), g.stride(0), g.stride(1),
                     ctx.blob.data_ptr(), _ptrs(dfb), _ptrs(dff), parts.data_ptr(), wgs, grads.data_ptr(), f, n, b, h, w,
                     L.DTYPE_CODE[dt], L.stream_ptr(dev))
        o1, o2, o3 = f2 * f2, f2 * f2 + f2, f2 * f2 + f2 + f2 * 75
        return (None, None, grads[:o1].view(f2, f2, 1, 1), grads[o1:o2], grads[o2:o3].view(f2, 3, 5, 5), grads[o3:]) + tuple(dsteps)


class _IgnoresSpynetKeys:
    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for k in [k for k in state_dict if k.startswith(prefix + "spynet.")]:
            del state_dict[k]                        # out-of-scope optical-flow prior of the reference checkpoint
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class MotionVectorVSR(_IgnoresSpynetKeys, nn.Module):
    # True: the ATen reconstruction (the reference's loop) for every call
    aten_reconstruction = False
    # 24 < F <= 64: True = a graph-recording call trains through the HIP trunks AND the HIP reconstruction (setting it opts the two
    # wide trunks in as well); False = the trunks' own rule (they refuse, or, after set_wide_training, train with the ATen
    # reconstruction).  F <= 24 trains in HIP either way.
    hot_training = False

    def __setattr__(self, name, value):
        if name == "hot_training":
            value = bool(value)
            set_wide_training(self, value)               # no wide trunk at F <= 24: nothing to set
            object.__setattr__(self, name, value)
            return
        super().__setattr__(name, value)

    def __init__(self, num_feat=64, num_block=15, spynet_path=None, hot_dtype=None):
        super().__init__()
        self.num_feat = num_feat
        self.scale = 4
        # propagation (hot path)
        self.backward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block, hot_dtype=hot_dtype)
        self.forward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block, hot_dtype=hot_dtype)
        # reconstruction (same layers, same construction order as mvvsr_arch.py:33-41)
        self.fusion = nn.Conv2d(num_feat * 2, num_feat * 2, 1, 1, 0, bias=True)
        self.upconv1 = nn.Conv2d(num_feat, num_feat * 4, 3, 1, 1, bias=True)
        self.upconv2 = nn.Conv2d(num_feat, num_feat * 4, 3, 1, 1, bias=True)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.ConvTranspose2d(num_feat * 2, 3, 5, stride=self.scale)
        self.pixel_shuffle = nn.PixelShuffle(2)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)

    def forward(self, x_, height=1080, weight=1920):
        """x_: (b, n, 5, h, w) = RGB frames + motion vectors (mvvsr_arch.py:57-67) -> (b, n, 3, height, weight)"""
        x = x_[:, :, :3, :, :]
        mv = x_[:, :, 3:, :, :]
        flows_forward = mv[:, 1:, :, :]
        flows_backward = flows_forward * (-1)
        b, n, _, h, w = x.size()
        if self._hot_reconstruction(x_, height, weight):
            return self._forward_hot(x_, x, flows_forward, flows_backward)
        feat_b, feat_f = propagate(x, flows_forward, flows_backward, self.backward_trunk, self.forward_trunk, flow_warp,
                                   num_feat=self.num_feat)
        out_l = []
        for i in range(n):
            out = torch.cat([feat_b[i], feat_f[i]], dim=1)
            out = self.lrelu(self.fusion(out))
            out = self.conv_last(out)
            out = F.interpolate(out, size=(height, weight), mode='bilinear')
            base = F.interpolate(x[:, i], size=(height, weight), mode='bilinear', align_corners=False)
            out_l.append(out + base)
        return torch.stack(out_l, dim=1)

    # ---- the HIP reconstruction (csrc/mv_recon.h) ----
    def _recon_params(self):
        return [self.fusion.weight, self.fusion.bias, self.conv_last.weight, self.conv_last.bias]

    def _hooked(self):
        """a hook on a layer the HIP route never calls (fusion, conv_last) or whose output it does not produce (the trunks' NCHW
        features): such a call keeps the ATen route, where the hooks fire as before"""
        names = ("_forward_hooks", "_forward_pre_hooks", "_backward_hooks", "_backward_pre_hooks")
        return any(getattr(m, a, None) for m in (self.fusion, self.conv_last, self.backward_trunk, self.forward_trunk) for a in names)

    def _records_graph(self, x_):
        return _records_graph([self.backward_trunk, self.forward_trunk, self.fusion, self.conv_last], x_)

    def _hot_reconstruction(self, x_, height, weight):
        b, n, _, h, w = x_.shape
        if self.aten_reconstruction or not x_.is_cuda or (height, weight) != (4 * h, 4 * w) or x_.requires_grad or self._hooked():
            return False
        if not all(p.is_cuda and p.device == x_.device for p in self._recon_params()):
            return False
        if not (_fusable(self.backward_trunk) and _fusable(self.forward_trunk)):
            return False
        if not self._records_graph(x_):              # state handles: paired or one direction after the other, either width
            return True
        return self._graph_route_hot()

    def _graph_route_hot(self):
        """the rule of a graph-recording call, tensors aside.  It needs the backward and the per-step states of the paired route
        (SR_VSR_SEPARATE_DIRECTIONS=1 trains through the ATen reconstruction); at 24 < F <= 64 it is opt-in (`hot_training`, with
        both trunks opted in): without it the 64-wide trunks refuse such a call themselves or, after set_wide_training alone, train
        with the ATen reconstruction"""
        if not paired(self.backward_trunk, self.forward_trunk):
            return False
        if not self.backward_trunk.wide:
            return True
        return self.hot_training and self.backward_trunk.hot_training and self.forward_trunk.hot_training

    def _recon_blob(self, dt):
        """(the two layers' MFMA-fragment weights and their transposes in one buffer, cw); re-packed only when a parameter changed"""
        ps = self._recon_params()
        key = (dt,) + tuple((p.data_ptr(), p._version) for p in ps)
        dev = ps[0].device
        pack, cw = _recon_pack(self.num_feat, dev.index if dev.index is not None else torch.cuda.current_device())
        if getattr(self, "_rblob_key", None) != key:
            flat = torch.cat([p.detach().reshape(-1).float() for p in ps] + [torch.zeros(1, device=dev)])
            self._rblob = flat.index_select(0, pack).to(dt)
            self._rblob_key = key
        return self._rblob, cw

    def _recon_bwd_blob(self, dt):
        """the backward's own blob at 24 < F <= 64 (packing.mv_recon_bwd_tables: wlb | wfut), cached like `_recon_blob`"""
        ps = self._recon_params()
        key = (dt,) + tuple((p.data_ptr(), p._version) for p in ps)
        dev = ps[0].device
        if getattr(self, "_rbblob_key", None) != key:
            pack = _recon_bwd_pack(self.num_feat, dev.index if dev.index is not None else torch.cuda.current_device())
            flat = torch.cat([p.detach().reshape(-1).float() for p in ps] + [torch.zeros(1, device=dev)])
            self._rbblob = flat.index_select(0, pack).to(dt)
            self._rbblob_key = key
        return self._rbblob

    def __getstate__(self):
        d = self.__dict__.copy()
        for k in ("_rblob", "_rblob_key", "_rbblob", "_rbblob_key"):
            d.pop(k, None)
        return d

    def _forward_hot(self, x_, x, flows_forward, flows_backward):
        b, n, _, h, w = x.size()
        if self._records_graph(x_):
            steps = propagate(x, flows_forward, flows_backward, self.backward_trunk, self.forward_trunk, flow_warp,
                              num_feat=self.num_feat, step_states=True)
            return _ReconFunction.apply(self, x_, *self._recon_params(), *steps)
        with torch.no_grad(), torch.cuda.device(x_.device):
            hb, hf = propagate(x, flows_forward, flows_backward, self.backward_trunk, self.forward_trunk, flow_warp,
                               num_feat=self.num_feat, handles=True)
            return _recon_fwd(self, [t.contiguous() for t in hb], [t.contiguous() for t in hf], x_)
