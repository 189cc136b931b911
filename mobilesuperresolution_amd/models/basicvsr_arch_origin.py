"""BasicVSR_origin on the MI355X hot path (reference: models/basicvsr_arch_origin.py:10-95).

Same constructor, state_dict keys and `forward(x, height, weight)`; the propagation loops (:61-82) run in HIP like
MotionVectorVSR's.  The reconstruction (:84-93: fusion, upconv1/2 + PixelShuffle(2), conv_hr, conv_last, + the bilinear x4
base) has two routes.  A call that records no autograd graph (torch.no_grad(), or nothing requires grad) runs it in HIP in the
trunks' hot dtype (csrc/vsr_recon.h via sr_c64_recon_fwd): the two trunks' NHWC state images are read directly, the shuffles and
activations are epilogues, and each frame lands in its slice of the preallocated result.  A call that records a graph keeps the
ATen convolutions with the standalone HIP shuffle (csrc/pixel_shuffle.h, bit-exact), which have a backward; so does a call while
a forward hook sits on one of the five reconstruction layers (the HIP route does not call them);
`BasicVSR_origin.aten_reconstruction = True` forces that route for every call.

`hot_training` (class default False; MotionVectorVSR's convention) matters at 24 < F <= 64 only: setting it on a model calls
`set_wide_training(model, on)`, and a graph-recording call that meets `_hot_training_route` then runs the whole reconstruction in HIP
both ways (csrc/vsr_recon_bwd.h via sr_c64_recon_bwd): ONE autograd.Function over the clip reads the trunks' per-step states and hands
their gradients back in the same layout.  Without it such a call does what it did: the trunks refuse, or, after
`set_wide_training(model)` alone, train with the ATen reconstruction.

`flow_training` (class default False; a second opt-in on top of `hot_training`): setting it on a model calls
`set_flow_training(model, on)`, and the HIP training route then returns the gradient of the flows (csrc/conv64_bwd.h,
c64_warp_dflow_kernel), whether they were given as leaves or computed by a SpyNet that trains (`spynet.hot_training`).  Without it
a flow that requires grad is refused by the wide trunks, as before.

Flows: `get_flow` (:42-51) runs SpyNet on every adjacent frame pair in both directions, as the reference does; SpyNet's 7x7
convolutions are MFMA kernels (models/spynet_arch.py, csrc/spynet_conv.h; inference only -- the reference's trainer keeps SPyNet
out of the optimizer).  Flows may also be GIVEN: `forward(x, height, weight, flows=(flows_forward, flows_backward))` with
(b, n-1, 2, h, w) tensors, or -- as MotionVectorVSR takes them -- as motion-vector channels 3..4 of a 5-channel input."""
from __future__ import annotations

import torch
from torch import nn as nn
from torch.nn import functional as F
from functools import lru_cache

from .. import _lib as L
from .. import packing as P
from .basicvsr_arch import ConvResidualBlocks, _inner_contiguous, _records_graph, paired, propagate, set_flow_training, set_wide_training
from .spynet_arch import SpyNet, flow_warp

__all__ = ["BasicVSR_origin", "pixel_shuffle"]


class _PixelShuffle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r):
        n, c, h, w = x.shape
        if c % (r * r):
            raise ValueError(f"pixel_shuffle: {c} channels not divisible by {r * r}")
        out = torch.empty((n, c // (r * r), h * r, w * r), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            L.launch("sr_pixel_shuffle", L.lib().sr_pixel_shuffle, x.data_ptr(), out.data_ptr(), n, c // (r * r), h, w, r, 0,
                     L.stream_ptr(x.device))
        ctx.r = r
        return out

    @staticmethod
    def backward(ctx, g):
        r = ctx.r
        g = g.contiguous().float()
        n, c, hr, wr = g.shape
        dx = torch.empty((n, c * r * r, hr // r, wr // r), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            L.launch("sr_pixel_shuffle", L.lib().sr_pixel_shuffle, g.data_ptr(), dx.data_ptr(), n, c, hr // r, wr // r, r, 1,
                     L.stream_ptr(g.device))
        return dx, None


def pixel_shuffle(x: torch.Tensor, r: int) -> torch.Tensor:
    """nn.PixelShuffle(r) on the hot path (NCHW fp32, bit-exact); no CPU fallback"""
    if not x.is_cuda:
        raise L.HotpathError("pixel_shuffle (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
    return _PixelShuffle.apply(x.contiguous().float(), int(r))


@lru_cache(maxsize=None)
def _recon_tables(num_feat: int, device_index: int):
    """packing.c64_recon_tables on the device: (pack index, blob offsets as a C long array)"""
    import ctypes
    t = P.c64_recon_tables(num_feat)
    return torch.from_numpy(t["pack"]).to(torch.device("cuda", device_index)), (ctypes.c_long * 5)(*t["boff"])


RECON_ALL = 31                                       # sr_c64_recon_fwd `stages`: all five layers
_RECON_BWD_WGS = 128                                 # weight-gradient workgroups (= slabs) per section of sr_c64_recon_bwd; not swept


@lru_cache(maxsize=None)
def _recon_bwd_tables(num_feat: int, device_index: int):
    """packing.c64_recon_bwd_tables on the device: (pack index, blob offsets as a C long array, reduce table)"""
    import ctypes
    t = P.c64_recon_bwd_tables(num_feat)
    dev = torch.device("cuda", device_index)
    return torch.from_numpy(t["pack"]).to(dev), (ctypes.c_long * 6)(*t["boff"]), torch.from_numpy(t["reduce"]).to(dev)


def recon_scratch(b, h, w, dt, dev):
    """the four images of one frame's reconstruction: fused, up1, up2, hr (also the shapes of d_fused, d_up1, d_up2, d_hr)"""
    return (torch.empty((b, h, w, 64), dtype=dt, device=dev), torch.empty((b, 2 * h, 2 * w, 64), dtype=dt, device=dev),
            torch.empty((b, 4 * h, 4 * w, 64), dtype=dt, device=dev), torch.empty((b, 4 * h, 4 * w, 64), dtype=dt, device=dev))


class _ReconTrainFunction(torch.autograd.Function):
    """the whole clip's reconstruction as one node: inputs = the ten reconstruction parameters and the n per-step state tensors of
    propagate(step_states=True), (2b, h, w, 64); frame i reads steps[n - 1 - i][:b] and steps[i][b:].  Kept for the backward: the
    four post-activation images of every frame (37 h w 64 elements per clip-frame in the hot dtype); the LeakyReLU masks are the
    signs of these stored outputs."""

    @staticmethod
    def forward(ctx, mod, x, *args):
        params, steps = args[:10], args[10:]
        b, n, _, h, w = x.shape
        dt, dev = mod.backward_trunk.hot_dtype, x.device
        if len(steps) != n or any(s.shape != (2 * b, h, w, 64) or s.dtype != dt for s in steps):
            raise ValueError("BasicVSR_origin reconstruction with a backward: the n (2b, h, w, 64) step states of the 64-wide trunks")
        with torch.cuda.device(dev):
            steps = [s.detach() for s in steps]
            out = torch.empty((b, n, 3, 4 * h, 4 * w), dtype=torch.float32, device=dev)
            saved = []
            for i in range(n):
                saved.append(mod.reconstruct_hot(steps[n - 1 - i][:b], steps[i][b:], x[:, i], out[:, i], recon_scratch(b, h, w, dt, dev)))
        # plain attributes, as MotionVectorVSR's node keeps them: `steps` are views of the trunk Function's activations
        ctx.mod, ctx.geom, ctx.saved, ctx.steps = mod, (b, n, h, w), saved, steps
        ctx.blob = mod._recon_bwd_blob(dt)
        return out

    @staticmethod
    def backward(ctx, g):
        mod, (b, n, h, w), saved, steps = ctx.mod, ctx.geom, ctx.saved, ctx.steps
        dt, dev, f = mod.backward_trunk.hot_dtype, g.device, mod.num_feat
        with torch.cuda.device(dev):
            g = g.float()
            if g.stride()[2:] != (16 * h * w, 4 * w, 1):
                g = g.contiguous()
            lib = L.lib()
            _, boff, table = _recon_bwd_tables(f, dev.index if dev.index is not None else torch.cuda.current_device())
            dsteps = [torch.empty_like(s) for s in steps]
            dimg = recon_scratch(b, h, w, dt, dev)           # d_fused, d_up1, d_up2, d_hr: reused by every frame
            wgs = _RECON_BWD_WGS
            parts = torch.empty(wgs * lib.sr_c64_recon_bwd_slab(), dtype=torch.float32, device=dev)
            grads = torch.empty(table.numel(), dtype=torch.float32, device=dev)
            st = L.stream_ptr(dev)
            for i in range(n):
                fused, up1, up2, hr = saved[i]
                gi = g[:, i]
                L.launch("sr_c64_recon_bwd", lib.sr_c64_recon_bwd, steps[n - 1 - i][:b].data_ptr(), steps[i][b:].data_ptr(),
                         fused.data_ptr(), up1.data_ptr(), up2.data_ptr(), hr.data_ptr(), gi.data_ptr(), gi.stride(0),
                         ctx.blob.data_ptr(), boff, dimg[3].data_ptr(), dimg[2].data_ptr(), dimg[1].data_ptr(), dimg[0].data_ptr(),
                         dsteps[n - 1 - i][:b].data_ptr(), dsteps[i][b:].data_ptr(), parts.data_ptr(), wgs, b, h, w, L.DTYPE_CODE[dt],
                         RECON_ALL, st)
                L.launch("sr_c64_recon_reduce", lib.sr_c64_recon_reduce, parts.data_ptr(), wgs, table.data_ptr(), table.numel(),
                         grads.data_ptr(), int(i > 0), b, h, w, st)
                saved[i] = None
        out, o = [], 0
        for _, shape in P.c64_recon_shapes(f):
            k = 1
            for d in shape:
                k *= d
            out.append(grads[o:o + k].view(shape))
            o += k
        return (None, None) + tuple(out) + tuple(dsteps)


class BasicVSR_origin(nn.Module):
    # True: the ATen reconstruction (the route of a graph-recording call) for every call, also under no_grad
    aten_reconstruction = False
    # 24 < F <= 64: True = a graph-recording call trains through the HIP trunks AND the HIP reconstruction (setting it opts the two
    # wide trunks in as well); False = the trunks' own rule (they refuse, or, after set_wide_training, train with the ATen
    # reconstruction).  At F <= 24 it changes nothing.
    hot_training = False
    # 24 < F <= 64, on top of hot_training: True = flows that require grad (given as leaves, or SpyNet's under its own hot_training)
    # receive their gradient from the HIP route (setting it sets `flow_training` on the two wide trunks); False = such a call does
    # what it did: the trunks refuse the flow.
    flow_training = False

    def __setattr__(self, name, value):
        if name == "hot_training":
            value = bool(value)
            set_wide_training(self, value)               # no wide trunk at F <= 24: nothing to set
            object.__setattr__(self, name, value)
            return
        if name == "flow_training":
            value = bool(value)
            set_flow_training(self, value)
            object.__setattr__(self, name, value)
            return
        super().__setattr__(name, value)

    def __init__(self, num_feat=64, num_block=15, spynet_path=None, hot_dtype=None):
        super().__init__()
        self.num_feat = num_feat
        self.spynet = SpyNet(spynet_path)            # alignment (basicvsr_arch_origin.py:25)
        self.scale = 4
        self.backward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block, hot_dtype=hot_dtype)
        self.forward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block, hot_dtype=hot_dtype)
        # reconstruction: same layers, same construction order as basicvsr_arch_origin.py:30-35
        self.fusion = nn.Conv2d(num_feat * 2, num_feat, 1, 1, 0, bias=True)
        self.upconv1 = nn.Conv2d(num_feat, num_feat * 4, 3, 1, 1, bias=True)
        self.upconv2 = nn.Conv2d(num_feat, 64 * 4, 3, 1, 1, bias=True)
        self.conv_hr = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_last = nn.Conv2d(64, 3, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)

    def get_flow(self, x):
        """basicvsr_arch_origin.py:42-51"""
        b, n, c, h, w = x.size()
        x_1 = x[:, :-1, :, :, :].reshape(-1, c, h, w)
        x_2 = x[:, 1:, :, :, :].reshape(-1, c, h, w)
        flows_backward = self.spynet(x_1, x_2).view(b, n - 1, 2, h, w)
        flows_forward = self.spynet(x_2, x_1).view(b, n - 1, 2, h, w)
        return flows_forward, flows_backward

    def forward(self, x, height, weight, flows=None):
        if flows is None:
            if x.shape[2] != 5:
                flows = self.get_flow(x)
            else:                                    # motion vectors ride in channels 3..4, as MotionVectorVSR takes them
                mv = x[:, :, 3:, :, :]
                x = x[:, :, :3, :, :]
                flows = (mv[:, 1:, :, :], mv[:, 1:, :, :] * (-1))
        flows_forward, flows_backward = flows
        b, n, _, h, w = x.size()
        if x.is_cuda and not self.aten_reconstruction and not self._recon_hooked() and \
                not _records_graph(self._graph_modules(), x, flows_forward, flows_backward):
            return self._forward_hot(x, flows_forward, flows_backward, height, weight)
        if self._hot_training_route(x, flows_forward, flows_backward, height, weight)[0]:
            steps = propagate(x, flows_forward, flows_backward, self.backward_trunk, self.forward_trunk, flow_warp,
                              num_feat=self.num_feat, step_states=True)
            return _ReconTrainFunction.apply(self, x, *self._recon_params(), *steps)
        feat_b, feat_f = propagate(x, flows_forward, flows_backward, self.backward_trunk, self.forward_trunk, flow_warp,
                                   num_feat=self.num_feat)
        out_l = []
        for i in range(n):
            out = torch.cat([feat_b[i], feat_f[i]], dim=1)
            out = self.lrelu(self.fusion(out))
            out = self.lrelu(pixel_shuffle(self.upconv1(out), 2))
            out = self.lrelu(pixel_shuffle(self.upconv2(out), 2))
            out = self.lrelu(self.conv_hr(out))
            out = self.conv_last(out)
            base = F.interpolate(x[:, i], scale_factor=4, mode='bilinear', align_corners=False)
            out = out + base
            out = F.interpolate(out, size=(height, weight), mode='bilinear')
            out_l.append(out)
        return torch.stack(out_l, dim=1)

    def _graph_modules(self):
        """the modules whose parameters a forward with these flows touches: the trunks and the reconstruction (SPyNet reaches the
        result only through the flows, which are checked as inputs)"""
        return [self.backward_trunk, self.forward_trunk] + [getattr(self, name) for name in P.C64_RECON_LAYERS]

    def _recon_hooked(self):
        """a forward (pre-)hook on a reconstruction layer: the HIP route never calls these modules, so such a call keeps the ATen
        route, where the hooks fire"""
        return any(m._forward_hooks or m._forward_pre_hooks for m in (getattr(self, name) for name in P.C64_RECON_LAYERS))

    def _hot_training_route(self, x, flows_forward, flows_backward, height, weight):
        """the rule of a graph-recording call: (True, "hot") when it runs the HIP reconstruction forward and backward, else
        (False, the first condition that fails); such a call then does what it did before the route existed"""
        b, n, _, h, w = x.shape
        if not 24 < self.num_feat <= 64:
            return False, "num_feat <= 24 trains on the 24-wide route"
        if not self.hot_training:
            return False, "hot_training is not set"
        if not (getattr(self.backward_trunk, "hot_training", False) and getattr(self.forward_trunk, "hot_training", False)):
            return False, "hot_training is not set on both trunks"
        if not paired(self.backward_trunk, self.forward_trunk):
            return False, "the trunks are not paired"
        if (height, weight) != (4 * h, 4 * w):
            return False, "(height, weight) != (4h, 4w)"
        flow_grad = flows_forward.requires_grad or flows_backward.requires_grad
        if x.requires_grad or (flow_grad and not (getattr(self.backward_trunk, "flow_training", False) and
                                                  getattr(self.forward_trunk, "flow_training", False))):
            return False, "x or a flow requires grad"
        if self.aten_reconstruction:
            return False, "aten_reconstruction is set"
        if self._recon_hooked():
            return False, "a hook sits on a reconstruction layer"
        if not (x.is_cuda and flows_forward.is_cuda and flows_backward.is_cuda and
                all(p.is_cuda and p.device == x.device for p in self._recon_params())):
            return False, "the tensors are not on the GPU"
        return True, "hot"

    def _recon_bwd_blob(self, dt):
        """the backward's blob (packing.c64_recon_bwd_tables: the transposed weights), cached like `_recon_blob`"""
        ps = self._recon_params()
        key = (dt,) + tuple((p.data_ptr(), p._version) for p in ps)
        if getattr(self, "_rbblob_key", None) != key:
            dev = ps[0].device
            pack = _recon_bwd_tables(self.num_feat, dev.index if dev.index is not None else torch.cuda.current_device())[0]
            flat = torch.cat([p.detach().reshape(-1).float() for p in ps] + [torch.zeros(1, device=dev)])
            self._rbblob = flat.index_select(0, pack).to(dt)
            self._rbblob_key = key
        return self._rbblob

    def _recon_params(self):
        return [p for name in P.C64_RECON_LAYERS for p in (getattr(self, name).weight, getattr(self, name).bias)]

    def _recon_blob(self, dt):
        """the five reconstruction layers' MFMA-fragment weights in one buffer, re-packed only when a parameter changed"""
        ps = self._recon_params()
        key = (dt,) + tuple((p.data_ptr(), p._version) for p in ps)
        if getattr(self, "_rblob_key", None) != key:
            dev = ps[0].device
            pack, _ = _recon_tables(self.num_feat, dev.index if dev.index is not None else torch.cuda.current_device())
            flat = torch.cat([p.detach().reshape(-1).float() for p in ps] + [torch.zeros(1, device=dev)])
            self._rblob = flat.index_select(0, pack).to(dt)
            self._rblob_key = key
        return self._rblob

    def __getstate__(self):
        d = self.__dict__.copy()
        for k in ("_rblob", "_rblob_key", "_rbblob", "_rbblob_key"):
            d.pop(k, None)
        return d

    def reconstruct_hot(self, feat_b, feat_f, frame, out, scratch=None, stages=RECON_ALL):
        """sr_c64_recon_fwd on one frame of every clip: feat_b / feat_f (b, h, w, cw) NHWC state handles of the two trunks (hot dtype),
        frame (b, 3, h, w) fp32, out (b, 3, 4h, 4w) fp32 with a dense (3, 4h, 4w) block (a slice of the result).  scratch: the four
        images (fused, up1, up2, hr) to reuse; returns them."""
        dt = self.backward_trunk.hot_dtype
        b, h, w, cw = feat_b.shape
        dev = feat_b.device
        if feat_f.shape != feat_b.shape or feat_b.dtype != dt or feat_f.dtype != dt or cw not in (24, 64) or \
                not (feat_b.is_contiguous() and feat_f.is_contiguous()):
            raise ValueError("reconstruct_hot: the two state handles of propagate(handles=True)")
        if out.shape != (b, 3, 4 * h, 4 * w) or out.dtype != torch.float32 or out.stride()[1:] != (16 * h * w, 4 * w, 1):
            raise ValueError("reconstruct_hot: out must be (b, 3, 4h, 4w) fp32 with a dense (3, 4h, 4w) block")
        frame = _inner_contiguous(frame.detach().float())
        if scratch is None:
            scratch = (torch.empty((b, h, w, 64), dtype=dt, device=dev), torch.empty((b, 2 * h, 2 * w, 64), dtype=dt, device=dev),
                       torch.empty((b, 4 * h, 4 * w, 64), dtype=dt, device=dev), torch.empty((b, 4 * h, 4 * w, 64), dtype=dt, device=dev))
        with torch.cuda.device(dev):
            blob = self._recon_blob(dt)
            _, boff = _recon_tables(self.num_feat, dev.index if dev.index is not None else torch.cuda.current_device())
            L.launch("sr_c64_recon_fwd", L.lib().sr_c64_recon_fwd, feat_b.data_ptr(), feat_f.data_ptr(), cw, frame.data_ptr(),
                     frame.stride(0), blob.data_ptr(), boff, scratch[0].data_ptr(), scratch[1].data_ptr(), scratch[2].data_ptr(),
                     scratch[3].data_ptr(), out.data_ptr(), out.stride(0), b, h, w, L.DTYPE_CODE[dt], stages, L.stream_ptr(dev))
        return scratch

    def _forward_hot(self, x, flows_forward, flows_backward, height, weight):
        """the no-graph route: propagation -> NHWC state handles -> csrc/vsr_recon.h, frame by frame into the preallocated result"""
        b, n, _, h, w = x.size()
        with torch.no_grad():
            hb, hf = propagate(x, flows_forward, flows_backward, self.backward_trunk, self.forward_trunk, flow_warp,
                               num_feat=self.num_feat, handles=True)
            out = torch.empty((b, n, 3, 4 * h, 4 * w), dtype=torch.float32, device=x.device)
            scratch = None
            for i in range(n):
                scratch = self.reconstruct_hot(hb[i], hf[i], x[:, i], out[:, i], scratch)
                hb[i] = hf[i] = None                 # the handles die as the loop passes them
            if (height, weight) != (4 * h, 4 * w):
                out = F.interpolate(out.view(b * n, 3, 4 * h, 4 * w), size=(height, weight), mode='bilinear').view(b, n, 3, height, weight)
        return out
