"""The per-frame video network of the reference's video scripts (`--model_type single`; reference: models/single_image_model.py,
`Result_Model(scale, channel=32, blocks=8, kernel=3)` at train_video_superresolution.py:245) for the MI355X.

Same constructor, module tree, construction order, state_dict keys and shapes as the reference, so a seeded build draws the same
numbers and its checkpoints load with strict=True:

    encoder.{bias,weight_g,weight_v}        weight-normed 3x3 conv, 3 -> C (no mean subtraction)
    body.{i}.body.0.body.{0,2}.*            Block i: y = conv2(ReLU(conv1(x))) + x, both weight-normed k x k, C -> C
    body.{blocks}.*                         weight-normed 3x3 conv, C -> C
    skip.*, img_upsample                    constructed and never called, as in the reference
    shuf.0.{weight,bias}                    ConvTranspose2d(C, 3, 5, stride=scale)

forward(x, height, weight), per frame of a (B, N, 3, H, W) clip: e = encoder(x); f = body(e) + e; D = shuf(f) ((4H + 1) x (4W + 1) at
scale 4); out = F.interpolate(D, (height, weight), 'bilinear').

Three routes, chosen per call by `hot_route_reason(x, height, weight)` (None: the HIP inference route runs; else why not) and, for the
calls it turns away, `train_route_reason(x, height, weight)` (None: the HIP training route runs); `last_route` records "hip",
"hip_train" or "aten" ("hip_train_step" after `train_step`, the whole step as one C call: DESIGN.md section 19).
  * ATen: the reference's forward, every layer its own module call (torch._weight_norm + F.conv2d / F.conv_transpose2d /
    F.interpolate).  It serves every call that records an autograd graph unless `hot_training` is set -- DDP wraps the model as it
    is -- and CPU tensors, scale != 4, channel > 32, kernel != 3, a forward (pre-)hook on any submodule, `aten_forward = True`, and,
    with `hot_resize`, an output size other than (4H, 4W) beyond packing.FN_MAX_OUT (32768) a side.
  * HIP training (`hot_training = True`, default False; csrc/frame_net.h, csrc/frame_net_bwd.h, csrc/result_block.h through
    sr_fn_net_train_fwd / sr_fn_net_bwd): a graph-recording call on device tensors with (height, weight) = (4H, 4W) -- with
    `hot_resize = True` (default False) any (height, weight) >= (1, 1), through sr_fn_net_train_fwd_sized / sr_fn_net_bwd_sized --, an input that
    does not require grad and every parameter of encoder, body and shuf requiring grad.  One autograd.Function spans the clip; it
    takes the effective tensors (weight() and bias per conv, shuf.0's) and returns their gradients, so the weight-norm backward,
    the optimisers, the losses and DDP are torch's as before.  Forward value bit-identical to the HIP inference route.  Anything
    the rule excludes keeps the ATen route silently.  The criteria of mobilesuperresolution_amd.training fold into the backward at
    (4H, 4W), and `train_step` runs there; with `hot_resize_fold = True` (default False, acts only together with `hot_resize`) both
    do so at any size the sized kernels take (sr_fn_net_bwd_loss_sized, sr_fn_net_train_step_sized).
  * HIP (csrc/frame_net.h, sr_fn_net_fwd): no graph recorded, device tensors, scale 4, 1 <= channel <= 32, kernel 3.  All B N frames go
    through each layer as one batch and the result lands in the (B, N, 3, height, weight) fp32 output; (height, weight) = (4H, 4W)
    fuses the resize, any other size has the kernel write D and one F.interpolate finish (the reference resizes D, not a x4 image)
    or, with `hot_resize`, is resized inside the upsampler kernel from packing.resize_axis' tables (sr_fn_net_fwd_sized; DESIGN.md
    section 26), bit-identical to the training route's forward.  The weight norm of the parameters stays an ATen op in front.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib as L
from .. import hotpath as HP
from .. import packing as P
from . import clip_train as CT

__all__ = ["Result_Model", "Block", "Conv_sep"]


class _WNConv2d(nn.Module):
    """torch.nn.utils.weight_norm(nn.Conv2d(cin, cout, k, padding=k // 2, groups=groups)): the conv's own init, then bias, weight_g,
    weight_v registered in that order"""

    def __init__(self, cin, cout, k, groups=1):
        super().__init__()
        conv = nn.Conv2d(cin, cout, k, padding=k // 2, groups=groups)
        v = conv.weight.detach().clone()
        self.bias = nn.Parameter(conv.bias.detach().clone())
        self.weight_g = nn.Parameter(torch.norm_except_dim(v, 2, 0).detach())
        self.weight_v = nn.Parameter(v)
        self.kernel_size, self.groups = k, groups

    def weight(self):
        return torch._weight_norm(self.weight_v, self.weight_g, 0)

    def forward(self, x):
        return F.conv2d(x, self.weight(), self.bias, padding=self.kernel_size // 2, groups=self.groups)


class Conv_sep(nn.Module):
    """conv k x k -> ReLU -> conv k x k (keys body.0, body.2); seperate=True builds the reference's depthwise / pointwise chain, whose
    last pointwise conv the reference constructs and leaves out of `body`"""

    def __init__(self, input_dim, output_dim, kernal_size, weight_norm=None, seperate=False):
        super().__init__()
        self.seperate, self.kernel_size = seperate, kernal_size
        if seperate:
            body = [_WNConv2d(input_dim, input_dim, kernal_size, groups=input_dim), nn.ReLU(inplace=True),
                    _WNConv2d(input_dim, output_dim, 1),
                    _WNConv2d(input_dim, input_dim, kernal_size, groups=input_dim), nn.ReLU(inplace=True)]
            _WNConv2d(input_dim, output_dim, 1)                # drawn, never used
        else:
            body = [_WNConv2d(input_dim, output_dim, kernal_size), nn.ReLU(inplace=True),
                    _WNConv2d(input_dim, output_dim, kernal_size)]
        self.body = nn.Sequential(*body)

    def forward(self, x):
        return self.body(x)


class Block(nn.Module):
    def __init__(self, IN, split, kernel_size, weight_norm=None):
        super().__init__()
        self.split, self.IN, self.conv_channel = IN - split, IN, split
        self.body = nn.Sequential(Conv_sep(split, split, kernel_size))

    def forward(self, x):
        return self.body(x) + x


class _FrameNetTrain(CT.ClipTrain):
    """The whole clip through sr_fn_net_train_fwd / sr_fn_net_bwd (the node protocol: clip_train.ClipTrain).  Inputs: the model (for its
    blob cache and geometry), the frames, the output size (height, weight), then the EFFECTIVE tensors: encoder (weight, bias), the
    2 blocks + 1 convs' (weight, bias) in forward order, shuf.0 (weight, bias).  The folded backward is sr_fn_net_bwd_loss: the output
    gradient is formed inside the upsampler's backward, no d(loss)/d(sr) tensor.  An output size other than (4H, 4W) (`hot_resize`)
    goes through the sized entry points with the model's cached axis tables (`ctx.resize`); it is foldable only when the model's
    `hot_resize_fold` is set, then through sr_fn_net_bwd_loss_sized."""
    LEAD = 3
    _grad_sizes = staticmethod(P.fn_grad_sizes)

    @staticmethod
    def _run_backward(ctx, g, hr=None, kind=0, gscale=0.0):
        frames, bwd, acts, ts, masks = ctx.saved
        channel, nb, wgs = ctx.geom
        n, _, h, w = frames.shape
        dev = frames.device
        wgs = wgs or HP.fn_bwd_wgs(n, h, w)
        gs = torch.empty((4, n, h, w, P.FN_C), dtype=bwd.dtype, device=dev)
        parts = torch.empty(P.fn_bwd_parts(nb, wgs), dtype=torch.float32, device=dev)
        grads = torch.empty(sum(P.fn_grad_sizes(channel, nb)), dtype=torch.float32, device=dev)
        if ctx.resize is not None:
            g_is = 3 * ctx.out_size[0] * ctx.out_size[1]
            if hr is not None:
                return grads, HP.fn_net_bwd_loss_sized(frames, g, hr, kind, gscale, g_is, ctx.resize, bwd, acts, ts, masks, gs, parts, wgs,
                                                       grads, channel, nb)
            HP.fn_net_bwd_sized(frames, g, g_is, ctx.resize, bwd, acts, ts, masks, gs, parts, wgs, grads, channel, nb)
            return grads, None
        if hr is None:
            HP.fn_net_bwd(frames, g, 48 * h * w, bwd, acts, ts, masks, gs, parts, wgs, grads, channel, nb)
            return grads, None
        return grads, HP.fn_net_bwd_loss(frames, g, hr, kind, gscale, 48 * h * w, bwd, acts, ts, masks, gs, parts, wgs, grads, channel, nb)

    @staticmethod
    def forward(ctx, model, x, size, *eff):
        b, n, _, h, w = x.shape
        oh, ow = size
        dev, dt, nb = x.device, model.hot_dtype, model.blocks
        with torch.cuda.device(dev):
            blob, offs, head, bwd = model._blobs(eff)
            frames = CT.frames_of(x)
            acts = torch.empty((nb + 2, b * n, h, w, P.FN_C), dtype=dt, device=dev)
            ts = torch.empty((nb, b * n, h, w, P.FN_C), dtype=dt, device=dev)
            masks = torch.empty((nb, b * n, h, w), dtype=torch.int32, device=dev)
            out = torch.empty((b, n, 3, oh, ow), dtype=torch.float32, device=dev)
            ctx.resize = None if (oh, ow) == (4 * h, 4 * w) else model._resize(dev, h, w, oh, ow)
            if ctx.resize is None:
                HP.fn_net_train_fwd(frames, blob, offs, head, acts, ts, masks, out, 48 * h * w, nb)
            else:
                HP.fn_net_train_fwd_sized(frames, blob, offs, head, acts, ts, masks, out, 3 * oh * ow, ctx.resize, nb)
        ctx.saved = (frames, bwd, acts, ts, masks)
        ctx.geom = (model.IN, nb, model.train_wgs)
        ctx.out_size = (oh, ow)
        _FrameNetTrain._record(ctx, out, eff)
        ctx.foldable = ctx.resize is None or bool(model.hot_resize_fold)
        return out


class Result_Model(nn.Module):
    # True (class or instance): the ATen route for every call
    aten_forward = False
    # True (class or instance): graph-recording calls that train_route_reason() admits run the HIP training route
    hot_training = False
    # True (class or instance): an output size other than (4H, 4W) is resized inside the upsampler kernels, forward and backward
    # (sr_fn_net_*_sized); with hot_training, train_route_reason() then admits any (height, weight) up to packing.FN_MAX_OUT a side
    hot_resize = False
    # True (class or instance), acts only together with hot_resize: at another size than (4H, 4W) the criteria of training fold into the
    # sized backward (sr_fn_net_bwd_loss_sized) and train_step runs (sr_fn_net_train_step_sized); False: both stay at (4H, 4W)
    hot_resize_fold = False
    # workgroups of the training route's weight-gradient launches; 0: hotpath.fn_bwd_wgs
    train_wgs = 0

    def __init__(self, scale, channel=48, blocks=7, kernel=3, hot_dtype=None):
        super().__init__()
        self.image_mean = 0.5
        self.scale, self.IN, self.blocks, self.kernel = scale, channel, blocks, kernel
        self.hot_dtype = L.hot_dtype(hot_dtype)
        self.last_route = None
        self.encoder = _WNConv2d(3, channel, 3)
        body = [Block(channel, channel, kernel) for _ in range(blocks)]
        body.append(_WNConv2d(channel, channel, 3))
        self.body = nn.Sequential(*body)
        self.skip = _WNConv2d(3, scale * scale * 3, 5)
        self.shuf = nn.Sequential(nn.ConvTranspose2d(channel, 3, 5, stride=scale))
        self.img_upsample = nn.Upsample(scale_factor=4, mode='bilinear', align_corners=False)

    # ---- the route rule ----
    def _convs(self):
        """the 2 blocks + 1 C -> C convs in forward order"""
        out = []
        for i in range(self.blocks):
            cs = self.body[i].body[0].body
            out += [cs[0], cs[2]]
        return out + [self.body[self.blocks]]

    def _effective(self):
        """the effective tensors: encoder, convs, upsampler, (weight, bias) each"""
        up = self.shuf[0]
        eff = [self.encoder.weight(), self.encoder.bias] + [t for c in self._convs() for t in (c.weight(), c.bias)]
        return eff + [up.weight, up.bias]

    def _route_reason(self, x, train, **kw):
        return CT.route_reason(self, x, "Result_Model", train=train, modules=self.modules(), params=self.parameters(),
                               kernel_reason=f"kernel {self.kernel} (the kernels are 3x3)" if self.kernel != 3 else None, **kw)

    def hot_route_reason(self, x, height=1080, weight=1920):
        """None when this call runs on the HIP route, else a short reason why it keeps the ATen route"""
        return self._route_reason(x, False, out_size=(height, weight),
                                  empty="empty input or output" if x.numel() == 0 or height < 1 or weight < 1 else None)

    def train_route_reason(self, x, height=1080, weight=1920):
        """None when this graph-recording call runs on the HIP training route, else a short reason why it keeps the ATen route"""
        trained = [p for m in (self.encoder, self.body, self.shuf) for p in m.parameters()]
        return self._route_reason(x, True, trained=trained, out_size=(height, weight),
                                  empty="empty input or output" if x.numel() == 0 or height < 1 or weight < 1 else None)

    def forward(self, x, height=1080, weight=1920):
        if self.hot_route_reason(x, height, weight) is None:
            self.last_route = "hip"
            return self._forward_hip(x, height, weight)
        if self.hot_training and self.train_route_reason(x, height, weight) is None:
            self.last_route = "hip_train"
            return _FrameNetTrain.apply(self, x, (height, weight), *self._effective())
        self.last_route = "aten"
        outs = []
        for i in range(x.shape[1]):
            e = self.encoder(x[:, i])
            f = self.body(e) + e
            outs.append(F.interpolate(self.shuf(f), size=(height, weight), mode='bilinear'))
        return torch.stack(outs, dim=1)

    # ---- the one-call training step ----
    def _step_geom(self):
        return "fn", self.IN, self.blocks

    def _step_entries(self):
        """the trained tensors in the order of the flat gradient vector (packing.fn_grad_sizes): (weight_g, weight_v) then bias per conv,
        the upsampler's weight and bias, the encoder's"""
        up = self.shuf[0]
        out = [t for c in self._convs() for t in ((c.weight_g, c.weight_v), c.bias)]
        return out + [up.weight, up.bias, (self.encoder.weight_g, self.encoder.weight_v), self.encoder.bias]

    def train_step_reason(self, lr, hr, optimizer):
        """None when train_step(lr, hr, optimizer) runs, else a short reason why it raises: train_route_reason's rule with the output size
        read off hr (`hot_training` need not be set), an optimizer that is a training.Adam over exactly the trained parameters, hr fp32
        (B, N, 3, 4H, 4W) on the device -- with `hot_resize` and `hot_resize_fold` both set (B, N, 3, OH, OW), 1 <= OH, OW <=
        packing.FN_MAX_OUT --, one step count for all parameters"""
        trained = [p for m in (self.encoder, self.body, self.shuf) for p in m.parameters()]
        size = tuple(hr.shape[3:5]) if torch.is_tensor(hr) and hr.dim() == 5 else (-1, -1)
        reason = self._route_reason(lr, True, trained=trained, out_size=size, opt_in=True,
                                    empty="empty input or output" if lr.numel() == 0 else None)
        return CT.train_step_reason(self, lr, hr, optimizer, reason)

    def train_step(self, lr, hr, optimizer, criterion="charbonnier", loss_weight=1.0, sr_out=None):
        """One training step as ONE C call (sr_fn_net_train_step): weight norm, packing, the HIP training forward, the loss folded into the
        backward, the weight-norm backward and Adam on every trained tensor.  lr (B, N, 3, H, W), hr fp32 (B, N, 3, 4H, 4W), optimizer a
        training.Adam over the trained parameters; criterion "charbonnier" or "l1".  sr_out: None, or a contiguous fp32 device tensor of hr's
        shape that receives the network's output.  With `hot_resize` and `hot_resize_fold` both set, hr may be (B, N, 3, OH, OW) of any other
        size: the same call through sr_fn_net_train_step_sized, the resize inside the upsampler kernels.  Returns loss_weight x the mean loss, a 0-dim fp32 device tensor; no host sync, no autograd graph,
        no `.grad`.  Raises HotpathError with train_step_reason's text when that is not
        None: the caller asked for this route by name."""
        def launch(step, st, kind):
            b, n, _, h, w = lr.shape
            dev, dt, nb, bn = lr.device, self.hot_dtype, self.blocks, b * n
            frames = CT.frames_of(lr)
            wgs = self.train_wgs or HP.fn_bwd_wgs(bn, h, w)
            acts = torch.empty((nb + 2, bn, h, w, P.FN_C), dtype=dt, device=dev)
            ts = torch.empty((nb, bn, h, w, P.FN_C), dtype=dt, device=dev)
            masks = torch.empty((nb, bn, h, w), dtype=torch.int32, device=dev)
            oh, ow = hr.shape[3:]
            out = CT.step_output(sr_out, lr, (oh, ow))
            gs = torch.empty((4, bn, h, w, P.FN_C), dtype=dt, device=dev)
            parts = torch.empty(P.fn_bwd_parts(nb, wgs), dtype=torch.float32, device=dev)
            grads = torch.empty(sum(P.fn_grad_sizes(self.IN, nb)), dtype=torch.float32, device=dev)
            loss_part = torch.empty(wgs, dtype=torch.float32, device=dev)
            if (oh, ow) == (4 * h, 4 * w):
                HP.fn_net_train_step(step, frames, hr.contiguous(), kind, st["offs"], acts, ts, masks, out, gs, parts, wgs, grads,
                                     loss_part, self.IN, nb, dt)
            else:
                HP.fn_net_train_step_sized(step, frames, hr.contiguous(), kind, st["offs"], acts, ts, masks, out,
                                           self._resize(dev, h, w, oh, ow), gs, parts, wgs, grads, loss_part, self.IN, nb, dt)
            self.last_route = "hip_train_step"
        return CT.train_step(self, "_fn", lr, hr, optimizer, criterion, loss_weight, self.train_step_reason(lr, hr, optimizer), launch)

    # ---- the HIP route ----
    def _blobs(self, eff=None):
        """(packed convs + upsampler, host offsets, encoder head blob) in the hot dtype; re-packed only when a parameter changed.
        eff: the training route's effective tensors (encoder, convs, upsampler: weight, bias each), already computed for this call;
        then a fourth entry, the backward blob of transposed, flipped weights, is packed from the same source vector."""
        backward = eff is not None

        def pack():
            e = eff if backward else self._effective()
            packed = HP.fn_pack(list(zip(e[2:-2:2], e[3:-2:2])), e[-2], e[-1], self.hot_dtype, backward=backward)
            return (packed[0], packed[1], HP.fn_pack_encoder(e[0], e[1], self.hot_dtype)) + tuple(packed[2:])
        return CT.cached_blobs(self, "_fn", self.parameters(), backward, pack)

    def _resize(self, dev, h, w, oh, ow):
        """the sized kernels' resize argument (hotpath.fn_resize) for H x W frames -> (oh, ow), uploaded once per (device, size) and kept
        on the model next to the blobs (the last 8 sizes; not pickled)"""
        cache = self.__dict__.setdefault("_fn_resize", {})
        key = (dev, h, w, oh, ow)
        if key not in cache:
            while len(cache) >= 8:
                cache.pop(next(iter(cache)))
            cache[key] = HP.fn_resize(h, w, oh, ow, dev)
        return cache[key]

    def __getstate__(self):
        return CT.state_without_blobs(self, "_fn")

    def _forward_hip(self, x, height, weight):
        b, n, _, h, w = x.shape
        with torch.no_grad(), torch.cuda.device(x.device):
            blob, offs, head = self._blobs()
            frames = CT.frames_of(x)
            scratch = torch.empty((3, b * n, h, w, P.FN_C), dtype=self.hot_dtype, device=x.device)
            if (height, weight) == (4 * h, 4 * w):
                out = torch.empty((b, n, 3, height, weight), dtype=torch.float32, device=x.device)
                HP.fn_net_fwd(frames, blob, offs, head, scratch, out, 3 * height * weight, self.blocks)
                return out
            if self.hot_resize:
                out = torch.empty((b, n, 3, height, weight), dtype=torch.float32, device=x.device)
                HP.fn_net_fwd_sized(frames, blob, offs, head, scratch, out, 3 * height * weight, self._resize(x.device, h, w, height, weight),
                                    self.blocks)
                return out
            d = torch.empty((b * n, 3, 4 * h + 1, 4 * w + 1), dtype=torch.float32, device=x.device)
            HP.fn_net_fwd(frames, blob, offs, head, scratch, d, d.stride(0), self.blocks, P.FN_ALL | P.FN_WRITE_D)
            return F.interpolate(d, size=(height, weight), mode='bilinear').view(b, n, 3, height, weight)
