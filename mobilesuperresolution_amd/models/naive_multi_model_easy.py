"""The multi-frame video network of the reference's video scripts (`--model_type multi`; reference:
models/naive_multi_model_easy.py, `Naive_model(scale, filename, spynet_pretrained)`) for the MI355X.

Same module tree, registration order, construction (draw) order, state_dict keys and shapes as the reference, so a seeded build draws
the same numbers and its checkpoints load with strict=True.  `status` is the `[IN, split, kernel]` list per block of the last line of
`filename` (result_model.parse_status), C = status[0][0]:

    flownet.*                               this package's SpyNet (key naming of the vendored SPyNet, as BasicVSR documents), frozen
    body.{i}.skip.{weight,bias}             Conv2d(2 IN, IN, 1): constructed, never called (drawn AFTER the block's body convs)
    body.{i}.body.{0,2}.{weight,bias}       plain k x k convs IN -> C -> C; block 0 has IN = 2 C + 2, the others IN = C
    encode.{bias,weight_g,weight_v}         weight-normed 3x3, 3 -> C (drawn BEFORE the blocks, registered after them)
    decode.*                                weight-normed k x k, C -> 3 scale^2, k = the LAST block's kernel
    skip.*                                  weight-normed 5x5, 3 -> 3 scale^2: constructed, never called
    shuf                                    PixelShuffle(scale)

forward(x, height=None, weight=None), x (B, N, 3, H, W): flows = get_flow(x) (B, N - 1, 2, H, W); per frame i: e_i = encode(x_i);
y = body0(cat(flow, warp, e_i)) + e_i with (flow, warp) = (0, e_0) for i = 0 and (flows[:, i - 1], flow_warp(e_{i-1}, flow)) after;
y = body_j(y) + y; out_i = shuf(decode(y)) + interpolate(x_i, scale_factor=4, bilinear).  The x4 of the base is hard-coded in the
reference, so the network runs at scale 4 only; the trainer's `model(lr, h, w)` extras must equal (4H, 4W).

Three routes, chosen per call by `hot_route_reason(x)` (None: the HIP inference route runs; else why not) and, for the calls it turns
away, `train_route_reason(x)` (None: the HIP training route runs); `last_route` records "hip", "hip_train" or "aten"
("hip_train_step" after `train_step`, the whole step as one C call: DESIGN.md section 19).
  * ATen: the reference's forward, layer by layer (without its .to('cuda')).  It serves every call that records an autograd graph
    unless `hot_training` is set -- DDP wraps the model as it is -- and CPU tensors, scale != 4, C > 32, any block kernel != 3, blocks
    whose IN differ, a forward (pre-)hook on any submodule other than the flownet's, oversized grids, and `aten_forward = True`.
  * HIP training (`hot_training = True`, default False; csrc/multi_frame.h, csrc/multi_frame_bwd.h, csrc/result_block.h through
    sr_mf_net_train_fwd / sr_mf_net_bwd): a graph-recording call on device tensors, an input that does not require grad, and every
    parameter of encode, body.*.body.{0,2} and decode requiring grad (the never-called skip convs and the frozen flownet are not
    consulted and get no gradient).  One autograd.Function spans the clip batch; it takes the frames, the flows (no gradient) and the
    effective tensors (encode.weight() and bias, each block's two plain convs, decode.weight() and bias) and returns their
    gradients as views of one flat fp32 vector, so the weight-norm backward, the optimisers, the losses and DDP are torch's as
    before.  Forward value bit-identical to the HIP inference route.  Anything the rule excludes keeps the ATen route silently.
  * HIP (csrc/multi_frame.h, sr_mf_net_fwd): the network has no recurrence (frame i uses the ENCODER output of frame i - 1), so given
    the flows all B N frames go through each layer as one batch: one C call per clip batch, no ATen convolution, warp, concat or
    interpolate.  The weight norm of encode / decode stays an ATen op in front of the packing, once per parameter version.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib as L
from .. import hotpath as HP
from .. import packing as P
from . import clip_train as CT
from .result_model import parse_status
from .single_image_model import _WNConv2d
from .spynet_arch import SpyNet

__all__ = ["Naive_model", "Block", "aten_flow_warp"]

def aten_flow_warp(x, flow):
    """the vendored flow_warp (bilinear, zeros padding, align_corners=True) as ATen ops, for the route that records a graph or runs on
    the CPU.  x (n, c, h, w); flow (n, h, w, 2), [..., 0] = dx"""
    n, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(0, h, device=x.device, dtype=x.dtype), torch.arange(0, w, device=x.device, dtype=x.dtype),
                            indexing="ij")
    vx = 2.0 * (gx + flow[..., 0]) / max(w - 1, 1) - 1.0
    vy = 2.0 * (gy + flow[..., 1]) / max(h - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((vx, vy), dim=3), mode="bilinear", padding_mode="zeros", align_corners=True)


class Block(nn.Module):
    """conv k x k IN -> OUT, ReLU, conv k x k OUT -> OUT (keys body.0, body.2); `skip` is drawn after them, registered before them and
    never called, as in the reference"""

    def __init__(self, IN, OUT, split, kernel_size, weight_norm=None):
        super().__init__()
        self.split, self.IN, self.OUT, self.conv_channel = IN - split, IN, OUT, split
        body = [nn.Conv2d(IN, OUT, kernel_size, padding=kernel_size // 2), nn.ReLU(inplace=True),
                nn.Conv2d(OUT, OUT, kernel_size, padding=kernel_size // 2)]
        self.skip = nn.Conv2d(2 * IN, IN, 1, padding=0)
        self.body = nn.Sequential(*body)

    def forward(self, x):
        return self.body(x)


class _MultiFrameTrain(CT.ClipTrain):
    """The whole clip batch through sr_mf_net_train_fwd / sr_mf_net_bwd (the node protocol: clip_train.ClipTrain).  Inputs: the model (for
    its blob cache and geometry), the frames (B, N, 3, H, W), the flows (B, N - 1, 2, H, W), then the EFFECTIVE tensors: encode (weight,
    bias), per block (w1, b1, w2, b2), decode (weight, bias).  The folded backward is sr_mf_net_bwd_loss: the un-shuffled output gradient
    is formed from sr and hr, no d(loss)/d(sr) tensor."""
    LEAD = 3
    _grad_sizes = staticmethod(P.mf_grad_sizes)

    @staticmethod
    def _run_backward(ctx, g, hr=None, kind=0, gscale=0.0):
        frames, flows, bound, bwd, acts, ts, masks, wf = ctx.saved
        channel, nb, b, n, wgs = ctx.geom
        bn, _, h, w = frames.shape
        dev = frames.device
        wgs = wgs or HP.fn_bwd_wgs(bn, h, w)
        gs = torch.empty((6, bn, h, w, P.FN_C), dtype=bwd.dtype, device=dev)
        parts = torch.empty(P.mf_bwd_parts(nb, wgs), dtype=torch.float32, device=dev)
        grads = torch.empty(sum(P.mf_grad_sizes(channel, nb)), dtype=torch.float32, device=dev)
        if hr is None:
            HP.mf_net_bwd(frames, flows, bound, g, bwd, acts, ts, masks, wf, gs, parts, wgs, grads, channel, nb, b, n)
            return grads, None
        return grads, HP.mf_net_bwd_loss(frames, flows, bound, g, hr, kind, gscale, bwd, acts, ts, masks, wf, gs, parts, wgs, grads,
                                         channel, nb, b, n)

    @staticmethod
    def forward(ctx, model, x, flows, *eff):
        b, n, _, h, w = x.shape
        dev, dt, nb = x.device, model.hot_dtype, len(model.idx)
        with torch.cuda.device(dev):
            blob, head, bwd = model._blobs(eff)
            frames = CT.frames_of(x)
            flows = CT.flows_of(flows, b, n, h, w)
            bound = flows.abs().amax().reshape(1) if n > 1 else None      # the warp backward's window, left on the device
            acts = torch.empty((nb + 1, b * n, h, w, P.FN_C), dtype=dt, device=dev)
            ts = torch.empty((nb, b * n, h, w, P.FN_C), dtype=dt, device=dev)
            masks = torch.empty((nb, b * n, h, w), dtype=torch.int32, device=dev)
            wf = torch.empty((2, b * n, h, w, P.FN_C), dtype=dt, device=dev)
            out = torch.empty((b, n, 3, 4 * h, 4 * w), dtype=torch.float32, device=dev)
            HP.mf_net_train_fwd(frames, flows, blob, head, acts, ts, masks, wf, out, nb, b, n)
        ctx.saved = (frames, flows, bound, bwd, acts, ts, masks, wf)
        ctx.geom = (model.IN, nb, b, n, model.train_wgs)
        return _MultiFrameTrain._record(ctx, out, eff)


class Naive_model(nn.Module):
    # True (class or instance): the ATen route for every call
    aten_forward = False
    # True (class or instance): graph-recording calls that train_route_reason() admits run the HIP training route
    hot_training = False
    # workgroups of the training route's weight-gradient launches; 0: hotpath.fn_bwd_wgs
    train_wgs = 0

    def __init__(self, scale, filename=None, spynet_pretrained=None, hot_dtype=None, status=None):
        super().__init__()
        if (status is None) == (filename is None):
            raise ValueError("Naive_model: give either filename or status")
        self.image_mean = 0.5
        self.scale = scale
        self.idx = [list(b) for b in (status if status is not None else parse_status(filename))]
        if not self.idx:
            raise ValueError("Naive_model: status without blocks")
        self.IN = self.idx[0][0]
        self.hot_dtype = L.hot_dtype(hot_dtype)
        self.last_route = None
        self.flownet = SpyNet(spynet_pretrained)
        self.flownet.requires_grad_(False)
        num_outputs = scale * scale * 3
        self.body = nn.ModuleDict()
        encode = _WNConv2d(3, self.IN, 3)
        kernel_size = 3
        for i, (cin, split, kernel_size) in enumerate(self.idx):
            self.body[str(i)] = Block(2 * cin + 2 if i == 0 else cin, cin, split, kernel_size)
        self.encode = encode
        self.decode = _WNConv2d(self.IN, num_outputs, kernel_size)       # the last block's kernel, as the reference's loop leaves it
        self.skip = _WNConv2d(3, num_outputs, 5)
        self.shuf = nn.Sequential(*([nn.PixelShuffle(scale)] if scale > 1 else []))

    # ---- flows ----
    def get_flow(self, x):
        """(B, N - 1, 2, H, W): the flow that warps frame i - 1's features onto frame i at index i - 1; empty for N = 1 (SPyNet is not
        called then)"""
        b, n, c, h, w = x.shape
        with torch.no_grad():
            if n < 2:
                return x.new_zeros((b, 0, 2, h, w), dtype=torch.float32)
            x_1 = x[:, :-1].reshape(-1, c, h, w)
            x_2 = x[:, 1:].reshape(-1, c, h, w)
            return self.flownet(x_2, x_1).view(b, n - 1, 2, h, w)

    # ---- the route rule ----
    def _route_reason(self, x, train, **kw):
        kernel_reason = None
        if any(b[2] != 3 for b in self.idx):
            kernel_reason = "a block kernel other than 3 (the kernels are 3x3)"
        elif any(b[0] != self.IN for b in self.idx):
            kernel_reason = "blocks of different widths"
        # the flownet runs in front of every route: its hooks are not consulted
        modules = [m for name, m in self.named_modules() if not name.startswith("flownet")]
        return CT.route_reason(self, x, "Naive_model", train=train, kernel_reason=kernel_reason, modules=modules,
                               empty="empty input" if x.numel() == 0 else None, **kw)

    def hot_route_reason(self, x):
        """None when this call runs on the HIP route, else a short reason why it keeps the ATen route"""
        return self._route_reason(x, False, params=self.parameters())

    def _trained(self):
        """the modules whose parameters the training route reads and gives gradients to"""
        mods = [self.encode]
        for i in range(len(self.idx)):
            mods += [self.body[str(i)].body[0], self.body[str(i)].body[2]]
        return mods + [self.decode]

    def train_route_reason(self, x):
        """None when this graph-recording call runs on the HIP training route, else a short reason why it keeps the ATen route"""
        trained = [p for m in self._trained() for p in m.parameters()]
        return self._route_reason(x, True, params=trained, trained=trained)

    def _effective(self):
        eff = [self.encode.weight(), self.encode.bias]
        for i in range(len(self.idx)):
            c1, c2 = self.body[str(i)].body[0], self.body[str(i)].body[2]
            eff += [c1.weight, c1.bias, c2.weight, c2.bias]
        return eff + [self.decode.weight(), self.decode.bias]

    def forward(self, x, height=None, weight=None):
        if x.dim() != 5 or x.shape[2] != 3:
            raise ValueError(f"Naive_model: input (B, N, 3, H, W), got {tuple(x.shape)}")
        b, n, _, h, w = x.shape
        if (height is not None and height != 4 * h) or (weight is not None and weight != 4 * w):
            raise ValueError(f"Naive_model: output size ({height}, {weight}) for a {h} x {w} clip; the network has no resize and gives "
                             f"({4 * h}, {4 * w})")
        flows = self.get_flow(x)
        if self.hot_route_reason(x) is None:
            self.last_route = "hip"
            return self._forward_hip(x, flows)
        if self.hot_training and self.train_route_reason(x) is None:
            self.last_route = "hip_train"
            return _MultiFrameTrain.apply(self, x, flows, *self._effective())
        self.last_route = "aten"
        outs, prev = [], None
        for i in range(n):
            xi = x[:, i]
            e = self.encode(xi)
            if i == 0:
                flow, warp = torch.zeros((b, 2, h, w), dtype=e.dtype, device=e.device), e
            else:
                flow = flows[:, i - 1].to(e.dtype)
                warp = aten_flow_warp(prev, flow.permute(0, 2, 3, 1))
            prev = e
            y = self.body["0"](torch.cat((flow, warp, e), dim=1)) + e
            for j in range(1, len(self.idx)):
                y = self.body[str(j)](y) + y
            base = F.interpolate(xi, scale_factor=4, mode='bilinear', align_corners=False)
            outs.append(self.shuf(self.decode(y)) + base)
        return torch.stack(outs, dim=1)

    # ---- the one-call training step ----
    def _step_geom(self):
        return "mf", self.IN, len(self.idx)

    def _step_entries(self):
        """the trained tensors in the order of the flat gradient vector (packing.mf_grad_sizes): per block w1, b1, w2, b2, then decode's
        (weight_g, weight_v) and bias, then encode's"""
        out = []
        for i in range(len(self.idx)):
            c1, c2 = self.body[str(i)].body[0], self.body[str(i)].body[2]
            out += [c1.weight, c1.bias, c2.weight, c2.bias]
        return out + [(self.decode.weight_g, self.decode.weight_v), self.decode.bias, (self.encode.weight_g, self.encode.weight_v),
                      self.encode.bias]

    def train_step_reason(self, lr, hr, optimizer):
        """None when train_step(lr, hr, optimizer) runs, else a short reason why it raises: train_route_reason's rule (`hot_training` need
        not be set), an optimizer that is a training.Adam over exactly the trained parameters, hr fp32 (B, N, 3, 4H, 4W) on the device, one
        step count for all parameters"""
        trained = [p for m in self._trained() for p in m.parameters()]
        return CT.train_step_reason(self, lr, hr, optimizer, self._route_reason(lr, True, params=trained, trained=trained, opt_in=True))

    def train_step(self, lr, hr, optimizer, criterion="charbonnier", loss_weight=1.0, flows=None, sr_out=None):
        """One training step as ONE C call (sr_mf_net_train_step) behind the flows: weight norm of encode / decode, packing, the HIP training
        forward, the loss folded into the backward, the weight-norm backward and Adam on every trained tensor.  lr (B, N, 3, H, W), hr fp32
        (B, N, 3, 4H, 4W), optimizer a training.Adam over the trained parameters; criterion "charbonnier" or "l1"; flows None: get_flow(lr)
        as in forward, else (B, N - 1, 2, H, W).  sr_out: None, or a contiguous fp32 (B, N, 3, 4H, 4W) device tensor that
        receives the network's output.  Returns loss_weight x the mean loss, a 0-dim fp32 device tensor; no host sync, no autograd graph,
        no `.grad`.  Raises HotpathError with train_step_reason's text when that is not None."""
        def launch(step, st, kind):
            b, n, _, h, w = lr.shape
            dev, dt, nb, bn = lr.device, self.hot_dtype, len(self.idx), b * n
            frames = CT.frames_of(lr)
            fl = CT.flows_of(self.get_flow(lr) if flows is None else flows, b, n, h, w)
            bound = fl.abs().amax().reshape(1) if n > 1 else None
            wgs = self.train_wgs or HP.fn_bwd_wgs(bn, h, w)
            acts = torch.empty((nb + 1, bn, h, w, P.FN_C), dtype=dt, device=dev)
            ts = torch.empty((nb, bn, h, w, P.FN_C), dtype=dt, device=dev)
            masks = torch.empty((nb, bn, h, w), dtype=torch.int32, device=dev)
            wf = torch.empty((2, bn, h, w, P.FN_C), dtype=dt, device=dev)
            out = CT.step_output(sr_out, lr)
            gs = torch.empty((6, bn, h, w, P.FN_C), dtype=dt, device=dev)
            parts = torch.empty(P.mf_bwd_parts(nb, wgs), dtype=torch.float32, device=dev)
            grads = torch.empty(sum(P.mf_grad_sizes(self.IN, nb)), dtype=torch.float32, device=dev)
            loss_part = torch.empty(wgs, dtype=torch.float32, device=dev)
            HP.mf_net_train_step(step, frames, fl, bound, hr.contiguous(), kind, acts, ts, masks, wf, out, gs, parts, wgs, grads, loss_part,
                                 self.IN, nb, b, n, dt)
            self.last_route = "hip_train_step"
        return CT.train_step(self, "_mf", lr, hr, optimizer, criterion, loss_weight, self.train_step_reason(lr, hr, optimizer), launch)

    # ---- the HIP route ----
    def _blobs(self, eff=None):
        """(packed blocks + decode, encoder head blob) in the hot dtype; re-packed only when a parameter changed.  eff: the training
        route's effective tensors (encode, blocks, decode), already computed for this call; then a third entry, the backward blob of
        transposed, tap-flipped operands (packing.mf_bwd_tables), is packed from the same source vector."""
        backward = eff is not None

        def pack():
            e = eff if backward else self._effective()
            blocks = [tuple(e[2 + 4 * i:6 + 4 * i]) for i in range(len(self.idx))]
            if backward:
                packed = HP.mf_pack_train(blocks, e[-2], e[-1], self.hot_dtype)
            else:
                packed = (HP.mf_pack(blocks, e[-2], e[-1], self.hot_dtype),)
            return (packed[0], HP.fn_pack_encoder(e[0], e[1], self.hot_dtype)) + tuple(packed[1:])
        ps = [p for name, p in self.named_parameters() if not name.startswith("flownet")]
        return CT.cached_blobs(self, "_mf", ps, backward, pack)

    def __getstate__(self):
        return CT.state_without_blobs(self, "_mf")

    def _forward_hip(self, x, flows):
        b, n, _, h, w = x.shape
        with torch.no_grad(), torch.cuda.device(x.device):
            blob, head = self._blobs()[:2]
            frames = CT.frames_of(x)
            flows = CT.flows_of(flows, b, n, h, w)
            scratch = torch.empty((3, b * n, h, w, P.FN_C), dtype=self.hot_dtype, device=x.device)
            out = torch.empty((b, n, 3, 4 * h, 4 * w), dtype=torch.float32, device=x.device)
            HP.mf_net_fwd(frames, flows, blob, head, scratch, out, len(self.idx), b, n)
            return out
