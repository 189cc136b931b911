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

Two routes, chosen per call by `hot_route_reason(x)` (None: the HIP route runs; else why not); `last_route` records "hip" or "aten".
  * ATen: the reference's forward, layer by layer (without its .to('cuda')).  It serves every call that records an autograd graph --
    training stays here, DDP wraps the model as it is -- and CPU tensors, scale != 4, C > 32, any block kernel != 3, blocks whose IN
    differ, a forward (pre-)hook on any submodule other than the flownet's, oversized grids, and `aten_forward = True`.
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
from .result_model import parse_status
from .single_image_model import _WNConv2d
from .spynet_arch import SpyNet

__all__ = ["Naive_model", "Block", "aten_flow_warp"]

_HOOKS = ("_forward_hooks", "_forward_pre_hooks")


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


class Naive_model(nn.Module):
    # True (class or instance): the ATen route for every call
    aten_forward = False

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
    def hot_route_reason(self, x):
        """None when this call runs on the HIP route, else a short reason why it keeps the ATen route"""
        if x.dim() != 5 or x.shape[2] != 3:
            raise ValueError(f"Naive_model: input (B, N, 3, H, W), got {tuple(x.shape)}")
        if self.aten_forward:
            return "aten_forward is set"
        if self.scale != 4:
            return f"scale {self.scale} (the kernels upsample x4)"
        if not 1 <= self.IN <= P.FN_C:
            return f"{self.IN} channels (the kernels are 32 wide)"
        if any(b[2] != 3 for b in self.idx):
            return "a block kernel other than 3 (the kernels are 3x3)"
        if any(b[0] != self.IN for b in self.idx):
            return "blocks of different widths"
        if any(getattr(m, a, None) for name, m in self.named_modules() if not name.startswith("flownet") for a in _HOOKS):
            return "a forward hook on a module"
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return "the call records an autograd graph"
        if not x.is_cuda:
            return "CPU input"
        if any(p.device != x.device for p in self.parameters()):
            return "parameters on another device"
        if x.numel() == 0:
            return "empty input"
        if x.shape[0] * x.shape[1] > 65535 or x.shape[3] > 8192 or x.shape[4] > 8192:
            return "frame count or frame size beyond the kernels' grid"
        return None

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

    # ---- the HIP route ----
    def _blobs(self):
        """(packed blocks + decode, encoder head blob) in the hot dtype; re-packed only when a parameter changed"""
        ps = [p for name, p in self.named_parameters() if not name.startswith("flownet")]
        key = (self.hot_dtype,) + tuple((p.data_ptr(), p._version) for p in ps)
        if getattr(self, "_mf_key", None) != key:
            blocks = []
            for i in range(len(self.idx)):
                c1, c2 = self.body[str(i)].body[0], self.body[str(i)].body[2]
                blocks.append((c1.weight, c1.bias, c2.weight, c2.bias))
            blob = HP.mf_pack(blocks, self.decode.weight(), self.decode.bias, self.hot_dtype)
            self._mf_blobs = (blob, HP.fn_pack_encoder(self.encode.weight(), self.encode.bias, self.hot_dtype))
            self._mf_key = key
        return self._mf_blobs

    def __getstate__(self):
        d = self.__dict__.copy()
        d.pop("_mf_blobs", None)
        d.pop("_mf_key", None)
        return d

    def _forward_hip(self, x, flows):
        b, n, _, h, w = x.shape
        with torch.no_grad(), torch.cuda.device(x.device):
            blob, head = self._blobs()
            frames = x.detach().reshape(b * n, 3, h, w)
            if frames.dtype != torch.float32 or not frames.is_contiguous():
                frames = frames.float().contiguous()
            if n > 1:
                flows = flows.detach()
                if tuple(flows.shape) != (b, n - 1, 2, h, w):
                    raise ValueError(f"Naive_model: flows {tuple(flows.shape)} for a clip {tuple(x.shape)}")
                if flows.dtype != torch.float32 or not flows.is_contiguous():
                    flows = flows.float().contiguous()
            scratch = torch.empty((3, b * n, h, w, P.FN_C), dtype=self.hot_dtype, device=x.device)
            out = torch.empty((b, n, 3, 4 * h, 4 * w), dtype=torch.float32, device=x.device)
            HP.mf_net_fwd(frames, flows if n > 1 else None, blob, head, scratch, out, len(self.idx), b, n)
            return out
