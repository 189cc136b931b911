"""BasicVSR propagation trunk on the MI355X hot path.

`ConvResidualBlocks(num_in_ch, num_out_ch, num_block)` mirrors the reference class of the same name
(models/basicvsr_arch.py:108-124 with ResidualBlockNoBN :126-147; identical copies in
basicvsr_arch_origin.py and mvvsr_arch.py): conv3x3(num_in_ch -> F) + LeakyReLU(0.1), then
num_block x [x + conv2(relu(conv1(x)))]; plain convs with bias, PyTorch-default init; state_dict keys
`main.0.{weight,bias}`, `main.2.{i}.conv{1,2}.{weight,bias}`.  Input/output are NCHW fp32 like the
reference's (it is called on `torch.cat([x_i, feat_prop], 1)` inside the propagation loops,
basicvsr_arch.py:67-88); every convolution, activation, residual add and their backward run in
csrc/conv3x3.h.  The kernels are 24 features wide; a narrower trunk (the trainer's MotionVectorVSR uses
num_feat = 20, train_video_superresolution.py:251) is embedded exactly: its parameters keep the reference shapes and
are scattered into the 24-wide layout with zero rows / columns, whose channels stay exactly zero through every
LeakyReLU / ReLU / residual add.  24 < num_out_ch <= 64 (the reference's default num_feat = 64) runs on the 64-wide
kernels of csrc/conv64.h, embedded the same way (packing.c64_tables).  Their default route is inference: nothing is saved, and a
call that would record an autograd graph raises.  Training is opt-in per trunk (`hot_training = True`, or `set_wide_training(model)`):
a graph-recording call then runs the two-launch forward that keeps a_i and t_i, and the HIP backward of csrc/conv64_bwd.h.
Supported: num_out_ch <= 64, num_in_ch in {num_out_ch, num_out_ch + 3}.
No CPU / ATen fallback.

`propagate(...)` restates the two recurrent loops of MotionVectorVSR.forward (mvvsr_arch.py:72-93) around
the trunk; flow_warp itself is the next row of SURVEY 8(f) and is taken as a callable.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from functools import lru_cache

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib as L
from .. import packing as P

__all__ = ["BasicVSR", "ConvResidualBlocks", "ResidualBlockNoBN", "paired", "propagate", "set_wide_training"]

@lru_cache(maxsize=None)
def _tables(ci_real: int, device_index: int):
    t = P.c3_tables(ci_real)
    dev = torch.device("cuda", device_index)
    return (torch.from_numpy(t["w"]).to(dev), torch.from_numpy(t["grad"]).to(dev), t["off"]["size"])


def _pack(conv: nn.Conv2d, dtype):
    """one conv's packed weights (per-op entry points / tests)"""
    w = conv.weight
    idx, _, size = _tables(w.shape[1], w.device.index if w.device.index is not None else torch.cuda.current_device())
    src = torch.cat([w.detach().reshape(-1).float(), conv.bias.detach().float(), torch.tensor([0.0, 1.0], device=w.device)])
    assert src.numel() == size
    return src.index_select(0, idx).to(dtype).contiguous()


@lru_cache(maxsize=None)
def _trunk_tables(cin: int, nb: int, device_index: int):
    """Combined tables of a whole trunk over the flat parameter (conv k = weight | bias, contiguous, in state_dict
    order): `blob = cat(flat, [0, 1])[pack_idx]` packs every conv at once (conv k starts at element blob_off[k]);
    `gflat = slabs.flatten()[grad_idx]` gathers the gradient of the flat parameter."""
    import ctypes
    dev = torch.device("cuda", device_index)
    first, rest = P.c3_tables(cin), P.c3_tables(24)
    total = (24 * cin * 9 + 24) + 2 * nb * (24 * 24 * 9 + 24)
    pack, grad, boff, foff, npk = [], [], [], 0, 0
    for k in range(1 + 2 * nb):
        t = first if k == 0 else rest
        nreal = t["off"]["zero"]                               # weight | bias elements of this conv
        idx = t["w"].astype(np.int64)
        idx = np.where(idx < nreal, idx + foff, total + (idx - nreal))      # zero / one -> the two appended constants
        boff.append(npk)
        npk += len(idx)
        pack.append(idx)
        grad.append(t["grad"].astype(np.int64) + k * 9 * 1024)
        foff += nreal
    assert foff == total
    return (torch.from_numpy(np.concatenate(pack)).to(dev), torch.from_numpy(np.concatenate(grad)).to(dev),
            (ctypes.c_long * len(boff))(*boff), torch.tensor([0.0, 1.0], device=dev))


@lru_cache(maxsize=None)
def _unpack_tables(cin: int, device_index: int):
    """int32 tables for the slab -> flat-gradient reduction inside sr_c3_trunk_bwd: (sidx0, dst0, sidx1, dst1)"""
    dev = torch.device("cuda", device_index)

    def mk(t):                                       # in slab order: coalesced reads of the 64 partial slabs, scattered result
        g = t["grad"].astype(np.int64)
        o = np.argsort(g, kind="stable")
        return torch.from_numpy(g[o].astype(np.int32)).to(dev), torch.from_numpy(o.astype(np.int32)).to(dev)
    return mk(P.c3_tables(cin)) + mk(P.c3_tables(24))


@lru_cache(maxsize=None)
def _trunk64_tables(cin: int, f: int, nb: int, device_index: int):
    """packing.c64_trunk_tables on the device: (pack index, blob offsets as a C long array, first conv's kernel input width)"""
    import ctypes
    pack, boff, ci_k = P.c64_trunk_tables(cin, f, nb)
    return torch.from_numpy(pack).to(torch.device("cuda", device_index)), (ctypes.c_long * len(boff))(*boff), ci_k


@lru_cache(maxsize=None)
def _trunk64_bwd_tables(cin: int, f: int, nb: int, device_index: int):
    """packing.c64_trunk_bwd_tables on the device: (pack index, the table dict, the four unpack tables)"""
    t = P.c64_trunk_bwd_tables(cin, f, nb)
    dev = torch.device("cuda", device_index)
    return torch.from_numpy(t["pack"]).to(dev), t, tuple(torch.from_numpy(u).to(dev) for u in t["unpack"])


_NO_GRAPH_MSG = ("ConvResidualBlocks with more than 24 features runs by default on inference-only kernels (nothing is saved for a "
                 "backward at F > 24): call it under torch.no_grad(), or take the trunk's parameters out of autograd with "
                 "requires_grad_(False) and pass inputs that do not require grad; to TRAIN it, opt in with `trunk.hot_training = True` "
                 "(models.set_wide_training(model) sets it on every wide trunk; a paired call needs it on both trunks)")
_NO_FLOW_GRAD_MSG = ("the 64-wide training route has no gradient to the flow by default: detach the flow, or opt in with "
                     "`trunk.flow_training = True` (models.set_flow_training(model) sets it on every wide trunk; a paired call needs it "
                     "on both trunks)")


def _wide_route(mods, features, *inputs):
    """24 < F <= 64: does this call take the training route?  No graph would be recorded: False (the inference kernels).  A graph
    would be recorded: True when every trunk has opted in (`hot_training`), else refuse at once, rather than return a result whose
    gradient is wrong."""
    if not (torch.is_grad_enabled() and (any(m.flat.requires_grad for m in mods) or
                                         any(t is not None and t.requires_grad for t in inputs))):
        return False
    if not all(m.hot_training for m in mods):
        raise NotImplementedError(_NO_GRAPH_MSG)
    if features is False:
        raise NotImplementedError("features=False is an inference route: call it under torch.no_grad()")
    return True


def set_wide_training(module, on=True):
    """opt every wide (24 < F <= 64) ConvResidualBlocks below `module` in to (or out of) the HIP training route; returns the trunks"""
    found = [m for m in module.modules() if isinstance(m, ConvResidualBlocks) and m.wide]
    for m in found:
        m.hot_training = bool(on)
    return found


def set_flow_training(module, on=True):
    """opt every wide (24 < F <= 64) ConvResidualBlocks below `module` in to (or out of) the flow gradient of the HIP training route
    (`flow_training`; it matters only where `hot_training` is set as well); returns the trunks"""
    found = [m for m in module.modules() if isinstance(m, ConvResidualBlocks) and m.wide]
    for m in found:
        m.flow_training = bool(on)
    return found


def _flow_route(mods, flow):
    """a flow that requires grad on the wide training route: every trunk of the call must have opted in with `flow_training`"""
    if flow is not None and flow.requires_grad and not all(m.flow_training for m in mods):
        raise NotImplementedError(_NO_FLOW_GRAD_MSG)


class ResidualBlockNoBN(nn.Module):
    """parameter holder: conv1, conv2 (reference models/basicvsr_arch.py:126-147)"""

    def __init__(self, num_feat=64, res_scale=1, pytorch_init=False):
        super().__init__()
        if res_scale != 1:
            raise NotImplementedError("res_scale != 1 is not on the hot path (the reference always uses 1)")
        self.res_scale = res_scale
        self.conv1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1, bias=True)
        self.conv2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1, bias=True)


class ConvResidualBlocks(nn.Module):
    """One flat fp32 nn.Parameter (`flat`) holds every conv in the reference's state_dict order; `state_dict()` /
    `load_state_dict()` expose / accept the reference keys (`main.0.weight`, `main.2.{i}.conv1.bias`, ...) as views.
    The recurrent loops call the trunk once per frame and direction: with per-tensor parameters every call
    would cost 2 x (1 + 2 n) gradient accumulations in autograd, with the flat buffer it costs one.
    `hot_training` (wide trunks only; the convention of the two video networks): False = a graph-recording call raises, True = it
    runs the HIP training route.
    `flow_training` (wide trunks only, a second opt-in on top of `hot_training`): False = a flow that requires grad is refused on the
    training route, True = forward_warped / forward_warped_pair return its gradient (csrc/conv64_bwd.h, c64_warp_dflow_kernel)."""

    hot_training = False
    flow_training = False

    def __init__(self, num_in_ch=3, num_out_ch=64, num_block=15, hot_dtype=None):
        super().__init__()
        if not (1 <= num_out_ch <= 64) or num_in_ch not in (num_out_ch, num_out_ch + 3):
            raise NotImplementedError("MI355X hot path supports ConvResidualBlocks(F or F + 3, F, n) with F <= 24 (training and "
                                      f"inference) or 24 < F <= 64 (inference; training with hot_training) (got {num_in_ch}, {num_out_ch}); there is no generic fallback")
        self.num_in_ch, self.num_feat, self.num_block = num_in_ch, num_out_ch, num_block
        self.wide = num_out_ch > 24                                 # the 64-wide kernels (csrc/conv64.h, conv64_bwd.h)
        if self.wide:
            self.cin_k = P.c64_ci_kernel(num_in_ch, num_out_ch)     # 80 (state | frame | 0) or 64
        else:
            self.cin_k = 27 if num_in_ch == num_out_ch + 3 else 24  # input width of the first conv as the kernels see it
        self.hot_dtype = L.hot_dtype(hot_dtype)
        # same constructor calls, in the same order, as the reference (same RNG draws); then flattened
        main = nn.Sequential(nn.Conv2d(num_in_ch, num_out_ch, 3, 1, 1, bias=True), nn.Identity(),
                             nn.Sequential(*[ResidualBlockNoBN(num_feat=num_out_ch) for _ in range(num_block)]))
        self.entries, off, vals = OrderedDict(), 0, []
        for key, t in main.state_dict(prefix="main.").items():
            self.entries[key] = (off, tuple(t.shape))
            vals.append(t.detach().reshape(-1))
            off += t.numel()
        self.flat = nn.Parameter(torch.cat(vals).float())
        self._pad = None
        if num_out_ch < 24:                                  # scatter / gather tables between the real and the 24-wide layout
            f, cin, ck = num_out_ch, num_in_ch, self.cin_k
            real = torch.arange(self.flat.numel(), dtype=torch.int64)
            zero = self.flat.numel()                          # index of the appended 0
            pads, off = [], 0
            for k in range(1 + 2 * num_block):
                ci_r, ci_p = (cin, ck) if k == 0 else (f, 24)
                wp = torch.full((24, ci_p, 3, 3), zero, dtype=torch.int64)
                wp[:f, :ci_r] = real[off:off + f * ci_r * 9].view(f, ci_r, 3, 3)
                off += f * ci_r * 9
                bp = torch.full((24,), zero, dtype=torch.int64)
                bp[:f] = real[off:off + f]
                off += f
                pads += [wp.reshape(-1), bp]
            pad_idx = torch.cat(pads)
            inv = torch.empty(self.flat.numel(), dtype=torch.int64)
            pos = torch.nonzero(pad_idx != zero).squeeze(1)
            inv[pad_idx[pos]] = pos
            self.register_buffer("_pad_idx", pad_idx, persistent=False)
            self.register_buffer("_unpad_idx", inv, persistent=False)
            self._pad = True

    def __getstate__(self):
        d = self.__dict__.copy()
        for k in ("_blob", "_blob_key", "_bwd_blob", "_bwd_blob_key", "_pair_blob_t", "_pair_key", "_pair_bwd_t", "_pair_bwd_key"):
            d.pop(k, None)
        return d

    # ---- reference-compatible checkpoints ----
    def named_tensors(self, source=None):
        """(reference key, view) over the flat parameter (or any tensor laid out like it, e.g. its gradient)"""
        base = self.flat.detach() if source is None else source
        for name, (off, shape) in self.entries.items():
            yield name, base[off:off + int(np.prod(shape))].view(shape)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        if destination is None:
            destination = OrderedDict()
        for name, view in self.named_tensors():
            destination[prefix + name] = view
        return destination

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        with torch.no_grad():
            for name, view in self.named_tensors():
                key = prefix + name
                if key not in state_dict:
                    missing_keys.append(key)
                    continue
                src = state_dict[key]
                if tuple(src.shape) != tuple(view.shape):
                    error_msgs.append(f"size mismatch for {key}: checkpoint {tuple(src.shape)} vs model {tuple(view.shape)}")
                    continue
                view.copy_(src)
        for key in state_dict:
            if key.startswith(prefix) and key[len(prefix):] not in self.entries and key != prefix + "flat":
                unexpected_keys.append(key)

    def _packed(self, flat):
        """every conv's MFMA-fragment weights in one buffer; re-packed (3 launches) only when the parameter changed —
        the recurrent loops call the trunk once per frame and direction with the same weights"""
        key = (self.hot_dtype, flat.data_ptr(), flat._version)
        if getattr(self, "_blob_key", None) != key and self.wide:
            dev = flat.device
            pack, _, _ = _trunk64_tables(self.num_in_ch, self.num_feat, self.num_block,
                                         dev.index if dev.index is not None else torch.cuda.current_device())
            fl = flat.detach()
            self._blob = torch.cat([fl, fl.new_zeros(1)]).index_select(0, pack).to(self.hot_dtype)
            self._blob_key = key
        elif getattr(self, "_blob_key", None) != key:
            dev = flat.device
            tabs = _trunk_tables(self.cin_k, self.num_block,
                                 dev.index if dev.index is not None else torch.cuda.current_device())
            fl = flat.detach()
            if self._pad:
                fl = torch.cat([fl, fl.new_zeros(1)]).index_select(0, self._pad_idx)
            self._blob = torch.cat([fl, tabs[3]]).index_select(0, tabs[0]).to(self.hot_dtype)
            self._blob_key = key
        return self._blob

    def _packed_bwd(self, flat):
        """the wide training route's backward blob (packing.c64_trunk_bwd_tables), cached like `_packed`"""
        key = (self.hot_dtype, flat.data_ptr(), flat._version)
        if getattr(self, "_bwd_blob_key", None) != key:
            dev = flat.device
            pack, _, _ = _trunk64_bwd_tables(self.num_in_ch, self.num_feat, self.num_block,
                                             dev.index if dev.index is not None else torch.cuda.current_device())
            fl = flat.detach()
            self._bwd_blob = torch.cat([fl, fl.new_zeros(1)]).index_select(0, pack).to(self.hot_dtype)
            self._bwd_blob_key = key
        return self._bwd_blob

    def forward(self, fea: torch.Tensor, state=None, flow=None, flow_bound=None, warped: bool = False, features: bool = True):
        if warped:                                   # (frame, state, flow) -> (features, state): see forward_warped
            return self._forward_warped(fea, state, flow, flow_bound, features)
        if not fea.is_cuda:
            raise L.HotpathError("ConvResidualBlocks (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
        if fea.dim() != 4 or fea.shape[1] != self.num_in_ch:
            raise ValueError(f"expected N x {self.num_in_ch} x H x W input, got {tuple(fea.shape)}")
        if fea.device != self.flat.device:
            raise L.HotpathError(f"input on {fea.device}, parameters on {self.flat.device}")
        if self.wide:
            with torch.cuda.device(fea.device):
                if _wide_route((self,), True, fea):
                    return _Trunk64TrainFunction.apply(fea, None, None, None, self, self.flat, None, None, True, True)
                return _trunk64_plain(self, fea)
        with torch.cuda.device(fea.device):          # kernels go to THIS device's current stream
            return _TrunkFunction.apply(fea, self, self.flat)

    def forward_warped(self, frame, state=None, flow=None, flow_bound=None, features=True):
        """through __call__, so that module hooks see the fused step too (their output is the (features, state) pair).
        features=False (no graph may be recorded): the NCHW fp32 feature copy is skipped and the features are None."""
        return self(frame, state, flow, flow_bound, warped=True, features=features)

    def _forward_warped(self, frame, state=None, flow=None, flow_bound=None, features=True):
        """The recurrent step of the reference's propagation loops in one call (models/basicvsr_arch.py:74-76,85-87):
            feat = flow_warp(feat, flow.permute(0, 2, 3, 1)); feat = trunk(torch.cat([frame, feat], dim=1))
        with the warp and the concat gathered straight into the first conv's LDS tile (csrc/conv3x3.h, c3_stage_x_warp).
        frame (N,3,H,W) fp32; state = the handle the previous call returned (None: zero state, the first frame of a
        direction); flow (N,2,H,W) fp32 pixel displacements (None: no warp); flow_bound: 0-dim device tensor >= max|flow|
        (computed here when omitted).  Returns (features (N,F,H,W) fp32 like the reference's, state handle)."""
        if self.num_in_ch != self.num_feat + 3:
            raise NotImplementedError("forward_warped needs a trunk built as ConvResidualBlocks(F + 3, F, n)")
        if not frame.is_cuda:
            raise L.HotpathError("ConvResidualBlocks (MI355X hot path) needs CUDA/HIP tensors; there is no CPU fallback")
        if frame.dim() != 4 or frame.shape[1] != 3:
            raise ValueError(f"expected N x 3 x H x W frames, got {tuple(frame.shape)}")
        if flow is not None and state is None:
            raise ValueError("a flow without a state to warp")
        for name, t in (("frame", frame), ("state", state), ("flow", flow)):
            if t is not None and t.device != self.flat.device:
                raise L.HotpathError(f"{name} on {t.device}, parameters on {self.flat.device}")
        if self.wide:
            if _wide_route((self,), features, frame, state, flow):
                _flow_route((self,), flow)
                if flow is not None and flow_bound is None:
                    flow_bound = flow.detach().abs().amax()
                return _Trunk64TrainFunction.apply(frame, state, flow, flow_bound, self, self.flat, None, None, features, False)
            return _trunk64_warped(frame, state, flow, self, features=features)
        if not features and _records_graph((self,), frame, state, flow):
            raise NotImplementedError("forward_warped(features=False) is an inference route: call it under torch.no_grad()")
        if flow is not None and flow_bound is None:
            flow_bound = flow.detach().abs().amax()
        return _TrunkWarpFunction.apply(frame, state, flow, flow_bound, self, self.flat, None, None, features)


def forward_warped_pair(trunk_a, trunk_b, frames, state=None, flow=None, flow_bound=None, features=True):
    """ONE recurrent step of BOTH propagation directions (reference: the two loops of basicvsr_arch.py:67-88, which are
    independent of each other): frames (2N, 3, H, W) = [the backward-time loop's frame | the forward-time loop's frame], state / flow
    likewise (2N, ...); the first half runs through `trunk_a`, the second through `trunk_b`, in the same launches -- twice the
    workgroups per launch and half the dependent launches of two forward_warped calls.  Returns (trunk_a's features (N, F, H, W),
    trunk_b's features (N, F, H, W), state (2N, ...)).  features=False (a consumer that reads the NHWC state itself, as the
    reconstruction of BasicVSR_origin does): the NCHW fp32 feature copies are skipped and the two features are None.
    features=None (24-wide trunks): the same, but the autograd node is kept, so the state can be differentiated through."""
    if trunk_a.wide or trunk_b.wide:
        if _wide_route((trunk_a, trunk_b), features, frames, state, flow):
            _flow_route((trunk_a, trunk_b), flow)
            if flow is not None and flow_bound is None:
                flow_bound = flow.detach().abs().amax()
            feat_a, feat_b, new_state = _Trunk64TrainFunction.apply(frames, state, flow, flow_bound, trunk_a, trunk_a.flat, trunk_b,
                                                                    trunk_b.flat, features, False)
        else:
            feat_a, feat_b, new_state = _trunk64_warped(frames, state, flow, trunk_a, trunk_b, features=features)
    else:
        if flow is not None and flow_bound is None:
            flow_bound = flow.detach().abs().amax()
        feat_a, feat_b, new_state = _TrunkWarpFunction.apply(frames, state, flow, flow_bound, trunk_a, trunk_a.flat, trunk_b,
                                                             trunk_b.flat, features)
    half = frames.shape[0] // 2
    for tr, sl, ft in ((trunk_a, slice(0, half), feat_a), (trunk_b, slice(half, None), feat_b)):
        for hook in tr._forward_hooks.values():       # forward hooks of the two modules see their half of the step, as with forward_warped
            hook(tr, (frames[sl], None if state is None else state[sl], None if flow is None else flow[sl], flow_bound),
                 (ft, new_state[sl]))
    return feat_a, feat_b, new_state


_TILE = 16                                             # csrc/conv3x3.h C3Cfg::TH = TW


def _wgrad_wgs(n, h, w, cap=None):
    """workgroups per conv for the weight-gradient launches: every workgroup walks the same number of 16x16 tiles (256 tiles
    at C4 with both directions in one launch -> 64 workgroups x 4 tiles; 128 and 256 workgroups measured slower: more slabs to reduce)"""
    cap = int(os.environ.get("SR_C3_WGRAD_WGS", 64)) if cap is None else cap
    total = n * ((h + _TILE - 1) // _TILE) * ((w + _TILE - 1) // _TILE)
    per = -(-total // cap)
    return -(-total // per)


def _launch(name, *args):
    L.launch(name, getattr(L.lib(), name), *args, L.stream_ptr())


class _TrunkFunction(torch.autograd.Function):
    """whole trunk forward / backward as one C call each (csrc/conv3x3.h via sr_c3_trunk_fwd / _bwd)"""

    @staticmethod
    def forward(ctx, fea, mod, flat):
        dt, nb, cin = mod.hot_dtype, mod.num_block, mod.num_in_ch
        n, _, h, w = fea.shape
        dev = fea.device
        ci0 = 32 if mod.cin_k == 27 else 24
        if ci0 != cin:
            x0 = torch.zeros((n, h, w, ci0), dtype=dt, device=dev)
            x0[..., :cin] = fea.detach().permute(0, 2, 3, 1)
        else:
            x0 = fea.detach().permute(0, 2, 3, 1).to(dt).contiguous()
        blob = mod._packed(flat)
        tabs = _trunk_tables(mod.cin_k, nb, dev.index if dev.index is not None else torch.cuda.current_device())
        acts = torch.empty((nb + 1, n, h, w, 24), dtype=dt, device=dev)              # a_0 .. a_nb
        mids = torch.empty((max(nb, 1), n, h, w, 24), dtype=dt, device=dev)          # t_i = relu(conv1(a_i))
        _launch("sr_c3_trunk_fwd", x0.data_ptr(), None, acts.data_ptr(), mids.data_ptr(), blob.data_ptr(), tabs[2], nb, n, h, w,
                ci0, L.DTYPE_CODE[dt], 0, 0)
        ctx.mod, ctx.x0, ctx.acts, ctx.mids, ctx.blob = mod, x0, acts, mids, blob
        ctx.need_dx = fea.requires_grad
        out = torch.empty((n, mod.num_feat, h, w), dtype=torch.float32, device=dev)
        out.copy_(acts[nb][..., :mod.num_feat].permute(0, 3, 1, 2))      # NHWC hot dtype -> NCHW fp32 in one kernel
        return out

    @staticmethod
    def backward(ctx, dy):
        with torch.cuda.device(ctx.x0.device):
            return _TrunkFunction._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        mod, x0, acts, mids, blob = ctx.mod, ctx.x0, ctx.acts, ctx.mids, ctx.blob
        dt, nb, cin = mod.hot_dtype, mod.num_block, mod.num_in_ch
        n, h, w, ci0 = x0.shape
        dev = x0.device
        wgs = _wgrad_wgs(n, h, w)
        _, grad_idx, boff, _ = _trunk_tables(mod.cin_k, nb, dev.index if dev.index is not None else torch.cuda.current_device())
        ga = torch.empty_like(acts)                                                  # gradient at a_0 .. a_nb
        gt = torch.empty_like(mids)
        if mod.num_feat < 24:
            ga[nb].zero_()
            ga[nb][..., :mod.num_feat] = dy.permute(0, 2, 3, 1)
        else:
            ga[nb] = dy.permute(0, 2, 3, 1)
        import ctypes
        parts = torch.empty((1 + 2 * nb, wgs, 9 * 1024), dtype=torch.float32, device=dev)
        dx0 = torch.empty_like(x0) if ctx.need_dx else None
        s0, d0, s1, d1 = _unpack_tables(mod.cin_k, dev.index if dev.index is not None else torch.cuda.current_device())
        gflat = torch.empty(s0.numel() + 2 * nb * s1.numel(), dtype=torch.float32, device=dev)      # dW | db of every conv, flat order
        unpack = L.C3Unpack(s0.data_ptr(), d0.data_ptr(), s0.numel(), s1.data_ptr(), d1.data_ptr(), s1.numel(), gflat.data_ptr())
        _launch("sr_c3_trunk_bwd", x0.data_ptr(), None, acts.data_ptr(), mids.data_ptr(), ga.data_ptr(), gt.data_ptr(),
                blob.data_ptr(), boff, parts.data_ptr(), dx0.data_ptr() if dx0 is not None else None, ctypes.byref(unpack), nb, wgs,
                n, h, w, ci0, L.DTYPE_CODE[dt], 0, 0)
        dfea = None
        if dx0 is not None:
            dfea = torch.empty((n, cin, h, w), dtype=torch.float32, device=dev)
            dfea.copy_(dx0[..., :cin].permute(0, 3, 1, 2))
        if mod._pad:
            gflat = gflat.index_select(0, mod._unpad_idx)
        return dfea, None, gflat


def _inner_contiguous(t):
    """(N, C, H, W) view whose (C, H, W) block is dense: the kernels take the batch stride as an argument"""
    _, c, h, w = t.shape
    return t if t.stride()[1:] == (h * w, w, 1) else t.contiguous()


def _pair_blob(mod, flat, mod2, flat2):
    """the two trunks' packed weights one behind the other (cached until either parameter changes)"""
    b1, b2 = mod._packed(flat), mod2._packed(flat2)
    key = (b1.data_ptr(), mod._blob_key, b2.data_ptr(), mod2._blob_key)
    if getattr(mod, "_pair_key", None) != key:
        mod._pair_blob_t = torch.cat([b1, b2])
        mod._pair_key = key
    return mod._pair_blob_t, b1.numel()


class _TrunkWarpFunction(torch.autograd.Function):
    """flow_warp -> concat -> whole trunk, forward / backward as one C call each (sr_c3_trunk_fwd / _bwd with a
    sr_c3_warp_t): outputs (features NCHW fp32, the same features NHWC in the hot dtype = the next call's state).
    With `mod2` / `flat2`: TWO trunks in the same launches -- the first half of the batch through `mod`, the second half through
    `mod2` (the two time directions of a frame step of the propagation loops, which are independent)."""

    @staticmethod
    def forward(ctx, frame, state, flow, bound, mod, flat, mod2=None, flat2=None, features=True):
        import ctypes
        dt, nb = mod.hot_dtype, mod.num_block
        n, _, h, w = frame.shape
        dev = frame.device
        frame_ = _inner_contiguous(frame.detach().float())
        flow_ = _inner_contiguous(flow.detach().float()) if flow is not None else None
        state_ = state.detach() if state is not None else None
        if state_ is not None and (state_.shape != (n, h, w, 24) or state_.dtype != dt or not state_.is_contiguous()):
            raise ValueError("state must be the handle returned by the previous forward_warped call of this clip")
        if flow_ is not None and flow_.shape != (n, 2, h, w):
            raise ValueError(f"expected N x 2 x H x W flow, got {tuple(flow_.shape)}")
        bound_ = bound.detach().float().reshape(()) if bound is not None else None
        with torch.cuda.device(dev):
            if mod2 is None:
                blob, n_dir, bstride = mod._packed(flat), 0, 0
            else:
                if n % 2 or (mod2.num_block, mod2.hot_dtype, mod2.num_feat, mod2.cin_k) != (nb, dt, mod.num_feat, mod.cin_k):
                    raise ValueError("two trunks in one call: an even batch (one half per trunk) and trunks of the same geometry")
                blob, bstride = _pair_blob(mod, flat, mod2, flat2)
                n_dir = n // 2
            tabs = _trunk_tables(27, nb, dev.index)
            acts = torch.empty((nb + 1, n, h, w, 24), dtype=dt, device=dev)
            mids = torch.empty((max(nb, 1), n, h, w, 24), dtype=dt, device=dev)
            # the gathered input is kept (2 MB at C4) when a backward will want the first conv's weight gradient
            x0 = torch.empty((n, h, w, 32), dtype=dt, device=dev) if (ctx.needs_input_grad[5] or (mod2 is not None and ctx.needs_input_grad[7])) else None
            warp = L.C3Warp(frame_.data_ptr(), frame_.stride(0), state_.data_ptr() if state_ is not None else None,
                            flow_.data_ptr() if flow_ is not None else None, flow_.stride(0) if flow_ is not None else 0,
                            None, None, None, 0, x0.data_ptr() if x0 is not None else None)
            _launch("sr_c3_trunk_fwd", None, ctypes.byref(warp), acts.data_ptr(), mids.data_ptr(), blob.data_ptr(), tabs[2], nb,
                    n, h, w, 32, L.DTYPE_CODE[dt], n_dir, bstride)
            if features:
                out = torch.empty((n, mod.num_feat, h, w), dtype=torch.float32, device=dev)
                out.copy_(acts[nb][..., :mod.num_feat].permute(0, 3, 1, 2))
        if features is False:                        # no graph is being recorded (propagate checks): nothing to save
            # the handle OWNS its storage: a view of `acts` would keep all nb + 1 activation images of this step alive for as long
            # as the caller holds the handle (a whole clip, in BasicVSR_origin's reconstruction)
            last = acts[nb].clone()
            return (None, None, last) if mod2 is not None else (None, last)
        ctx.mod, ctx.acts, ctx.mids, ctx.blob, ctx.x0 = mod, acts, mids, blob, x0
        ctx.mod2, ctx.n_dir, ctx.bstride = mod2, n_dir, bstride
        ctx.frame, ctx.state, ctx.flow, ctx.bound = frame_, state_, flow_, bound_
        ctx.need = (frame.requires_grad, state is not None and state.requires_grad, flow is not None and flow.requires_grad)
        ctx.set_materialize_grads(False)
        if features is None:                         # a consumer that reads (and differentiates through) the NHWC state itself
            return (None, None, acts[nb]) if mod2 is not None else (None, acts[nb])
        if mod2 is not None:
            # the two trunks' features as two outputs: slicing one output outside would cost autograd a fill, a copy and an add per
            # half and step on the way back
            return out[:n_dir], out[n_dir:], acts[nb]
        return out, acts[nb]

    @staticmethod
    def backward(ctx, *grads):
        import ctypes
        if ctx.mod2 is not None:
            dya, dyb, dnext = grads
            dy = None
        else:
            dy, dnext = grads
            dya = dyb = None
        mod, acts, mids, blob = ctx.mod, ctx.acts, ctx.mids, ctx.blob
        frame, state, flow, bound = ctx.frame, ctx.state, ctx.flow, ctx.bound
        dt, nb, nf = mod.hot_dtype, mod.num_block, mod.num_feat
        _, n, h, w, _ = acts.shape
        dev = acts.device
        need_frame, need_state, need_flow = ctx.need
        n_dir, bstride, mod2 = ctx.n_dir, ctx.bstride, ctx.mod2
        # two trunks: half of the cap each, at least one workgroup per trunk (a cap of 1 halves to 0)
        wgs = _wgrad_wgs(n, h, w) if not n_dir else 2 * _wgrad_wgs(n_dir, h, w, max(1, int(os.environ.get("SR_C3_WGRAD_WGS", 64)) // 2))
        with torch.cuda.device(dev):
            _, _, boff, _ = _trunk_tables(27, nb, dev.index)
            s0, d0, s1, d1 = _unpack_tables(27, dev.index)
            ga = torch.empty_like(acts)
            gt = torch.empty_like(mids)
            tgt = ga[nb]
            if ctx.mod2 is not None:                      # per half: its feature gradient (or none) plus the state's
                for sl, d in ((slice(0, n_dir), dya), (slice(n_dir, None), dyb)):
                    t_, dn = tgt[sl], (dnext[sl] if dnext is not None else None)
                    if d is not None:
                        src = d.permute(0, 2, 3, 1)
                        if nf < 24:
                            t_.zero_()
                            t_[..., :nf] = src
                            if dn is not None:
                                t_.add_(dn)
                        elif dn is not None:
                            torch.add(src, dn, out=t_)
                        else:
                            t_.copy_(src)
                    elif dn is not None:
                        t_.copy_(dn)
                    else:
                        t_.zero_()
            elif dy is not None:
                src = dy.permute(0, 2, 3, 1)
                if nf < 24:
                    tgt.zero_()
                    tgt[..., :nf] = src
                    if dnext is not None:
                        tgt.add_(dnext)
                elif dnext is not None:
                    torch.add(src, dnext, out=tgt)
                else:
                    tgt.copy_(src)
            elif dnext is not None:
                tgt.copy_(dnext)
            else:
                tgt.zero_()
            parts = torch.empty((1 + 2 * nb, wgs, 9 * 1024), dtype=torch.float32, device=dev)
            need_dx0 = need_frame or need_state or need_flow
            dx0 = torch.empty((n, h, w, 32), dtype=dt, device=dev) if need_dx0 else None
            dstate = torch.empty((n, h, w, 24), dtype=dt, device=dev) if (need_state or need_flow) and state is not None else None
            dflow = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev) if need_flow else None
            warp = L.C3Warp(frame.data_ptr(), frame.stride(0), state.data_ptr() if state is not None else None,
                            flow.data_ptr() if flow is not None else None, flow.stride(0) if flow is not None else 0,
                            bound.data_ptr() if bound is not None else None,
                            dstate.data_ptr() if dstate is not None else None,
                            dflow.data_ptr() if dflow is not None else None, 2 * h * w,
                            ctx.x0.data_ptr() if ctx.x0 is not None else None)
            total = s0.numel() + 2 * nb * s1.numel()
            gflat = torch.empty(total * (2 if n_dir else 1), dtype=torch.float32, device=dev)
            unpack = L.C3Unpack(s0.data_ptr(), d0.data_ptr(), s0.numel(), s1.data_ptr(), d1.data_ptr(), s1.numel(), gflat.data_ptr())
            _launch("sr_c3_trunk_bwd", None, ctypes.byref(warp), acts.data_ptr(), mids.data_ptr(), ga.data_ptr(), gt.data_ptr(),
                    blob.data_ptr(), boff, parts.data_ptr(), dx0.data_ptr() if dx0 is not None else None, ctypes.byref(unpack),
                    nb, wgs, n, h, w, 32, L.DTYPE_CODE[dt], n_dir, bstride)
            dframe = dx0[..., :3].permute(0, 3, 1, 2).float() if need_frame else None
            g1, g2 = (gflat[:total], gflat[total:]) if n_dir else (gflat, None)
            if mod._pad:
                g1 = g1.index_select(0, mod._unpad_idx)
                if g2 is not None:
                    g2 = g2.index_select(0, mod2._unpad_idx)
        return dframe, (dstate if need_state else None), dflow, None, None, g1, None, g2, None


# ---- the 64-wide training route (opt-in: hot_training): sr_c64_trunk_train_fwd / sr_c64_trunk_bwd ----
WGRAD64_WGS = 64                                       # cap on the weight-gradient workgroups per conv


def _wgrad64_wgs(n, h, w, n_dir=0):
    """workgroups per conv of the 64-wide weight-gradient launches: _wgrad_wgs under the cap WGRAD64_WGS; two trunks in one launch
    take half of the cap each, at least one workgroup per trunk"""
    if n_dir:
        return 2 * _wgrad_wgs(n_dir, h, w, max(1, WGRAD64_WGS // 2))
    return _wgrad_wgs(n, h, w, WGRAD64_WGS)


def _pair_bwd_blob(mod, flat, mod2, flat2):
    """the two trunks' backward blobs one behind the other (cached until either parameter changes)"""
    b1, b2 = mod._packed_bwd(flat), mod2._packed_bwd(flat2)
    key = (b1.data_ptr(), mod._bwd_blob_key, b2.data_ptr(), mod2._bwd_blob_key)
    if getattr(mod, "_pair_bwd_key", None) != key:
        mod._pair_bwd_t = torch.cat([b1, b2])
        mod._pair_bwd_key = key
    return mod._pair_bwd_t, b1.numel()


class _Trunk64TrainFunction(torch.autograd.Function):
    """The wide trunk with a backward, one C call each way.  plain: `inp` is the NCHW input of ConvResidualBlocks.__call__ and the
    output the NCHW fp32 features.  Otherwise the contract of _TrunkWarpFunction at 64 channels: `inp` = frames, outputs (features,
    state) or, with `mod2` (two trunks in the same launches), (features_a, features_b, state); the state is a_nb, NHWC in the hot
    dtype, and its gradient comes back and goes out in that layout.  Saved: acts a_0..a_nb, mids t_0..t_{nb-1} and, when a weight
    gradient is wanted, the first conv's gathered input x0."""

    @staticmethod
    def forward(ctx, inp, state, flow, bound, mod, flat, mod2, flat2, features, plain):
        import ctypes
        dt, nb, f = mod.hot_dtype, mod.num_block, mod.num_feat
        n, _, h, w = inp.shape
        dev = inp.device
        want_w = ctx.needs_input_grad[5] or (mod2 is not None and ctx.needs_input_grad[7])
        with torch.cuda.device(dev):
            if mod2 is None:
                blob, n_dir, bstride = mod._packed(flat), 0, 0
            else:
                if n % 2 or (mod2.num_block, mod2.hot_dtype, mod2.num_feat, mod2.cin_k) != (nb, dt, f, mod.cin_k):
                    raise ValueError("two trunks in one call: an even batch (one half per trunk) and trunks of the same geometry")
                blob, bstride = _pair_blob(mod, flat, mod2, flat2)
                n_dir = n // 2
            _, boff, ci_k = _trunk64_tables(mod.num_in_ch, f, nb, dev.index if dev.index is not None else torch.cuda.current_device())
            acts = torch.empty((nb + 1, n, h, w, 64), dtype=dt, device=dev)
            mids = torch.empty((max(nb, 1), n, h, w, 64), dtype=dt, device=dev)
            frame_ = flow_ = state_ = bound_ = warp = None
            if plain:
                x0 = torch.zeros((n, h, w, ci_k), dtype=dt, device=dev)
                src = inp.detach().permute(0, 2, 3, 1)
                if ci_k == 80:                           # the (f + 3)-channel concat [frame | state] -> [state | frame | 0]
                    x0[..., :f] = src[..., 3:]
                    x0[..., 64:67] = src[..., :3]
                else:
                    x0[..., :f] = src
            else:
                frame_ = _inner_contiguous(inp.detach().float())
                flow_ = _inner_contiguous(flow.detach().float()) if flow is not None else None
                state_ = state.detach() if state is not None else None
                if state_ is not None and (state_.shape != (n, h, w, 64) or state_.dtype != dt or not state_.is_contiguous()):
                    raise ValueError("state must be the handle returned by the previous forward_warped call of this clip")
                if flow_ is not None and flow_.shape != (n, 2, h, w):
                    raise ValueError(f"expected N x 2 x H x W flow, got {tuple(flow_.shape)}")
                bound_ = bound.detach().float().reshape(()) if bound is not None else None
                x0 = torch.empty((n, h, w, 80), dtype=dt, device=dev) if want_w else None
                warp = L.C3Warp(frame_.data_ptr(), frame_.stride(0), state_.data_ptr() if state_ is not None else None,
                                flow_.data_ptr() if flow_ is not None else None, flow_.stride(0) if flow_ is not None else 0,
                                None, None, None, 0, x0.data_ptr() if x0 is not None else None)
            _launch("sr_c64_trunk_train_fwd", x0.data_ptr() if plain else None, ctypes.byref(warp) if warp is not None else None,
                    acts.data_ptr(), mids.data_ptr(), blob.data_ptr(), boff, nb, n, h, w, ci_k, L.DTYPE_CODE[dt], n_dir, bstride)
            out = _features64(acts[nb], f) if features else None
        ctx.mod, ctx.mod2, ctx.acts, ctx.mids, ctx.x0 = mod, mod2, acts, mids, x0
        ctx.flat, ctx.flat2, ctx.want_w = flat, flat2, want_w
        ctx.n_dir, ctx.plain, ctx.ci_k = n_dir, plain, ci_k
        ctx.frame, ctx.state, ctx.flow, ctx.bound = frame_, state_, flow_, bound_
        ctx.need = (inp.requires_grad, state is not None and state.requires_grad, flow is not None and flow.requires_grad)
        ctx.set_materialize_grads(False)
        if plain:
            return out
        if mod2 is not None:
            return (out[:n_dir], out[n_dir:], acts[nb]) if features else (None, None, acts[nb])
        return out, acts[nb]

    @staticmethod
    def backward(ctx, *grads):
        import ctypes
        mod, mod2, acts, mids = ctx.mod, ctx.mod2, ctx.acts, ctx.mids
        dt, nb, f, cin = mod.hot_dtype, mod.num_block, mod.num_feat, mod.num_in_ch
        _, n, h, w, _ = acts.shape
        dev = acts.device
        n_dir, plain, ci_k = ctx.n_dir, ctx.plain, ctx.ci_k
        need_in, need_state, need_flow = ctx.need
        if plain:
            parts_in = [(slice(None), grads[0], None)]
        elif mod2 is not None:
            dn = grads[2]
            parts_in = [(slice(0, n_dir), grads[0], None if dn is None else dn[:n_dir]),
                        (slice(n_dir, None), grads[1], None if dn is None else dn[n_dir:])]
        else:
            parts_in = [(slice(None), grads[0], grads[1])]
        with torch.cuda.device(dev):
            di = dev.index if dev.index is not None else torch.cuda.current_device()
            _, tab, (s0, d0, s1, d1) = _trunk64_bwd_tables(cin, f, nb, di)
            ga = torch.empty_like(acts)
            gt = torch.empty_like(mids)
            for sl, d, dn in parts_in:                    # d(loss)/d(a_nb): the features' gradient (NCHW fp32) plus the state's (NHWC)
                t_ = ga[nb][sl]
                if d is not None:
                    src = d.permute(0, 2, 3, 1)
                    if f < 64:
                        t_.zero_()
                        t_[..., :f] = src
                        if dn is not None:
                            t_.add_(dn)
                    elif dn is not None:
                        torch.add(src, dn, out=t_)
                    else:
                        t_.copy_(src)
                elif dn is not None:
                    t_.copy_(dn)
                else:
                    t_.zero_()
            if mod2 is None:
                bblob, bstride = mod._packed_bwd(ctx.flat), 0
            else:
                bblob, bstride = _pair_bwd_blob(mod, ctx.flat, mod2, ctx.flat2)
            need_frame = need_in and ci_k == 80           # the frame (or, plain, the first three input channels): conv 0's second half
            boff = list(tab["boff"])
            if not need_frame:
                boff[-1] = -1
            boff = (ctypes.c_long * len(boff))(*boff)
            need_dx0 = need_in or need_state or need_flow      # the flow's gradient reads dx0's state half
            dx0 = torch.empty((2 if need_frame else 1, n, h, w, 64), dtype=dt, device=dev) if need_dx0 else None
            dstate = torch.empty((n, h, w, 64), dtype=dt, device=dev) if need_state else None
            dflow = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev) if need_flow else None
            warp = None
            if not plain:
                frame, state, flow, bound = ctx.frame, ctx.state, ctx.flow, ctx.bound
                warp = L.C3Warp(frame.data_ptr(), frame.stride(0), state.data_ptr() if state is not None else None,
                                flow.data_ptr() if flow is not None else None, flow.stride(0) if flow is not None else 0,
                                bound.data_ptr() if bound is not None else None,
                                dstate.data_ptr() if dstate is not None else None,
                                dflow.data_ptr() if dflow is not None else None, 2 * h * w,
                                ctx.x0.data_ptr() if ctx.x0 is not None else None)
            wgs, parts, unpack, gflat = 0, None, None, None
            total = tab["n0"] + 2 * nb * tab["n1"]
            if ctx.want_w:
                wgs = _wgrad64_wgs(n, h, w, n_dir)
                parts = torch.empty(wgs * (tab["slab0"] + 2 * nb * tab["slab1"]), dtype=torch.float32, device=dev)
                gflat = torch.empty(total * (2 if n_dir else 1), dtype=torch.float32, device=dev)
                unpack = L.C3Unpack(s0.data_ptr(), d0.data_ptr(), s0.numel(), s1.data_ptr(), d1.data_ptr(), s1.numel(), gflat.data_ptr())
            _launch("sr_c64_trunk_bwd", ctx.x0.data_ptr() if plain else None,
                    ctypes.byref(warp) if warp is not None else None, acts.data_ptr(), mids.data_ptr(), ga.data_ptr(), gt.data_ptr(),
                    bblob.data_ptr(), boff, parts.data_ptr() if parts is not None else None,
                    dx0.data_ptr() if dx0 is not None else None, ctypes.byref(unpack) if unpack is not None else None, nb, wgs,
                    n, h, w, ci_k, L.DTYPE_CODE[dt], n_dir, bstride)
            din = None
            if need_in and plain:
                din = torch.empty((n, cin, h, w), dtype=torch.float32, device=dev)
                if ci_k == 80:
                    din[:, :3].copy_(dx0[1][..., :3].permute(0, 3, 1, 2))
                    din[:, 3:].copy_(dx0[0][..., :f].permute(0, 3, 1, 2))
                else:
                    din.copy_(dx0[0][..., :f].permute(0, 3, 1, 2))
            elif need_in:
                din = dx0[1][..., :3].permute(0, 3, 1, 2).float()
            g1 = g2 = None
            if gflat is not None:
                g1, g2 = (gflat[:total], gflat[total:]) if n_dir else (gflat, None)
                if not ctx.needs_input_grad[5]:
                    g1 = None
                if mod2 is not None and not ctx.needs_input_grad[7]:
                    g2 = None
        return din, dstate, dflow, None, None, g1, None, g2, None, None


# ---- the 64-wide inference route (csrc/conv64.h via sr_c64_trunk_fwd): no autograd.Function, nothing saved ----
def _run64(mod, x0, warp, n, h, w, dev, blob, n_dir=0, bstride=0):
    """the whole trunk in one C call; scratch = a ping-pong pair of 64-channel images, output = a third (the state handle)"""
    import ctypes
    dt, nb = mod.hot_dtype, mod.num_block
    _, boff, ci_k = _trunk64_tables(mod.num_in_ch, mod.num_feat, nb, dev.index if dev.index is not None else torch.cuda.current_device())
    out = torch.empty((n, h, w, 64), dtype=dt, device=dev)
    scratch = torch.empty((2, n, h, w, 64), dtype=dt, device=dev) if nb > 0 else None
    _launch("sr_c64_trunk_fwd", x0.data_ptr() if x0 is not None else None, ctypes.byref(warp) if warp is not None else None,
            scratch[0].data_ptr() if scratch is not None else None, scratch[1].data_ptr() if scratch is not None else None,
            out.data_ptr(), blob.data_ptr(), boff, nb, n, h, w, ci_k, L.DTYPE_CODE[dt], n_dir, bstride)
    return out


def _features64(img, f):
    """NHWC hot-dtype image -> the reference's NCHW fp32 features (the real f channels)"""
    n, h, w, _ = img.shape
    out = torch.empty((n, f, h, w), dtype=torch.float32, device=img.device)
    out.copy_(img[..., :f].permute(0, 3, 1, 2))
    return out


def _trunk64_plain(mod, fea):
    """ConvResidualBlocks.forward at 24 < F <= 64: NCHW input (reference channel order) -> NHWC in the kernels' layout"""
    n, _, h, w = fea.shape
    f, dev = mod.num_feat, fea.device
    x0 = torch.zeros((n, h, w, mod.cin_k), dtype=mod.hot_dtype, device=dev)
    src = fea.detach().permute(0, 2, 3, 1)
    if mod.cin_k == 80:                              # the (f + 3)-channel concat [frame | state] -> [state | frame | 0]
        x0[..., :f] = src[..., 3:]
        x0[..., 64:67] = src[..., :3]
    else:
        x0[..., :f] = src
    return _features64(_run64(mod, x0, None, n, h, w, dev, mod._packed(mod.flat)), f)


def _trunk64_warped(frame, state, flow, mod, mod2=None, features=True):
    """forward_warped (mod2 None) or forward_warped_pair at 24 < F <= 64: returns (features, state) or (features_a, features_b, state);
    features=False skips the NHWC -> NCHW fp32 copy (the features are None)"""
    n, _, h, w = frame.shape
    dev, dt = frame.device, mod.hot_dtype
    frame_ = _inner_contiguous(frame.detach().float())
    flow_ = _inner_contiguous(flow.detach().float()) if flow is not None else None
    state_ = state.detach() if state is not None else None
    if state_ is not None and (state_.shape != (n, h, w, 64) or state_.dtype != dt or not state_.is_contiguous()):
        raise ValueError("state must be the handle returned by the previous forward_warped call of this clip")
    if flow_ is not None and flow_.shape != (n, 2, h, w):
        raise ValueError(f"expected N x 2 x H x W flow, got {tuple(flow_.shape)}")
    with torch.cuda.device(dev):
        if mod2 is None:
            blob, n_dir, bstride = mod._packed(mod.flat), 0, 0
        else:
            if n % 2 or (mod2.num_block, mod2.hot_dtype, mod2.num_feat, mod2.cin_k) != (mod.num_block, dt, mod.num_feat, mod.cin_k):
                raise ValueError("two trunks in one call: an even batch (one half per trunk) and trunks of the same geometry")
            blob, bstride = _pair_blob(mod, mod.flat, mod2, mod2.flat)
            n_dir = n // 2
        warp = L.C3Warp(frame_.data_ptr(), frame_.stride(0), state_.data_ptr() if state_ is not None else None,
                        flow_.data_ptr() if flow_ is not None else None, flow_.stride(0) if flow_ is not None else 0,
                        None, None, None, 0, None)
        img = _run64(mod, None, warp, n, h, w, dev, blob, n_dir, bstride)
        if not features:
            return (None, None, img) if mod2 is not None else (None, img)
        feat = _features64(img, mod.num_feat)
    if mod2 is not None:
        return feat[:n_dir], feat[n_dir:], img
    return feat, img


_SIDE = {}


def _side_stream(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


def _fusable(trunk):
    return isinstance(trunk, ConvResidualBlocks) and trunk.num_in_ch == trunk.num_feat + 3


def _records_graph(mods, *inputs):
    """the condition _wide_route tests: would this call record an autograd graph?"""
    return torch.is_grad_enabled() and (any(p.requires_grad for m in mods for p in m.parameters()) or
                                        any(t is not None and t.requires_grad for t in inputs))


def paired(backward_trunk, forward_trunk):
    """do the two directions of a frame step share their launches (forward_warped_pair)?  Two distinct fusable trunks of one geometry"""
    return (_fusable(backward_trunk) and _fusable(forward_trunk) and backward_trunk is not forward_trunk and
            (backward_trunk.num_block, backward_trunk.hot_dtype, backward_trunk.num_feat) ==
            (forward_trunk.num_block, forward_trunk.hot_dtype, forward_trunk.num_feat) and
            os.environ.get("SR_VSR_SEPARATE_DIRECTIONS", "0") != "1")


def propagate(x, flows_forward, flows_backward, backward_trunk, forward_trunk, flow_warp, num_feat=24, handles=False,
              step_states=False):
    """The two recurrent loops of the reference (mvvsr_arch.py:72-93 / basicvsr_arch.py:67-88):
    returns (backward features, forward features) per frame.  x: (b, n, 3, h, w); flows: (b, n-1, 2, h, w).
    handles=True (inference only: the call must not record a graph) returns the per-frame NHWC state handles in the hot dtype
    instead -- (b, h, w, 24) images on the narrow route (a copy of `acts[nb]` that owns its storage, so that the step's other
    activations die with the step), (b, h, w, 64) on the wide route (the trunk's output image), channels >= num_feat exactly zero
    -- and skips the NCHW fp32 feature copies on every branch.  The backward-time handles of all frames stay alive until the caller
    drops them: one state image per frame and direction.
    step_states=True (the paired route of the 24-wide trunks, or of two wide trunks that have both opted in with `hot_training`: (2b,
    h, w, 64) states; a graph MAY be recorded) returns ONE list instead: the state of every
    frame step k, (2b, h, w, 24) in the hot dtype = [backward-time loop at frame n - 1 - k | forward-time loop at frame k], the very
    tensors the trunk Function returned -- a consumer that differentiates through them hands `dnext` back in the same layout, with
    no slice, fill or add in between.  The NCHW fp32 feature copies are skipped."""
    b, n, _, h, w = x.shape
    out_b, out_f = [], []
    from .spynet_arch import flow_warp as hot_flow_warp
    fused = _fusable(backward_trunk) and _fusable(forward_trunk) and flow_warp is hot_flow_warp and x.is_cuda
    if handles:
        if not fused:
            raise L.HotpathError("propagate(handles=True) needs the fused route: two ConvResidualBlocks(F + 3, F, n) trunks, the hot "
                                 "flow_warp and CUDA/HIP tensors")
        if _records_graph((backward_trunk, forward_trunk), x, flows_forward, flows_backward):
            raise NotImplementedError("propagate(handles=True) is an inference route: call it under torch.no_grad()")
    if step_states and not (fused and paired(backward_trunk, forward_trunk) and
                            (not backward_trunk.wide or (backward_trunk.hot_training and forward_trunk.hot_training))):
        raise L.HotpathError("propagate(step_states=True) needs the paired route of two 24-wide ConvResidualBlocks(F + 3, F, n) trunks")
    if fused:
        # warp + concat gathered into the first conv (ConvResidualBlocks.forward_warped); one bound for the whole clip
        bound = None
        if n > 1:
            bound = torch.maximum(flows_forward.detach().abs().amax(), flows_backward.detach().abs().amax())
        # The two directions are independent recurrences and one of them fills barely half of the chip (144 workgroups at
        # 8 clips of 64x64): the backward-time loop runs on a side stream, the forward-time loop on the caller's; autograd
        # replays each node's backward on the stream its forward ran on.  Opt-in (SR_VSR_TWO_STREAMS=1): at C4 the step is bound
        # by host issue, and the stream switches cost more host time (2.24 -> 2.63 ms) than the overlap returns.
        if paired(backward_trunk, forward_trunk):
            # both directions of a frame step in ONE set of launches (round 3): step k = the backward-time loop's frame n - 1 - k next to
            # the forward-time loop's frame k, batched; the trunk kernels pick the weights by batch half
            xp = torch.cat([x.flip(1), x], 0)
            fl = torch.cat([flows_backward.flip(1), flows_forward], 0) if n > 1 else None
            state, steps = None, []
            for k in range(n):
                fb, ff, state = forward_warped_pair(backward_trunk, forward_trunk, xp[:, k], state, fl[:, k - 1] if k > 0 else None, bound,
                                                    features=None if step_states else not handles)
                if step_states:
                    steps.append(state)
                    continue
                out_b.insert(0, state[:b] if handles else fb)
                out_f.append(state[b:] if handles else ff)
            return steps if step_states else (out_b, out_f)
        cur = torch.cuda.current_stream(x.device)
        side = _side_stream(x.device) if os.environ.get("SR_VSR_TWO_STREAMS", "0") == "1" else cur
        if side is not cur:
            side.wait_stream(cur)
        with torch.cuda.stream(side):
            state = None
            for i in range(n - 1, -1, -1):
                feat, state = backward_trunk.forward_warped(x[:, i], state, flows_backward[:, i] if i < n - 1 else None, bound,
                                                            features=not handles)
                out_b.insert(0, state if handles else feat)
        state = None
        for i in range(n):
            feat, state = forward_trunk.forward_warped(x[:, i], state, flows_forward[:, i - 1] if i > 0 else None, bound,
                                                       features=not handles)
            out_f.append(state if handles else feat)
        if side is not cur:
            cur.wait_stream(side)
            for t in out_b:
                t.record_stream(cur)                 # allocated on the side stream, consumed on the caller's
        return out_b, out_f
    feat = x.new_zeros(b, num_feat, h, w)
    for i in range(n - 1, -1, -1):
        if i < n - 1:
            feat = flow_warp(feat, flows_backward[:, i].permute(0, 2, 3, 1))
        feat = backward_trunk(torch.cat([x[:, i], feat], dim=1))
        out_b.insert(0, feat)
    feat = torch.zeros_like(feat)
    for i in range(n):
        if i > 0:
            feat = flow_warp(feat, flows_forward[:, i - 1].permute(0, 2, 3, 1))
        feat = forward_trunk(torch.cat([x[:, i], feat], dim=1))
        out_f.append(feat)
    return out_b, out_f


class BasicVSR(nn.Module):
    """The trainer's 'basic' model (reference: models/basicvsr_arch.py:10-105; constructed at
    train_video_superresolution.py:249 as BasicVSR(num_feat=24, num_block=8, spynet_path=...)).

    Same constructor, same submodules in the same order (so a seeded init and the state_dict keys agree; `spynet.*` follows
    the vendored models/spynet_arch.py naming -- the reference imports mmedit's SPyNet here, which is not in the repository),
    `.scale`, `get_flow` and `forward(x, height, weight)`: SpyNet flows (MFMA kernels) -> the two recurrent propagation loops
    (HIP, warp + concat gathered into the first conv) -> fusion -> conv_last -> bilinear resize -> `out += base`.  The last
    statement fails in the REFERENCE as well: conv_last is ConvTranspose2d(2F -> F), so `out` has F channels and `base` three
    (basicvsr_arch.py:36,96-100; SURVEY section 0: "RuntimeError: size of tensor a (24) must match b (3)"); conv_hr (F -> 3) is
    defined and never called.  The same statement is kept, so the same error is raised -- after the propagation half, which is
    what `propagation_features` exposes for use and for the parity tests."""

    def __init__(self, num_feat=64, num_block=15, spynet_path=None, hot_dtype=None):
        super().__init__()
        from .spynet_arch import SpyNet
        self.num_feat = num_feat
        self.spynet = SpyNet(spynet_path)
        self.scale = 4
        self.backward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block, hot_dtype=hot_dtype)
        self.forward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block, hot_dtype=hot_dtype)
        self.fusion = nn.Conv2d(num_feat * 2, num_feat * 2, 1, 1, 0, bias=True)
        self.upconv1 = nn.Conv2d(num_feat, num_feat * 4, 3, 1, 1, bias=True)
        self.upconv2 = nn.Conv2d(num_feat, num_feat * 4, 3, 1, 1, bias=True)
        self.conv_last = nn.ConvTranspose2d(num_feat * 2, num_feat, 5, stride=self.scale)
        self.conv_hr = nn.Conv2d(num_feat, 3, 3, 1, 1)
        self.pixel_shuffle = nn.PixelShuffle(2)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)

    def get_flow(self, x):
        b, n, c, h, w = x.size()
        x_1 = x[:, :-1, :, :, :].reshape(-1, c, h, w)
        x_2 = x[:, 1:, :, :, :].reshape(-1, c, h, w)
        flows_backward = self.spynet(x_1, x_2).view(b, n - 1, 2, h, w)
        flows_forward = self.spynet(x_2, x_1).view(b, n - 1, 2, h, w)
        return flows_forward, flows_backward

    def propagation_features(self, x, flows=None):
        """(backward features, forward features) per frame: basicvsr_arch.py:67-88 without the reconstruction"""
        from .spynet_arch import flow_warp
        flows_forward, flows_backward = flows if flows is not None else self.get_flow(x)
        return propagate(x, flows_forward, flows_backward, self.backward_trunk, self.forward_trunk, flow_warp, num_feat=self.num_feat)

    def forward(self, x, height=1080, weight=1920):
        feat_b, feat_f = self.propagation_features(x)
        out_l = []
        for i in range(x.size(1)):
            out = torch.cat([feat_b[i], feat_f[i]], dim=1)
            out = self.lrelu(self.fusion(out))
            out = self.conv_last(out)
            out = nn.functional.interpolate(out, size=(height, weight), mode='bilinear')
            base = nn.functional.interpolate(x[:, i], size=(height, weight), mode='bilinear', align_corners=False)
            out += base                              # (F channels += 3 channels: raises, as in the reference)
            out_l.append(out)
        return torch.stack(out_l, dim=1)
