"""What the two video networks (models/single_image_model.py, models/naive_multi_model_easy.py) share around their HIP routes: the
clip autograd node with its loss-fold protocol, the checks of the route rule, the clip's frames and flows as the kernels read them, and
the cache of packed parameter blobs."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from .. import hotpath as HP
from .. import packing as P

_HOOKS = ("_forward_hooks", "_forward_pre_hooks")


class ClipTrain(torch.autograd.Function):
    """A whole clip through one HIP forward and one HIP backward.  apply(model, x, .., *eff): LEAD inputs without a gradient, then the
    EFFECTIVE tensors, the encoder's (weight, bias) first; backward returns their gradients as views of one flat fp32 vector, the
    weight-norm backward onto (g, v) is torch's.  A subclass gives
      * forward(ctx, ..): allocation, the HIP forward, `ctx.saved` (the fp32 frames (B N, 3, H, W) first) and `ctx.geom` (channels and
        blocks first), then `return cls._record(ctx, out, eff)`;
      * _run_backward(ctx, g, hr=None, kind=0, gscale=0.0): the HIP backward from g = d(loss)/d(out), or with hr from g = the network's
        output -> (flat gradients, the encoder's LAST, per-workgroup loss sums or None);
      * _grad_sizes(channel, nb): the flat vector's pieces; LEAD.

    The node protocol of mobilesuperresolution_amd.training's criteria (wdsr_b._TailFunction carries its own, for a pair):
    `can_fold(node, sr, hr)` is the whole rule for folding the loss into this node's backward; `fold_loss(node, sr, hr, kind)` runs that
    backward at once, the output gradient formed inside its first stage, and returns (the flat gradient vector, the loss sums); the
    criterion parks it as `folded`, and backward() hands it over, times the incoming loss gradient, when it receives the criterion's
    zero token."""
    LEAD = 2

    @staticmethod
    def _can_fold(node, sr, hr) -> bool:
        return (node.folded is None and not node.fold_started and not node.ran and sr.data_ptr() == node.out_ptr and sr.dtype == torch.float32
                and sr.is_contiguous() and hr.dtype == torch.float32 and hr.device == sr.device and hr.shape == sr.shape
                and not hr.requires_grad)

    @staticmethod
    def _fold_loss(node, sr, hr, kind):
        gscale = float(np.float32(1.0) / np.float32(sr.numel()))
        node.fold_started = True                             # a second criterion on the same output takes torch's ops
        with L.device_guard(node.saved[0].device):
            return node.cls._run_backward(node, sr, hr.contiguous(), HP.LOSS_KINDS[kind], gscale)

    @classmethod
    def _record(cls, ctx, out, eff):
        """the end of forward(): the protocol's state on the node"""
        ctx.cls = cls
        ctx.shapes = [t.shape for t in eff]
        ctx.out_ptr, ctx.folded, ctx.fold_started, ctx.ran = out.data_ptr(), None, False, False
        ctx.can_fold, ctx.fold_loss = cls._can_fold, cls._fold_loss
        return out

    @staticmethod
    def _split(ctx, grads):
        pieces = grads.split(ctx.cls._grad_sizes(ctx.geom[0], ctx.geom[1]))
        # grads holds the encoder last; eff has it first
        order = list(pieces[-2:]) + list(pieces[:-2])
        return (None,) * ctx.cls.LEAD + tuple(p.view(s) for p, s in zip(order, ctx.shapes))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        frames = ctx.saved[0]
        n, _, h, w = frames.shape
        ctx.ran = True
        with L.device_guard(frames.device):
            folded = None
            if ctx.folded is not None:
                # the criterion has run this backward already; `g` is its zero token (or the token plus the gradient of some OTHER
                # use of the output, which then runs the usual way)
                grads0, gloss, token_ptr = ctx.folded
                folded = HP.scale_by(grads0, gloss)
                if g.data_ptr() == token_ptr and all(st_ == 0 for st_ in g.stride()):
                    return ClipTrain._split(ctx, folded)
            g = g.reshape(n, 3, 4 * h, 4 * w)
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
            grads, _ = ctx.cls._run_backward(ctx, g)
            if folded is not None:
                grads = grads + folded
        return ClipTrain._split(ctx, grads)


def route_reason(model, x, who, *, train, kernel_reason, modules, params, trained=None, out_size=None, empty=None):
    """The checks both networks' hot_route_reason (train False) and train_route_reason (train True) make, in the order in which their
    reasons win; None when all pass.  model: `aten_forward`, `hot_training`, `scale`, `IN`.  The caller's own:
      kernel_reason  why the blocks do not fit the 3x3 kernels, or None;
      modules        the modules whose forward (pre-)hooks keep the ATen route;
      params         the parameters that must sit on x's device;
      trained        train: the parameters that must require grad;
      out_size       train, the network with a resize only: (height, weight), which must be (4H, 4W);
      empty          the reason when x is empty (or what the caller knows to be empty besides), else None."""
    if x.dim() != 5 or x.shape[2] != 3:
        raise ValueError(f"{who}: input (B, N, 3, H, W), got {tuple(x.shape)}")
    if train and not model.hot_training:
        return "hot_training is not set"
    if model.aten_forward:
        return "aten_forward is set"
    if model.scale != 4:
        return f"scale {model.scale} (the kernels upsample x4)"
    if not 1 <= model.IN <= P.FN_C:
        return f"{model.IN} channels (the kernels are 32 wide)"
    if kernel_reason:
        return kernel_reason
    if any(getattr(m, a, None) for m in modules for a in _HOOKS):
        return "a forward hook on a module"
    if not train and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in model.parameters())):
        return "the call records an autograd graph"
    if not x.is_cuda:
        return "CPU input"
    if any(p.device != x.device for p in params):
        return "parameters on another device"
    if train:
        if out_size is not None and tuple(out_size) != (4 * x.shape[3], 4 * x.shape[4]):
            return "output size is not (4H, 4W)"
        if x.requires_grad:
            return "the input requires grad (no input gradient is produced)"
        if not torch.is_grad_enabled():
            return "grad mode is off"
        if not all(p.requires_grad for p in trained):
            return "a frozen parameter"
    if empty:
        return empty
    if x.shape[0] * x.shape[1] > 65535 or x.shape[3] > 8192 or x.shape[4] > 8192:
        return "frame count or frame size beyond the kernels' grid"
    return None


def frames_of(x):
    """the clip (B, N, 3, H, W) as the kernels read it: (B N, 3, H, W) fp32 contiguous, detached"""
    b, n, _, h, w = x.shape
    frames = x.detach().reshape(b * n, 3, h, w)
    if frames.dtype != torch.float32 or not frames.is_contiguous():
        frames = frames.float().contiguous()
    return frames


def flows_of(flows, b, n, h, w):
    """the flows (B, N - 1, 2, H, W) as the kernels read them: fp32 contiguous, detached; None for a clip of one frame"""
    if n < 2:
        return None
    flows = flows.detach()
    if tuple(flows.shape) != (b, n - 1, 2, h, w):
        raise ValueError(f"Naive_model: flows {tuple(flows.shape)} for a clip {(b, n, 3, h, w)}")
    if flows.dtype != torch.float32 or not flows.is_contiguous():
        flows = flows.float().contiguous()
    return flows


def cached_blobs(model, name, params, backward, pack):
    """model.<name>_blobs, re-packed by pack() (under no_grad) only when the hot dtype, `backward` or one of `params` changed"""
    key = (model.hot_dtype, backward) + tuple((p.data_ptr(), p._version) for p in params)
    if getattr(model, name + "_key", None) != key:
        with torch.no_grad():
            blobs = pack()
        setattr(model, name + "_blobs", blobs)
        setattr(model, name + "_key", key)
    return getattr(model, name + "_blobs")


def state_without_blobs(model, name):
    """__getstate__ of a model that keeps cached_blobs(model, name, ..): device blobs do not travel with a pickle"""
    d = model.__dict__.copy()
    d.pop(name + "_blobs", None)
    d.pop(name + "_key", None)
    return d
