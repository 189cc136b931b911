"""The loss-fold protocol between a criterion of mobilesuperresolution_amd.training and the autograd node whose output it is applied to:
BASIC_MODEL's whole-network node (basic_wdsr_b._NetFunction), NAS_MODEL's tail node (wdsr_b._TailFunction) and the video networks' clip
nodes (clip_train.ClipTrain).

A node ends its forward with `arm(ctx, out)` and gives one hook, a static method of its Function class,
    run_folded(node, sr, hr, kind_code, gscale) -> (payload, loss_part)
its HIP backward with d(loss)/d(out) formed inside the kernel from `sr` (its own output) and a contiguous `hr`; the payload is a tensor or a tuple of
tensors (the gradients it will return), loss_part the per-workgroup loss sums.  Its backward sets `ctx.ran = True`, then asks
`take_folded(ctx, g)`.

The criterion asks `can_fold(node, sr, hr)`, THE RULE: `sr` is the node's own contiguous fp32 output, `hr` is fp32, on the same device,
of the same shape and needs no gradient, and the node has neither been folded (nor is about to be: `fold_started`) nor run, nor has it
set `foldable = False` after arm() (the per-frame network's node at an output size other than (4H, 4W) unless the model's
`hot_resize_fold` is set: its folded backward then runs at any size, sr_fn_net_bwd_loss_sized).  Anything
else -- a second criterion on the same output among them -- keeps torch's ops, and its gradient reaches the node as an ordinary `g`.
When the rule holds, `fold(node, sr, hr, kind)` runs the hook at once with loss weight 1; the criterion's backward parks
(payload, loss gradient, data pointer of its zero token) on the node as `folded` and sends the token up the graph, and the node's
backward returns the payload times the loss gradient, plus its plain backward of `g` when `g` is more than the token."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from .. import hotpath as HP


def arm(ctx, out):
    """the end of a node's forward(): the protocol's state, and the hook where the criterion finds it (the backward node is no instance
    of the Function's class, so class attributes do not show on it)"""
    ctx.out_ptr, ctx.folded, ctx.fold_started, ctx.ran = out.data_ptr(), None, False, False
    ctx.run_folded = ctx._forward_cls.run_folded


def can_fold(node, sr, hr) -> bool:
    return (getattr(node, "foldable", True) and node.folded is None and not node.fold_started and not node.ran
            and sr.data_ptr() == node.out_ptr and sr.dtype == torch.float32
            and sr.is_contiguous() and hr.dtype == torch.float32 and hr.device == sr.device and hr.shape == sr.shape
            and not hr.requires_grad)


def gscale(weight: float, numel: int) -> float:
    """upstream gradient / numel as torch's mean-reduced loss backward forms it: an fp32 division of fp32 values"""
    return float(np.float32(weight) / np.float32(numel))


def fold(node, sr, hr, kind: str):
    """run the node's backward NOW with the criterion `kind` of (sr, hr) folded in (loss weight 1: the caller's scalar factors arrive
    through autograd) -> (payload, loss_part)"""
    node.fold_started = True
    with L.device_guard(sr.device):
        return node.run_folded(node, sr, hr, HP.LOSS_KINDS[kind], gscale(1.0, sr.numel()))


def take_folded(ctx, g):
    """in a node's backward -> (the parked payload times the loss gradient, or None when no criterion was folded; whether `g` is only
    the criterion's zero token, so that the payload is the whole answer)"""
    if ctx.folded is None:
        return None, False
    payload, gloss, token_ptr = ctx.folded
    if isinstance(payload, tuple):
        scaled = tuple(HP.scale_by(t, gloss) for t in payload)
    else:
        scaled = HP.scale_by(payload, gloss)
    return scaled, g.data_ptr() == token_ptr and all(s == 0 for s in g.stride())
