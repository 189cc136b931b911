"""Drop-ins for the two torch objects the reference trainers build next to the model, so that their training loops run
UNCHANGED on the fast route:

    pretrain.py:137      optim.Adam(filter(...model.parameters()), lr)        ->  training.Adam(...)
    pretrain.py:220      criterions = {'l1': nn.L1Loss()}                      ->  {'l1': training.L1Loss()}
    train_video_superresolution.py:43-53   L1_Charbonnier_loss()              ->  training.L1_Charbonnier_loss()

and then, as before (pretrain.py:69-82):

    optimizer.zero_grad(); sr = model(lr); loss = w * criterions['l1'](sr, hr); loss.backward(); optimizer.step(); loss.item()

What changes underneath.  `criterion(sr, hr)` recognises an `sr` that is the own output of one of four autograd nodes and, when
models/loss_fold.py's rule `can_fold(node, sr, hr)` holds (stated there, once), runs that node's backward right there with the loss
gradient formed inside its first kernel: no d(loss)/d(sr) tensor, none of the seven small ATen loss kernels.  `loss.backward()` then
only hands the parked gradients over, scaled by whatever the trainer multiplied the loss with.  The four nodes:

    BASIC_MODEL.forward (pretrain.py:69-82)                    the whole network; sr_tail_bwd_loss (csrc/wdsr_ends.h) leads its backward
    NAS_MODEL's `sr, speed = model(lr)` (search.py:74)         the tail; the body's backward runs later under autograd
    `--model_type single` / `multi` with hot_training = True   the clip (train_video_superresolution.py:86-100); sr_fn_net_bwd_loss /
                                                               sr_mf_net_bwd_loss (csrc/frame_net_bwd.h, csrc/multi_frame_bwd.h); torch's
                                                               weight-norm backward carries the gradients onto weight_g / weight_v

Anything the rule refuses (`sr` from another module, a sliced `sr`, an `hr` that is not fp32, a second criterion on the same output, no
grad mode) takes torch's own ops: that is the reference's behaviour, not a fallback of the hot path.

`Adam.step()` has torch.optim.Adam's arithmetic bit for bit (tests/test_gpu_train_step.py): a lone tensor (BASIC_MODEL's flat parameter)
is ONE launch of sr_adam_step, where torch's multi-tensor path takes ~43 us for it; a param group's tensors of equal step count go in
ceil(tensors / 80) launches of sr_adam_step_multi (one table of up to _lib.ADAM_MULTI_CAP rows per launch, passed in the kernel
arguments).  Its bookkeeping -- adam_scalars, ensure_adam_state, bump_version -- is also what the one-call steps use:
BASIC_MODEL.train_step with its own AdamState, and the video networks' `model.train_step(lr, hr, optimizer, criterion)`
(models/clip_train.py), whose `optimizer` is this module's Adam, its state read and written in place."""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from . import _lib as L
from .models import loss_fold

__all__ = ["L1Loss", "L1_Charbonnier_loss", "Adam", "adam_scalars", "ensure_adam_state", "bump_version"]


# the autograd nodes that carry the loss-fold protocol (models/loss_fold.py): BASIC_MODEL's whole network (models/basic_wdsr_b.py),
# NAS_MODEL's tail (models/wdsr_b.py), the two video networks' clip nodes (models/clip_train.ClipTrain, subclassed in
# single_image_model.py and naive_multi_model_easy.py)
_FOLDING_NODES = ("_NetFunctionBackward", "_TailFunctionBackward", "_FrameNetTrainBackward", "_MultiFrameTrainBackward")


def _network_node(sr: torch.Tensor):
    """the autograd node that produced `sr` if it is one of this package's folding nodes, else None"""
    fn = sr.grad_fn
    if fn is not None and type(fn).__name__ in _FOLDING_NODES and hasattr(fn, "run_folded"):
        return fn
    return None


class _FoldedCriterion(torch.autograd.Function):
    """loss(sr, hr) where sr is a folding node's own output: forward() runs the BACKWARD of sr's node with the loss gradient formed
    inside its first kernel (loss_fold.fold) and returns the loss value; backward() parks the result on the node and sends a
    zero-stride zero token up the graph in place of d(loss)/d(sr)."""

    @staticmethod
    def forward(ctx, sr, hr, node, kind):
        payload, loss_part = loss_fold.fold(node, sr, hr, kind)
        loss = torch.empty((), dtype=torch.float32, device=sr.device)
        with L.device_guard(sr.device):
            L.launch("sr_loss_value", L.lib().sr_loss_value, loss_part.data_ptr(), loss_part.numel(), 1.0 / sr.numel(), loss.data_ptr(),
                     L.stream_ptr(sr.device))
        ctx.node = node
        ctx.token = torch.zeros(1, dtype=sr.dtype, device=sr.device).expand(sr.shape)
        ctx.payload = payload
        return loss

    @staticmethod
    def backward(ctx, gloss):
        ctx.node.folded = (ctx.payload, gloss, ctx.token.data_ptr())
        return ctx.token, None, None, None


class _HotLoss(nn.Module):
    KIND = "l1"

    def forward(self, sr: torch.Tensor, hr: torch.Tensor) -> torch.Tensor:
        node = _network_node(sr) if (torch.is_grad_enabled() and sr.requires_grad) else None
        if node is None or not loss_fold.can_fold(node, sr, hr):
            return self._torch_loss(sr, hr)
        return _FoldedCriterion.apply(sr, hr.detach().contiguous(), node, self.KIND)


class L1Loss(_HotLoss):
    """nn.L1Loss() (mean reduction) -- pretrain.py:220 / :73"""
    KIND = "l1"

    def _torch_loss(self, sr, hr):
        return torch.nn.functional.l1_loss(sr, hr)


class L1_Charbonnier_loss(_HotLoss):
    """train_video_superresolution.py:43-53: mean(sqrt((X - Y)^2 + 1e-12))"""
    KIND = "charbonnier"

    def __init__(self):
        super().__init__()
        self.eps = 1e-12

    def _torch_loss(self, sr, hr):
        diff = torch.add(sr, -hr)
        return torch.mean(torch.sqrt(diff * diff + self.eps))


def adam_scalars(lr, betas, eps, t) -> "L.AdamScalars":
    """the scalars torch.optim.Adam hands its kernels at step count t: computed in double, rounded to float by the structure"""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return L.AdamScalars(1.0 - b1, b2, 1.0 - b2, math.sqrt(bc2), eps, -(lr / bc1))


def ensure_adam_state(state, p):
    """torch.optim.Adam's lazily created state of parameter p (`state` = optimizer.state[p]); existing state is left as it is"""
    if len(state) == 0:
        state["step"] = torch.tensor(0.0, dtype=torch.float32)
        state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


def bump_version(tensors):
    """`tensors` (a list) were written through their raw pointers: tell autograd (in-place version counters) without a launch"""
    try:
        torch.autograd.graph.increment_version(tensors)
    except AttributeError:                               # a torch without it
        with torch.no_grad():
            for t in tensors:
                t.add_(0)


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps) on csrc/train_step.h's kernels (same fused-multiply-add forms as torch's foreach
    implementation: parameters bit-identical): a param group's tensors of equal step count go through sr_adam_step_multi, up to
    _lib.ADAM_MULTI_CAP tensors per launch; a lone tensor (BASIC_MODEL's flat parameter) is ONE launch of adam_step_kernel.  State keys
    are torch's (`step`, `exp_avg`, `exp_avg_sq`), so optimizer checkpoints interchange (pretrain.py:262-267); schedulers
    (MultiStepLR, pretrain.py:139-142) act on `param_groups[i]['lr']` as usual.  weight_decay / amsgrad / maximize: not on the
    reference's path, rejected."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("training.Adam mirrors the reference's optim.Adam(params, lr): no weight decay, no amsgrad")
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))

    def zero_grad(self, set_to_none: bool = True):
        """torch.optim.Optimizer.zero_grad's effect without its per-call bookkeeping (profiler record, foreach grouping: ~12 us of host
        time for one parameter -- in the reference's loop that sits between the per-step `loss.item()` sync and the forward's first
        launch, i.e. it is GPU idle time)"""
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    if set_to_none:
                        p.grad = None
                    else:
                        p.grad.detach_()
                        p.grad.requires_grad_(False)
                        p.grad.zero_()

    @staticmethod
    def _tables(params, capacity=L.ADAM_MULTI_CAP, chunk=L.ADAM_MULTI_CHUNK):
        """The launches of one multi-tensor step over `params` (tensors with `grad is None` are left out): a list of tables, each a
        list of at most `capacity` rows (param, n, blk0): the tensor, its element count, and the first of its ceil(n / chunk)
        workgroups within the table's launch -- workgroup blk0 + j steps elements [j chunk, min((j + 1) chunk, n)).  Pure Python;
        sr_adam_step_multi lays its rows out the same way."""
        tables, rows, blk = [], [], 0
        for p in params:
            if p.grad is None:
                continue
            if len(rows) == capacity:
                tables.append(rows)
                rows, blk = [], 0
            n = p.numel()
            rows.append((p, n, blk))
            blk += (n + chunk - 1) // chunk
        if rows:
            tables.append(rows)
        return tables

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.lib()
        for group in self.param_groups:
            lr, betas, eps = float(group["lr"]), group["betas"], float(group["eps"])
            by_step = {}                                     # step count after this step -> [(param, contiguous grad, state)]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or g.dtype != torch.float32 or g.is_sparse:
                    raise L.HotpathError("training.Adam steps contiguous fp32 CUDA parameters (there is no CPU fallback)")
                g = g.contiguous()
                state = self.state[p]
                ensure_adam_state(state, p)
                state["step"] += 1
                by_step.setdefault((int(state["step"]), p.device), []).append((p, g, state))
            for (t, device), members in by_step.items():
                scal = adam_scalars(lr, betas, eps, t)
                with L.device_guard(device):
                    if len(members) == 1:
                        p, g, state = members[0]
                        L.launch("sr_adam_step", lib.sr_adam_step, p.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(),
                                 state["exp_avg_sq"].data_ptr(), p.numel(), ctypes.byref(scal), None, 0, 0.0, None, L.stream_ptr(device))
                    else:
                        by_param = {id(p): (g, state) for p, g, state in members}
                        for table in self._tables([p for p, _, _ in members]):
                            rows = (L.AdamRow * len(table))()
                            for r, (p, n, _) in zip(rows, table):
                                g, state = by_param[id(p)]
                                r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.n = (p.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(),
                                                                                 state["exp_avg_sq"].data_ptr(), n)
                            L.launch("sr_adam_step_multi", lib.sr_adam_step_multi, rows, len(table), ctypes.byref(scal),
                                     L.stream_ptr(device))
                bump_version([p for p, _, _ in members])
        return loss
