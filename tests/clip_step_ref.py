"""Float64 reference of the weight norm w = g v / |v| (torch.nn.utils.weight_norm, dim 0) forward and backward in closed form, as the video
networks' one-call training step computes it (csrc/clip_param_step.h), the parameter gradients of the two networks carried through it,
and the length of the fp32 chain the kernels add on the way from an effective-weight gradient to a weight_g / weight_v gradient.  Plain
torch on the CPU; tests/test_clip_step_host.py pins it against torch's weight norm and autograd, tests/test_gpu_clip_step.py holds the
kernels to it."""
import torch

from tests import frame_net_train_ref as FT

WN_SHAPES = ((8, 3, 3, 3), (32, 32, 3, 3), (48, 8, 3, 3))


def wn_forward(g, v):
    """(w, 1 / |v| per row) in float64; g (rows, 1, 1, 1), v (rows, ..)"""
    g, v = g.double(), v.double()
    inv = 1.0 / v.flatten(1).pow(2).sum(1).sqrt()
    return v * (g.flatten() * inv).view(-1, *([1] * (v.dim() - 1))), inv


def wn_backward(g, v, dw):
    """(dg like g, dv like v) in float64 from dw = d(loss)/dw: s = sum dw v per row, dg = s / |v|, dv = (g / |v|) (dw - v s / |v|^2)"""
    g, v, dw = g.double(), v.double(), dw.double()
    shape = (-1,) + (1,) * (v.dim() - 1)
    inv = 1.0 / v.flatten(1).pow(2).sum(1).sqrt()
    s = (dw * v).flatten(1).sum(1)
    dg = (s * inv).view(g.shape)
    dv = (g.flatten() * inv).view(shape) * (dw - v * (s * inv * inv).view(shape))
    return dg, dv


def wn_case(shape, sd=0):
    """(g, v, dw) float64 random; row 1 of v is scaled to 1e-4, so its 1 / |v| is large"""
    gen = torch.Generator().manual_seed(4100 + 17 * sd + sum(shape))
    v = torch.randn(shape, generator=gen, dtype=torch.float64)
    v[1] *= 1e-4
    g = torch.rand(shape[0], 1, 1, 1, generator=gen, dtype=torch.float64) + 0.5
    dw = torch.randn(shape, generator=gen, dtype=torch.float64)
    return g, v, dw


def wn_chain_length(row_len):
    """fp32 roundings on the longest path from an effective-weight gradient to an element of the weight_v gradient, as
    clip_wn_fwd_kernel / clip_wn_bwd_adam_kernel compute it for a row of `row_len` elements (one wave per row, lane l takes elements
    l, l + 64, ..):
      1 / |v| (forward)     ceil(len / 64) fused multiply-adds per lane, a six-level shuffle tree, the square root, the reciprocal
      s = sum dw v          the loss weight times dw, ceil(len / 64) fused multiply-adds per lane, a six-level shuffle tree
      dg = s / |v|          one product                                   (the weight_g gradient ends here)
      dv                    s / |v|^2, g / |v|, the fused v s / |v|^2 subtraction, the final product
    Every term enters once, so to first order the relative error is at most this count times 2^-24."""
    lane = -(-row_len // 64)
    return (lane + 6 + 2) + (1 + lane + 6) + 1 + 4


def _through(sd, prefix, dw, db, out):
    out[prefix + ".weight_g"], out[prefix + ".weight_v"] = wn_backward(sd[prefix + ".weight_g"], sd[prefix + ".weight_v"], dw)
    out[prefix + ".bias"] = db


def single_param_grads(sd, nb, g):
    """frame_net_train_ref.backward(..)["grads"] -> {state_dict key: float64 gradient} of Result_Model, through wn_backward"""
    out = {}
    for prefix, (dw, db) in FT.module_grads(g, nb).items():
        if prefix == "shuf.0":
            out["shuf.0.weight"], out["shuf.0.bias"] = dw, db
        else:
            _through(sd, prefix, dw, db, out)
    return out


def multi_param_grads(sd, nb, g):
    """multi_frame_train_ref.backward(..)["grads"] -> {state_dict key: float64 gradient} of Naive_model, through wn_backward"""
    out = {}
    for i, bk in enumerate(g["blocks"]):
        out[f"body.{i}.body.0.weight"], out[f"body.{i}.body.0.bias"], out[f"body.{i}.body.2.weight"], out[f"body.{i}.body.2.bias"] = bk
    _through(sd, "encode", g["enc_w"], g["enc_b"], out)
    _through(sd, "decode", g["dec_w"], g["dec_b"], out)
    return out


def row_len_of(key, sd):
    """elements per output row of the weight-normed conv that state_dict key `key` (a weight_g or weight_v) belongs to, else None"""
    if not key.endswith((".weight_g", ".weight_v")):
        return None
    return sd[key.rsplit(".", 1)[0] + ".weight_v"][0].numel()
