"""Float64 reference of the loss the video trainers' criteria fold into the HIP backward of the per-frame and the multi-frame network
(mobilesuperresolution_amd.training on sr_fn_net_bwd_loss / sr_mf_net_bwd_loss), and the length of the fp32 summation chain the kernels
build for the loss value.  Plain torch on the CPU; tests/test_video_fold_host.py pins it against autograd, tests/test_gpu_video_fold.py
holds the kernels to it."""
import torch

EPS = 1e-12
KINDS = ("l1", "charbonnier")


def loss_value(sr, hr, kind):
    """float64 mean over all elements of |d| (l1) or sqrt(d^2 + 1e-12) (charbonnier), d = sr - hr"""
    d = sr.double() - hr.double()
    return (d.abs() if kind == "l1" else torch.sqrt(d * d + EPS)).mean()


def loss_grad(sr, hr, kind):
    """float64 d(loss_value)/d(sr) in closed form: sign(d) / n resp. d / sqrt(d^2 + 1e-12) / n"""
    d = sr.double() - hr.double()
    return (torch.sign(d) if kind == "l1" else d / torch.sqrt(d * d + EPS)) / d.numel()


def kernel_formula_fp32(sr, hr, kind):
    """the kernels' formula for the same gradient as one fp32 torch expression (its evaluation order is torch's, not the kernels')"""
    d = sr - hr
    gscale = 1.0 / d.numel()
    return torch.sign(d) * gscale if kind == "l1" else d / torch.sqrt(d * d + 1e-12) * gscale


def chain_length(kind, items, workgroups, adds_per_item):
    """roundings on the longest path a loss term takes into the fp32 loss value, as the kernels sum it:
      the term itself                    l1: d = sr - hr (|.| is exact); charbonnier: d, d d, + eps, sqrt
      the thread's running sum           ceil(items / workgroups) tiles x adds_per_item additions
      the workgroup's 256 sums           fn_sum8: 32 additions on one of eight interleaved chains, then a three-level tree
      sr_loss_value                      ceil(workgroups / 64) additions per lane, a six-level shuffle tree, one multiplication by 1 / n
    Every term is >= 0, so the relative error of the sum is at most this count times 2^-24 (first order)."""
    term = 1 if kind == "l1" else 4
    thread = -(-items // workgroups) * adds_per_item
    return term + thread + (32 + 3) + (-(-workgroups // 64) + 6 + 1)
