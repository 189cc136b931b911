#!/usr/bin/env python3
"""Time forward + backward of SpyNet on the opt-in HIP training route (SpyNet.hot_training):

    python tools/spynet_train_step.py [--pairs 64] [--size 64] [--runs 7]

64 frame pairs of 64 x 64 are the C4 clip batch, both directions.  Loss = a fixed cotangent dotted with the flow.  Next to it,
alternating in the same process: a bf16 channels_last ATen restatement of the same step under autograd (the pattern of
tools/vsr64_step.py).  Per route: median and min-max of --runs runs after a warm-up and the peak memory of a step; for the HIP
route also the per-kernel times of the two new kernels (the backward-data instances of conv7_fwd_kernel and conv7_wgrad_kernel),
of the slab reduction and of the forward convolutions, from a torch.profiler trace of one step.  Writes
profiles/spynet_train_step.json and prints it.  Nothing here is a target: the numbers are what came out."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


# conv7_fwd_kernel<CIN, COUT, RELU, OUT_F32, BWD>: the backward-data instances end in BWD = true (mangled and demangled spellings)
BWD_KEYS = ("Lb1EEv", "true>(")


def _kernels(fn):
    """kernel time of one step by group, in ms, with the launch counts"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        by, tot = {}, 0.0
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            if not t:
                continue
            tot += t
            name = ev.key
            if "conv7_wgrad_kernel" in name:
                grp = "conv7_wgrad_kernel"
            elif "conv7_fwd_kernel" in name:
                grp = "conv7_bwd_data" if any(k in name for k in BWD_KEYS) else "conv7_fwd"
            elif "unpack_all" in name:
                grp = "slab_reduction"
            else:
                grp = "torch_glue"
            g = by.setdefault(grp, {"ms": 0.0, "launches": 0})
            g["ms"] += t / 1e3
            g["launches"] += ev.count
        if tot <= 0:
            return {"error": "the trace holds no kernel times"}
        return {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in sorted(by.items())} | {"kernel_ms_total": round(tot / 1e3, 3)}
    except Exception as e:                               # a box without the tracer: say so rather than invent a time
        return {"error": f"not measured: {type(e).__name__}: {e}"[:200]}


def _aten_spynet(p, mean, std, ref, supp):
    """SpyNet.forward with the five convolutions per level in bf16 channels_last ATen, the glue in fp32 as in the package"""
    import math
    from mobilesuperresolution_amd.models.spynet_arch import _border_warp
    refs, supps = [(ref - mean) / std], [(supp - mean) / std]
    for _ in range(5):
        refs.insert(0, F.avg_pool2d(refs[0], 2, 2, count_include_pad=False))
        supps.insert(0, F.avg_pool2d(supps[0], 2, 2, count_include_pad=False))
    flow = refs[0].new_zeros(refs[0].size(0), 2, int(math.floor(refs[0].size(2) / 2.0)), int(math.floor(refs[0].size(3) / 2.0)))
    for lv in range(6):
        up = F.interpolate(flow, scale_factor=2, mode="bilinear", align_corners=True) * 2.0
        x = torch.cat([refs[lv], _border_warp(supps[lv], up), up], 1).bfloat16().contiguous(memory_format=torch.channels_last)
        for i in range(5):
            x = F.conv2d(x, p[f"basic_module.{lv}.basic_module.{2 * i}.weight"], p[f"basic_module.{lv}.basic_module.{2 * i}.bias"], padding=3)
            x = F.relu(x) if i < 4 else x
        flow = x.float() + up
    return flow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spynet_train_step.json"))
    a = ap.parse_args()
    from mobilesuperresolution_amd.models.spynet_arch import SpyNet
    n, h = a.pairs, a.size
    assert h % 32 == 0, "the restatement skips the resize to a multiple of 32"
    g = torch.Generator().manual_seed(1)
    ref, supp = torch.rand(n, 3, h, h, generator=g).cuda(), torch.rand(n, 3, h, h, generator=g).cuda()
    cot = torch.randn(n, 2, h, h, generator=g).cuda()
    torch.manual_seed(0)
    net = SpyNet().cuda()
    net.hot_training = True
    p = {k: (v.detach().bfloat16().contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.detach().bfloat16()).requires_grad_(True)
         for k, v in net.named_parameters()}

    def hip():
        for q in net.parameters():
            q.grad = None
        (net(ref, supp) * cot).sum().backward()

    def aten():
        for q in p.values():
            q.grad = None
        (_aten_spynet(p, net.mean, net.std, ref, supp) * cot).sum().backward()

    def hip_forward_only():
        with torch.no_grad():
            net(ref, supp)

    steps = {"hip_bf16": hip, "aten_bf16": aten, "hip_inference_forward": hip_forward_only}
    for fn in steps.values():                               # warm-up: packing, tables, allocator, kernel load
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(a.runs):                                 # the routes alternate
        for k, fn in steps.items():
            times[k].append(_once(fn))
    res = {"shape": [n, 3, h, h], "runs": a.runs, "device": torch.cuda.get_device_name(0)}
    res |= {k: _stats(v) | {"peak_mib": _peak(steps[k])} for k, v in times.items()}
    res["hip_bf16"]["kernels"] = _kernels(hip)
    res["hip_bf16_speedup_vs_aten_bf16"] = round(res["aten_bf16"]["median_ms"] / res["hip_bf16"]["median_ms"], 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
