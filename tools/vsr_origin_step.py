#!/usr/bin/env python
"""Training-step timing of BasicVSR_origin at 64 features: `model.hot_training = True` (HIP trunks + the HIP reconstruction forward
and backward, csrc/vsr_recon_bwd.h) against `set_wide_training(model)` alone (HIP trunks + the ATen reconstruction), in ONE process
on one device.

    python tools/vsr_origin_step.py [--steps 3] [--out profiles/vsr_origin_step.json]

Workload: 8 clips x 5 frames x 64x64 -> 256x256, given flows, forward + Charbonnier + backward + torch.optim.Adam;
BasicVSR_origin(64, 30) and (64, 8), bf16 and fp32.  The two routes share one model and alternate after a warm-up: 7 runs per route,
each the mean of --steps steps between two HIP events; reported as median [min - max], the difference next to each route's
max - min, the peak allocated memory of each route, the HIP-event times of the sr_c64_recon_* calls and the kernel-time shares of
one hot step (torch.profiler kernel trace)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilesuperresolution_amd import _lib as L                                    # noqa: E402
from mobilesuperresolution_amd.models import BasicVSR_origin, set_wide_training   # noqa: E402


def charbonnier(a, b, eps=1e-6):
    return torch.sqrt((a - b) ** 2 + eps).mean()


def calls_of(fn):
    names, real = [], L.launch

    def counting(name, f, *a):
        names.append(name)
        return real(name, f, *a)
    L.launch = counting
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.launch = real
    return {k: names.count(k) for k in sorted(set(names))}


def kernel_times(fn, reps=3):
    t = L.KernelTimer()
    L.set_timer(t)
    try:
        for _ in range(reps):
            fn()
        s = t.summary()
    finally:
        L.set_timer(None)
    return {k: dict(calls=v[0] // reps, mean_ms=v[1]) for k, v in s.items() if k.startswith("sr_c64_recon")}


_GROUPS = (("reconstruction backward: vr_last_bwd / vr_last_wgrad / vr_upconv_bwd / vr_reduce", ("vr_last_bwd", "vr_last_wgrad", "vr_upconv_bwd", "vr_reduce")),
           ("reconstruction forward: vr_fusion / vr_upconv / vr_last", ("vr_fusion", "vr_upconv_kernel", "vr_last_kernel")),
           ("c64_wgrad_kernel (trunks and reconstruction)", ("c64_wgrad",)),
           ("c64_conv_kernel (trunks and reconstruction, forward and backward-data)", ("c64_conv",)),
           ("slab reduction of the trunks (unpack_all_kernel)", ("unpack_all",)),
           ("warp backward", ("c64_warp_bwd",)))


def kernel_shares(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    tot, acc = 0.0, {k: 0.0 for k, _ in _GROUPS}
    acc["everything else (layout copies, the loss, packing, Adam)"] = 0.0
    for ev in prof.key_averages():
        us = getattr(ev, "device_time_total", None)
        if us is None:
            us = getattr(ev, "cuda_time_total", 0.0)
        if not us:
            continue
        tot += us
        for k, pats in _GROUPS:
            if any(p in ev.key for p in pats):
                acc[k] += us
                break
        else:
            acc["everything else (layout copies, the loss, packing, Adam)"] += us
    return dict(kernel_time_ms=tot / 1e3, shares_percent={k: round(100.0 * v / tot, 1) for k, v in acc.items()} if tot else {})


def case(num_block, dtype, steps, warmup=2, runs=7):
    torch.manual_seed(0)
    m = BasicVSR_origin(num_feat=64, num_block=num_block, hot_dtype=dtype).cuda().train()
    for p in m.spynet.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(8, 5, 3, 64, 64, generator=g).cuda()
    mv = (torch.rand(8, 5, 2, 64, 64, generator=g) * 6 - 3).cuda()
    flows = (mv[:, 1:], -mv[:, 1:])
    hr = torch.rand(8, 5, 3, 256, 256, generator=g).cuda()
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        charbonnier(m(x, 256, 256, flows=flows), hr).backward()
        opt.step()

    def route(hot):
        m.hot_training = hot                             # False opts the trunks out too:
        set_wide_training(m)                             # the trunks stay on the HIP training route on both
    names = (("hot_training", True), ("set_wide_training_only", False))
    res = {k: dict(runs_ms=[]) for k, _ in names}
    for k, hot in names:
        route(hot)
        for _ in range(warmup):
            step()
        res[k]["c_abi_calls_per_step"] = calls_of(step)
    for _ in range(runs):
        for k, hot in names:
            route(hot)
            step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            e1.synchronize()
            res[k]["runs_ms"].append(e0.elapsed_time(e1) / steps)
            res[k]["peak_memory_mib"] = max(res[k].get("peak_memory_mib", 0.0), torch.cuda.max_memory_allocated() / 2 ** 20)
    for k, _ in names:
        ts = res[k]["runs_ms"]
        res[k].update(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), spread_ms=max(ts) - min(ts), steps_per_run=steps)
    route(True)
    res["hot_training"]["kernel_event_ms"] = kernel_times(step)
    try:
        res["hot_training"]["kernel_trace"] = kernel_shares(step)
    except Exception as e:                                # the trace is an extra: the step times above stand without it
        res["hot_training"]["kernel_trace"] = dict(error=repr(e))
    a, b = res["hot_training"], res["set_wide_training_only"]
    res["difference_ms"] = b["median_ms"] - a["median_ms"]
    res["beyond_both_spreads"] = abs(res["difference_ms"]) > max(a["spread_ms"], b["spread_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), workload="8 clips x 5 frames x 64x64 -> 256x256, given flows, forward + Charbonnier + backward + Adam",
               train_8x5x64x64={f"f64_b{nb}": {dt: case(nb, dt, a.steps) for dt in ("bf16", "fp32")} for nb in (30, 8)})
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
