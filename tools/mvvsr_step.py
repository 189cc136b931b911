#!/usr/bin/env python
"""Training-step and evaluation timing of MotionVectorVSR with the HIP reconstruction (csrc/mv_recon.h) against the ATen
reconstruction (`MotionVectorVSR.aten_reconstruction = True`: the loop the model ran before, statement for statement), in ONE
process on one device.

    python tools/mvvsr_step.py [--steps 50] [--warmup 10] [--out profiles/mvvsr_step.json]
    python tools/mvvsr_step.py --wide [--out profiles/mvvsr_step_wide.json]     (the wide leg alone)

Train: MotionVectorVSR(20, 8), 8 clips x 5 frames x 64x64 -> 256x256 (the trainer's C4 shape), forward + Charbonnier + backward +
torch.optim.Adam, as the reference trainer's loop body does (the ATen loss and optimiser are the same on both routes, so they
cancel in the comparison), bf16 and fp32.  Eval: 1 x 15 x 180 x 320, F = 64, bf16,
under no_grad.  Every figure: median / min / max over --steps steps after --warmup, each step timed with HIP events.  Also: the
C-ABI calls of one step by name, the event time of each sr_mv_recon_* call, and the ATen reconstruction alone (forward + backward
on detached features), which is the share of the old step this work replaces.

The parent commit: with the switch set, `forward` runs the statements the parent ran (`propagate` with feature copies, then the
ATen loop) on the same trunk kernels, which this work does not touch, so that route IS the parent's step; `parent_stand_in` in
the JSON says so.  The per-call times are HIP-event times around the two C calls (`_lib.KernelTimer`), not a kernel trace.

Wide leg (`train_wide`): MotionVectorVSR() (64 features, 15 blocks) and MotionVectorVSR(64, 8) at the same clip shape, one step =
forward + Charbonnier + backward + torch.optim.Adam, `model.hot_training = True` (HIP trunks + HIP reconstruction, sr_mv_recon_bwd64)
against `set_wide_training(model)` alone (HIP trunks + ATen reconstruction: the fastest route without sr_mv_recon_bwd64), bf16 and
fp32.  The two routes share one model and alternate in one process after a warm-up: 7 runs per route, each the mean of --wide-steps
steps between two HIP events; reported as median [min - max] with the peak memory of each route."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilesuperresolution_amd import _lib as L                                    # noqa: E402
from mobilesuperresolution_amd.models import MotionVectorVSR, set_wide_training   # noqa: E402


def charbonnier(a, b, eps=1e-6):
    return torch.sqrt((a - b) ** 2 + eps).mean()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), steps=steps)


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


def kernel_times(fn, reps=20):
    t = L.KernelTimer()
    L.set_timer(t)
    try:
        for _ in range(reps):
            fn()
        s = t.summary()
    finally:
        L.set_timer(None)
    return {k: dict(calls=v[0] // reps, mean_ms=v[1]) for k, v in s.items() if k.startswith("sr_mv_recon")}


def aten_recon_alone(m, x, steps, warmup):
    """the old reconstruction by itself: forward + backward of the ATen loop on detached trunk features"""
    b, n, _, h, w = x.shape
    g = torch.Generator().manual_seed(3)
    fb = [torch.randn(b, m.num_feat, h, w, generator=g).cuda().requires_grad_(True) for _ in range(n)]
    ff = [torch.randn(b, m.num_feat, h, w, generator=g).cuda().requires_grad_(True) for _ in range(n)]
    tgt = torch.rand(b, n, 3, 4 * h, 4 * w, generator=g).cuda()

    def run():
        out_l = []
        for i in range(n):
            out = torch.cat([fb[i], ff[i]], dim=1)
            out = m.lrelu(m.fusion(out))
            out = m.conv_last(out)
            out = F.interpolate(out, size=(4 * h, 4 * w), mode='bilinear')
            out_l.append(out + F.interpolate(x[:, i, :3], size=(4 * h, 4 * w), mode='bilinear', align_corners=False))
        charbonnier(torch.stack(out_l, dim=1), tgt).backward()
    return timed(run, steps, warmup)


def train_case(dtype, steps, warmup):
    torch.manual_seed(0)
    m = MotionVectorVSR(num_feat=20, num_block=8, hot_dtype=dtype).cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(8, 5, 5, 64, 64, generator=g)
    x[:, :, 3:] = x[:, :, 3:] * 6 - 3
    x, hr = x.cuda(), torch.rand(8, 5, 3, 256, 256, generator=g).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        charbonnier(m(x, 256, 256), hr).backward()
        opt.step()
    res = {}
    for route, aten in (("hot", False), ("aten_reconstruction", True)):
        m.aten_reconstruction = aten
        res[route] = timed(step, steps, warmup)
        res[route]["c_abi_calls_per_step"] = calls_of(step)
    m.aten_reconstruction = False
    res["hot"]["kernel_event_ms"] = kernel_times(step)
    res["aten_reconstruction_alone_fwd_bwd"] = aten_recon_alone(m, x, steps, warmup)
    return res


def wide_case(num_block, dtype, steps, warmup, runs=7):
    torch.manual_seed(0)
    m = MotionVectorVSR(num_feat=64, num_block=num_block, hot_dtype=dtype).cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(8, 5, 5, 64, 64, generator=g)
    x[:, :, 3:] = x[:, :, 3:] * 6 - 3
    x, hr = x.cuda(), torch.rand(8, 5, 3, 256, 256, generator=g).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        charbonnier(m(x, 256, 256), hr).backward()
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
        res[k].update(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), steps_per_run=steps)
    route(True)
    res["hot_training"]["kernel_event_ms"] = kernel_times(step, reps=5)
    a, b = res["hot_training"], res["set_wide_training_only"]
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    diff = b["median_ms"] - a["median_ms"]
    res["difference_ms"] = diff if abs(diff) > spread else None      # stated only beyond either route's max - min
    res["spread_ms"] = spread
    return res


def eval_case(steps, warmup):
    torch.manual_seed(0)
    m = MotionVectorVSR(num_feat=64, num_block=15, hot_dtype="bf16").cuda().eval()
    g = torch.Generator().manual_seed(2)
    x = torch.rand(1, 15, 5, 180, 320, generator=g)
    x[:, :, 3:] = x[:, :, 3:] * 6 - 3
    x = x.cuda()

    def run():
        with torch.no_grad():
            m(x, 720, 1280)
    res = {}
    for route, aten in (("hot", False), ("aten_reconstruction", True)):
        m.aten_reconstruction = aten
        res[route] = timed(run, steps, warmup)
        res[route]["c_abi_calls_per_step"] = calls_of(run)
    m.aten_reconstruction = False
    res["hot"]["kernel_event_ms"] = kernel_times(run, reps=5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--wide", action="store_true", help="the wide leg (F = 64) alone")
    ap.add_argument("--wide-steps", type=int, default=5)
    a = ap.parse_args()
    wide = {f"f64_b{nb}": {dt: wide_case(nb, dt, a.wide_steps, 3) for dt in ("bf16", "fp32")} for nb in (15, 8)}
    if a.wide:
        res = dict(device=torch.cuda.get_device_name(0), train_wide_8x5x64x64=wide)
    else:
        res = dict(device=torch.cuda.get_device_name(0),
                   parent_stand_in="aten_reconstruction: the parent's forward, statement for statement, on the same trunk kernels",
                   train_c4={dt: train_case(dt, a.steps, a.warmup) for dt in ("bf16", "fp32")},
                   eval_1x15x180x320_f64_bf16=eval_case(max(a.steps // 5, 10), 3),
                   train_wide_8x5x64x64=wide)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
