#!/usr/bin/env python3
"""Time one training step of the per-frame video network (`single`: Result_Model(4, 32, 8, 3)) on the trainer's shape:

    python tools/frame_net_step.py [--clips 8] [--frames 5] [--size 64] [--steps 7] [--warmup 2] [--out profiles/frame_net_step.json]

A step is forward + training.L1_Charbonnier_loss + backward + torch.optim.Adam on 8 clips x 5 frames x 64 x 64 -> 256 x 256.  Four
routes alternate in ONE process, round by round (so drift of the clocks hits all of them alike): the HIP training route
(hot_training) in bf16 and in fp32, and the ATen route (hot_training = False, the route every graph-recording call took before the
training route existed) under bf16 autocast and in fp32.  Each route gets `warmup` untimed rounds, then `steps` timed steps, device
events around each step.  A last pass times the HIP route's C calls one by one (KernelTimer) and its backward per stage.  Writes
the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "frame_net_step.json"))
    args = ap.parse_args()
    from mobilesuperresolution_amd import hotpath as HP, packing as P, training
    from mobilesuperresolution_amd.models import SingleFrameVSR
    b, n, s = args.clips, args.frames, args.size
    g = torch.Generator().manual_seed(0)
    x = torch.rand(b, n, 3, s, s, generator=g).cuda()
    hr = torch.rand(b, n, 3, 4 * s, 4 * s, generator=g).cuda()
    crit = training.L1_Charbonnier_loss()

    def route(dt, hot, autocast):
        torch.manual_seed(1)
        m = SingleFrameVSR(4, 32, 8, 3, hot_dtype=dt).cuda()
        m.hot_training = hot
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)

        def step():
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                sr = m(x, 4 * s, 4 * s)
            loss = crit(sr.float(), hr)
            loss.backward()
            opt.step()
            return m.last_route
        return step

    routes = {"hip_bf16": route("bf16", True, False), "hip_fp32": route("fp32", True, False),
              "aten_bf16_autocast": route("fp32", False, True), "aten_fp32": route("fp32", False, False)}
    times = {k: [] for k in routes}
    taken = {}
    for r in range(args.warmup + args.steps):
        for k, step in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            taken[k] = step()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
    out = {"tool": "frame_net_step", "device": torch.cuda.get_device_name(0), "clips": b, "frames": n, "lr_size": s, "steps": args.steps,
           "warmup": args.warmup, "routes": {}}
    for k, t in times.items():
        t = sorted(t)
        out["routes"][k] = {"route": taken[k], "ms": t, "median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "spread_ms": t[-1] - t[0]}
    for dt in ("bf16", "fp32"):
        hip, aten = out["routes"][f"hip_{dt}"], out["routes"]["aten_bf16_autocast" if dt == "bf16" else "aten_fp32"]
        out[f"speedup_{dt}"] = aten["median_ms"] / hip["median_ms"]
        out[f"margin_ms_{dt}"] = aten["median_ms"] - hip["median_ms"]
        out[f"margin_exceeds_spread_{dt}"] = out[f"margin_ms_{dt}"] > max(hip["spread_ms"], aten["spread_ms"])

    # where the HIP step's time goes: the two C calls, then the backward one stage at a time on the saved images
    for dt in ("bf16", "fp32"):
        torch.manual_seed(1)
        m = SingleFrameVSR(4, 32, 8, 3, hot_dtype=dt).cuda()
        m.hot_training = True
        timer = HP.KernelTimer()
        HP.set_timer(timer)
        for _ in range(5):
            m.zero_grad()
            sr = m(x, 4 * s, 4 * s)
            sr.backward(torch.ones_like(sr))
        HP.set_timer(None)
        calls = {k: v[1] for k, v in timer.summary().items()}
        ctx = m(x, 4 * s, 4 * s).grad_fn
        frames, bwd, acts, ts, masks = ctx.saved
        wgs = HP.fn_bwd_wgs(b * n, s, s)
        gs = torch.zeros((4, b * n, s, s, 32), dtype=bwd.dtype, device="cuda")
        parts = torch.zeros(P.fn_bwd_parts(8, wgs), dtype=torch.float32, device="cuda")
        grads = torch.zeros(sum(P.fn_grad_sizes(32, 8)), dtype=torch.float32, device="cuda")
        gout = torch.ones(b * n, 3, 4 * s, 4 * s, device="cuda")
        stages = {}
        for name, bit in (("upsampler", P.FN_BWD_UP), ("last_conv", P.FN_BWD_LAST), ("blocks", P.FN_BWD_BLOCKS), ("encoder", P.FN_BWD_ENCODER)):
            ts_ = []
            for _ in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                HP.fn_net_bwd(frames, gout, gout.stride(0), bwd, acts, ts, masks, gs, parts, wgs, grads, 32, 8, bit)
                e1.record()
                torch.cuda.synchronize()
                ts_.append(e0.elapsed_time(e1))
            stages[name] = sorted(ts_[1:])[2]
        out[f"hip_{dt}_calls_ms"] = calls
        out[f"hip_{dt}_bwd_stage_ms"] = stages                   # each includes the one reduce launch
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
