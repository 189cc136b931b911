#!/usr/bin/env python3
"""Time one training step of the multi-frame video network (`multi`: Naive_model(4, 8 blocks of [32, 32, 3])) on the trainer's shape:

    python tools/multi_frame_step.py [--clips 8] [--frames 5] [--size 64] [--steps 7] [--warmup 2] [--out profiles/multi_frame_step.json]

A step is forward + training.L1_Charbonnier_loss + backward + torch.optim.Adam on 8 clips x 5 frames x 64 x 64 -> 256 x 256, once
with GIVEN flows (uniform in +-3 px; get_flow replaced) and once with SPyNet computing them (the same frozen, randomly initialised
SpyNet on every route).  Four routes alternate in ONE process, round by round (so drift of the clocks hits all of them alike): the HIP
training route (hot_training) in bf16 and in fp32, and the ATen route (hot_training = False, the route every graph-recording call
took before the training route existed) under bf16 autocast and in fp32.  Each route gets `warmup` untimed rounds, then `steps` timed
steps, device events around each step.  A last pass times the HIP route's C calls one by one (KernelTimer), its backward per stage,
and the warp backward at flow amplitudes of 0, about 3 and about 12 px (its window, and so its cost, follows the largest flow).
Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps=6):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts[1:])[(reps - 1) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "multi_frame_step.json"))
    args = ap.parse_args()
    from mobilesuperresolution_amd import hotpath as HP, packing as P, training
    from mobilesuperresolution_amd.models import MultiFrameVSR
    b, n, s, nb = args.clips, args.frames, args.size, args.blocks
    g = torch.Generator().manual_seed(0)
    x = torch.rand(b, n, 3, s, s, generator=g).cuda()
    hr = torch.rand(b, n, 3, 4 * s, 4 * s, generator=g).cuda()
    given = (6 * torch.rand(b, n - 1, 2, s, s, generator=g) - 3).cuda()
    crit = training.L1_Charbonnier_loss()

    def model(dt, hot, flows):
        torch.manual_seed(1)
        m = MultiFrameVSR(4, status=[[32, 32, 3]] * nb, hot_dtype=dt).cuda()
        m.hot_training = hot
        if flows is not None:
            m.get_flow = lambda x_: flows
        return m

    def route(dt, hot, autocast, flows):
        m = model(dt, hot, flows)
        opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4)

        def step():
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                sr = m(x, 4 * s, 4 * s)
            loss = crit(sr.float(), hr)
            loss.backward()
            opt.step()
            return m.last_route
        return step

    out = {"tool": "multi_frame_step", "device": torch.cuda.get_device_name(0), "clips": b, "frames": n, "lr_size": s, "blocks": nb,
           "steps": args.steps, "warmup": args.warmup}
    for flow_name, flows in (("given_flows", given), ("spynet", None)):
        routes = {"hip_bf16": route("bf16", True, False, flows), "hip_fp32": route("fp32", True, False, flows),
                  "aten_bf16_autocast": route("fp32", False, True, flows), "aten_fp32": route("fp32", False, False, flows)}
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
        res = {"routes": {}}
        for k, t in times.items():
            t = sorted(t)
            res["routes"][k] = {"route": taken[k], "ms": t, "median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "spread_ms": t[-1] - t[0]}
        for dt in ("bf16", "fp32"):
            hip, aten = res["routes"][f"hip_{dt}"], res["routes"]["aten_bf16_autocast" if dt == "bf16" else "aten_fp32"]
            res[f"speedup_{dt}"] = aten["median_ms"] / hip["median_ms"]
            res[f"margin_ms_{dt}"] = aten["median_ms"] - hip["median_ms"]
            res[f"margin_exceeds_spread_{dt}"] = res[f"margin_ms_{dt}"] > max(hip["spread_ms"], aten["spread_ms"])
        out[flow_name] = res
        del routes
        torch.cuda.empty_cache()

    # where the HIP step's time goes: the two C calls, then the backward one stage at a time on the saved images
    for dt in ("bf16", "fp32"):
        m = model(dt, True, given)
        timer = HP.KernelTimer()
        HP.set_timer(timer)
        for _ in range(5):
            m.zero_grad()
            sr = m(x, 4 * s, 4 * s)
            sr.backward(torch.ones_like(sr))
        HP.set_timer(None)
        out[f"hip_{dt}_calls_ms"] = {k: v[1] for k, v in timer.summary().items()}
        ctx = m(x, 4 * s, 4 * s).grad_fn
        frames, flows, bound, bwd, acts, ts, masks, wf = ctx.saved
        wgs = HP.fn_bwd_wgs(b * n, s, s)
        gs = torch.zeros((6, b * n, s, s, 32), dtype=bwd.dtype, device="cuda")
        parts = torch.zeros(P.mf_bwd_parts(nb, wgs), dtype=torch.float32, device="cuda")
        grads = torch.zeros(sum(P.mf_grad_sizes(32, nb)), dtype=torch.float32, device="cuda")
        gout = torch.ones(b * n, 3, 4 * s, 4 * s, device="cuda")
        run = lambda bit, fl=flows, bd=bound: HP.mf_net_bwd(frames, fl, bd, gout, bwd, acts, ts, masks, wf, gs, parts, wgs, grads, 32, nb, b, n, bit)
        stages = {}
        for name, bit in (("tail", P.MF_BWD_TAIL), ("blocks", P.MF_BWD_BLOCKS), ("first", P.MF_BWD_FIRST), ("warp", P.MF_BWD_WARP),
                          ("encoder", P.MF_BWD_ENCODER)):
            stages[name] = _timed(lambda: run(bit))
        out[f"hip_{dt}_bwd_stage_ms"] = stages                   # each includes the one reduce launch
        warp = {}
        for amp in (0.0, 3.0, 12.0):
            fl = ((2 * torch.rand(b, n - 1, 2, s, s, generator=g) - 1) * amp).cuda()
            bd = fl.abs().amax().reshape(1)
            warp[f"amplitude_{amp:g}px"] = _timed(lambda: run(P.MF_BWD_WARP, fl, bd))
        out[f"hip_{dt}_warp_bwd_ms"] = warp
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
