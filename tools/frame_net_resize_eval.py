#!/usr/bin/env python3
"""Time the per-frame video network (`single`: Result_Model(4, 32, 8, 3)) at the NEMO shape, where the output is NOT (4H, 4W): 240 x 426
frames resized to 1080 x 1920 (D is 961 x 1705), with and without `hot_resize`:

    python tools/frame_net_resize_eval.py [--runs 7] [--warmup 2] [--out profiles/frame_net_resize.json]

  inference  1 x 15 x 3 x 240 x 426 under no_grad, bf16 and fp32: `hot_resize` (the resize inside the upsampler kernel) against the flag
             off (the kernel writes D, one F.interpolate finishes)
  training   a step = forward + training.L1_Charbonnier_loss + backward + training.Adam on 8 x 2 x 3 x 240 x 426 (nemo_single.bash's
             batch), bf16 and fp32: hot_training + hot_resize against the ATen route (bf16: under autocast), with each route's peak
             allocated memory during a step

The routes of a row alternate in ONE process, round by round (so drift of the clocks hits them alike); `warmup` untimed rounds, then
`runs` timed ones, device events around each call.  Per route: the median, min, max and max - min.  A gain counts only when the
medians differ by more than the larger of the two spreads (`margin_exceeds_spread`).  One box, one run.  Writes the JSON to --out and
prints it as one line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, W, OH, OW = 240, 426, 1080, 1920


def alternate(routes, runs, warmup, peak=False):
    times, taken, mem = {k: [] for k in routes}, {}, {k: 0 for k in routes}
    for r in range(warmup + runs):
        for k, call in routes.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            taken[k] = call()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[k].append(e0.elapsed_time(e1))
                mem[k] = max(mem[k], torch.cuda.max_memory_allocated())
    out = {}
    for k, t in times.items():
        t = sorted(t)
        out[k] = {"route": taken[k], "ms": t, "median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "spread_ms": t[-1] - t[0]}
        if peak:
            out[k]["peak_allocated_mib"] = mem[k] / 2 ** 20
    return out


def compare(rows, new, old):
    a, b = rows[new], rows[old]
    margin = b["median_ms"] - a["median_ms"]
    return {"new": new, "old": old, "speedup": b["median_ms"] / a["median_ms"], "margin_ms": margin,
            "margin_exceeds_spread": margin > max(a["spread_ms"], b["spread_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "frame_net_resize.json"))
    args = ap.parse_args()
    from mobilesuperresolution_amd import training
    from mobilesuperresolution_amd.models import SingleFrameVSR
    g = torch.Generator().manual_seed(0)
    out = {"tool": "frame_net_resize_eval", "device": torch.cuda.get_device_name(0), "lr_size": [H, W], "out_size": [OH, OW],
           "runs": args.runs, "warmup": args.warmup, "note": "one box, one run; the routes of a row alternate in one process"}

    # ---- inference ----
    x = torch.rand(1, 15, 3, H, W, generator=g).cuda()

    def infer(dt, resize):
        torch.manual_seed(1)
        m = SingleFrameVSR(4, 32, 8, 3, hot_dtype=dt).cuda().eval()
        m.hot_resize = resize

        def call():
            with torch.no_grad():
                m(x, OH, OW)
            return m.last_route
        return call

    routes = {f"{'fused' if rz else 'd_plus_interpolate'}_{dt}": infer(dt, rz) for dt in ("bf16", "fp32") for rz in (True, False)}
    rows = alternate(routes, args.runs, args.warmup)
    out["inference"] = {"clip": [1, 15, 3, H, W], "routes": rows,
                        "bf16": compare(rows, "fused_bf16", "d_plus_interpolate_bf16"), "fp32": compare(rows, "fused_fp32", "d_plus_interpolate_fp32")}
    del routes, x
    torch.cuda.empty_cache()

    # ---- training ----
    x = torch.rand(8, 2, 3, H, W, generator=g).cuda()
    hr = torch.rand(8, 2, 3, OH, OW, generator=g).cuda()
    crit = training.L1_Charbonnier_loss()

    def train(dt, hot, autocast):
        torch.manual_seed(1)
        m = SingleFrameVSR(4, 32, 8, 3, hot_dtype=dt).cuda()
        m.hot_training = m.hot_resize = hot
        opt = training.Adam(m.parameters(), lr=1e-4)

        def step():
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                sr = m(x, OH, OW)
            loss = crit(sr.float(), hr)
            loss.backward()
            opt.step()
            return m.last_route
        return step

    routes = {"hip_bf16": train("bf16", True, False), "hip_fp32": train("fp32", True, False),
              "aten_bf16_autocast": train("fp32", False, True), "aten_fp32": train("fp32", False, False)}
    rows = alternate(routes, args.runs, args.warmup, peak=True)
    out["training"] = {"clip": [8, 2, 3, H, W], "routes": rows, "bf16": compare(rows, "hip_bf16", "aten_bf16_autocast"),
                       "fp32": compare(rows, "hip_fp32", "aten_fp32")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
