#!/usr/bin/env python3
"""Time `evaluation.clip_metrics` and the two 8-bit packs (csrc/eval.h) against the other ways to get the same numbers for
one clip, in one process:

    python tools/eval_clip_eval.py [--calls 50] [--warmup 10] [--runs 2] [--out profiles/eval_clip.json]

Shape: lr 1x15x3x180x320 -> sr, hr 1x15x3x720x1280 (a REDS clip), shave 4, align_corners=False.  Routes:
  clip_metrics     one call: (4, 15) psnr, psnr_y, psnr of the bilinear baseline, Charbonnier mean per frame
  composed_device  the same four rows from the pieces that existed before: per frame ATen `F.interpolate`, `metrics.psnr`
                   twice, `metrics.psnr_y`, and the Charbonnier expression in torch, stacked to (4, 15) on device
  host             `sr.cpu()` + `lr.cpu()` and the reference's formulas in torch on the CPU (hr is on the host there already)
  u8_sr / u8_sr_torch          `to_uint8_hwc(sr)` against clamp.mul.add.clamp.to(uint8).permute.contiguous on device
  u8_base / u8_base_torch      `bilinear_baseline_u8(lr, size)` against `F.interpolate` + the same expression on device
Every call is timed on its own with a host clock around the call and a device synchronise; the routes ALTERNATE inside a
run (call i of every route before call i + 1 of any); a run is --warmup untimed and --calls timed calls per route; the
run is repeated --runs times and the spread of a route is the largest difference between its runs' medians.  The claim
checked: clip_metrics is faster than composed_device by more than the larger of the two routes' spreads.  Prints one JSON
line and writes it to --out.  Needs a GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _pct(ts, q):
    s = sorted(ts)
    return s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]


def _summ(ts):
    return {"median_us": round(statistics.median(ts), 1), "p10_us": round(_pct(ts, 0.1), 1), "p90_us": round(_pct(ts, 0.9), 1)}


def _host_psnr(sr, hr, shave):
    sr = sr.mul(255).round().clamp(0, 255).div(255).clamp(0, 1)
    d = (sr - hr)[..., shave:-shave, shave:-shave]
    return -10 * torch.log10(d.pow(2).mean(dim=(-3, -2, -1)))


def _host_psnr_y(sr, hr, shave):
    d = sr.clamp(0, 1) - hr
    d = (0.257 * d[:, 0] + 0.504 * d[:, 1] + 0.098 * d[:, 2])[..., shave:-shave, shave:-shave]
    return -10 * torch.log10(d.pow(2).mean(dim=(-2, -1)))


def _charbonnier(sr, hr):
    d = torch.add(sr, -hr)
    return torch.sqrt(d * d + 1e-12).mean(dim=(-3, -2, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--lr", type=int, nargs=2, default=(180, 320))
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--shave", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_clip_eval needs a GPU: a CPU run measures nothing")
    from mobilesuperresolution_amd import metrics
    from mobilesuperresolution_amd.evaluation import bilinear_baseline_u8, clip_metrics, to_uint8_hwc
    n, (h, w), shave = a.frames, a.lr, a.shave
    H, W = h * a.scale, w * a.scale
    g = torch.Generator().manual_seed(720)
    lr_h = torch.rand(1, n, 3, h, w, generator=g)
    hr_h = torch.rand(1, n, 3, H, W, generator=g)
    sr = (hr_h + 0.05 * torch.randn(hr_h.shape, generator=g)).cuda()
    lr, hr = lr_h.cuda(), hr_h.cuda()

    def composed():
        rows = []
        for i in range(n):
            s, l, t = sr[:, i], lr[:, i], hr[:, i]
            base = F.interpolate(l, (H, W), mode="bilinear")
            rows.append(torch.stack([metrics.psnr(s, t, shave=shave), metrics.psnr_y(s, t, shave=shave),
                                     metrics.psnr(base, t, shave=shave), _charbonnier(s, t)[0]]))
        return torch.stack(rows, dim=1)

    def host():
        s, l, t = sr.cpu()[0], lr.cpu()[0], hr_h[0]
        base = F.interpolate(l, (H, W), mode="bilinear")
        return torch.stack([_host_psnr(s, t, shave), _host_psnr_y(s, t, shave), _host_psnr(base, t, shave), _charbonnier(s, t)])

    def u8_torch(x):
        return x.clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    routes = {
        "clip_metrics": lambda: clip_metrics(sr, lr, hr, shave=shave),
        "composed_device": composed,
        "host": host,
        "u8_sr": lambda: to_uint8_hwc(sr),
        "u8_sr_torch": lambda: u8_torch(sr[0]),
        "u8_base": lambda: bilinear_baseline_u8(lr, (H, W)),
        "u8_base_torch": lambda: u8_torch(F.interpolate(lr[0], (H, W), mode="bilinear")),
    }
    runs = []
    for _ in range(a.runs):
        ts = {k: [] for k in routes}
        for i in range(a.warmup + a.calls):
            for k, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ts[k].append((time.perf_counter() - t0) * 1e6)
        runs.append({k: _summ(v) for k, v in ts.items()})
    med = {k: [r[k]["median_us"] for r in runs] for k in routes}
    spread = {k: round(max(v) - min(v), 1) for k, v in med.items()}
    one, comp = clip_metrics(sr, lr, hr, shave=shave).cpu().double(), composed().cpu().double()
    hst = host().double()
    gain = min(med["composed_device"]) - max(med["clip_metrics"])
    noise = max(spread["clip_metrics"], spread["composed_device"])
    res = {
        "device": torch.cuda.get_device_name(0), "shape": {"lr": list(lr.shape), "hr": list(hr.shape), "shave": shave},
        "unit": "us per call: host clock around the call and a device synchronise; median, p10, p90 of %d calls after %d "
                "warm-up, routes alternating; %d runs in one process" % (a.calls, a.warmup, a.runs),
        "note": "measured on one box in one run of this tool",
        "runs": runs, "median_us_per_run": med, "spread_between_runs_us": spread,
        "claim": {"statement": "clip_metrics is faster than composed_device by more than the spread between runs of the same route",
                  "composed_minus_clip_us_worst_pairing": round(gain, 1), "spread_us": noise, "holds": bool(gain > noise)},
        "ratios_of_mean_medians": {
            "composed_device_over_clip_metrics": round(statistics.mean(med["composed_device"]) / statistics.mean(med["clip_metrics"]), 2),
            "host_over_clip_metrics": round(statistics.mean(med["host"]) / statistics.mean(med["clip_metrics"]), 1),
            "u8_sr_torch_over_u8_sr": round(statistics.mean(med["u8_sr_torch"]) / statistics.mean(med["u8_sr"]), 2),
            "u8_base_torch_over_u8_base": round(statistics.mean(med["u8_base_torch"]) / statistics.mean(med["u8_base"]), 2)},
        "clip_metrics_GB_s_algorithmic": round((2 * sr.numel() + lr.numel()) * 4 / statistics.mean(med["clip_metrics"]) / 1e3, 1),
        "agreement": {"max_abs_rows012_dB_vs_composed": float((one[:3] - comp[:3]).abs().max()),
                      "max_rel_row3_vs_composed": float((one[3] / comp[3] - 1).abs().max()),
                      "max_abs_rows012_dB_vs_host": float((one[:3] - hst[:3]).abs().max()),
                      "u8_sr_equal": bool(torch.equal(to_uint8_hwc(sr), u8_torch(sr[0]))),
                      "u8_base_bytes_differing_from_torch_device": int(
                          (bilinear_baseline_u8(lr, (H, W)) != u8_torch(F.interpolate(lr[0], (H, W), mode="bilinear"))).sum())},
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
