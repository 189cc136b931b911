#!/usr/bin/env python3
"""Time `metrics.ssim` (csrc/ssim.h) against the route the reference's evaluation loop takes today, in one process:

    python tools/ssim_eval.py [--reps 7] [--iters 50] [--host-reps 3] [--out profiles/ssim_eval.json]

Shapes: 1x3x720x1280 (a REDS HR frame) and 1x3x512x512.  Device leg: `--iters` calls of `metrics.ssim` between two device
events, per call; median (min, max) of `--reps` such windows after a warm-up.  Host leg: `sr.cpu()` (and `hr.cpu()`)
followed by the float64 computation skimage's `structural_similarity` does, here tests/ssim_ref.py with
`scipy.ndimage.gaussian_filter` as the filter where scipy imports (what skimage itself calls), else its numpy "valid"
filter; host clock around copy + computation, median (min, max) of `--host-reps`.  skimage itself is not a dependency
of this project and is not run.  Prints one JSON line and writes it to --out.  Needs a GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(ts, nd):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd)}


def _device_us(fn, reps, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / iters)
    return _stats(ts, 2)


def _host_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return _stats(ts, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--shave", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_eval needs a GPU: a CPU run measures nothing")
    from mobilesuperresolution_amd.metrics import ssim
    from tests import ssim_ref as SR
    try:
        from scipy import ndimage
        r = SR.RADIUS
        filt, host_filter = (lambda x: ndimage.gaussian_filter(x, sigma=SR.SIGMA, truncate=3.5, mode="reflect")[r:-r, r:-r]), \
            "scipy.ndimage.gaussian_filter"
    except ImportError:
        filt, host_filter = None, "numpy valid filter (scipy not importable)"
    res = {"device": torch.cuda.get_device_name(0), "shave": a.shave, "host_filter": host_filter,
           "unit": {"device_us": "us per call, median (min, max) of %d windows of %d calls" % (a.reps, a.iters),
                    "host_ms": "ms for sr.cpu() + hr.cpu() + the float64 computation, median (min, max) of %d" % a.host_reps},
           "note": "measured on one box in one run; the host leg restates skimage's structural_similarity, skimage itself is not run",
           "shapes": {}}
    for shape in ((1, 3, 720, 1280), (1, 3, 512, 512)):
        g = torch.Generator().manual_seed(shape[-1])
        hr = torch.rand(shape, generator=g)
        sr = (hr + 0.05 * torch.randn(shape, generator=g)).cuda()
        hr = hr.cuda()
        dev = _device_us(lambda: ssim(sr, hr, shave=a.shave), a.reps, a.iters)
        host = _host_ms(lambda: SR.ssim_ref(sr.cpu().numpy(), hr.cpu().numpy(), a.shave, filt), a.host_reps)
        copy = _host_ms(lambda: (sr.cpu(), hr.cpu()), a.host_reps)
        got, exp = float(ssim(sr, hr, shave=a.shave)), SR.ssim_ref(sr.cpu().numpy(), hr.cpu().numpy(), a.shave, filt)
        px = (shape[2] - 2 * a.shave - 2 * SR.RADIUS) * (shape[3] - 2 * a.shave - 2 * SR.RADIUS)
        res["shapes"]["x".join(map(str, shape))] = {
            "device_us": dev, "host_ms": host, "of_which_copy_ms": copy,
            "host_over_device": round(host["median"] * 1e3 / dev["median"], 1),
            "device_Mpixel_per_s": round(px / dev["median"], 1),
            "device_GB_s_algorithmic": round(2 * 3 * shape[2] * shape[3] * 4 / dev["median"] / 1e3, 1),
            "value_device": got, "value_host": exp, "abs_diff": abs(got - exp)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
