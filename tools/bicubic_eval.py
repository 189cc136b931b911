#!/usr/bin/env python3
"""Time the bicubic-on-the-fly input route (csrc/bicubic.h) against the host route and against the pre-made-pairs route, in
one process:

    python tools/bicubic_eval.py [--reps 7] [--iters 50] [--host-reps 3] [--out profiles/bicubic_eval.json]

Training batch: x4, lr_patch_size 48, ignored_boundary_size 1, batch 32, from 8 HR images of 480 x 640 --
`DeviceBicubicPatchCache.batch` (HR only resident, LR made on device), `DevicePatchCache.batch` on the same batch geometry (LR
made beforehand), and the host loop the reference's dataset runs per item (crop, resize, slices, flips, to_tensor layout) with
tests/bicubic_ref.py standing in for the reference's `imresize` (the same arithmetic in numpy; the reference itself is not run).
Frame: `bicubic_downscale` of one 1080 x 1920 frame at x4 against tests/bicubic_ref.py.  Device legs: `--iters` calls between
two device events, per call, median (min, max) of `--reps` windows after a warm-up; `batch()` includes its host side (draws,
record upload).  Host legs: host clock, median (min, max) of `--host-reps`.  Also checks that the device results equal the host
ones bit for bit.  Prints one JSON line and writes it to --out.  Needs a GPU: no fallback."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
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
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return _stats(ts, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bicubic_eval needs a GPU: a CPU run measures nothing")
    from mobilesuperresolution_amd.datasets import DeviceBicubicPatchCache, DevicePatchCache, bicubic_downscale
    from tests import bicubic_ref as BR
    scale, P, ig, B = 4, 48, 1, 32
    g = np.random.default_rng(0)
    hrs = [g.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(8)]
    lrs = [g.integers(0, 256, (120, 160, 3), dtype=np.uint8) for _ in range(8)]          # content does not matter for the timing
    new, old = DeviceBicubicPatchCache(hrs, P, scale, ig), DevicePatchCache(lrs, hrs, P, scale, ig)
    idx = [k % 8 for k in range(B)]
    rng = random.Random(0)

    def host_batch(r=None):
        r = r or rng
        items = [BR.train_item(hrs[i], *new.draw(i, r)[2:], P, scale, ig) for i in idx]
        return (torch.from_numpy(np.stack([l for l, _ in items])).float().div(255),
                torch.from_numpy(np.stack([h for _, h in items])).float().div(255))

    lr, hr = new.batch(idx, random.Random(3))
    el, eh = host_batch(random.Random(3))
    batch_equal = bool(torch.equal(lr.cpu(), el) and torch.equal(hr.cpu(), eh))
    S = (P + 2 * ig) * scale
    res = {"device": torch.cuda.get_device_name(0),
           "unit": {"device_us": "us per call, median (min, max) of %d windows of %d calls" % (a.reps, a.iters),
                    "host_ms": "ms per call, median (min, max) of %d" % a.host_reps},
           "note": "measured on one box in one run; the host legs run tests/bicubic_ref.py (numpy, the reference's arithmetic), "
                   "not the reference's imresize itself",
           "batch": {"scale": scale, "lr_patch_size": P, "ignored_boundary_size": ig, "batch": B,
                     "bytes_read": B * S * S * 3, "bytes_written": B * 3 * 4 * (P * P + (P * scale) ** 2),
                     "bicubic_cache_us": _device_us(lambda: new.batch(idx, rng), a.reps, a.iters),
                     "paired_cache_us": _device_us(lambda: old.batch(idx, rng), a.reps, a.iters),
                     "bicubic_cache_lr_only_us": _device_us(lambda: new.batch(idx, rng, want_hr=False), a.reps, a.iters),
                     "host_loop_ms": _host_ms(host_batch, a.host_reps), "device_equals_host": batch_equal}}
    b = res["batch"]
    b["host_over_device"] = round(b["host_loop_ms"]["median"] * 1e3 / b["bicubic_cache_us"]["median"], 1)
    frame = g.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    dframe = torch.from_numpy(frame).cuda()
    exp = BR.downscale(frame, scale)
    f = {"shape": [1080, 1920, 3], "scale": scale,
         "device_us": _device_us(lambda: bicubic_downscale(dframe, scale), a.reps, a.iters),
         "host_ms": _host_ms(lambda: BR.downscale(frame, scale), a.host_reps),
         "device_equals_host": bool(torch.equal(bicubic_downscale(dframe, scale).cpu(), torch.from_numpy(exp)))}
    f["host_over_device"] = round(f["host_ms"]["median"] * 1e3 / f["device_us"]["median"], 1)
    f["device_Mpixel_in_per_s"] = round(1080 * 1920 / f["device_us"]["median"], 1)
    res["frame"] = f
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
