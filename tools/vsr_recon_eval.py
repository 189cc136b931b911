#!/usr/bin/env python3
"""Time the WHOLE BasicVSR_origin(64, 30) -- propagation and reconstruction -- on a REDS-shaped clip, with given flows:

    python tools/vsr_recon_eval.py [--frames 15] [--height 180] [--width 320] [--blocks 30] [--reps 5] [--out profiles/vsr_recon_eval.json]

Three routes of `forward(x, 4h, 4w, flows=...)` under no_grad in one process: the HIP reconstruction (csrc/vsr_recon.h) in bf16 and
in fp32, and the ATen reconstruction (`aten_reconstruction = True`, the route before the HIP one existed) behind the same bf16
trunks.  Each is split into propagation (`propagate`, with the state handles or the NCHW fp32 features that route needs) and
reconstruction (whole forward minus propagation).  Also: a bf16 channels_last ATen restatement of the reconstruction alone, and every
HIP layer alone (`stages` bits of sr_c64_recon_fwd) with its algorithmic TFLOP/s.  Every figure is the median of --reps
repetitions after a warm-up, with (min, max); ms per frame.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps, per):
    fn()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / per)
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def _aten_recon_bf16(p, fb, ff, frame):
    out = torch.cat([fb, ff], 1)
    out = F.leaky_relu(F.conv2d(out, p["fusion.weight"], p["fusion.bias"]), 0.1)
    out = F.leaky_relu(F.pixel_shuffle(F.conv2d(out, p["upconv1.weight"], p["upconv1.bias"], padding=1), 2), 0.1)
    out = F.leaky_relu(F.pixel_shuffle(F.conv2d(out, p["upconv2.weight"], p["upconv2.bias"], padding=1), 2), 0.1)
    out = F.leaky_relu(F.conv2d(out, p["conv_hr.weight"], p["conv_hr.bias"], padding=1), 0.1)
    out = F.conv2d(out, p["conv_last.weight"], p["conv_last.bias"], padding=1)
    return out.float() + F.interpolate(frame, scale_factor=4, mode="bilinear", align_corners=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--blocks", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--profile", action="store_true", help="only the bf16 HIP forward, warm-up + one run (for rocprofv3 --kernel-trace)")
    a = ap.parse_args()
    from mobilesuperresolution_amd.models import flow_warp
    from mobilesuperresolution_amd.models.basicvsr_arch import propagate
    from mobilesuperresolution_amd.models.basicvsr_arch_origin import BasicVSR_origin
    n, h, w, nb = a.frames, a.height, a.width, a.blocks
    torch.manual_seed(0)
    sd = BasicVSR_origin(64, nb).state_dict()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, n, 3, h, w, generator=g).cuda()
    ff = (torch.rand(1, n - 1, 2, h, w, generator=g) * 8 - 4).cuda()
    fb = (torch.rand(1, n - 1, 2, h, w, generator=g) * 8 - 4).cuda()
    px = h * w
    gflop = {"fusion": 2 * 128 * 64 * px / 1e9, "upconv1": 2 * 64 * 256 * 9 * px / 1e9, "upconv2": 2 * 64 * 256 * 9 * 4 * px / 1e9,
             "conv_hr": 2 * 64 * 64 * 9 * 16 * px / 1e9, "conv_last": 2 * 64 * 3 * 9 * 16 * px / 1e9}
    res = {"shape": [1, n, 3, h, w], "blocks": nb, "unit": "ms per frame; median (min, max) of %d repetitions" % a.reps,
           "gflop_per_frame": {k: round(v, 2) for k, v in gflop.items()}}
    res["gflop_per_frame"]["reconstruction"] = round(sum(gflop.values()), 1)
    if a.profile:
        m = BasicVSR_origin(64, nb, hot_dtype="bf16")
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        with torch.no_grad():
            for _ in range(2):
                m(x, 4 * h, 4 * w, flows=(ff, fb))
        torch.cuda.synchronize()
        return
    with torch.no_grad():
        for name, dt, aten in (("hip_bf16", "bf16", False), ("hip_fp32", "fp32", False), ("aten_recon_bf16_trunks", "bf16", True)):
            m = BasicVSR_origin(64, nb, hot_dtype=dt)
            m.load_state_dict(sd, strict=True)
            m = m.cuda().eval()
            m.aten_reconstruction = aten
            whole = _time(lambda: m(x, 4 * h, 4 * w, flows=(ff, fb)), a.reps, n)
            prop = _time(lambda: propagate(x, ff, fb, m.backward_trunk, m.forward_trunk, flow_warp, num_feat=64, handles=not aten),
                         a.reps, n)
            res[name] = {"whole": whole, "propagation": prop,
                         "reconstruction": {k: round(whole[k] - prop["median"], 4) for k in ("median", "min", "max")}}
            if not aten:                                 # every layer alone, on one frame's images
                hb, hf = propagate(x[:, :1], ff[:, :0], fb[:, :0], m.backward_trunk, m.forward_trunk, flow_warp, num_feat=64, handles=True)
                out = torch.empty(1, 3, 4 * h, 4 * w, device="cuda")
                scratch = m.reconstruct_hot(hb[0], hf[0], x[:, 0], out)
                layers = {}
                for k, lname in enumerate(gflop):
                    t = _time(lambda: m.reconstruct_hot(hb[0], hf[0], x[:, 0], out, scratch, stages=1 << k), a.reps, 1)
                    t["tflops"] = round(gflop[lname] / t["median"], 1)
                    layers[lname] = t
                t = _time(lambda: m.reconstruct_hot(hb[0], hf[0], x[:, 0], out, scratch), a.reps, 1)
                t["tflops"] = round(sum(gflop.values()) / t["median"], 1)
                layers["all_five"] = t
                res[name]["layers"] = layers
                del scratch, hb, hf
            del m
            torch.cuda.empty_cache()
        # the reconstruction alone in bf16 channels_last ATen, on one frame
        p = {k: v.cuda().bfloat16() for k, v in sd.items() if k.split(".")[0] in ("fusion", "upconv1", "upconv2", "conv_hr", "conv_last")}
        for k, v in p.items():
            if v.dim() == 4:
                p[k] = v.contiguous(memory_format=torch.channels_last)
        fb_ = torch.randn(1, 64, h, w, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
        ff_ = torch.randn(1, 64, h, w, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
        res["aten_bf16_channels_last_reconstruction"] = _time(lambda: _aten_recon_bf16(p, fb_, ff_, x[:, 0]), a.reps, 1)
    hip, at = res["hip_bf16"]["reconstruction"], res["aten_recon_bf16_trunks"]["reconstruction"]
    res["bf16_reconstruction_speedup_vs_aten_fp32"] = round(at["median"] / hip["median"], 2)
    res["bf16_reconstruction_speedup_vs_aten_bf16_channels_last"] = round(
        res["aten_bf16_channels_last_reconstruction"]["median"] / res["hip_bf16"]["layers"]["all_five"]["median"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
