#!/usr/bin/env python3
"""Time the per-frame video network (models/single_image_model.py Result_Model(4, 32, 8, 3)) on one 1x15x3x180x320 clip to 720x1280,
in one process:

    python tools/frame_net_eval.py [--runs 7] [--out profiles/frame_net_eval.json]

Four routes on the same box and the same clip, alternating (hip bf16, hip fp32, aten fp32, aten under bf16 autocast, hip bf16, ..),
`--runs` timed calls each after two warm-up rounds; ms per clip between two device events around one forward; median, min, max and
the spread (max - min) / median per route.  Also per stage of the HIP route (the `stages` mask of sr_fn_net_fwd: encoder, the 8 block
launches, the last conv, the upsampler), from event pairs around single-stage calls on the scratch as it stands.  Prints one JSON line
and writes it to --out.  Needs a GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(ts):
    med = statistics.median(ts)
    return {"median": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "spread": round((max(ts) - min(ts)) / med, 4),
            "runs": len(ts)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_net_eval needs a GPU: a CPU run measures nothing")
    if a.runs < 5:
        raise SystemExit("at least five runs per route")
    from mobilesuperresolution_amd import hotpath as HP, packing as P
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base = Result_Model(4, 32, 8, 3, hot_dtype="bf16").to(dev).eval()
    f32 = Result_Model(4, 32, 8, 3, hot_dtype="fp32").to(dev).eval()
    f32.load_state_dict(base.state_dict())
    aten = Result_Model(4, 32, 8, 3).to(dev).eval()
    aten.load_state_dict(base.state_dict())
    aten.aten_forward = True
    x = torch.rand(1, 15, 3, 180, 320, device=dev)

    def autocast():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return aten(x, 720, 1280)

    routes = {"hip_bf16": lambda: base(x, 720, 1280), "hip_fp32": lambda: f32(x, 720, 1280), "aten_fp32": lambda: aten(x, 720, 1280),
              "aten_bf16_autocast": autocast}
    times = {k: [] for k in routes}
    with torch.no_grad():
        for rnd in range(a.runs + 2):
            for k, fn in routes.items():
                t = _timed(fn)
                if rnd >= 2:
                    times[k].append(t)
        assert base.last_route == "hip" and f32.last_route == "hip" and aten.last_route == "aten"
        ref = aten(x, 720, 1280)
        err = {k: round(((routes[k]().float() - ref).abs().max() / ref.abs().max()).item(), 6) for k in ("hip_bf16", "hip_fp32", "aten_bf16_autocast")}
        # per stage, HIP route
        stages = {}
        for name, m in (("bf16", base), ("fp32", f32)):
            blob, offs, head = m._blobs()
            frames = x.reshape(15, 3, 180, 320).contiguous()
            scratch = torch.zeros((3, 15, 180, 320, P.FN_C), dtype=m.hot_dtype, device=dev)
            out = torch.empty((15, 3, 720, 1280), dtype=torch.float32, device=dev)
            per = {}
            for sname, bit in (("encoder", P.FN_ENCODER), ("blocks_x8", P.FN_BLOCKS), ("last_conv", P.FN_LAST), ("upsampler", P.FN_UP)):
                call = lambda: HP.fn_net_fwd(frames, blob, offs, head, scratch, out, out.stride(0), 8, bit)
                for _ in range(2):
                    call()
                per[sname] = _stats([_timed(call) for _ in range(a.runs)])
            stages[name] = per
    res = {"device": torch.cuda.get_device_name(0), "model": "Result_Model(4, 32, 8, 3)", "clip": [1, 15, 3, 180, 320], "output": [720, 1280],
           "unit": "ms per clip (15 frames), device events around one forward; routes alternate in one process",
           "routes": {k: _stats(v) for k, v in times.items()}, "hip_stages_ms": stages,
           "rel_max_abs_vs_aten_fp32": err}
    r = res["routes"]
    res["hip_bf16_over_aten_bf16"] = round(r["aten_bf16_autocast"]["median"] / r["hip_bf16"]["median"], 3)
    res["hip_bf16_over_aten_fp32"] = round(r["aten_fp32"]["median"] / r["hip_bf16"]["median"], 3)
    res["hip_fp32_over_aten_fp32"] = round(r["aten_fp32"]["median"] / r["hip_fp32"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
