#!/usr/bin/env python3
"""Time the multi-frame video network (models/naive_multi_model_easy.py Naive_model(4, status = 8 blocks of [32, 32, 3])) on one
1x15x3x180x320 clip to 720x1280 under no_grad, in one process:

    python tools/multi_frame_eval.py [--runs 7] [--out profiles/multi_frame_eval.json]

Four routes on the same box and the same clip, alternating (hip bf16, hip fp32, aten under bf16 autocast, aten fp32, hip bf16, ..),
each once with given flows (`get_flow` replaced by a stored tensor) and once with SPyNet included; `--runs` timed calls each after
two warm-up rounds; ms per clip between two device events around one forward; median, min, max and the spread (max - min) / median
per route.  Also per stage of the HIP route (the `stages` mask of sr_mf_net_fwd: encoder, block 0, the 7 per-frame-network block
launches, the tail), from event pairs around single-stage calls on the scratch as it stands: block 0 and the tail against
blocks / 7 is the yardstick for "the new kernels are not the bottleneck".  Prints one JSON line and writes it to --out.  Needs a
GPU: no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NB = 8


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
        raise SystemExit("multi_frame_eval needs a GPU: a CPU run measures nothing")
    if a.runs < 5:
        raise SystemExit("at least five runs per route")
    from mobilesuperresolution_amd import hotpath as HP, packing as P
    from mobilesuperresolution_amd.models.naive_multi_model_easy import Naive_model
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    status = [[32, 32, 3]] * NB
    base = Naive_model(4, status=status, hot_dtype="bf16").to(dev).eval()
    f32 = Naive_model(4, status=status, hot_dtype="fp32").to(dev).eval()
    f32.load_state_dict(base.state_dict())
    aten = Naive_model(4, status=status).to(dev).eval()
    aten.load_state_dict(base.state_dict())
    aten.aten_forward = True
    models = (base, f32, aten)
    x = torch.rand(1, 15, 3, 180, 320, device=dev)
    with torch.no_grad():
        flows = base.get_flow(x).contiguous()

    def given(on):
        for m in models:
            if on:
                m.get_flow = lambda x_: flows
            else:
                m.__dict__.pop("get_flow", None)

    def autocast():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return aten(x)

    routes = {"hip_bf16": lambda: base(x), "hip_fp32": lambda: f32(x), "aten_bf16_autocast": autocast, "aten_fp32": lambda: aten(x)}
    times = {f"{k}/{v}": [] for v in ("given_flows", "with_spynet") for k in routes}
    with torch.no_grad():
        for rnd in range(a.runs + 2):
            for variant in ("given_flows", "with_spynet"):
                given(variant == "given_flows")
                for k, fn in routes.items():
                    t = _timed(fn)
                    if rnd >= 2:
                        times[f"{k}/{variant}"].append(t)
        assert base.last_route == "hip" and f32.last_route == "hip" and aten.last_route == "aten"
        given(True)
        ref = aten(x)
        err = {k: round(((routes[k]().float() - ref).abs().max() / ref.abs().max()).item(), 6) for k in ("hip_bf16", "hip_fp32", "aten_bf16_autocast")}
        spynet = _stats([_timed(lambda: base.flownet(x[0, 1:], x[0, :-1])) for _ in range(a.runs + 2)][2:])
        stages = {}
        for name, m in (("bf16", base), ("fp32", f32)):
            blob, head = m._blobs()
            frames = x.reshape(15, 3, 180, 320).contiguous()
            scratch = torch.zeros((3, 15, 180, 320, P.FN_C), dtype=m.hot_dtype, device=dev)
            out = torch.empty((15, 3, 720, 1280), dtype=torch.float32, device=dev)
            per = {}
            for sname, bit in (("encoder", P.MF_ENCODER), ("first_block", P.MF_FIRST), ("blocks_x7", P.MF_BLOCKS), ("tail", P.MF_TAIL)):
                call = lambda: HP.mf_net_fwd(frames, flows, blob, head, scratch, out, NB, 1, 15, bit)
                for _ in range(2):
                    call()
                per[sname] = _stats([_timed(call) for _ in range(a.runs)])
            per["per_fn_block"] = round(per["blocks_x7"]["median"] / (NB - 1), 4)
            stages[name] = per
    res = {"device": torch.cuda.get_device_name(0), "model": f"Naive_model(4, status={NB} x [32, 32, 3])", "clip": [1, 15, 3, 180, 320],
           "output": [720, 1280], "unit": "ms per clip (15 frames), device events around one forward; routes alternate in one process",
           "routes": {k: _stats(v) for k, v in times.items()}, "spynet_14_pairs_ms": spynet, "hip_stages_ms": stages,
           "rel_max_abs_vs_aten_fp32": err}
    r = res["routes"]
    for v in ("given_flows", "with_spynet"):
        hip, at = r[f"hip_bf16/{v}"], r[f"aten_bf16_autocast/{v}"]
        res[f"hip_bf16_over_aten_bf16/{v}"] = round(at["median"] / hip["median"], 3)
        # the difference of the medians against the larger absolute run-to-run spread of the two routes
        res[f"difference_exceeds_spread/{v}"] = bool(abs(at["median"] - hip["median"]) > max(at["max"] - at["min"], hip["max"] - hip["min"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
