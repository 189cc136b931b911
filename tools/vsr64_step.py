#!/usr/bin/env python3
"""Time one training step of the two-trunk propagation of BasicVSR_origin(64, nb) on the opt-in HIP training route
(ConvResidualBlocks.hot_training):

    python tools/vsr64_step.py [--blocks 30,8] [--clips 8] [--frames 5] [--size 64] [--runs 7] [--caps 32,64,128]

forward + Charbonnier loss on the features + backward, both time directions in the same launches, given flows, bf16 and fp32.
Next to it, alternating in the same process: the bf16 channels_last ATen restatement of the same step under autograd (the
pattern of tools/vsr64_eval.py).  Per route: median and min-max of --runs runs after a warm-up, the peak memory of a step, and
(HIP bf16) the kernel-time shares of backward-data, weight gradient, slab reduction and warp backward from a torch.profiler
trace.  --caps also times the HIP bf16 step at those values of WGRAD64_WGS.  Writes profiles/vsr64_step.json and prints it."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _aten_trunk(p, x, nb):
    y = F.leaky_relu(F.conv2d(x, p["main.0.weight"], p["main.0.bias"], padding=1), 0.1)
    for i in range(nb):
        t = F.relu(F.conv2d(y, p[f"main.2.{i}.conv1.weight"], p[f"main.2.{i}.conv1.bias"], padding=1))
        y = y + F.conv2d(t, p[f"main.2.{i}.conv2.weight"], p[f"main.2.{i}.conv2.bias"], padding=1)
    return y


def _aten_propagate(pb, pf, x, ff, fb, nb, grid):
    n = x.shape[1]
    feat_b = feat_f = None
    out_b, out_f = [], []
    for k in range(n):
        i = n - 1 - k
        xb = x[:, i].contiguous(memory_format=torch.channels_last)
        xf = x[:, k].contiguous(memory_format=torch.channels_last)
        if k == 0:
            wb = wf = torch.zeros_like(xb[:, :1]).expand(-1, 64, -1, -1)
        else:
            wb = F.grid_sample(feat_b, grid(fb[:, i]), mode="bilinear", padding_mode="zeros", align_corners=True)
            wf = F.grid_sample(feat_f, grid(ff[:, k - 1]), mode="bilinear", padding_mode="zeros", align_corners=True)
        feat_b = _aten_trunk(pb, torch.cat([xb, wb], 1).contiguous(memory_format=torch.channels_last), nb)
        feat_f = _aten_trunk(pf, torch.cat([xf, wf], 1).contiguous(memory_format=torch.channels_last), nb)
        out_b.insert(0, feat_b)
        out_f.append(feat_f)
    return out_b, out_f


def _charbonnier(feats, target):
    return torch.sqrt((torch.stack(feats, 1).float() - target) ** 2 + 1e-6).mean()


def _once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


GROUPS = (("weight_gradient", "c64_wgrad"), ("warp_backward", "c64_warp_bwd"), ("slab_reduction", "unpack_all"))
# c64_conv_kernel<T, 64, none, ADD, false, DZ, false> instances that only the backward launches (mangled and demangled spellings)
BWD_DATA = ("Li64ELi0ELb0ELb0ELi0ELb0E", "Li64ELi0ELb1ELb0ELi1", "Li64ELi0ELb0ELb0ELi2", "64, 0, false, false, 0, false", "64, 0, true, false, 1",
            "64, 0, false, false, 2")


def _shares(fn):
    """kernel-time shares of one step by kernel name; the backward-data launches are the c64_conv_kernel instances with the masked
    staging (DZ = 1, 2) plus the plain 64 -> 64 conv without activation that only the backward launches"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        tot, by = 0.0, {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            if not t:
                continue
            tot += t
            name = ev.key
            grp = "other"
            if "c64_conv_kernel" in name and any(k in name for k in BWD_DATA):
                grp = "backward_data"
            elif "c64_conv_kernel" in name:
                grp = "forward_convs"
            else:
                for g, key in GROUPS:
                    if key in name:
                        grp = g
            by[grp] = by.get(grp, 0.0) + t
        if tot <= 0:
            return {"error": "the trace holds no kernel times"}
        return {k: round(v / tot, 3) for k, v in sorted(by.items())} | {"kernel_ms_total": round(tot / 1e3, 3)}
    except Exception as e:                               # a box without the tracer: say so rather than invent a share
        return {"error": f"not measured: {type(e).__name__}: {e}"[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="30,8")
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--caps", default="32,64,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vsr64_step.json"))
    a = ap.parse_args()
    from mobilesuperresolution_amd.models import flow_warp, set_wide_training
    from mobilesuperresolution_amd.models import basicvsr_arch as A
    from mobilesuperresolution_amd.models.basicvsr_arch_origin import BasicVSR_origin
    b, n, h = a.clips, a.frames, a.size
    g = torch.Generator().manual_seed(1)
    x = torch.rand(b, n, 3, h, h, generator=g).cuda()
    ff = (torch.rand(b, n - 1, 2, h, h, generator=g) * 8 - 4).cuda()
    fb = (torch.rand(b, n - 1, 2, h, h, generator=g) * 8 - 4).cuda()
    target = torch.rand(b, 2 * n, 64, h, h, generator=g).cuda()
    gy, gx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(h, device="cuda", dtype=torch.float32),
                            indexing="ij")

    def grid(fl):
        vx = 2.0 * (gx + fl[:, 0]) / max(h - 1, 1) - 1.0
        vy = 2.0 * (gy + fl[:, 1]) / max(h - 1, 1) - 1.0
        return torch.stack((vx, vy), 3).bfloat16()

    res = {"shape": [b, n, 3, h, h], "runs": a.runs, "default_cap": A.WGRAD64_WGS, "models": {}}
    for nb in [int(v) for v in a.blocks.split(",")]:
        torch.manual_seed(0)
        sd = BasicVSR_origin(64, nb).state_dict()
        steps = {}
        for dt in ("bf16", "fp32"):
            m = BasicVSR_origin(64, nb, hot_dtype=dt)
            m.load_state_dict(sd, strict=True)
            m = m.cuda()
            set_wide_training(m)

            def hip(m=m):
                m.backward_trunk.flat.grad = m.forward_trunk.flat.grad = None
                ob, of = A.propagate(x, ff, fb, m.backward_trunk, m.forward_trunk, flow_warp, num_feat=64)
                _charbonnier(ob + of, target).backward()
            steps["hip_" + dt] = hip
        pb = {k[len("backward_trunk."):]: v.cuda().bfloat16() for k, v in sd.items() if k.startswith("backward_trunk.")}
        pf = {k[len("forward_trunk."):]: v.cuda().bfloat16() for k, v in sd.items() if k.startswith("forward_trunk.")}
        for p in (pb, pf):
            for k, v in p.items():
                p[k] = (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v).requires_grad_(True)
        xb = x.bfloat16()

        def aten():
            for p in (pb, pf):
                for v in p.values():
                    v.grad = None
            ob, of = _aten_propagate(pb, pf, xb, ff, fb, nb, grid)
            _charbonnier(ob + of, target).backward()
        steps["aten_bf16"] = aten
        for fn in steps.values():                           # warm-up: packing, tables, allocator, kernel load
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in steps}
        for _ in range(a.runs):                             # the routes alternate
            for k, fn in steps.items():
                times[k].append(_once(fn))
        out = {k: _stats(v) | {"peak_mib": _peak(steps[k])} for k, v in times.items()}
        out["hip_bf16"]["kernel_shares"] = _shares(steps["hip_bf16"])
        out["hip_bf16_speedup_vs_aten_bf16"] = round(out["aten_bf16"]["median_ms"] / out["hip_bf16"]["median_ms"], 2)
        caps = {}
        keep = A.WGRAD64_WGS
        for cap in [int(v) for v in a.caps.split(",") if v]:
            A.WGRAD64_WGS = cap
            steps["hip_bf16"]()
            caps[str(cap)] = _stats([_once(steps["hip_bf16"]) for _ in range(a.runs)])
        A.WGRAD64_WGS = keep
        out["hip_bf16_by_wgrad_cap"] = caps
        res["models"][f"BasicVSR_origin(64, {nb})"] = out
        del steps, pb, pf
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
