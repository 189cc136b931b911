#!/usr/bin/env python
"""Training-step timing of BasicVSR_origin at 64 features with and without the flow gradient (`flow_training`),
in ONE process on one device, bf16.

    python tools/vsr64_flow_step.py [--steps 3] [--rows abcd] [--blocks 8,30] [--out profiles/vsr64_flow_step.json]

Workload: 8 clips x 5 frames x 64x64 -> 256x256, forward + Charbonnier + backward + torch.optim.Adam; BasicVSR_origin(64, 8) and
(64, 30), `hot_training` on.  The protocol of tools/vsr_origin_step.py: the rows share one model and alternate after a warm-up, 7 runs
per row, each the mean of --steps steps between two HIP events; reported as median [min - max].

  a  given flows, flow_training off                       (the default route: what the step cost before the flag existed)
  b  given LEAF flows that require grad, flow_training on  (a + c64_warp_dflow_kernel per frame step + dx0 where it was not wanted)
  c  SPyNet computes the flows and receives gradients      (spynet.hot_training; SPyNet's parameters in Adam at a quarter of the rate)
  d  a bf16 channels_last ATen restatement of (c) under autograd

`--rows a` touches nothing the flag added, so the same file also times row (a) on a checkout that does not have it:
SR_PACKAGE_ROOT=<that checkout> makes the package import from there."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.environ.get("SR_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilesuperresolution_amd import _lib as L                                    # noqa: E402
from mobilesuperresolution_amd.models import BasicVSR_origin                       # noqa: E402


def charbonnier(a, b, eps=1e-6):
    return torch.sqrt((a - b) ** 2 + eps).mean()


def calls_of(fn):
    names, real = [], L.launch

    def counting(name, f, *a):
        names.append(name)
        return real(name, f, *a)
    L.launch = counting
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.launch = real
    return {k: names.count(k) for k in sorted(set(names))}


def dflow_kernel_ms(fn):
    """device time of c64_warp_dflow_kernel in one step (torch.profiler kernel trace): (launches, total ms)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n, us = 0, 0.0
    for ev in prof.key_averages():
        if "c64_warp_dflow" in ev.key:
            t = getattr(ev, "device_time_total", None)
            us += t if t is not None else getattr(ev, "cuda_time_total", 0.0)
            n += ev.count
    return dict(launches=n, total_ms=us / 1e3)


# ---- row d: the model in bf16 channels_last ATen ------------------------------------------------------------------------------------
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _aten_spynet(p, mean, std, ref, supp):
    """SpyNet.forward, the five convolutions per level in bf16 channels_last, the glue in fp32 as in the package (tools/spynet_train_step.py)"""
    from mobilesuperresolution_amd.models.spynet_arch import _border_warp
    refs, supps = [(ref - mean) / std], [(supp - mean) / std]
    for _ in range(5):
        refs.insert(0, F.avg_pool2d(refs[0], 2, 2, count_include_pad=False))
        supps.insert(0, F.avg_pool2d(supps[0], 2, 2, count_include_pad=False))
    flow = refs[0].new_zeros(refs[0].size(0), 2, refs[0].size(2) // 2, refs[0].size(3) // 2)
    for lv in range(6):
        up = F.interpolate(flow, scale_factor=2, mode="bilinear", align_corners=True) * 2.0
        x = _cl(torch.cat([refs[lv], _border_warp(supps[lv], up), up], 1).bfloat16())
        for i in range(5):
            q = f"spynet.basic_module.{lv}.basic_module.{2 * i}."
            x = F.conv2d(x, p[q + "weight"], p[q + "bias"], padding=3)
            x = F.relu(x) if i < 4 else x
        flow = x.float() + up
    return flow


def _aten_warp(x, flow):
    _, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=x.device), torch.arange(w, dtype=torch.float32, device=x.device),
                            indexing="ij")
    grid = torch.stack((2.0 * (gx + flow[:, 0]) / max(w - 1, 1) - 1.0, 2.0 * (gy + flow[:, 1]) / max(h - 1, 1) - 1.0), 3)
    return _cl(F.grid_sample(x.float(), grid, mode="bilinear", padding_mode="zeros", align_corners=True).bfloat16())


def _aten_trunk(p, prefix, x, nb):
    y = F.leaky_relu(F.conv2d(x, p[prefix + "main.0.weight"], p[prefix + "main.0.bias"], padding=1), 0.1)
    for i in range(nb):
        q = f"{prefix}main.2.{i}."
        t = F.relu(F.conv2d(y, p[q + "conv1.weight"], p[q + "conv1.bias"], padding=1))
        y = y + F.conv2d(t, p[q + "conv2.weight"], p[q + "conv2.bias"], padding=1)
    return y


def aten_model(p, mean, std, x, nb, f=64):
    b, n, c, h, w = x.shape
    x1, x2 = x[:, :-1].reshape(-1, c, h, w), x[:, 1:].reshape(-1, c, h, w)
    fb = _aten_spynet(p, mean, std, x1, x2).view(b, n - 1, 2, h, w)
    ff = _aten_spynet(p, mean, std, x2, x1).view(b, n - 1, 2, h, w)
    xh = x.bfloat16()
    feats = {}
    for name, flows, order in (("backward", fb, range(n - 1, -1, -1)), ("forward", ff, range(n))):
        feat, res = _cl(xh.new_zeros(b, f, h, w)), {}
        for k, i in enumerate(order):
            if k:
                feat = _aten_warp(feat, flows[:, i if name == "backward" else i - 1])
            feat = _aten_trunk(p, name + "_trunk.", _cl(torch.cat([xh[:, i], feat], 1)), nb)
            res[i] = feat
        feats[name] = res
    lrelu = lambda t: F.leaky_relu(t, 0.1)
    conv = lambda name, t, pad: F.conv2d(t, p[name + ".weight"], p[name + ".bias"], padding=pad)
    outs = []
    for i in range(n):
        out = lrelu(conv("fusion", _cl(torch.cat([feats["backward"][i], feats["forward"][i]], 1)), 0))
        out = lrelu(F.pixel_shuffle(conv("upconv1", out, 1), 2))
        out = lrelu(F.pixel_shuffle(conv("upconv2", out, 1), 2))
        out = conv("conv_last", lrelu(conv("conv_hr", out, 1)), 1)
        outs.append(out.float() + F.interpolate(x[:, i], scale_factor=4, mode="bilinear", align_corners=False))
    return torch.stack(outs, 1)


# ---- the rows ----------------------------------------------------------------------------------------------------------------------
def case(num_block, rows, steps, warmup=2, runs=7, dtype="bf16"):
    torch.manual_seed(0)
    m = BasicVSR_origin(num_feat=64, num_block=num_block, hot_dtype=dtype).cuda().train()
    m.hot_training = True
    g = torch.Generator().manual_seed(1)
    x = torch.rand(8, 5, 3, 64, 64, generator=g).cuda()
    mv = (torch.rand(8, 5, 2, 64, 64, generator=g) * 6 - 3).cuda()
    given = (mv[:, 1:].contiguous(), (-mv[:, 1:]).contiguous())
    leaves = tuple(t.clone().requires_grad_(True) for t in given)
    hr = torch.rand(8, 5, 3, 256, 256, generator=g).cuda()
    spy = list(m.spynet.parameters())
    body = [q for k, q in m.named_parameters() if not k.startswith("spynet.")]
    opt = torch.optim.Adam(body, lr=1e-4)
    opt_spy = torch.optim.Adam(spy, lr=2.5e-5)
    fns = {}

    def hip_step(flows, spynet):
        for q in spy:
            q.requires_grad_(spynet)
        m.spynet.hot_training = spynet
        opt.zero_grad(set_to_none=True)
        opt_spy.zero_grad(set_to_none=True)
        for t in leaves:
            t.grad = None
        charbonnier(m(x, 256, 256, flows=flows), hr).backward()
        opt.step()
        if spynet:
            opt_spy.step()

    def flag(on):
        if "b" in rows or "c" in rows:                   # row a alone never names the flag
            m.flow_training = on

    if "a" in rows:
        fns["a_given_flows"] = lambda: (flag(False), hip_step(given, False))
    if "b" in rows:
        fns["b_leaf_flows_flow_training"] = lambda: (flag(True), hip_step(leaves, False))
    if "c" in rows:
        fns["c_spynet_trained"] = lambda: (flag(True), hip_step(None, True))
    if "d" in rows:
        p = {k: (_cl(v.detach().bfloat16()) if v.dim() == 4 else v.detach().bfloat16()).requires_grad_(True) for k, v in m.state_dict().items()
             if v.is_floating_point() and k not in ("spynet.mean", "spynet.std")}     # the trunks' reference keys are views of `flat`
        opt_d = torch.optim.Adam([{"params": [v for k, v in p.items() if not k.startswith("spynet.")], "lr": 1e-4},
                                  {"params": [v for k, v in p.items() if k.startswith("spynet.")], "lr": 2.5e-5}])
        mean, std = m.spynet.mean, m.spynet.std

        def aten_step():
            opt_d.zero_grad(set_to_none=True)
            charbonnier(aten_model(p, mean, std, x, num_block), hr).backward()
            opt_d.step()
        fns["d_aten_bf16_channels_last"] = aten_step
    res = {k: dict(runs_ms=[]) for k in fns}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        if not k.startswith("d_"):
            res[k]["c_abi_calls_per_step"] = calls_of(fn)
    torch.cuda.synchronize()
    for _ in range(runs):
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            res[k]["runs_ms"].append(e0.elapsed_time(e1) / steps)
            res[k]["peak_memory_mib"] = max(res[k].get("peak_memory_mib", 0.0), torch.cuda.max_memory_allocated() / 2 ** 20)
    for k in fns:
        ts = res[k]["runs_ms"]
        res[k].update(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), spread_ms=max(ts) - min(ts), steps_per_run=steps)
    if "b_leaf_flows_flow_training" in fns:
        try:
            res["b_leaf_flows_flow_training"]["c64_warp_dflow_kernel"] = dflow_kernel_ms(fns["b_leaf_flows_flow_training"])
        except Exception as e:                            # the trace is an extra: the step times above stand without it
            res["b_leaf_flows_flow_training"]["c64_warp_dflow_kernel"] = dict(error=repr(e)[:200])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rows", default="abcd")
    ap.add_argument("--blocks", default="8,30")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), dtype="bf16",
               workload="8 clips x 5 frames x 64x64 -> 256x256, forward + Charbonnier + backward + Adam; rows: see tools/vsr64_flow_step.py",
               train_8x5x64x64={f"f64_b{nb}": case(int(nb), a.rows, a.steps) for nb in a.blocks.split(",")})
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
