#!/usr/bin/env python3
"""Time the video trainer's loop (reference train_video_superresolution.py:86-100) on the HIP training routes, with and without the
two drop-ins of mobilesuperresolution_amd.training:

    python tools/video_loop_step.py [--parent-root DIR] [--rounds 2] [--runs 3] [--steps 40] [--warmup 10] [--out profiles/video_loop_step.json]

The loop, per step: optimizer.zero_grad(); sr = model(lr, h, w); loss = 0; loss += weight * criterion(sr, hr); loss.backward();
optimizer.step(); optimizer.zero_grad(); loss.item() -- the per-step read of the loss included.  Shape: 8 clips x 5 frames x 3 x 64 x 64
-> 256 x 256, `single` = Result_Model(4, 32, 8, 3) and `multi` = Naive_model with 8 blocks of [32, 32, 3] and GIVEN flows (uniform in
+-3 px), hot_training = True, bf16 and fp32.

Columns:
  torch      the trainer's own pieces: mean(sqrt(d d + 1e-12)) as torch ops + torch.optim.Adam(betas=(0.9, 0.99))
  dropins    training.L1_Charbonnier_loss() + training.Adam: the loss folded into the HIP backward, the multi-tensor Adam step
  train_step model.train_step(lr, hr, optimizer, "charbonnier", loss_weight=weight) with a training.Adam over the trained parameters: the
             whole step as one C call (weight norm, packing, forward, folded loss, backward, weight-norm backward, Adam), then loss.item()
  parent     the same two drop-ins of the package found under --parent-root (a built checkout of the parent commit)

A child process per package root measures every (network, dtype); inside it the columns alternate run by run.  The driver alternates
parent and current children `rounds` times, so both see the same drift.  A run is `steps` steps timed with the host clock (every
step ends in loss.item(), a device synchronise) after `warmup` untimed steps per column; the figure of a run is its mean step time.
Per column: the median over all runs and max - min over them.  Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NETS = ("single", "multi")
DTYPES = ("bf16", "fp32")


def child(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from mobilesuperresolution_amd import training
    from mobilesuperresolution_amd.models import MultiFrameVSR, SingleFrameVSR
    assert torch.cuda.is_available(), "video_loop_step needs a GPU (there is no CPU timing)"
    b, n, s, nb = 8, 5, 64, 8
    g = torch.Generator().manual_seed(0)
    lr_clip = torch.rand(b, n, 3, s, s, generator=g).cuda()
    hr = torch.rand(b, n, 3, 4 * s, 4 * s, generator=g).cuda()
    given = (6 * torch.rand(b, n - 1, 2, s, s, generator=g) - 3).cuda()
    weight = 1.0
    columns = args.columns.split(",")
    out = {}

    def loop(net, dt, column):
        torch.manual_seed(1)
        if net == "single":
            m = SingleFrameVSR(4, 32, nb, 3, hot_dtype=dt).cuda()
        else:
            m = MultiFrameVSR(4, status=[[32, 32, 3]] * nb, hot_dtype=dt).cuda()
            m.get_flow = lambda x_: given
        m.hot_training = True
        params = [p for p in m.parameters() if p.requires_grad]
        seen = {}
        if column == "train_step":
            never_called = lambda k: k.startswith(("flownet.", "skip.")) or ".skip." in k
            optimizer = training.Adam([p for k, p in m.named_parameters() if not never_called(k)], lr=1e-4, betas=(0.9, 0.99))

            def one_call():
                loss = m.train_step(lr_clip, hr, optimizer, "charbonnier", loss_weight=weight)
                seen["node"] = "none"
                seen["loss"] = loss.item()
                seen["route"] = m.last_route
            return one_call, seen
        if column == "torch":
            charb = training.L1_Charbonnier_loss()
            criterion = charb._torch_loss                     # the trainer's own expression, torch ops
            optimizer = torch.optim.Adam(params, lr=1e-4, betas=(0.9, 0.99))
        else:
            criterion = training.L1_Charbonnier_loss()
            optimizer = training.Adam(params, lr=1e-4, betas=(0.9, 0.99))

        def step():
            optimizer.zero_grad()
            sr = m(lr_clip, hr.shape[3], hr.shape[4])
            term = criterion(sr, hr)
            seen["node"] = type(term.grad_fn).__name__
            loss = 0
            loss += weight * term
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
            seen["loss"] = loss.item()
            seen["route"] = m.last_route
        return step, seen

    for net in NETS:
        for dt in DTYPES:
            loops = {c: loop(net, dt, c) for c in columns}
            for step, _ in loops.values():
                for _ in range(args.warmup):
                    step()
            runs = {c: [] for c in columns}
            for _ in range(args.runs):
                for c, (step, _) in loops.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    runs[c].append((time.perf_counter() - t0) * 1e3 / args.steps)
            out[f"{net}_{dt}"] = {c: {"run_ms": runs[c], "route": loops[c][1]["route"], "loss_node": loops[c][1]["node"],
                                      "last_loss": loops[c][1]["loss"]} for c in columns}
            del loops
            torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "results": out}))


def _spawn(root, columns, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--columns", columns, "--runs", str(args.runs),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
    if res.returncode != 0:
        raise RuntimeError(f"child for {root} ended with {res.returncode}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def _column(runs):
    t = sorted(runs)
    return {"run_ms": runs, "median_ms": t[len(t) // 2], "spread_ms": t[-1] - t[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (its package directory's parent)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_loop_step.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--columns", default="torch,dropins")
    args = ap.parse_args()
    if args.child:
        return child(args)
    merged, meta, device = {}, {}, None
    for _ in range(args.rounds):
        for name, root, columns in (("parent", args.parent_root, "dropins"), ("current", ROOT, "torch,dropins,train_step")):
            if root is None:
                continue
            got = _spawn(root, columns, args)
            device = got["device"]
            for key, cols in got["results"].items():
                for c, v in cols.items():
                    col = "parent" if name == "parent" else c
                    merged.setdefault(key, {}).setdefault(col, []).extend(v["run_ms"])
                    meta.setdefault(key, {})[col] = {k: v[k] for k in ("route", "loss_node", "last_loss")}
    out = {"tool": "video_loop_step", "device": device, "clips": 8, "frames": 5, "lr_size": 64, "blocks": 8, "rounds": args.rounds,
           "runs_per_child": args.runs, "steps_per_run": args.steps, "warmup": args.warmup, "unit": "ms per step, host clock, loss.item() included",
           "results": {}}
    for key, cols in merged.items():
        res = {c: dict(_column(r), **meta[key][c]) for c, r in cols.items()}
        res["torch_pieces_share_ms"] = res["torch"]["median_ms"] - res["dropins"]["median_ms"]
        if "parent" in res:
            gain = res["parent"]["median_ms"] - res["dropins"]["median_ms"]
            res["gain_over_parent_ms"] = gain
            res["gain_exceeds_spread"] = gain > max(res["parent"]["spread_ms"], res["dropins"]["spread_ms"])
            if "train_step" in res:
                gain = res["parent"]["median_ms"] - res["train_step"]["median_ms"]
                res["train_step_gain_over_parent_ms"] = gain
                res["train_step_gain_exceeds_spread"] = gain > max(res["parent"]["spread_ms"], res["train_step"]["spread_ms"])
        else:
            res["parent"] = "not measured"
        out["results"][key] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
