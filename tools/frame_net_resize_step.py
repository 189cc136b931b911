#!/usr/bin/env python3
"""Time one training step of the per-frame video network (`single`: Result_Model(4, 32, 8, 3)) at the NEMO shape, 8 x 2 x 3 x 240 x 426
frames trained towards 1080 x 1920 (nemo_single.bash's batch), with and without `hot_resize_fold`:

    python tools/frame_net_resize_step.py [--runs 7] [--warmup 2] [--out profiles/frame_net_resize_fold.json]

  baseline    hot_training + hot_resize: forward, training.L1_Charbonnier_loss on torch's ops (the fold declines at this size), backward,
              training.Adam -- what the parent commit runs, flag for flag
  folded      the same loop with hot_resize_fold: the criterion folds into the sized backward (sr_fn_net_bwd_loss_sized)
  train_step  model.train_step(lr, hr, optimizer): the whole step as one C call (sr_fn_net_train_step_sized)

in bf16 and fp32, with each route's peak allocated memory during a step.  The three routes of a dtype alternate in ONE process, round by
round (so drift of the clocks hits them alike); `warmup` untimed rounds, then `runs` timed ones, device events around each step, the
loss read back inside the timed span in every route (the trainer's per-step loss.item()).  Per route: the median, min, max and max -
min.  A gain counts only when the medians differ by more than the larger of the two spreads (`margin_exceeds_spread`); `not_slower`
says that the new route's median does not exceed the baseline's by more than that spread.  One box, one run.  Writes the JSON to --out
and prints it as one line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.frame_net_resize_eval import H, OH, OW, W, alternate, compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "frame_net_resize_fold.json"))
    args = ap.parse_args()
    from mobilesuperresolution_amd import training
    from mobilesuperresolution_amd.models import SingleFrameVSR
    g = torch.Generator().manual_seed(0)
    x = torch.rand(8, 2, 3, H, W, generator=g).cuda()
    hr = torch.rand(8, 2, 3, OH, OW, generator=g).cuda()
    crit = training.L1_Charbonnier_loss()
    out = {"tool": "frame_net_resize_step", "device": torch.cuda.get_device_name(0), "clip": [8, 2, 3, H, W], "out_size": [OH, OW],
           "runs": args.runs, "warmup": args.warmup,
           "note": "one box, one run; the three routes of a dtype alternate in one process; the baseline row is the parent commit's route"}

    def model(dt, fold):
        torch.manual_seed(1)
        m = SingleFrameVSR(4, 32, 8, 3, hot_dtype=dt).cuda()
        m.hot_training = m.hot_resize = True
        m.hot_resize_fold = fold
        return m

    def loop(dt, fold):
        m = model(dt, fold)
        opt = training.Adam(m.parameters(), lr=1e-4)

        def step():
            opt.zero_grad()
            loss = crit(m(x, OH, OW), hr)
            folded = type(loss.grad_fn).__name__ == "_FoldedCriterionBackward"
            loss.backward()
            opt.step()
            loss.item()
            return m.last_route + ("+fold" if folded else "")
        return step

    def one_call(dt):
        m = model(dt, True)
        opt = training.Adam([p for mod in (m.encoder, m.body, m.shuf) for p in mod.parameters()], lr=1e-4)

        def step():
            m.train_step(x, hr, opt).item()
            return m.last_route
        return step

    for dt in ("bf16", "fp32"):
        routes = {"baseline": loop(dt, False), "folded": loop(dt, True), "train_step": one_call(dt)}
        rows = alternate(routes, args.runs, args.warmup, peak=True)
        assert rows["baseline"]["route"] == "hip_train" and rows["folded"]["route"] == "hip_train+fold"
        assert rows["train_step"]["route"] == "hip_train_step"
        cmp = {k: compare(rows, k, "baseline") for k in ("folded", "train_step")}
        for k, c in cmp.items():
            c["not_slower"] = -c["margin_ms"] <= max(rows[k]["spread_ms"], rows["baseline"]["spread_ms"])
        out[dt] = {"routes": rows, **cmp}
        del routes
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
