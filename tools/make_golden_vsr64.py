#!/usr/bin/env python3
"""Write fixture G17 (tests/golden/g17_vsr_trunk64.npz) by running the REFERENCE's BasicVSR_origin at 64 features on the CPU:

    SR_REFERENCE_ROOT=<reference checkout> python tools/make_golden_vsr64.py

models/basicvsr_arch_origin.py is imported from the reference with mmedit stubbed (oracle/make_golden.py's `_mmedit_stubs`).
`BasicVSR_origin(num_feat=64, num_block=1)` runs in eval mode under torch.no_grad() on 1 clip x 3 frames of 18 x 20 (partial
16 x 16 tiles in both directions) with GIVEN flows (`get_flow` overridden, as for G12); forward hooks on the two trunks record
their per-frame features (call order: the backward-time trunk sees frame n-1 .. 0).

Stored: the frames, both flows, both trunks' parameters and the hooked features -- no reconstruction weights, which the
trunk tests do not need.  The trunk parameters are rounded to bf16-representable values before the run (the reference then
computes with exactly those fp32 values): the same model for both hot dtypes, and a fixture that compresses below 1 MiB."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
REF = os.environ.get("SR_REFERENCE_ROOT", "")
OUT = os.path.join(ROOT, "tests", "golden", "g17_vsr_trunk64.npz")


def main():
    if not os.path.isfile(os.path.join(REF, "models", "basicvsr_arch_origin.py")):
        sys.exit("set SR_REFERENCE_ROOT to a checkout of the reference")
    sys.path.insert(0, ROOT)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from oracle.make_golden import _mmedit_stubs
    _mmedit_stubs()
    import models.basicvsr_arch_origin as bo

    torch.manual_seed(170)
    m = bo.BasicVSR_origin(num_feat=64, num_block=1, spynet_path=None).eval()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "_trunk." in k:
                p.copy_(p.bfloat16().float())
    g = torch.Generator().manual_seed(171)
    b, n, h, w = 1, 3, 18, 20
    x = torch.rand(b, n, 3, h, w, generator=g)
    ff = torch.rand(b, n - 1, 2, h, w, generator=g) * 4 - 2
    fb = torch.rand(b, n - 1, 2, h, w, generator=g) * 4 - 2
    m.get_flow = lambda x: (ff, fb)                                  # SPyNet is out of scope: flows are given
    feats = {"backward_trunk": [], "forward_trunk": []}
    hooks = [getattr(m, k).register_forward_hook(lambda mod, i, o, k=k: feats[k].append(o.detach().clone())) for k in feats]
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m(x, 4 * h, 4 * w)
    for hk in hooks:
        hk.remove()
    d = {"x": x.numpy(), "flows_forward": ff.numpy(), "flows_backward": fb.numpy(),
         "feat_backward": torch.stack(feats["backward_trunk"], 1).numpy(),      # in call order: frame n-1 .. 0
         "feat_forward": torch.stack(feats["forward_trunk"], 1).numpy()}
    for k, p in m.named_parameters():
        if "_trunk." in k:
            d["p/" + k] = p.detach().numpy().astype(np.float32)
    np.savez_compressed(OUT, **d)
    print("G17 ok", d["feat_forward"].shape, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
