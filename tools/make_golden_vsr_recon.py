#!/usr/bin/env python3
"""Write fixture G19 (tests/golden/g19_vsr_recon.npz) by running the REFERENCE's BasicVSR_origin end to end on the CPU:

    SR_REFERENCE_ROOT=<reference checkout> python tools/make_golden_vsr_recon.py

models/basicvsr_arch_origin.py is imported from the reference with mmedit stubbed (oracle/make_golden.py's `_mmedit_stubs`), as
tools/make_golden_vsr64.py does.  Two models run in eval mode under torch.no_grad() on G17's frames (1 clip x 3 frames of 18 x 20)
with G17's GIVEN flows (`get_flow` overridden) and `forward(x, 4h, 4w)`:

  * BasicVSR_origin(64, 1) with G17's trunk parameters loaded, so that G17 and G19 describe ONE model; its five reconstruction
    layers are seeded here and rounded to bf16-representable values with five explicit mantissa bits (exact in both hot dtypes;
    the two bits bf16 could hold beyond that are what keeps the compressed fixture below 1 MiB).  Stored: the reconstruction
    parameters as uint16 bf16 bit patterns (`q/<key>`: exact, and half the bytes of fp32) and the output `out64` (1, 3, 3, 72, 80).
  * BasicVSR_origin(24, 1), every trunk and reconstruction parameter seeded and rounded the same way.  Stored: all of them
    (`q24/<key>`) and `out24`.

Frames, flows and the 64-feature trunks are NOT repeated here: the tests read them from G17."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
REF = os.environ.get("SR_REFERENCE_ROOT", "")
G17 = os.path.join(ROOT, "tests", "golden", "g17_vsr_trunk64.npz")
OUT = os.path.join(ROOT, "tests", "golden", "g19_vsr_recon.npz")
RECON = ("fusion.", "upconv1.", "upconv2.", "conv_hr.", "conv_last.")


def _round5(p):
    """fp32 -> the nearest value with five explicit mantissa bits (a bf16-representable fp32)"""
    v = p.detach().contiguous().view(torch.int32)
    return ((v + (1 << 17)) & ~((1 << 18) - 1)).view(torch.float32)


def _bits(p):
    """bf16-representable fp32 -> uint16 bit pattern"""
    return (p.detach().contiguous().view(torch.int32) >> 16).to(torch.int16).numpy().view(np.uint16)


def main():
    if not os.path.isfile(os.path.join(REF, "models", "basicvsr_arch_origin.py")):
        sys.exit("set SR_REFERENCE_ROOT to a checkout of the reference")
    sys.path.insert(0, ROOT)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from oracle.make_golden import _mmedit_stubs
    _mmedit_stubs()
    import models.basicvsr_arch_origin as bo

    g17 = np.load(G17)
    x, ff, fb = (torch.from_numpy(g17[k]) for k in ("x", "flows_forward", "flows_backward"))
    h, w = x.shape[-2:]
    d = {}

    def run(m):
        m.get_flow = lambda x: (ff, fb)                              # SPyNet is out of scope: flows are given
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return m(x, 4 * h, 4 * w).numpy()

    torch.manual_seed(190)
    m = bo.BasicVSR_origin(num_feat=64, num_block=1, spynet_path=None).eval()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "_trunk." in k:
                p.copy_(torch.from_numpy(g17["p/" + k]))
            elif k.startswith(RECON):
                p.copy_(_round5(p))
                d["q/" + k] = _bits(p)
    d["out64"] = run(m)

    torch.manual_seed(191)
    m = bo.BasicVSR_origin(num_feat=24, num_block=1, spynet_path=None).eval()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "_trunk." in k or k.startswith(RECON):
                p.copy_(_round5(p))
                d["q24/" + k] = _bits(p)
    d["out24"] = run(m)
    np.savez_compressed(OUT, **d)
    size = os.path.getsize(OUT)
    print("G19 ok", d["out64"].shape, d["out24"].shape, size, "bytes")
    assert size < 2 ** 20, "G19 must stay below 1 MiB"


if __name__ == "__main__":
    main()
