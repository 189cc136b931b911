#!/usr/bin/env python3
"""Write fixture G18 (tests/golden/g18_result_model.npz) by running the REFERENCE's stage-3 network on the CPU:

    SR_REFERENCE_ROOT=<reference checkout> python tools/make_golden_result_model.py

pretrain_simplified_model.py is imported from the reference with the packages its trainer code needs but the network does
not (tensorboard, torchvision, mmedit, skimage, h5py, cv2) stubbed in sys.modules.  `Result_Model(scale, filename)` is built
from a block_index.txt written here, for two architectures:

    a: IN = 27 (F = 32), scale 2, [[27,16,3],[27,27,5],[27,9,7]]   7x7 tail, partial and full splits
    b: IN = 20 (F = 24), scale 4, [[20,20,3],[20,12,5],[20,8,3]]   3x3 tail

Per architecture: the parameters (rounded to bf16-representable values first, as G17), x (odd H and W), hr, the output,
the L1 loss and the gradient of every state_dict tensor (one backward of nn.L1Loss).  `init/<key>` holds the parameters as
the reference initialises them under torch.manual_seed(seed) (before rounding)."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
REF = os.environ.get("SR_REFERENCE_ROOT", "")
OUT = os.path.join(ROOT, "tests", "golden", "g18_result_model.npz")

ARCHS = {
    "a": dict(scale=2, status=[[27, 16, 3], [27, 27, 5], [27, 9, 7]], seed=180, n=2, h=13, w=11),
    "b": dict(scale=4, status=[[20, 20, 3], [20, 12, 5], [20, 8, 3]], seed=181, n=2, h=9, w=15),
}


class _AnyAttr(types.ModuleType):
    def __getattr__(self, name):
        return None


def _stub(name, **attrs):
    m = sys.modules.get(name) or _AnyAttr(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _stubs():
    import importlib.util
    missing = {name for name in ("torchvision", "mmedit", "skimage", "h5py", "cv2") if importlib.util.find_spec(name) is None}
    _stub("torch.utils.tensorboard", SummaryWriter=object)
    for name in missing:
        _stub(name)
    if "torchvision" in missing:
        _stub("torchvision.utils", save_image=lambda *a, **k: None)
        sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    if "mmedit" in missing:
        _stub("mmedit.core")
        _stub("mmedit.core.evaluation")
        _stub("mmedit.core.evaluation.metrics", psnr=None, ssim=None)
    if "skimage" in missing:
        for sub in ("skimage.metrics", "skimage.measure", "skimage.color", "skimage.io", "skimage.transform"):
            _stub(sub)


def main():
    if not os.path.isfile(os.path.join(REF, "pretrain_simplified_model.py")):
        sys.exit("set SR_REFERENCE_ROOT to a checkout of the reference")
    if REF not in sys.path:
        sys.path.insert(0, REF)
    _stubs()
    import importlib
    while True:                                    # stub whatever else the trainer's imports want and this machine lacks
        try:
            psm = importlib.import_module("pretrain_simplified_model")
            break
        except ModuleNotFoundError as e:
            parts = e.name.split(".")
            for i in range(1, len(parts) + 1):
                nm = ".".join(parts[:i])
                if nm not in sys.modules:
                    sys.modules[nm] = _AnyAttr(nm)
    d = {}
    for tag, a in ARCHS.items():
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("([0], [[0, 0, 3]])\n")                          # only the last line counts
            f.write(repr(([1, 2, 4], a["status"])) + "\n")
            fname = f.name
        torch.manual_seed(a["seed"])
        m = psm.Result_Model(a["scale"], fname)
        os.unlink(fname)
        for k, v in m.state_dict().items():
            d[f"{tag}/init/{k}"] = v.numpy().astype(np.float32)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(p.bfloat16().float())
        g = torch.Generator().manual_seed(a["seed"] + 100)
        n, h, w, s = a["n"], a["h"], a["w"], a["scale"]
        x = torch.rand(n, 3, h, w, generator=g)
        hr = torch.rand(n, 3, s * h, s * w, generator=g)
        m.zero_grad()
        y = m(x)
        loss = torch.nn.L1Loss()(y, hr)
        loss.backward()
        d[f"{tag}/x"], d[f"{tag}/hr"], d[f"{tag}/y"] = x.numpy(), hr.numpy(), y.detach().numpy()
        d[f"{tag}/loss"] = np.float32(loss.item())
        d[f"{tag}/status"] = np.array(a["status"], dtype=np.int64)
        d[f"{tag}/scale"] = np.int64(s)
        for k, p in m.named_parameters():
            d[f"{tag}/p/{k}"] = p.detach().numpy().astype(np.float32)
            d[f"{tag}/g/{k}"] = p.grad.numpy().astype(np.float32)
        print(tag, "keys", len(m.state_dict()), "out", tuple(y.shape), "loss", loss.item())
    np.savez_compressed(OUT, **d)
    print("G18 ok", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
