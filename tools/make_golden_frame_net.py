#!/usr/bin/env python3
"""Write fixture G21 (tests/golden/g21_single_frame.npz) by running the REFERENCE's per-frame video network on the CPU:

    SR_REFERENCE_ROOT=<reference checkout> python tools/make_golden_frame_net.py

models/single_image_model.py is loaded from the reference by path, with the packages its imports name and the network never uses
(torch.utils.tensorboard, torchvision.utils) stubbed in sys.modules where they are not installed.  Two models,
`Result_Model(4, 32, 2, 3)` and `Result_Model(4, 20, 1, 3)`, each built under torch.manual_seed(seed).  Per model `tag`:

    tag/p/<key>        the state_dict as initialised (key order = the reference's)
    tag/keys           the keys, in order
    tag/x              a (1, 2, 3, 12, 20) clip
    tag/y48x80         forward(x, 48, 80)    (the x4 size)
    tag/y50x77         forward(x, 50, 77)
    tag/g/<key>        the gradient of every parameter for forward(x, 48, 80).sum()
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
REF = os.environ.get("SR_REFERENCE_ROOT", "")
OUT = os.path.join(ROOT, "tests", "golden", "g21_single_frame.npz")

MODELS = {"a": dict(args=(4, 32, 2, 3), seed=210), "b": dict(args=(4, 20, 1, 3), seed=211)}
SIZES = ((48, 80), (50, 77))


def _stub(name, **attrs):
    try:
        importlib.import_module(name)
        return
    except ImportError:
        pass
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        nm = ".".join(parts[:i])
        if nm not in sys.modules:
            sys.modules[nm] = types.ModuleType(nm)
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def load_reference():
    path = os.path.join(REF, "models", "single_image_model.py")
    if not os.path.isfile(path):
        sys.exit("set SR_REFERENCE_ROOT to a checkout of the reference")
    _stub("torch.utils.tensorboard", SummaryWriter=object)
    _stub("torchvision.utils", save_image=lambda *a, **k: None)
    spec = importlib.util.spec_from_file_location("ref_single_image_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    d = {}
    for tag, cfg in MODELS.items():
        torch.manual_seed(cfg["seed"])
        m = ref.Result_Model(*cfg["args"])
        sd = m.state_dict()
        d[f"{tag}/keys"] = np.array(list(sd.keys()))
        d[f"{tag}/args"] = np.array(cfg["args"], dtype=np.int64)
        for k, v in sd.items():
            d[f"{tag}/p/{k}"] = v.detach().numpy().copy()
        x = torch.rand(1, 2, 3, 12, 20, generator=torch.Generator().manual_seed(cfg["seed"] + 100))
        d[f"{tag}/x"] = x.numpy()
        for hh, ww in SIZES:
            m.zero_grad()
            y = m(x, hh, ww)
            d[f"{tag}/y{hh}x{ww}"] = y.detach().numpy()
            if (hh, ww) == SIZES[0]:
                y.sum().backward()
                for k, p in m.named_parameters():
                    d[f"{tag}/g/{k}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
        print(tag, "keys", len(sd), "params", sum(v.numel() for v in sd.values()))
    np.savez_compressed(OUT, **d)
    print("G21 ok", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
