#!/usr/bin/env python3
"""Write fixture G22 (tests/golden/g22_multi_frame.npz) by running the REFERENCE's multi-frame video network on the CPU:

    SR_REFERENCE_ROOT=<reference checkout> python tools/make_golden_multi_frame.py

models/naive_multi_model_easy.py is loaded from the reference by path.  What its imports name and the network never uses
(tensorboard, torchvision.utils, the reference's common / utils / models / loss_config packages, mmedit) is stubbed in sys.modules;
mmedit's flow_warp is the reference's vendored one (models/spynet_arch.py, loaded by path), and mmedit's SPyNet is a parameter-free
stub that returns the fixture's flows.  The reference moves its zero flow of frame 0 `.to('cuda')`: while a model runs, Tensor.to
ignores that one argument.  For a one-frame clip the reference takes `zeros_like(flows[:, 0])` of an empty flow tensor; the stub's
result then answers `.view(B, 0, 2, H, W)` with one zero flow so that the line runs (the flow is zero either way).

Three models built under torch.manual_seed(seed) from a status file of `blocks` lines [C, C, 3]:

    a   C = 32, 3 blocks, clip (2, 3)      b   C = 20, 1 block, clip (2, 3)      c   C = 32, 2 blocks, clip (1, 1)

all on 12 x 20 frames, flows uniform in +-3 px.  Per model `tag`:

    tag/keys, tag/shape/<key>  the state_dict's keys in order and their shapes
    tag/sha256/<key>           SHA-256 of the tensor as initialised (fp32, C order)
    tag/x, tag/flows           the clip (B, N, 3, 12, 20) and the flows (B, N - 1, 2, 12, 20)
    tag/stride                 1 or 3: `y` and `g/<key>` hold every stride-th element of the flattened tensor
    tag/y                      forward(x), (B, N, 3, 48, 80)
    tag/g/<key>                the gradient of every parameter for forward(x).sum() (zeros where the reference leaves none)
    tag/p/<key>                the state_dict as initialised -- model b only

Random fp32 data does not compress, and the three models' parameters, gradients and outputs are 2 MB: more than a fixture may take.
So the small model b is held in full, and a and c hold the digest of every initial tensor (a seeded build must reproduce it bit for
bit; the tests then take the parameters from that build) and every third element of y and of each gradient (3 is coprime to the
image sizes, the shuffle phases and the 9 taps, so every phase and tap is sampled).
"""
import contextlib
import hashlib
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__ + "/.."))
REF = os.environ.get("SR_REFERENCE_ROOT", "")
OUT = os.path.join(ROOT, "tests", "golden", "g22_multi_frame.npz")

MODELS = {"a": dict(c=32, blocks=3, clip=(2, 3), seed=220, stride=3), "b": dict(c=20, blocks=1, clip=(2, 3), seed=221, stride=1),
          "c": dict(c=32, blocks=2, clip=(1, 1), seed=222, stride=3)}
H, W = 12, 20


def _force_stub(name, **attrs):
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        nm = ".".join(parts[:i])
        if nm not in sys.modules:
            sys.modules[nm] = types.ModuleType(nm)
            if i > 1:
                setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], sys.modules[nm])
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def _stub(name, **attrs):
    try:
        importlib.import_module(name)
    except ImportError:
        _force_stub(name, **attrs)


def _by_path(name, *rel):
    path = os.path.join(REF, *rel)
    if not os.path.isfile(path):
        sys.exit("set SR_REFERENCE_ROOT to a checkout of the reference")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Flows:
    """what the stub returns: the flows, reshaped as the reference asks (see the module docstring for the one-frame clip)"""

    def __init__(self, t):
        self.t = t

    def view(self, b, n1, c, h, w):
        return self.t.view(b, n1, c, h, w) if n1 else torch.zeros(b, 1, c, h, w)


class StubSPyNet(torch.nn.Module):
    flows = None

    def __init__(self, pretrained=None):
        super().__init__()

    def forward(self, ref, supp):
        return _Flows(StubSPyNet.flows.reshape(-1, 2, *StubSPyNet.flows.shape[-2:]))


def load_reference():
    warp = _by_path("ref_spynet_arch", "models", "spynet_arch.py").flow_warp
    _stub("torch.utils.tensorboard", SummaryWriter=object)
    _stub("torchvision.utils", save_image=lambda *a, **k: None)
    for name, attrs in (("common.meters", {}), ("common.modes", {}), ("common.metrics", {}), ("utils.estimate", dict(test=None)),
                        ("utils", dict(logging_tool=None, attr_extractor=None, loss_printer=None)), ("models", {}),
                        ("loss_config", dict(update_weight=None)),
                        ("mmedit.models.backbones.sr_backbones.basicvsr_net", dict(ResidualBlocksWithInputConv=None, SPyNet=StubSPyNet)),
                        ("mmedit.models.common", dict(PixelShufflePack=None, flow_warp=warp))):
        _force_stub(name, **attrs)
    return _by_path("ref_naive_multi_model_easy", "models", "naive_multi_model_easy.py")


@contextlib.contextmanager
def cuda_moves_ignored():
    real = torch.Tensor.to

    def to(self, *args, **kwargs):
        args = tuple(a for a in args if not (isinstance(a, str) and a.startswith("cuda")))
        return real(self, *args, **kwargs) if args or kwargs else self

    torch.Tensor.to = to
    try:
        yield
    finally:
        torch.Tensor.to = real


def main():
    ref = load_reference()
    d = {}
    for tag, cfg in MODELS.items():
        status = [[cfg["c"], cfg["c"], 3] for _ in range(cfg["blocks"])]
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write("header\n" + repr([0, status]) + "\n")
        torch.manual_seed(cfg["seed"])
        m = ref.Naive_model(4, f.name)
        os.unlink(f.name)
        sd = m.state_dict()
        stride = cfg["stride"]
        d[f"{tag}/keys"] = np.array(list(sd.keys()))
        d[f"{tag}/status"] = np.array(status, dtype=np.int64)
        d[f"{tag}/seed"] = np.array(cfg["seed"], dtype=np.int64)
        d[f"{tag}/stride"] = np.array(stride, dtype=np.int64)
        for k, v in sd.items():
            a = np.ascontiguousarray(v.detach().numpy().astype(np.float32))
            d[f"{tag}/shape/{k}"] = np.array(a.shape, dtype=np.int64)
            d[f"{tag}/sha256/{k}"] = np.array(hashlib.sha256(a.tobytes()).hexdigest())
            if stride == 1:
                d[f"{tag}/p/{k}"] = a
        b, n = cfg["clip"]
        g = torch.Generator().manual_seed(cfg["seed"] + 100)
        x = torch.rand(b, n, 3, H, W, generator=g)
        flows = 6.0 * torch.rand(b, n - 1, 2, H, W, generator=g) - 3.0
        StubSPyNet.flows = flows
        d[f"{tag}/x"], d[f"{tag}/flows"] = x.numpy(), flows.numpy()
        m.zero_grad()
        with cuda_moves_ignored():
            y = m(x)
            y.sum().backward()
        d[f"{tag}/y"] = y.detach().numpy().reshape(-1)[::stride].copy() if stride > 1 else y.detach().numpy()
        none = []
        for k, p in m.named_parameters():
            if p.grad is None:
                none.append(k)
            gk = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
            d[f"{tag}/g/{k}"] = gk.reshape(-1)[::stride].copy() if stride > 1 else gk.copy()
        d[f"{tag}/gradless"] = np.array(none)
        print(tag, "keys", len(sd), "params", sum(v.numel() for v in sd.values()), "without a gradient:", none)
    np.savez_compressed(OUT, **d)
    print("G22 ok", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
