"""The video trainers' loss fold on the MI355X: training.L1Loss / L1_Charbonnier_loss applied to the output of Result_Model (`single`)
and Naive_model (`multi`) on their HIP training routes run sr_fn_net_bwd_loss / sr_mf_net_bwd_loss (csrc/frame_net_bwd.h,
csrc/multi_frame_bwd.h), against tests/video_fold_ref.py and the float64 references of the two networks' backward.

Shapes: the smallest that leave ragged tiles in both directions and cross a clip boundary -- `single` 1 x 2 frames of 9 x 17 (8 x 16 LR
tiles in the upsampler's backward), `multi` 2 x 2 frames of 9 x 33 (8 x 32 in the tail's first stage), given flows, one of which leaves
the image.  Every measured ratio is printed before it is asserted."""
import functools
import math

import pytest
import torch

from tests import frame_net_ref as FR
from tests import frame_net_train_ref as FT
from tests import multi_frame_ref as MR
from tests import multi_frame_train_ref as MT
from tests import video_fold_ref as V
from tests.parity_kit import hold_rounded, rel_max

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("fp32", "bf16")
SINGLE = [("single", c, nb) for c in (8, 32) for nb in (1, 2)]
MULTI = [("multi", c, 2) for c in (8, 32)]
NETS = SINGLE + MULTI
_id = lambda k: "{}-c{}-nb{}".format(*k)


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    import gc
    from mobilesuperresolution_amd import hotpath as HP
    for f in (HP._fn_pack_index, HP._fn_bwd_pack_index, HP._mf_pack_index, HP._mf_bwd_pack_index):
        f.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class Net:
    """one network of the table above: the module on its HIP training route, the reference's view of it, the loss geometry"""

    def __init__(self, key, mode, hot=True):
        self.net, self.c, self.nb = key
        self.mode = mode
        if self.net == "single":
            from mobilesuperresolution_amd.models.single_image_model import Result_Model
            self.case = FR.rounded_case(self.c, self.nb, 2, 9, 17)
            self.h, self.w, self.frames = 9, 17, 2
            m = Result_Model(4, self.c, self.nb, 3, hot_dtype=mode)
            m.load_state_dict(FR.state_dict_of(self.case["p"]), strict=False)
            self.x = self.case["x"].float().unsqueeze(0)
            self.flows = None
            self.tile, self.adds = (8, 16), 3 * 16 * 128 // 256
        else:
            from mobilesuperresolution_amd.models.naive_multi_model_easy import Naive_model
            self.case = MR.rounded_case(self.c, self.nb, 2, 2, 9, 33)
            self.h, self.w, self.frames = 9, 33, 4
            m = Naive_model(4, status=[[self.c, self.c, 3]] * self.nb, hot_dtype=mode)
            m.load_state_dict(MR.state_dict_of(self.case["p"]), strict=False)
            self.x = self.case["x"].float()
            self.flows = _flows_with_one_leaving(self.case["flows"])
            fl = self.flows.float().to(DEV)
            m.get_flow = lambda x_: fl
            self.tile, self.adds = (8, 32), 48
        m.hot_training = hot
        self.m = m.to(DEV)

    def forward(self):
        x = self.x.to(DEV)
        y = self.m(x, 4 * self.h, 4 * self.w) if self.net == "single" else self.m(x)
        return y

    def loss_geometry(self):
        """(tiles the loss stage walks, its workgroups)"""
        from mobilesuperresolution_amd import hotpath as HP
        items = self.frames * math.ceil(self.h / self.tile[0]) * math.ceil(self.w / self.tile[1])
        return items, min(items, HP.fn_bwd_wgs(self.frames, self.h, self.w))

    def sd(self):
        return {k: v.detach().cpu() for k, v in self.m.state_dict().items() if not k.startswith("flownet.")}

    def ref_grads(self, gout, rnd=None):
        """float64 parameter gradients of the reference's backward from the output gradient gout (frames, 3, 4h, 4w)"""
        sd = self.sd()
        if self.net == "single":
            p = FR.effective(sd, self.nb)
            return FT.param_grads(sd, self.nb, FT.backward(self.x[0], p, gout, rnd=rnd)["grads"])
        p = MR.effective(sd, self.nb)
        return MT.param_grads(sd, self.nb, MT.backward(self.x, self.flows.float(), p, gout, rnd=rnd)["grads"])

    def grads(self):
        return {k: (p.grad.detach().double().cpu() if p.grad is not None else None) for k, p in self.m.named_parameters()}

    def trained(self):
        skip = lambda k: k.startswith("flownet.") or k.startswith("skip.") or ".skip." in k
        return [(k, p) for k, p in self.m.named_parameters() if not skip(k)]


def _flows_with_one_leaving(flows):
    fl = flows.clone()                                   # the cached case stays as it is
    fl[0, 0, 0, 2, 3] = 50.0                             # leaves the 33-wide image to the right
    fl[1, 0, 1, 8, 32] = -40.0                           # and the 9-high one upwards, from the ragged corner
    return fl


@functools.lru_cache(maxsize=None)
def _hr(frames, h, w):
    return torch.rand(frames, 3, 4 * h, 4 * w, generator=torch.Generator().manual_seed(77))


def _criterion(kind):
    from mobilesuperresolution_amd import training as TR
    return TR.L1Loss() if kind == "l1" else TR.L1_Charbonnier_loss()


def _backward_with(net, gout):
    """parameter gradients of the UNFOLDED route from an explicit output gradient (frames, 3, 4h, 4w) on the device"""
    net.m.zero_grad()
    y = net.forward()
    (y.view(gout.shape) * gout).sum().backward()
    return net.grads()


def test_the_new_symbols_exist_under_abi_25():
    from mobilesuperresolution_amd import _lib as L
    assert all(hasattr(L.lib(), s) for s in ("sr_fn_net_bwd_loss", "sr_mf_net_bwd_loss", "sr_adam_step_multi"))
    assert L.lib().sr_abi_version() == 25


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", NETS, ids=_id)
def test_folded_loss_value_gradients_and_timing(key, mode, kind):
    net = Net(key, mode)
    hr = _hr(net.frames, net.h, net.w)
    y = net.forward()
    assert net.m.last_route == "hip_train"
    loss = _criterion(kind)(y, hr.view(y.shape).to(DEV))
    # 7: the criterion folded; 5: no parameter gradient yet
    assert type(loss.grad_fn).__name__ == "_FoldedCriterionBackward"
    assert all(p.grad is None for _, p in net.m.named_parameters())
    loss.backward()
    trained = net.trained()
    assert trained and all(p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32 for _, p in trained)
    got = net.grads()
    # 1: the loss value against the float64 mean over the same sr
    sr = y.detach().cpu().view(hr.shape)
    want = V.loss_value(sr, hr, kind).item()
    items, wgs = net.loss_geometry()
    tol = V.chain_length(kind, items, wgs, net.adds) * 2.0 ** -24
    err = abs(loss.item() - want) / want
    print(f"video fold | {_id(key)} {mode} {kind} | loss {loss.item():.8f} float64 {want:.8f} | rel err {err:.2e} | bound {tol:.2e}")
    assert err <= tol
    # 2: parameter gradients against the float64 reference fed the float64 loss gradient of the same sr
    gout = V.loss_grad(sr, hr, kind)
    ref = net.ref_grads(gout)
    gdev = gout.float().to(DEV)
    if mode == "fp32":
        tf32 = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
        torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
        try:
            yard = _backward_with(Net(key, mode, hot=False), gdev)
        finally:
            torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = tf32
    else:
        rnd = FR.bf16_round if net.net == "single" else MR.bf16_round
        yard = net.ref_grads(gout, rnd=rnd)
    yards = {k: rel_max(yard[k], ref[k]) for k in ref}
    hold_rounded("video fold", f"{_id(key)} {kind}", mode, [(k, got[k], ref[k], yards[k]) for k in ref])
    # 6: the unfolded entry point, its g from the kernels' formula as one fp32 torch expression, agrees within the same bound
    g32 = V.kernel_formula_fp32(y.detach().view(hr.shape), hr.to(DEV), kind)
    unfolded = _backward_with(net, g32)
    assert net.m.last_route == "hip_train"
    hold_rounded("video fold vs unfolded", f"{_id(key)} {kind}", mode, [(k, got[k], unfolded[k], yards[k]) for k in ref])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", [("single", 32, 1), ("multi", 32, 2)], ids=_id)
def test_every_hr_pixel_is_counted_once(key, mode):
    """sr == hr except at ONE HR pixel on a corner that four tiles of the loss stage share: L1 = |d| / n; counting the pixel in every
    tile that reads it would give 2 x or 4 x"""
    net = Net(key, mode)
    y = net.forward()
    hr = y.detach().clone()
    py, px = 4 * net.tile[0], 4 * net.tile[1]                            # first HR pixel of the tile diagonal to tile (0, 0)
    assert py < 4 * net.h and px < 4 * net.w
    flat = hr.view(net.frames, 3, 4 * net.h, 4 * net.w)
    flat[net.frames - 1, 1, py, px] += 0.5
    loss = _criterion("l1")(y, hr)
    assert type(loss.grad_fn).__name__ == "_FoldedCriterionBackward"
    want = (y.detach().double() - hr.double()).abs().sum().item() / y.numel()
    err = abs(loss.item() - want) / want
    print(f"video fold | {_id(key)} {mode} | one pixel: loss {loss.item():.6e} expected {want:.6e} | rel err {err:.2e}")
    assert want > 0 and err <= 3 * 2.0 ** -24                            # d, the sum of zeros and one value, the scale


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", [("single", 8, 2), ("multi", 8, 2)], ids=_id)
def test_loss_weight_scales_the_gradients_exactly(key, mode):
    net = Net(key, mode)
    hr = _hr(net.frames, net.h, net.w).to(DEV)
    crit = _criterion("charbonnier")

    def run(weight):
        net.m.zero_grad()
        y = net.forward()
        loss = crit(y, hr.view(y.shape))
        assert type(loss.grad_fn).__name__ == "_FoldedCriterionBackward"
        (loss if weight is None else weight * loss).backward()
        return {k: p.grad.detach().clone() for k, p in net.trained()}

    plain, quarter = run(None), run(0.25)
    assert plain and all(torch.equal(quarter[k], 0.25 * plain[k]) for k in plain)
    assert any(bool(v.abs().max() > 0) for v in plain.values())


@pytest.mark.parametrize("key", [("single", 8, 1), ("multi", 8, 2)], ids=_id)
def test_what_can_fold_refuses_keeps_torch_ops(key):
    net = Net(key, "fp32")
    hr = _hr(net.frames, net.h, net.w).to(DEV)
    crit = _criterion("l1")
    y = net.forward()
    folded = lambda t: type(t.grad_fn).__name__ == "_FoldedCriterionBackward"
    assert not folded(crit(y, hr.view(y.shape).double()))                # hr not fp32
    assert not folded(crit(y[:, :1], hr.view(y.shape)[:, :1]))           # a slice of the output
    with torch.no_grad():
        assert not folded(crit(y, hr.view(y.shape)))                     # grad mode off
    first = crit(y, hr.view(y.shape))
    assert folded(first)
    assert not folded(crit(y, hr.view(y.shape)))                         # the node is folded already
    first.backward()
    assert all(p.grad is not None for _, p in net.trained())
    y2 = net.forward()
    torch.nn.functional.l1_loss(y2, hr.view(y2.shape)).backward()
    assert not folded(crit(y2, hr.view(y2.shape)))                       # the node's backward has run
