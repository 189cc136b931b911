"""The video networks' one-call training step on the MI355X: Result_Model.train_step / Naive_model.train_step (sr_fn_net_train_step /
sr_mf_net_train_step, csrc/clip_param_step.h) against the float64 references of the two networks' backward carried through
tests/clip_step_ref.py's weight-norm backward, against torch.optim.Adam, and against the ordinary loop.

Shapes: those of tests/test_gpu_video_fold.py -- `single` 1 x 2 frames of 9 x 17, `multi` 2 x 2 frames of 9 x 33 with given flows of which
two leave the image.

How the gradient of a step is read: the call writes no gradient, so a first step from a fresh training.Adam with beta1 = 0 is taken;
then exp_avg = fma(1, g - 0, 0) = g, the fp32 gradient the step used, bit for bit (exp_avg / (1 - beta1) with beta1 = 0).  The kernels
have no atomics and a fixed summation order, so a second fresh model with the same state_dict takes the same gradient: that run, with
the reference's hyper-parameters, is the one compared with torch.optim.Adam fed those gradients.  Every measured ratio is printed
before it is asserted."""
import copy
import functools
import math

import pytest
import torch

from tests import clip_step_ref as S
from tests import frame_net_ref as FR
from tests import frame_net_train_ref as FT
from tests import multi_frame_ref as MR
from tests import multi_frame_train_ref as MT
from tests import video_fold_ref as V
from tests.parity_kit import bound, rel_max

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
    _first_step.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _flows_with_two_leaving(flows):
    fl = flows.clone()
    fl[0, 0, 0, 2, 3] = 50.0                             # leaves the 33-wide image to the right
    fl[1, 0, 1, 8, 32] = -40.0                           # and the 9-high one upwards, from the ragged corner
    return fl


class Net:
    """one network of the table above on the device, the reference's view of it, the loss geometry"""

    def __init__(self, key, mode, state=None):
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
            self.flows = _flows_with_two_leaving(self.case["flows"])
            fl = self.flows.float().to(DEV)
            m.get_flow = lambda x_: fl
            self.tile, self.adds = (8, 32), 48
        if state is not None:
            m.load_state_dict(state, strict=False)
        self.m = m.to(DEV)
        self.xd = self.x.to(DEV)
        self.hr = _hr(self.frames, self.h, self.w).view(self.x.shape[0], self.x.shape[1], 3, 4 * self.h, 4 * self.w)
        self.hrd = self.hr.to(DEV)

    def trained(self):
        skip = lambda k: k.startswith("flownet.") or k.startswith("skip.") or ".skip." in k
        return [(k, p) for k, p in self.m.named_parameters() if not skip(k)]

    def untouched(self):
        names = {k for k, _ in self.trained()}
        return [(k, p) for k, p in self.m.named_parameters() if k not in names]

    def adam(self, **kw):
        from mobilesuperresolution_amd import training as TR
        return TR.Adam([p for _, p in self.trained()], **kw)

    def step(self, opt, kind="charbonnier", **kw):
        if kw.pop("give_flows", False) and self.net == "multi":
            kw["flows"] = self.flows.float().to(DEV)
        return self.m.train_step(self.xd, self.hrd, opt, criterion=kind, **kw)

    def sd(self):
        return {k: v.detach().cpu().clone() for k, v in self.m.state_dict().items() if not k.startswith("flownet.")}

    def loss_geometry(self):
        from mobilesuperresolution_amd import hotpath as HP
        items = self.frames * math.ceil(self.h / self.tile[0]) * math.ceil(self.w / self.tile[1])
        return items, min(items, HP.fn_bwd_wgs(self.frames, self.h, self.w))

    def ref_grads(self, sd, gout, rnd=None):
        """float64 parameter gradients from the output gradient gout (frames, 3, 4h, 4w), through clip_step_ref's weight-norm backward"""
        if self.net == "single":
            p = FR.effective(sd, self.nb)
            return S.single_param_grads(sd, self.nb, FT.backward(self.x[0], p, gout, rnd=rnd)["grads"])
        p = MR.effective(sd, self.nb)
        return S.multi_param_grads(sd, self.nb, MT.backward(self.x, self.flows.float(), p, gout, rnd=rnd)["grads"])

    def aten_grads(self, sd, gout):
        """the fp32 yardstick of sections 16 / 17: the ATen route's backward (TF32 off) from the same output gradient"""
        other = Net((self.net, self.c, self.nb), self.mode, state=sd)
        tf32 = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
        torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
        try:
            y = other.m(other.xd, 4 * self.h, 4 * self.w) if self.net == "single" else other.m(other.xd)
            assert other.m.last_route == "aten"
            (y.view(gout.shape) * gout.float().to(DEV)).sum().backward()
        finally:
            torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = tf32
        return {k: p.grad.detach().double().cpu() for k, p in other.trained()}


@functools.lru_cache(maxsize=None)
def _hr(frames, h, w):
    return torch.rand(frames, 3, 4 * h, 4 * w, generator=torch.Generator().manual_seed(77))


@functools.lru_cache(maxsize=None)
def _first_step(key, mode, kind, loss_weight=1.0):
    """one step with beta1 = 0 from a fresh model and optimizer: (state_dict before, sr, loss, {name: the gradient the step used})"""
    net = Net(key, mode)
    sd0 = net.sd()
    opt = net.adam(lr=1e-4, betas=(0.0, 0.999))
    sr = torch.full_like(net.hrd, float("nan"))
    loss = net.step(opt, kind, loss_weight=loss_weight, sr_out=sr)
    grads = {k: opt.state[p]["exp_avg"].detach().clone() for k, p in net.trained()}
    return sd0, sr.cpu().view(net.frames, 3, 4 * net.h, 4 * net.w), loss.detach().cpu(), grads


def test_the_new_symbols_exist_under_abi_25():
    from mobilesuperresolution_amd import _lib as L
    assert all(hasattr(L.lib(), s) for s in ("sr_fn_net_train_step", "sr_mf_net_train_step")) and L.lib().sr_abi_version() == 25


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", NETS, ids=_id)
def test_gradients_reach_the_optimizer_and_the_loss_value(key, mode, kind):
    sd0, sr, loss, grads = _first_step(key, mode, kind)
    net = Net(key, mode)
    hr = _hr(net.frames, net.h, net.w)
    assert not bool(torch.isnan(sr).any())
    # 3: the loss value against the float64 mean over the same sr
    want = V.loss_value(sr, hr, kind).item()
    items, wgs = net.loss_geometry()
    tol = V.chain_length(kind, items, wgs, net.adds) * 2.0 ** -24
    err = abs(loss.item() - want) / want
    print(f"clip step | {_id(key)} {mode} {kind} | loss {loss.item():.8f} float64 {want:.8f} | rel err {err:.2e} | bound {tol:.2e}")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and err <= tol
    # 1: the gradients the step used against the float64 references fed the float64 loss gradient of the same sr
    gout = V.loss_grad(sr, hr, kind)
    ref = net.ref_grads(sd0, gout)
    assert set(ref) == set(grads)
    if mode == "fp32":
        yard = net.aten_grads(sd0, gout)
    else:
        yard = net.ref_grads(sd0, gout, rnd=FR.bf16_round if net.net == "single" else MR.bf16_round)
    bad = []
    for k in ref:
        e_ref = rel_max(yard[k], ref[k])
        row = S.row_len_of(k, sd0)
        if row is not None:                              # weight_g / weight_v: the yardstick widened by the row's fp32 chain
            e_ref += S.wn_chain_length(row) * 2.0 ** -24
        e, tol = rel_max(grads[k].double().cpu(), ref[k]), bound(mode, e_ref)
        print(f"clip step | {_id(key)} {mode} {kind} | {k} | yardstick {e_ref:.2e} | kernel {e:.2e} | ratio {e / e_ref:.2f} | bound {tol:.2e}")
        if not e <= tol:
            bad.append((k, e, tol))
    assert not bad, bad
    assert any(bool(g.abs().max() > 0) for g in grads.values())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", NETS, ids=_id)
def test_adam_arithmetic_is_torchs(key, mode):
    sd0, _, loss0, grads = _first_step(key, mode, "charbonnier")
    net = Net(key, mode, state=sd0)
    opt = net.adam(lr=1e-3)                               # the reference's hyper-parameters: betas (0.9, 0.999), eps 1e-8
    loss = net.step(opt)
    assert torch.equal(loss.cpu(), loss0)
    twins = {k: torch.nn.Parameter(sd0[k].to(DEV).clone()) for k, _ in net.trained()}
    ref = torch.optim.Adam(list(twins.values()), lr=1e-3)
    for k, p in twins.items():
        p.grad = grads[k].clone()
    ref.step()
    bad = []
    for k, p in net.trained():
        st, rt = opt.state[p], ref.state[twins[k]]
        for what, a, b in (("param", p.detach(), twins[k].detach()), ("exp_avg", st["exp_avg"], rt["exp_avg"]),
                           ("exp_avg_sq", st["exp_avg_sq"], rt["exp_avg_sq"])):
            if not torch.equal(a, b):
                bad.append((k, what, (a - b).abs().max().item()))
        assert float(st["step"]) == 1.0 and not st["step"].is_cuda
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
    assert not bad, bad[:8]
    assert any(not torch.equal(p.detach().cpu(), sd0[k]) for k, p in net.trained())


def _ordinary_step(net, opt):
    from mobilesuperresolution_amd import training as TR
    net.m.hot_training = True
    opt.zero_grad()
    y = net.m(net.xd, 4 * net.h, 4 * net.w) if net.net == "single" else net.m(net.xd)
    assert net.m.last_route == "hip_train"
    loss = TR.L1_Charbonnier_loss()(y, net.hrd)
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", [("single", 8, 2), ("multi", 8, 2)], ids=_id)
def test_three_steps_then_interchange_and_determinism(key, mode):
    def three():
        net = Net(key, mode)
        opt = net.adam(lr=1e-3)
        losses = [net.step(opt, give_flows=True).clone() for _ in range(3)]
        return net, opt, losses

    a, opt_a, la = three()
    b, _, lb = three()
    # 5: determinism
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert all(torch.equal(p, q) for (_, p), (_, q) in zip(a.trained(), b.trained()))
    assert all(math.isfinite(v.item()) for v in la) and la[2].item() != la[0].item()
    # 4: checkpoint after three train_step calls, one step of the ordinary loop from it
    c = Net(key, mode, state=a.sd())
    opt_c = c.adam(lr=1e-3)
    opt_c.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    assert math.isfinite(_ordinary_step(c, opt_c).item())
    assert all(float(opt_c.state[p]["step"]) == 4.0 for _, p in c.trained())
    # and the other way round: three steps of the ordinary loop, then train_step
    d = Net(key, mode)
    opt_d = d.adam(lr=1e-3)
    for _ in range(3):
        _ordinary_step(d, opt_d)
    e = Net(key, mode, state=d.sd())
    opt_e = e.adam(lr=1e-3)
    opt_e.load_state_dict(copy.deepcopy(opt_d.state_dict()))
    assert e.m.train_step_reason(e.xd, e.hrd, opt_e) is None
    assert math.isfinite(e.step(opt_e).item())
    assert all(float(opt_e.state[p]["step"]) == 4.0 for _, p in e.trained())
    assert all(p.grad is None for _, p in e.trained())


@pytest.mark.parametrize("key", [("single", 8, 1), ("multi", 8, 2)], ids=_id)
def test_no_graph_no_grads_and_untouched_parameters(key):
    net = Net(key, "fp32")
    before = {k: p.detach().clone() for k, p in net.untouched()}
    assert before and all(k.startswith(("skip.", "flownet.")) or ".skip." in k for k in before)
    opt = net.adam(lr=1e-3)
    was = torch.is_grad_enabled()
    loss = net.step(opt)
    assert torch.is_grad_enabled() == was
    assert not loss.requires_grad and loss.grad_fn is None and loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32
    assert all(p.grad is None for p in net.m.parameters())
    assert net.m.last_route == "hip_train_step"
    assert all(torch.equal(p.detach(), before[k]) for k, p in net.untouched())
    assert all(p not in opt.state for _, p in net.untouched())
    assert len(opt.state) == len(net.trained())
    # the inference route packs the stepped parameters, not a stale blob
    def infer():
        with torch.no_grad():
            return (net.m(net.xd, 4 * net.h, 4 * net.w) if net.net == "single" else net.m(net.xd)).clone()

    y1 = infer()
    net.step(opt)
    y2 = infer()
    assert net.m.last_route == "hip" and not torch.equal(y1, y2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", [("single", 8, 2), ("multi", 8, 2)], ids=_id)
def test_loss_weight_scales_the_gradients_exactly(key, mode):
    _, _, loss, plain = _first_step(key, mode, "charbonnier")
    _, _, loss_q, quarter = _first_step(key, mode, "charbonnier", 0.25)
    assert plain and all(torch.equal(quarter[k], 0.25 * plain[k]) for k in plain)
    assert any(bool(v.abs().max() > 0) for v in plain.values())
    assert torch.equal(loss_q, 0.25 * loss)


@pytest.mark.parametrize("key", [("single", 8, 1), ("multi", 8, 2)], ids=_id)
def test_refusal_on_the_device(key):
    from mobilesuperresolution_amd import _lib as L
    net = Net(key, "fp32")
    opt = net.adam(lr=1e-3)
    sd0 = net.sd()

    def refused(hr=None, why=None):
        hr = net.hrd if hr is None else hr
        reason = net.m.train_step_reason(net.xd, hr, opt)
        assert reason is not None and (why is None or reason == why)
        with pytest.raises(L.HotpathError) as info:
            net.m.train_step(net.xd, hr, opt)
        assert reason in str(info.value)

    refused(torch.rand(net.hrd.shape[:3] + (4 * net.h + 1, 4 * net.w), device=DEV))      # (height, weight) cannot be (4H, 4W)
    refused(net.hrd.cpu())
    name, p = net.trained()[0]
    p.requires_grad_(False)
    refused(why="a frozen parameter")
    p.requires_grad_(True)
    p.data = p.data.cpu()                                                                # a parameter on another device
    refused(why="parameters on another device")
    p.data = p.data.to(DEV)
    assert net.m.train_step_reason(net.xd, net.hrd, opt) is None
    with pytest.raises(ValueError):
        net.m.train_step(net.xd, net.hrd, opt, criterion="mse")
    # nothing ran: no state, no change
    assert len(opt.state) == 0 and all(torch.equal(v, sd0[k]) for k, v in net.sd().items())
