"""Result_Model (the NAS stage-3 network) on the MI355X: fixture G18 (the reference's own network) in fp32 and bf16, every
block-kernel instance and the tail at every k_last against F.conv2d, three steps of the reference's training loop, and
tiled inference.  Importing the model module fails on a tree without the feature."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mobilesuperresolution_amd import hotpath as HP
from mobilesuperresolution_amd import packing as P
from mobilesuperresolution_amd.models.result_model import Result_Model

pytestmark = pytest.mark.gpu

G18 = os.path.join(os.path.dirname(__file__), "golden", "g18_result_model.npz")
# bf16 bound (relative L2 of the output and of every gradient): measured worst over G18 a / b, times about two
BF16_OUT_L2, BF16_GRAD_L2 = 6e-3, 7.5e-2


def _wn(v, g):
    return torch._weight_norm(v, g, 0)


def aten_forward(sd, status, scale, x):
    """fp32 ATen restatement of pretrain_simplified_model.Result_Model.forward from a state_dict"""
    c = lambda p, t, k: F.conv2d(t, _wn(sd[p + ".weight_v"], sd[p + ".weight_g"]), sd[p + ".bias"], padding=k // 2)
    x = x - 0.5
    y = c("body.0", x, 3)
    IN = status[0][0]
    for i, (_, split, k) in enumerate(status):
        a = IN - split
        ys = y[:, a:]
        ys = torch.relu(c(f"body.{i + 1}.body.0.body.0", ys, k)) + ys
        y = torch.cat([y[:, :a], ys], 1) if a > 0 else ys
    y = c(f"body.{len(status) + 1}", y, status[-1][2]) + c("skip", x, 5)
    return F.pixel_shuffle(y, scale)


def _g18(tag):
    z = np.load(G18)
    g = lambda pre: {k[len(f"{tag}/{pre}/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{tag}/{pre}/")}
    return dict(params=g("p"), grads=g("g"), x=torch.from_numpy(z[f"{tag}/x"]), hr=torch.from_numpy(z[f"{tag}/hr"]),
                y=torch.from_numpy(z[f"{tag}/y"]), loss=float(z[f"{tag}/loss"]), status=z[f"{tag}/status"].tolist(),
                scale=int(z[f"{tag}/scale"]))


def _run(m, x, hr):
    m.zero_grad()
    y = m(x.cuda())
    loss = F.l1_loss(y, hr.cuda())
    loss.backward()
    return y.detach().cpu(), loss.item(), {k: p.grad.detach().cpu() for k, p in m.named_parameters()}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g18_fp32_parity(tag):
    d = _g18(tag)
    m = Result_Model(d["scale"], status=d["status"], hot_dtype="fp32").cuda()
    m.load_state_dict(d["params"], strict=True)
    y, loss, grads = _run(m, d["x"], d["hr"])
    rel = ((y - d["y"]).abs().max() / d["y"].abs().max()).item()
    assert rel <= 2e-5, rel
    assert abs(loss - d["loss"]) <= 1e-5 * abs(d["loss"])
    worst = max(((grads[k] - g).abs().max() / g.abs().max().clamp_min(1e-12)).item() for k, g in d["grads"].items())
    assert worst <= 3e-4, worst
    print(f"\nG18 {tag} fp32: out {rel:.2e} rel max-abs, worst grad {worst:.2e}")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g18_bf16(tag):
    d = _g18(tag)
    m = Result_Model(d["scale"], status=d["status"], hot_dtype="bf16").cuda()
    m.load_state_dict(d["params"], strict=True)
    y, _, grads = _run(m, d["x"], d["hr"])
    rel = ((y - d["y"]).norm() / d["y"].norm()).item()
    worst = max(((grads[k] - g).norm() / g.norm().clamp_min(1e-12)).item() for k, g in d["grads"].items())
    print(f"\nG18 {tag} bf16: out {rel:.2e} rel L2, worst grad {worst:.2e} rel L2")
    assert rel <= BF16_OUT_L2 and worst <= BF16_GRAD_L2, (rel, worst)


def _bf(t):
    return t.bfloat16().float()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F_,IN,split", [(24, 20, 12), (32, 27, 27)])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_block_kernels_against_conv2d(dtype, F_, IN, split, k):
    """sr_rm_block_fwd / _bwd_data / sr_rm_wgrad of one (k, F, dtype) instance against F.conv2d in fp32 on bf16-rounded inputs"""
    g = torch.Generator().manual_seed(k * 1000 + F_ + split)
    n, h, w = 2, 19, 37
    a = IN - split
    x = torch.zeros(n, F_, h, w)
    x[:, :IN] = _bf(torch.randn(n, IN, h, w, generator=g))
    wt = _bf(torch.randn(split, split, k, k, generator=g) / (split * k))
    b = _bf(torch.randn(split, generator=g) * 0.1)
    gy = torch.zeros(n, F_, h, w)
    gy[:, :IN] = _bf(torch.randn(n, IN, h, w, generator=g))
    xs = x[:, a:IN].clone().cuda().requires_grad_(True)
    wr, br = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    z = F.conv2d(xs, wr, br, padding=k // 2)
    ys = xs + torch.relu(z)
    ys.backward(gy[:, a:IN].cuda())
    ref = x.clone().cuda()
    ref[:, a:IN] = ys.detach()
    refdx = gy.clone().cuda()
    refdx[:, a:IN] = xs.grad

    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda().to(dtype)
    wd = torch.zeros(F_, F_, k, k, device="cuda")
    wd[a:IN, a:IN] = wt.cuda()
    b32 = torch.zeros(32, device="cuda")
    b32[a:IN] = b.cuda()
    xin, dy = nhwc(x), nhwc(gy)
    y = torch.empty_like(xin)
    m = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
    HP.rm_block_fwd(xin, y, m, HP.rm_pack(wd, dtype), b32, k)
    dx = torch.empty_like(dy)
    HP.rm_block_bwd_data(dy, m, dx, HP.rm_pack(wd.transpose(0, 1).flip(2, 3).contiguous(), dtype), k)
    gw, gb = HP.rm_wgrad(dy, m, xin, F_, F_, k)
    torch.cuda.synchronize()
    mask_ref = (z.detach() > 0)
    bits = torch.zeros(n, h, w, dtype=torch.int64, device="cuda")
    for c in range(split):
        bits |= mask_ref[:, c].long() << (a + c)
    assert torch.equal(m.long() & 0xFFFFFFFF, bits)
    yf, dxf = y.float().permute(0, 3, 1, 2), dx.float().permute(0, 3, 1, 2)
    tol = 1e-5 if dtype == torch.float32 else 1.5e-2
    e_y = ((yf - ref).abs().max() / ref.abs().max()).item()
    e_dx = ((dxf - refdx).abs().max() / refdx.abs().max()).item()
    e_w = ((gw[a:IN, a:IN] - wr.grad).abs().max() / wr.grad.abs().max()).item()
    e_b = ((gb[a:IN] - br.grad).abs().max() / br.grad.abs().max()).item()
    assert max(e_y, e_dx) <= tol and max(e_w, e_b) <= (1e-4 if dtype == torch.float32 else 1e-2), (e_y, e_dx, e_w, e_b)
    assert torch.equal(yf[:, :a], ref[:, :a]) and torch.equal(yf[:, IN:], torch.zeros_like(yf[:, IN:]))
    assert gw[:a].abs().sum().item() == 0 and gw[IN:].abs().sum().item() == 0


def _model_vs_aten(scale, status, dtype, n=2, h=13, w=17, seed=0):
    torch.manual_seed(seed)
    m = Result_Model(scale, status=status, hot_dtype=dtype).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.bfloat16().float())
    g = torch.Generator().manual_seed(seed + 1)
    x = _bf(torch.rand(n, 3, h, w, generator=g)).cuda()
    hr = torch.rand(n, 3, scale * h, scale * w, generator=g).cuda()
    y, loss, grads = _run(m, x, hr)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    yr = aten_forward(sd, status, scale, x)
    F.l1_loss(yr, hr).backward()
    return y, yr.detach().cpu(), grads, {k: v.grad.cpu() for k, v in sd.items()}


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("k_last", [3, 5, 7])
def test_tail_every_k_last_against_aten(scale, k_last):
    status = [[24, 10, 5], [24, 24, k_last]] if scale != 3 else [[30, 30, 3], [30, 7, k_last]]
    y, yr, grads, gref = _model_vs_aten(scale, status, "fp32", seed=scale * 10 + k_last)
    rel = ((y - yr).abs().max() / yr.abs().max()).item()
    worst = max(((grads[k] - g).abs().max() / g.abs().max().clamp_min(1e-12)).item() for k, g in gref.items())
    assert rel <= 2e-5 and worst <= 3e-4, (rel, worst)


def test_reference_training_loop_three_steps_hot_adam_vs_torch_adam():
    """pretrain_simplified_model.py:186-198 with training.L1Loss + training.Adam against an fp32 ATen restatement stepped by
    torch.optim.Adam; and the same loop with nn.L1Loss + torch.optim.Adam on the model itself"""
    from mobilesuperresolution_amd import training
    status, scale = [[27, 16, 3], [27, 27, 5], [27, 9, 7]], 2
    torch.manual_seed(5)
    m = Result_Model(scale, status=status, hot_dtype="fp32").cuda()
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    opt = training.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-3)
    opt_ref = torch.optim.Adam(sd.values(), lr=1e-3)
    crit = {"l1": training.L1Loss()}
    g = torch.Generator().manual_seed(6)
    for _ in range(3):
        lr = torch.rand(4, 3, 15, 13, generator=g).cuda()
        hr = torch.rand(4, 3, 30, 26, generator=g).cuda()
        opt.zero_grad()
        sr = m(lr)
        loss = 1.0 * crit["l1"](sr, hr)
        loss.backward()
        opt.step()
        opt.zero_grad()
        opt_ref.zero_grad()
        lref = F.l1_loss(aten_forward(sd, status, scale, lr), hr)
        lref.backward()
        opt_ref.step()
        assert abs(loss.item() - lref.item()) <= 1e-5 * lref.item()
    diff = torch.cat([(v - sd[k]).abs().reshape(-1) for k, v in m.state_dict().items()])
    assert (diff <= 1e-4).float().mean().item() >= 0.99
    # the stock objects of the reference's loop work too
    m2 = Result_Model(scale, status=status, hot_dtype="bf16").cuda()
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3)
    for _ in range(3):
        o2.zero_grad()
        l2 = torch.nn.L1Loss()(m2(lr), hr)
        l2.backward()
        o2.step()
    assert torch.isfinite(l2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tiled_forward_is_bit_identical(dtype):
    from mobilesuperresolution_amd.inference import tiled_forward
    torch.manual_seed(7)
    m = Result_Model(2, status=[[27, 16, 3], [27, 27, 5], [27, 9, 7]], hot_dtype=dtype).cuda().eval()
    x = torch.rand(1, 3, 61, 75, generator=torch.Generator().manual_seed(8)).cuda()
    with torch.no_grad():
        whole = m(x)
    tiled = tiled_forward(m, x, 24, max_windows=4)
    assert torch.equal(tiled, whole)
