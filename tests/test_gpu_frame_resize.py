"""`hot_resize` of the per-frame video network on the MI355X: the sized upsampler kernels (csrc/frame_net.h fn_up_sized_kernel,
csrc/frame_net_bwd.h fn_up_bwd_sized_kernel) through sr_fn_net_fwd_sized / sr_fn_net_train_fwd_sized / sr_fn_net_bwd_sized and
models/single_image_model.py, both hot dtypes.  The float64 references are those of tests/frame_net_ref.py and
tests/frame_net_train_ref.py with the resize written from packing.resize_axis' tables (tests/frame_resize_ref.py); the accuracy rule
is tests/parity_kit.bound.  Everything a call writes starts as NaN; every measured ratio is printed.

  forward    the upsampler stage alone on exact cases (D exact, so only the blend is measured; yardstick: the same blend in fp32 torch
             ops), at 2 x 2 tiles with remainders, one exact tile and 1 x 1, up / identity / down / many-per-cell / empty workgroups /
             one pixel; through the module against the ATen route's (fp32) and the rounding-point restatement's (bf16) distance;
             repeats, a non-contiguous view, flag off = the parent's WRITE_D + F.interpolate bits, (4H, 4W) = today's kernel's bits
  backward   the upsampler stage alone (df, dW_up, db_up) against float64 autograd on the operands the kernel read, exact zeros
             where a one-pixel gradient reaches nothing, two equal calls; through the module with loss.backward(), a criterion of
             `training` (the fold declines) and hot_training alone (ATen)
  refusals   an oversized output, bad geometry and null tables at the three C entry points
"""
import pytest
import torch
import torch.nn.functional as F

from tests import frame_net_ref as R
from tests import frame_net_train_ref as T
from tests import frame_resize_ref as Z
from tests.parity_kit import bound, hold_rounded, rel_max
from tests.test_gpu_frame_net import Net
from tests.test_gpu_frame_net_train import TrainNet, _module, _param_grads

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """as tests/test_gpu_frame_net.py: drop the device-resident pack indices and hand the free blocks back"""
    yield
    import gc
    from mobilesuperresolution_amd import hotpath as HP
    HP._fn_pack_index.cache_clear()
    HP._fn_bwd_pack_index.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# frames H x W -> D (4H + 1) x (4W + 1); 9 x 17: 2 x 2 upsampler tiles (8 x 16) with a one-pixel remainder each
SIZES_9x17 = [(41, 77), (37, 69), (20, 31), (111, 207), (5, 7), (1, 1), (36, 68)]
STAGE = ([((20, 1, 2, 9, 17), s) for s in SIZES_9x17] + [((32, 2, 3, 9, 17), s) for s in ((41, 77), (20, 31))]
         + [((32, 1, 2, 8, 16), s) for s in ((36, 70), (33, 65), (17, 30), (32, 64))]
         + [((20, 2, 3, 1, 1), s) for s in ((7, 3), (5, 5), (1, 1), (13, 11))])
_id = lambda k: "c{}-nb{}-n{}-{}x{}".format(*k) if len(k) == 5 else "to{}x{}".format(*k)


def _resize(net_or_hw, size):
    from mobilesuperresolution_amd import hotpath as HP
    h, w = net_or_hw if isinstance(net_or_hw, tuple) else (net_or_hw.h, net_or_hw.w)
    return HP.fn_resize(h, w, size[0], size[1], torch.device(DEV))


# ---- forward: the upsampler stage alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key, size", STAGE, ids=_id)
def test_forward_stage_on_exact_cases(key, size, mode):
    from mobilesuperresolution_amd import hotpath as HP, packing as P
    case = R.exact_case(*key)
    net = Net(case, DTYPES[mode])
    net.run(P.FN_ENCODER | P.FN_BLOCKS | P.FN_LAST)
    out = torch.full((net.n, 3) + size, NAN, dtype=torch.float32, device=DEV)
    HP.fn_net_fwd_sized(net.x, net.blob, net.offs, net.head, net.scratch, out, out.stride(0), _resize(net, size), net.nb, P.FN_UP)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()), "an output pixel was not written"
    D = case["ref"]["D"]                                       # exact on the device (tests/test_gpu_frame_net.py holds that)
    ref = Z.blend(D, size)
    yard = rel_max(Z.blend(D.float(), size, torch.float32), ref)
    hold_rounded("frame resize fwd stage", f"{_id(key)} -> {size[0]}x{size[1]}", mode, [("out", out, ref, yard)])
    assert bool(torch.isnan(net.out).all()) and bool(torch.isnan(net.d).all())


# ---- forward: through the module ------------------------------------------------------------------------------------------------------
def _module_d(m, x):
    """the parent's route at a free size, first half: D from the WRITE_D kernel (models/single_image_model._forward_hip)"""
    from mobilesuperresolution_amd import hotpath as HP, packing as P
    from mobilesuperresolution_amd.models import clip_train as CT
    b, n, _, h, w = x.shape
    blob, offs, head = m._blobs()
    scratch = torch.empty((3, b * n, h, w, P.FN_C), dtype=m.hot_dtype, device=x.device)
    d = torch.empty((b * n, 3, 4 * h + 1, 4 * w + 1), dtype=torch.float32, device=x.device)
    HP.fn_net_fwd(CT.frames_of(x), blob, offs, head, scratch, d, d.stride(0), m.blocks, P.FN_ALL | P.FN_WRITE_D)
    return d


MODULE = [(20, 2, 3, 9, 17), (32, 1, 2, 9, 17)]


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key", MODULE, ids=_id)
def test_forward_through_the_module(key, mode):
    case = R.rounded_case(*key)
    n, h, w = key[2:]
    m = _module(case, mode, hot_resize=True).eval()
    p = R.effective({k: v.cpu() for k, v in m.state_dict().items()}, case["nb"])
    x = case["x"].float()
    xd = x.to(DEV).unsqueeze(0)
    D = R.forward(x, p)["D"]
    for size in ((41, 77), (20, 31), (111, 207)):
        ref = Z.blend(D, size)
        with torch.no_grad():
            got = m(xd, *size)
            assert m.last_route == "hip" and got.shape == (1, n, 3) + size
            again = m(xd, *size)
            m.hot_resize = False
            plain = m(xd, *size)
            assert m.last_route == "hip"
            parent = F.interpolate(_module_d(m, xd), size=size, mode="bilinear").view(1, n, 3, *size)
            m.aten_forward = True
            aten = m(xd, *size)
            assert m.last_route == "aten"
            m.aten_forward, m.hot_resize = False, True
        assert torch.equal(got, again)
        assert torch.equal(plain, parent), "flag off: the parent's route, bit for bit"
        if mode == "fp32":
            yard = rel_max(aten[0].double().cpu(), ref)
        else:
            yard = rel_max(Z.blend(R.forward(x, p, rnd=R.bf16_round)["D"], size), ref)
        err = rel_max(got[0].double().cpu(), ref)
        tol = bound(mode, yard, slack=0.0)
        print(f"frame resize fwd module | {_id(key)} -> {size} | {mode} | yardstick {yard:.3e} | kernel {err:.3e} | ratio {err / yard:.2f}")
        assert err <= tol, (size, mode, err, tol)
    # (4H, 4W): today's kernel, flag or no flag
    with torch.no_grad():
        on = m(xd, 4 * h, 4 * w)
        m.hot_resize = False
        off = m(xd, 4 * h, 4 * w)
    assert torch.equal(on, off)


@pytest.mark.parametrize("mode", DTYPES)
def test_forward_repeats_and_views(mode):
    case = R.rounded_case(32, 2, 3, 20, 28)
    m = _module(case, mode, hot_resize=True).eval()
    x = case["x"].float().unsqueeze(0).to(DEV)
    wide = torch.rand(1, 3, 5, 20, 30, device=DEV)
    wide[:, :, 1:4, :, 1:29] = x
    view = wide[:, :, 1:4, :, 1:29]
    assert not view.is_contiguous()
    with torch.no_grad():
        a, b, c = m(x, 90, 126), m(x, 90, 126), m(view, 90, 126)
        d, e = m(x, 77, 100), m(view, 77, 100)
    assert m.last_route == "hip" and len(m._fn_resize) == 2
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(d, e)
    import pickle
    assert "_fn_resize" not in m.__getstate__() and pickle.loads(pickle.dumps(m.cpu())).hot_resize is True


# ---- backward: the upsampler stage alone ----------------------------------------------------------------------------------------------
def _up_backward(f, up_w, up_b, g, size, dtype=torch.float64, rnd=None):
    """(df, dW_up, db_up) of out = blend(conv_transpose2d(f, up_w, up_b, stride 4), size) for the output gradient g, as
    frame_net_train_ref.backward forms them at (4H, 4W): dD by autograd through the table blend, then df and dW_up from dD with the
    route's rounding points (rnd: dD as the MFMA operand, df as it is stored; db_up an fp32 accumulator over the rows)"""
    r = rnd if rnd is not None else (lambda t: t)
    f, up_w, g = f.to(dtype), r(up_w.to(dtype)), g.to(dtype)
    D = F.conv_transpose2d(f, up_w, r(up_b.to(dtype)), stride=4).detach().requires_grad_(True)
    dD, = torch.autograd.grad(Z.blend(D, size, dtype), D, g)
    dDr = r(dD)
    df = r(F.conv2d(dDr, up_w, stride=4))
    dw = torch.nn.grad.conv2d_weight(dDr, tuple(up_w.shape), f, stride=4)
    db = g.sum((0, 2, 3))
    if rnd is not None:
        acc = torch.zeros(3, dtype=torch.float32)
        for row in g.float().permute(0, 2, 1, 3).reshape(-1, 3, g.shape[-1]):
            acc = acc + row.sum(-1)
        db = acc.to(dtype)
    return dict(df=df.double(), up_w=dw.double(), up_b=db.double())


def _stage_bwd(net, g, size):
    """the sized upsampler backward alone on net's saved f; -> (df (N, C, H, W), dW_up, db_up) as float64 CPU tensors"""
    from mobilesuperresolution_amd import hotpath as HP, packing as P
    g = g.float().to(DEV).contiguous()
    HP.fn_net_bwd_sized(net.x, g, g.stride(0), _resize(net, size), net.bwd_blob, net.acts, net.ts, net.masks, net.gs, net.parts, net.wgs,
                        net.grads, net.c, net.nb, P.FN_BWD_UP)
    torch.cuda.synchronize()
    pieces = net.pieces()
    df = net.g(0)
    assert not bool(df[..., net.c:].any()), "padding channels of df"
    return dict(df=df[..., :net.c].permute(0, 3, 1, 2), up_w=pieces["up_w"].double().view(net.c, 3, 5, 5), up_b=pieces["up_b"].double())


def _saved_f(net):
    return net.acts[net.nb + 1].double().cpu()[..., :net.c].permute(0, 3, 1, 2).contiguous()


BWD_STAGE = [((20, 1, 2, 9, 17), s) for s in SIZES_9x17] + [((32, 2, 3, 9, 17), (41, 77)), ((32, 1, 2, 8, 16), (36, 70)),
                                                           ((32, 1, 2, 8, 16), (17, 30)), ((20, 2, 3, 1, 1), (7, 3)), ((20, 2, 3, 1, 1), (1, 1))]


@pytest.mark.parametrize("wgs", (0, 1), ids=("wgs-default", "wgs-1"))
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key, size", BWD_STAGE, ids=_id)
def test_backward_stage(key, size, mode, wgs):
    case = R.rounded_case(*key)
    net = TrainNet(case, DTYPES[mode], wgs)
    net.fwd()
    g = torch.randn(net.n, 3, *size, generator=torch.Generator().manual_seed(13)).double()
    got = _stage_bwd(net, g, size)
    assert bool(torch.isnan(net.gs[1:].float()).all()) and net.nan_except(("up_w", "up_b"))
    # the operands the kernel read: f as the forward left it, the upsampler's weights as they were packed
    f, p = _saved_f(net), case["p"]
    rnd = R.bf16_round if mode == "bf16" else (lambda t: t.float().to(t.dtype))
    ref = _up_backward(f, rnd(p["up_w"].double()), p["up_b"], g, size)
    if mode == "fp32":
        yard = _up_backward(f, rnd(p["up_w"].double()), p["up_b"], g, size, dtype=torch.float32)
    else:
        yard = _up_backward(f, p["up_w"], p["up_b"], g, size, rnd=R.bf16_round)
    hold_rounded("frame resize bwd stage", f"{_id(key)} -> {size[0]}x{size[1]}", mode,
                 [(k, got[k], ref[k], rel_max(yard[k], ref[k])) for k in ("df", "up_w", "up_b")])
    # two equal calls: the same bits
    first = {k: v.clone() for k, v in got.items()}
    net.gs.fill_(NAN)
    net.grads.fill_(NAN)
    net.parts.fill_(NAN)
    again = _stage_bwd(net, g, size)
    assert all(torch.equal(first[k], again[k]) for k in first)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("spot", [(0, 1, 7, 12), (1, 2, 19, 30), (1, 0, 0, 0), (0, 0, 10, 30)], ids=str)
def test_backward_of_one_output_pixel_touches_only_its_cells(spot, mode):
    """(20, 31) from a 37 x 69 D: most D rows and columns have no output at all.  g = one pixel: dD is non-zero on its (at most) four
    cells of one channel and EXACTLY zero elsewhere, seen through db_up (one channel), dW_up (only the taps of the LR pixels whose
    5 x 5 patch holds a cell, only that channel) and df (only those LR pixels) of a one-channel network"""
    size = (20, 31)
    case = R.rounded_case(1, 1, 2, 9, 17)
    net = TrainNet(case, DTYPES[mode])
    net.fwd()
    n, o, oy, ox = spot
    g = torch.zeros(net.n, 3, *size, dtype=torch.float64)
    g[n, o, oy, ox] = 1.5
    got = _stage_bwd(net, g, size)
    rnd = R.bf16_round if mode == "bf16" else (lambda t: t.float().to(t.dtype))
    ref = _up_backward(_saved_f(net), rnd(case["p"]["up_w"].double()), case["p"]["up_b"], g, size)
    for k in ("df", "up_w", "up_b"):
        dead = ref[k] == 0
        assert bool(dead.any()) and not bool(dead.all()), k
        assert not bool(got[k][dead].any()), (k, "a D cell no output names carried a gradient")
    assert torch.equal(got["up_b"], g.sum((0, 2, 3)))
    assert int((got["df"] != 0).sum()) <= 4 and int((got["up_w"][:, o] != 0).sum()) <= 16
    yard = _up_backward(_saved_f(net), case["p"]["up_w"], case["p"]["up_b"], g, size, dtype=torch.float32 if mode == "fp32" else torch.float64,
                        rnd=R.bf16_round if mode == "bf16" else None)
    hold_rounded("frame resize bwd one pixel", str(spot), mode, [(k, got[k], ref[k], rel_max(yard[k], ref[k])) for k in ("df", "up_w")])


# ---- backward: through the module -----------------------------------------------------------------------------------------------------
def _reference_grads(sd, nb, x, p, gout, size, rnd=None):
    """{state_dict key: gradient} in float64: frame_net_train_ref.backward's chain, entered at df, behind the table blend"""
    fw = R.forward(x, p, rnd=rnd)
    up = _up_backward(fw["f"], p["up_w"].double(), p["up_b"].double(), gout, size, rnd=rnd)
    grads = T.backward(x, p, None, rnd=rnd, df=up["df"])["grads"]
    grads.update(up_w=up["up_w"], up_b=up["up_b"])
    return T.param_grads(sd, nb, grads)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("size", [(41, 77), (20, 31)], ids=_id)
@pytest.mark.parametrize("key", [(20, 2, 3, 9, 17), (32, 1, 2, 9, 17)], ids=_id)
def test_backward_through_the_module(key, size, mode):
    case = R.rounded_case(*key)
    n = key[2]
    m = _module(case, mode, hot_training=True, hot_resize=True)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    p = R.effective(sd, case["nb"])
    x = case["x"].float()
    xd = x.to(DEV).unsqueeze(0)
    gout = torch.randn(n, 3, *size, generator=torch.Generator().manual_seed(11)).double()
    ref = _reference_grads(sd, case["nb"], x, p, gout, size)

    def run(mm):
        mm.zero_grad()
        y = mm(xd, *size)
        (y[0] * gout.float().to(DEV)).sum().backward()
        return y.detach(), _param_grads(mm)

    if mode == "fp32":
        tf32 = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
        torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
        try:
            plain = _module(case, mode)
            _, yard = run(plain)
            assert plain.last_route == "aten"
        finally:
            torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = tf32
    else:
        yard = _reference_grads(sd, case["nb"], x, p, gout, size, rnd=R.bf16_round)
    assert m.train_route_reason(xd, *size) is None
    y, got = run(m)
    assert m.last_route == "hip_train" and y.shape == (1, n, 3) + size
    with torch.no_grad():
        assert torch.equal(y, m(xd, *size)) and m.last_route == "hip"
    assert all((got[k] is None) == k.startswith("skip.") for k in got)
    hold_rounded("frame resize train", f"{_id(key)} -> {size[0]}x{size[1]}", mode, [(k, got[k], ref[k], rel_max(yard[k], ref[k])) for k in ref])
    _, again = run(m)
    assert all(torch.equal(got[k], again[k]) for k in ref)


@pytest.mark.parametrize("mode", DTYPES)
def test_criterion_takes_its_torch_path_and_hot_training_alone_stays_aten(mode):
    from mobilesuperresolution_amd import training
    case = R.rounded_case(20, 2, 3, 9, 17)
    size = (41, 77)
    m = _module(case, mode, hot_training=True, hot_resize=True)
    x = case["x"].float().unsqueeze(0).to(DEV)
    hr = torch.rand(1, 3, 3, *size, generator=torch.Generator().manual_seed(2)).to(DEV)
    crit = training.L1_Charbonnier_loss()

    def grads(loss_of):
        m.zero_grad()
        loss = loss_of(m(x, *size), hr)
        assert m.last_route == "hip_train"
        loss.backward()
        return type(loss.grad_fn).__name__, _param_grads(m)

    name, folded = grads(crit)
    assert name != "_FoldedCriterionBackward"
    def charbonnier(sr, t):
        diff = torch.add(sr, -t)
        return torch.mean(torch.sqrt(diff * diff + 1e-12))

    _, written = grads(charbonnier)
    assert all(torch.equal(folded[k], written[k]) for k in folded if folded[k] is not None)
    # at (4H, 4W) the same node still folds
    m.zero_grad()
    loss = crit(m(x, 36, 68), torch.rand(1, 3, 3, 36, 68, device=DEV))
    assert type(loss.grad_fn).__name__ == "_FoldedCriterionBackward"
    loss.backward()
    # hot_training alone: the size keeps the ATen route, as before
    alone = _module(case, mode, hot_training=True)
    assert alone.train_route_reason(x, *size) == "output size is not (4H, 4W)"
    out = alone(x, *size)
    assert alone.last_route == "aten" and out.requires_grad
    # train_step stays at (4H, 4W)
    opt = training.Adam([q for mod in (m.encoder, m.body, m.shuf) for q in mod.parameters()], lr=1e-3)
    assert m.train_step_reason(x, hr, opt) == "hr is not fp32 (B, N, 3, 4H, 4W) on the input's device"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", DTYPES)
def test_an_oversized_output_is_refused_by_the_route_rule(mode):
    from mobilesuperresolution_amd import hotpath as HP, packing as P
    case = R.rounded_case(20, 2, 3, 9, 17)
    m = _module(case, mode, hot_training=True, hot_resize=True)
    x = case["x"].float().unsqueeze(0).to(DEV)
    big = P.FN_MAX_OUT + 1
    assert "beyond the sized kernels' tables" in m.train_route_reason(x, 2, big)
    with torch.no_grad():
        assert "beyond the sized kernels' tables" in m.hot_route_reason(x, 2, big)
        out = m(x, 2, big)
    assert m.last_route == "aten" and out.shape == (1, 3, 3, 2, big) and "_fn_resize" not in m.__dict__
    with pytest.raises(ValueError):
        HP.fn_resize(9, 17, 2, big, torch.device(DEV))


@pytest.mark.parametrize("mode", DTYPES)
def test_sized_entry_points_refuse_bad_arguments_untouched(mode):
    from mobilesuperresolution_amd import _lib as L
    net = TrainNet(R.exact_case(32, 1, 1, 3, 3), DTYPES[mode])
    inf = Net(R.exact_case(32, 1, 1, 3, 3), DTYPES[mode])
    lib, code = L.lib(), L.DTYPE_CODE[DTYPES[mode]]
    oh, ow = 14, 11
    rz = _resize((3, 3), (oh, ow))
    out = torch.full((1, 3, oh, ow), NAN, dtype=torch.float32, device=DEV)
    g = torch.zeros(1, 3, oh, ow, device=DEV)
    ptr = lambda t: t.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        bufs = (net.acts, net.ts, net.out, net.gs, net.parts, net.grads, inf.scratch, out)
        return all(bool(torch.isnan(t.float()).all()) for t in bufs) and bool((net.masks == -1).all())

    def tabs(kw):
        return kw.get("oh", oh), kw.get("ow", ow), kw.get("ty", ptr(rz[2])), kw.get("ly", ptr(rz[3])), kw.get("tx", ptr(rz[4])), kw.get("lx", ptr(rz[5]))

    def fwd(n=1, h=3, w=3, nb=1, dtype=code, stages=15, out_is=out.stride(0), **kw):
        return lib.sr_fn_net_fwd_sized(ptr(inf.x), ptr(inf.blob), inf.offs, ptr(inf.head), ptr(inf.scratch[0]), ptr(inf.scratch[1]),
                                       ptr(inf.scratch[2]), ptr(out), out_is, *tabs(kw), nb, n, h, w, dtype, stages, L.stream_ptr())

    def train(n=1, h=3, w=3, nb=1, dtype=code, stages=15, out_is=out.stride(0), **kw):
        return lib.sr_fn_net_train_fwd_sized(ptr(net.x), ptr(net.blob), net.offs, ptr(net.head), ptr(net.acts), ptr(net.ts), ptr(net.masks),
                                             ptr(out), out_is, *tabs(kw), nb, n, h, w, dtype, stages, L.stream_ptr())

    def bwd(n=1, h=3, w=3, nb=1, dtype=code, stages=15, out_is=g.stride(0), **kw):
        return lib.sr_fn_net_bwd_sized(ptr(net.x), ptr(g), out_is, *tabs(kw), ptr(net.bwd_blob), ptr(net.acts), ptr(net.ts), ptr(net.masks),
                                       ptr(net.gs), ptr(net.parts), net.wgs, ptr(net.grads), 32, nb, n, h, w, dtype, stages, L.stream_ptr())

    for kw in (dict(n=65536), dict(h=8193), dict(w=8193), dict(dtype=7), dict(nb=1025), dict(oh=32769), dict(ow=32769)):
        assert fwd(**kw) == -1 and train(**kw) == -1 and bwd(**kw) == -1 and untouched(), kw
    for kw in (dict(ty=None), dict(ly=None), dict(tx=None), dict(lx=None), dict(oh=0), dict(ow=0), dict(oh=-3), dict(stages=0), dict(stages=16),
               dict(nb=-1), dict(n=0), dict(out_is=3 * oh * ow - 1)):
        assert fwd(**kw) == -2 and train(**kw) == -2 and bwd(**kw) == -2 and untouched(), kw
    assert fwd() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    kept = out.clone()
    out.fill_(NAN)
    assert train() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, kept) and not bool(torch.isnan(net.grads).any())
