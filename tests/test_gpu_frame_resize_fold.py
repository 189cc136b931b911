"""`hot_resize_fold` of the per-frame video network on the MI355X: the loss folded into the SIZED upsampler backward
(csrc/frame_net_bwd.h fn_up_bwd_sized_kernel<T, LOSS>, sr_fn_net_bwd_loss_sized) and the one-call step at any output size
(sr_fn_net_train_step_sized), through the C entry points and models/single_image_model.py, both hot dtypes, both criteria.

Frames are 9 x 17: 2 x 2 upsampler tiles (8 x 16 LR pixels, 32 x 64 D cells) with a one-pixel remainder each.  Output sizes: (41, 77) up,
(20, 31) down (most D cells, and whole tiles' worth of them, own no output), (111, 207) many outputs per cell, (37, 69) the identity on
D, (5, 7), (1, 1); a 1 x 1 frame -> (7, 3).  The float64 references are tests/video_fold_ref.py (loss and its gradient) in front of
tests/test_gpu_frame_resize.py's chain (the table blend, frame_net_train_ref.backward), the accuracy rule is parity_kit.bound, the
loss value's bound video_fold_ref.chain_length with the per-thread add count of the sized owner geometry (owner_adds).  Everything a
call writes starts as NaN; every measured figure is printed before it is asserted."""
import functools

import pytest
import torch

from mobilesuperresolution_amd import packing as P
from tests import clip_step_ref as S
from tests import frame_net_ref as R
from tests import frame_net_train_ref as T
from tests import video_fold_ref as V
from tests.parity_kit import bound, hold_rounded, rel_max
from tests.test_gpu_frame_net_train import TrainNet, _module, _param_grads
from tests.test_gpu_frame_resize import _reference_grads, _resize, _saved_f, _stage_bwd, _up_backward

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
DEV = "cuda:0"
NAN = float("nan")
TH, TW, NT = 8, 16, 256                                       # the upsampler backward's LR tile and workgroup size (FnBwdCfg)
_id = lambda k: "c{}-nb{}-n{}-{}x{}".format(*k) if len(k) == 5 else "to{}x{}".format(*k)
FLAGS = dict(hot_training=True, hot_resize=True, hot_resize_fold=True)


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    import gc
    from mobilesuperresolution_amd import hotpath as HP
    HP._fn_pack_index.cache_clear()
    HP._fn_bwd_pack_index.cache_clear()
    _hr.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- the sized owner geometry ---------------------------------------------------------------------------------------------------------
def owned(n_lr, tile, n_out):
    """per tile along one axis, the outputs it OWNS by the forward's rule: (first, count) from packing.resize_axis' ranges -- the
    outputs whose i0 lies in the tile's 4 x tile D rows, the last tile taking row 4 n_lr as well"""
    ax = P.resize_axis(4 * n_lr + 1, n_out)
    out = []
    for t0 in range(0, n_lr, tile):
        r0, r1 = 4 * t0, 4 * n_lr if t0 + tile >= n_lr else 4 * t0 + 4 * tile - 1
        out.append((int(ax.lo[r0]), int(ax.hi[r1]) - int(ax.lo[r0]) + 1))
    return out


def owner_adds(h, w, size):
    """the most additions one thread makes to its loss sum in one tile: the gather's first loop strides the tile's ny x nx owned outputs
    by 256 threads and adds three channels' terms per visit"""
    return max(3 * -(-(ny * nx) // NT) for _, ny in owned(h, TH, size[0]) for _, nx in owned(w, TW, size[1]))


def test_every_output_has_one_owner():
    for (h, w), size in (((9, 17), s) for s in SIZES_9x17 + [(36, 68)]):
        for n_lr, tile, n_out in ((h, TH, size[0]), (w, TW, size[1])):
            runs = owned(n_lr, tile, n_out)
            assert runs[0][0] == 0 and sum(c for _, c in runs) == n_out and all(c >= 0 for _, c in runs)
            assert all(a[0] + a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert any(c == 0 for _, c in owned(9, TH, 1)), "at (1, 1) a tile row owns nothing"


@functools.lru_cache(maxsize=None)
def _hr(n, size, seed=77):
    return torch.rand(n, 3, *size, generator=torch.Generator().manual_seed(seed))


def _criterion(kind):
    from mobilesuperresolution_amd import training as TR
    return TR.L1Loss() if kind == "l1" else TR.L1_Charbonnier_loss()


def _folded(t):
    return type(t.grad_fn).__name__ == "_FoldedCriterionBackward"


def _tf32_off():
    class Off:
        def __enter__(self):
            self.was = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
            torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False

        def __exit__(self, *exc):
            torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = self.was
    return Off()


# ---- the stage alone, and the persistent walk -----------------------------------------------------------------------------------------
SIZES_9x17 = [(41, 77), (20, 31), (111, 207), (37, 69), (5, 7), (1, 1)]
STAGE = ([((20, 1, 2, 9, 17), s, 0) for s in SIZES_9x17] + [((32, 2, 3, 9, 17), (41, 77), 0), ((8, 1, 2, 9, 17), (20, 31), 0),
         ((20, 2, 3, 1, 1), (7, 3), 0)]
         + [((32, 2, 3, 9, 17), s, wgs) for s in ((41, 77), (20, 31)) for wgs in (1, 3)])          # fewer workgroups than the 12 tiles


def _loss_call(net, sr, hr, kind, size, loss_part, stages=P.FN_BWD_UP, **kw):
    """sr_fn_net_bwd_loss_sized itself (the wrapper of hotpath runs every stage and owns loss_part)"""
    from mobilesuperresolution_amd import _lib as L
    from mobilesuperresolution_amd.models import loss_fold as LF
    rz = kw.pop("rz", None) or _resize(net, size)
    ptr = lambda t: None if t is None else t.data_ptr()
    a = dict(hr=hr, loss_part=loss_part, kind=kind if isinstance(kind, int) else V.KINDS.index(kind) + 1, oh=rz[0], ow=rz[1], ty=rz[2],
             ly=rz[3], tx=rz[4], lx=rz[5])
    a.update(kw)
    return L.lib().sr_fn_net_bwd_loss_sized(
        ptr(net.x), ptr(sr), ptr(a["hr"]), a["kind"], LF.gscale(1.0, sr.numel()), ptr(a["loss_part"]), sr.stride(0), a["oh"], a["ow"],
        ptr(a["ty"]), ptr(a["ly"]), ptr(a["tx"]), ptr(a["lx"]), ptr(net.bwd_blob), ptr(net.acts), ptr(net.ts), ptr(net.masks), ptr(net.gs),
        ptr(net.parts), net.wgs, ptr(net.grads), net.c, net.nb, net.n, net.h, net.w, L.DTYPE_CODE[net.dtype], stages, L.stream_ptr())


def _sized_sr(net, size):
    from mobilesuperresolution_amd import hotpath as HP
    net.fwd()
    sr = torch.full((net.n, 3) + size, NAN, dtype=torch.float32, device=DEV)
    HP.fn_net_train_fwd_sized(net.x, net.blob, net.offs, net.head, net.acts, net.ts, net.masks, sr, sr.stride(0), _resize(net, size), net.nb,
                              P.FN_UP)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(sr).any())
    return sr


def _read_stage(net):
    pieces = net.pieces()
    df = net.g(0)
    assert not bool(df[..., net.c:].any()), "padding channels of df"
    return dict(df=df[..., :net.c].permute(0, 3, 1, 2), up_w=pieces["up_w"].double().view(net.c, 3, 5, 5), up_b=pieces["up_b"].double())


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key, size, wgs", STAGE, ids=lambda v: _id(v) if isinstance(v, tuple) else f"wgs{v}")
def test_stage_alone_and_the_persistent_walk(key, size, wgs, mode, kind):
    case = R.exact_case(*key)
    net = TrainNet(case, DTYPES[mode], wgs)
    sr = _sized_sr(net, size)
    hr = _hr(net.n, size).to(DEV)
    tiles = -(-net.h // TH) * -(-net.w // TW)
    items, up_wgs = net.n * tiles, min(net.n * tiles, net.wgs)
    loss_part = torch.full((net.wgs,), NAN, dtype=torch.float32, device=DEV)
    assert _loss_call(net, sr, hr, kind, size, loss_part) == 0
    torch.cuda.synchronize()
    got = _read_stage(net)
    assert bool(torch.isnan(net.gs[1:].float()).all()) and net.nan_except(("up_w", "up_b"))
    # every loss_part element the reduction reads was written (0 from a workgroup whose tiles own nothing), none beyond
    assert not bool(torch.isnan(loss_part[:up_wgs]).any()) and bool(torch.isnan(loss_part[up_wgs:]).all())
    src, hrc = sr.cpu(), hr.cpu()
    want = V.loss_value(src, hrc, kind).item()
    value = loss_part[:up_wgs].double().sum().item() / sr.numel()
    tol = V.chain_length(kind, items, up_wgs, owner_adds(net.h, net.w, size)) * 2.0 ** -24
    err = abs(value - want) / want
    print(f"resize fold stage | {_id(key)} -> {size} wgs {net.wgs} {mode} {kind} | loss {value:.8f} float64 {want:.8f} | rel err {err:.2e} | "
          f"bound {tol:.2e}")
    assert err <= tol
    # df, dW_up, db_up: float64 autograd fed the float64 loss gradient of the same sr; yardstick: the unfolded entry point fed the formula
    f, p = _saved_f(net), case["p"]
    rnd = R.bf16_round if mode == "bf16" else (lambda t: t.float().to(t.dtype))
    ref = _up_backward(f, rnd(p["up_w"].double()), p["up_b"], V.loss_grad(src, hrc, kind), size)
    first = {k: v.clone() for k, v in got.items()}
    part_first = loss_part[:up_wgs].clone()
    net.gs.fill_(NAN), net.grads.fill_(NAN), net.parts.fill_(NAN)
    yard = _stage_bwd(net, V.kernel_formula_fp32(sr, hr, kind), size)
    hold_rounded("resize fold stage", f"{_id(key)} -> {size[0]}x{size[1]} wgs {net.wgs} {kind}", mode,
                 [(k, first[k], ref[k], rel_max(yard[k], ref[k])) for k in ("df", "up_w", "up_b")])
    # two equal calls: equal bits, the loss sums included
    net.gs.fill_(NAN), net.grads.fill_(NAN), net.parts.fill_(NAN), loss_part.fill_(NAN)
    assert _loss_call(net, sr, hr, kind, size, loss_part) == 0
    torch.cuda.synchronize()
    again = _read_stage(net)
    assert all(torch.equal(first[k], again[k]) for k in first) and torch.equal(part_first, loss_part[:up_wgs])


# ---- every output is counted once -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("spots", ("corner", "last", "both"))
def test_every_output_is_counted_once(spots, mode):
    """sr == hr except at ONE output whose source cell (i0_y, i0_x) is D row 32 / column 64, the corner all four tiles' gathers read
    (rows 0 .. 32 and 32 .. 36, columns 0 .. 64 and 64 .. 68): L1 = |d| / n, a pixel counted by every tile that reads it would give 2 x
    or 4 x.  `last`: the last output row and column, whose cell is owned through the bottom / right tiles' 4H / 4W rule."""
    size = (41, 77)
    ay, ax = P.resize_axis(37, size[0]), P.resize_axis(69, size[1])
    cy, cx = int(ay.lo[32]), int(ax.lo[64])
    assert ay.hi[32] >= cy and ax.hi[64] >= cx and ay.i0[cy] == 32 and ax.i0[cx] == 64
    assert ay.i0[size[0] - 1] == 36 and ax.i0[size[1] - 1] == 68
    m = _module(R.rounded_case(32, 1, 2, 9, 17), mode, **FLAGS)
    x = R.rounded_case(32, 1, 2, 9, 17)["x"].float().unsqueeze(0).to(DEV)
    y = m(x, *size)
    hr = y.detach().clone()
    if spots in ("corner", "both"):
        hr[0, 1, 1, cy, cx] += 0.5
    if spots in ("last", "both"):
        hr[0, 0, 2, size[0] - 1, size[1] - 1] -= 0.25
    loss = _criterion("l1")(y, hr)
    assert _folded(loss) and m.last_route == "hip_train"
    want = (y.detach().double() - hr.double()).abs().sum().item() / y.numel()
    err = abs(loss.item() - want) / want
    print(f"resize fold | {spots} {mode} | loss {loss.item():.6e} expected {want:.6e} | rel err {err:.2e}")
    # d, the sum of zeros and one value, the scale; `both`: one addition of two values more
    assert want > 0 and err <= (4 if spots == "both" else 3) * 2.0 ** -24


# ---- through the module -----------------------------------------------------------------------------------------------------------------
MODULE = [((8, 2, 2, 9, 17), (41, 77)), ((32, 1, 3, 9, 17), (41, 77)), ((20, 1, 2, 9, 17), (20, 31))]


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("key, size", MODULE, ids=_id)
def test_folded_criterion_through_the_module(key, size, mode, kind):
    case = R.rounded_case(*key)
    n = key[2]
    m = _module(case, mode, **FLAGS)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    p = R.effective(sd, case["nb"])
    x = case["x"].float()
    xd = x.to(DEV).unsqueeze(0)
    hr = _hr(n, size)
    hrd = hr.view(1, n, 3, *size).to(DEV)
    crit = _criterion(kind)

    def fold(weight=None):
        m.zero_grad()
        y = m(xd, *size)
        assert m.last_route == "hip_train"
        loss = crit(y, hrd)
        assert _folded(loss) and all(q.grad is None for q in m.parameters())
        (loss if weight is None else weight * loss).backward()
        return y.detach(), loss.detach(), _param_grads(m)

    y, loss, got = fold()
    assert all((got[k] is None) == k.startswith("skip.") for k in got)
    # the loss value against the float64 mean over the same sr
    sr = y.cpu().view(n, 3, *size)
    want = V.loss_value(sr, hr, kind).item()
    from mobilesuperresolution_amd import hotpath as HP
    items = n * 4
    wgs = min(items, HP.fn_bwd_wgs(n, 9, 17))
    tol = V.chain_length(kind, items, wgs, owner_adds(9, 17, size)) * 2.0 ** -24
    err = abs(loss.item() - want) / want
    print(f"resize fold module | {_id(key)} -> {size} {mode} {kind} | loss {loss.item():.8f} float64 {want:.8f} | rel err {err:.2e} | bound {tol:.2e}")
    assert err <= tol
    # the gradients against the float64 reference fed the float64 loss gradient of the same sr
    gout = V.loss_grad(sr, hr, kind)
    ref = _reference_grads(sd, case["nb"], x, p, gout, size)
    if mode == "fp32":
        with _tf32_off():
            plain = _module(case, mode)
            (plain(xd, *size)[0] * gout.float().to(DEV)).sum().backward()
            assert plain.last_route == "aten"
            yard = _param_grads(plain)
    else:
        yard = _reference_grads(sd, case["nb"], x, p, gout, size, rnd=R.bf16_round)
    yards = {k: rel_max(yard[k], ref[k]) for k in ref}
    hold_rounded("resize fold module", f"{_id(key)} -> {size[0]}x{size[1]} {kind}", mode, [(k, got[k], ref[k], yards[k]) for k in ref])
    # the unfolded route of the same node, its g the kernels' formula as one fp32 torch expression: within the same bound
    m.zero_grad()
    y2 = m(xd, *size)
    (y2 * V.kernel_formula_fp32(y, hrd, kind)).sum().backward()
    assert m.last_route == "hip_train" and torch.equal(y2.detach(), y)
    unfolded = _param_grads(m)
    hold_rounded("resize fold vs unfolded", f"{_id(key)} -> {size[0]}x{size[1]} {kind}", mode, [(k, got[k], unfolded[k], yards[k]) for k in ref])
    # two equal folded steps: equal bits; 0.25 x the loss: exactly 0.25 x the gradients
    _, loss2, again = fold()
    assert torch.equal(loss, loss2) and all(torch.equal(got[k], again[k]) for k in ref)
    _, _, quarter = fold(0.25)
    assert all(torch.equal(quarter[k], 0.25 * got[k]) for k in ref) and any(bool(got[k].abs().max() > 0) for k in ref)
    # hot_resize_fold off: the same call does not fold (the parent's behaviour), and gives the unfolded route's bits
    m.hot_resize_fold = False
    m.zero_grad()
    y3 = m(xd, *size)
    loss3 = crit(y3, hrd)
    assert m.last_route == "hip_train" and not _folded(loss3) and torch.equal(y3.detach(), y)
    m.hot_resize_fold = True


# ---- train_step -------------------------------------------------------------------------------------------------------------------------
STEP_KEY = (8, 2, 2, 9, 17)


def _trained(m):
    return [(k, q) for k, q in m.named_parameters() if not k.startswith("skip.")]


def _adam(m, **kw):
    from mobilesuperresolution_amd import training as TR
    return TR.Adam([q for _, q in _trained(m)], **kw)


def _fresh(mode, state=None, key=STEP_KEY, **attrs):
    m = _module(R.rounded_case(*key), mode, **attrs)
    if state is not None:
        m.load_state_dict(state, strict=False)
    return m


def _clip(key=STEP_KEY):
    return R.rounded_case(*key)["x"].float().unsqueeze(0).to(DEV)


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("size", [(41, 77), (20, 31)], ids=_id)
def test_train_step_against_the_folded_loop(size, mode, kind):
    """One step from a fresh training.Adam with beta1 = 0, so that exp_avg is the fp32 gradient the step used (tests/test_gpu_clip_step.py),
    by train_step and by the loop folded criterion + loss.backward() + training.Adam.step() from the same state.  Both gradients are
    held to the float64 reference of the SAME state (fed the float64 loss gradient of each route's own sr, carried through
    clip_step_ref's weight-norm backward) by parity_kit.bound on the ATen (fp32, TF32 off) / rounding-point (bf16) yardstick, weight_g /
    weight_v widened by the row's fp32 chain: the two routes then agree within twice that bound, which is asserted too, for the
    gradients and -- Adam's first step being lr x sign(g) where |g| >> eps -- for the parameters wherever both gradients are far
    from zero."""
    case, n, nb = R.rounded_case(*STEP_KEY), STEP_KEY[2], STEP_KEY[1]
    x, xd = case["x"].float(), _clip()
    hr = _hr(n, size)
    hrd = hr.view(1, n, 3, *size).to(DEV)
    a = _fresh(mode, hot_resize=True, hot_resize_fold=True)
    sd0 = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
    opt_a = _adam(a, lr=1e-4, betas=(0.0, 0.999))
    assert a.train_step_reason(xd, hrd, opt_a) is None
    sr_a = torch.full_like(hrd, NAN)
    loss_a = a.train_step(xd, hrd, opt_a, criterion=kind, sr_out=sr_a)
    assert a.last_route == "hip_train_step" and loss_a.dim() == 0 and loss_a.dtype == torch.float32 and loss_a.grad_fn is None
    assert all(q.grad is None for q in a.parameters()) and len(opt_a.state) == len(_trained(a))
    assert all(float(opt_a.state[q]["step"]) == 1.0 for _, q in _trained(a))
    assert not bool(torch.isnan(sr_a).any())
    # sr_out is the hot_resize forward of the blobs the step itself packed, bit for bit (the same kernels on the same operands)
    from mobilesuperresolution_amd import hotpath as HP
    from mobilesuperresolution_amd.models import clip_train as CT
    st = a._fn_step
    scratch = torch.empty((3, n, 9, 17, P.FN_C), dtype=a.hot_dtype, device=DEV)
    own = torch.full_like(sr_a, NAN)
    HP.fn_net_fwd_sized(CT.frames_of(xd), st["blobs"][0], st["offs"], st["blobs"][2], scratch, own, 3 * size[0] * size[1], _resize((9, 17), size),
                        nb)
    assert torch.equal(sr_a, own), "sr_out: the sized forward of the step's own blobs"
    ga ={k: opt_a.state[q]["exp_avg"].detach().double().cpu() for k, q in _trained(a)}
    # the loop
    b = _fresh(mode, state=sd0, **FLAGS)
    opt_b = _adam(b, lr=1e-4, betas=(0.0, 0.999))
    y = b(xd, *size)
    loss_b = _criterion(kind)(y, hrd)
    assert _folded(loss_b) and b.last_route == "hip_train"
    loss_b.backward()
    opt_b.step()
    gb = {k: opt_b.state[q]["exp_avg"].detach().double().cpu() for k, q in _trained(b)}
    # losses: each within the chain bound of the float64 mean over its own sr
    from mobilesuperresolution_amd import hotpath as HP
    items = n * 4
    tol = V.chain_length(kind, items, min(items, HP.fn_bwd_wgs(n, 9, 17)), owner_adds(9, 17, size)) * 2.0 ** -24
    for tag, loss, sr in (("train_step", loss_a, sr_a), ("loop", loss_b.detach(), y.detach())):
        want = V.loss_value(sr.cpu().view(n, 3, *size), hr, kind).item()
        err = abs(loss.item() - want) / want
        print(f"resize fold step | -> {size} {mode} {kind} | {tag} loss {loss.item():.8f} float64 {want:.8f} | rel err {err:.2e} | bound {tol:.2e}")
        assert err <= tol
    # gradients
    p = R.effective(sd0, nb)

    def reference(sr, rnd=None):
        gout = V.loss_grad(sr.cpu().view(n, 3, *size), hr, kind)
        fw = R.forward(x, p, rnd=rnd)
        up = _up_backward(fw["f"], p["up_w"].double(), p["up_b"].double(), gout, size, rnd=rnd)
        grads = T.backward(x, p, None, rnd=rnd, df=up["df"])["grads"]
        grads.update(up_w=up["up_w"], up_b=up["up_b"])
        return gout, S.single_param_grads(sd0, nb, grads)

    gout, ref = reference(sr_a)
    assert set(ref) == set(ga)
    if mode == "fp32":
        with _tf32_off():
            other = _fresh(mode, state=sd0)
            (other(xd, *size)[0] * gout.float().to(DEV)).sum().backward()
            assert other.last_route == "aten"
            yard = {k: q.grad.detach().double().cpu() for k, q in _trained(other)}
    else:
        _, yard = reference(sr_a, rnd=R.bf16_round)
    _, ref_b = reference(y.detach())
    bad, checked = [], 0
    lr, eps = 1e-4, 1e-8
    pa, pb = dict(_trained(a)), dict(_trained(b))
    for k in ref:
        e_ref = rel_max(yard[k], ref[k])
        row = S.row_len_of(k, sd0)
        if row is not None:
            e_ref += S.wn_chain_length(row) * 2.0 ** -24
        t = bound(mode, e_ref)
        between = 2 * t + rel_max(ref_b[k], ref[k])             # each route within t of its reference; the references' own distance
        ea, eb, eab = rel_max(ga[k], ref[k]), rel_max(gb[k], ref_b[k]), rel_max(ga[k], gb[k])
        # the parameters: Adam's first step is lr g / (|g| + eps).  Where both |g| exceed `floor` -- twice the gap the bound above
        # leaves between the routes, and 1e-4 -- the signs agree and the two steps differ by at most lr 2 eps / floor, plus the fp32
        # rounding of the two updated parameters
        scale = ref[k].abs().max().item()
        floor = max(1e-4, 2 * between * scale)
        far = (ga[k].abs() > floor) & (gb[k].abs() > floor)
        qa, qb = pa[k].detach().double().cpu(), pb[k].detach().double().cpu()
        moved = (qa - qb).abs()[far].max().item() if bool(far.any()) else 0.0
        ptol = lr * 2 * eps / floor + 2 * 2.0 ** -24 * max(1.0, qa.abs().max().item())
        checked += int(far.sum())
        print(f"resize fold step | -> {size} {mode} {kind} | {k} | yardstick {e_ref:.2e} | train_step {ea:.2e} | loop {eb:.2e} | "
              f"between {eab:.2e} | bound {t:.2e} | parameters {moved:.2e} of {int(far.sum())} | bound {ptol:.2e}")
        if not (ea <= t and eb <= t and eab <= between and moved <= ptol):
            bad.append((k, ea, eb, eab, t, moved, ptol))
        assert not torch.equal(pa[k].detach().cpu(), sd0[k])
    assert not bad, bad
    assert checked > 0 and any(bool(g.abs().max() > 0) for g in ga.values())


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("size", [(41, 77), (20, 31)], ids=_id)
@pytest.mark.parametrize("key", [STEP_KEY, (32, 1, 2, 9, 17), (20, 2, 3, 9, 17)], ids=_id)
def test_train_step_sr_out_is_the_no_grad_forward(key, size, mode):
    """sr_out against the model's own no_grad hot_resize forward from the same state, torch.equal, in both dtypes.  The two share every
    network kernel; who forms w = g v / |v| differs -- torch._weight_norm in front of the inference route, the step's own kernel inside
    the call -- so the sized step forms it in torch's arithmetic (clip_wn_fwd_aten_kernel; rows of 72, 180 and 288 elements here, the
    encoder's 27).  The figures are printed before the assertion."""
    n = key[2]
    xd = _clip(key)
    hrd = _hr(n, size).view(1, n, 3, *size).to(DEV)
    m = _fresh(mode, key=key, hot_resize=True, hot_resize_fold=True)
    with torch.no_grad():
        plain = m(xd, *size).clone()
        assert m.last_route == "hip"
    sr = torch.full_like(hrd, NAN)
    m.train_step(xd, hrd, _adam(m, lr=1e-4), sr_out=sr)
    differ = int((sr != plain).sum())
    gap = (sr.double() - plain.double()).abs().max().item() / plain.double().abs().max().item()
    print(f"resize fold step | {_id(key)} -> {size} {mode} | sr_out vs the no_grad forward: {differ} of {sr.numel()} elements differ, rel max {gap:.2e}")
    assert torch.equal(sr, plain)


@pytest.mark.parametrize("mode", DTYPES)
def test_train_step_three_steps_twice_and_the_x4_size(mode):
    xd = _clip()
    n = STEP_KEY[2]

    def three(size, **attrs):
        m = _fresh(mode, **attrs)
        opt = _adam(m, lr=1e-3)
        hrd = _hr(n, size).view(1, n, 3, *size).to(DEV)
        losses = [m.train_step(xd, hrd, opt).clone() for _ in range(3)]
        assert m.last_route == "hip_train_step" and all(q.grad is None for q in m.parameters())
        return m, opt, losses

    for size in ((41, 77), (20, 31)):
        (a, opt_a, la), (b, _, lb) = three(size, hot_resize=True, hot_resize_fold=True), three(size, hot_resize=True, hot_resize_fold=True)
        assert all(torch.equal(u, v) for u, v in zip(la, lb)) and la[2].item() != la[0].item()
        assert all(torch.equal(u, v) for (_, u), (_, v) in zip(_trained(a), _trained(b)))
        assert all(bool(torch.isfinite(v)) for v in la) and all(float(opt_a.state[q]["step"]) == 3.0 for _, q in _trained(a))
    # (4H, 4W): the x4 entry point, flag or no flag
    (a, opt_a, la), (b, opt_b, lb) = three((36, 68), hot_resize=True, hot_resize_fold=True), three((36, 68))
    assert "_fn_resize" not in a.__dict__
    assert all(torch.equal(u, v) for u, v in zip(la, lb)) and all(torch.equal(u, v) for (_, u), (_, v) in zip(_trained(a), _trained(b)))
    assert len(opt_a.state) == len(opt_b.state) == len(_trained(a))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_flag_off_refuses_with_todays_text_and_touches_nothing():
    from mobilesuperresolution_amd import _lib as L
    xd, n = _clip(), STEP_KEY[2]
    hrd = _hr(n, (41, 77)).view(1, n, 3, 41, 77).to(DEV)
    why = "hr is not fp32 (B, N, 3, 4H, 4W) on the input's device"
    for attrs in (dict(), dict(hot_resize=True), dict(hot_resize_fold=True), dict(hot_training=True, hot_resize=True)):
        m = _fresh("fp32", **attrs)
        sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
        opt = _adam(m, lr=1e-3)
        assert m.train_step_reason(xd, hrd, opt) == why
        with pytest.raises(L.HotpathError) as info:
            m.train_step(xd, hrd, opt)
        assert why in str(info.value)
        assert len(opt.state) == 0 and all(torch.equal(v, sd0[k]) for k, v in m.state_dict().items())
    # both flags: an hr on the host, of another dtype or of another clip is still refused
    m = _fresh("fp32", hot_resize=True, hot_resize_fold=True)
    opt = _adam(m, lr=1e-3)
    for hr in (hrd.cpu(), hrd.double(), hrd[:, :1], hrd[:, :, :2]):
        reason = m.train_step_reason(xd, hr, opt)
        assert reason == "hr is not fp32 (B, N, 3, OH, OW) on the input's device"
        with pytest.raises(L.HotpathError):
            m.train_step(xd, hr, opt)
    assert len(opt.state) == 0
    with pytest.raises(ValueError):
        m.train_step(xd, hrd, opt, sr_out=torch.empty(1, n, 3, 36, 68, device=DEV))


@pytest.mark.parametrize("mode", DTYPES)
def test_entry_points_refuse_bad_arguments_untouched(mode):
    from mobilesuperresolution_amd import _lib as L
    net = TrainNet(R.exact_case(32, 1, 1, 3, 3), DTYPES[mode])
    size = (14, 11)
    rz = _resize((3, 3), size)
    sr, hr = torch.zeros(1, 3, *size, device=DEV), torch.ones(1, 3, *size, device=DEV)
    loss_part = torch.full((net.wgs,), NAN, dtype=torch.float32, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        bufs = (net.acts, net.ts, net.out, net.gs, net.parts, net.grads, loss_part)
        return all(bool(torch.isnan(t.float()).all()) for t in bufs) and bool((net.masks == -1).all())

    call = lambda **kw: _loss_call(net, sr, kw.pop("hr", hr), kw.pop("kind", "l1"), size, kw.pop("loss_part", loss_part),
                                   **{"stages": P.FN_BWD_ALL, "rz": rz, **kw})
    for kw in (dict(oh=P.FN_MAX_OUT + 1), dict(ow=P.FN_MAX_OUT + 1)):
        assert call(**kw) == -1 and untouched(), kw
    nothing = torch.empty(0)                                              # data_ptr() == 0: a NULL argument
    assert nothing.data_ptr() == 0
    for kw in (dict(ty=nothing), dict(ly=nothing), dict(tx=nothing), dict(lx=nothing), dict(hr=nothing), dict(loss_part=nothing), dict(kind=0),
               dict(kind=3), dict(oh=0), dict(ow=-1), dict(stages=0), dict(stages=P.FN_BWD_ALL & ~P.FN_BWD_UP), dict(stages=16)):
        assert call(**kw) == -2 and untouched(), kw
    # the one-call step: the same refusals before anything is launched (its table is never read: the resize is checked first)
    lib, ptr = L.lib(), lambda t: t.data_ptr()
    step = L.ClipStep()

    def step_call(oh=size[0], ow=size[1], ty=rz[2], kind=1):
        import ctypes
        return lib.sr_fn_net_train_step_sized(ctypes.byref(step), ptr(net.x), ptr(hr), kind, net.offs, ptr(net.acts), ptr(net.ts), ptr(net.masks),
                                              ptr(sr), oh, ow, ptr(ty), ptr(rz[3]), ptr(rz[4]), ptr(rz[5]), ptr(net.gs), ptr(net.parts), net.wgs,
                                              ptr(net.grads), ptr(loss_part), net.c, net.nb, net.n, net.h, net.w, L.DTYPE_CODE[net.dtype],
                                              L.stream_ptr())

    assert step_call(oh=P.FN_MAX_OUT + 1) == -1 and step_call(ow=P.FN_MAX_OUT + 1) == -1 and untouched()
    assert step_call(ty=nothing) == -2 and step_call(kind=0) == -2 and step_call(oh=0) == -2 and untouched()
    assert step_call() == -2 and untouched(), "an empty parameter table"
    # and the call itself
    net.fwd()
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(net.grads).any()) and not bool(torch.isnan(loss_part[:1]).any())
