"""One whole training step of the two wide video models (BasicVSR_origin and MotionVectorVSR at 24 < F <= 64 under `hot_training`):
forward, the Charbonnier loss, backward -- composed in plain torch on the CPU from the references the kernels are already pinned to,
with the indexing of the Python glue that wires the kernels together (the paired batch [backward-time loop | forward-time loop], the
per-step states and their halves, the per-clip views of frames, flows and cotangents).  Nothing of the package is used here.

  propagation      trunk_ref.step_ref per half of the paired batch (rnd = the trunks' rounding points); the warp in front of it is
                   warp_ref.warp_ref in float64 and warp_ref.grid_sample_warp, the op as the reference model states it, in float32
  origin recon     forward: recon_ref.conv_ref layer by layer (conv_hr, which has no kind of its own there, with the same hooks:
                   operands and the stored image); backward: recon_bwd_ref.stage_run over the stored images, the loop of
                   recon_bwd_ref.chain_backward
  mv recon         recon_ref.mv_run over the whole clip, frame-major as the kernel takes it, forward and backward
  loss             _charbonnier, differentiated by autograd in the step's dtype

Modes:  dtype=float64, hot=ident            the reference
        dtype=float32, hot=ident            the fp32 yardstick
        dtype=float64, hot=bf16_round       the bf16 yardstick (rnd = bf16_round in the trunks)

What the bf16 composition rounds, and where: in the trunks the input [frame | warped state], the weights and biases, a_0, every t_i
and a_{i+1}, and backward dz of the first conv, every gt_i and ga_i and the gradient of the trunk's whole input (trunk_ref.trunk_ref);
in the reconstructions every operand, every stored image, u, dD, dz / dpre and every stored gradient image including the two state
gradients (recon_ref.conv_ref, recon_bwd_ref.stage_run, recon_ref.mv_run).  The state a trunk hands on is a_nb, rounded once; its
gradient is the sum of the reconstruction's (rounded) state gradient and the next step's warp gradient, rounded once as ga_nb.  The
output, the loss, its cotangent and every parameter gradient stay unrounded, as the fp32 buffers they are.

Two families of cases (case(positive=)): bf16 is held on cases with both signs in front of every mask; fp32 on twins whose biases keep
every masked pre-activation of the float64 step at least MARGIN above zero, because 8 fp32 yardsticks are a few 1e-6 while one
LeakyReLU mask that an fp32 sum signs differently from float64 moves a gradient by 1e-4.

`defect=` seeds one wiring mistake into the indexing (DEFECTS): tests/test_wide_model_ref_host.py shows on the reference alone that
each of them moves a tensor far outside the bound the GPU suite applies, i.e. that the cases tell clips and halves apart.

Also here: the restatement of both models in ATen (_aten_model) and the loss (_charbonnier) that the whole-model GPU suites share.
"""
import functools

import torch
import torch.nn.functional as F

from tests import recon_bwd_ref as B
from tests import recon_ref as R
from tests import trunk_ref as T
from tests.parity_kit import bf16_round, leaf, rel_max, seed
from tests.warp_ref import grid_sample_warp, warp_ref

_seed = functools.partial(seed, 97531, 5)

ORIGIN_RECON = tuple(f"{l}.{p}" for l in ("fusion", "upconv1", "upconv2", "conv_hr", "conv_last") for p in ("weight", "bias"))
MV_RECON = ("fusion.weight", "fusion.bias", "conv_last.weight", "conv_last.bias")
RECON = {"origin": ORIGIN_RECON, "mv": MV_RECON}
TRUNKS = ("backward_trunk", "forward_trunk")
DEFECTS = ("halves_swapped", "clip0_frame", "clip0_flow", "clip0_cotangent", "dense_stride", "flows_not_flipped")


# ---- the two models restated in ATen (shared by the whole-model GPU suites) -------------------------------------------------------
def _aten_trunk(p, prefix, x, nb):
    y = F.leaky_relu(F.conv2d(x, p[prefix + "main.0.weight"], p[prefix + "main.0.bias"], padding=1), 0.1)
    for i in range(nb):
        q = f"{prefix}main.2.{i}."
        t = F.relu(F.conv2d(y, p[q + "conv1.weight"], p[q + "conv1.bias"], padding=1))
        y = y + F.conv2d(t, p[q + "conv2.weight"], p[q + "conv2.bias"], padding=1)
    return y


def _aten_warp(x, flow):
    _, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=x.dtype, device=x.device), torch.arange(w, dtype=x.dtype, device=x.device),
                            indexing="ij")
    vx = 2.0 * (gx + flow[:, 0]) / max(w - 1, 1) - 1.0
    vy = 2.0 * (gy + flow[:, 1]) / max(h - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((vx, vy), 3), mode="bilinear", padding_mode="zeros", align_corners=True)


def _aten_model(kind, p, x, ff, fb, nb, f, size):
    """the whole model restated in ATen in the dtype of `p` (propagation loops of basicvsr_arch_origin.py:61-82 / mvvsr_arch.py:72-93,
    then the model's reconstruction)"""
    b, n, _, h, w = x.shape
    feats = {}
    for name, flows, order in (("backward", fb, range(n - 1, -1, -1)), ("forward", ff, range(n))):
        feat, res = x.new_zeros(b, f, h, w), {}
        for k, i in enumerate(order):
            if k:
                feat = _aten_warp(feat, flows[:, i if name == "backward" else i - 1])
            feat = _aten_trunk(p, name + "_trunk.", torch.cat([x[:, i], feat], 1), nb)
            res[i] = feat
        feats[name] = res
    lrelu = lambda t: F.leaky_relu(t, 0.1)
    conv = lambda name, t, pad: F.conv2d(t, p[name + ".weight"], p[name + ".bias"], padding=pad)
    outs = []
    for i in range(n):
        out = lrelu(conv("fusion", torch.cat([feats["backward"][i], feats["forward"][i]], 1), 0))
        if kind == "origin":
            out = lrelu(F.pixel_shuffle(conv("upconv1", out, 1), 2))
            out = lrelu(F.pixel_shuffle(conv("upconv2", out, 1), 2))
            out = conv("conv_last", lrelu(conv("conv_hr", out, 1)), 1)
            out = out + F.interpolate(x[:, i], scale_factor=4, mode="bilinear", align_corners=False)
            out = F.interpolate(out, size=size, mode="bilinear")
        else:
            out = F.conv_transpose2d(out, p["conv_last.weight"], p["conv_last.bias"], stride=4)
            out = F.interpolate(out, size=size, mode="bilinear") + F.interpolate(x[:, i], size=size, mode="bilinear", align_corners=False)
        outs.append(out)
    return torch.stack(outs, 1)


def _charbonnier(out, target):
    return torch.sqrt((out - target) ** 2 + 1e-6).mean()


def trunk_keys(trunk, nb):
    return [f"{trunk}.{k}" for k in T.param_names(nb)]


def group_grads(kind, nb, grad_of):
    """{group: gradient}: the two trunks flat in state_dict order, then the reconstruction tensors; grad_of(name) -> tensor"""
    grads = {tr: torch.cat([grad_of(k).reshape(-1) for k in trunk_keys(tr, nb)]) for tr in TRUNKS}
    grads.update({k: grad_of(k) for k in RECON[kind]})
    return grads


def aten_step(kind, params, x, ff, fb, target, nb, f, dtype):
    """the ATen restatement's step in `dtype`: (output, {group: gradient})"""
    p = {k: leaf(v, dtype) for k, v in params.items()}
    out = _aten_model(kind, p, x.to(dtype), ff.to(dtype), fb.to(dtype), nb, f, tuple(target.shape[-2:]))
    _charbonnier(out, target.to(dtype)).backward()
    return out.detach(), group_grads(kind, nb, lambda k: p[k].grad)


# ---- the glue's indexing, with its seeded defects -----------------------------------------------------------------------------------
def _clip0(b):
    """clip 1 read at clip 0's offset"""
    return [0, 0] + list(range(2, b))


def frame_view(x, i, defect=None):
    """x[:, i] of the (b, n, 3, h, w) clips: one frame of every clip, batch stride n * 3 * h * w"""
    b, n = x.shape[:2]
    if defect == "clip0_frame":
        return x[_clip0(b), i]
    if defect == "dense_stride":                          # clip c at c dense strides (3 h w) behind clip 0's frame i
        return x.reshape(b * n, *x.shape[2:])[[i + c for c in range(b)]]
    return x[:, i]


def _warp(state, flow, dtype):
    if dtype == torch.float64:
        return warp_ref(state, flow.permute(0, 2, 3, 1))
    return grid_sample_warp(state, flow.permute(0, 2, 3, 1))


def propagate(pb, pf, x, ff, fb, nb, rnd=None, defect=None, inters=None):
    """the paired propagation: the state of every frame step k, (2b, F, h, w) = [backward-time loop at frame n - 1 - k | forward-time
    loop at frame k].  pb, pf: the two trunks' parameter lists (trunk_ref's order).  inters: a list that receives (trunk index,
    trunk_ref's intermediates) of every trunk call."""
    b, n = x.shape[:2]
    if defect == "clip0_flow":
        ff, fb = ff[_clip0(b)], fb[_clip0(b)]
    fl = torch.cat([fb if defect == "flows_not_flipped" else fb.flip(1), ff], 0) if n > 1 else None
    state, steps = None, []
    for k in range(n):
        frames = (frame_view(x, n - 1 - k, defect), frame_view(x, k, defect))
        prev = _warp(state, fl[:, k - 1], x.dtype) if k > 0 else None
        halves = []
        for t, (fr, sl, p) in enumerate(zip(frames, (slice(0, b), slice(b, None)), (pb, pf))):
            inter = {} if inters is not None else None
            halves.append(T.step_ref(fr, None if prev is None else prev[sl], None, p, nb, inter, rnd))
            if inters is not None:
                inters.append((t, inter))
        state = torch.cat(halves, 0)
        steps.append(state)
    return steps


class _Cotangent(torch.autograd.Function):
    """identity; the cotangent of clip 1 read at clip 0's offset"""

    @staticmethod
    def forward(ctx, out):
        return out.view_as(out)

    @staticmethod
    def backward(ctx, g):
        return g[_clip0(g.shape[0])]


# ---- the reconstructions as autograd nodes over the pinned references ------------------------------------------------------------
def origin_recon_forward(p, fb, ff, frame, dtype=torch.float64, hot=R.ident):
    """(out, fused, up1, up2, hr): recon_ref.conv_ref layer by layer, the stored images in the hot precision"""
    lay = lambda kind, name, **kw: R.conv_ref(dict(kind=kind, w=p[name + ".weight"], b=p[name + ".bias"], **kw), dtype, hot)
    fused = lay("fusion", "fusion", fb=fb, ff=ff)
    up1 = lay("up1", "upconv1", x=fused)
    up2 = lay("up2", "upconv2", x=up1)
    t = lambda v: hot(v.to(dtype))
    hr = hot(R.lrelu(F.conv2d(t(up2), t(p["conv_hr.weight"]), t(p["conv_hr.bias"]), padding=1)))
    return lay("last", "conv_last", x=hr, frame=frame), fused, up1, up2, hr


def origin_recon_backward(p, fb, ff, images, g, dtype=torch.float64, hot=R.ident):
    """recon_bwd_ref.chain_backward's loop on the STORED images of the forward: {parameter name: gradient}, 'dfb', 'dff'"""
    fused, up1, up2, hr = images
    res, gin = {}, g.to(dtype)
    for st, a, x in ((16, None, hr), (8, None, up2), (4, up2, up1), (2, up1, fused), (1, fused, torch.cat([fb, ff], 1).to(dtype))):
        case = dict(stage=st, gin=gin, x=x, w=p[B.NAMES[st] + ".weight"])
        if a is not None:
            case["a"] = a
        r = B.stage_run(case, dtype, hot)
        res[B.NAMES[st] + ".weight"], res[B.NAMES[st] + ".bias"], gin = r["dW"], r["db"], r["dx"]
    f = fb.shape[1]
    res["dfb"], res["dff"] = gin[:, :f], gin[:, f:]
    return res


class _OriginRecon(torch.autograd.Function):
    """one frame of every clip: (fb, ff, frame, hot, the ten parameters) -> out (b, 3, 4h, 4w)"""

    @staticmethod
    def forward(ctx, fb, ff, frame, hot, *ps):
        p = dict(zip(ORIGIN_RECON, ps))
        out, *images = origin_recon_forward(p, fb, ff, frame, fb.dtype, hot)
        ctx.keep = (p, fb, ff, images, hot)
        return out

    @staticmethod
    def backward(ctx, g):
        p, fb, ff, images, hot = ctx.keep
        r = origin_recon_backward(p, fb, ff, images, g, fb.dtype, hot)
        return (r["dfb"], r["dff"], None, None) + tuple(r[k] for k in ORIGIN_RECON)


def _mv_case(fb, ff, xs, ps):
    return dict(zip(("w_fu", "b_fu", "w_last", "b_last"), ps), fb=fb, ff=ff, x=xs)


class _MvRecon(torch.autograd.Function):
    """the whole clip, frame-major: (fb, ff (n b, F, h, w), frames (n b, 3, h, w), hot, the four parameters) -> out (n b, 3, 4h, 4w)"""

    @staticmethod
    def forward(ctx, fb, ff, xs, hot, *ps):
        ctx.keep = (fb, ff, xs, hot, ps)
        return R.mv_run(_mv_case(fb, ff, xs, ps), fb.dtype, hot)["out"]

    @staticmethod
    def backward(ctx, g):
        fb, ff, xs, hot, ps = ctx.keep
        r = R.mv_run(dict(_mv_case(fb, ff, xs, ps), g=g), fb.dtype, hot)
        f = fb.shape[1]
        return (r["dc"][:, :f], r["dc"][:, f:], None, None, r["dW_fu"], r["db_fu"], r["dW_last"], r["db_last"])


# ---- the whole step --------------------------------------------------------------------------------------------------------------
def _step(kind, params, x, ff, fb, target, nb, f, dtype, hot, rnd, defect):
    assert defect is None or defect in DEFECTS, defect
    if rnd is None and hot is not R.ident:
        rnd = hot
    p = {k: leaf(params[k], dtype) for k in trunk_keys(TRUNKS[0], nb) + trunk_keys(TRUNKS[1], nb) + list(RECON[kind])}
    x, ff, fb, target = (t.detach().to(dtype) for t in (x, ff, fb, target))
    b, n, _, h, w = x.shape
    assert p[TRUNKS[0] + ".main.0.weight"].shape[0] == f
    steps = propagate([p[k] for k in trunk_keys(TRUNKS[0], nb)], [p[k] for k in trunk_keys(TRUNKS[1], nb)], x, ff, fb, nb, rnd, defect)
    first, second = (slice(b, None), slice(0, b)) if defect == "halves_swapped" else (slice(0, b), slice(b, None))
    recon = [p[k] for k in RECON[kind]]
    if kind == "origin":
        out = torch.stack([_OriginRecon.apply(steps[n - 1 - i][first], steps[i][second], frame_view(x, i, defect), hot, *recon)
                           for i in range(n)], 1)
    else:
        sfb = torch.cat([steps[n - 1 - i][first] for i in range(n)], 0)
        sff = torch.cat([steps[i][second] for i in range(n)], 0)
        xs = torch.cat([frame_view(x, i, defect) for i in range(n)], 0)
        out = _MvRecon.apply(sfb, sff, xs, hot, *recon).view(n, b, 3, 4 * h, 4 * w).transpose(0, 1)
    if defect == "clip0_cotangent":
        out = _Cotangent.apply(out)
    _charbonnier(out, target).backward()
    return out.detach().contiguous(), group_grads(kind, nb, lambda k: p[k].grad)


def origin_step(params, x, flows_forward, flows_backward, target, nb, f, dtype=torch.float64, hot=R.ident, rnd=None, defect=None):
    """BasicVSR_origin(f, nb) with given flows: x (b, n, 3, h, w), flows (b, n - 1, 2, h, w), target (b, n, 3, 4h, 4w); params by
    state_dict name.  Returns (output, {group: gradient}): backward_trunk and forward_trunk flat, then ORIGIN_RECON."""
    return _step("origin", params, x, flows_forward, flows_backward, target, nb, f, dtype, hot, rnd, defect)


def mv_step(params, x, flows_forward, flows_backward, target, nb, f, dtype=torch.float64, hot=R.ident, rnd=None, defect=None):
    """MotionVectorVSR(f, nb) the same way (the model takes flows_forward = mv[:, 1:], flows_backward = -flows_forward); groups: the
    two trunks flat, then MV_RECON"""
    return _step("mv", params, x, flows_forward, flows_backward, target, nb, f, dtype, hot, rnd, defect)


STEP = {"origin": origin_step, "mv": mv_step}
MODES = {"f64": (torch.float64, R.ident), "fp32": (torch.float32, R.ident), "bf16": (torch.float64, bf16_round)}


# ---- the cases of tests/test_gpu_wide_batch.py ---------------------------------------------------------------------------------------
KINDS = ("origin", "mv")
WIDTHS = ((40, 1), (64, 2))                              # (F, nb)
BATCHES = (2, 3)
FRAMES, HEIGHT, WIDTH = 3, 18, 20                        # partial 16 x 16 tiles in both directions
# motion vector (x, y) per clip and frame (frame 0's is never read) and the target's offset per clip
SHIFTS = (((0.0, 0.0), (1.5, -1.0), (-7.0, 5.0)), ((0.0, 0.0), (-6.0, 4.0), (2.0, 1.5)), ((0.0, 0.0), (3.0, -6.0), (-1.0, -1.5)))
TARGET_OFFSETS = (0.0, 1.0, 0.5)


def recon_shapes(kind, f):
    if kind == "origin":
        return dict(zip(ORIGIN_RECON, ((f, 2 * f, 1, 1), (f,), (4 * f, f, 3, 3), (4 * f,), (256, f, 3, 3), (256,), (64, 64, 3, 3), (64,),
                                       (3, 64, 3, 3), (3,))))
    return dict(zip(MV_RECON, ((2 * f, 2 * f, 1, 1), (2 * f,), (2 * f, 3, 5, 5), (3,))))


MARGIN = 0.25


def pre_minima(kind, params, x, ff, fb, nb):
    """{bias name: (C,) minimum over the step of the pre-activation in front of every LeakyReLU / ReLU, per output channel of its
    conv}, in float64: the first conv and every conv1 of both trunks, and the masked layers of the reconstruction"""
    p = {k: v.double() for k, v in params.items()}
    x, ff, fb = x.double(), ff.double(), fb.double()
    b, n = x.shape[:2]
    inters, mins = [], {}

    def put(name, t):
        m = t.amin((0, 2, 3))
        mins[name] = torch.minimum(mins[name], m) if name in mins else m
    pre = lambda img: torch.where(img > 0, img, img / R.SLOPE)        # the stored LeakyReLU image back to its pre-activation
    with torch.no_grad():
        steps = propagate([p[k] for k in trunk_keys(TRUNKS[0], nb)], [p[k] for k in trunk_keys(TRUNKS[1], nb)], x, ff, fb, nb,
                          inters=inters)
        for t, d in inters:
            put(f"{TRUNKS[t]}.main.0.bias", d["z0"])
            for i in range(nb):
                put(f"{TRUNKS[t]}.main.2.{i}.conv1.bias", d[f"z1_{i}"])
        for i in range(n):
            sfb, sff = steps[n - 1 - i][:b], steps[i][b:]
            if kind == "origin":
                _, fused, up1, up2, hr = origin_recon_forward(p, sfb, sff, x[:, i])
                put("fusion.bias", pre(fused))
                put("upconv1.bias", F.pixel_unshuffle(pre(up1), 2))
                put("upconv2.bias", F.pixel_unshuffle(pre(up2), 2))
                put("conv_hr.bias", pre(hr))
            else:
                put("fusion.bias", R.mv_run(_mv_case(sfb, sff, x[:, i], [p[k] for k in MV_RECON]))["pre"])
    return mins


def _raise_biases(kind, params, x, ff, fb, nb, margin):
    """raise biases, never weights, until every masked pre-activation of the float64 step is at least `margin`"""
    for _ in range(40):
        low = {k: (margin - m).clamp(min=0) for k, m in pre_minima(kind, params, x, ff, fb, nb).items()}
        if not any(bool((d > 0).any()) for d in low.values()):
            return params
        for k, d in low.items():
            params[k] = (params[k].double() + 1.5 * d).float()
    raise ValueError("wide case: the biases did not settle")


@functools.lru_cache(maxsize=None)
def case(kind, f, nb, b, positive=False):
    """seeded parameters (fan-in-sized weights, the first conv's state channels doubled so that the recurrence carries weight in the
    result; biases of both signs) and b clips that differ in kind, not only in noise, so that reading one clip's or one time step's
    slice for another's moves whole sums: every clip has its own frames; its motion vectors are a shift of their own per clip and
    time step (from a pixel to a third of the image, so the steps lose different parts of the state) plus half a pixel of noise; the
    target of clip 0 straddles the output, that of clip 1 lies above it and that of clip 2 half way, so the cotangents of the clips
    differ in sign pattern without cancelling each other in the gradient sums.  Cached: shared, not to be written to."""
    g = torch.Generator().manual_seed(_seed(KINDS.index(kind), f, nb, b))
    rn = lambda *s: torch.randn(*s, generator=g)
    params = {}
    for tr in TRUNKS:
        for k in range(1 + 2 * nb):
            ci = f + 3 if k == 0 else f
            name = trunk_keys(tr, nb)[2 * k][:-len(".weight")]
            params[name + ".weight"], params[name + ".bias"] = rn(f, ci, 3, 3) / (3.0 * ci ** 0.5), 0.1 * rn(f)
            if k == 0:
                params[name + ".weight"][:, 3:] *= 2.0
    for name, shape in recon_shapes(kind, f).items():
        if name.endswith(".bias"):
            params[name] = 0.1 * rn(*shape)
        elif kind == "mv" and name == "conv_last.weight":
            params[name] = rn(*shape) / shape[0] ** 0.5
        else:
            params[name] = rn(*shape) / (shape[2] * shape[1] ** 0.5)
    x = torch.rand(b, FRAMES, 3, HEIGHT, WIDTH, generator=g)
    shifts = torch.tensor(SHIFTS, dtype=torch.float32)[:b, :FRAMES]
    mv = shifts.view(b, FRAMES, 2, 1, 1) + 0.5 * rn(b, FRAMES, 2, HEIGHT, WIDTH)
    target = torch.rand(b, FRAMES, 3, 4 * HEIGHT, 4 * WIDTH, generator=g) + torch.tensor(TARGET_OFFSETS[:b]).view(b, 1, 1, 1, 1)
    if positive:
        for k in params:                                 # all-positive activations have a mean: gains below one keep the recurrence bounded
            if k.endswith(".weight"):
                params[k] = 0.3 * params[k]
        params = _raise_biases(kind, params, x, mv[:, 1:], -mv[:, 1:], nb, MARGIN)
    return dict(kind=kind, f=f, nb=nb, b=b, params=params, x=x, mv=mv, ff=mv[:, 1:], fb=-mv[:, 1:], target=target, positive=positive)


def run(kind, f, nb, b, mode="f64", defect=None, positive=False):
    c = case(kind, f, nb, b, positive)
    dtype, hot = MODES[mode]
    return STEP[kind](c["params"], c["x"], c["ff"], c["fb"], c["target"], nb, f, dtype, hot, defect=defect)


def tensors(res):
    """(name, tensor) of a step's result: the output, then every gradient group"""
    out, grads = res
    return [("out", out)] + list(grads.items())


POSITIVE = {"fp32": True, "bf16": False}                 # which family of cases a mode is held on


@functools.lru_cache(maxsize=None)
def reference(kind, f, nb, b, mode):
    """(case, float64 result, {tensor name: yardstick}) of the case `mode` is held on: the yardstick is the emulation's own rel_max
    from float64.  Cached per (model, f, nb, b, mode): shared, not to be written to."""
    pos = POSITIVE[mode]
    ref = run(kind, f, nb, b, positive=pos)
    emu = dict(tensors(run(kind, f, nb, b, mode, positive=pos)))
    return case(kind, f, nb, b, pos), ref, {k: rel_max(emu[k], v) for k, v in tensors(ref)}
