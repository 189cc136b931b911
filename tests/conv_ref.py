"""The two dense k x k implicit-GEMM families written out in plain torch, float64 on the CPU, plus the case generators of their
parity tests: SPyNet's 7x7 convolutions (csrc/spynet_conv.h: conv7_ref, basic_module_ref, spynet_ref) and the searched network's
residual block, tail and un-shuffle (csrc/result_block.h: rm_block_ref, rm_tail_ref, unshuffle_ref).  Nothing of the package or of
the oracle is used here: this is the outside reference the kernels are held against (tests/test_gpu_conv_ref.py).
tests/test_conv_ref_host.py pins it to fixtures G15 and G18 and to a shift-and-add loop, and checks on the CPU that every exact case
satisfies its exactness conditions.

Three families of cases (a case is a dict; 'kind' says which runner applies; 'ref' is check_exact()'s result):
  exact     dyadic data on which every reduction satisfies sum |terms| < 2^24 quanta of its lattice, so fp32 accumulation is exact
            in ANY order.  Dense cases: every weight +-2^k (none zero, so every tap and every input channel enters every output),
            inputs in {-1, 0, 1} times a per-channel power of two, pairwise different dyadic biases.  The exact value is stored
            rounded ONCE to the hot dtype: the reference rounds its float64 value to bf16 (round to nearest even) and the kernel has
            to return the same bits; check_exact() requires an element exactly on a bf16 tie wherever a bias lets one be made (a
            bias is moved until one exists).  Block cases: z is exactly 0 somewhere in the window (mask bit 0, y = x there),
            negative and positive elsewhere.  Tap-identity cases: one non-zero weight per output channel, so the output is a
            shifted copy of one input channel plus the bias and a failure names the tap.  Chain cases: the five layers of
            BasicModule as an integer network (sparse +-1 weights, biases fitted to the data so every activation is a small
            integer, per-channel power-of-two scales), every inter-layer tensor its own bf16 rounding.
  rounded   random normal data; the yardstick is emulate(): the same reference run in float32 on operands rounded where the
            kernels round.

The conditions named need_* / is_*, the roundings, the seed recipe and the bound of the rounded cases are tests/parity_kit.py's,
shared by all parity suites and pinned by tests/test_parity_kit_host.py.
"""
import functools
import math

import torch
import torch.nn.functional as F_

from tests.parity_kit import BIG, bf16_round, bf16_ties, chan_quantum, fail, is_bf16, is_fp32, lowbit, need_biases, need_sum, rel_max, seed

LAYERS = ((8, 32, True), (32, 64, True), (64, 32, True), (32, 16, True), (16, 2, False))     # BasicModule: (cin, cout, relu)
RM_CP = {2: 16, 3: 32, 4: 48}                                                                # rm_cp(R): 3 R^2 padded to 16


# ---- references: SPyNet ----------------------------------------------------------------------------------------------------
def conv7_ref(x, w, b, relu):
    y = F_.conv2d(x, w, b, padding=3)
    return torch.relu(y) if relu else y


def basic_module_ref(x, params, rnd=None, inter=None):
    """x (n, 8, h, w); params [w0, b0, .., w4, b4]: the five layers with ReLU between.  rnd: the rounding applied where the
    kernels round -- the input, the weights and the four inter-layer activations; the biases stay fp32 and the last output is
    not rounded.  inter: a list that receives the four inter-layer tensors."""
    r = rnd if rnd is not None else (lambda t: t)
    x = r(x)
    for i, (_, _, relu) in enumerate(LAYERS):
        x = conv7_ref(x, r(params[2 * i]), params[2 * i + 1], relu)
        if i < 4:
            x = r(x)
            if inter is not None:
                inter.append(x)
    return x


def spynet_param_names():
    return [f"basic_module.{lv}.basic_module.{i}.{p}" for lv in range(6) for i in (0, 2, 4, 6, 8) for p in ("weight", "bias")]


def _border_warp(x, flow):
    n, _, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(0, h, dtype=x.dtype), torch.arange(0, w, dtype=x.dtype), indexing="ij")
    vx = 2.0 * (gx + flow[:, 0]) / max(w - 1, 1) - 1.0
    vy = 2.0 * (gy + flow[:, 1]) / max(h - 1, 1) - 1.0
    return F_.grid_sample(x, torch.stack((vx, vy), dim=3), mode="bilinear", padding_mode="border", align_corners=True)


def spynet_ref(ref, supp, state_dict, rnd=None, dtype=torch.float64):
    """SpyNet.forward of models/spynet_arch.py in `dtype`: resize to a multiple of 32, normalisation, five average poolings, per
    level the x2 bilinear (align_corners=True) upsampling of the flow, the border-padded warp of the support image and
    basic_module_ref, then the resize back and the rescale.  rnd is handed to basic_module_ref."""
    sd = {k: v.detach().to(dtype) for k, v in state_dict.items()}
    ref, supp = ref.to(dtype), supp.to(dtype)
    h, w = ref.shape[2:]
    wf, hf = math.floor(math.ceil(w / 32.0) * 32.0), math.floor(math.ceil(h / 32.0) * 32.0)
    ref = F_.interpolate(ref, size=(hf, wf), mode="bilinear", align_corners=False)
    supp = F_.interpolate(supp, size=(hf, wf), mode="bilinear", align_corners=False)
    refs, supps = [(ref - sd["mean"]) / sd["std"]], [(supp - sd["mean"]) / sd["std"]]
    for _ in range(5):
        refs.insert(0, F_.avg_pool2d(refs[0], kernel_size=2, stride=2, count_include_pad=False))
        supps.insert(0, F_.avg_pool2d(supps[0], kernel_size=2, stride=2, count_include_pad=False))
    flow = refs[0].new_zeros(refs[0].shape[0], 2, refs[0].shape[2] // 2, refs[0].shape[3] // 2)
    for lv in range(6):
        up = F_.interpolate(flow, scale_factor=2, mode="bilinear", align_corners=True) * 2.0
        if up.shape[2] != refs[lv].shape[2]:
            up = F_.pad(up, [0, 0, 0, 1], mode="replicate")
        if up.shape[3] != refs[lv].shape[3]:
            up = F_.pad(up, [0, 1, 0, 0], mode="replicate")
        params = [sd[f"basic_module.{lv}.basic_module.{i}.{p}"] for i in (0, 2, 4, 6, 8) for p in ("weight", "bias")]
        flow = basic_module_ref(torch.cat([refs[lv], _border_warp(supps[lv], up), up], 1), params, rnd) + up
    flow = F_.interpolate(flow, size=(h, w), mode="bilinear", align_corners=False)
    scale = torch.tensor([float(w) / float(wf), float(h) / float(hf)], dtype=dtype).view(1, 2, 1, 1)
    return flow * scale


# ---- references: Result_Model ----------------------------------------------------------------------------------------------
def pack_mask(pos):
    """(n, C, h, w) bool -> (n, h, w) int64: bit c of a pixel's word = pos[:, c], as rm_conv_kernel packs its ReLU mask"""
    bits = torch.zeros(pos.shape[0], pos.shape[2], pos.shape[3], dtype=torch.int64)
    for c in range(pos.shape[1]):
        bits |= pos[:, c].long() << c
    return bits


def rm_block_ref(x, w, b, a, IN, k, gy=None, mask=None):
    """Block [IN, split = IN - a, k] on x (n, F, h, w): y = x, with x[:, a:IN] + relu(conv_k(x[:, a:IN], w) + b) on the window.
    The window is written as the kernels hold it, as a (F, F, k, k) weight that is zero outside [a, IN) x [a, IN), so that the
    weight gradient of the whole embedding (what rm_wgrad returns) comes out of the same autograd pass.
    Returns y, z (the pre-activation, zero outside the window) and 'bits' (pack_mask(z > 0)); for a cotangent gy also dx, gw
    (split, split, k, k), gb (split) and gw_dense (F, F, k, k), gb_dense (F), all from autograd.  mask (bool, as z): the ReLU
    gate the backward uses in place of z > 0 (y is relu's all the same)."""
    f = x.shape[1]
    xl = x.detach().clone().requires_grad_(gy is not None)
    wd = torch.zeros(f, f, k, k, dtype=x.dtype)
    wd[a:IN, a:IN] = w
    bd = torch.zeros(f, dtype=x.dtype)
    bd[a:IN] = b
    wd.requires_grad_(gy is not None)
    bd.requires_grad_(gy is not None)
    z = F_.conv2d(xl, wd, bd, padding=k // 2)
    y = xl + torch.relu(z)
    out = dict(y=y.detach(), z=z.detach(), bits=pack_mask(z.detach() > 0))
    if gy is not None:
        if mask is not None:
            (xl + z * mask.to(z.dtype)).backward(gy)
        else:
            y.backward(gy)
        out.update(dx=xl.grad, gw=wd.grad[a:IN, a:IN].clone(), gb=bd.grad[a:IN].clone(), gw_dense=wd.grad, gb_dense=bd.grad)
    return out


def unshuffle_ref(dout, R, cp=None):
    """(n, 3, R h, R w) -> (n, cp, h, w): channel c R^2 + i R + j of pixel (y, x) = dout[c, R y + i, R x + j]; zero past 3 R^2"""
    d = F_.pixel_unshuffle(dout, R)
    cp = d.shape[1] if cp is None else cp
    return torch.cat([d, d.new_zeros(d.shape[0], cp - d.shape[1], d.shape[2], d.shape[3])], 1)


def rm_tail_ref(feat, w, base, R, k, dout=None):
    """out = base + pixel_shuffle(conv_k(feat, w)); for a cotangent dout also dfeat, gw (3 R^2, F, k, k) and gb (3 R^2) -- the
    gradients of the conv against the un-shuffled cotangent -- and dconv = unshuffle_ref(dout, R, rm_cp(R))"""
    fl = feat.detach().clone().requires_grad_(dout is not None)
    wl = w.detach().clone().requires_grad_(dout is not None)
    bz = torch.zeros(w.shape[0], dtype=w.dtype, requires_grad=dout is not None)
    o = base + F_.pixel_shuffle(F_.conv2d(fl, wl, bz, padding=k // 2), R)
    out = dict(out=o.detach())
    if dout is not None:
        o.backward(dout)
        out.update(dfeat=fl.grad, gw=wl.grad, gb=bz.grad, dconv=unshuffle_ref(dout, R, RM_CP[R]))
    return out


# ---- runners: a case in a precision ------------------------------------------------------------------------------------------
def run_case(case, dtype=torch.float64, rnd=None, mask=None):
    """the tensors a kernel route returns for `case`, computed in `dtype` with `rnd` applied where the kernels store or read the
    hot dtype (None: nowhere).  conv7: y.  chain: y, inter.  block: y, z, bits, dx, gw, gb, gw_dense, gb_dense.  tail: out,
    dconv, dfeat, gw, gb."""
    r = rnd if rnd is not None else (lambda t: t)
    c = lambda name: case[name].to(dtype)
    kind = case["kind"]
    if kind == "conv7":
        relu, last = LAYERS[case["layer"]][2], case["layer"] == 4
        y = conv7_ref(r(c("x")), r(c("w")), c("b"), relu)
        return dict(y=y if last else r(y))
    if kind == "chain":
        inter = []
        y = basic_module_ref(c("x"), [p.to(dtype) for p in case["params"]], rnd, inter)
        return dict(y=y, inter=inter)
    if kind == "block":
        out = rm_block_ref(r(c("x")), r(c("w")), c("b"), case["a"], case["IN"], case["k"], r(c("gy")), mask)
        out["y"], out["dx"] = r(out["y"]), r(out["dx"])
        return out
    if kind == "tail":
        # (the cotangent reaches the convs through the un-shuffled image, which is stored in the hot dtype)
        out = rm_tail_ref(r(c("feat")), r(c("w")), c("base"), case["R"], case["k"], r(c("dout")))
        out["dfeat"] = r(out["dfeat"])
        return out
    raise ValueError(kind)


def emulate(case, mode, mask=None):
    """the case in the kernels' precision on the CPU: float32 throughout, in 'bf16' mode on operands and stores rounded to bf16"""
    return run_case(case, torch.float32, bf16_round if mode == "bf16" else None, mask)


# ---- exactness conditions ----------------------------------------------------------------------------------------------------
def _tie_near(v):
    """a bf16 tie in the binade of v > 0"""
    mant, exp = math.frexp(v)
    return math.ldexp((int(mant * 512.0) | 1) / 512.0, exp)


def _check_operands(name, w, b, *hot):
    for t in (w,) + hot:
        if not is_bf16(t):
            fail(f"{name}: an operand is not its own bf16 rounding")
    if not is_fp32(b):
        fail(f"{name}: a bias is not representable in fp32")
    if b.numel() > 1:
        need_biases(name, b)


def _conv_sums(name, xin, w, b, k, extra=None):
    """forward accumulator of conv_k(xin, w) + b (+ extra, a tensor added in the same fp32 register)"""
    cv = lambda t: t.view(1, -1, 1, 1)
    qx, qw = chan_quantum(xin), lowbit(w).amin((2, 3))
    q = (qw * qx.view(1, -1)).amin(1)
    s = F_.conv2d(xin.abs(), w.abs(), None, padding=k // 2)
    if b is not None:
        q, s = torch.minimum(q, lowbit(b)), s + cv(b.abs())
    if extra is not None:
        q, s = torch.minimum(q, chan_quantum(extra)), s + extra.abs()
    return need_sum(name, s, cv(q))


def _wgrad_sums(name, g, xin, w_shape, k):
    qg, qx = chan_quantum(g), chan_quantum(xin)
    tw = torch.nn.grad.conv2d_weight(xin.abs(), w_shape, g.abs(), padding=k // 2)
    need_sum(name + " weight gradient", tw, qg.view(-1, 1, 1, 1) * qx.view(1, -1, 1, 1))
    need_sum(name + " bias gradient", g.abs().sum((0, 2, 3)), qg)


def check_exact(case):
    """Verify the exactness conditions of an exact case on the float64 reference alone; raises ValueError if one fails.  Returns
    run_case()'s float64 result with every tensor that the kernels store in bf16 as well under '<name>_bf16' (rounded once),
    'ties' (how many of those elements sit exactly on a bf16 tie) and 'quanta' (the largest sum |terms| met, in quanta)."""
    kind = case["kind"]
    d = lambda name: case[name].double()
    out = run_case(case)
    worst = 0.0
    if kind == "conv7":
        x, w, b = d("x"), d("w"), d("b")
        cin, cout, relu = LAYERS[case["layer"]]
        if tuple(w.shape) != (cout, cin, 7, 7) or x.shape[1] != cin:
            fail("conv7: shapes")
        _check_operands("conv7", w, b, x)
        nz = w != 0
        if "taps" in case:
            if not bool((nz.flatten(1).sum(1) == 1).all()):
                fail("conv7 tap identity: exactly one weight per output channel")
            for co, (ci, ky, kx) in enumerate(case["taps"]):
                if not bool(nz[co, ci, ky, kx]):
                    fail("conv7 tap identity: the weight is not at the tap the case names")
        elif not bool(nz.all()):
            fail("conv7: a weight is zero")
        worst = _conv_sums("conv7 forward", x, w, b, 7)
        if not is_fp32(out["y"]):
            fail("conv7: y is not representable in fp32")
        if case["layer"] < 4:
            out["y_bf16"] = bf16_round(out["y"])
            out["ties"] = int(bf16_ties(out["y"]).sum())
            if out["ties"] == 0 and "taps" not in case:
                fail("conv7: no element on a bf16 tie")
    elif kind == "chain":
        params = [p.double() for p in case["params"]]
        xin = d("x")
        if not is_bf16(xin):
            fail("chain: x is not its own bf16 rounding")
        for i in range(5):
            w, b = params[2 * i], params[2 * i + 1]
            _check_operands(f"chain layer {i}", w, b)
            if not bool((w != 0).any(0).any(0).all()) or not bool((w != 0).any(0).any(1).any(1).all()):
                fail(f"chain layer {i}: a tap or an input channel carries no weight")
            worst = max(worst, _conv_sums(f"chain layer {i} forward", xin, w, b, 7))
            if i < 4:
                xin = out["inter"][i]
                if not is_bf16(xin):
                    fail(f"chain: the output of layer {i} is not its own bf16 rounding")
                frac = float((xin != 0).double().mean())
                if not 0.02 < frac < 1.0:
                    fail(f"chain: the output of layer {i} is idle ({frac} nonzero)")
        if not is_fp32(out["y"]) or not bool((out["y"] != 0).any()):
            fail("chain: y is not representable in fp32, or zero")
    elif kind == "block":
        x, w, b, gy = d("x"), d("w"), d("b"), d("gy")
        a, IN, k = case["a"], case["IN"], case["k"]
        _check_operands("block", w, b, x, gy)
        if not bool((w != 0).all()):
            fail("block: a weight is zero")
        if bool((x[:, IN:] != 0).any()) or bool((gy[:, IN:] != 0).any()):
            fail("block: padded channels must be zero")
        xs, z = x[:, a:IN], out["z"][:, a:IN]
        worst = _conv_sums("block forward", xs, w, b, k, extra=xs)
        if not (bool((z == 0).any()) and bool((z < 0).any()) and bool((z > 0).any())):
            fail("block: z must be exactly zero somewhere in the window, negative and positive elsewhere")
        if bool((out["z"][:, :a] != 0).any()) or bool((out["z"][:, IN:] != 0).any()):
            fail("block: z outside the window")
        gm = gy[:, a:IN] * (z > 0)
        _conv_sums("block backward data", gm, w.transpose(0, 1).flip(2, 3), None, k, extra=gy[:, a:IN])
        _wgrad_sums("block", gy * (out["z"] > 0), x, (x.shape[1], x.shape[1], k, k), k)
        for name in ("y", "dx", "gw", "gb", "gw_dense", "gb_dense"):
            if not is_fp32(out[name]):
                fail(f"block: {name} is not representable in fp32")
        if not (bool((out["gw"] != 0).any()) and bool((out["gb"] != 0).any())):
            fail("block: a gradient is idle")
        out["y_bf16"], out["dx_bf16"] = bf16_round(out["y"]), bf16_round(out["dx"])
        out["ties"] = int(bf16_ties(out["y"]).sum())
        if out["ties"] == 0:
            fail("block: no element of y on a bf16 tie")
    elif kind == "tail":
        feat, w, base, dout = d("feat"), d("w"), d("base"), d("dout")
        R, k = case["R"], case["k"]
        co = 3 * R * R
        _check_operands("tail", w, w.new_zeros(1), feat, dout)
        if not bool((w != 0).all()) or not bool((base != 0).all()):
            fail("tail: a weight or an element of the base is zero")
        worst = _conv_sums("tail forward", feat, w, None, k, extra=F_.pixel_unshuffle(base, R))
        dc = out["dconv"][:, :co]
        _conv_sums("tail backward data", dc, w.transpose(0, 1).flip(2, 3), None, k)
        _wgrad_sums("tail", dc, feat, tuple(w.shape), k)
        for name in ("out", "dfeat", "gw", "gb", "dconv"):
            if not is_fp32(out[name]):
                fail(f"tail: {name} is not representable in fp32")
        if bool((out["dconv"][:, co:] != 0).any()):
            fail("tail: padded channels of the un-shuffled cotangent")
        out["dfeat_bf16"] = bf16_round(out["dfeat"])
        out["ties"] = int(bf16_ties(out["dfeat"]).sum())
    else:
        raise ValueError(kind)
    out["quanta"] = worst
    return out


# ---- exact cases -------------------------------------------------------------------------------------------------------------
SEED = (24680, 11)                                          # (start, step) of parity_kit.seed
_seed = functools.partial(seed, *SEED)


def _pow2(lo, hi, shape, g):
    """2^e, e uniform in lo..hi"""
    return 2.0 ** torch.randint(lo, hi + 1, shape, generator=g).double()


def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _ternary(shape, g, density=1.0):
    t = torch.randint(-1, 2, shape, generator=g).double()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density).double()
    return t


def _odd_biases(c, g, scale=0.125):
    """c pairwise different nonzero dyadics: c consecutive odd numbers around 0 in a random order, times `scale`"""
    return (2.0 * torch.randperm(c, generator=g).double() + 1.0 - 2 * (c // 2)) * scale


def _bump_bias(b, c, delta):
    """b[c] += delta if the result stays nonzero and different from every other entry; says whether it did"""
    v = float(b[c]) + delta
    if v == 0.0 or any(float(b[j]) == v for j in range(b.numel()) if j != c):
        return False
    b[c] = v
    return True


@functools.lru_cache(maxsize=None)
def conv7_exact_case(layer, n, h, w, seed=0):
    """one layer of BasicModule on dense dyadic data; a bias is moved so that one output sits on a bf16 tie if the draw gave none"""
    cin, cout, relu = LAYERS[layer]
    g = torch.Generator().manual_seed(_seed(1, layer, n, h, w, seed))
    x = _ternary((n, cin, h, w), g) * _pow2(-2, 2, (cin,), g).view(1, -1, 1, 1)
    wt = _signs((cout, cin, 7, 7), g) * _pow2(-2, 1, (cout, cin, 7, 7), g)
    b = _odd_biases(cout, g)
    if layer < 4:
        y = conv7_ref(x, wt, b, relu)
        if not bool(bf16_ties(y).any()):
            flat = int(y.argmax())
            c = (flat // (h * w)) % cout
            v = float(y.flatten()[flat])
            if not (v > 0 and _bump_bias(b, c, _tie_near(v) - v)):
                fail("conv7: no output could be put on a tie")
    case = dict(kind="conv7", layer=layer, x=x.float(), w=wt.float(), b=b.float())
    case["ref"] = check_exact(case)
    return case


def conv7_tap_count(layer):
    cin, cout, _ = LAYERS[layer]
    return -(-max(49, cin) // cout) + (1 if cin == 8 else 0)


@functools.lru_cache(maxsize=None)
def conv7_tap_cases(layer, n, h, w, seed=0):
    """the tap-identity set of a layer: conv7_tap_count() cases, slot i = case * cout + co holds its one weight (+-2^k) at tap
    i mod 49 and input channel i mod cin, so the set covers all 49 taps and every input channel; for cin = 8 the set has one
    case more, which puts all eight channels on a tap with kx = 6 (whose k-step partner is the zero tap kx = 7)"""
    cin, cout, relu = LAYERS[layer]
    g = torch.Generator().manual_seed(_seed(2, layer, n, h, w, seed))
    x = torch.randint(-7, 8, (n, cin, h, w), generator=g).double() * _pow2(-2, 2, (cin,), g).view(1, -1, 1, 1)
    cases = []
    for j in range(conv7_tap_count(layer)):
        wt = torch.zeros(cout, cin, 7, 7, dtype=torch.float64)
        val = _signs((cout,), g) * _pow2(-2, 1, (cout,), g)
        taps = []
        for co in range(cout):
            i = j * cout + co
            tap, ci = i % 49, i % cin
            wt[co, ci, tap // 7, tap % 7] = val[co]
            taps.append((ci, tap // 7, tap % 7))
        case = dict(kind="conv7", layer=layer, x=x.float(), w=wt.float(), b=_odd_biases(cout, g).float(), taps=tuple(taps))
        case["ref"] = check_exact(case)
        cases.append(case)
    return tuple(cases)


CHAIN_NZ = (2, 2, 2, 4, 25)                                # weights per output channel: cout nz >= max(49, cin) in every layer


def _sparse7(cout, cin, nz, layer, g):
    """(cout, cin, 7, 7) with nz weights +-1 per output channel: entry i = co nz + j at tap 5 i + layer (mod 49) and input channel
    3 i + layer (mod cin); the rows together use every tap and every input channel"""
    assert cout * nz >= max(49, cin)
    w = torch.zeros(cout, cin, 7, 7, dtype=torch.float64)
    sg = _signs((cout * nz,), g)
    for i in range(cout * nz):
        tap, ci = (5 * i + layer) % 49, (3 * i + layer) % cin
        w[i // nz, ci, tap // 7, tap % 7] = sg[i]
    return w


@functools.lru_cache(maxsize=None)
def chain_exact_case(n, h, w, seed=0):
    """BasicModule as an integer network: inputs in {-1, 0, 1}; the bias of each ReLU layer is -(max of the channel's
    pre-activation - m), m from 3 up, so every activation is an integer in 0..m; then every channel of every tensor gets its own
    power-of-two scale, which turns the weights into +-2^k and makes the biases pairwise different"""
    g = torch.Generator().manual_seed(_seed(3, n, h, w, seed))
    a = _ternary((n, 8, h, w), g)
    s_in = _pow2(-2, 2, (8,), g)
    x = a * s_in.view(1, -1, 1, 1)
    params = []
    for layer, (cin, cout, relu) in enumerate(LAYERS):
        wl = _sparse7(cout, cin, CHAIN_NZ[layer], layer, g)
        pre = F_.conv2d(a, wl, None, padding=3)
        s_out = _pow2(-2, 2, (cout,), g)
        if relu:
            top = pre.amax((0, 2, 3))
            b, used = torch.zeros(cout, dtype=torch.float64), set()
            for c in range(cout):
                m = 3 + int(torch.randint(0, 4, (1,), generator=g))
                while float(top[c]) == m or float((m - top[c]) * s_out[c]) in used:
                    m += 1
                b[c] = m - top[c]
                used.add(float(b[c] * s_out[c]))
            a = torch.relu(pre + b.view(1, -1, 1, 1))
        else:
            b = torch.tensor([3.0, -5.0], dtype=torch.float64)
            a = pre + b.view(1, -1, 1, 1)
        params += [(wl * s_out.view(-1, 1, 1, 1) / s_in.view(1, -1, 1, 1)).float(), (b * s_out).float()]
        s_in = s_out
    case = dict(kind="chain", x=x.float(), params=params)
    case["ref"] = check_exact(case)
    if not torch.equal(case["ref"]["y"], a * s_in.view(1, -1, 1, 1)):
        fail("chain: the scaled network does not compute the scaled integers")
    return case


@functools.lru_cache(maxsize=None)
def block_exact_case(F, IN, split, k, n, h, w, seed=0, density=0.5):
    """Block [IN, split, k] in F channels on dense dyadic data with a cotangent.  Two biases are fitted to the data: one so that
    an element of y (z > 0 there) sits on a bf16 tie, one -- of another channel -- so that the z of smallest magnitude is 0."""
    a = IN - split
    g = torch.Generator().manual_seed(_seed(4, F, IN, split, k, n, h, w, seed))
    x = torch.zeros(n, F, h, w, dtype=torch.float64)
    x[:, :IN] = _ternary((n, IN, h, w), g) * _pow2(-2, 2, (IN,), g).view(1, -1, 1, 1)
    wt = _signs((split, split, k, k), g) * _pow2(-2, 1, (split, split, k, k), g)
    b = _odd_biases(split, g)
    gy = torch.zeros(n, F, h, w, dtype=torch.float64)
    gy[:, :IN] = _ternary((n, IN, h, w), g, density) * _pow2(-2, 2, (IN,), g).view(1, -1, 1, 1)
    z = F_.conv2d(x[:, a:IN], wt, b, padding=k // 2)
    c_tie = -1
    if split > 1:
        flat = int(z.argmax())
        c_tie = (flat // (h * w)) % split
        zv = float(z.flatten()[flat])
        yv = float((x[:, a:IN] + z).flatten()[flat])
        if zv > 0 and yv > 0 and zv + _tie_near(yv) - yv > 0:
            _bump_bias(b, c_tie, _tie_near(yv) - yv)
        z = F_.conv2d(x[:, a:IN], wt, b, padding=k // 2)
    za = z.abs().clone()
    if c_tie >= 0:
        za[:, c_tie] = BIG
    for flat in za.flatten().argsort()[:64].tolist():          # the smallest |z| whose channel's bias can take the change
        if _bump_bias(b, (flat // (h * w)) % split, -float(z.flatten()[flat])):
            break
    case = dict(kind="block", F=F, IN=IN, a=a, k=k, x=x.float(), w=wt.float(), b=b.float(), gy=gy.float())
    case["ref"] = check_exact(case)
    return case


@functools.lru_cache(maxsize=None)
def tail_exact_case(F, R, k, n, h, w, seed=0, density=0.5):
    """the k x k tail on dense dyadic data: conv F -> 3 R^2, pixel shuffle, added onto a non-zero dyadic base; a cotangent"""
    co = 3 * R * R
    g = torch.Generator().manual_seed(_seed(5, F, R, k, n, h, w, seed))
    feat = _ternary((n, F, h, w), g) * _pow2(-2, 2, (F,), g).view(1, -1, 1, 1)
    wt = _signs((co, F, k, k), g) * _pow2(-2, 1, (co, F, k, k), g)
    base = _signs((n, 3, R * h, R * w), g) * torch.randint(1, 8, (n, 3, R * h, R * w), generator=g).double() * 0.25
    dout = _ternary((n, 3, R * h, R * w), g, density) * _pow2(-2, 2, (3,), g).view(1, -1, 1, 1)
    case = dict(kind="tail", F=F, R=R, k=k, feat=feat.float(), w=wt.float(), base=base.float(), dout=dout.float())
    case["ref"] = check_exact(case)
    return case


# the cases of the parity tests: (n, h, w).  conv7: tile 8 x 32, halo 3, one row per wave.  Result_Model conv: tile 32 wide and 16
# (bf16) or 8 (fp32) rows, halo k / 2; weight-gradient tile 16 x 16.
CONV7_GEOMETRIES = ((1, 1, 1), (1, 3, 3), (1, 7, 31), (1, 8, 32), (2, 9, 33), (1, 16, 64), (2, 17, 65), (1, 5, 70), (3, 24, 8))
CONV7_TAP_GEOMETRY = (2, 9, 33)
CHAIN_GEOMETRIES = ((1, 9, 33), (2, 16, 64))
CONV7_ROUNDED_GEOMETRIES = ((2, 17, 65), (1, 8, 32))
CHAIN_ROUNDED_GEOMETRY = (1, 32, 32)
SPYNET_ROUNDED = ((1, 32, 32), (1, 40, 56), (1, 64, 64))             # 32 x 32: the network itself refuses it
RM_KS = (3, 5, 7)
RM_TAIL_KS = (5, 7)
RM_GEOMETRIES = ((1, 1, 1), (1, 2, 5), (1, 7, 31), (1, 8, 32), (2, 9, 33), (1, 15, 16), (1, 16, 17), (2, 17, 15), (1, 33, 65))
RM_SWEEP_WINDOWS = ((24, 20, 12), (32, 27, 27))                              # (F, IN, split)
RM_WINDOWS = ((24, 24, 24), (24, 8, 8), (24, 20, 12), (32, 32, 5), (32, 27, 27))
RM_WINDOW_GEOMETRIES = ((2, 9, 33), (1, 16, 17))
RM_TAIL_GEOMETRIES = ((1, 1, 1), (2, 9, 33), (1, 17, 31))
RM_TAIL_RS = (2, 3, 4)
RM_TAIL_FS = (24, 32)
RM_LOOP_GEOMETRY = (2, 16, 33)                                               # 6 tiles of 16 x 16
RM_LOOP_WGS = (1, 2, 5, 6, 7, 256)
RM_LOOP_KS = (3, 7)
RM_LOOP_WINDOW = (32, 27, 27)
RM_MANY_TILES = ((2, 48, 80), 4)                                             # 30 tiles over 4 workgroups
RM_ROUNDED_GEOMETRY = (2, 19, 37)


def wgrad_tiles(n, h, w):
    return n * ((h + 15) // 16) * ((w + 15) // 16)


# ---- rounded cases -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv7_rounded_case(layer, n, h, w, seed=0):
    cin, cout, _ = LAYERS[layer]
    g = torch.Generator().manual_seed(_seed(6, layer, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(kind="conv7", layer=layer, w=rn(cout, cin, 7, 7) * (2.0 / (49 * cin)) ** 0.5, b=0.1 * rn(cout), x=rn(n, cin, h, w))


@functools.lru_cache(maxsize=None)
def chain_rounded_case(n, h, w, seed=0):
    g = torch.Generator().manual_seed(_seed(7, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    params = []
    for cin, cout, _ in LAYERS:
        params += [rn(cout, cin, 7, 7) * (2.0 / (49 * cin)) ** 0.5, 0.1 * rn(cout)]
    return dict(kind="chain", params=params, x=rn(n, 8, h, w))


@functools.lru_cache(maxsize=None)
def block_rounded_case(F, IN, split, k, n, h, w, seed=0):
    g = torch.Generator().manual_seed(_seed(8, F, IN, split, k, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    x, gy = torch.zeros(n, F, h, w), torch.zeros(n, F, h, w)
    x[:, :IN], gy[:, :IN] = rn(n, IN, h, w), rn(n, IN, h, w)
    return dict(kind="block", F=F, IN=IN, a=IN - split, k=k, x=x, gy=gy, w=rn(split, split, k, k) / (k * split ** 0.5), b=0.1 * rn(split))


@functools.lru_cache(maxsize=None)
def tail_rounded_case(F, R, k, n, h, w, seed=0):
    g = torch.Generator().manual_seed(_seed(9, F, R, k, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(kind="tail", F=F, R=R, k=k, feat=rn(n, F, h, w), w=rn(3 * R * R, F, k, k) / (k * F ** 0.5), base=rn(n, 3, R * h, R * w),
                dout=rn(n, 3, R * h, R * w))


@functools.lru_cache(maxsize=None)
def rounded_reference(kind, mode, *key):
    """(case, float64 reference, yardstick per tensor name): the yardstick is the distance of emulate() from the float64
    reference in the tests' metric -- computed from the reference alone.  The backward of a block case uses the float64
    reference's ReLU gate in the emulation too (the kernels are handed it)."""
    case = {"conv7": conv7_rounded_case, "chain": chain_rounded_case, "block": block_rounded_case, "tail": tail_rounded_case}[kind](*key)
    ref = run_case(case)
    emu = emulate(case, mode, (ref["z"] > 0) if kind == "block" else None)
    names = {"conv7": ("y",), "chain": ("y",), "block": ("y", "dx", "gw", "gb"), "tail": ("out", "dfeat", "gw", "gb")}[kind]
    return case, ref, {nm: rel_max(emu[nm], ref[nm]) for nm in names}
