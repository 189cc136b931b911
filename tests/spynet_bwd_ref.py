"""The backward of SPyNet's 7x7 convolutions (csrc/spynet_conv.h, BWD epilogue and conv7_wgrad_kernel) written out in plain torch,
float64 on the CPU, with the kernels' rounding points applied where the kernels apply them, plus the case generators and the
per-element bounds of tests/test_gpu_spynet_train.py.  Nothing of the package is used; tests/conv_ref.py and tests/parity_kit.py
are used as they are.  tests/test_spynet_bwd_host.py pins these functions to torch autograd in float64.

Rounding points (restated from the kernel header):
  * the incoming flow gradient is fp32 and is rounded ONCE to bf16 as an MFMA operand (round_in);
  * the weights are rounded to bf16 as the backward-data operand;
  * every dx_l (l >= 1) is rounded once to bf16 AFTER the mask; that value is both the next backward-data operand and the
    weight-gradient operand of layer l - 1;
  * x_l are the bf16 activations the forward wrote, and the ReLU mask is x_l > 0 of those SAVED activations -- the functions below
    take them as arguments and never re-derive a mask from a differently rounded forward;
  * every accumulation is fp32; db is summed in fp32 from the bf16 dy; dx_0 is stored in fp32, unmasked.

Bounds.  The kernels' results differ from the float64 value of the same operands only by fp32 accumulation and the store.  Every
partial sum of a reduction is at most S = sum |terms| in magnitude, so each of its K additions rounds by at most 2^-24 S (bf16 x
bf16 products are exact in fp32): |error| <= K 2^-24 S, in any order -- which also covers the order in which the workgroup slabs are
summed, so a weight gradient is independent of the workgroup cap only up to this bound, not bit for bit.  A bf16 store adds half an
ulp of the stored value: bf16 carries 8 significant bits, so that is 2^(e - 8) for a magnitude in [2^e, 2^(e + 1)) (half_ulp16).  K counts the terms of an accumulator: 49 x (contraction channels) for
backward-data; n h w pixels, plus one addition per slab and the 16 partial sums of the reduction launch, for the weight gradient."""
import functools

import torch
import torch.nn.functional as F_

from tests import conv_ref as R
from tests.parity_kit import bf16_round, seed

LAYERS = R.LAYERS
U32 = 2.0 ** -24                                           # unit roundoff of an fp32 addition
REDUCE_Q = 16                                              # partial sums per element in the slab reduction launch

_seed = functools.partial(seed, 20250131, 29)


def half_ulp16(mag):
    """half an ulp of bf16 at the magnitude `mag` (>= 0): 2^(e - 8) with 2^e <= mag < 2^(e + 1); 0 at 0"""
    _, exp = torch.frexp(mag.double())                     # mag = m 2^exp, m in [0.5, 1): e = exp - 1
    return torch.where(mag > 0, torch.ldexp(torch.ones_like(mag, dtype=torch.float64), exp - 9), torch.zeros_like(mag, dtype=torch.float64))


# ---- one layer -----------------------------------------------------------------------------------------------------------------
def bwd_data_ref(dy, w, act=None):
    """dx (n, cin, h, w) of y = conv7(x, w): the 7x7 / pad 3 convolution of dy with the weights rotated by 180 degrees and the
    channel roles swapped; times act > 0 (the saved input of the layer) when given"""
    dx = F_.conv2d(dy, w.flip(2, 3).transpose(0, 1), None, padding=3)
    return dx if act is None else dx * (act > 0).to(dx.dtype)


def wgrad_ref(dy, x):
    """(dW (cout, cin, 7, 7), db (cout)): dW[co][ci][ky][kx] = sum_{n, y, x} dy[n, co, y, x] x[n, ci, y + ky - 3, x + kx - 3]"""
    n, cin, h, w = x.shape
    xp = F_.pad(x, (3, 3, 3, 3))
    dw = torch.zeros(dy.shape[1], cin, 7, 7, dtype=dy.dtype)
    for ky in range(7):
        for kx in range(7):
            dw[:, :, ky, kx] = torch.einsum("nchw,ndhw->cd", dy, xp[:, :, ky:ky + h, kx:kx + w])
    return dw, dy.sum((0, 2, 3))


def wgrad_terms(n, h, w, wgs):
    return n * h * w + wgs + REDUCE_Q


def layer_ref(layer, dy, w, x, wgs):
    """One layer's backward on operands AS THE KERNELS HOLD THEM: dy (n, cout, h, w) and x (n, cin, h, w) bf16 values in float64,
    w the fp32 weight (rounded to bf16 here for backward-data).  Returns the float64 values and their per-element bounds:
    dx (masked by x > 0 for layer >= 1, not yet rounded), dw, db, tol_dx, tol_dw, tol_db."""
    cin, cout, _ = LAYERS[layer]
    dy, x, wr = dy.double(), x.double(), bf16_round(w.double())
    dx = bwd_data_ref(dy, wr, x if layer else None)
    e_dx = 49 * max(cout, 8) * U32 * bwd_data_ref(dy.abs(), wr.abs())
    tol_dx = e_dx if layer == 0 else e_dx + half_ulp16(dx.abs() + e_dx)
    dw, db = wgrad_ref(dy, x)
    sw, sb = wgrad_ref(dy.abs(), x.abs())
    k = wgrad_terms(dy.shape[0], dy.shape[2], dy.shape[3], wgs)
    return dict(dx=dx, dw=dw, db=db, tol_dx=tol_dx, tol_dw=k * U32 * sw, tol_db=k * U32 * sb)


def round_in(dflow):
    """the flow gradient as the kernels take it: rounded once to bf16"""
    return bf16_round(dflow.double())


def chain_bwd_ref(dflow, params, xs, rnd=bf16_round):
    """The backward of a BasicModule call in float64: dflow (n, 2, h, w); params [w0, b0, .., w4, b4]; xs: the five SAVED layer
    inputs (n, c_l, h, w) whose sign is the ReLU mask.  rnd is applied at the rounding points (None: nowhere -- then this is
    plain autograd of the chain with the given masks).  Returns (dinput (n, 8, h, w), [dw0, db0, .., dw4, db4])."""
    r = rnd if rnd is not None else (lambda t: t)
    g = r(dflow.double())
    grads = [None] * 10
    for l in range(4, -1, -1):
        x = xs[l].double()
        grads[2 * l], grads[2 * l + 1] = wgrad_ref(g, x)
        g = bwd_data_ref(g, r(params[2 * l].double()), x if l else None)
        if l:
            g = r(g)
    return g, grads


# ---- cases ---------------------------------------------------------------------------------------------------------------------
# (n, h, w): one full 8 x 32 tile; one past both tile edges, batch 2; interior tiles plus ragged edges; the coarsest pyramid levels,
# where the image is smaller than the halo
GEOMETRIES = ((1, 8, 32), (2, 9, 33), (1, 17, 65), (1, 2, 2), (1, 1, 1))
# weight gradient, (n, h, w, workgroup cap): the same at the default cap; 18 tiles of 16 x 16 over 5 workgroups (the tile loop runs
# four times, in the last workgroup twice); the same tiles on a single workgroup
WGRAD_CASES = tuple(g + (32,) for g in GEOMETRIES) + ((2, 33, 40, 5), (2, 33, 40, 1))
CHAIN_GEOMETRY = (2, 16, 32)
TAP_GEOMETRY = (2, 9, 33)


def _act(shape, g):
    """a saved bf16 activation: small integers times a per-channel power of two, about half of them zero (ReLU's output)"""
    a = torch.randint(0, 8, shape, generator=g).double() * (torch.rand(shape, generator=g) < 0.5).double()
    return a * R._pow2(-2, 2, (shape[1],), g).view(1, -1, 1, 1)


def tap_count(layer):
    cin, cout, _ = LAYERS[layer]
    return -(-max(49, cout) // cin) + (1 if layer == 4 else 0)


@functools.lru_cache(maxsize=None)
def tap_cases(layer, n, h, w):
    """Tap-identity cases of backward-data: every INPUT channel ci of the forward layer (an output channel of the transposed one)
    holds one weight +-2^k, slot i = case * cin + ci at tap i mod 49 and output channel i mod cout, so a set covers all 49 taps
    (every rotation) and every channel of dy (every swap); dx[ci] is then a shifted copy of one dy channel times that weight,
    times the mask.  Layer 4 (dy padded to 8 channels, two taps per k-step) has one case more with every channel on the tap
    kx = 0, which the rotation sends to kx = 6, the partner of the zero tap.  All operands are their own bf16 rounding and every
    result is a single product, so a kernel must return 'dx' bit for bit."""
    cin, cout, _ = LAYERS[layer]
    g = torch.Generator().manual_seed(_seed(1, layer, n, h, w))
    dy = torch.randint(-7, 8, (n, cout, h, w), generator=g).double() * R._pow2(-2, 2, (cout,), g).view(1, -1, 1, 1)
    act = _act((n, cin, h, w), g)
    cases = []
    for j in range(tap_count(layer)):
        wt = torch.zeros(cout, cin, 7, 7, dtype=torch.float64)
        val = R._signs((cin,), g) * R._pow2(-2, 1, (cin,), g)
        taps = []
        for ci in range(cin):
            i = j * cin + ci
            tap, co = i % 49, i % cout
            if layer == 4 and j == tap_count(layer) - 1:
                tap = 3 * 7 + 0
            wt[co, ci, tap // 7, tap % 7] = val[ci]
            taps.append((co, tap // 7, tap % 7))
        dx = bwd_data_ref(dy, wt, act if layer else None)
        assert torch.equal(dx, bf16_round(dx))
        cases.append(dict(layer=layer, dy=dy.float(), w=wt.float(), act=act.float(), dx=dx, taps=tuple(taps)))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def rounded_case(layer, n, h, w):
    """random operands as the kernels hold them: dy and x in bf16 (x a ReLU output for layer >= 1), w fp32"""
    cin, cout, _ = LAYERS[layer]
    g = torch.Generator().manual_seed(_seed(2, layer, n, h, w))
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(n, cin, h, w)
    return dict(layer=layer, dy=bf16_round(rn(n, cout, h, w)), x=bf16_round(x.clamp_min(0) if layer else x),
                w=rn(cout, cin, 7, 7) * (2.0 / (49 * cin)) ** 0.5)


@functools.lru_cache(maxsize=None)
def chain_case(n, h, w):
    g = torch.Generator().manual_seed(_seed(3, n, h, w))
    rn = lambda *s: torch.randn(*s, generator=g)
    params = []
    for cin, cout, _ in LAYERS:
        params += [rn(cout, cin, 7, 7) * (2.0 / (49 * cin)) ** 0.5, 0.1 * rn(cout)]
    return dict(params=params, x=rn(n, 8, h, w), dflow=rn(n, 2, h, w))


# ---- the whole network -----------------------------------------------------------------------------------------------------------
SPYNET_GEOMETRY = (2, 64, 64)                              # the smallest input whose coarsest level is not empty
SPYNET_SEED = 3
MASK_CAP = 0.01                                            # at most 1 % of a tensor's elements may sit on a flipped mask


def spynet_case(seed_=SPYNET_SEED):
    """(state_dict, ref, supp, cotangent): a seeded SpyNet-shaped state_dict (He-scaled weights, small biases), two image
    batches in [0, 1] (supp = ref shifted by a pixel plus noise, so the flow is not trivial), a fixed random cotangent"""
    n, h, w = SPYNET_GEOMETRY
    g = torch.Generator().manual_seed(_seed(4, n, h, w, seed_))
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {}
    for lv in range(6):
        for i, (cin, cout, _) in zip((0, 2, 4, 6, 8), LAYERS):
            sd[f"basic_module.{lv}.basic_module.{i}.weight"] = rn(cout, cin, 7, 7) * (2.0 / (49 * cin)) ** 0.5
            sd[f"basic_module.{lv}.basic_module.{i}.bias"] = 0.1 * rn(cout)
    sd["mean"] = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    sd["std"] = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    base = F_.interpolate(torch.rand(n, 3, h // 4, w // 4, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    ref = (base + 0.05 * rn(n, 3, h, w)).clamp(0, 1)
    supp = (torch.roll(base, (1, 1), (2, 3)) + 0.05 * rn(n, 3, h, w)).clamp(0, 1)
    return sd, ref, supp, rn(n, 2, h, w)


class _RoundBoth(torch.autograd.Function):
    """value rounded on the way forward and gradient rounded on the way back: a tensor AND its gradient held in bf16"""

    @staticmethod
    def forward(ctx, x):
        return bf16_round(x)

    @staticmethod
    def backward(ctx, g):
        return bf16_round(g)


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return bf16_round(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16_round(g)


def _module_restated(x, params, rounded, masks):
    """BasicModule with autograd, in x's dtype.  rounded: the conv operands are rounded to bf16 at the stated points (input,
    weights and inter-layer activations forward; the flow gradient and every dx_l, l >= 1, backward).  masks: a list that
    receives the four ReLU masks."""
    if rounded:
        x = _RoundFwd.apply(x)
    for l in range(5):
        wt = _RoundFwd.apply(params[2 * l]) if rounded else params[2 * l]
        x = F_.conv2d(x, wt, params[2 * l + 1], padding=3)
        if l < 4:
            x = torch.relu(x)
            x = _RoundBoth.apply(x) if rounded else x
            masks.append((x > 0).detach())
        elif rounded:
            x = _RoundBwd.apply(x)
    return x


def spynet_restated(sd, ref, supp, cot, rounded, dtype=torch.float64):
    """SpyNet.forward restated with autograd (conv_ref.spynet_ref's arithmetic) in `dtype`; loss = cot . flow.  Returns (flow,
    {name: gradient} for the 60 parameter tensors and 'ref' / 'supp', the list of the 24 ReLU masks)."""
    import math
    p = {k: v.detach().to(dtype).requires_grad_(k not in ("mean", "std")) for k, v in sd.items()}
    ref, supp = ref.detach().to(dtype).requires_grad_(True), supp.detach().to(dtype).requires_grad_(True)
    h, w = ref.shape[2:]
    wf, hf = math.floor(math.ceil(w / 32.0) * 32.0), math.floor(math.ceil(h / 32.0) * 32.0)
    r0 = F_.interpolate(ref, size=(hf, wf), mode="bilinear", align_corners=False)
    s0 = F_.interpolate(supp, size=(hf, wf), mode="bilinear", align_corners=False)
    refs, supps = [(r0 - p["mean"]) / p["std"]], [(s0 - p["mean"]) / p["std"]]
    for _ in range(5):
        refs.insert(0, F_.avg_pool2d(refs[0], kernel_size=2, stride=2, count_include_pad=False))
        supps.insert(0, F_.avg_pool2d(supps[0], kernel_size=2, stride=2, count_include_pad=False))
    flow = refs[0].new_zeros(refs[0].shape[0], 2, refs[0].shape[2] // 2, refs[0].shape[3] // 2)
    masks = []
    for lv in range(6):
        up = F_.interpolate(flow, scale_factor=2, mode="bilinear", align_corners=True) * 2.0
        if up.shape[2] != refs[lv].shape[2]:
            up = F_.pad(up, [0, 0, 0, 1], mode="replicate")
        if up.shape[3] != refs[lv].shape[3]:
            up = F_.pad(up, [0, 1, 0, 0], mode="replicate")
        params = [p[f"basic_module.{lv}.basic_module.{i}.{q}"] for i in (0, 2, 4, 6, 8) for q in ("weight", "bias")]
        flow = _module_restated(torch.cat([refs[lv], R._border_warp(supps[lv], up), up], 1), params, rounded, masks) + up
    flow = F_.interpolate(flow, size=(h, w), mode="bilinear", align_corners=False)
    flow = flow * torch.tensor([float(w) / float(wf), float(h) / float(hf)], dtype=dtype).view(1, 2, 1, 1)
    (flow * cot.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in p.items() if v.requires_grad}
    grads["ref"], grads["supp"] = ref.grad, supp.grad
    return flow.detach(), grads, masks


def rel_l2(got, ref):
    ref = ref.double()
    d = (got.double() - ref).norm().item()
    s = ref.norm().item()
    return d / s if s > 0 else d


@functools.lru_cache(maxsize=None)
def spynet_noise(seed_=SPYNET_SEED):
    """The rounding noise the reference alone shows: per tensor, the relative L2 difference between the float64 restatement with
    its conv operands rounded to bf16 at the stated points and the same restatement unrounded; and the largest fraction of a
    ReLU mask's elements that the rounding flipped.  Returns (unrounded gradients, {name: noise}, flipped fraction)."""
    sd, ref, supp, cot = spynet_case(seed_)
    _, g64, m64 = spynet_restated(sd, ref, supp, cot, False)
    _, g16, m16 = spynet_restated(sd, ref, supp, cot, True)
    flipped = max(float((a != b).double().mean()) for a, b in zip(m64, m16))
    return g64, {k: rel_l2(g16[k], g64[k]) for k in g64}, flipped
