"""The BasicVSR propagation trunk (ConvResidualBlocks: conv3x3(cin -> F) + LeakyReLU(0.1), then nb x [a + conv2(relu(conv1(a)))])
and the recurrent step around it written out in plain torch, float64 on the CPU, plus the case generators of the trunk parity
tests.  Nothing of the package or of the oracle is used here: this is the outside reference that csrc/conv3x3.h and
csrc/conv64.h are held against (tests/test_gpu_trunk_ref.py).  tests/test_trunk_ref_host.py pins it to fixture G7 and to
oracle.wdsr_oracle and checks on the CPU that every exact case satisfies its exactness conditions.  The warp of the recurrent
step is tests/warp_ref.py's, which tests/test_warp_ref_host.py pins.

Parameters are a list in the reference's state_dict order: [w0, b0, (w1_i, b1_i, w2_i, b2_i) for every block].

Two families of cases:
  exact     dyadic data on which every tensor the kernels store in the hot dtype is its own bf16 rounding and every reduction
            satisfies sum |terms| < 2^24 quanta, so fp32 accumulation is exact in ANY order: a kernel must return the float64
            reference bit for bit, in fp32 and in bf16 (check_exact() verifies the conditions on the float64 reference alone and
            raises if one fails).  0.1 is not dyadic, so the first conv's pre-activation is kept strictly positive.
  rounded   random normal data; the yardstick is a CPU emulation of the kernels' precision (emulate()).

How an exact case is built.  An INTEGER network (weights +-1, two per output channel, placed so that the rows together use every tap
and every input channel; integer biases; inputs in {-1, 0, 1}) is drawn first.  The bias of each conv1 is chosen from the data:
-(max of the channel's pre-activation - m), m in 2..4, so that t = relu(.) takes the values 0..m only and the residual stream grows
by a few units per block -- that is what keeps every value within 8 significant bits through 1 + 2 nb layers.  Then every channel
of every tensor is given its own power-of-two scale (the activations of the residual stream share one set of scales, each t_i has
its own), which turns the weights into +-2^k with k all over the place and makes the biases of a conv pairwise different, while
every dot product still sums terms of ONE lattice: the scaled network computes the scaled integers exactly.

The conditions named need_* / is_*, the roundings, the seed recipe and the bound of the rounded cases are tests/parity_kit.py's,
shared by all parity suites and pinned by tests/test_parity_kit_host.py.
"""
import functools

import torch
import torch.nn.functional as F_

from tests.parity_kit import (RoundBackward, RoundForward, bf16_round, chan_quantum, fail, is_bf16, leaf, lowbit, need_bf16, need_biases,
                              need_fp32, need_sum, need_taps, rel_max, seed)
from tests.warp_ref import warp_ref

SLOPE = 0.1
TILE = 16


def n_tiles(n, h, w):
    return n * ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)


def param_names(nb):
    names = ["main.0.weight", "main.0.bias"]
    for i in range(nb):
        names += [f"main.2.{i}.conv1.weight", f"main.2.{i}.conv1.bias", f"main.2.{i}.conv2.weight", f"main.2.{i}.conv2.bias"]
    return names


def state_dict_of(params):
    nb = (len(params) - 2) // 4
    return {k: v.detach().float() for k, v in zip(param_names(nb), params)}


def trunk_ref(x, params, nb, inter=None, rnd=None):
    """x (n, cin, h, w), params as above, all of one dtype (float64 for the reference).  Returns a_nb (n, F, h, w).
    inter: a dict that receives every intermediate formed here -- 'x', 'z0', 'a0', and per block 'z1_i', 't_i', 'z2_i',
    'a{i+1}' -- each with its gradient retained.  rnd: None for the reference; else the rounding applied where the bf16 kernels
    round: forward the input, the packed weights and biases, a_0, t_i, a_{i+1}; backward dz of the first conv (ga_0 act'(a_0)),
    gt_i, ga_i (the sum of its two terms, once) and dx (the caller rounds the cotangent, which is ga_nb)."""
    assert len(params) == 2 + 4 * nb
    keep = {}
    rf = (lambda t: RoundForward.apply(t, rnd)) if rnd is not None else (lambda t: t)
    rb = (lambda t: RoundBackward.apply(t, rnd)) if rnd is not None else (lambda t: t)
    params = [rf(p) for p in params]
    x = rf(rb(x))
    keep["x"] = x
    z0 = rb(F_.conv2d(x, params[0], params[1], padding=1))
    a = rb(rf(F_.leaky_relu(z0, SLOPE)))
    keep["z0"], keep["a0"] = z0, a
    for i in range(nb):
        w1, b1, w2, b2 = params[2 + 4 * i:6 + 4 * i]
        z1 = rb(F_.conv2d(a, w1, b1, padding=1))
        t = rb(rf(torch.relu(z1)))
        z2 = F_.conv2d(t, w2, b2, padding=1)
        a = rb(rf(a + z2))
        keep[f"z1_{i}"], keep[f"t_{i}"], keep[f"z2_{i}"], keep[f"a{i + 1}"] = z1, t, z2, a
    if inter is not None:
        for name, t in keep.items():
            if t.requires_grad:
                t.retain_grad()
            inter[name] = t
    return a


def step_ref(frame, prev, flow, params, nb, inter=None, rnd=None):
    """the recurrent step of the propagation loops: trunk(cat([frame, warp(prev, flow)])).  frame (n, 3, h, w); prev (n, F, h, w)
    or None (zero state); flow (n, 2, h, w) pixel displacements, x then y, or None (no warp)."""
    n, _, h, w = frame.shape
    f = params[0].shape[0]
    if prev is None:
        prev = frame.new_zeros(n, f, h, w)
    elif flow is not None:
        prev = warp_ref(prev, flow.permute(0, 2, 3, 1)).to(frame.dtype)
    return trunk_ref(torch.cat([frame, prev], 1), params, nb, inter, rnd)


def run_case(case, dtype=torch.float64, rnd=None, want_inter=False):
    """forward and backward of a case in `dtype`: a dict with 'y' (list, one per step), 'dx' (list: gradient of the trunk's whole
    input for a plain case, of each frame for a step case), 'grads' (one per parameter, state_dict order) and, on request,
    'inter' (one dict per step: every intermediate and, under 'd <name>', its gradient)."""
    nb = case["nb"]
    params = [leaf(p, dtype) for p in case["params"]]
    inters = []
    cot = rnd if rnd is not None else (lambda t: t)
    if "frames" in case:
        ins = [leaf(fr, dtype) for fr in case["frames"]]
        ys, prev = [], None
        for k, fr in enumerate(ins):
            d = {}
            fl = case["flows"][k - 1].to(dtype) if k > 0 else None
            prev = step_ref(fr, prev, fl, params, nb, d, rnd)
            ys.append(prev)
            inters.append(d)
        if "dys" in case:
            torch.autograd.backward(ys, [cot(g.to(dtype)) for g in case["dys"]])
    else:
        ins = [leaf(case["x"], dtype)]
        d = {}
        ys = [trunk_ref(ins[0], params, nb, d, rnd)]
        inters.append(d)
        if "dy" in case:
            ys[0].backward(cot(case["dy"].to(dtype)))
    out = dict(y=[y.detach() for y in ys], dx=[t.grad for t in ins], grads=[p.grad for p in params])
    if rnd is not None:
        out["dx"] = [None if g is None else rnd(g) for g in out["dx"]]
    if want_inter:
        out["inter"] = []
        for d in inters:
            o = {}
            for name, t in d.items():
                o[name] = t.detach()
                if t.grad is not None:
                    o["d " + name] = t.grad
            out["inter"].append(o)
    return out


def emulate(case, mode):
    """the trunk in the kernels' precision on the CPU: 'fp32' -- float32 ATen throughout; 'bf16' -- the float64 graph with a
    rounding to bf16 at every tensor the kernels store in bf16 (trunk_ref's rnd), the cotangent included"""
    if mode == "bf16":
        return run_case(case, torch.float64, bf16_round)
    return run_case(case, torch.float32, None)


# ---- exactness conditions ------------------------------------------------------------------------------------------------
def _check_conv(tag, xin, w, b, dz, wsum):
    """one conv of one step: xin its input, dz the gradient at its output (None: forward only).  wsum: dict that accumulates
    sum |terms| of the weight and bias gradient over the steps."""
    cv = lambda t: t.view(1, -1, 1, 1)
    qx, qw = chan_quantum(xin), lowbit(w).amin((2, 3))                 # (ci,), (co, ci)
    q_out = torch.minimum((qw * qx.view(1, -1)).amin(1), lowbit(b))
    need_sum(f"{tag} forward", F_.conv2d(xin.abs(), w.abs(), b.abs(), padding=1), cv(q_out))
    if dz is None:
        return
    qd = chan_quantum(dz)
    q_in = (qw * qd.view(-1, 1)).amin(0)
    need_sum(f"{tag} backward data", F_.conv_transpose2d(dz.abs(), w.abs(), padding=1), cv(q_in))
    tw = torch.nn.grad.conv2d_weight(xin.abs(), w.shape, dz.abs(), padding=1)
    tb = dz.abs().sum((0, 2, 3))
    key = tag.split(": ", 1)[1]
    if key in wsum:
        tw, tb = tw + wsum[key][0], tb + wsum[key][1]
        qx, qd = torch.minimum(qx, wsum[key][2]), torch.minimum(qd, wsum[key][3])
    wsum[key] = (tw, tb, qx, qd)


def _check_weights(name, w, b):
    if not bool((w != 0).any(0).any(0).all()):
        fail(f"{name}: a tap is zero in every channel pair")
    if not bool((w != 0).any(0).any(1).any(1).all()):
        fail(f"{name}: an input channel carries no weight")
    if not bool((w != 0).any(1).any(1).any(1).all()):
        fail(f"{name}: an output channel carries no weight")
    need_taps(name, w)
    need_biases(name, b)


def check_exact(case):
    """Verify the exactness conditions of an exact case on the float64 reference alone; raises ValueError if one fails.
    Returns run_case()'s result (without the intermediates).  A case without a cotangent ('dy' / 'dys') is a forward case: only
    the forward conditions apply, and its first pre-activation may have either sign ('signs': True)."""
    nb = case["nb"]
    backward = "dy" in case or "dys" in case
    out = run_case(case, want_inter=True)
    params = [p.double() for p in case["params"]]
    names = param_names(nb)
    for k in range(0, len(params), 2):
        _check_weights(names[k][:-7], params[k], params[k + 1])
    for name, p in zip(names, params):
        need_bf16(name, p)
    wsum = {}
    for s, d in enumerate(out["inter"]):
        tag = f"step {s}: "
        if not case.get("signs") and not bool((d["z0"] > 0).all()):
            fail(f"{tag}the first pre-activation is not strictly positive")
        for name, t in d.items():
            if name.startswith("z") or name.startswith("d z2") or (case.get("signs") and name == "a0"):
                continue                                   # pre-activations live in fp32 accumulators; d z2_i is ga_{i+1}
            need_bf16(tag + name, t)
        g = lambda nm: d.get("d " + nm) if backward else None
        _check_conv(tag + names[0][:-7], d["x"], params[0], params[1], g("z0"), wsum)
        for i in range(nb):
            w1, b1, w2, b2 = params[2 + 4 * i:6 + 4 * i]
            _check_conv(tag + names[2 + 4 * i][:-7], d[f"a{i}"], w1, b1, g(f"z1_{i}"), wsum)
            _check_conv(tag + names[4 + 4 * i][:-7], d[f"t_{i}"], w2, b2, g(f"z2_{i}"), wsum)
    for key, (tw, tb, qx, qd) in wsum.items():
        need_sum(f"d {key}.weight", tw, qd.view(-1, 1, 1, 1) * qx.view(1, -1, 1, 1))
        need_sum(f"d {key}.bias", tb, qd)
    finals = [("y", out["y"])] + ([("dx", out["dx"]), ("grads", out["grads"])] if backward else [])
    for name, ts in ([] if case.get("signs") else finals):    # (0.1 z is not dyadic: the sign case bounds it instead)
        for t in ts:
            need_fp32(name, t)
    if not case.get("signs"):
        for t in out["y"] + (out["dx"] if backward else []):
            if not is_bf16(t):
                fail("y or dx is not its own bf16 rounding")
    del out["inter"]
    return out


# ---- exact cases ---------------------------------------------------------------------------------------------------------
_seed = functools.partial(seed, 12345, 7)


def _sparse_conv(cout, cin, layer, g, plus_from=None, nz=2):
    """(cout, cin, 3, 3) with nz weights +-1 per output channel: entry i = co nz + j sits at input channel 7 i + 3 layer (mod cin)
    and tap 2 i + i // 9 + layer (mod 9), so the rows together use every input channel (7 is coprime to every width used) and
    every tap.  plus_from (the first conv of a recurrent case, cin = plus_from + cout): every row reads ONE state channel, with +1,
    and one frame channel -- the state carries the first conv's bias once per step, so a row that read two state channels would
    triple it."""
    assert cout * nz >= max(cin, 9) and cin % 7 != 0 and cout % 7 != 0
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    sg = torch.randint(0, 2, (cout * nz,), generator=g) * 2 - 1
    for i in range(cout * nz):
        ci, tap = (7 * i + 3 * layer) % cin, (2 * i + i // 9 + layer) % 9
        s = float(sg[i])
        if plus_from is not None:
            assert nz == 2 and cin == plus_from + cout
            ci = plus_from + (7 * (i // 2) + 5) % cout if i % 2 == 0 else (i // 2) % plus_from
            s = 1.0 if i % 2 == 0 else s
        w[i // nz, ci, tap // 3, tap % 3] = s
    return w


def _grouped_scales(c, g):
    """(exponent (c,), rank within the group of channels that share an exponent (c,))"""
    ns = max(8, c // 2)
    perm = torch.randperm(c, generator=g)
    return (perm % ns - ns // 2).double(), perm // ns


_ODD = (1.0, -1.0, 3.0, -3.0, 5.0, -5.0, 7.0, -7.0)


def _int_forward(x, ip, nb):
    a = F_.conv2d(x, ip[0], ip[1], padding=1)
    z0 = a
    for i in range(nb):
        t = torch.relu(F_.conv2d(a, ip[2 + 4 * i], ip[3 + 4 * i], padding=1))
        a = a + F_.conv2d(t, ip[4 + 4 * i], ip[5 + 4 * i], padding=1)
    return z0, a


def _draw(cin, f, nb, xs, g, b0_shift=0, warped=False):
    """integer network on the inputs `xs` (the data the conv1 biases are fitted to), then the channel scales.  Returns
    (scaled params, input scale (cin,), output scale (f,), integer params)."""
    ea, rank = _grouped_scales(f, g)
    sa = 2.0 ** ea
    if cin == f + 3:
        sx = torch.cat([2.0 ** torch.randint(-2, 3, (3,), generator=g).double(), sa])     # [frame | state on the stream's scales]
    else:
        sx = 2.0 ** torch.randint(-2, 3, (cin,), generator=g).double()
    ip, sp = [], []
    w0 = _sparse_conv(f, cin, 0, g, plus_from=3 if warped else None)
    b0 = torch.tensor([3.0 + 2.0 * int(r) for r in rank], dtype=torch.float64) + b0_shift
    ip += [w0, b0]
    sp += [w0 * sa.view(-1, 1, 1, 1) / sx.view(1, -1, 1, 1), b0 * sa]
    a = torch.cat([F_.conv2d(x, w0, b0, padding=1) for x in xs], 0)
    for i in range(nb):
        et, _ = _grouped_scales(f, g)
        st = 2.0 ** et
        w1 = _sparse_conv(f, f, 1 + 2 * i, g)
        pre = F_.conv2d(a, w1, None, padding=1)
        top = pre.amax((0, 2, 3))
        b1, used = torch.zeros(f, dtype=torch.float64), set()
        for c in range(f):
            m = 2 + int(torch.randint(0, 3, (1,), generator=g))
            while float(top[c]) == m or float((m - top[c]) * st[c]) in used:
                m += 1
            b1[c] = m - top[c]
            used.add(float(b1[c] * st[c]))
        t = torch.relu(pre + b1.view(1, -1, 1, 1))
        w2 = _sparse_conv(f, f, 2 + 2 * i, g)
        rot = int(torch.randint(0, 4, (1,), generator=g))
        b2 = torch.tensor([_ODD[(int(r) + rot) % len(_ODD)] for r in rank], dtype=torch.float64)
        a = a + F_.conv2d(t, w2, b2, padding=1)
        ip += [w1, b1, w2, b2]
        sp += [w1 * st.view(-1, 1, 1, 1) / sa.view(1, -1, 1, 1), b1 * st, w2 * sa.view(-1, 1, 1, 1) / st.view(1, -1, 1, 1), b2 * sa]
    return [p.float() for p in sp], sx, sa, ip


def _sparse_int(shape, lo, hi, density, g):
    t = torch.randint(lo, hi + 1, shape, generator=g).double()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density).double()
    return t


@functools.lru_cache(maxsize=None)
def exact_case(cin, f, nb, n, h, w, seed=0, dy_density=0.25, forward_only=False):
    """One trunk call on dyadic data; checked by check_exact() before it is returned (raises if a condition fails).  Cached: the
    tensors are shared and must not be written to."""
    g = torch.Generator().manual_seed(_seed(1, cin, f, nb, n, h, w, seed))
    x = _sparse_int((n, cin, h, w), -1, 1, 1.0, g)
    params, sx, sa, _ = _draw(cin, f, nb, [x], g)
    case = dict(nb=nb, params=params, x=(x * sx.view(1, -1, 1, 1)).float())
    if not forward_only:
        case["dy"] = (_sparse_int((n, f, h, w), -1, 1, dy_density, g) / sa.view(1, -1, 1, 1)).float()
    case["ref"] = check_exact(case)
    return case


@functools.lru_cache(maxsize=None)
def exact_sign_case(cin, f, n, h, w, seed=0):
    """the first conv alone (nb = 0), forward only, with pre-activations of both signs and some exactly zero: the biases are small,
    so z = +-x +- x + b crosses zero"""
    g = torch.Generator().manual_seed(_seed(2, cin, f, n, h, w, seed))
    x = _sparse_int((n, cin, h, w), -3, 3, 1.0, g)
    params, sx, sa, ip = _draw(cin, f, 0, [x], g, b0_shift=-4)          # biases -1, 1, 3 (and 5 ..): nonzero, distinct per scale group
    case = dict(nb=0, params=params, x=(x * sx.view(1, -1, 1, 1)).float(), signs=True)
    case["ref"] = check_exact(case)
    z = F_.conv2d(case["x"].double(), params[0].double(), params[1].double(), padding=1)
    if not (bool((z > 0).any()) and (bool((z < 0).any()) and bool((z == 0).any()) or n * h * w < 4)):
        fail("the sign case lacks a sign")
    case["z"] = z
    return case


def exact_shift_flow(n, h, w, shift):
    """(n, 2, h, w) float32, integer-valued: the uniform displacement `shift` = (x, y), except where the fp32 normalise /
    un-normalise round trip of the op (2 g / (size - 1) - 1, then ((v + 1) / 2) (size - 1), each operation rounded once) does not
    return the integer position exactly -- there the displacement moves to the nearest integer whose round trip is exact (position
    0 and size - 1 always are), so that every sample is a pure copy or a zero in fp32 as in float64.  The division is a tensor by
    a tensor: torch divides a tensor by a Python scalar by multiplying with the rounded reciprocal, which is not the IEEE quotient."""
    flow = torch.empty(n, 2, h, w)
    for k, size in ((0, w), (1, h)):
        grid = torch.arange(size, dtype=torch.float32)
        d = float(max(size - 1, 1))

        def exact(gpos):
            v = (2.0 * gpos) / torch.full_like(gpos, d) - 1.0
            return ((v + 1.0) * 0.5) * float(size - 1) == gpos

        want = grid + float(shift[k])
        pos = want.clone()
        for delta in sorted(range(-size - 2, size + 3), key=abs):
            cand = want + float(delta)
            pos = torch.where(exact(pos), pos, cand)
        assert bool(exact(pos).all())
        if size == 1:
            pos = want                                      # the position component is 0 whatever the flow says
        line = pos - grid
        flow[:, k] = line.view(1, 1, w) if k == 0 else line.view(1, h, 1)
    return flow


@functools.lru_cache(maxsize=None)
def exact_step_case(f, nb, n, h, w, shifts=((1, 0),), seed=0, dy_density=0.25, forward_only=False):
    """1 + len(shifts) recurrent steps of one trunk(F + 3, F, nb) on dyadic data: step 0 from the zero state, step k warps the output
    of step k - 1 by the integer flow exact_shift_flow(shifts[k - 1]); a cotangent on every output.  The state enters the first
    conv with +1 weights only and the first conv's bias is raised until the pre-activation of every step is positive."""
    cin, shift = f + 3, 0
    for _ in range(24):
        g = torch.Generator().manual_seed(_seed(3, f, nb, n, h, w, seed))
        frames = [_sparse_int((n, 3, h, w), -1, 1, 1.0, g) for _ in range(1 + len(shifts))]
        x0 = torch.cat([frames[0], torch.zeros(n, f, h, w, dtype=torch.float64)], 1)
        params, sx, sa, ip = _draw(cin, f, nb, [x0], g, b0_shift=shift, warped=True)
        flows = [exact_shift_flow(n, h, w, s) for s in shifts]
        zmin, prev = 1.0, None
        for k, fr in enumerate(frames):                     # the integer network, step by step
            st = torch.zeros(n, f, h, w, dtype=torch.float64) if prev is None else warp_ref(prev, flows[k - 1].permute(0, 2, 3, 1))
            z0, prev = _int_forward(torch.cat([fr, st], 1), ip, nb)
            zmin = min(zmin, float(z0.min()))
        if zmin >= 1.0:
            break
        shift += 2 * int((2.0 - zmin) // 2 + 1)
    dys = [(_sparse_int((n, f, h, w), -1, 1, dy_density, g) / sa.view(1, -1, 1, 1)).float() for _ in frames]
    case = dict(nb=nb, params=params, frames=[(fr * sx[:3].view(1, -1, 1, 1)).float() for fr in frames], flows=flows)
    if not forward_only:
        case["dys"] = dys
    case["ref"] = check_exact(case)
    return case


# the cases of the parity tests (16 x 16 tiles; halo 1 per conv, 2 in the pair kernels, 4 in the quad kernel): (n, h, w)
GEOMETRIES = (
    (1, 1, 1), (1, 1, 37), (1, 37, 1), (1, 3, 3), (1, 4, 5),            # inside the 4-pixel halo on both sides
    (1, 15, 15), (1, 16, 16), (1, 17, 17),                              # one tile under / exact / one-pixel slivers
    (1, 16, 33), (1, 33, 16), (1, 20, 36),
    (1, 48, 48),                                                        # 3 x 3 tiles: an interior tile whose halo is all live
    (1, 35, 50),                                                        # uneven last row and column of tiles
    (3, 17, 18),                                                        # the batch stride
)
TRUNKS = ((27, 24), (24, 24))                                           # (cin, F) of test a, nb = 3
BLOCK_COUNTS = (0, 1, 2, 4)                                             # first conv alone, pair only, quad only, two quads
BLOCK_COUNT_GEOMETRIES = ((1, 17, 33), (2, 16, 16))
NARROW = (23, 20, 2)
NARROW_GEOMETRIES = ((1, 17, 18), (2, 16, 16))
STEP_NB = 1
STEP_CASES = (((1, 16, 16), ((2, -1),)), ((2, 17, 33), ((-3, 2), (36, 0))), ((1, 5, 40), ((1, 1), (0, -7))))   # (geometry, shifts)
PAIR_CASES = ((2, 17, 18), (6, 17, 18), (2, 33, 16), (6, 33, 16))      # whole batch: half per trunk
TILE_LOOP_GEOMETRY = (3, 32, 32)                                         # 12 tiles; paired: 6 images, 24 tiles
TILE_LOOP_DENSITY = 0.5
TILE_LOOP_WGS = (1, 5, 12, 13, None)
MANY_TILES = (5, 64, 64)                                                 # 80 tiles > the default cap of 64 workgroups
MANY_TILES_DENSITY = 0.125
SIGN_GEOMETRIES = ((1, 17, 18), (2, 5, 33))
WIDE_GEOMETRIES = ((1, 1, 1), (1, 3, 3), (1, 16, 16), (1, 17, 17), (1, 16, 33), (1, 48, 48), (3, 17, 18))
WIDE_TRUNKS = ((67, 64, 3), (64, 64, 2), (43, 40, 2))
WIDE_STEP_GEOMETRIES = ((1, 17, 17), (3, 17, 18))
WIDE_STEP_SHIFTS = ((1, -2),)


def pair_halves(n, h, w, nb=3, density=0.25):
    """the two exact cases of a paired call on a batch of n: different seeds, so different weights and data per trunk"""
    return exact_case(27, 24, nb, n // 2, h, w, 1, density), exact_case(27, 24, nb, n // 2, h, w, 2, density)


# ---- rounded cases -------------------------------------------------------------------------------------------------------
ROUNDED_GEOMETRIES = ((2, 20, 28), (1, 48, 48))


@functools.lru_cache(maxsize=None)
def rounded_case(cin, f, nb, n, h, w, mode, seed=0):
    """random normal data, PyTorch-default-sized weights, biases of both signs (so the first pre-activation has both signs).
    Nothing is rounded beforehand in either mode: rounding the input, the weights and the cotangent to bf16 is part of what the
    bf16 route does, so it belongs to the emulation and to the yardstick.  Cached: shared, not to be written to."""
    g = torch.Generator().manual_seed(_seed(4, cin, f, nb, n, h, w, seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    params = []
    for k in range(1 + 2 * nb):
        ci = cin if k == 0 else f
        params += [rn(f, ci, 3, 3) / (3.0 * ci ** 0.5), 0.1 * rn(f)]
    return dict(nb=nb, params=params, x=rn(n, cin, h, w), dy=rn(n, f, h, w))


def tensors_of(out):
    """[y, dx, every parameter gradient] of a plain case's result"""
    return [out["y"][0], out["dx"][0]] + list(out["grads"])


def tensor_names(nb):
    return ["y", "dx"] + ["d " + k for k in param_names(nb)]


@functools.lru_cache(maxsize=None)
def rounded_reference(cin, f, nb, n, h, w, mode, seed=0):
    """(case, float64 reference [y, dx, grads], yardstick per tensor): the yardstick is the distance of the CPU emulation of the
    kernels' precision from the float64 reference, in the tests' metric -- computed from the reference alone"""
    case = rounded_case(cin, f, nb, n, h, w, mode, seed)
    ref = tensors_of(run_case(case))
    emu = tensors_of(emulate(case, mode))
    return case, ref, [rel_max(a, b) for a, b in zip(emu, ref)]
