"""Trunk parity: the 3x3 convolution kernels of the BasicVSR propagation trunk (csrc/conv3x3.h, and the 64-wide inference kernels
of csrc/conv64.h), driven through the public routes -- ConvResidualBlocks.__call__, forward_warped, forward_warped_pair, weights
through load_state_dict -- against tests/trunk_ref.py (plain torch, float64, CPU): features, input gradients and every entry of
flat.grad, fp32 and bf16.

  exact cases    dyadic data on which the kernels must return the reference bit for bit whatever their summation order and
                 rounding points (conditions: tests/trunk_ref.py, verified on the host by tests/test_trunk_ref_host.py): every
                 geometry at the edges of the 16 x 16 tile and of the 1-, 2- and 4-pixel halos; 0, 1, 2, 3 and 4 blocks (first
                 conv alone, pair launch, quad launch, quad + pair, two quads); the narrow embed; the gathered first conv over
                 two and three recurrent steps with integer flows; two trunks in one launch; the weight-gradient tile loop at
                 SR_C3_WGRAD_WGS below, at and above the number of tiles and at the default cap with 80 tiles
  sign cases     the negative LeakyReLU side: exact where z > 0, within the two (fp32) or three (bf16) roundings of 0.1 z elsewhere
  rounded cases  random normal data; per tensor, max |got - ref| / max |ref| within 8 x (fp32) or 4 x (bf16) the same metric
                 of a CPU emulation of the kernels' precision (+ 1e-6 in fp32); the ratio to that yardstick is printed for
                 every tensor and DESIGN.md keeps the table
"""
import pytest
import torch

from tests import trunk_ref as R
from tests.parity_kit import hold_exact, hold_rounded

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
_gid = lambda g: "%dx%dx%d" % g


def _module(cin, f, params, dtype):
    from mobilesuperresolution_amd.models import ConvResidualBlocks
    m = ConvResidualBlocks(cin, f, (len(params) - 2) // 4, hot_dtype=dtype)
    m.load_state_dict(R.state_dict_of(params), strict=True)
    return m.cuda()


def _flat_grads(m):
    return [g.cpu() for _, g in m.named_tensors(m.flat.grad)]


def _hold_exact(tag, names, got, ref):
    assert len(names) == len(got) == len(ref), (tag, len(names), len(got), len(ref))
    hold_exact(tag, zip(names, got, ref))


def _run_plain(case, cin, f, dtype):
    """ConvResidualBlocks.__call__ -> _TrunkFunction: [y, dx, every entry of flat.grad]"""
    m = _module(cin, f, case["params"], dtype)
    x = case["x"].cuda().requires_grad_(True)
    y = m(x)
    y.backward(case["dy"].cuda())
    return [y, x.grad] + _flat_grads(m)


def _exact_plain(cin, f, nb, geom, dtype, seed=0, density=0.25):
    case = R.exact_case(cin, f, nb, *geom, seed, density)
    _hold_exact((cin, f, nb, geom, dtype), R.tensor_names(nb), _run_plain(case, cin, f, dtype), R.tensors_of(case["ref"]))


# ---- a. exact geometries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("trunk", R.TRUNKS, ids=lambda t: "%dto%d" % t)
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_gid)
def test_exact_geometries(geom, trunk, dtype):
    """three blocks (bf16: the quad launch for blocks 0-1, the pair launch for block 2; fp32: the per-layer kernels): images inside
    the 4-pixel halo, one tile under / exact / one-pixel slivers, 3 x 3 tiles with an interior tile, uneven last tiles, a batch of 3"""
    _exact_plain(*trunk, 3, geom, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("trunk", R.TRUNKS, ids=lambda t: "%dto%d" % t)
@pytest.mark.parametrize("nb", R.BLOCK_COUNTS)
def test_exact_block_counts(nb, trunk, dtype):
    """the first conv alone, the pair launch only, the quad launch only, two quad launches"""
    for geom in R.BLOCK_COUNT_GEOMETRIES:
        _exact_plain(*trunk, nb, geom, dtype)


# ---- b. narrow embed -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("geom", R.NARROW_GEOMETRIES, ids=_gid)
def test_exact_narrow_embed(geom, dtype):
    """ConvResidualBlocks(23, 20, 2) inside the 24-wide kernels: every real gradient entry equals the reference, and the padded
    channels 20..23 of the state handle are exactly zero"""
    cin, f, nb = R.NARROW
    _exact_plain(cin, f, nb, geom, dtype)
    case = R.exact_case(cin, f, nb, *geom)
    m = _module(cin, f, case["params"], dtype)
    x = case["x"].cuda()
    state = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 24, dtype=DTYPES[dtype], device="cuda")
    state[..., :f] = x[:, 3:].permute(0, 2, 3, 1)
    with torch.no_grad():
        y, handle = m.forward_warped(x[:, :3].contiguous(), state)
    _hold_exact((geom, dtype, "forward_warped"), ["y"], [y], case["ref"]["y"])
    assert handle.shape == state.shape and handle.dtype == DTYPES[dtype]
    assert torch.equal(handle[..., :f].float().cpu(), case["ref"]["y"][0].permute(0, 2, 3, 1).float())
    assert int((handle[..., f:] != 0).sum()) == 0


# ---- c. the gathered first conv over recurrent steps -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("spec", R.STEP_CASES, ids=lambda s: _gid(s[0]))
def test_exact_recurrent_steps(spec, dtype):
    """y_0, state = forward_warped(f_0); y_k, state = forward_warped(f_k, state, flow_k) with integer flows (one of them moves the whole
    state off the image); a loss on every output: features, every frame's gradient and flat.grad (c3_fwd<WARP>, x0_save and
    c3_wgrad on the saved input, the state gradient through the gather-form warp backward).

    16x16 and 5x40 (size - 1 not a power of two) are what found the contraction in warp_taps: wx = fma(h, size - 1, -floor(px)) left
    the rounding residual of the position (a few 1e-7) as a blend weight where the position rounds to an integer, and y_1 came out one
    fp32 ulp off in 2001 of 6144 elements."""
    geom, shifts = spec
    case = R.exact_step_case(24, R.STEP_NB, *geom, shifts)
    m = _module(27, 24, case["params"], dtype)
    frames = [fr.cuda().requires_grad_(True) for fr in case["frames"]]
    ys, state = [], None
    for k, fr in enumerate(frames):
        y, state = m.forward_warped(fr, state, case["flows"][k - 1].cuda() if k > 0 else None)
        ys.append(y)
    torch.autograd.backward(ys, [g.cuda() for g in case["dys"]])
    ref = case["ref"]
    ns = len(frames)
    names = [f"y{k}" for k in range(ns)] + [f"dframe{k}" for k in range(ns)] + R.tensor_names(R.STEP_NB)[2:]
    _hold_exact((geom, shifts, dtype), names, ys + [fr.grad for fr in frames] + _flat_grads(m), ref["y"] + ref["dx"] + ref["grads"])


# ---- d. two trunks in one launch -------------------------------------------------------------------------------------------
def _run_pair(ca, cb, dtype):
    """forward_warped_pair on [ca's batch | cb's batch] with the 27-channel input split into frame and (unwarped) state: per half
    [y, dframe, dstate (NHWC), flat.grad entries]"""
    from mobilesuperresolution_amd.models.basicvsr_arch import forward_warped_pair
    ma, mb = _module(27, 24, ca["params"], dtype), _module(27, 24, cb["params"], dtype)
    x = torch.cat([ca["x"], cb["x"]])
    half = ca["x"].shape[0]
    frame = x[:, :3].contiguous().cuda().requires_grad_(True)
    state = x[:, 3:].permute(0, 2, 3, 1).to(DTYPES[dtype]).contiguous().cuda().requires_grad_(True)
    fa, fb, _ = forward_warped_pair(ma, mb, frame, state)
    torch.autograd.backward([fa, fb], [ca["dy"].cuda(), cb["dy"].cuda()])
    out = []
    for sl, y, m in ((slice(0, half), fa, ma), (slice(half, None), fb, mb)):
        out.append([y, frame.grad[sl], state.grad[sl]] + _flat_grads(m))
    return out


def _hold_pair(tag, ca, cb, dtype):
    nb = ca["nb"]
    names = ["y", "dframe", "dstate"] + R.tensor_names(nb)[2:]
    for which, case, got in zip("ab", (ca, cb), _run_pair(ca, cb, dtype)):
        y, dx = case["ref"]["y"][0], case["ref"]["dx"][0]
        _hold_exact(tag + (which,), names, got, [y, dx[:, :3], dx[:, 3:].permute(0, 2, 3, 1)] + case["ref"]["grads"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("geom", R.PAIR_CASES, ids=_gid)
def test_exact_two_trunks_in_one_launch(geom, dtype):
    """different weights per trunk: each half's features, input gradients and flat.grad equal the reference run with that trunk's
    weights on that half alone (a kernel that ignored n_dir, or split the weight-gradient grid at the wrong image, fails)"""
    ca, cb = R.pair_halves(*geom)
    assert not torch.equal(ca["params"][0], cb["params"][0])
    _hold_pair((geom, dtype), ca, cb, dtype)


# ---- e. the weight-gradient tile loop --------------------------------------------------------------------------------------
def _set_wgs(monkeypatch, wgs):
    if wgs is None:
        monkeypatch.delenv("SR_C3_WGRAD_WGS", raising=False)
    else:
        monkeypatch.setenv("SR_C3_WGRAD_WGS", str(wgs))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("wgs", R.TILE_LOOP_WGS)
def test_tile_loop_workgroup_counts(monkeypatch, wgs, dtype):
    """12 tiles under a cap of 1, 5, 12, 13 and 64 workgroups: twelve trips, uneven trips, one trip each; the slabs of every count
    sum to the reference, bit for bit"""
    assert R.n_tiles(*R.TILE_LOOP_GEOMETRY) == 12
    _set_wgs(monkeypatch, wgs)
    _exact_plain(27, 24, 3, R.TILE_LOOP_GEOMETRY, dtype, 0, R.TILE_LOOP_DENSITY)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("wgs", R.TILE_LOOP_WGS)
def test_tile_loop_workgroup_counts_two_trunks(monkeypatch, wgs, dtype):
    """6 images, 24 tiles, 12 per trunk: the cap is halved per trunk, so a cap of 1 has to be clamped to one workgroup per trunk"""
    n, h, w = R.TILE_LOOP_GEOMETRY
    _set_wgs(monkeypatch, wgs)
    ca, cb = R.pair_halves(2 * n, h, w, 3, R.TILE_LOOP_DENSITY)
    _hold_pair((wgs, dtype), ca, cb, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tile_loop_at_the_production_default(monkeypatch, dtype):
    """80 tiles under the default cap of 64 workgroups: 40 workgroups of two trips"""
    monkeypatch.delenv("SR_C3_WGRAD_WGS", raising=False)
    assert R.n_tiles(*R.MANY_TILES) == 80
    _exact_plain(27, 24, 3, R.MANY_TILES, dtype, 0, R.MANY_TILES_DENSITY)


# ---- f. the negative LeakyReLU side ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("geom", R.SIGN_GEOMETRIES, ids=_gid)
def test_leaky_relu_negative_side(geom, dtype):
    """the first conv alone on exact pre-activations z of both signs, some exactly zero: equal to z where z > 0; elsewhere within the
    roundings of 0.1 z -- the constant 0.1f and the product (2^-22 relative in fp32), and the store to bf16 (2^-8 in bf16)"""
    case = R.exact_sign_case(27, 24, *geom)
    m = _module(27, 24, case["params"], dtype)
    with torch.no_grad():
        y = m(case["x"].cuda()).cpu().double()
    z = case["z"]
    pos = z > 0
    assert bool(pos.any()) and bool((z < 0).any()) and bool((z == 0).any())
    assert torch.equal(y[pos], z[pos]), int((y[pos] != z[pos]).sum())
    want = 0.1 * z[~pos]
    err = (y[~pos] - want).abs()
    bound = (2.0 ** -22 if dtype == "fp32" else 2.0 ** -8) * want.abs()
    worst = float((err / want.abs().clamp_min(1e-300)).max())
    print(f"trunk parity | leaky {dtype} {_gid(geom)} | worst relative error on z <= 0: {worst:.3e}")
    assert bool((err <= bound).all()), (int((err > bound).sum()), worst)


# ---- g. rounded cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("geom", R.ROUNDED_GEOMETRIES, ids=_gid)
def test_rounded(geom, dtype):
    case, ref, yard = R.rounded_reference(27, 24, 3, *geom, dtype)
    got = _run_plain(case, 27, 24, dtype)
    hold_rounded("trunk parity", f"{dtype} {_gid(geom)}", dtype, zip(R.tensor_names(3), got, ref, yard))


# ---- 3. the 64-wide inference trunk, forward only --------------------------------------------------------------------------
def _wide_state(x, f, dtype):
    state = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 64, dtype=DTYPES[dtype], device="cuda")
    state[..., :f] = x[:, 3:].permute(0, 2, 3, 1)
    return state


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("trunk", R.WIDE_TRUNKS, ids=lambda t: "%dto%dx%d" % t)
def test_wide_exact_geometries(trunk, dtype):
    """c64_conv_kernel, the bf16 c64_resblock_kernel and the embed of packing.c64_tables on the plain route"""
    cin, f, nb = trunk
    for geom in R.WIDE_GEOMETRIES:
        case = R.exact_case(cin, f, nb, *geom, 0, 0.25, True)
        m = _module(cin, f, case["params"], dtype)
        with torch.no_grad():
            y = m(case["x"].cuda())
        _hold_exact((trunk, geom, dtype), ["y"], [y], case["ref"]["y"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("trunk", [t for t in R.WIDE_TRUNKS if t[0] == t[1] + 3], ids=lambda t: "%dto%dx%d" % t)
def test_wide_exact_recurrent_steps(trunk, dtype):
    """two forward_warped steps with an integer flow; the padded channels of the state handle stay zero."""
    cin, f, nb = trunk
    for geom in R.WIDE_STEP_GEOMETRIES:
        case = R.exact_step_case(f, nb, *geom, R.WIDE_STEP_SHIFTS, 0, 0.25, True)
        m = _module(cin, f, case["params"], dtype)
        ys, state = [], None
        with torch.no_grad():
            for k, fr in enumerate(case["frames"]):
                y, state = m.forward_warped(fr.cuda(), state, case["flows"][k - 1].cuda() if k > 0 else None)
                ys.append(y)
                assert int((state[..., f:] != 0).sum()) == 0
        _hold_exact((trunk, geom, dtype), ["y0", "y1"], ys, case["ref"]["y"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("trunk", [t for t in R.WIDE_TRUNKS if t[0] == t[1] + 3], ids=lambda t: "%dto%dx%d" % t)
def test_wide_exact_two_trunks_in_one_launch(trunk, dtype):
    """the paired call with different weights at batch 2: each half equals the reference of its own trunk"""
    from mobilesuperresolution_amd.models.basicvsr_arch import forward_warped_pair
    cin, f, nb = trunk
    ca, cb = (R.exact_case(cin, f, nb, 1, 17, 18, seed, 0.25, True) for seed in (1, 2))
    ma, mb = _module(cin, f, ca["params"], dtype), _module(cin, f, cb["params"], dtype)
    x = torch.cat([ca["x"], cb["x"]]).cuda()
    with torch.no_grad():
        fa, fb, _ = forward_warped_pair(ma, mb, x[:, :3].contiguous(), _wide_state(x, f, dtype))
    _hold_exact((trunk, dtype, "a"), ["y"], [fa], ca["ref"]["y"])
    _hold_exact((trunk, dtype, "b"), ["y"], [fb], cb["ref"]["y"])
