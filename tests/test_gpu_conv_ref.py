"""Conv parity: the two dense k x k implicit-GEMM families -- SPyNet's 7x7 layers (csrc/spynet_conv.h) and the searched network's
block, tail, weight-gradient and un-shuffle kernels (csrc/result_block.h) -- driven through the public entries (sr_conv7_fwd with
packing.conv7_tables as BasicModule._pack does, BasicModule.forward, SpyNet.forward, the hotpath.rm_* functions) against
tests/conv_ref.py (plain torch, float64, CPU).  Output buffers are pre-filled with NaN (a sentinel where the kernel accumulates or
writes integers), so an unwritten element shows.

  exact cases    dyadic data on which the kernels must return the reference bit for bit whatever their summation order, the
                 stored value being the exact one rounded once to the hot dtype (conditions: tests/conv_ref.py, verified on the
                 host by tests/test_conv_ref_host.py).  conv7: all five layers at the edges of the 8 x 32 tile and inside the
                 3-pixel halo; tap-identity sets (one weight per output channel; a failure names the tap); the five layers
                 chained; the _pack cache.  Result_Model: fp32 and bf16, k = 3, 5, 7, at the edges of the 32 x 16 / 32 x 8 conv
                 tile and of the 16 x 16 weight-gradient tile, five channel windows, the tail at R = 2, 3, 4 added onto a
                 non-zero base, and the weight-gradient tile loop with 1 .. 256 workgroups for 6 tiles and 4 for 30
  rounded cases  random normal data; per tensor, max |got - ref| / max |ref| within 8 x (fp32, + 1e-6) or 4 x (bf16) the same
                 metric of conv_ref.emulate(); the ratio to that yardstick is printed for every tensor and DESIGN.md keeps the table
"""
import pytest
import torch

from tests import conv_ref as R
from tests.parity_kit import hold_exact, hold_rounded, seed

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
SENTINEL = 0x5A5A5A5A
_gid = lambda g: "%dx%dx%d" % g


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().cuda().to(dtype)


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


def _hold_exact(tag, got, ref, names):
    """a tensor that came back in bf16 is held to the reference rounded once, '<name>_bf16', where the reference has one"""
    hold_exact(tag, [(n, got[n], ref[n + "_bf16" if got[n].dtype == torch.bfloat16 and n + "_bf16" in ref else n]) for n in names])


def _hold_rounded(tag, mode, got, ref, yard):
    hold_rounded("conv parity", tag, mode, [(n, got[n], ref[n], e_ref) for n, e_ref in yard.items()])


# =============================================================================================================================
# SPyNet's 7x7 convolutions
# =============================================================================================================================
def _conv7(case):
    """sr_conv7_fwd on one layer, packed as BasicModule._pack packs it: y (n, cout, h, w), bf16 (the last layer: fp32)"""
    from mobilesuperresolution_amd import _lib as L, packing as P
    cin, cout, relu = R.LAYERS[case["layer"]]
    n, _, h, w = case["x"].shape
    tab = P.conv7_tables(cin, cout)
    src = torch.cat([case["w"].cuda().reshape(-1), torch.zeros(1, device="cuda")])
    wp = src.index_select(0, torch.from_numpy(tab["idx"]).cuda()).to(torch.bfloat16).contiguous()
    bias = torch.zeros(tab["mt"] * 32, device="cuda")
    bias[:cout] = case["b"].cuda()
    xin = _nhwc(case["x"], torch.bfloat16)
    last = cout == 2
    y = torch.full((n, h, w, cout), float("nan"), dtype=torch.float32 if last else torch.bfloat16, device="cuda")
    L.launch("sr_conv7_fwd", L.lib().sr_conv7_fwd, xin.data_ptr(), wp.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, w, cin, cout,
             1 if relu else 0, 1 if last else 0, L.stream_ptr())
    return dict(y=_nchw(y))


@pytest.mark.parametrize("layer", range(5), ids=lambda i: "%dto%d" % R.LAYERS[i][:2])
@pytest.mark.parametrize("geom", R.CONV7_GEOMETRIES, ids=_gid)
def test_conv7_exact_geometries(geom, layer):
    """dense +-2^k weights: images inside the halo, one tile under / exact / one-pixel slivers of the 8 x 32 tile, several tiles in
    both directions, a batch of 3"""
    case = R.conv7_exact_case(layer, *geom)
    _hold_exact((layer, geom), _conv7(case), case["ref"], ["y"])


@pytest.mark.parametrize("layer", range(5), ids=lambda i: "%dto%d" % R.LAYERS[i][:2])
def test_conv7_tap_identity(layer):
    """one weight per output channel: the output is a shifted copy of one input channel plus the bias.  The sets cover all 49 taps
    and every input channel (cin = 8: kx = 6, the partner of the zero tap, with every channel)."""
    bad = []
    for j, case in enumerate(R.conv7_tap_cases(layer, *R.CONV7_TAP_GEOMETRY)):
        got = _conv7(case)["y"]
        exp = case["ref"]["y_bf16" if got.dtype == torch.bfloat16 else "y"].to(got.dtype)
        ne = (got != exp) | (got != got)
        for co in ne.any(0).any(1).any(1).nonzero().flatten().tolist():
            ci, ky, kx = case["taps"][co]
            bad.append(f"case {j} output channel {co}: tap (ky {ky}, kx {kx}) of input channel {ci}: {int(ne[:, co].sum())} elements differ")
    assert not bad, (R.LAYERS[layer], bad)


def _chain_state_dict(params):
    return {f"basic_module.{2 * i}.{p}": params[2 * i + j].clone() for i in range(5) for j, p in enumerate(("weight", "bias"))}


@pytest.mark.parametrize("geom", R.CHAIN_GEOMETRIES, ids=_gid)
def test_basic_module_chain_exact(geom):
    """the five layers through BasicModule.forward (weights through load_state_dict): every inter-layer tensor is its own bf16
    rounding, so the fp32 flow equals the float64 reference bit for bit"""
    from mobilesuperresolution_amd.models.spynet_arch import BasicModule
    case = R.chain_exact_case(*geom)
    m = BasicModule()
    m.load_state_dict(_chain_state_dict(case["params"]), strict=True)
    y = m.cuda()(case["x"].cuda())
    assert y.dtype == torch.float32
    _hold_exact(geom, dict(y=y), case["ref"], ["y"])


def test_basic_module_pack_cache_follows_the_parameters():
    """_pack keeps the packed weights until a parameter changes: after .cuda() on a fresh module, after load_state_dict of other
    weights, and after an in-place weight.mul_ / bias.add_ the output is the reference's for the weights the module holds now"""
    from mobilesuperresolution_amd.models.spynet_arch import BasicModule
    geom = R.CHAIN_GEOMETRIES[0]
    ca, cb = R.chain_exact_case(*geom), R.chain_exact_case(*geom, 1)
    assert not torch.equal(ca["params"][0], cb["params"][0])
    m = BasicModule()
    m.load_state_dict(_chain_state_dict(ca["params"]), strict=True)
    m = m.cuda()
    x = ca["x"].cuda()
    _hold_exact("fresh .cuda()", dict(y=m(x)), ca["ref"], ["y"])
    _hold_exact("second call", dict(y=m(x)), ca["ref"], ["y"])
    m.load_state_dict(_chain_state_dict(cb["params"]), strict=True)
    _hold_exact("load_state_dict", dict(y=m(cb["x"].cuda())), cb["ref"], ["y"])
    with torch.no_grad():
        m.basic_module[8].weight.mul_(2.0)
    params = list(cb["params"])
    params[8] = params[8] * 2.0
    ref = R.check_exact(dict(kind="chain", x=cb["x"], params=params))
    assert not torch.equal(ref["y"], cb["ref"]["y"])
    _hold_exact("weight.mul_", dict(y=m(cb["x"].cuda())), ref, ["y"])
    with torch.no_grad():
        m.basic_module[8].bias.add_(0.5)
    params[9] = params[9] + 0.5
    ref = R.check_exact(dict(kind="chain", x=cb["x"], params=params))
    _hold_exact("bias.add_", dict(y=m(cb["x"].cuda())), ref, ["y"])


@pytest.mark.parametrize("layer", range(5), ids=lambda i: "%dto%d" % R.LAYERS[i][:2])
def test_conv7_rounded(layer):
    for geom in R.CONV7_ROUNDED_GEOMETRIES:
        case, ref, yard = R.rounded_reference("conv7", "bf16", layer, *geom)
        _hold_rounded("conv7 %dto%d %s" % (R.LAYERS[layer][:2] + (_gid(geom),)), "bf16", _conv7(case), ref, yard)


def test_basic_module_rounded():
    from mobilesuperresolution_amd.models.spynet_arch import BasicModule
    case, ref, yard = R.rounded_reference("chain", "bf16", *R.CHAIN_ROUNDED_GEOMETRY)
    m = BasicModule()
    m.load_state_dict(_chain_state_dict(case["params"]), strict=True)
    y = m.cuda()(case["x"].cuda())
    _hold_rounded("BasicModule " + _gid(R.CHAIN_ROUNDED_GEOMETRY), "bf16", dict(y=y), ref, yard)


@pytest.mark.parametrize("geom", R.SPYNET_ROUNDED, ids=_gid)
def test_spynet_rounded(geom):
    """SpyNet.forward against spynet_ref in float64; the yardstick is spynet_ref in float32 with the BasicModules' bf16 roundings.
    40 x 56 takes the resize branch.  32 x 32 is below what the network can take: five poolings leave a 1 x 1 image and the initial
    flow is 0 x 0, which the first upsampling refuses -- in the reference network and in spynet_ref alike; there the case holds the
    hot path to the same RuntimeError, and 64 x 64 is the smallest image that has a flow to compare."""
    from mobilesuperresolution_amd.models import SpyNet
    n, h, w = geom
    torch.manual_seed(151)
    net = SpyNet().eval()
    g = torch.Generator().manual_seed(seed(*R.SEED, 10, *geom))
    ref_img = torch.rand(n, 3, h, w, generator=g)
    supp = (0.7 * torch.roll(ref_img, (1, 2), (2, 3)) + 0.3 * torch.rand(n, 3, h, w, generator=g)).contiguous()
    sd = net.state_dict()
    net = net.cuda()
    if max(h, w) <= 32:
        with pytest.raises(RuntimeError, match="sizes should be greater than 0") as want_err:
            R.spynet_ref(ref_img, supp, sd)
        with pytest.raises(RuntimeError, match="sizes should be greater than 0") as got_err:
            net(ref_img.cuda(), supp.cuda())
        assert str(got_err.value).split(",")[0] == str(want_err.value).split(",")[0]
        return
    want = R.spynet_ref(ref_img, supp, sd)
    yard = R.rel_max(R.spynet_ref(ref_img, supp, sd, R.bf16_round, torch.float32), want)
    flow = net(ref_img.cuda(), supp.cuda())
    assert flow.shape == (n, 2, h, w) and flow.dtype == torch.float32
    _hold_rounded("SpyNet " + _gid(geom), "bf16", dict(flow=flow), dict(flow=want), dict(flow=yard))


# =============================================================================================================================
# Result_Model: block, tail, weight gradient, un-shuffle
# =============================================================================================================================
BLOCK_NAMES = ["y", "bits", "dx", "gw", "gb", "gw_dense", "gb_dense"]
TAIL_NAMES = ["out", "dconv", "dfeat", "gw", "gb"]


def _run_block(case, dtype, wgs=0, bits=None):
    """rm_block_fwd, then rm_block_bwd_data, rm_wgrad on the dense embedding and rm_block_wgrad with the forward's own mask (bits:
    with these mask words instead).  NCHW on the host."""
    from mobilesuperresolution_amd import hotpath as HP
    dt = DTYPES[dtype]
    f, IN, a, k = case["F"], case["IN"], case["a"], case["k"]
    n, _, h, w = case["x"].shape
    xin, dy = _nhwc(case["x"], dt), _nhwc(case["gy"], dt)
    wt, b = case["w"].cuda(), case["b"].cuda()
    y = torch.full_like(xin, float("nan"))
    m = torch.full((n, h, w), SENTINEL, dtype=torch.int32, device="cuda")
    HP.rm_block_fwd(xin, y, m, HP.rm_pack_block(wt, f, IN, dt), HP.rm_bias32(b, IN), k)
    mk = m
    if bits is not None:
        mk = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).cuda()
    dx = torch.full_like(dy, float("nan"))
    HP.rm_block_bwd_data(dy, mk, dx, HP.rm_pack_block(wt, f, IN, dt, transposed=True), k)
    gwd, gbd = HP.rm_wgrad(dy, mk, xin, f, f, k, wgs)
    gw, gb = HP.rm_block_wgrad(dy, mk, xin, IN, IN - a, k, wgs)
    torch.cuda.synchronize()
    return dict(y=_nchw(y), bits=m.cpu().long() & 0xFFFFFFFF, dx=_nchw(dx), gw=gw, gb=gb, gw_dense=gwd, gb_dense=gbd)


def _run_tail(case, dtype):
    """rm_tail_fwd onto the base, rm_unshuffle, rm_tail_bwd_data and rm_wgrad(mask=None, CA = rm_cp(R)) as _ResultNet chains them"""
    from mobilesuperresolution_amd import hotpath as HP, packing as P
    dt = DTYPES[dtype]
    f, r_, k = case["F"], case["R"], case["k"]
    co, cp = 3 * r_ * r_, P.rm_cp(r_)
    feat, wt = _nhwc(case["feat"], dt), case["w"].cuda()
    out = case["base"].cuda().clone()
    HP.rm_tail_fwd(feat, out, HP.rm_pack(wt, dt), r_, k)
    dconv = HP.rm_unshuffle(case["dout"].cuda(), r_, dt)
    wtt = wt.new_zeros((f, cp, k, k))
    wtt[:, :co] = wt.transpose(0, 1).flip(2, 3)
    dfeat = torch.full_like(feat, float("nan"))
    HP.rm_tail_bwd_data(dconv, dfeat, HP.rm_pack(wtt, dt), r_, k)
    gw, gb = HP.rm_wgrad(dconv, None, feat, co, f, k)
    torch.cuda.synchronize()
    return dict(out=out, dconv=_nchw(dconv), dfeat=_nchw(dfeat), gw=gw, gb=gb)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k", R.RM_KS)
@pytest.mark.parametrize("geom", R.RM_GEOMETRIES, ids=_gid)
def test_block_exact_geometries(geom, k, dtype):
    """y, the mask words, the pass-through and padded channels, dx, and the weight and bias gradient by both routes, bit for bit:
    images inside the halo, one tile under / exact / one-pixel slivers of the conv tile (32 x 16 bf16, 32 x 8 fp32) and of the
    16 x 16 weight-gradient tile, several tiles in both directions, a batch of 2"""
    for window in R.RM_SWEEP_WINDOWS:
        case = R.block_exact_case(*window, k, *geom)
        _hold_exact((window, k, geom, dtype), _run_block(case, dtype), case["ref"], BLOCK_NAMES)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k", R.RM_KS)
def test_block_exact_windows(k, dtype):
    """the whole row, a window at the front, in the middle, a narrow one at the end of a full 32-channel row, an odd width"""
    for window in R.RM_WINDOWS:
        for geom in R.RM_WINDOW_GEOMETRIES:
            case = R.block_exact_case(*window, k, *geom)
            _hold_exact((window, k, geom, dtype), _run_block(case, dtype), case["ref"], BLOCK_NAMES)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k", R.RM_TAIL_KS)
@pytest.mark.parametrize("r_", R.RM_TAIL_RS)
def test_tail_exact(r_, k, dtype):
    """the k x k tail added onto a non-zero base (R = 3: 27 channels, a partial group of four), the un-shuffled cotangent with its
    padded channels, the feature gradient, and the weight and bias gradient against the un-shuffled cotangent"""
    for f in R.RM_TAIL_FS:
        for geom in R.RM_TAIL_GEOMETRIES:
            case = R.tail_exact_case(f, r_, k, *geom)
            _hold_exact((f, r_, k, geom, dtype), _run_tail(case, dtype), case["ref"], TAIL_NAMES)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k", R.RM_LOOP_KS)
def test_wgrad_tile_loop_workgroup_counts(k, dtype):
    """6 tiles under 1, 2, 5, 6, 7 and 256 workgroups: six trips, three, uneven trips, one trip each, idle workgroups; the slabs of
    every count sum to the reference, bit for bit"""
    assert R.wgrad_tiles(*R.RM_LOOP_GEOMETRY) == 6
    case = R.block_exact_case(*R.RM_LOOP_WINDOW, k, *R.RM_LOOP_GEOMETRY)
    for wgs in R.RM_LOOP_WGS:
        _hold_exact((k, dtype, "wgs", wgs), _run_block(case, dtype, wgs), case["ref"], BLOCK_NAMES)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k", R.RM_LOOP_KS)
def test_wgrad_tile_loop_many_tiles(k, dtype):
    """30 tiles over 4 workgroups: seven or eight trips each"""
    geom, wgs = R.RM_MANY_TILES
    assert R.wgrad_tiles(*geom) == 30
    case = R.block_exact_case(*R.RM_LOOP_WINDOW, k, *geom)
    _hold_exact((k, dtype, geom, wgs), _run_block(case, dtype, wgs), case["ref"], BLOCK_NAMES)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k", R.RM_KS)
def test_block_rounded(k, dtype):
    """the backward kernels are handed the float64 reference's mask, so a sign flip of a near-zero z does not enter dx and gw"""
    key = (24, 20, 12, k) + R.RM_ROUNDED_GEOMETRY
    case, ref, yard = R.rounded_reference("block", dtype, *key)
    _hold_rounded(f"block {dtype} k{k}", dtype, _run_block(case, dtype, 0, ref["bits"]), ref, yard)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k", R.RM_TAIL_KS)
def test_tail_rounded(k, dtype):
    key = (32, 3, k) + R.RM_ROUNDED_GEOMETRY
    case, ref, yard = R.rounded_reference("tail", dtype, *key)
    _hold_rounded(f"tail {dtype} k{k}", dtype, _run_tail(case, dtype), ref, yard)
