"""Block parity: the WDSR residual-block kernels (csrc/wdsr_block.h, wdsr_fwd_rs.h, wdsr_fwd_stream.h, wdsr_bwd_rs.h,
wdsr_bwd_pair_lds.h, wdsr_wgrad_rs.h) through their per-kernel entries of the C ABI and of hotpath.py -- sr_wdsr_block_fwd,
sr_wdsr_fwd_rs (one and two blocks; tile, persistent, pipeline and streaming forms), sr_wdsr_block2_fwd, sr_wdsr_block_bwd_data,
sr_wdsr_block2_bwd_data, sr_wdsr_block_wgrad and sr_wdsr_block_wgrad_saved -- against tests/block_ref.py (plain torch, float64,
CPU).  Output buffers are pre-filled with NaN, so an unwritten element shows; gradients are compared after the gather with
tables()["grad"], and the two constant slots must be zero.

  exact cases    dyadic data on which the kernels must return the reference bit for bit whatever their summation order, the stored
                 y / dx being the exact value rounded once to the hot dtype (conditions: tests/block_ref.py, verified on the host
                 by tests/test_block_ref_host.py)
  rounded cases  random normal data; per tensor, max |got - ref| / max |ref| within 8 x (fp32, + 1e-6) or 4 x (bf16) the same
                 metric of block_ref.emulate(); the ratio to that yardstick is printed for every tensor and DESIGN.md keeps the table
"""
import pytest
import torch

from tests import block_ref as R
from tests.parity_kit import hold_exact, hold_rounded

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
BF = torch.bfloat16
_gid = lambda g: "%dx%dx%d" % g
NAN = float("nan")
LAYER_BLOCKS = "aba"                                        # which block of the chain a layer of a multi-layer call is


def _nan_like(t, dtype=None):
    return torch.full_like(t, NAN, dtype=dtype or t.dtype)


class Dev:
    """one chain on the device in one dtype: packed weights of both blocks and, per block, the inputs of its entries (NHWC)"""

    def __init__(self, f, pa, pb, dtype, tensors):
        from mobilesuperresolution_amd import hotpath as HP
        self.f, self.dtype = f, dtype
        self.l, self.lp = R.DIMS[f][2], R.lp_of(f)
        src = torch.stack([R.block_vec(pa), R.block_vec(pb)]).cuda()
        args = [torch.stack([pa[k], pb[k]]).cuda() for k in R.NAMES]
        assert torch.equal(src, HP.block_src(*args))
        self.tb = HP.tables(f, src.device)
        self.blob, self.cinit = HP.pack_blocks(src, f, dtype)
        self.t = {k: R.nhwc(v).cuda().to(dtype) for k, v in tensors.items()}
        self.n, self.h, self.w, _ = self.t["xa"].shape
        self.tiles = R.tiles_of(self.h, self.w)
        self.i = dict(a=0, b=1)

    def side(self, k=1):
        return torch.full((k, self.n, self.tiles, R.NPX, self.lp), NAN, device="cuda", dtype=BF)


def _exact_dev(case, dtype):
    ref = case["ref"]
    return Dev(case["F"], case["pa"], case["pb"], dtype, dict(xa=case["x"], xb=ref["a"]["y_st"], dyb=case["dyb"], dya=ref["b"]["dx_st"]))


def _stored(r, name, dtype):
    return R.nhwc(r[name + "_st"] if dtype == BF else r[name])


def _p(t):
    return t.data_ptr() if t is not None else None


def _fwd_rs(d, x, nblk, blk, save, want_a=True):
    """sr_wdsr_fwd_rs: (ya or None, yb, saved t images [nblk] or None); nblk = 1 runs block `blk`"""
    from mobilesuperresolution_amd import _lib as L
    ya = _nan_like(x) if (nblk == 2 and want_a) else None
    yb = _nan_like(x)
    ts = d.side(nblk) if save else None
    i0, i1 = (0, 1) if nblk == 2 else (d.i[blk], None)
    n, h, w, f = x.shape
    L.check(L.lib().sr_wdsr_fwd_rs(_p(x), _p(ya), _p(yb), _p(d.blob[i0]), _p(d.blob[i1]) if nblk == 2 else None, _p(d.cinit[i0]),
                                   _p(d.cinit[i1]) if nblk == 2 else None, _p(ts[0]) if save else None,
                                   _p(ts[1]) if save and nblk == 2 else None, nblk, n, h, w, f, 1, L.stream_ptr()), "sr_wdsr_fwd_rs")
    return ya, yb, ts


def _t_pairs(prefix, d, ts, t_ref):
    """the saved t image at every core pixel inside the image, L channels"""
    return [(prefix + "saved t", R.untile_image(ts.float().cpu(), d.h, d.w, d.l), t_ref)]


def _forward_pairs(case, d, ref=None, x=None, single=True, tag=""):
    """every forward route of the dtype of `d` on the chain: [(name, got, expected)]"""
    from mobilesuperresolution_amd import _lib as L, hotpath as HP
    ref = ref or case["ref"]
    x = d.t["xa"] if x is None else x
    dtype, pairs = d.dtype, []
    exp = {b: R.nhwc(ref[b]["y_st"] if dtype == BF else ref[b]["y"]) for b in "ab"}
    if single:
        for b, xin in (("a", x), ("b", d.t["xb"])):
            y = _nan_like(xin)
            HP.block_fwd(xin, y, d.blob[d.i[b]], d.cinit[d.i[b]])
            pairs.append((f"{tag}block_fwd {b} y", y, exp[b]))
    if dtype != BF:
        return pairs
    if single:
        for b, xin in (("a", x), ("b", d.t["xb"])):
            for save in (False, True):
                _, y, ts = _fwd_rs(d, xin, 1, b, save)
                pairs.append((f"{tag}fwd_rs 1 {b} save={save} y", y, exp[b]))
                if save:
                    pairs += _t_pairs(f"{tag}fwd_rs 1 {b} ", d, ts[0], ref[b]["t"])
    for save in (False, True):
        for want_a in (True, False):
            ya, yb, ts = _fwd_rs(d, x, 2, None, save, want_a)
            name = f"{tag}fwd_rs 2 save={save} ya={want_a} "
            pairs.append((name + "yb", yb, exp["b"]))
            if want_a:
                pairs.append((name + "ya", ya, exp["a"]))
            if save:
                pairs += _t_pairs(name + "a ", d, ts[0], ref["a"]["t"]) + _t_pairs(name + "b ", d, ts[1], ref["b"]["t"])
    if single:
        ya, yb = _nan_like(x), _nan_like(x)
        n, h, w, f = x.shape
        L.check(L.lib().sr_wdsr_block2_fwd(_p(x), _p(ya), _p(yb), _p(d.blob[0]), _p(d.blob[1]), _p(d.cinit[0]), _p(d.cinit[1]), None, None,
                                           n, h, w, f, 1, L.stream_ptr()), "sr_wdsr_block2_fwd")
        pairs += [(tag + "block2_fwd ya", ya, exp["a"]), (tag + "block2_fwd yb", yb, exp["b"])]
    torch.cuda.synchronize()
    return pairs


def _pair_bwd(d, save):
    from mobilesuperresolution_amd import _lib as L
    t = d.t
    dxb, dxa = _nan_like(t["xa"]), _nan_like(t["xa"])
    dts = d.side(2) if save else None
    L.check(L.lib().sr_wdsr_block2_bwd_data(_p(t["xa"]), _p(t["xb"]), _p(t["dyb"]), _p(dxb), _p(dxa), _p(d.blob[0]), _p(d.blob[1]),
                                            _p(d.cinit[0]), _p(d.cinit[1]), _p(dts[0]) if save else None, _p(dts[1]) if save else None,
                                            d.n, d.h, d.w, d.f, 1, L.stream_ptr()), "sr_wdsr_block2_bwd_data")
    return dxb, dxa, dts


def _backward_pairs(case, d):
    from mobilesuperresolution_amd import hotpath as HP
    ref, dtype, pairs = case["ref"], d.dtype, []
    for b in "ab":
        dx = _nan_like(d.t["x" + b])
        HP.block_bwd_data(d.t["x" + b], d.t["dy" + b], dx, d.blob[d.i[b]], d.cinit[d.i[b]])
        pairs.append((f"block_bwd_data {b} dx", dx, _stored(ref[b], "dx", dtype)))
    if dtype == BF:
        for save in (False, True):
            dxb, dxa, dts = _pair_bwd(d, save)
            pairs += [(f"block2_bwd_data save={save} dxb", dxb, _stored(ref["b"], "dx", dtype)),
                      (f"block2_bwd_data save={save} dxa", dxa, _stored(ref["a"], "dx", dtype))]
            if save:                                         # the whole image: zeros in channels L .. LP - 1 and outside the image
                pairs += [(f"block2_bwd_data saved dt {b}", dts[d.i[b]].float().cpu(), R.tile_image(ref[b]["dt"], d.lp)) for b in "ab"]
    torch.cuda.synchronize()
    return pairs


def _layered(d, key, layers, gap):
    """[layers] views of one NaN-filled buffer, `gap` elements between two layers' tensors: (buffer, stride in elements)"""
    srcs = [d.t[key + b] for b in LAYER_BLOCKS[:layers]]
    stride = srcs[0].numel() + gap
    buf = torch.full((layers, stride), NAN, device="cuda", dtype=srcs[0].dtype)
    for i, s in enumerate(srcs):
        buf[i, :s.numel()] = s.reshape(-1)
    return buf, stride


def _wgrad(d, layers, wgs, saved=None, gap=40):
    """sr_wdsr_block_wgrad / sr_wdsr_block_wgrad_saved through the ABI on NaN-filled [layers][wgs][slab] partials, layer strides
    larger than the tensors with NaN in the gaps: (partial_a, partial_b).  saved: (t images [2], dt images [2]) by block."""
    from mobilesuperresolution_amd import _lib as L
    idx = [d.i[b] for b in LAYER_BLOCKS[:layers]]
    xs, x_ls = _layered(d, "x", layers, gap)
    dys, dy_ls = _layered(d, "dy", layers, gap)
    w_ls, c_ls = d.blob.shape[1] + 8 * gap, d.cinit.shape[1] + gap
    blob = torch.full((layers, w_ls), NAN, device="cuda", dtype=d.dtype)
    cin = torch.full((layers, c_ls), NAN, device="cuda")
    for i, k in enumerate(idx):
        blob[i, :d.blob.shape[1]], cin[i, :d.cinit.shape[1]] = d.blob[k], d.cinit[k]
    pa = torch.full((layers, wgs, d.tb["slab_a"]), NAN, device="cuda")
    pb = torch.full((layers, wgs, d.tb["slab_b"]), NAN, device="cuda")
    code = L.DTYPE_CODE[d.dtype]
    if saved is None:
        L.check(L.lib().sr_wdsr_block_wgrad(_p(xs), _p(dys), _p(blob), _p(cin), _p(pa), _p(pb), layers, wgs, d.n, d.h, d.w, d.f, code,
                                            x_ls, dy_ls, w_ls, c_ls, L.stream_ptr()), "sr_wdsr_block_wgrad")
    else:
        side_ls = saved[0][0].numel() + 8 * gap
        tsv = torch.full((layers, side_ls), NAN, device="cuda", dtype=BF)
        dtv = torch.full((layers, side_ls), NAN, device="cuda", dtype=BF)
        for i, k in enumerate(idx):
            tsv[i, :saved[0][k].numel()], dtv[i, :saved[1][k].numel()] = saved[0][k].reshape(-1), saved[1][k].reshape(-1)
        L.check(L.lib().sr_wdsr_block_wgrad_saved(_p(xs), _p(dys), _p(tsv), _p(dtv), _p(blob), _p(cin), _p(pa), _p(pb), layers, wgs, d.n, d.h,
                                                  d.w, d.f, code, x_ls, dy_ls, side_ls, w_ls, c_ls, L.stream_ptr()), "sr_wdsr_block_wgrad_saved")
    torch.cuda.synchronize()
    return pa, pb


def _grad_pairs(prefix, vec, r, f):
    s = R.split_vec(vec.cpu(), f)
    return [(prefix + k, s[k], r[k]) for k in R.GRADS] + [(prefix + "const", s["const"], torch.zeros(2))]


def _slab_pairs(prefix, case, d, pa, pb, work_a, work_b):
    """the partial slabs of a raw call: after the gather the columns of every row are finite, exactly 0 in the rows (workgroups)
    beyond work_a / work_b units of work, and the sums over the rows are the reference's gradients, layer by layer"""
    g = d.tb["grad"]
    cols_a, cols_b = g[g < d.tb["slab_a"]], g[g >= d.tb["slab_a"]] - d.tb["slab_a"]
    ga, gb = pa.index_select(2, cols_a), pb.index_select(2, cols_b)
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gb).all()), prefix + "a gathered column of a partial slab is not finite"
    pairs = []
    if pa.shape[1] > work_a:
        pairs.append((prefix + "idle slabs a", ga[:, work_a:], torch.zeros_like(ga[:, work_a:])))
    if pb.shape[1] > work_b:
        pairs.append((prefix + "idle slabs b", gb[:, work_b:], torch.zeros_like(gb[:, work_b:])))
    vec = torch.cat([pa.sum(1), pb.sum(1)], dim=1).index_select(1, g)
    for i in range(pa.shape[0]):
        blk = LAYER_BLOCKS[i]
        s = R.split_vec(torch.cat([vec[i].cpu(), torch.zeros(2)]), d.f)      # (the raw slabs have no constant slots: nothing to compare there)
        pairs += [(f"{prefix}layer {i} (block {blk}) {k}", s[k], case["ref"][blk][k]) for k in R.GRADS]
    return pairs


def _side_images(case, d):
    """the side images a training step hands to sr_wdsr_block_wgrad_saved, written by the kernels themselves onto NaN-filled
    buffers (t: sr_wdsr_fwd_rs with two blocks; dt: sr_wdsr_block2_bwd_data), and the reference's images with NaN wherever the
    producers wrote nothing"""
    ref = case["ref"]
    _, _, ts = _fwd_rs(d, d.t["xa"], 2, None, True)
    _, _, dts = _pair_bwd(d, True)
    torch.cuda.synchronize()
    rts = torch.stack([R.tile_image(ref[b]["t"], d.lp, ones_at=d.l) for b in "ab"]).cuda().to(BF)
    rdts = torch.stack([R.tile_image(ref[b]["dt"], d.lp) for b in "ab"]).cuda().to(BF)
    nan = torch.full_like(rts, NAN)
    return (ts, dts), (torch.where(torch.isnan(ts), nan, rts), torch.where(torch.isnan(dts), nan, rdts))


def _wgrad_pairs(case, d, wgs, layers_list=(1, 3)):
    """every weight-gradient route of the dtype of `d`"""
    from mobilesuperresolution_amd import hotpath as HP
    tiles, chunks = R.n_tiles(d.n, d.h, d.w), R.n_chunks(d.n, d.h, d.w)
    pairs = []
    for layers in layers_list:
        pa, pb = _wgrad(d, layers, wgs or 16)
        pairs += _slab_pairs(f"wgrad layers={layers} ", case, d, pa, pb, tiles, tiles)
    if wgs is None:
        xs, dys = torch.stack([d.t["xa"], d.t["xb"]]), torch.stack([d.t["dya"], d.t["dyb"]])
        vec = HP.block_wgrad(xs, dys, d.blob, d.cinit)
        for i, b in enumerate("ab"):
            pairs += _grad_pairs(f"hotpath.block_wgrad {b} ", vec[i], case["ref"][b], d.f)
    if d.dtype == BF:
        own, fed = _side_images(case, d)
        work_a = chunks if d.f == 24 else tiles
        for name, imgs in (("own images ", own), ("reference images ", fed)):
            for layers in layers_list:
                pa, pb = _wgrad(d, layers, wgs or 16, saved=imgs)
                pairs += _slab_pairs(f"wgrad_saved {name}layers={layers} ", case, d, pa, pb, work_a, tiles)
    torch.cuda.synchronize()
    return pairs


# =============================================================================================================================
# exact cases: geometries
# =============================================================================================================================
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_gid)
def test_forward_exact(geom, f, mode):
    """images inside the halos (1 pixel; 2 in the two-block kernels), one tile under / exact / one-pixel slivers of the 12 x 24
    tile, 3 x 3 tiles with an interior one, a batch of 3: sr_wdsr_block_fwd in both dtypes, sr_wdsr_fwd_rs with one and two
    blocks, with and without the saved t images and ya, sr_wdsr_block2_fwd (24 units: eight waves; 32: wdsr_fwd_rs16_kernel)"""
    case = R.exact_case(f, *geom)
    hold_exact((geom, f, mode), _forward_pairs(case, _exact_dev(case, DTYPES[mode])))


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_gid)
def test_backward_data_exact(geom, f, mode):
    """sr_wdsr_block_bwd_data in both dtypes and sr_wdsr_block2_bwd_data (24 units: wdsr_bwd_rs_kernel, 32: wdsr_bwd_pair_lds_kernel)
    with and without the saved dt images, which equal the reference's everywhere"""
    case = R.exact_case(f, *geom)
    hold_exact((geom, f, mode), _backward_pairs(case, _exact_dev(case, DTYPES[mode])))


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_gid)
def test_weight_gradients_exact(geom, f, mode):
    """sr_wdsr_block_wgrad (both roles, both dtypes) and sr_wdsr_block_wgrad_saved (24 units: a8 + b8; 32: saved kernel + b8), one and
    three layers with NaN between the layers' tensors; the saved route once on the images the kernels wrote themselves and once
    on the reference's"""
    case = R.exact_case(f, *geom)
    hold_exact((geom, f, mode), _wgrad_pairs(case, _exact_dev(case, DTYPES[mode]), 16))


@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("store,geom", R.STORE_CASES, ids=lambda v: _gid(v) if isinstance(v, tuple) else ("", "ya", "dxb")[v])
def test_stores_between_the_blocks_are_rounded_exact(store, geom, f):
    """the families in which ya (block a's larger 3x3 weights) resp. dxb (block b's larger W1 columns) pass 2^8 quanta and lie on
    bf16 ties: a pair kernel that handed the next block the unrounded value would differ.  Every route, both dtypes (the fp32
    single-block entries get the rounded tensor as their input)"""
    case = R.exact_case(f, *geom, 0, 0.5, store)
    assert case["ref"]["ties_of"]["ya" if store == R.STORE_YA else "dxb"] > 0
    for mode, dtype in DTYPES.items():
        d = _exact_dev(case, dtype)
        hold_exact((store, geom, f, mode), _forward_pairs(case, d) + _backward_pairs(case, d) + _wgrad_pairs(case, d, 16, layers_list=(3,)))


# =============================================================================================================================
# tap-identity sets
# =============================================================================================================================
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
def test_tap_identity(f, mode):
    """one 3x3 weight per output channel: y - x - b3 is a shifted copy of one t channel.  The sets cover all 9 L taps; both 3x3
    forms (the tap-major one of sr_wdsr_block_fwd and the dense-K one of sr_wdsr_fwd_rs)"""
    from mobilesuperresolution_amd import hotpath as HP
    bad, dtype = [], DTYPES[mode]
    for j, case in enumerate(R.tap_cases(f, *R.TAP_GEOMETRY)):
        d = Dev(f, case["p"], case["p"], dtype, dict(xa=case["x"]))
        exp = R.nhwc(case["ref"]["y_bf16"] if dtype == BF else case["ref"]["y"]).to(dtype)
        y = _nan_like(d.t["xa"])
        HP.block_fwd(d.t["xa"], y, d.blob[0], d.cinit[0])
        outs = [("block_fwd", y)]
        if dtype == BF:
            outs.append(("fwd_rs", _fwd_rs(d, d.t["xa"], 1, "a", False)[1]))
        torch.cuda.synchronize()
        for route, got in outs:
            ne = (got.cpu() != exp) | (got.cpu() != got.cpu())
            for fo in ne.any(0).any(0).any(0).nonzero().flatten().tolist():
                l, ky, kx = case["taps"][fo]
                bad.append(f"{route} set {j} output channel {fo}: tap (ky {ky}, kx {kx}) of t channel {l}: {int(ne[..., fo].sum())} elements differ")
    assert not bad, ((f, mode), bad[:12], len(bad))


# =============================================================================================================================
# the weight-gradient loops
# =============================================================================================================================
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("wgs", R.TILE_LOOP_WGS, ids=lambda v: "wgs%s" % v)
def test_weight_gradient_loops_exact(wgs, f):
    """3 x 13x25: 12 tiles and 14 chunks of 256 saved pixels -- a chunk straddles the 288-pixel tiles, rolls from the last tile of
    one image into the next image, and the last chunk is half empty -- under 1, 5, 12, 13, 14, 15 workgroups per layer (one
    workgroup walking everything, uneven shares, one unit each, idle workgroups) and hotpath.block_wgrad's default"""
    geom = R.TILE_LOOP_GEOMETRY
    assert R.n_tiles(*geom) == 12 and R.n_chunks(*geom) == 14
    case = R.exact_case(f, *geom)
    for mode, dtype in DTYPES.items():
        hold_exact((wgs, f, mode), _wgrad_pairs(case, _exact_dev(case, dtype), wgs, layers_list=(3,)))


@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("wgs", R.MANY_TILES_WGS, ids=lambda v: "wgs%s" % v)
def test_more_tiles_than_workgroups_exact(wgs, f):
    """260 tiles (293 chunks) under 16 and 64 workgroups per layer; dy three quarters zero keeps the sums below 2^24 quanta"""
    assert R.n_tiles(*R.MANY_TILES) == 260
    case = R.exact_case(f, *R.MANY_TILES, 0, R.MANY_TILES_DENSITY)
    for mode, dtype in DTYPES.items():
        hold_exact((wgs, f, mode), _wgrad_pairs(case, _exact_dev(case, dtype), wgs, layers_list=(1,)))


# =============================================================================================================================
# the persistent, pipeline and streaming forms of sr_wdsr_fwd_rs (24 units)
# =============================================================================================================================
def _big_batch(n, h, w):
    """a large batch of R.DISTINCT_IMAGES distinct images in a non-periodic order: (case, device chain on the batch, reference)"""
    case = R.exact_case(24, R.DISTINCT_IMAGES, h, w)
    x, ref = R.replicate(case, R.batch_order(n, R.DISTINCT_IMAGES))
    return case, Dev(24, case["pa"], case["pb"], BF, dict(xa=x, xb=ref["a"]["y_st"])), ref


@pytest.mark.parametrize("geom", R.PERSIST_BATCHES, ids=_gid)
def test_persistent_and_pipeline_forward_exact(geom):
    """>= 768 tiles per launch, not a multiple of the 256 workgroups: one block with and without the saved t image
    (wdsr_fwd_rs_persist_kernel), two blocks without (wdsr_fwd_rs_pipe_kernel) and with (per-tile launch) -- every image of the
    batch against the float64 reference of its distinct image"""
    n, h, w = geom
    assert R.n_tiles(n, h, w) >= 768 and R.n_tiles(n, h, w) % 256 != 0 and not (w == 48 and h % 4 == 0)
    case, d, ref = _big_batch(n, h, w)
    hold_exact(geom, _forward_pairs(case, d, ref=ref, single=False) + _forward_single_rs(d, ref))


def _forward_single_rs(d, ref):
    pairs = []
    for b in "ab":
        for save in (False, True):
            _, y, ts = _fwd_rs(d, d.t["x" + b], 1, b, save)
            pairs.append((f"fwd_rs 1 {b} save={save} y", y, R.nhwc(ref[b]["y_st"])))
            if save:
                pairs += _t_pairs(f"fwd_rs 1 {b} ", d, ts[0], ref[b]["t"])
    torch.cuda.synchronize()
    return pairs


@pytest.mark.parametrize("geom", R.STREAM_BATCHES, ids=_gid)
def test_streaming_forward_exact(geom):
    """>= 256 whole images of width 48, H % 4 == 0, the last round of workgroups at least 70 % full: wdsr_fwd_stream12_kernel, one
    round of workgroups and two with the second ragged; with and without the saved t images, with and without ya"""
    n, h, w = geom
    rounds = (n + 255) // 256
    assert w == 48 and h % 4 == 0 and h >= 8 and n >= 256 and n * 10 >= rounds * 256 * 7
    case, d, ref = _big_batch(n, h, w)
    hold_exact(geom, _forward_pairs(case, d, ref=ref, single=False))


# =============================================================================================================================
# documented refusals
# =============================================================================================================================
def test_unsupported_routes_write_nothing():
    """fp32 on the bf16-only entries and nblk = 3 return -1, an unsupported width -1, a missing pointer -2: NaN-filled outputs stay NaN"""
    from mobilesuperresolution_amd import _lib as L
    lib, sp = L.lib(), L.stream_ptr()
    case = R.exact_case(24, 1, 12, 24)
    for mode, dtype in DTYPES.items():
        d = _exact_dev(case, dtype)
        code, t = L.DTYPE_CODE[dtype], d.t
        x, bl, ci = t["xa"], d.blob, d.cinit
        fresh = lambda: (_nan_like(x), _nan_like(x), d.side(2).to(dtype), torch.full((2, 4, d.tb["slab_a"]), NAN, device="cuda"),
                         torch.full((2, 4, d.tb["slab_b"]), NAN, device="cuda"))

        def fwd(b, nblk=2, f=24, xin=x):
            return lib.sr_wdsr_fwd_rs(_p(xin), _p(b[0]), _p(b[1]), _p(bl[0]), _p(bl[1]), _p(ci[0]), _p(ci[1]), _p(b[2][0]), _p(b[2][1]), nblk, 1, 12, 24,
                                      f, code, sp)

        def fwd2(b, f=24):
            return lib.sr_wdsr_block2_fwd(_p(x), _p(b[0]), _p(b[1]), _p(bl[0]), _p(bl[1]), _p(ci[0]), _p(ci[1]), _p(b[2][0]), _p(b[2][1]), 1, 12, 24, f,
                                          code, sp)

        def bwd2(b, f=24):
            return lib.sr_wdsr_block2_bwd_data(_p(x), _p(t["xb"]), _p(t["dyb"]), _p(b[0]), _p(b[1]), _p(bl[0]), _p(bl[1]), _p(ci[0]), _p(ci[1]),
                                               _p(b[2][0]), _p(b[2][1]), 1, 12, 24, f, code, sp)

        def saved(b, f=24):
            n_ = x.numel()
            return lib.sr_wdsr_block_wgrad_saved(_p(x), _p(t["dya"]), _p(b[2][0]), _p(b[2][1]), _p(bl), _p(ci), _p(b[3]), _p(b[4]), 1, 4, 1, 12, 24, f,
                                                 code, n_, n_, b[2][0].numel(), bl.shape[1], ci.shape[1], sp)

        def single(b, f):
            return lib.sr_wdsr_block_fwd(_p(x), _p(b[0]), _p(bl[0]), _p(ci[0]), 1, 12, 24, f, code, sp)

        def single_bwd(b, f):
            return lib.sr_wdsr_block_bwd_data(_p(x), _p(t["dya"]), _p(b[0]), _p(bl[0]), _p(ci[0]), 1, 12, 24, f, code, sp)

        def wgrad(b, f):
            n_ = x.numel()
            return lib.sr_wdsr_block_wgrad(_p(x), _p(t["dya"]), _p(bl), _p(ci), _p(b[3]), _p(b[4]), 1, 4, 1, 12, 24, f, code, n_, n_, bl.shape[1],
                                           ci.shape[1], sp)

        refused = [(lambda b: fwd(b, nblk=3), -1), (lambda b: fwd(b, f=16), -1), (lambda b: fwd2(b, f=48), -1), (lambda b: bwd2(b, f=16), -1),
                   (lambda b: saved(b, f=40), -1), (lambda b: single(b, 16), -1), (lambda b: single_bwd(b, 48), -1), (lambda b: wgrad(b, 8), -1),
                   (lambda b: fwd(b, xin=None), -2)]
        if dtype == torch.float32:
            refused += [(fwd, -1), (fwd2, -1), (bwd2, -1), (saved, -1)]
        for call, rc in refused:
            bufs = fresh()
            assert call(bufs) == rc
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(b.float()).all()) for b in bufs)


# =============================================================================================================================
# rounded cases
# =============================================================================================================================
def _hold_rounded(tag, mode, got, ref, yard):
    """got: name -> (run, key, tensor) of block_ref._runs"""
    hold_rounded("block parity", tag, mode, [(f"{mode} | {name} | {run} {key}", g.float(), ref[run][key], yard[run][key])
                                             for name, (run, key, g) in got.items()])


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("geom", R.ROUNDED_GEOMETRIES, ids=_gid)
def test_rounded(geom, f, mode):
    """random normal data, nothing rounded beforehand: every route above once.  Runs (block_ref._runs): a and b are the two blocks
    on independent inputs; b2 is block b behind a in the two-block forward, a2 block a behind b in the two-block backward"""
    from mobilesuperresolution_amd import _lib as L, hotpath as HP
    dtype = DTYPES[mode]
    case, emu, ref, yard = R.rounded_reference(f, *geom, mode)
    d = Dev(f, case["pa"], case["pb"], dtype, dict(xa=case["x"], xb=case["xb"], dya=case["dya"], dyb=case["dyb"]))
    nc = lambda t: R.nchw(t.float().cpu())
    got = {}
    for b in "ab":
        xin, dy, k = d.t["x" + b], d.t["dy" + b], d.i[b]
        y, dx = _nan_like(xin), _nan_like(xin)
        HP.block_fwd(xin, y, d.blob[k], d.cinit[k])
        HP.block_bwd_data(xin, dy, dx, d.blob[k], d.cinit[k])
        got[f"block_fwd {b}"], got[f"block_bwd_data {b}"] = (b, "y_st", nc(y)), (b, "dx_st", nc(dx))
        if dtype == BF:
            _, y1, ts = _fwd_rs(d, xin, 1, b, True)
            got[f"fwd_rs 1 {b}"] = (b, "y_st", nc(y1))
            got[f"fwd_rs 1 {b} saved t"] = (b, "t", R.untile_image(ts[0].float().cpu(), d.h, d.w, d.l))
    xs, dys = torch.stack([d.t["xa"], d.t["xb"]]), torch.stack([d.t["dya"], d.t["dyb"]])
    vec = HP.block_wgrad(xs, dys, d.blob, d.cinit)
    for i, b in enumerate("ab"):
        s = R.split_vec(vec[i].cpu(), f)
        assert bool((s["const"] == 0).all())
        got.update({f"wgrad {b} {k}": (b, k, s[k]) for k in R.GRADS})
    pa, pb = _wgrad(d, 2, 16, gap=0)                        # the recompute route through the raw ABI (layers a, b)
    vraw = torch.cat([pa.sum(1), pb.sum(1)], dim=1).index_select(1, d.tb["grad"])
    for i, b in enumerate("ab"):
        s = R.split_vec(torch.cat([vraw[i].cpu(), torch.zeros(2)]), f)
        got.update({f"raw wgrad {b} {k}": (b, k, s[k]) for k in R.GRADS})
    if dtype == BF:
        ya, yb, ts = _fwd_rs(d, d.t["xa"], 2, None, True)
        got["fwd_rs 2 ya"], got["fwd_rs 2 yb"] = ("a", "y_st", nc(ya)), ("b2", "y_st", nc(yb))
        got["fwd_rs 2 saved t a"] = ("a", "t", R.untile_image(ts[0].float().cpu(), d.h, d.w, d.l))
        got["fwd_rs 2 saved t b"] = ("b2", "t", R.untile_image(ts[1].float().cpu(), d.h, d.w, d.l))
        ya, yb, _ = _fwd_rs(d, d.t["xa"], 2, None, False)
        got["fwd_rs 2 no t ya"], got["fwd_rs 2 no t yb"] = ("a", "y_st", nc(ya)), ("b2", "y_st", nc(yb))
        ya, yb = _nan_like(d.t["xa"]), _nan_like(d.t["xa"])
        L.check(L.lib().sr_wdsr_block2_fwd(_p(d.t["xa"]), _p(ya), _p(yb), _p(d.blob[0]), _p(d.blob[1]), _p(d.cinit[0]), _p(d.cinit[1]), None, None,
                                           d.n, d.h, d.w, f, 1, L.stream_ptr()), "sr_wdsr_block2_fwd")
        got["block2_fwd ya"], got["block2_fwd yb"] = ("a", "y_st", nc(ya)), ("b2", "y_st", nc(yb))
        dxb, dxa, _ = _pair_bwd(d, False)
        got["block2_bwd_data no dt dxb"], got["block2_bwd_data no dt dxa"] = ("b", "dx_st", nc(dxb)), ("a2", "dx_st", nc(dxa))
        dxb, dxa, dts = _pair_bwd(d, True)
        got["block2_bwd_data dxb"], got["block2_bwd_data dxa"] = ("b", "dx_st", nc(dxb)), ("a2", "dx_st", nc(dxa))
        got["block2_bwd_data saved dt b"] = ("b", "dt", R.untile_image(dts[1].float().cpu(), d.h, d.w, d.l))
        got["block2_bwd_data saved dt a"] = ("a2", "dt", R.untile_image(dts[0].float().cpu(), d.h, d.w, d.l))
        # the saved route on the images of independent blocks: t of fwd_rs with one block, dt of the pair backward's block b;
        # block a's dt image comes from a pair launch whose block b is a copy of a's inputs
        ts1 = torch.stack([_fwd_rs(d, d.t["x" + b], 1, b, True)[2][0] for b in "ab"])
        da = Dev(f, case["pa"], case["pa"], dtype, dict(xa=case["x"], xb=case["x"], dyb=case["dya"]))
        dt1 = torch.stack([_pair_bwd(da, True)[2][1], dts[1]])
        torch.cuda.synchronize()
        pa, pb = _wgrad(d, 2, 16, saved=(ts1, dt1), gap=0)
        vec2 = torch.cat([pa.sum(1), pb.sum(1)], dim=1).index_select(1, d.tb["grad"])
        for i, b in enumerate("ab"):
            s = R.split_vec(torch.cat([vec2[i].cpu(), torch.zeros(2)]), f)
            got.update({f"wgrad_saved {b} {k}": (b, k, s[k]) for k in R.GRADS})
    torch.cuda.synchronize()
    _hold_rounded((geom, f), mode, got, ref, yard)
