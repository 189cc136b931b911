"""Ends parity: the WDSR head and tail kernels (csrc/wdsr_ends.h) -- head conv, fused tail + skip + PixelShuffle + mean, the tail's
backward-data, weight-gradient and fused backward kernels, the loss fold, sr_tail_train and sr_head_wgrad -- driven through the
per-kernel entries of hotpath.py (head_fwd, tail_fwd, tail_bwd_data, tail_wgrad, tail_bwd, tail_bwd_loss, head_wgrad, with
pack_head / pack_tail) and through sr_tail_train of the C ABI, against tests/ends_ref.py (plain torch, float64, CPU).  Output
buffers are pre-filled with NaN, so an unwritten element shows; gradient vectors are compared after the gather (the slab columns
outside packing.ends_grad_tables are unused).

  exact cases    dyadic data on which the kernels must return the reference bit for bit whatever their summation order, the stored
                 y / dfeat being the exact value rounded once to the hot dtype (conditions: tests/ends_ref.py, verified on the host
                 by tests/test_ends_ref_host.py): images inside the halos, at the edges of the 12 x 24 tile, 3 x 3 tiles, a batch;
                 R = 2, 3, 4; F = 24, 32; tap-identity sets; the tile loops with 1 .. 256 workgroups for 12 tiles and the default
                 for 260; the loss fold with exact zeros of sr - hr and the core-only loss accounting
  rounded cases  random normal data; per tensor, max |got - ref| / max |ref| within 8 x (fp32, + 1e-6) or 4 x (bf16) the same
                 metric of ends_ref.emulate(); the ratio to that yardstick is printed for every tensor and DESIGN.md keeps the table
"""
import pytest
import torch

from tests import ends_ref as R
from tests.parity_kit import hold_exact, hold_rounded

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
_gid = lambda g: "%dx%dx%d" % g
NAN = float("nan")


def _grad_pairs(prefix, vec, ref, f, R_):
    s = R.split_tail_vec(vec.cpu(), f, R_)
    return [(prefix + k, s[k], ref[k]) for k in ("dwt", "dws", "dbtot")] + [(prefix + "const", s["const"], torch.zeros(2))]


def _stored(ref, name, dtype):
    return ref[name + "_bf16"] if dtype == torch.bfloat16 else ref[name]


def _tail_dev(case, dtype):
    from mobilesuperresolution_amd import hotpath as HP
    f, R_ = case["F"], case["R"]
    src = R.tail_vec(case["wt"], case["ws"], case["btot"]).cuda()
    assert torch.equal(src, HP.tail_src(case["wt"].cuda(), case["ws"].cuda(), case["btot"].cuda()))
    d = dict(blob=HP.pack_tail(src, f, R_, dtype), feat=case["feat"].cuda().to(dtype).contiguous(), x=case["x"].cuda().contiguous())
    for k in ("dout", "hr"):
        if k in case:
            d[k] = case[k].cuda().contiguous()
    return d


def _tail_fwd(case, d):
    from mobilesuperresolution_amd import hotpath as HP
    n, h, w, _ = case["feat"].shape
    out = torch.full((n, 3, case["R"] * h, case["R"] * w), NAN, device="cuda")
    HP.tail_fwd(d["feat"], d["x"], out, d["blob"], case["mean"], case["R"])
    return out


def _run_tail(case, dtype, wgs=None):
    """forward, backward-data, weight gradient and (bf16) the fused backward of one case: [(name, got, expected)]"""
    from mobilesuperresolution_amd import hotpath as HP
    f, R_, ref, mean = case["F"], case["R"], case["ref"], case["mean"]
    d = _tail_dev(case, dtype)
    kw = {} if wgs is None else dict(wgs=wgs)
    pairs = [("out", _tail_fwd(case, d), ref["out"])]
    dfeat = torch.full_like(d["feat"], NAN)
    HP.tail_bwd_data(d["dout"], dfeat, d["blob"], R_)
    pairs.append(("bwd_data dfeat", dfeat, _stored(ref, "dfeat", dtype)))
    pairs += _grad_pairs("wgrad ", HP.tail_wgrad(d["dout"], d["feat"], d["x"], mean, R_, **kw), ref, f, R_)
    if dtype == torch.bfloat16:
        dfeat2, vec = HP.tail_bwd(d["dout"], d["feat"], d["x"], d["blob"], mean, R_, **kw)
        pairs.append(("bwd dfeat", dfeat2, ref["dfeat_bf16"]))
        pairs += _grad_pairs("bwd ", vec, ref, f, R_)
    torch.cuda.synchronize()
    return pairs


def _head_dev(case, dtype):
    from mobilesuperresolution_amd import hotpath as HP
    src = R.head_vec(case["wh"], case["bh"]).cuda()
    assert torch.equal(src, HP.head_src(case["wh"].cuda(), case["bh"].cuda()))
    return dict(blob=HP.pack_head(src, case["F"], dtype), x=case["x"].cuda().contiguous(), dy0=case["dy0"].cuda().to(dtype).contiguous())


def _head_fwd(case, d, dtype):
    from mobilesuperresolution_amd import hotpath as HP
    n, _, h, w = case["x"].shape
    y = torch.full((n, h, w, case["F"]), NAN, dtype=dtype, device="cuda")
    HP.head_fwd(d["x"], y, d["blob"], case["mean"])
    return y


def _run_head(case, dtype, wgs=None):
    from mobilesuperresolution_amd import hotpath as HP
    f, ref = case["F"], case["ref"]
    d = _head_dev(case, dtype)
    pairs = [("y", _head_fwd(case, d, dtype), _stored(ref, "y", dtype))]
    s = R.split_head_vec(HP.head_wgrad(d["dy0"], d["x"], case["mean"], **({} if wgs is None else dict(wgs=wgs))).cpu(), f)
    torch.cuda.synchronize()
    return pairs + [("dwh", s["dwh"], ref["dwh"]), ("dbh", s["dbh"], ref["dbh"]), ("head const", s["const"], torch.zeros(2))]


# =============================================================================================================================
# exact cases: geometries, scales, units
# =============================================================================================================================
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_gid)
def test_tail_exact_geometries(geom, f, mode):
    """R = 4 (two row tiles of conv channels): images inside the 1-, 2- and 3-pixel halos, one tile under / exact / one-pixel
    slivers of the 12 x 24 tile, 3 x 3 tiles with an interior one, a batch of 3"""
    hold_exact((geom, f, mode), _run_tail(R.exact_tail_case(f, 4, *geom), DTYPES[mode]))


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("geom", R.SCALE_GEOMETRIES, ids=_gid)
def test_tail_exact_scales(geom, r, f, mode):
    """R = 2 (CO = 12 in 16 dconv channels) and R = 3 (CO = 27 in 32: five padded conv channels, scalar HR stores)"""
    hold_exact((geom, r, f, mode), _run_tail(R.exact_tail_case(f, r, *geom), DTYPES[mode]))


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_gid)
def test_head_exact_geometries(geom, f, mode):
    hold_exact((geom, f, mode), _run_head(R.exact_head_case(f, *geom), DTYPES[mode]))


# =============================================================================================================================
# tap-identity sets
# =============================================================================================================================
@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("r", [2, 3, 4])
def test_tail_tap_identity(r, f, mode):
    """one weight per conv channel: the output is a shifted, shuffled copy of one input plane plus the constant.  The sets cover
    all 9 F + 75 taps and, each, every conv channel c R R + i R + j (the padded channels CO .. COP - 1 must stay silent)."""
    bad = []
    for j, case in enumerate(R.tail_tap_cases(f, r, *R.TAP_GEOMETRY)):
        got = _tail_fwd(case, _tail_dev(case, DTYPES[mode])).cpu()
        exp = case["ref"]["out"].float()
        ne = R.unshuffle(((got != exp) | (got != got)).float(), r) > 0
        for ch in ne.any(0).any(1).any(1).nonzero().flatten().tolist():
            kind, ci, ky, kx = case["taps"][ch]
            c, i, jj = ch // (r * r), (ch % (r * r)) // r, ch % r
            bad.append(f"set {j} conv channel {ch} = colour {c} HR sub-pixel (i {i}, j {jj}): {kind} tap (ky {ky}, kx {kx}) of input "
                       f"channel {ci}: {int(ne[:, ch].sum())} elements differ")
    assert not bad, ((f, r, mode), bad[:12], len(bad))


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
def test_head_tap_identity(f, mode):
    from mobilesuperresolution_amd import hotpath as HP
    bad, dtype = [], DTYPES[mode]
    for j, case in enumerate(R.head_tap_cases(f, *R.TAP_GEOMETRY)):
        src = R.head_vec(case["wh"], case["bh"]).cuda()
        d = dict(blob=HP.pack_head(src, f, dtype), x=case["x"].cuda().contiguous())
        got = _head_fwd(case, d, dtype).cpu()
        exp = _stored(case["ref"], "y", dtype).to(dtype)
        ne = (got != exp) | (got != got)
        for fo in ne.any(0).any(0).any(0).nonzero().flatten().tolist():
            ci, ky, kx = case["taps"][fo]
            bad.append(f"set {j} output channel {fo}: tap (ky {ky}, kx {kx}) of colour {ci}: {int(ne[..., fo].sum())} elements differ")
    assert not bad, ((f, mode), bad)


# =============================================================================================================================
# the loss fold and the tile loops
# =============================================================================================================================
def _raw_bwd_loss(case, d, dtype, sr, wgs, train=False):
    """sr_tail_bwd_loss / sr_tail_train of the C ABI on NaN-filled buffers: (dfeat, slabs [wgs, .], loss_part [wgs])"""
    from mobilesuperresolution_amd import _lib as L, hotpath as HP
    n, h, w, f = case["feat"].shape
    tb = HP.ends_tables(f, case["R"], d["feat"].device)
    dfeat = torch.full_like(d["feat"], NAN)
    part = torch.full((wgs, tb["tail_slab"]), NAN, device="cuda")
    lpart = torch.full((wgs,), NAN, device="cuda")
    tail = (lpart.data_ptr(), d["feat"].data_ptr(), d["x"].data_ptr(), case["mean"], d["blob"].data_ptr(), dfeat.data_ptr(),
            part.data_ptr(), wgs, n, h, w, f, case["R"], L.DTYPE_CODE[dtype], L.stream_ptr())
    if train:
        L.check(L.lib().sr_tail_train(d["hr"].data_ptr(), case["loss_kind"], case["gscale"], *tail), "sr_tail_train")
    else:
        L.check(L.lib().sr_tail_bwd_loss(sr.data_ptr(), d["hr"].data_ptr(), case["loss_kind"], case["gscale"], *tail), "sr_tail_bwd_loss")
    torch.cuda.synchronize()
    return dfeat, part, lpart, tb


def _loss_pairs(prefix, case, dtype, dfeat, part, lpart, tb):
    """[(name, got, expected)] of a loss-fold call: dfeat, the gathered gradient vector, the loss sum; and every workgroup without
    a tile must have written exactly 0 to its slab and to its loss partial"""
    from mobilesuperresolution_amd import hotpath as HP
    ref, f, R_ = case["ref"], case["F"], case["R"]
    tiles, wgs = R.n_tiles(*case["feat"].shape[:3]), part.shape[0]
    pairs = [(prefix + "dfeat", dfeat, _stored(ref, "dfeat", dtype))]
    pairs += _grad_pairs(prefix, HP._tail_grad_vector(part, tb), ref, f, R_)
    pairs.append((prefix + "loss", lpart.double().sum().reshape(1).cpu(), ref["loss"].reshape(1)))
    if wgs > tiles:
        idle = part[tiles:].index_select(1, tb["tail_grad"])
        pairs.append((prefix + "idle slabs", idle, torch.zeros_like(idle)))
        pairs.append((prefix + "idle loss_part", lpart[tiles:], torch.zeros(wgs - tiles)))
    return pairs


def _run_loss(case, dtype, wgs=256, train=True):
    d = _tail_dev(case, dtype)
    sr = _tail_fwd(case, d)
    pairs = [("out", sr, case["ref"]["out"])]
    pairs += _loss_pairs("bwd_loss ", case, dtype, *_raw_bwd_loss(case, d, dtype, sr, wgs))
    if train and dtype == torch.bfloat16 and case["R"] == 4:
        pairs += _loss_pairs("train ", case, dtype, *_raw_bwd_loss(case, d, dtype, None, wgs, train=True))
    return pairs, d, sr


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("kind", [1, 2], ids=["l1", "charbonnier"])
@pytest.mark.parametrize("geom", R.LOSS_GEOMETRIES, ids=_gid)
def test_loss_fold_exact(geom, kind, f, mode):
    """hr = sr - d on the reference's sr, d in {+-1/2, +-1, +-2}, for L1 also d = 0 at >= 100 LR pixels inside tiles and >= 20 on
    their borders: dfeat and the weight gradients are the reference's for loss_ref's gradient, and the sum of loss_part is the
    float64 loss sum exactly (each HR pixel counted once, as a core pixel) -- sr_tail_bwd_loss (fp32: two launches; bf16: fused)
    through the ABI with NaN-filled buffers and through hotpath.tail_bwd_loss, and sr_tail_train (bf16)"""
    from mobilesuperresolution_amd import hotpath as HP
    dtype = DTYPES[mode]
    case = R.exact_tail_case(f, 4, *geom, 0, 0.5, kind)
    pairs, d, sr = _run_loss(case, dtype)
    dfeat, vec, lpart = HP.tail_bwd_loss(sr, d["hr"], kind, case["gscale"], d["feat"], d["x"], d["blob"], case["mean"], 4)
    pairs.append(("hotpath dfeat", dfeat, _stored(case["ref"], "dfeat", dtype)))
    pairs += _grad_pairs("hotpath ", vec, case["ref"], f, 4)
    pairs.append(("hotpath loss", lpart.double().sum().reshape(1).cpu(), case["ref"]["loss"].reshape(1)))
    hold_exact((geom, kind, f, mode), pairs)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("r", [2, 3])
def test_loss_fold_exact_scales(r, f, mode):
    for kind in (1, 2):
        case = R.exact_tail_case(f, r, *R.LOSS_GEOMETRIES[0], 0, 0.5, kind)
        hold_exact((r, kind, f, mode), _run_loss(case, DTYPES[mode])[0])


def _idle_pairs(prefix, part, used, tiles):
    """a workgroup without a tile must have written exactly 0 to the gathered columns of its (NaN-filled) slab"""
    if part.shape[0] <= tiles:
        return []
    idle = part[tiles:].index_select(1, used)
    return [(prefix + "idle slabs", idle, torch.zeros_like(idle))]


def _raw_slab_pairs(tcase, hcase, dtype, wgs_tail, wgs_bwd, wgs_head):
    """sr_tail_wgrad, sr_tail_bwd (bf16) and sr_head_wgrad of the C ABI on NaN-filled [wgs, slab] buffers: the gathered vectors
    against the reference, and the slabs of the idle workgroups"""
    from mobilesuperresolution_amd import _lib as L, hotpath as HP
    lib, code, sp = L.lib(), L.DTYPE_CODE[dtype], L.stream_ptr()
    f, ref, mean = tcase["F"], tcase["ref"], tcase["mean"]
    n, h, w, _ = tcase["feat"].shape
    tiles = R.n_tiles(n, h, w)
    d = _tail_dev(tcase, dtype)
    tb = HP.ends_tables(f, 4, d["feat"].device)
    part = torch.full((wgs_tail, tb["tail_slab"]), NAN, device="cuda")
    L.check(lib.sr_tail_wgrad(d["dout"].data_ptr(), d["feat"].data_ptr(), d["x"].data_ptr(), mean, part.data_ptr(), wgs_tail, n, h, w, f, 4,
                              code, sp), "sr_tail_wgrad")
    pairs = _grad_pairs("raw wgrad ", HP._tail_grad_vector(part, tb), ref, f, 4) + _idle_pairs("raw wgrad ", part, tb["tail_grad"], tiles)
    if dtype == torch.bfloat16:
        part2 = torch.full((wgs_bwd, tb["tail_slab"]), NAN, device="cuda")
        dfeat = torch.full_like(d["feat"], NAN)
        L.check(lib.sr_tail_bwd(d["dout"].data_ptr(), d["feat"].data_ptr(), d["x"].data_ptr(), mean, d["blob"].data_ptr(), dfeat.data_ptr(),
                                part2.data_ptr(), wgs_bwd, n, h, w, f, 4, code, sp), "sr_tail_bwd")
        pairs.append(("raw bwd dfeat", dfeat, ref["dfeat_bf16"]))
        pairs += _grad_pairs("raw bwd ", HP._tail_grad_vector(part2, tb), ref, f, 4) + _idle_pairs("raw bwd ", part2, tb["tail_grad"], tiles)
    hd = _head_dev(hcase, dtype)
    hpart = torch.full((wgs_head, tb["head_slab"]), NAN, device="cuda")
    L.check(lib.sr_head_wgrad(hd["dy0"].data_ptr(), hd["x"].data_ptr(), hcase["mean"], hpart.data_ptr(), wgs_head, n, h, w, f, code, sp),
            "sr_head_wgrad")
    torch.cuda.synchronize()
    s = R.split_head_vec(torch.cat([hpart.sum(0).index_select(0, tb["head_grad"]).cpu(), torch.zeros(2)]), f)
    pairs += [("raw dwh", s["dwh"], hcase["ref"]["dwh"]), ("raw dbh", s["dbh"], hcase["ref"]["dbh"])]
    return pairs + _idle_pairs("raw head ", hpart, tb["head_grad"], tiles)


@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("wgs", R.TILE_LOOP_WGS, ids=lambda v: "wgs%s" % v)
def test_tile_loops_exact(wgs, f):
    """12 tiles under 1, 5, 12, 13 and the default number of workgroups (one workgroup walking all tiles, an uneven share, one
    tile each, idle workgroups): tail_wgrad, tail_bwd, tail_bwd_loss of both kinds with loss_part, sr_tail_train and head_wgrad"""
    geom = R.TILE_LOOP_GEOMETRY
    for mode, dtype in DTYPES.items():
        hold_exact(("tail", wgs, f, mode), _run_tail(R.exact_tail_case(f, 4, *geom), dtype, wgs))
        hold_exact(("head", wgs, f, mode), _run_head(R.exact_head_case(f, *geom), dtype, wgs))
        hold_exact(("raw", wgs, f, mode), _raw_slab_pairs(R.exact_tail_case(f, 4, *geom), R.exact_head_case(f, *geom), dtype,
                                                          wgs or 64, wgs or 256, wgs or 64))
        for kind in (1, 2):
            case = R.exact_tail_case(f, 4, *geom, 0, 0.5, kind)
            hold_exact(("loss", kind, wgs, f, mode), _run_loss(case, dtype, 256 if wgs is None else wgs)[0])


@pytest.mark.parametrize("f", R.UNITS)
def test_more_tiles_than_workgroups_exact(f):
    """260 tiles: more than the 256 workgroups tail_bwd / sr_tail_train take by default and the 64 of tail_wgrad / head_wgrad"""
    assert R.n_tiles(*R.MANY_TILES) == 260
    tc = R.exact_tail_case(f, 4, *R.MANY_TILES, 0, R.MANY_TILES_DENSITY)
    hc = R.exact_head_case(f, *R.MANY_TILES, 0, R.MANY_TILES_DENSITY)
    for mode, dtype in DTYPES.items():
        hold_exact(("tail", f, mode), _run_tail(tc, dtype))
        hold_exact(("head", f, mode), _run_head(hc, dtype))
        hold_exact(("raw", f, mode), _raw_slab_pairs(tc, hc, dtype, 64, 256, 64))


@pytest.mark.parametrize("f", R.UNITS)
def test_more_tiles_than_workgroups_loss_exact(f):
    """the same 260 tiles through the loss fold with its default 256 workgroups (four of them walk two tiles): sr_tail_bwd_loss in
    both dtypes and sr_tail_train, L1 with exact zeros"""
    case = R.exact_tail_case(f, 4, *R.MANY_TILES, 0, 0.5, 1)
    for mode, dtype in DTYPES.items():
        hold_exact(("loss 260 tiles", f, mode), _run_loss(case, dtype)[0])


def test_unsupported_routes_return_minus_one():
    """sr_tail_bwd is bf16 only, sr_tail_train bf16 and R = 4 only: the documented -1, and nothing is written (NaN-filled buffers
    stay NaN)"""
    from mobilesuperresolution_amd import _lib as L, hotpath as HP
    case = R.exact_tail_case(24, 4, 1, 12, 24, 0, 0.5, 1)
    lib, wgs = L.lib(), 4
    for dtype in DTYPES.values():
        d = _tail_dev(case, dtype)
        sr = _tail_fwd(case, d)
        slab = max(HP.ends_tables(24, r, d["feat"].device)["tail_slab"] for r in (2, 3, 4))
        fresh = lambda: (torch.full_like(d["feat"], NAN), torch.full((wgs, slab), NAN, device="cuda"), torch.full((wgs,), NAN, device="cuda"))
        code = L.DTYPE_CODE[dtype]

        def bwd(bufs):
            return lib.sr_tail_bwd(sr.data_ptr(), d["feat"].data_ptr(), d["x"].data_ptr(), 0.5, d["blob"].data_ptr(), bufs[0].data_ptr(),
                                   bufs[1].data_ptr(), wgs, 1, 12, 24, 24, 4, code, L.stream_ptr())

        def train(bufs, r, lk):
            return lib.sr_tail_train(d["hr"].data_ptr(), lk, case["gscale"], bufs[2].data_ptr(), d["feat"].data_ptr(), d["x"].data_ptr(), 0.5,
                                     d["blob"].data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), wgs, 1, 12, 24, 24, r, code, L.stream_ptr())

        refused = [lambda b: train(b, 2, 1), lambda b: train(b, 3, 1), lambda b: train(b, 4, 3)]
        if dtype == torch.float32:
            refused += [bwd, lambda b: train(b, 4, 1)]
        else:
            bufs = fresh()
            assert bwd(bufs) == 0 and train(bufs, 4, 1) == 0
            torch.cuda.synchronize()
            assert not bool(torch.isnan(bufs[0].float()).any()) and not bool(torch.isnan(bufs[2]).any())
        for call in refused:
            bufs = fresh()
            assert call(bufs) == -1
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(b.float()).all()) for b in bufs)


# =============================================================================================================================
# rounded cases
# =============================================================================================================================
def _hold_rounded(tag, mode, got, ref, yard):
    """got: '<entry> <tensor>' -> tensor; the last word names the reference's tensor"""
    hold_rounded("ends parity", tag, mode, [(name, g, ref[name.split(" ")[-1]], yard[name.split(" ")[-1]]) for name, g in got.items()])


def _vec_tensors(prefix, vec, f, r):
    s = R.split_tail_vec(vec.cpu(), f, r)
    assert bool((s["const"] == 0).all())
    return {prefix + k: s[k] for k in ("dwt", "dws", "dbtot")}


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("geom", R.ROUNDED_GEOMETRIES, ids=_gid)
def test_tail_rounded(geom, f, mode):
    """random normal data, nothing rounded beforehand: out, dfeat and the weight gradients of every tail entry"""
    from mobilesuperresolution_amd import hotpath as HP
    dtype = DTYPES[mode]
    case = R.rounded_tail_case(f, 4, *geom)
    ref, yard = R.rounded_reference(case, mode)
    d = _tail_dev(case, dtype)
    got = {"out": _tail_fwd(case, d)}
    dfeat = torch.full_like(d["feat"], NAN)
    HP.tail_bwd_data(d["dout"], dfeat, d["blob"], 4)
    got["bwd_data dfeat"] = dfeat.float()
    got.update(_vec_tensors("wgrad ", HP.tail_wgrad(d["dout"], d["feat"], d["x"], case["mean"], 4), f, 4))
    if dtype == torch.bfloat16:
        dfeat2, vec = HP.tail_bwd(d["dout"], d["feat"], d["x"], d["blob"], case["mean"], 4)
        got["bwd dfeat"] = dfeat2.float()
        got.update(_vec_tensors("bwd ", vec, f, 4))
    _hold_rounded((geom, f), mode, got, ref, yard)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("kind", [1, 2], ids=["l1", "charbonnier"])
@pytest.mark.parametrize("geom", R.ROUNDED_GEOMETRIES, ids=_gid)
def test_loss_fold_rounded(geom, kind, f, mode):
    """the loss fold on random data, hr == sr at 2 % of the HR pixels (Charbonnier's d = 0 included).  sr is an INPUT of
    sr_tail_bwd_loss: the reference forms loss_ref's gradient from the same sr tensor (the tail's own output, whose parity
    test_tail_rounded holds), since a sign is not continuous in sr.  sr_tail_train forms sr itself; the exact cases hold its
    forward to the reference bit for bit, and here it must stay within the same bounds of the same reference."""
    dtype = DTYPES[mode]
    case = dict(R.rounded_tail_case(f, 4, *geom))
    d = _tail_dev(case, dtype)
    sr = _tail_fwd(case, d)
    hr = torch.where(case["hr_same"].cuda(), sr, sr + case["hr_noise"].cuda()).contiguous()
    assert int((hr == sr).sum()) >= 100
    d["hr"] = hr
    case.update(loss_kind=kind, gscale=0.7 / sr.numel())
    ref, yard = R.rounded_reference(case, mode, sr=sr.cpu(), hr=hr.cpu(), kind=kind, gscale=case["gscale"])
    got = {}
    for prefix, train in (("bwd_loss ", False), ("train ", True)):
        if train and dtype != torch.bfloat16:
            continue
        from mobilesuperresolution_amd import hotpath as HP
        dfeat, part, lpart, tb = _raw_bwd_loss(case, d, dtype, sr, 256, train)
        got[prefix + "dfeat"] = dfeat.float()
        got.update(_vec_tensors(prefix, HP._tail_grad_vector(part, tb), f, 4))
        got[prefix + "loss"] = lpart.double().sum().reshape(1)
    _hold_rounded((geom, kind, f), mode, got, ref, yard)


@pytest.mark.parametrize("mode", DTYPES)
@pytest.mark.parametrize("f", R.UNITS)
@pytest.mark.parametrize("geom", R.ROUNDED_GEOMETRIES, ids=_gid)
def test_head_rounded(geom, f, mode):
    from mobilesuperresolution_amd import hotpath as HP
    dtype = DTYPES[mode]
    case = R.rounded_head_case(f, *geom)
    ref, yard = R.rounded_reference(case, mode)
    d = _head_dev(case, dtype)
    s = R.split_head_vec(HP.head_wgrad(d["dy0"], d["x"], case["mean"]).cpu(), f)
    assert bool((s["const"] == 0).all())
    _hold_rounded((geom, f), mode, dict(y=_head_fwd(case, d, dtype).float(), dwh=s["dwh"], dbh=s["dbh"]), ref, yard)
