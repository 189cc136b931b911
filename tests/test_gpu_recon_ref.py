"""Reconstruction parity: the kernels of csrc/vsr_recon.h (vr_fusion_kernel, vr_upconv_kernel, vr_last_kernel; each alone through
BasicVSR_origin.reconstruct_hot(stages=...)) and of csrc/mv_recon.h (mv_recon_fwd_kernel in its four instantiations,
mv_recon_bwd_kernel, mv_recon_reduce_kernel; through the C ABI with weights packed by packing.mv_recon_tables) against
tests/recon_ref.py (plain torch, float64, CPU), element by element, fp32 and bf16.  Every buffer a kernel writes -- images, u_save,
state gradients, slabs, gradients, the output -- is pre-filled with NaN.

  exact cases     dyadic data on which the kernels must return the reference bit for bit (conditions: tests/recon_ref.py, verified
                  on the host by tests/test_recon_ref_host.py): the edges of the 16 x 16 tile (vsr_recon.h) and of the 8 x 16 / 4 x 16
                  tile (mv_recon.h), tap-identity sets, clips of 17 and 33 frames (two and three launches), the backward's tile walk
                  at workgroup counts below, at and above the number of items
  bounded cases   MotionVectorVSR sizes that are no power of two: u bit-exact, the output per element within the fp32 blend's
                  error (recon_ref.blend_bound)
  rounded cases   random normal data; per tensor within parity_kit.bound of the float32 / bf16 emulation's own distance
  refusals        a call the ABI refuses (-2) leaves its buffers untouched
"""
import ctypes

import pytest
import torch

from tests import recon_ref as R
from tests.parity_kit import hold_exact, hold_rounded

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")
_gid = lambda g: "x".join(str(v) for v in g)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _nhwc(t, dt, c):
    """(b, f, H, W) -> the kernels' (b, H, W, c) image in the hot dtype, channels >= f zero"""
    b, f, H, W = t.shape
    y = torch.zeros(b, H, W, c, dtype=dt, device="cuda")
    y[..., :f] = t.cuda().permute(0, 2, 3, 1)
    return y


def _nchw(img, f):
    return img[..., :f].permute(0, 3, 1, 2).float().cpu()


# ================================================================================================================================
# csrc/vsr_recon.h
# ================================================================================================================================
_MODELS = {}
_KEYS = {"fusion": "fusion", "up1": "upconv1", "up2": "upconv2", "last": "conv_last"}
_STAGE = {"fusion": 1, "up1": 2, "up2": 4, "last": 16}


def _vsr_model(f, mode, case):
    from mobilesuperresolution_amd.models.basicvsr_arch_origin import BasicVSR_origin
    if (f, mode) not in _MODELS:
        _MODELS[(f, mode)] = BasicVSR_origin(f, 1, hot_dtype=mode).cuda().eval()
    m = _MODELS[(f, mode)]
    layer = getattr(m, _KEYS[case["kind"]])
    with torch.no_grad():
        layer.weight.copy_(case["w"])
        layer.bias.copy_(case["b"])
    return m


def _run_conv(case, mode):
    """one kernel alone on NaN-filled scratch: (what it stored as (n, C, H, W) fp32 on the CPU, the padding channels, the rest of the
    output tensor)"""
    kind, f = case["kind"], case["f"]
    dt = DTYPES[mode]
    m = _vsr_model(f, mode, case)
    x = case["fb"] if kind == "fusion" else case["x"]
    n, _, H, W = x.shape
    h, w = {"fusion": (H, W), "up1": (H, W), "up2": (H // 2, W // 2), "last": (H // 4, W // 4)}[kind]
    cw = 24 if f <= 24 else 64
    hb, hf = torch.zeros(n, h, w, cw, dtype=dt, device="cuda"), torch.zeros(n, h, w, cw, dtype=dt, device="cuda")
    scratch = [_nan(n, h, w, 64, dtype=dt), _nan(n, 2 * h, 2 * w, 64, dtype=dt), _nan(n, 4 * h, 4 * w, 64, dtype=dt), _nan(n, 4 * h, 4 * w, 64, dtype=dt)]
    frame = case["frame"].cuda() if kind == "last" else torch.zeros(n, 3, h, w, device="cuda")
    big = _nan(n, 3, 3, 4 * h, 4 * w)
    if kind == "fusion":
        hb, hf = _nhwc(case["fb"], dt, cw), _nhwc(case["ff"], dt, cw)
    else:
        scratch[{"up1": 0, "up2": 1, "last": 3}[kind]] = _nhwc(case["x"], dt, 64)
    with torch.no_grad():
        m.reconstruct_hot(hb, hf, frame, big[:, 1], tuple(scratch), stages=_STAGE[kind])
    torch.cuda.synchronize()
    if kind == "last":
        assert _all_nan(big[:, 0]) and _all_nan(big[:, 2]), "conv_last wrote outside its slice"
        return big[:, 1].cpu(), None
    assert _all_nan(big), f"{kind} wrote the output tensor"
    img = scratch[{"fusion": 0, "up1": 1, "up2": 2}[kind]]
    co = 64 if kind == "up2" else f
    return _nchw(img, co), img[..., co:].float().cpu()


def _hold_conv(case, mode, tag):
    got, pad = _run_conv(case, mode)
    hold_exact(tag, [(case["kind"], got, R.conv_exact_ref(case, mode))])
    if pad is not None:
        assert not pad.ne(0).any() and not torch.isnan(pad).any(), (tag, "padding channels are not exactly zero")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", R.MV_WIDTHS)
@pytest.mark.parametrize("geom", R.VSR_GEOMETRIES, ids=_gid)
def test_fusion_exact(geom, f, mode):
    """[fb | ff]: every row reads one channel of each state, so the concat order, the cw + c - F mapping (F = 20, 24 on 24-channel
    states, 40, 64 on 64-channel ones) and the q * 8 < cw chunk test are all visible"""
    _hold_conv(R.conv_case("fusion", f, *geom), mode, ("fusion", f, geom, mode))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,f", [("up1", 24), ("up1", 64), ("up2", 24), ("up2", 64)])
@pytest.mark.parametrize("geom", R.VSR_GEOMETRIES, ids=_gid)
def test_upconv_exact(geom, kind, f, mode):
    """upconv1 at H x W, upconv2 at 2H x 2W (H, W = the geometry)"""
    n, h, w = geom
    k = 2 if kind == "up2" else 1
    _hold_conv(R.conv_case(kind, f, n, k * h, k * w), mode, (kind, f, geom, mode))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("geom", R.LAST_GEOMETRIES, ids=_gid)
def test_last_exact(geom, mode):
    n, h, w = geom
    _hold_conv(R.conv_case("last", 64, n, 4 * h, 4 * w), mode, ("last", geom, mode))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["up1", "up2"])
@pytest.mark.parametrize("s", range(9))
def test_upconv_tap_identity(s, kind, mode):
    case, table = R.upconv_tap_case(kind, s, *((5, 6) if kind == "up1" else (6, 8)))
    got, _ = _run_conv(case, mode)
    exp = R.conv_exact_ref(case, mode)
    ne = ((got != exp) | (got != got)).nonzero()
    if ne.numel():
        _, co, Y, X = ne[0].tolist()
        dy, dx = Y % 2, X % 2
        c, tap = table[(2 * dy + dx, co)]
        pytest.fail(f"{kind} set {s}: output channel {co} phase (dy, dx) = ({dy}, {dx}) at ({Y}, {X}) reads input channel {c} tap "
                    f"({tap // 3}, {tap % 3}): got {got[0, co, Y, X].item()} expected {exp[0, co, Y, X].item()}; {len(ne)} differ")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("s", range(9))
def test_last_tap_identity(s, mode):
    case = R.last_tap_case(s)
    got, _ = _run_conv(case, mode)
    exp = R.conv_exact_ref(case, mode)
    ne = ((got != exp) | (got != got)).nonzero()
    if ne.numel():
        _, o, Y, X = ne[0].tolist()
        tap = (s + 3 * o) % 9
        pytest.fail(f"conv_last set {s}: row {o} (tap ({tap // 3}, {tap % 3})) at ({Y}, {X}), tile row {Y % 16}: got "
                    f"{got[0, o, Y, X].item()} expected {exp[0, o, Y, X].item()}; {len(ne)} differ")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,f", [("fusion", 20), ("fusion", 24), ("fusion", 40), ("fusion", 64), ("up1", 24), ("up1", 64), ("up2", 24),
                                    ("up2", 64), ("last", 64)])
@pytest.mark.parametrize("geom", R.VSR_ROUNDED, ids=_gid)
def test_vsr_rounded(geom, kind, f, mode):
    n, h, w = geom
    k = {"fusion": 1, "up1": 1, "up2": 2, "last": 4}[kind]
    ref, yard, case = R.rounded_conv_reference(R.rounded_conv_case(kind, f, n, k * h, k * w), mode)
    got, _ = _run_conv(case, mode)
    hold_rounded("recon", f"{kind} F={f} {_gid(geom)} {mode}", mode, [(kind, got, ref, yard)])


# ================================================================================================================================
# csrc/mv_recon.h
# ================================================================================================================================
def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _mv_inputs(case, mode):
    from mobilesuperresolution_amd import packing as P
    f, b, n = case["f"], case["b"], case["n"]
    dt = DTYPES[mode]
    cw = P.mv_recon_cw(f)
    pack = torch.from_numpy(P.mv_recon_tables(f, cw)["pack"])
    flat = torch.cat([case[k].reshape(-1).float() for k in ("w_fu", "b_fu", "w_last", "b_last")] + [torch.zeros(1)])
    h, w = case["fb"].shape[-2:]
    fb, ff = case["fb"].view(n, b, f, h, w), case["ff"].view(n, b, f, h, w)
    return dict(dt=dt, cw=cw, blob=flat[pack].to(dt).cuda(), fb=[_nhwc(fb[i], dt, cw) for i in range(n)], ff=[_nhwc(ff[i], dt, cw) for i in range(n)],
                x=case["x"].view(n, b, 3, h, w).permute(1, 0, 2, 3, 4).contiguous().cuda(), geom=(f, b, n, h, w))


def _mv_fwd(inp, save=True, strided=False):
    """sr_mv_recon_fwd into a NaN-filled output (and u_save): (out (N, 3, 4h, 4w), u (N, 2f, h, w) or None, raw u_save), N frame-major.
    strided: the frames are [:, :, :3] of a NaN-filled (b, n, 5, h, w) parent (the model's input with its motion-vector channels) and
    the output is [:, 1:1 + n, :3] of a NaN-filled (b, n + 2, 4, 4h, 4w) parent, so that neither clip stride is n frame strides and
    neither frame stride is the dense frame; the rest of the output parent must still be NaN afterwards"""
    from mobilesuperresolution_amd import _lib as L
    f, b, n, h, w = inp["geom"]
    us = _nan(n, b, h, w, 2 * inp["cw"], dtype=inp["dt"]) if save else None
    x = inp["x"]
    xs, os_ = (n * 3 * h * w, 3 * h * w), (n * 48 * h * w, 48 * h * w)      # dense clip-major
    if strided:
        xp = _nan(b, n, 5, h, w)
        xp[:, :, :3] = inp["x"]
        x = xp[:, :, :3]
        big = _nan(b, n + 2, 4, 4 * h, 4 * w)
        out = big[:, 1:1 + n, :3]
        xs, os_ = (x.stride(0), x.stride(1)), (out.stride(0), out.stride(1))
        assert xs == (n * 5 * h * w, 5 * h * w) and os_ == ((n + 2) * 64 * h * w, 64 * h * w)
    else:
        out = _nan(b, n, 3, 4 * h, 4 * w)
    L.launch("sr_mv_recon_fwd", L.lib().sr_mv_recon_fwd, _ptrs(inp["fb"]), _ptrs(inp["ff"]), inp["cw"], x.data_ptr(), *xs,
             inp["blob"].data_ptr(), out.data_ptr(), *os_, us.data_ptr() if save else None, n, b, h, w,
             L.DTYPE_CODE[inp["dt"]], L.stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    if strided:
        assert _all_nan(big[:, 0]) and _all_nan(big[:, n + 1]) and _all_nan(big[:, 1:1 + n, 3]), "sr_mv_recon_fwd wrote outside its frames"
    o = out.permute(1, 0, 2, 3, 4).reshape(n * b, 3, 4 * h, 4 * w).cpu()
    if not save:
        return o, None, None
    assert not us[..., 2 * f:].ne(0).any() and not torch.isnan(us[..., 2 * f:]).any(), "u_save: padding channels are not exactly zero"
    return o, us.view(n * b, h, w, -1)[..., :2 * f].permute(0, 3, 1, 2).float().cpu(), us


def _mv_bwd(inp, case, us, wgs=128, rc_only=False):
    """sr_mv_recon_bwd on NaN-filled state gradients, slabs and gradients: dict(dc (N, 2f, h, w), the four gradients, parts)"""
    from mobilesuperresolution_amd import _lib as L
    f, b, n, h, w = inp["geom"]
    lib = L.lib()
    g = case["g"].view(n, b, 3, 4 * h, 4 * w).permute(1, 0, 2, 3, 4).contiguous().cuda()
    dfb = [_nan(b, h, w, 24, dtype=inp["dt"]) for _ in range(n)]
    dff = [_nan(b, h, w, 24, dtype=inp["dt"]) for _ in range(n)]
    parts = _nan(-(-n // 16) * wgs, lib.sr_mv_recon_slab())
    f2 = 2 * f
    grads = _nan(f2 * f2 + f2 + f2 * 75 + 3)
    L.launch("sr_mv_recon_bwd", lib.sr_mv_recon_bwd, _ptrs(inp["fb"]), _ptrs(inp["ff"]), us.data_ptr(), g.data_ptr(), n * 48 * h * w, 48 * h * w,
             inp["blob"].data_ptr(), _ptrs(dfb), _ptrs(dff), parts.data_ptr(), wgs, grads.data_ptr(), f, n, b, h, w, L.DTYPE_CODE[inp["dt"]],
             L.stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    pad = torch.stack(dfb + dff)[..., f:]
    assert not pad.ne(0).any() and not torch.isnan(pad).any(), "state gradients: padding channels are not exactly zero"
    dc = torch.cat([torch.stack(dfb)[..., :f], torch.stack(dff)[..., :f]], -1).view(n * b, h, w, f2).permute(0, 3, 1, 2).float().cpu()
    o1, o2, o3 = f2 * f2, f2 * f2 + f2, f2 * f2 + f2 + f2 * 75
    grads = grads.cpu()
    tiles = -(-h // 8) * -(-w // 16)
    owned = sum(min(min(16, n - f0) * b * tiles, wgs) for f0 in range(0, n, 16))
    # what a workgroup writes of its slab: rows 0..47 of dW_last [64][80] and of dW_fu [64][64], and db_last [3]
    for lo, hi in ((0, 48 * 80), (64 * 80, 64 * 80 + 48 * 64), (64 * 80 + 64 * 64, 64 * 80 + 64 * 64 + 3)):
        assert not torch.isnan(parts[:owned, lo:hi]).any(), "a slab a workgroup owns holds a NaN where it is summed"
    assert _all_nan(parts[owned:]), "a slab row no workgroup owns was written"
    return dict(dc=dc, dW_fu=grads[:o1].view(f2, f2, 1, 1), db_fu=grads[o1:o2], dW_last=grads[o2:o3].view(f2, 3, 5, 5), db_last=grads[o3:])


def _per_frame(name, got, exp, b):
    """one triple per frame, so that a failure names the frame"""
    return [(f"{name}[frame {i}]", got[i * b:(i + 1) * b], exp[i * b:(i + 1) * b]) for i in range(got.shape[0] // b)]


def _hold_mv(case, mode, tag, backward, wgs=128, save=True):
    inp = _mv_inputs(case, mode)
    ref = R.mv_exact_ref(case, mode)
    out, u, us = _mv_fwd(inp, save or backward)
    b = case["b"]
    pairs = _per_frame("out", out, ref["out"], b)
    if u is not None:
        pairs += _per_frame("u", u, ref["u"], b)
    if backward:
        hold_exact(tag, pairs)                             # the backward reads the kernel's own u_save
        got = _mv_bwd(inp, case, us, wgs)
        pairs = _per_frame("dc", got["dc"], ref["dc"], b) + [(k, got[k], ref[k]) for k in R.MV_GRADS]
    hold_exact(tag, pairs)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", R.MV_WIDTHS)
@pytest.mark.parametrize("geom", R.MV_EXACT, ids=_gid)
def test_mv_forward_exact(geom, f, mode):
    """all four instantiations (F = 20, 24: cw = 24; 40, 64: cw = 64, a 4 x 16 tile in fp32), with and without u_save"""
    case = R.mv_case(f, geom[0], 1, geom[1], geom[2])
    _hold_mv(case, mode, ("mv fwd", f, geom, mode), False, save=True)
    _hold_mv(case, mode, ("mv fwd no u_save", f, geom, mode), False, save=False)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [20, 24])
@pytest.mark.parametrize("geom", R.MV_EXACT, ids=_gid)
def test_mv_backward_exact(geom, f, mode):
    _hold_mv(R.mv_case(f, geom[0], 1, geom[1], geom[2]), mode, ("mv bwd", f, geom, mode), True)


@pytest.mark.parametrize("f", [20, 24])
@pytest.mark.parametrize("geom", R.MV_RICH, ids=_gid)
def test_mv_both_signs_exact_bf16(geom, f):
    """pre-activations of both signs and exact zeros, forward and backward (dpre = du * 0.1f on the negative side)"""
    _hold_mv(R.mv_case(f, geom[0], 1, geom[1], geom[2], True), "bf16", ("mv signs", f, geom), True)


def _hold_blend(tag, out, ref, h, w):
    err = (out.double() - ref["out"]).abs()
    tol = R.blend_bound(ref["D"], h, w) + 2.0 ** -24 * ref["out"].abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"recon blend | {tag} | max err {float(err.max()):.2e} | worst err / bound {worst:.3f}")
    assert not torch.isnan(out).any() and bool((err <= tol).all()), (tag, worst)


@pytest.mark.parametrize("f", R.MV_WIDTHS)
@pytest.mark.parametrize("geom", R.MV_RICH_FORWARD, ids=_gid)
def test_mv_both_signs_forward_bf16(geom, f):
    """u with both signs and bf16 ties bit for bit at every size; out bit for bit where mv_out_exact, else within blend_bound"""
    case = R.mv_case(f, geom[0], 1, geom[1], geom[2], True, False)
    ref = R.mv_exact_ref(case, "bf16")
    out, u, _ = _mv_fwd(_mv_inputs(case, "bf16"))
    hold_exact(("mv signs fwd", f, geom), [("u", u, ref["u"])] + ([("out", out, ref["out"])] if R.mv_out_exact(case) else []))
    _hold_blend(f"signs F={f} {_gid(geom)}", out, ref, geom[1], geom[2])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", R.MV_WIDTHS)
@pytest.mark.parametrize("geom", R.MV_BOUNDED, ids=_gid)
def test_mv_forward_bounded(geom, f, mode):
    """sizes that are no power of two: lambda is not exact in fp32, so u is held bit for bit and the output per element within
    recon_ref.blend_bound of the float64 blend of the exact D (its docstring says what that leaves for structural errors)."""
    case = R.mv_case(f, geom[0], 1, geom[1], geom[2], False, False)
    ref = R.mv_exact_ref(case, mode)
    out, u, _ = _mv_fwd(_mv_inputs(case, mode))
    hold_exact(("mv bounded", f, geom, mode), [("u", u, ref["u"])])
    _hold_blend(f"F={f} {_gid(geom)} {mode}", out, ref, geom[1], geom[2])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("s", range(2))
def test_mv_tap_identity(s, mode):
    """one u channel per (o, ky, kx): forward a placed, blended copy; backward dW_last and the state gradients (= du)"""
    case = R.mv_tap_case(s)
    inp = _mv_inputs(case, mode)
    ref = R.mv_exact_ref(case, mode)
    out, u, us = _mv_fwd(inp)
    msg = R.name_mv_tap(case, out, ref["out"].float())
    assert msg is None, (s, mode, msg)
    got = _mv_bwd(inp, case, us)
    hold_exact(("mv taps", s, mode), [("u", u, ref["u"]), ("du = dc", got["dc"], ref["dc"]), ("dW_last", got["dW_last"], ref["dW_last"]),
                                      ("db_last", got["db_last"], ref["db_last"])])
    d = ((got["dW_last"] != ref["dW_last"].float()) | (got["dW_last"] != got["dW_last"])).nonzero()
    assert d.numel() == 0, f"dW_last: first wrong entry (u channel, o, ky, kx) = {d[0].tolist()}"


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", R.MV_WIDTHS)
@pytest.mark.parametrize("n", R.MV_CHUNKS)
def test_mv_frame_chunks_forward(n, f, mode):
    """17 and 33 distinct frames: two and three launches of at most 16; every frame's output and u is that frame's reference"""
    _hold_mv(R.mv_case(f, 2, n, 8, 16, False, False), mode, ("mv chunks fwd", n, f, mode), False)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("n", R.MV_CHUNKS)
def test_mv_frame_chunks_backward(n, mode):
    """every frame's state gradients and the four parameter gradients over the whole clip; the last chunk is one frame (2 items)"""
    _hold_mv(R.mv_case(20, 2, n, 8, 16), mode, ("mv chunks bwd", n, mode), True)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("wgs", R.MV_WALK_WGS)
def test_mv_tile_walk(wgs, mode):
    """24 items on 1, 5, 23, 24, 25 and 128 workgroups: accumulators kept across tiles, LDS images rebuilt each trip, one slab per
    workgroup; unowned slab rows stay NaN (checked in _mv_bwd)"""
    _hold_mv(R.mv_case(20, *R.MV_WALK), mode, ("mv walk", wgs, mode), True, wgs=wgs)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("wgs", [1, 5])
def test_mv_tile_walk_across_chunks(wgs, mode):
    _hold_mv(R.mv_case(20, 2, 17, 8, 16), mode, ("mv walk chunks", wgs, mode), True, wgs=wgs)


# ---- a quarter-dense cotangent, sizes that are no power of two, both signs at tile sizes ---------------------------------------
def _hold_within(tag, rows):
    """rows: (name, got, float64 reference, per-element tolerance)"""
    bad = []
    for name, got, ref, tol in rows:
        err = (got.double() - ref).abs()
        worst = float((err / tol.clamp_min(1e-300)).max())
        print(f"recon bound | {tag} | {name} | max err {float(err.max()):.2e} of {float(ref.abs().max()):.2e} | worst err / bound {worst:.3f}")
        if bool(torch.isnan(got).any()) or not bool((err <= tol).all()) or not float(ref.abs().max()) > 0:
            bad.append((name, worst))
    assert not bad, (tag, bad)


def _hold_mv_dense(case, mode, tag, wgs=128):
    """forward: u bit for bit, out bit for bit where mv_out_exact, else within blend_bound.  Backward on a power-of-two image: dc
    and db_last bit for bit (a rich case: dc where case['dc_exact'], one bf16 ulp of its magnitude elsewhere); the gradients that
    sum over the clip within grad_bounds (fp32, per element) or the yardstick (bf16).  Other sizes: every gradient so."""
    from tests.parity_kit import rel_max
    inp = _mv_inputs(case, mode)
    ref = R.mv_exact_ref(case, mode)
    out, u, us = _mv_fwd(inp)
    b, (h, w) = case["b"], case["fb"].shape[-2:]
    lam_ok = R.is_pow2(h) and R.is_pow2(w)
    hold_exact(tag, _per_frame("u", u, ref["u"], b) + (_per_frame("out", out, ref["out"], b) if R.mv_out_exact(case) else []))
    _hold_blend(str(tag), out, ref, h, w)
    got = _mv_bwd(inp, case, us, wgs)
    loose = ("dW_fu", "db_fu", "dW_last")
    if lam_ok:
        pairs = [("db_last", got["db_last"], ref["db_last"])]
        if "dc_exact" in case:
            m, exp = case["dc_exact"], ref["dc"].float()
            assert torch.equal(got["dc"][m], exp[m]), (tag, "dc differs where its sum is exact", int((got["dc"][m] != exp[m]).sum()))
            mag = torch.einsum("oi,nohw->nihw", case["w_fu"].double().abs().flatten(1), ref["dpre"].abs())
            assert bool(((got["dc"].double() - ref["dc"]).abs() <= 2.0 ** -7 * mag)[~m].all()), (tag, "dc outside one bf16 ulp where it rounds")
        else:
            pairs += _per_frame("dc", got["dc"], ref["dc"], b)
        hold_exact(tag, pairs)
    else:
        loose = ("dc",) + loose
    if mode == "fp32":
        tol = R.grad_bounds(case, ref)
        _hold_within(tag, [(k, got[k], ref[k], tol[k]) for k in loose + (() if lam_ok else ("db_last",))])
    else:
        plain, emu = R.mv_run(case), R.emulate_mv(case, "bf16")
        hold_rounded("recon", str(tag), "bf16", [(k, got[k], plain[k], rel_max(emu[k], plain[k])) for k in loose])
        if not lam_ok:
            hold_rounded("recon", str(tag), "fp32", [("db_last", got["db_last"], plain["db_last"], rel_max(emu["db_last"], plain["db_last"]))])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [20, 24])
@pytest.mark.parametrize("geom", R.MV_EXACT, ids=_gid)
def test_mv_backward_dense(geom, f, mode):
    """a quarter of the cotangent nonzero at every exact size: dD, du, dpre, dc at every pixel of every tile"""
    _hold_mv_dense(R.mv_case(f, geom[0], 1, geom[1], geom[2], dense=True), mode, ("mv dense", f, geom, mode))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [20, 24])
@pytest.mark.parametrize("geom", R.MV_BOUNDED, ids=_gid)
def test_mv_backward_bounded(geom, f, mode):
    """ragged tiles, sizes that are no power of two: fp32 gradients per element within grad_bounds, bf16 within the yardstick"""
    _hold_mv_dense(R.mv_case(f, geom[0], 1, geom[1], geom[2], dense=True), mode, ("mv bounded bwd", f, geom, mode))


@pytest.mark.parametrize("f", [20, 24])
@pytest.mark.parametrize("geom", R.MV_RICH_TILES, ids=_gid)
def test_mv_both_signs_tiles_bf16(geom, f):
    """negative u in the contractions and dpre = du * 0.1f on whole tiles, seams included"""
    _hold_mv_dense(R.mv_case(f, geom[0], 1, geom[1], geom[2], True, True, 0, True), "bf16", ("mv signs tiles", f, geom))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("n", R.MV_CHUNKS)
def test_mv_frame_chunks_backward_dense(n, mode):
    _hold_mv_dense(R.mv_case(20, 2, n, 8, 16, dense=True), mode, ("mv chunks dense", n, mode))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("wgs", R.MV_WALK_WGS)
def test_mv_tile_walk_dense(wgs, mode):
    _hold_mv_dense(R.mv_case(20, *R.MV_WALK, dense=True), mode, ("mv walk dense", wgs, mode), wgs=wgs)


@pytest.mark.parametrize("wgs", [1, 5, 24])
def test_mv_tile_walk_both_signs_bf16(wgs):
    _hold_mv_dense(R.mv_case(20, *R.MV_WALK, True, True, 0, True), "bf16", ("mv walk signs", wgs), wgs=wgs)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("f", R.MV_WIDTHS)
@pytest.mark.parametrize("geom", R.MV_ROUNDED, ids=_gid)
def test_mv_rounded(geom, f, mode):
    case = R.mv_rounded_case(f, geom[0], 1, geom[1], geom[2])
    ref, yard = R.mv_rounded_reference(case, mode)
    inp = _mv_inputs(case, mode)
    out, u, us = _mv_fwd(inp)
    rows = [("out", out, ref["out"], yard["out"]), ("u", u, ref["u"], yard["u"])]
    if f <= 24:
        got = _mv_bwd(inp, case, us)
        rows += [(k, got[k], ref[k], yard[k]) for k in ("dc",) + R.MV_GRADS[:3]]
        # db_last is a sum of the fp32 cotangent: no bf16 value enters it in either mode, so the fp32 rule holds it in both
        hold_rounded("recon", f"mv F={f} {_gid(geom)} {mode}", "fp32", [("db_last", got["db_last"], ref["db_last"], yard["db_last"])])
    hold_rounded("recon", f"mv F={f} {_gid(geom)} {mode}", mode, rows)


# ================================================================================================================================
# refusals
# ================================================================================================================================
def test_refused_calls_leave_their_buffers_untouched():
    from mobilesuperresolution_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr(torch.device("cuda"))
    case = R.mv_case(20, 1, 2, 8, 16)
    inp = _mv_inputs(case, "fp32")
    f, b, n, h, w = inp["geom"]
    x, blob = inp["x"], inp["blob"]
    out, us = _nan(b, n, 3, 4 * h, 4 * w), _nan(n, b, h, w, 48)

    def fwd(fb, cw):
        return lib.sr_mv_recon_fwd(_ptrs(fb), _ptrs(inp["ff"]), cw, x.data_ptr(), n * 3 * h * w, 3 * h * w, blob.data_ptr(), out.data_ptr(),
                                   n * 48 * h * w, 48 * h * w, us.data_ptr(), n, b, h, w, 0, st)
    assert fwd(inp["fb"], 32) == -2                                            # bad cw
    assert fwd([inp["fb"][0], None], 24) == -2                                 # a null frame pointer
    torch.cuda.synchronize()
    assert _all_nan(out) and _all_nan(us)
    _, _, us_ok = _mv_fwd(inp)
    g = case["g"].view(n, b, 3, 4 * h, 4 * w).permute(1, 0, 2, 3, 4).contiguous().cuda()
    dfb, dff = [_nan(b, h, w, 24) for _ in range(n)], [_nan(b, h, w, 24) for _ in range(n)]
    parts, grads = _nan(128, lib.sr_mv_recon_slab()), _nan(40 * 40 + 40 + 40 * 75 + 3)

    def bwd(F, wgs, dfb_):
        return lib.sr_mv_recon_bwd(_ptrs(inp["fb"]), _ptrs(inp["ff"]), us_ok.data_ptr(), g.data_ptr(), n * 48 * h * w, 48 * h * w, blob.data_ptr(),
                                   _ptrs(dfb_), _ptrs(dff), parts.data_ptr(), wgs, grads.data_ptr(), F, n, b, h, w, 0, st)
    assert bwd(25, 128, dfb) == -2                                             # F > 24: the backward exists on the 24-wide route only
    assert bwd(20, 0, dfb) == -2                                               # wgs = 0
    assert bwd(20, 128, [dfb[0], None]) == -2                                  # a null frame pointer
    torch.cuda.synchronize()
    assert all(_all_nan(t) for t in dfb + dff + [parts, grads])
    # sr_c64_recon_fwd: a bad cw for the fusion stage
    from mobilesuperresolution_amd import packing as P
    boff = (ctypes.c_long * 5)(*P.c64_recon_tables(24)["boff"])
    blob64 = torch.zeros(P.c64_recon_tables(24)["pack"].size, device="cuda")
    hb = torch.zeros(1, 4, 4, 32, device="cuda")
    sc = [_nan(1, 4, 4, 64), _nan(1, 8, 8, 64), _nan(1, 16, 16, 64), _nan(1, 16, 16, 64)]
    o, fr = _nan(1, 3, 16, 16), torch.zeros(1, 3, 4, 4, device="cuda")
    for cw, stages in ((32, 31), (24, 0), (24, 32)):
        assert lib.sr_c64_recon_fwd(hb.data_ptr(), hb.data_ptr(), cw, fr.data_ptr(), fr.stride(0), blob64.data_ptr(), boff, sc[0].data_ptr(),
                                    sc[1].data_ptr(), sc[2].data_ptr(), sc[3].data_ptr(), o.data_ptr(), o.stride(0), 1, 4, 4, 0, stages, st) == -2
    torch.cuda.synchronize()
    assert all(_all_nan(t) for t in sc + [o])
