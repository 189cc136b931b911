"""tests/recon_ref.py without a GPU: the float64 references against fixtures G19, G4 and G11 and against ATen, the kernels' LeakyReLU
rule, the exactness conditions of every exact case of tests/test_gpu_recon_ref.py (and that check_exact rejects what it must), the
bf16 ties at every stated rounding point, the dropped-rounding families, and the fact the exact / bounded split of the
MotionVectorVSR cases rests on: the fp32 blend weight is exact if and only if the image size is a power of two."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mv_recon_ref as M
from tests import recon_ref as R
from tests.parity_kit import bf16_round, rel_max
from tests.test_mv_recon_host import load_g11
from tests.test_trunk64_layout import _flow_warp_cpu, _trunk_cpu
from tests.test_vsr_recon_host import load_g19

# measured distances of the float64 references from the fp32 fixtures (relative max-abs); the bounds are 4 x these
G19_MEASURED = {64: 1.3e-7, 24: 1.3e-7}
G11_MEASURED = 4.1e-7


# ---- the references, pinned ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [64, 24])
def test_references_reproduce_g19(f):
    """fixture G19 (the reference project's BasicVSR_origin, fp32) through the module's own parameters: the trunks as
    tests/test_vsr_recon_host.py restates them, the reconstruction through fusion_ref / upconv_ref / last_ref in float64"""
    x, ff, fb, models = load_g19()
    p, want = models[f]
    p = {k: v.double() for k, v in p.items()}
    x, ff, fb = x.double(), ff.double(), fb.double()
    b, n, _, h, w = x.shape
    feats = {}
    for name, flows, order in (("backward", fb, range(n - 1, -1, -1)), ("forward", ff, range(n))):
        feat, res = x.new_zeros(b, f, h, w), {}
        for i in order:
            if res:
                feat = _flow_warp_cpu(feat, flows[:, i if name == "backward" else i - 1].permute(0, 2, 3, 1))
            feat = _trunk_cpu(p, f"{name}_trunk.", torch.cat([x[:, i], feat], 1), 1)
            res[i] = feat
        feats[name] = res
    outs = []
    for i in range(n):
        t = R.fusion_ref(feats["backward"][i], feats["forward"][i], p["fusion.weight"], p["fusion.bias"])
        t = R.upconv_ref(t, p["upconv1.weight"], p["upconv1.bias"])
        t = R.upconv_ref(t, p["upconv2.weight"], p["upconv2.bias"])
        t = R.lrelu(F.conv2d(t, p["conv_hr.weight"], p["conv_hr.bias"], padding=1))
        outs.append(R.last_ref(t, p["conv_last.weight"], p["conv_last.bias"], x[:, i]))
    e = rel_max(torch.stack(outs, 1), want.double())
    print(f"\nrecon_ref against G19 F={f}: {e:.2e} (measured {G19_MEASURED[f]:.1e})")
    assert e <= 4 * G19_MEASURED[f]


def test_upconv_with_an_identity_centre_tap_is_g4_pixel_shuffle(golden_dir):
    import os
    z = np.load(os.path.join(golden_dir, "g4_pixel_shuffle.npz"))
    xin, want = torch.from_numpy(z["x_r2"]).double(), torch.from_numpy(z["y_r2"]).double()
    co = xin.shape[1]
    wt = torch.zeros(co, co, 3, 3, dtype=torch.float64)
    wt[torch.arange(co), torch.arange(co), 1, 1] = 1.0
    assert torch.equal(R.upconv_ref(xin, wt, torch.zeros(co, dtype=torch.float64), slope=1.0), want)


def test_base_equals_float32_interpolate_on_eighths():
    g = torch.Generator().manual_seed(3)
    fr = torch.randint(0, 9, (2, 3, 5, 7), generator=g).float() / 8.0
    got = R.last_ref(torch.zeros(2, 64, 20, 28, dtype=torch.float64), torch.zeros(3, 64, 3, 3, dtype=torch.float64),
                     torch.zeros(3, dtype=torch.float64), fr.double())
    assert torch.equal(got, F.interpolate(fr, scale_factor=4, mode="bilinear", align_corners=False).double())


def test_mv_reference_reproduces_g11():
    d = load_g11()
    x = d["x"].double()
    b, n, _, h, w = x.shape
    fl = lambda t: t.double().transpose(0, 1).reshape(n * b, -1, h, w)        # frame-major
    case = dict(fb=fl(d["feat_backward"].flip(1)), ff=fl(d["feat_forward"]), x=fl(x[:, :, :3]), w_fu=d["p/fusion.weight"], b_fu=d["p/fusion.bias"],
                w_last=d["p/conv_last.weight"], b_last=d["p/conv_last.bias"])
    out = R.mv_run(case)["out"].view(n, b, 3, 4 * h, 4 * w).transpose(0, 1)
    e = rel_max(out, d["out"].double())
    print(f"\nrecon_ref.mv_run against G11: {e:.2e}")
    assert e <= 4 * G11_MEASURED


def test_with_slope_a_tenth_the_references_are_the_plain_operations():
    case = R.mv_rounded_case(20, 2, 2, 5, 6)
    c64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in case.items()}
    r = R.mv_run(c64)
    out, c, u, D = M.forward(c64["fb"], c64["ff"], c64["x"], c64["w_fu"], c64["b_fu"], c64["w_last"], c64["b_last"])
    assert rel_max(r["out"], out) <= 1e-13 and torch.equal(r["u"], u)        # (mv_run blends columns first, as the kernels do)
    ref_u = F.leaky_relu(F.conv2d(torch.cat([c64["fb"], c64["ff"]], 1), c64["w_fu"], c64["b_fu"]), 0.1)
    assert (u - ref_u).abs().max() <= 1e-12
    b = M.backward(c64["g"], c, u, c64["w_fu"], c64["w_last"])
    for k in ("dc", "dW_fu", "db_fu", "dW_last"):
        assert rel_max(r[k], b[k]) <= 1e-13, k
    assert (r["db_last"] - b["db_last"]).abs().max() <= 1e-10                  # sum of g = sum of dD: the blend's weights sum to one
    # the analytic backward against autograd of the forward, float64
    leaves = {k: c64[k].clone().requires_grad_(True) for k in ("fb", "ff", "w_fu", "b_fu", "w_last", "b_last")}
    R.mv_run(dict(leaves, x=c64["x"]))["out"].backward(c64["g"])
    for got, ref in ((r["dc"][:, :20], leaves["fb"].grad), (r["dc"][:, 20:], leaves["ff"].grad), (r["dW_fu"], leaves["w_fu"].grad),
                     (r["db_fu"], leaves["b_fu"].grad), (r["dW_last"], leaves["w_last"].grad), (r["db_last"], leaves["b_last"].grad)):
        assert (got - ref).abs().max() <= 1e-11 * max(1.0, ref.abs().max().item())
    # BasicVSR_origin side
    for kind in ("fusion", "up1", "last"):
        cc = R.rounded_conv_case(kind, 24, 1, 8, 12)
        x = torch.cat([cc["fb"], cc["ff"]], 1).double() if kind == "fusion" else cc["x"].double()
        pre = F.conv2d(x, cc["w"].double(), cc["b"].double(), padding=cc["w"].shape[-1] // 2)
        want = {"fusion": lambda: F.leaky_relu(pre, 0.1), "up1": lambda: F.leaky_relu(F.pixel_shuffle(pre, 2), 0.1),
                "last": lambda: pre + F.interpolate(cc["frame"].double(), scale_factor=4, mode="bilinear", align_corners=False)}[kind]()
        assert (R.conv_ref(cc) - want).abs().max() <= 1e-12


def test_act_exact_is_one_fp32_multiply():
    t = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    want = torch.where(t > 0, t, torch.tensor(0.1, dtype=torch.float32) * t)
    assert torch.equal(R.act_exact(t.double()).float(), want) and R.SLOPE32 != 0.1


# ---- the exact cases -------------------------------------------------------------------------------------------------------------
def test_every_conv_case_is_exact_and_the_stores_see_bf16_ties():
    ties = {}
    for kind, fs, k in (("fusion", R.MV_WIDTHS, 1), ("up1", (24, 64), 1), ("up2", (24, 64), 2)):
        for f in fs:
            for n, h, w in R.VSR_GEOMETRIES:
                case = R.conv_case(kind, f, n, k * h, k * w)                # checked on construction; again here, explicitly
                ties[kind] = ties.get(kind, 0) + R.check_exact_conv(case)
                ref = R.conv_exact_ref(case, "bf16")
                assert torch.equal(ref, bf16_round(ref)) and not torch.equal(ref, R.conv_exact_ref(case, "fp32"))
    for n, h, w in R.LAST_GEOMETRIES:
        R.check_exact_conv(R.conv_case("last", 64, n, 4 * h, 4 * w))
    print("\nbf16 ties per store:", ties)
    assert all(v > 0 for v in ties.values())
    assert R.upconv_tap_sets_cover()
    for s in range(9):
        c = R.last_tap_case(s)
        assert int((c["w"] != 0).any(1).sum()) == 3 and int((c["x"] != 0).sum(1).max()) == 1


def test_every_mv_case_is_exact_and_every_rounding_point_sees_ties():
    total = {}
    def add(c):
        for k, v in c["ties"]["bf16"].items():
            total[k] = total.get(k, 0) + v
    for g in R.MV_EXACT:
        for f in R.MV_WIDTHS:
            add(R.mv_case(f, g[0], 1, g[1], g[2], False, f <= 24))
    for g in R.MV_RICH:
        for f in (20, 24):
            add(R.mv_case(f, g[0], 1, g[1], g[2], True))
    for g in R.MV_RICH_FORWARD:
        for f in R.MV_WIDTHS:
            c = R.mv_case(f, g[0], 1, g[1], g[2], True, False)
            add(c)
            assert c["ties"]["bf16"]["u"] > 0
    for g in R.MV_BOUNDED:
        for f in R.MV_WIDTHS:
            R.mv_case(f, g[0], 1, g[1], g[2], False, False)
    for n in R.MV_CHUNKS:
        add(R.mv_case(20, 2, n, 8, 16))
        for f in R.MV_WIDTHS:
            R.mv_case(f, 2, n, 8, 16, False, False)
    add(R.mv_case(20, *R.MV_WALK))
    for g in R.MV_EXACT[:8] + R.MV_BOUNDED[:3]:            # a quarter-dense cotangent (the rest are built by the GPU tests, same code)
        c = R.mv_case(20, g[0], 1, g[1], g[2], dense=True)
        assert 0.2 <= c["density"] <= 0.32
    for g in R.MV_RICH_TILES[:2]:
        c = R.mv_case(20, g[0], 1, g[1], g[2], True, True, 0, True)
        add(c)
        assert float(c["dc_exact"].double().mean()) >= 0.9 and bool((c["fb"] != 0).any())
    print("\nbf16 ties per rounding point:", total)
    assert all(total[k] > 0 for k in ("u", "dD", "dpre", "dc"))


def _broken(case, **kw):
    c = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in case.items()}
    c.update(kw)
    return c


def test_check_exact_rejects_what_it_must():
    case = R.conv_case("up1", 24, 1, 5, 6)
    w = case["w"]
    nz = (w != 0).nonzero()
    i = tuple(nz[0].tolist())
    def edit(fn):
        v = w.clone()
        fn(v)
        return _broken(case, w=v)
    def same_row(v):
        v[1] = v[0]
    def no_tap(v):
        v[:, :, 2, 2] = 0
    for name, bad in (("non-dyadic", edit(lambda v: v.__setitem__(i, v[i] * 0.3))), ("2^-40", edit(lambda v: v.__setitem__(i, 2.0 ** -40))),
                      ("repeated row", edit(same_row)), ("missing tap", edit(no_tap))):
        with pytest.raises(ValueError):
            R.check_exact_conv(bad)
    mv = R.mv_case(20, 1, 1, 4, 8)
    R.check_exact_mv(mv)
    wl = mv["w_last"]
    j = tuple((wl != 0).nonzero()[0].tolist())
    def edit_mv(fn):
        v = wl.clone()
        fn(v)
        return _broken(mv, w_last=v)
    def same_row_mv(v):
        v[:, 0, 0, 1] = v[:, 0, 0, 0]
    def no_tap_mv(v):
        v[:, 1, 3, 2] = 0
    for name, bad in (("non-dyadic", edit_mv(lambda v: v.__setitem__(j, v[j] * 0.3))), ("2^-40", edit_mv(lambda v: v.__setitem__(j, 2.0 ** -40))),
                      ("repeated row", edit_mv(same_row_mv)), ("missing tap", edit_mv(no_tap_mv))):
        with pytest.raises(ValueError):
            R.check_exact_mv(bad)
    # fp32: a pre-activation that is not positive; a cotangent too dense for the weight-gradient sums
    with pytest.raises(ValueError):
        R.check_exact_mv(_broken(mv, b_fu=-mv["b_fu"]), "fp32")
    big = R.mv_case(20, 1, 1, 32, 64)
    with pytest.raises(ValueError):
        R.check_exact_mv(_broken(big, g=torch.ones_like(big["g"])))


def test_backward_families_see_a_dropped_rounding():
    """a reference WITHOUT the dD rounding (dD fed to the contractions in fp32) or without the dpre rounding differs from the shipped
    one downstream, on every backward family: a kernel that skipped either rounding cannot pass these cases"""
    for case in [R.mv_case(20, g[0], 1, g[1], g[2], dense=True) for g in R.MV_EXACT[2:8]] + [R.mv_case(20, 2, 17, 8, 16, dense=True)]:
        ref = R.mv_exact_ref(case, "bf16")
        no_dd, no_dp = R.mv_exact_ref(case, "bf16", drop=("dD",)), R.mv_exact_ref(case, "bf16", drop=("dpre",))
        assert not torch.equal(no_dd["dW_last"], ref["dW_last"]) and not torch.equal(no_dd["du"], ref["du"])
        assert not torch.equal(no_dp["dW_fu"], ref["dW_fu"]) and not torch.equal(no_dp["dc"], ref["dc"])


# ---- the blend weight ------------------------------------------------------------------------------------------------------------
def test_the_fp32_blend_weight_is_exact_only_on_powers_of_two():
    for h in range(1, 65):
        want = (2 * np.arange(4 * h, dtype=np.float64) + 1) / (8 * h)
        for fused in (False, True):
            lam, one_minus = R.mv_lambda32(h, fused)
            exact = np.array_equal(lam, want) and np.array_equal(one_minus, 1 - want)
            if R.is_pow2(h):
                assert exact, (h, fused)
                assert np.abs(lam - want).max() <= 4 * h * 2.0 ** -23
    lam, _ = R.mv_lambda32(12)
    assert not np.array_equal(lam, (2 * np.arange(48, dtype=np.float64) + 1) / 96)
    for h in (7, 9, 12, 18, 25, 49):                       # the bounded sizes: within the 4 max(h, w) ulp the bound allows
        for fused in (False, True):
            lam, _ = R.mv_lambda32(h, fused)
            assert np.abs(lam - (2 * np.arange(4 * h, dtype=np.float64) + 1) / (8 * h)).max() <= 4 * h * 2.0 ** -23
    assert R.mv_out_exact(R.mv_case(20, 1, 1, 8, 16)) and not R.mv_out_exact(R.mv_case(20, 1, 1, 12, 16, False, False))


def test_mv_tap_sets_reach_every_neighbour_term_at_seams_and_image_edges():
    """for every row (o, ky, kx) of conv_last: its u channel is live at a pixel whose D neighbour term crosses the 8 x 16 tile seam
    (ky = 4: LR row 7 feeds D row 32, the first of the next tile; kx = 4: LR column 15) and at the last LR row / column, which
    feed image row 4h / column 4w; and the [i = j = 0] corner (ky = kx = 4) at the seam corner and at the image corner"""
    seen = set()
    for s in range(2):
        case = R.mv_tap_case(s)
        c = torch.cat([case["fb"], case["ff"]], 1)[0]
        h, w = c.shape[-2:]
        for k, r in case["rows"].items():
            o, ky, kx = r // 25, (r % 25) // 5, r % 5
            seen.add(r)
            live = c[k] != 0
            assert int((case["w_last"][k] != 0).sum()) == 1 and case["w_last"][k, o, ky, kx] != 0
            if ky == 4:
                assert bool(live[7].any()) and bool(live[h - 1].any()), (r, "row seam / image row 4h")
            if kx == 4:
                assert bool(live[:, 15].any()) and bool(live[:, w - 1].any()), (r, "column seam / image column 4w")
            if ky == 4 and kx == 4:
                assert bool(live[7, 15]) and bool(live[h - 1, w - 1]), (r, "corner term at the seam corner / image corner")
    assert seen == set(range(75))
