"""tests/prep_ref.py pinned on the CPU: its restatements against torch's own formulations (torch._weight_norm and its autograd,
index_select / index_add, autograd of the block formula), on the tables of packing.nas_prep_tables, its exact cases against their
own conditions (shipped cases accepted, spoiled ones refused), and every seeded defect shown on at least one shipped case -- the
cases test_gpu_prep_ref.py holds the kernels to can fail."""
import copy

import numpy as np
import pytest
import torch

from tests import prep_ref as R
from tests.parity_kit import rel_max

NAN = float("nan")


def _same(a, b):
    """equal, NaN (unwritten) equal to NaN"""
    return torch.equal(a.double().nan_to_num(1e300), b.double().nan_to_num(1e300))


# ---- the restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", R.ROUNDED_CASES)
def test_weight_norm_reference_equals_torch_weight_norm_and_its_autograd(i):
    t = R.grads_case(i, exact=False)["table"]
    f = t["flat"]
    src = R.wn_forward(f, t["src0"], t["chan_tab"], t["bias_tab"], t["bias_const"])
    gflat = R.wn_backward(f, t["dw"], torch.full_like(f, NAN), t["chan_tab"], t["bias_tab"])
    for v_off, g_off, k, dst in t["chan_tab"].tolist():
        v = f[v_off:v_off + k].clone().view(1, k).requires_grad_(True)
        g = f[g_off].clone().view(1, 1).requires_grad_(True)
        w = torch._weight_norm(v, g, 0)
        w.backward(t["dw"][dst:dst + k].view(1, k))
        assert rel_max(src[dst:dst + k], w.detach().view(-1)) <= 1e-12
        assert rel_max(gflat[v_off:v_off + k], v.grad.view(-1)) <= 1e-12
        assert rel_max(gflat[g_off].view(1), g.grad.view(1)) <= 1e-12
    for j, (a, b, d) in enumerate(t["bias_tab"].tolist()):
        assert src[d] == f[a] + (f[b] if b >= 0 else 0.0) + t["bias_const"][j]
        assert gflat[a] == t["dw"][d] and (b < 0 or gflat[b] == t["dw"][d])
    assert bool(gflat[~t["gnamed"]].isnan().all()) and not bool(gflat[t["gnamed"]].isnan().any())
    assert _same(src[~t["named"]], t["src0"][~t["named"]])


@pytest.mark.parametrize("i", R.PACK_CASES)
def test_pack_equals_index_select(i):
    case = R.pack_case(i)
    src, blobs = R.pack_expected(case, torch.bfloat16)
    for s, blob in zip(case["segs"], blobs):
        rows = [torch.index_select(src[s["src_off"] + r * s["src_stride"]:], 0, s["idx"].long()) for r in range(s["reps"])]
        exp = torch.cat(rows).float()
        assert torch.equal(blob, exp if s["as_float"] else exp.bfloat16())
        assert blob.dtype == (torch.float32 if s["as_float"] else torch.bfloat16) and blob.numel() == s["n"] * s["reps"]


@pytest.mark.parametrize("i", R.GRADS_CASES)
def test_unpack_equals_index_add(i):
    case = R.grads_case(i)
    got = R.unpack(case["dsrc0"], case["segs"])
    exp = case["dsrc0"].clone()
    exp[case["dnamed"]] = 0.0
    for s in case["segs"]:
        p = s["partial"].view(s["reps"], s["wgs"], s["slab"])
        for r in range(s["reps"]):
            for w in range(s["wgs"]):
                exp.index_add_(0, s["dst_off"] + r * s["dst_stride"] + s["dst"].long(), p[r, w].index_select(0, s["sidx"].long()))
    assert _same(got, exp)


def test_restatements_on_the_tables_of_nas_prep_tables():
    """the numbers tests/test_nas_host_logic.py computes with its numpy restatement of the four kernels, from prep_ref's"""
    from mobilesuperresolution_amd import packing as P
    from mobilesuperresolution_amd.models.wdsr_b import _body_kinds
    f, nb, wgs = 24, 3, 3
    rng = np.random.default_rng(0)
    layout, off = [], 0
    for name, shape in _body_kinds(f):
        n = nb * int(np.prod(shape))
        layout.append((name, off, n, (nb,) + tuple(shape)))
        off += n
    flat = torch.from_numpy(rng.standard_normal(off).astype(np.float32)).double()
    t = P.nas_prep_tables(f, nb, tuple(layout))
    base, size, ds = P.nas_tables(f), t["size"], t["ds"]
    tt = {k: torch.from_numpy(np.asarray(t[k])) for k in ("chan_tab", "bias_tab", "chan_bwd", "bias_bwd", "pw_sidx", "pw_dst", "dw_sidx", "dw_dst")}
    src = R.wn_forward(flat, torch.zeros(nb * size, dtype=torch.float64), tt["chan_tab"], tt["bias_tab"], torch.zeros(len(tt["bias_tab"])))
    exp = np.zeros(nb * size)
    fl = flat.numpy()
    for v_off, g_off, k, dst in t["chan_tab"]:
        exp[dst:dst + k] = fl[v_off:v_off + k] * (fl[g_off] / np.sqrt((fl[v_off:v_off + k] ** 2).sum()))
    for a, b, dst in t["bias_tab"]:
        exp[dst] = fl[a]
    np.testing.assert_allclose(src.numpy(), exp, rtol=1e-13, atol=0)
    # the operand gathers: every index table of the supernet body, as one launch of three segments
    segs = [dict(idx=torch.from_numpy(np.asarray(base[k])).int().reshape(-1), src_off=0, src_stride=size, n=int(np.asarray(base[k]).size),
                 reps=nb, as_float=int(k != "frags")) for k in ("dwp", "frags", "tabs")]
    for s, blob in zip(segs, R.pack(src.float(), segs, torch.bfloat16)):
        e = src.float().view(nb, size)[:, s["idx"].long()].reshape(-1)
        assert torch.equal(blob, e if s["as_float"] else e.bfloat16())
    part_pw = torch.from_numpy(rng.standard_normal((nb, wgs, base["pw_slab"])).astype(np.float32))
    part_dw = torch.from_numpy(rng.standard_normal((nb, wgs, base["dw_slab"])).astype(np.float32))
    useg = [dict(partial=part_pw.reshape(-1), sidx=tt["pw_sidx"], dst=tt["pw_dst"], dst_off=0, dst_stride=ds, slab=base["pw_slab"], wgs=wgs,
                 n=len(tt["pw_sidx"]), reps=nb),
            dict(partial=part_dw.reshape(-1), sidx=tt["dw_sidx"], dst=tt["dw_dst"], dst_off=0, dst_stride=ds, slab=base["dw_slab"], wgs=wgs,
                 n=len(tt["dw_sidx"]), reps=nb)]
    dsrc = R.unpack(torch.zeros(nb * ds, dtype=torch.float64), useg).view(nb, ds)
    e = torch.zeros(nb, ds, dtype=torch.float64)
    e[:, tt["pw_dst"].long()] = part_pw.double().sum(1)[:, tt["pw_sidx"].long()]
    e[:, tt["dw_dst"].long()] = part_dw.double().sum(1)[:, tt["dw_sidx"].long()]
    assert torch.equal(dsrc, e)
    gflat = R.wn_backward(flat, dsrc.reshape(-1), torch.zeros_like(flat), tt["chan_bwd"], tt["bias_bwd"])
    eg, dflat = np.zeros(off), dsrc.reshape(-1).numpy()
    for v_off, g_off, k, dst in t["chan_bwd"]:
        v, dw = fl[v_off:v_off + k], dflat[dst:dst + k]
        ss, dot = (v * v).sum(), (v * dw).sum()
        eg[v_off:v_off + k] = (fl[g_off] / np.sqrt(ss)) * (dw - v * dot / ss)
        eg[g_off] = dot / np.sqrt(ss)
    for a, b, dst in t["bias_bwd"]:
        eg[a] = dflat[dst]
    np.testing.assert_allclose(gflat.numpy(), eg, rtol=1e-12, atol=1e-14)
    lay = {name: (o_, n_) for name, o_, n_, _ in layout}
    for name in ("alpha", "beta", "alpha1", "alpha2", "split.weight"):
        assert not bool(gflat[lay[name][0]:lay[name][0] + lay[name][1]].any())


@pytest.mark.parametrize("nb,f", R.MASK_CASES[:4])
def test_mask_gradient_reference_equals_autograd(nb, f):
    """The block's output is y = mg yin + beta2 ms sum_k p_k relu(pw_k(..)) (models/wdsr_b.py, _NasBlockFunction and the gate of
    MyAggregationLayer.forward); contracted with the upstream gradient, the activations held fixed, it is linear in each of mg, ms,
    p and beta with the block kernels' sums r, sxy, sA, sB as coefficients.  Autograd of that form against mask_grads()."""
    c = R.mask_case(nb, f)
    d = c["dsrc"].view(nb, c["ds"])
    off_r, off_sxy, off_sa, off_sb = c["off"]
    r, sxy = d[:, off_r:off_r + 3 * f].reshape(nb, 3, f), d[:, off_sxy]
    sa, sb = d[:, off_sa:off_sa + f], d[:, off_sb:off_sb + f]
    ms, p, beta = (c[k].clone().requires_grad_(True) for k in ("ms", "p", "beta"))
    mg = torch.ones(f, dtype=torch.float64, requires_grad=True)
    q = (r * ms.view(nb, 1, f)).sum(2)
    loss = ((beta[:, 0] + beta[:, 1]) * sxy).sum() + (beta[:, 1] * (p * q).sum(1)).sum() + (ms * sa).sum() + (mg.view(1, f) * sb).sum()
    loss.backward()
    exp = torch.cat([p.grad.reshape(-1), beta.grad.reshape(-1), ms.grad.reshape(-1), mg.grad])
    assert rel_max(R.mask_expected(c), exp) <= 1e-14


def test_loss_reference_rounds_the_float64_product_once():
    for n in R.LOSS_SIZES:
        part = R.loss_case(n)
        for s in R.LOSS_SCALES.values():
            assert float(torch.tensor(s, dtype=torch.float32)) == s
            got = R.loss_value(part, s)
            assert got.dtype == torch.float32 and float(got) == float(np.float32(float(part.sum()) * s))
            assert float(got) == float(part.float().sum() * torch.tensor(s, dtype=torch.float32))      # the kernels' fp32 product


# ---- the exact cases and their conditions ----------------------------------------------------------------------------------------
def test_check_exact_accepts_every_shipped_case():
    cases = [R.pack_case(i) for i in R.PACK_CASES] + [R.grads_case(i) for i in R.GRADS_CASES]
    for case in cases + [R.mask_case(nb, f) for nb, f in R.MASK_CASES] + [R.loss_case(n) for n in R.LOSS_SIZES]:
        R.check_exact(case)


def test_shipped_cases_cover_the_edges():
    ks = {k for t in R.TABLES for k in t[0]}
    assert ks >= {9, 25, 27, 49, 63, 64, 65, 216, 288}
    assert {t[1] for t in R.TABLES} >= {1, 3, 4, 5, 9} and {t[2] for t in R.TABLES} >= {0, 1, 255, 256, 257}
    assert {t[3] for t in R.TABLES} >= {0, 30, -30}
    segs = [s for c in R.PACK_SEGS for s in c]
    assert {s[0] for s in segs} >= {1, 255, 256, 257, 513} and {s[1] for s in segs} == {1, 3}
    assert {len(c) for c in R.PACK_SEGS} == {1, 2, 3, 4} and any(len({s[2] for s in c}) == 2 for c in R.PACK_SEGS)
    assert any(R.pack_case(i)["table"]["src_off"] > 0 for i in R.PACK_CASES)
    assert all(s["src_stride"] > R.pack_case(i)["table"]["row"] for i in R.PACK_CASES for s in R.pack_case(i)["segs"])
    us = [s for c in R.UNPACK_SEGS for s in c]
    assert {s[0] for s in us} >= {1, 15, 16, 17, 49, 64, 65, 240, 241, 256, 257, 300}
    assert {s[1] for s in us} >= {1, 63, 64, 65, 255, 256, 257} and {s[2] for s in us} == {1, 3} and {s[3] for s in us} == {0, 1}
    assert {len(c) for c in R.UNPACK_SEGS} == {1, 2, 3, 4}
    assert any({R.unpack_j(s[0]) for s in c} == {1, 4} for c in R.UNPACK_SEGS)
    for i in R.GRADS_CASES:
        for s in R.grads_case(i)["segs"]:
            assert s["slab"] > s["n"]
            if s["n"] > 1:                                               # permuted and not contiguous
                assert not torch.equal(s["sidx"], s["sidx"].sort().values)
                assert not torch.equal(s["sidx"].sort().values, torch.arange(s["n"], dtype=torch.int32))
    assert any(bool((R.grads_case(i)["dnamed"][:R.grads_case(i)["table"]["dw"].numel()]).any()) for i in R.GRADS_CASES)   # chained
    # every table row is written once, nothing overlaps
    for i in R.PACK_CASES:
        t = R.pack_case(i)["table"]
        assert int(t["named"].sum()) == int(t["chan_tab"][:, 2].sum()) + len(t["bias_tab"])
        assert int(t["gnamed"].sum()) == int(t["chan_tab"][:, 2].sum()) + len(t["chan_tab"]) + len(t["bias_tab"]) + int((t["bias_tab"][:, 1] >= 0).sum())


def _spoiled_table(edit):
    t = copy.deepcopy(R.grads_case(1)["table"])
    edit(t)
    return t


def test_check_exact_rejects_spoiled_cases():
    v_off, g_off, k, dst = R.grads_case(1)["table"]["chan_tab"][0].tolist()

    def non_integer_norm(t):
        nz = (t["flat"][v_off:v_off + k] != 0).nonzero()[0, 0]
        t["flat"][v_off + nz] += 1.0

    def too_large(t):
        t["flat"][v_off:v_off + k] *= 3.0                                  # |v|^2 passes 2^24 quanta of the row's lattice ...
        t["flat"][v_off] += 2.0 ** -13                                     # ... once one entry lies on a much finer lattice

    for edit in (non_integer_norm, too_large):
        with pytest.raises(ValueError):
            R.check_table(_spoiled_table(edit))
    seg = copy.deepcopy(R.grads_case(2)["segs"][0])
    R.check_slabs(seg)
    p = seg["partial"].view(seg["reps"], seg["wgs"], seg["slab"])
    col = int(seg["sidx"][0])
    spoiled = dict(seg, partial=p.clone().reshape(-1))
    spoiled["partial"].view_as(p)[0, 1, col] = p[0, 0, col]
    with pytest.raises(ValueError, match="two equal slabs"):
        R.check_slabs(spoiled)
    spoiled = dict(seg, partial=p.clone().reshape(-1))
    spoiled["partial"].view_as(p)[0, 0, col] = 2.0 ** 24 * float(R.K.lowbit(p[0, :, col]).min())
    with pytest.raises(ValueError, match="quanta"):
        R.check_slabs(spoiled)
    part = R.loss_case(65).clone()
    part[3] = 2.0 ** 24 * 2.0 ** -6
    with pytest.raises(ValueError, match="quanta"):
        R.check_loss(part)
    c = copy.deepcopy(R.mask_case(3, 24))
    c["dsrc"][c["off"][3]] = 2.0 ** 30 + 0.25                               # an sB term
    with pytest.raises(ValueError):
        R.check_mask(c)


# ---- the shipped cases can fail --------------------------------------------------------------------------------------------------
def _pack_shows(defect):
    for i in R.PACK_CASES:
        case = R.pack_case(i)
        (s0, b0), (s1, b1) = R.pack_expected(case, torch.bfloat16), R.pack_expected(case, torch.bfloat16, defect)
        named = case["table"]["named"]
        if not _same(s0[named], s1[named]) or any(not _same(a, b) for a, b in zip(b0, b1)):
            return True
    return False


def _grads_show(defect):
    for i in R.GRADS_CASES:
        case = R.grads_case(i)
        (d0, g0), (d1, g1) = R.grads_expected(case), R.grads_expected(case, defect)
        if not _same(d0[case["dnamed"]], d1[case["dnamed"]]) or not _same(g0, g1):
            return True
    return False


@pytest.mark.parametrize("defect", ["src_b", "bias_const", "last_element", "block0", "truncate"])
def test_pack_cases_detect_seeded_defect(defect):
    assert _pack_shows(defect)
    assert not _pack_shows(None)


@pytest.mark.parametrize("defect", ["drop_last_slab", "slab0_twice", "src_b", "last_element", "block0", "dot_ss"])
def test_grads_cases_detect_seeded_defect(defect):
    assert _grads_show(defect)
    assert not _grads_show(None)


def test_every_case_with_the_path_detects_its_defect():
    """not one lucky case: every segment shows a dropped or doubled slab, every case of two or more segments a wrong block0, every
    case with bf16 ties the truncation"""
    for i in R.GRADS_CASES:
        case = R.grads_case(i)
        d0 = R.grads_expected(case)[0]
        for defect in ("drop_last_slab", "slab0_twice", "last_element") + (("block0",) if len(case["segs"]) > 1 else ()):
            assert not _same(d0[case["dnamed"]], R.grads_expected(case, defect)[0][case["dnamed"]]), (i, defect)
    for i in R.PACK_CASES:
        case = R.pack_case(i)
        b0 = R.pack_expected(case, torch.bfloat16)[1]
        if len(case["table"]["bias_tab"]) >= 4 and any(not s["as_float"] for s in case["segs"]):
            assert any(not _same(a, b) for a, b in zip(b0, R.pack_expected(case, torch.bfloat16, "truncate")[1])), i
