"""The host side of MotionVectorVSR's HIP reconstruction backward at 24 < F <= 64 (csrc/mv_recon.h: mv_recon_bwd64_kernel):
packing.mv_recon_bwd_tables against a direct restatement, the forward's tables pinned to what they were before this backward
existed, and the route rule of `MotionVectorVSR.hot_training`.  No GPU."""
import hashlib

import numpy as np
import pytest
import torch

WIDTHS = (25, 40, 64)


def _src_layout(f):
    f2 = 2 * f
    return dict(wfu=0, bfu=f2 * f2, wl=f2 * f2 + f2, bl=f2 * f2 + f2 + f2 * 75, zero=f2 * f2 + f2 + f2 * 75 + 3)


def _restated_pack(f):
    """wlb | wfut element by element: fragment (m, s), lane l, element j = A[16 m + (l & 15)][32 s + 8 (l >> 4) + j]"""
    o, f2 = _src_layout(f), 2 * f
    out = []
    for m in range(8):                                   # wlb: A[uc][r] = conv_last.weight[uc, r]
        for s in range(3):
            for l in range(64):
                for j in range(8):
                    uc, r = 16 * m + (l & 15), 32 * s + 8 * (l >> 4) + j
                    out.append(o["wl"] + uc * 75 + r if (uc < f2 and r < 75) else o["zero"])
    for m in range(8):                                   # wfut: A[kc][oc] = fusion.weight[oc, c(kc)]
        for s in range(4):
            for l in range(64):
                for j in range(8):
                    kc, oc = 16 * m + (l & 15), 32 * s + 8 * (l >> 4) + j
                    c = kc if kc < f else (f + kc - 64 if 64 <= kc < 64 + f else None)
                    out.append(o["wfu"] + oc * f2 + c if (c is not None and oc < f2) else o["zero"])
    return np.array(out, dtype=np.int64)


def _restated_reduce(f):
    f2 = 2 * f
    wl, wfu, bfu, bl = 0, 128 * 80, 128 * 80 + 128 * 128, 128 * 80 + 128 * 128 + 128
    out = [wfu + oc * 128 + (ic if ic < f else 64 + ic - f) for oc in range(f2) for ic in range(f2)]
    out += [bfu + oc for oc in range(f2)]
    out += [wl + uc * 80 + r for uc in range(f2) for r in range(75)]
    out += [bl + o for o in range(3)]
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("f", WIDTHS)
def test_backward_tables_match_a_direct_restatement(f):
    from mobilesuperresolution_amd import packing as P
    t = P.mv_recon_bwd_tables(f)
    assert t["pack"].dtype == np.int64 and t["reduce"].dtype == np.int64
    assert np.array_equal(t["pack"], _restated_pack(f))
    assert np.array_equal(t["reduce"], _restated_reduce(f))
    assert (t["wlb"], t["wfut"], t["pack"].size) == (0, 8 * 3 * 512, 8 * 3 * 512 + 8 * 4 * 512)
    assert t["slab"] == 128 * 80 + 128 * 128 + 128 + 16 and t["zero"] == _src_layout(f)["zero"] and t["size"] == t["zero"] + 1


@pytest.mark.parametrize("f", WIDTHS)
def test_every_index_points_at_a_real_element_or_the_zero_slot(f):
    """pack: each real weight exactly once per table, everything else the zero slot, no bias; reduce: inside the slab, no element
    twice, only rows < 2F of both matrices, only the 75 real columns of dW_last and the 2F real kernel channels of dW_fu"""
    from mobilesuperresolution_amd import packing as P
    t, o, f2 = P.mv_recon_bwd_tables(f), _src_layout(f), 2 * f
    pack = t["pack"]
    assert pack.min() >= 0 and pack.max() <= o["zero"]
    wlb, wfut = pack[:t["wfut"]], pack[t["wfut"]:]
    for tab, lo, hi in ((wlb, o["wl"], o["bl"]), (wfut, o["wfu"], o["bfu"])):
        real = tab[tab != o["zero"]]
        assert real.min() >= lo and real.max() < hi
        assert np.array_equal(np.sort(real), np.arange(lo, hi))
    red = t["reduce"]
    assert red.size == f2 * f2 + f2 + f2 * 75 + 3 and np.unique(red).size == red.size
    assert red.min() >= 0 and red.max() < t["slab"] - 13          # db_last's three floats, not the slab's padding
    n0, n1, n2 = f2 * f2, f2 * f2 + f2, f2 * f2 + f2 + f2 * 75
    S = P.MV_SLAB64
    row, col = np.divmod(red[:n0] - S["wfu"], 128)
    assert row.max() < f2 and bool(((col < f) | ((col >= 64) & (col < 64 + f))).all())
    assert np.array_equal(red[n0:n1], S["bfu"] + np.arange(f2))
    row, col = np.divmod(red[n1:n2] - S["wl"], 80)
    assert row.max() < f2 and col.max() == 74
    assert np.array_equal(red[n2:], S["bl"] + np.arange(3))


def test_backward_tables_refuse_other_widths():
    from mobilesuperresolution_amd import packing as P
    for f in (0, 24, 65):
        with pytest.raises(ValueError):
            P.mv_recon_bwd_tables(f)


# sha256 of mv_recon_tables(f, 64)["pack"] (int64, native byte order) on the commit before mv_recon_bwd_tables was added
_FWD_PACK_SHA256 = {25: "3cbbe2a0d5e8ccf6ce988e87a48199ee2c4a2d1580ab1011f695a6989efbc8bc",
                    40: "7c117089059d096ac3c3ed9b1f231611fa98c1acb87099568daab4d5f5ff898e",
                    43: "928e71b05e9c16f3f17ebd4a31df33976f72e3a6a5778073606d068a7037e5ab",
                    64: "111e15b2e4a7962fc2205b31f1bacf8e6afc396e56e2a1a6103e63bfb6c953b3"}
_GEOM64 = {'kp': 128, 'ks': 4, 'mb': 8, 'wfu': 0, 'bfu': 16384, 'wl': 16512, 'bl': 26752, 'fwd_elems': 26760, 'wlb': 26760,
           'wfut': 39048, 'all_elems': 55432}
_GEOM24 = {'kp': 64, 'ks': 2, 'mb': 4, 'wfu': 0, 'bfu': 4096, 'wl': 4160, 'bl': 9280, 'fwd_elems': 9288, 'wlb': 9288, 'wfut': 15432,
           'all_elems': 19528}


@pytest.mark.parametrize("f", sorted(_FWD_PACK_SHA256))
def test_forward_tables_are_what_they_were(f):
    from mobilesuperresolution_amd import packing as P
    t = P.mv_recon_tables(f, 64)
    assert t["pack"].dtype == np.int64 and t["pack"].size == 26760
    assert hashlib.sha256(np.ascontiguousarray(t["pack"]).tobytes()).hexdigest() == _FWD_PACK_SHA256[f]
    assert P.mv_recon_geom(64) == _GEOM64 and P.mv_recon_geom(24) == _GEOM24 and t["geom"] == _GEOM64


# ---- the route rule ------------------------------------------------------------------------------------------------------------
def _model(f, nb=1):
    from mobilesuperresolution_amd.models import MotionVectorVSR
    return MotionVectorVSR(f, nb, hot_dtype="fp32")


def test_hot_training_is_off_by_default():
    from mobilesuperresolution_amd.models import MotionVectorVSR
    assert MotionVectorVSR.hot_training is False
    m = _model(40)
    assert m.hot_training is False and not m.backward_trunk.hot_training and not m.forward_trunk.hot_training
    assert m._graph_route_hot() is False                 # the wide trunks refuse a graph-recording call themselves


def test_hot_training_opts_the_wide_trunks_in_and_out():
    m = _model(40)
    m.hot_training = True
    assert m.hot_training is True and m.backward_trunk.hot_training and m.forward_trunk.hot_training
    assert m._graph_route_hot() is True
    m.hot_training = False
    assert m.hot_training is False and not m.backward_trunk.hot_training and not m.forward_trunk.hot_training
    assert m._graph_route_hot() is False
    assert type(m).hot_training is False                 # the class default is untouched
    assert "hot_training" not in m.state_dict()


def test_hot_training_changes_nothing_at_24_features():
    for on in (False, True):
        m = _model(20)
        m.hot_training = on
        assert not m.backward_trunk.wide and not m.backward_trunk.hot_training and not m.forward_trunk.hot_training
        assert m._graph_route_hot() is True              # the 24-wide route trains in HIP either way


def test_set_wide_training_alone_keeps_the_aten_reconstruction():
    from mobilesuperresolution_amd.models import set_wide_training
    m = _model(64)
    assert len(set_wide_training(m)) == 2
    assert m.backward_trunk.hot_training and m.forward_trunk.hot_training and m.hot_training is False
    assert m._graph_route_hot() is False
    m.hot_training = True
    set_wide_training(m, False)                          # the trunks opted out again: they refuse, the reconstruction follows
    assert m._graph_route_hot() is False


def test_separate_directions_keep_the_aten_reconstruction(monkeypatch):
    m24, m40 = _model(20), _model(40)
    m40.hot_training = True
    monkeypatch.setenv("SR_VSR_SEPARATE_DIRECTIONS", "1")
    assert m24._graph_route_hot() is False and m40._graph_route_hot() is False
    monkeypatch.setenv("SR_VSR_SEPARATE_DIRECTIONS", "0")
    assert m24._graph_route_hot() is True and m40._graph_route_hot() is True


def test_hooks_and_the_switch_keep_the_aten_reconstruction():
    """tensors aside: a CPU call never takes the HIP route, so the conditions are read one by one"""
    m = _model(40)
    m.hot_training = True
    x = torch.zeros(1, 2, 5, 4, 4)
    assert m._hot_reconstruction(x, 16, 16) is False     # CPU tensors
    assert not m._hooked()
    h = m.fusion.register_forward_hook(lambda *a: None)
    assert m._hooked()
    h.remove()
    h = m.forward_trunk.register_forward_hook(lambda *a: None)
    assert m._hooked()
    h.remove()
    assert not m._hooked()
