"""packing.resize_axis, the one definition of the sized upsampler kernels' resize arithmetic, and the route rule of `hot_resize`, on
the CPU and without the library: the tables' identities, the adjoint (gather) form against the transposed dense matrix, the tables'
accuracy against ATen's own fp32 and float64 F.interpolate, and which reason each route gives with the flag on and off."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mobilesuperresolution_amd import packing as P
from mobilesuperresolution_amd.models import loss_fold as LF
from tests import frame_resize_ref as Z

AXES = [(37, 41), (37, 36), (37, 20), (37, 111), (37, 5), (37, 37), (37, 1), (69, 77), (69, 68), (69, 31), (69, 207), (69, 7), (69, 69),
        (69, 1), (1, 1), (1, 9), (5, 4), (5, 32768), (961, 1080), (1705, 1920)]


@pytest.mark.parametrize("n_in, n_out", AXES, ids=lambda v: str(v))
def test_identities(n_in, n_out):
    ax = P.resize_axis(n_in, n_out)
    assert ax.i0.dtype == ax.i1.dtype == ax.lo.dtype == ax.hi.dtype == np.int32 and ax.lam.dtype == np.float32
    assert ax.i0.shape == ax.i1.shape == ax.lam.shape == (n_out,) and ax.lo.shape == ax.hi.shape == (n_in,)
    assert bool((np.diff(ax.i0) >= 0).all()) and ax.i0.min() >= 0 and ax.i0.max() <= n_in - 1
    assert bool((ax.i1 == np.minimum(ax.i0 + 1, n_in - 1)).all())
    assert bool((ax.lam >= 0).all()) and bool((ax.lam <= 1).all())
    # the ranges partition the outputs: consecutive, none lost, each holding exactly the outputs with i0 == i
    assert ax.lo[0] == 0 and ax.hi[-1] == n_out - 1 and bool((ax.lo[1:] == ax.hi[:-1] + 1).all()) and bool((ax.hi >= ax.lo - 1).all())
    for i in range(n_in):
        assert bool((ax.i0[ax.lo[i]:ax.hi[i] + 1] == i).all())
    assert int((ax.hi - ax.lo + 1).sum()) == n_out
    if n_out == n_in:
        assert bool((ax.i0 == np.arange(n_in)).all()) and not ax.lam.any()
    assert not any(a.flags.writeable for a in ax)
    ti, tf = P.fn_resize_tables(n_in, n_out)
    assert ti.dtype == np.int32 and tf.dtype == np.float32 and ti.shape == (n_out + 2 * n_in,)
    assert np.array_equal(ti, np.concatenate([ax.i0, ax.lo, ax.hi])) and np.array_equal(tf, ax.lam)


def test_bad_sizes_raise():
    for n_in, n_out in ((0, 4), (4, 0), (-1, 3)):
        with pytest.raises(ValueError):
            P.resize_axis(n_in, n_out)


@pytest.mark.parametrize("n_in, n_out", [a for a in AXES if a[1] <= 2000], ids=lambda v: str(v))
def test_adjoint_ranges_give_the_transposed_matrix(n_in, n_out):
    assert np.array_equal(Z.dense(n_in, n_out).T, Z.dense_adjoint(n_in, n_out))


SIZES = [((37, 69), (41, 77)), ((37, 69), (36, 68)), ((37, 69), (20, 31)), ((37, 69), (111, 207)), ((37, 69), (5, 7)),
         ((961, 1705), (1080, 1920)), ((37, 69), (37, 69)), ((37, 69), (1, 1))]


@pytest.mark.parametrize("n_in, n_out", SIZES, ids=lambda v: "{}x{}".format(*v))
def test_tables_are_as_close_to_float64_aten_as_fp32_aten_is(n_in, n_out):
    """absolute errors (max |difference|): the tables' blend done in float64 against F.interpolate in float64, and ATen's own fp32
    F.interpolate against the same.  Both carry an fp32 weight and differ only in where src is rounded, hence the factor 2; `<=` so
    that the two exact sizes (identity: every lam 0; 1 x 1: a single sample of D) pass at 0."""
    x = torch.rand(2, 3, *n_in, generator=torch.Generator().manual_seed(5), dtype=torch.float64).float()
    ref = F.interpolate(x.double(), size=n_out, mode="bilinear")
    aten = (F.interpolate(x, size=n_out, mode="bilinear").double() - ref).abs().max().item()
    ours = (Z.blend(x, n_out) - ref).abs().max().item()
    print(f"resize tables | {n_in} -> {n_out} | tables {ours:.3e} | fp32 ATen {aten:.3e} | ratio {ours / aten if aten else float('nan'):.2f}")
    assert ours <= 2 * aten
    if n_out in ((37, 69), (1, 1)):
        assert ours == 0.0 and aten == 0.0


# ---- the route rule ---------------------------------------------------------------------------------------------------------------
def _model(**attrs):
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    m = Result_Model(4, 8, 1, 3)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _device_clip():
    """what the route rule reads of a (1, 2, 3, 9, 17) clip that sits where the parameters are and calls itself a device tensor"""
    return types.SimpleNamespace(dim=lambda: 5, shape=(1, 2, 3, 9, 17), is_cuda=True, device=torch.device("cpu"), requires_grad=False,
                                 numel=lambda: 1)


def test_route_reasons_with_the_flag_on_and_off():
    from mobilesuperresolution_amd.models.single_image_model import Result_Model
    assert Result_Model.hot_resize is False
    x = torch.zeros(1, 2, 3, 9, 17)
    off, on = _model(hot_training=True), _model(hot_training=True, hot_resize=True)
    # flag off: today's reasons, word for word (the CPU check comes before the size check)
    assert off.train_route_reason(x, 41, 77) == "CPU input" and off.hot_route_reason(x, 41, 77) == "the call records an autograd graph"
    assert _model().train_route_reason(x, 41, 77) == "hot_training is not set"
    assert _model(hot_resize=True).train_route_reason(x, 41, 77) == "hot_training is not set"
    # past the device check: a stand-in for a device clip (`is_cuda` and `device` are what the rule reads)
    dev = _device_clip()
    assert off.train_route_reason(dev, 41, 77) == "output size is not (4H, 4W)"
    assert on.train_route_reason(dev, 41, 77) is None and on.train_route_reason(dev, 36, 68) is None
    assert off.train_route_reason(dev, 36, 68) is None
    # flag on: the size check is gone, the next failing check speaks
    assert on.train_route_reason(x, 41, 77) == "CPU input"
    # beyond the tables: refused by both routes with the flag on; the x4 size is never "beyond"
    big = P.FN_MAX_OUT + 1
    assert "beyond the sized kernels' tables" in on.train_route_reason(dev, big, 77)
    assert "beyond the sized kernels' tables" in on.train_route_reason(dev, 41, big)
    assert on.train_route_reason(dev, P.FN_MAX_OUT, P.FN_MAX_OUT) is None
    assert on.train_route_reason(dev, 0, 77) == "empty input or output" and on.train_route_reason(dev, 41, -1) == "empty input or output"
    with torch.no_grad():
        assert "beyond the sized kernels' tables" in on.hot_route_reason(dev, big, 77)
        assert on.hot_route_reason(dev, 41, 77) is None and off.hot_route_reason(dev, big, 77) is None


def test_train_step_keeps_its_size_reason():
    from mobilesuperresolution_amd import training as TR
    x = torch.zeros(1, 2, 3, 9, 17)
    for m in (_model(hot_resize=True, hot_training=True), _model()):
        trained = [p for mod in (m.encoder, m.body, m.shuf) for p in mod.parameters()]
        opt = TR.Adam(trained, lr=1e-3)
        assert m.train_step_reason(x, torch.zeros(1, 2, 3, 41, 77), opt) == "hr is not fp32 (B, N, 3, 4H, 4W) on the input's device"
        # the route rule under train_step keeps the (4H, 4W) reason whatever the flag says
        dev = _device_clip()
        assert m._route_reason(dev, True, trained=trained, out_size=(41, 77), opt_in=True) == "output size is not (4H, 4W)"
        assert m._route_reason(dev, True, trained=trained, out_size=(36, 68), opt_in=True) is None


def test_can_fold_declines_a_node_that_is_not_foldable():
    sr, hr = torch.zeros(1, 2, 3, 41, 77), torch.ones(1, 2, 3, 41, 77)
    node = lambda **kw: types.SimpleNamespace(**{**dict(folded=None, fold_started=False, ran=False, out_ptr=sr.data_ptr()), **kw})
    assert LF.can_fold(node(), sr, hr) is True and LF.can_fold(node(foldable=True), sr, hr) is True
    assert not LF.can_fold(node(foldable=False), sr, hr)


def test_tables_do_not_travel_with_a_pickle():
    m = _model(hot_resize=True)
    m._fn_resize = {("cpu", 9, 17, 41, 77): object()}
    assert "_fn_resize" not in m.__getstate__()
