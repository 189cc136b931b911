"""NAS block parity: the supernet block kernels (csrc/nas_block.h, csrc/nas_dw_lc.h, csrc/nas_bwd_fused.h), driven through
_NasBlockFunction / _NasBodyFunction with effective weights, against tests/nas_ref.py (plain torch, float64, CPU): output and
all eleven gradients, F = 24 and 32, fp32 and bf16.

  exact cases    dyadic data on which the kernels must return the reference bit for bit whatever their summation order and
                 rounding points (conditions: tests/nas_ref.py, verified on the host by tests/test_nas_ref_host.py) -- every
                 geometry at the edges of the 12 x 24 tile, the 3-pixel halo, the 12-column half-row unit and the pixel pairs;
                 every mask / branch-weight / gate corner; and the persistent tile loop of the backward kernels (SR_NAS_WGS
                 below, at and above the number of tiles; 260 tiles at the default 256 workgroups; the body's switch between
                 the fused and the separate backward)
  rounded cases  random normal data; per tensor, max |got - ref| / max |ref| within 8 x (fp32) or 4 x (bf16) the same metric
                 of a CPU emulation of the kernels' precision (+ 1e-6 in fp32); the ratio to that yardstick is printed for
                 every tensor and DESIGN.md keeps the table
"""
import pytest
import torch

from tests import nas_ref as R
from tests.parity_kit import hold_exact, hold_rounded

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
NAMES = ("y",) + R.GRAD_NAMES


def _run(case, dtype, split=None):
    """forward and backward of a case on the device: (y, gyin, the ten parameter gradients)"""
    from mobilesuperresolution_amd.models.wdsr_b import _NasBlockFunction, _NasBodyFunction
    dt = DTYPES[dtype]
    yin = case["yin"].to(dt).cuda().requires_grad_(True)
    params = [case[k].cuda().requires_grad_(True) for k in R.PARAM_NAMES]
    if case["wdw3"].dim() == 5:
        y = _NasBodyFunction.apply(yin, *params, split)
    else:
        y = _NasBlockFunction.apply(yin, *params)
    y.backward(case["gy"].to(dt).cuda())
    return [y.detach().cpu(), yin.grad.cpu()] + [p.grad.cpu() for p in params]


def _hold_exact(tag, got, ref):
    y, grads = ref
    hold_exact(tag, zip(NAMES, got, [y] + grads))


def _exact(f, dtype, geom, masks="all", p=R.P_MIX, beta=(0.0, 1.0), density=1.0):
    case = R.exact_case(f, *geom, masks, p, beta, 0, density)
    _hold_exact((f, dtype, geom, masks, p, beta), _run(case, dtype), case["ref"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=lambda g: "%dx%dx%d" % g)
def test_exact_geometries(geom, f, dtype):
    """images inside the 7 x 7 window, one tile exactly / one under / one-pixel slivers, widths around the 12-column unit,
    3 x 3 tiles with an interior tile, a batch of three; all channels on, then random masks"""
    _exact(f, dtype, geom, "all", R.P_MIX)
    _exact(f, dtype, geom, "random", (1.0, 0.0, 0.0))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("geom", R.CORNER_GEOMETRIES, ids=lambda g: "%dx%dx%d" % g)
@pytest.mark.parametrize("corner", R.CORNERS, ids=lambda c: "%s-p%s-beta%s" % (c[0], "".join("%g" % (4 * v) for v in c[1]), "%g%g" % c[2]))
def test_exact_mask_and_gate_corners(corner, geom, f, dtype):
    """all on, random masks, ms = 0, mg = 0, one live channel (the first; the last, next to the padding to 32), each one-hot p,
    the closed gate"""
    masks, p, beta = corner
    _exact(f, dtype, geom, masks, p, beta)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("wgs", [1, 5, 12, 13, None])
def test_tile_loop_workgroup_counts(monkeypatch, wgs, f, dtype):
    """12 tiles on 1, 5, 12, 13 and 256 workgroups: twelve trips, uneven trips, one trip each, an idle workgroup; the slabs of
    every count sum to the reference, bit for bit"""
    assert R.n_tiles(*R.TILE_LOOP_GEOMETRY) == 12
    if wgs is None:
        monkeypatch.delenv("SR_NAS_WGS", raising=False)
    else:
        monkeypatch.setenv("SR_NAS_WGS", str(wgs))
    _exact(f, dtype, R.TILE_LOOP_GEOMETRY, "random", R.P_MIX)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [24, 32])
def test_tile_loop_at_the_production_default(monkeypatch, f, dtype):
    """260 tiles on the default 256 workgroups: four workgroups take a second tile"""
    monkeypatch.delenv("SR_NAS_WGS", raising=False)
    m = R.MANY_TILES
    assert R.n_tiles(m["n"], m["h"], m["w"]) == 260
    _exact(f, dtype, (m["n"], m["h"], m["w"]), m["masks"], m["p"], (0.0, 1.0), m["gy_density"])


@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("split", [(0, 0), (1, 1)], ids=["fused", "split"])
@pytest.mark.parametrize("geom", [R.BODY_FUSED, R.BODY_SEPARATE], ids=["8tiles", "9tiles"])
def test_body_backward_route_switch(monkeypatch, geom, split, f):
    """three blocks, bf16, SR_NAS_WGS = 8: 8 tiles take the fused backward (one tile per workgroup), 9 tiles the separate
    kernels with a second trip; with and without the split flags: all four equal the reference"""
    monkeypatch.setenv("SR_NAS_WGS", "8")
    assert R.n_tiles(*geom) == (8 if geom == R.BODY_FUSED else 9)
    case = R.exact_body_case(f, *geom)
    _hold_exact((f, geom, split), _run(case, "bf16", split), case["ref"])


@pytest.mark.parametrize("f", [24, 32])
def test_body_fp32_matches_reference(monkeypatch, f):
    """the stacked form in the fp32 parity mode (generic kernels, two trips)"""
    monkeypatch.setenv("SR_NAS_WGS", "5")
    case = R.exact_body_case(f, *R.BODY_SEPARATE)
    _hold_exact((f, "fp32 body"), _run(case, "fp32", (0, 0)), case["ref"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("f", [24, 32])
@pytest.mark.parametrize("geom", R.ROUNDED_GEOMETRIES, ids=lambda g: "%dx%dx%d" % g)
def test_rounded(geom, f, dtype):
    case, (y, grads), yard = R.rounded_reference(f, *geom, dtype)
    got = _run(case, dtype)
    hold_rounded("nas block parity", f"F={f} {dtype} {geom[0]}x{geom[1]}x{geom[2]}", dtype, zip(NAMES, got, [y] + grads, yard))
