"""tests/warp_ref.py, the float64 warp that the HIP warp kernels are held against (tests/test_gpu_warp.py), pinned before
anything is compared with it: against float64 F.grid_sample under the reference's normalisation on every input class of the
GPU tests, and against fixture G8 of the reference's own flow_warp."""
import os

import numpy as np
import pytest
import torch

from tests import warp_ref as WR


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("name", sorted(WR.STANDALONE_CASES))
def test_warp_ref_equals_float64_grid_sample(name):
    x, flow, dy = WR.standalone_case(name)
    got = WR.warp_ref_grads(x, flow, dy)
    exp = WR.warp_ref_grads(x, flow, dy, fn=WR.grid_sample_warp)
    n, c, h, w = x.shape
    exact = "dyadic" in name or name.startswith("shift")            # the normalisation is exact where size - 1 is a power of two
    for what, a, b in zip(("y", "dx", "dflow"), got, exp):
        e = _rel(a, b)
        print(f"{name} {what}: rel max-abs vs float64 grid_sample {e:.1e}")
        if exact and what != "dflow":                                # same cells, same weights: bit for bit
            assert torch.equal(a, b), (name, what)
        else:                                                        # dflow: grid_sample adds its tap terms in another order
            assert e <= 1e-12, (name, what, e)
    if w == 1:
        assert not got[2][..., 0].any() and not exp[2][..., 0].any()
    if h == 1:
        assert not got[2][..., 1].any() and not exp[2][..., 1].any()


def test_flow_generators_reach_what_they_are_for():
    g = torch.Generator().manual_seed(0)
    f = WR.off_integer_flow((2, 30, 41, 2), 6, gen=g)
    frac = f.double() - f.double().floor()
    assert frac.min() >= 1 / 16 - 1e-6 and frac.max() <= 15 / 16 + 1e-6 and 5 < f.abs().max() <= 6
    assert WR.same_cell(f).all()
    assert not WR.off_integer_flow((1, 4, 4, 2), 0, gen=g).floor().any()
    d = WR.dyadic_flow((1, 9, 17, 2), gen=g)
    assert torch.equal(d * 4, (d * 4).round()) and d.abs().max() <= 4 * 17 and WR.same_cell(d).all()
    x, d, _ = WR.standalone_case("borders-3x9x17-dyadic")
    px = d[0, :, :, 0] + torch.arange(17.0)
    py = d[0, :, :, 1] + torch.arange(9.0).view(9, 1)
    inside = (px > -1) & (px < 17) & (py > -1) & (py < 9)
    assert inside.any() and (~inside).any()                          # samples wholly outside, and samples that are not
    assert ((px == px.floor()) & inside).any()                       # exact landings
    c = WR.converging_flow(12, 40, 17, 0.37)
    assert torch.allclose(c[0, :, :, 0] + torch.arange(40.0), torch.full((12, 40), 17.37))
    # zero flow at a size whose size - 1 is no power of two: the fp32 round trip leaves some integer positions below the integer
    z = WR.same_cell(torch.zeros(1, 30, 41, 2))
    assert not z.all() and z.float().mean() > 0.8


def test_warp_ref_matches_fixture_g8(golden_dir):
    z = np.load(os.path.join(golden_dir, "g8_flow_warp.npz"))
    d = {k: torch.from_numpy(z[k]) for k in z.files}
    got = WR.warp_ref_grads(d["x"], d["flow"], d["dy"])
    # the fixture is the reference's fp32 result: 1.5e-6, 9.2e-7 and 1.2e-6 of the maximum measured, its own rounding
    for what, a, bound in zip(("y", "dx", "dflow"), got, (5e-6, 5e-6, 5e-6)):
        e = ((a - d[what].double()).abs().max() / d[what].abs().max()).item()
        print(f"G8 {what}: warp_ref vs fixture, rel to max {e:.1e}")
        assert e <= bound, (what, e)
