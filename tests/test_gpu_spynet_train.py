"""SpyNet's training route on the GPU (SpyNet.hot_training): the backward-data and weight-gradient kernels of csrc/spynet_conv.h
through sr_conv7_bwd_data / sr_conv7_wgrad / sr_conv7_module_bwd, held per element to the float64 reference of
tests/spynet_bwd_ref.py (bounds derived there: K 2^-24 sum |terms| for an fp32 accumulator of K terms, plus half an ulp of a bf16
store; no literal tolerance), tap-identity cases bit for bit, then the BasicModule chain, the whole network and BasicVSR end to end.

A weight gradient is independent of the workgroup cap only up to its bound (the slabs are summed in another order), not bit for bit:
the cases with caps 5 and 1 are each held to the reference, not to each other.  Two equal calls give equal bits."""
import pytest
import torch

from tests import spynet_bwd_ref as B
from tests.parity_kit import hold_exact

pytestmark = pytest.mark.gpu

_gid = lambda g: "x".join(str(v) for v in g)
LAYER_IDS = ["%dto%d" % l[:2] for l in B.LAYERS]


def _nhwc(t, dtype=torch.bfloat16, pad_to=0):
    t = t.permute(0, 2, 3, 1)
    if pad_to > t.shape[3]:
        t = torch.cat([t, t.new_zeros(t.shape[:3] + (pad_to - t.shape[3],))], 3)
    return t.contiguous().cuda().to(dtype)


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


def _bwd_data(layer, dy, w, act):
    """sr_conv7_bwd_data on one layer, packed as the training route packs it: dx (n, cin, h, w), bf16 (the first layer: fp32)"""
    from mobilesuperresolution_amd import _lib as L, packing as P
    cin, cout, _ = B.LAYERS[layer]
    n, _, h, wd = dy.shape
    idx = torch.from_numpy(P.conv7_bwd_tables(cin, cout)["idx"]).cuda()
    wp = torch.cat([w.float().cuda().reshape(-1), torch.zeros(1, device="cuda")]).index_select(0, idx).to(torch.bfloat16).contiguous()
    dyd, actd = _nhwc(dy, pad_to=8), _nhwc(act)
    dx = torch.full((n, h, wd, cin), float("nan"), dtype=torch.float32 if layer == 0 else torch.bfloat16, device="cuda")
    L.launch("sr_conv7_bwd_data", L.lib().sr_conv7_bwd_data, dyd.data_ptr(), wp.data_ptr(), actd.data_ptr() if layer else None,
             dx.data_ptr(), n, h, wd, cin, cout, L.stream_ptr())
    return _nchw(dx)


def _wgrad(layer, dy, x, cap):
    """sr_conv7_wgrad on one layer: (dW, db, workgroups)"""
    from mobilesuperresolution_amd import _lib as L, packing as P
    cin, cout, _ = B.LAYERS[layer]
    n, _, h, wd = dy.shape
    tab = P.conv7_wgrad_tables(cin, cout)
    wgs = P.conv7_wgrad_wgs(n, h, wd, cap)
    sidx, dst = torch.from_numpy(tab["sidx"]).cuda(), torch.from_numpy(tab["dst"]).cuda()
    part = torch.full((wgs * tab["slab"],), float("nan"), device="cuda")
    gflat = torch.full((cout * cin * 49 + cout,), float("nan"), device="cuda")
    dyd, xd = _nhwc(dy, pad_to=8), _nhwc(x)
    L.launch("sr_conv7_wgrad", L.lib().sr_conv7_wgrad, dyd.data_ptr(), xd.data_ptr(), part.data_ptr(), wgs, sidx.data_ptr(),
             dst.data_ptr(), gflat.data_ptr(), n, h, wd, cin, cout, L.stream_ptr())
    g = gflat.cpu()
    return g[:cout * cin * 49].view(cout, cin, 7, 7), g[cout * cin * 49:], wgs


def _hold(tag, rows):
    """rows: (name, got, float64 reference, per-element bound); prints the worst ratio |got - ref| / bound per row"""
    bad = []
    for name, got, ref, tol in rows:
        err = (got.double() - ref).abs()
        ok = err <= tol
        worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
        print(f"spynet train | {tag} | {name} | max |err| {float(err.max()) if err.numel() else 0.0:.3e} | worst err / bound {worst:.3f}")
        if not bool(ok.all()) or not bool(torch.isfinite(got.float()).all()):
            bad.append((name, int((~ok).sum()), worst))
    assert not bad, (tag, bad)


def test_entries_are_exported_and_refuse_other_shapes():
    from mobilesuperresolution_amd import _lib as L
    lib = L.lib()
    for name in ("sr_conv7_bwd_data", "sr_conv7_wgrad", "sr_conv7_module_bwd"):
        assert hasattr(lib, name)
    buf = torch.full((4096,), 7.0, device="cuda")
    idx = torch.zeros(16, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    assert lib.sr_conv7_bwd_data(p, p, p, p, 1, 1, 1, 24, 24, L.stream_ptr()) == -1
    assert lib.sr_conv7_bwd_data(p, p, None, p, 1, 1, 1, 32, 64, L.stream_ptr()) == -2
    assert lib.sr_conv7_wgrad(p, p, p, 1, idx.data_ptr(), idx.data_ptr(), p, 1, 1, 1, 8, 2, L.stream_ptr()) == -1
    assert lib.sr_conv7_wgrad(p, p, p, 0, idx.data_ptr(), idx.data_ptr(), p, 1, 1, 1, 8, 32, L.stream_ptr()) == -2
    assert lib.sr_conv7_module_bwd(None, 1, 1, 1, 1, L.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


@pytest.mark.parametrize("layer", range(5), ids=LAYER_IDS)
def test_bwd_data_tap_identity(layer):
    """one weight per input channel: dx is a shifted copy of one dy channel times the mask, bit for bit; the sets pin every tap's
    rotation and every channel's swap"""
    bad = []
    for j, case in enumerate(B.tap_cases(layer, *B.TAP_GEOMETRY)):
        got = _bwd_data(layer, case["dy"], case["w"], case["act"])
        exp = case["dx"].to(got.dtype)
        ne = (got != exp) | (got != got)
        for ci in ne.any(0).any(1).any(1).nonzero().flatten().tolist():
            co, ky, kx = case["taps"][ci]
            bad.append(f"case {j} input channel {ci}: tap (ky {ky}, kx {kx}) of output channel {co}: {int(ne[:, ci].sum())} elements differ")
    assert not bad, (bad[:8], len(bad))


@pytest.mark.parametrize("layer", range(5), ids=LAYER_IDS)
@pytest.mark.parametrize("geom", B.GEOMETRIES, ids=_gid)
def test_bwd_data_rounded(geom, layer):
    case = B.rounded_case(layer, *geom)
    ref = B.layer_ref(layer, case["dy"], case["w"], case["x"], 1)
    got = _bwd_data(layer, case["dy"], case["w"], case["x"])
    assert got.dtype == (torch.float32 if layer == 0 else torch.bfloat16)
    _hold("bwd-data %s %s" % (LAYER_IDS[layer], _gid(geom)), [("dx", got, ref["dx"], ref["tol_dx"])])
    if layer:
        assert bool((got[case["x"] <= 0] == 0).all())


@pytest.mark.parametrize("layer", range(5), ids=LAYER_IDS)
@pytest.mark.parametrize("geom", B.WGRAD_CASES, ids=_gid)
def test_wgrad_rounded(geom, layer):
    """every geometry of backward-data, then 18 tiles over 5 workgroups (the tile loop runs more than once per workgroup) and the
    same on a single workgroup; two equal calls give equal bits"""
    n, h, w, cap = geom
    case = B.rounded_case(layer, n, h, w)
    dw, db, wgs = _wgrad(layer, case["dy"], case["x"], cap)
    assert wgs == {5: 5, 1: 1}.get(cap, wgs)
    ref = B.layer_ref(layer, case["dy"], case["w"], case["x"], wgs)
    _hold("wgrad %s %s" % (LAYER_IDS[layer], _gid(geom)), [("dw", dw, ref["dw"], ref["tol_dw"]), ("db", db, ref["db"], ref["tol_db"])])
    dw2, db2, _ = _wgrad(layer, case["dy"], case["x"], cap)
    hold_exact(("wgrad twice", layer, geom), [("dw", dw2, dw), ("db", db2, db)])


def _module(params):
    from mobilesuperresolution_amd.models.spynet_arch import BasicModule
    mod = BasicModule().cuda()
    with torch.no_grad():
        for c, i in zip((mod.basic_module[k] for k in (0, 2, 4, 6, 8)), range(5)):
            c.weight.copy_(params[2 * i])
            c.bias.copy_(params[2 * i + 1])
    return mod


def test_basic_module_chain():
    """BasicModule at (2, 16, 32): the forward value is the inference route's bit for bit; every layer of sr_conv7_module_bwd is
    held to the one-layer reference fed the kernel's own saved activations and the kernel's own incoming gradient, so every
    element has its bound; the autograd.Function returns the same bits as the C call"""
    import ctypes
    from mobilesuperresolution_amd import _lib as L, packing as P
    from mobilesuperresolution_amd.models import spynet_arch as S
    case = B.chain_case(*B.CHAIN_GEOMETRY)
    n, h, w = B.CHAIN_GEOMETRY
    mod = _module(case["params"])
    x = case["x"].cuda().requires_grad_(True)
    with torch.no_grad():
        want = mod(x)
    y = mod.forward_train(x)
    assert y.requires_grad and torch.equal(y, want)
    y.backward(case["dflow"].cuda())
    node_xs = S._conv7_chain(x.detach().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16), mod._pack(x.device), n, h, w, x.device)[:5]
    # the same backward through the C entry with buffers of our own
    tabs = S._bwd_tables(torch.cuda.current_device())
    g = [torch.full((n, h, w, max(co, 8)), float("nan"), dtype=torch.bfloat16, device="cuda") for _, co, _ in B.LAYERS]
    g[4] = _nhwc(case["dflow"], pad_to=8)
    dx0 = torch.full((n, h, w, 8), float("nan"), device="cuda")
    wts = [torch.cat([case["params"][2 * l].cuda().reshape(-1), torch.zeros(1, device="cuda")]).index_select(0, tabs[l][0]).to(torch.bfloat16)
           for l in range(5)]
    gflat = [torch.full((co * ci * 49 + co,), float("nan"), device="cuda") for ci, co, _ in B.LAYERS]
    wgs = P.conv7_wgrad_wgs(n, h, w)
    part = torch.empty(wgs * max(P.conv7_wgrad_tables(ci, co)["slab"] for ci, co, _ in B.LAYERS), device="cuda")
    m = L.Conv7ModuleBwd()
    for l in range(5):
        m.x[l], m.g[l], m.wpacked_t[l] = node_xs[l].data_ptr(), g[l].data_ptr(), wts[l].data_ptr()
        m.sidx[l], m.dst[l], m.gflat[l] = tabs[l][1].data_ptr(), tabs[l][2].data_ptr(), gflat[l].data_ptr()
    m.partial, m.dx0 = part.data_ptr(), dx0.data_ptr()
    L.launch("sr_conv7_module_bwd", L.lib().sr_conv7_module_bwd, ctypes.byref(m), wgs, n, h, w, L.stream_ptr())
    rows = []
    for l in range(5):
        ci, co, _ = B.LAYERS[l]
        ref = B.layer_ref(l, _nchw(g[l])[:, :co].double(), case["params"][2 * l], _nchw(node_xs[l]).double(), wgs)
        gf = gflat[l].cpu()
        rows += [(f"dw{l}", gf[:co * ci * 49].view(co, ci, 7, 7), ref["dw"], ref["tol_dw"]), (f"db{l}", gf[co * ci * 49:], ref["db"], ref["tol_db"]),
                 (f"dx{l}", _nchw(g[l - 1] if l else dx0), ref["dx"], ref["tol_dx"])]
    _hold("chain %s" % _gid(B.CHAIN_GEOMETRY), rows)
    convs = [mod.basic_module[k] for k in (0, 2, 4, 6, 8)]
    pairs = [("dinput", x.grad.cpu(), _nchw(dx0))]
    for l, c in enumerate(convs):
        ci, co, _ = B.LAYERS[l]
        gf = gflat[l].cpu()
        pairs += [(f"dw{l}", c.weight.grad.cpu(), gf[:co * ci * 49].view(co, ci, 7, 7)), (f"db{l}", c.bias.grad.cpu(), gf[co * ci * 49:])]
    hold_exact("chain: autograd.Function against the C call", pairs)


def _spynet(sd):
    from mobilesuperresolution_amd.models.spynet_arch import SpyNet
    net = SpyNet().cuda()
    net.load_state_dict({k: v for k, v in sd.items()})
    return net


def test_whole_spynet_gradients():
    """2 pairs of 64 x 64, loss = a fixed cotangent dotted with the flow: the gradients of all 60 tensors and of ref / supp, per
    tensor in relative L2 against the unrounded float64 restatement, within TWICE the rounding noise the reference alone shows
    (its bf16-rounded restatement against the unrounded one; ReLU and border-clamp decisions may differ near ties).  No element
    is excluded; the seed keeps the reference's own flipped masks under the 1 % cap (checked on the host)."""
    sd, ref, supp, cot = B.spynet_case()
    g64, noise, flipped = B.spynet_noise()
    assert flipped <= B.MASK_CAP
    net = _spynet(sd)
    net.hot_training = True
    r, s = ref.cuda().requires_grad_(True), supp.cuda().requires_grad_(True)
    assert net.train_route_reason(r, s) is None
    flow = net(r, s)
    assert flow.requires_grad
    (flow * cot.cuda()).sum().backward()
    got = {k: p.grad for k, p in net.named_parameters()}
    got["ref"], got["supp"] = r.grad, s.grad
    bad = []
    for k in sorted(g64):
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), k
        err = B.rel_l2(got[k].cpu(), g64[k])
        print(f"spynet train | whole network | {k} | reference noise {noise[k]:.3e} | kernel {err:.3e} | ratio {err / noise[k]:.2f}")
        if not err <= 2 * noise[k]:
            bad.append((k, err, noise[k]))
    assert not bad, bad


def test_default_is_untouched():
    """hot_training unset: the flow has no history and equals the inference flow bit for bit, grad mode on or off; a refused call
    (frozen network, inputs without grad) keeps that behaviour with hot_training set"""
    sd, ref, supp, _ = B.spynet_case()
    net = _spynet(sd)
    with torch.no_grad():
        want = net(ref.cuda(), supp.cuda())
    got = net(ref.cuda(), supp.cuda())
    assert not got.requires_grad and got.grad_fn is None and torch.equal(got, want)
    net.hot_training = True
    trained = net(ref.cuda(), supp.cuda())
    assert trained.requires_grad and torch.equal(trained.detach(), want)
    for p in net.parameters():
        p.requires_grad_(False)
    assert net.train_route_reason(ref.cuda(), supp.cuda()) == "nothing requires grad"
    frozen = net(ref.cuda(), supp.cuda())
    assert not frozen.requires_grad and torch.equal(frozen, want)


def test_flow_warp_consumer():
    """flow_warp(x, spynet(ref, supp).permute(0, 2, 3, 1)): the HIP warp's flow gradient reaches spynet.*.grad"""
    from mobilesuperresolution_amd.models.spynet_arch import flow_warp
    sd, ref, supp, _ = B.spynet_case()
    net = _spynet(sd)
    net.hot_training = True
    out = flow_warp(supp.cuda(), net(ref.cuda(), supp.cuda()).permute(0, 2, 3, 1))
    (out - ref.cuda()).abs().mean().backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), k


def _vsr_step(flows_detached, seed_=5):
    from mobilesuperresolution_amd.models.basicvsr_arch import BasicVSR
    torch.manual_seed(seed_)
    model = BasicVSR(24, 2).cuda()
    model.spynet.hot_training = True
    g = torch.Generator().manual_seed(seed_)
    x = torch.rand(1, 3, 3, 64, 64, generator=g).cuda()
    flows = None
    if flows_detached:
        ff, fb = model.get_flow(x)
        flows = (ff.detach(), fb.detach())
    feat_b, feat_f = model.propagation_features(x, flows)
    cot = torch.randn(2, len(feat_b), *feat_b[0].shape, generator=g).cuda()
    loss = sum((a * cot[0, i]).sum() + (b * cot[1, i]).sum() for i, (a, b) in enumerate(zip(feat_b, feat_f)))
    loss.backward()
    return model


def test_basicvsr_end_to_end():
    """BasicVSR(24, 2) on a 1 x 3 x 3 x 64 x 64 clip with spynet.hot_training: every spynet.* parameter gets a finite, non-zero
    gradient through the 24-wide trunks' dflow; the trunk gradients are those of the same step with the flows detached, bit for
    bit; two equal steps give equal spynet.*.grad"""
    a, b, det = _vsr_step(False), _vsr_step(False), _vsr_step(True)
    trunk = lambda m: [(k, p.grad) for k, p in m.named_parameters() if not k.startswith("spynet.") and p.grad is not None]
    spy = lambda m: [(k, p.grad) for k, p in m.named_parameters() if k.startswith("spynet.")]
    assert len(spy(a)) == 60 and trunk(a)
    for k, gr in spy(a):
        assert gr is not None and bool(torch.isfinite(gr).all()) and bool((gr != 0).any()), k
    for k, gr in spy(det):
        assert gr is None, k
    hold_exact("trunk gradients, flows detached or not", [(k, ga, gd) for (k, ga), (_, gd) in zip(trunk(a), trunk(det))])
    hold_exact("two equal steps", [(k, ga, gb) for (k, ga), (_, gb) in zip(spy(a), spy(b))])


def test_basicvsr_origin_graph_route():
    """BasicVSR_origin at F <= 24 on its graph-recording route: the loss on the output reaches spynet.*.grad"""
    from mobilesuperresolution_amd.models.basicvsr_arch_origin import BasicVSR_origin
    torch.manual_seed(7)
    model = BasicVSR_origin(24, 2).cuda()
    model.spynet.hot_training = True
    x = torch.rand(1, 3, 3, 64, 64, generator=torch.Generator().manual_seed(7)).cuda()
    model(x, 256, 256).abs().mean().backward()
    for k, p in model.spynet.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), k
