"""The clip node base both video networks' training nodes derive from (models/clip_train.ClipTrain), on the CPU: a stand-in subclass
whose "HIP backward" is a few torch ops returning a flat vector, through the plain path, the folded path, their sum, and can_fold's
refusals.  hotpath.scale_by, a kernel launch, is replaced by the fp32 product it computes."""
import pytest
import torch

from mobilesuperresolution_amd.models import loss_fold as LF

SIZES = [4, 2, 6, 3]                       # the flat vector: the body's (weight, bias), then the encoder's -- the encoder LAST
BASE = torch.arange(1.0, 16.0)


def _toy(lead):
    from mobilesuperresolution_amd.models import clip_train as CT

    class _Toy(CT.ClipTrain):
        LEAD = lead
        calls = []

        @staticmethod
        def _grad_sizes(channel, nb):
            assert (channel, nb) == (7, 5)
            return SIZES

        @staticmethod
        def _run_backward(ctx, g, hr=None, kind=0, gscale=0.0):
            _Toy.calls.append((hr is not None, kind, gscale))
            assert g.dtype == torch.float32 and g.is_contiguous()
            if hr is None:
                assert g.shape == (ctx.saved[0].shape[0], 3, 8, 12)        # normalised to the frames' batch
                return BASE * g.sum(), None
            d = g - hr
            return BASE * (gscale * torch.sign(d)).sum(), d.abs().sum().reshape(1)

        @staticmethod
        def forward(ctx, *args):
            x, eff = args[1], args[lead:]                                  # (model, x, ..no-gradient inputs.., *eff)
            ctx.saved = (CT.frames_of(x),)
            ctx.geom = (7, 5)
            out = x.detach().repeat_interleave(4, 3).repeat_interleave(4, 4).float()
            return _Toy._record(ctx, out, eff)

    return _Toy


@pytest.fixture
def toy(request, monkeypatch):
    """(the stand-in class, a call -> (out, eff)) for LEAD = request.param"""
    from mobilesuperresolution_amd import hotpath as HP
    monkeypatch.setattr(HP, "scale_by", lambda x, scale: x * scale.detach().float().reshape(1))
    lead = request.param
    cls = _toy(lead)
    g = torch.Generator().manual_seed(3)

    def call():
        x = torch.rand(2, 3, 3, 2, 3, generator=g, dtype=torch.float64)              # not fp32: frames_of converts
        eff = [torch.rand(s, generator=g, requires_grad=True) for s in ((2, 3), (3,), (2, 2), (2,))]     # encoder first
        out = cls.apply(*["model", x, "flows"][:lead], *eff)
        assert type(out.grad_fn).__name__ == "_ToyBackward" and out.shape == (2, 3, 3, 8, 12)
        return out, eff
    return cls, call


def _expected(vec, lead):
    w, b, ew, eb = vec.split(SIZES)
    return (None,) * lead + (ew.view(2, 3), eb.view(3), w.view(2, 2), b.view(2))


def _same(got, want):
    assert len(got) == len(want)
    for a, e in zip(got, want):
        assert (a is None and e is None) or (a.shape == e.shape and torch.equal(a, e))


def _fold(node, out, hr, gloss):
    """what training._FoldedCriterion does with the node: fold, park, and the zero token it sends up"""
    payload, loss_part = LF.fold(node, out, hr, "l1")
    token = torch.zeros(1).expand(out.shape)
    node.folded = (payload, gloss, token.data_ptr())
    return payload, loss_part, token


LEADS = pytest.mark.parametrize("toy", (2, 3), indirect=True, ids=("lead2", "lead3"))


@LEADS
def test_plain_path_splits_and_puts_the_encoder_first(toy):
    cls, call = toy
    out, eff = call()
    g = torch.rand(out.shape, generator=torch.Generator().manual_seed(4)).transpose(3, 4).contiguous().transpose(3, 4)   # not contiguous
    want = BASE * g.contiguous().sum()
    _same(cls.backward(out.grad_fn, g), _expected(want, cls.LEAD))
    assert cls.calls == [(False, 0, 0.0)] and out.grad_fn.ran
    # and through autograd: every effective tensor gets its piece
    out, eff = call()
    (out * g).sum().backward()
    _same([t.grad for t in eff], _expected(want, 0))


@LEADS
def test_folded_with_the_token_returns_the_parked_vector_times_the_loss_gradient(toy):
    cls, call = toy
    out, eff = call()
    node = out.grad_fn
    hr = torch.rand(out.shape, generator=torch.Generator().manual_seed(5))
    assert LF.can_fold(node, out, hr)
    payload, loss_part, token = _fold(node, out, hr, torch.tensor(0.25))
    gscale = float(torch.tensor(1.0) / torch.tensor(float(out.numel())))
    assert cls.calls == [(True, 1, gscale)]
    assert torch.equal(payload, BASE * (gscale * torch.sign(out.detach() - hr)).sum())
    assert torch.equal(loss_part, (out.detach() - hr).abs().sum().reshape(1))
    _same(cls.backward(node, token), _expected(payload * torch.tensor(0.25), cls.LEAD))
    assert len(cls.calls) == 1                                             # the hook did not run again


@LEADS
def test_folded_with_another_gradient_returns_the_sum(toy):
    cls, call = toy
    out, eff = call()
    node = out.grad_fn
    hr = torch.rand(out.shape, generator=torch.Generator().manual_seed(6))
    payload, _, token = _fold(node, out, hr, torch.tensor(2.0))
    other = torch.rand(out.shape, generator=torch.Generator().manual_seed(7))
    g = token + other                                                      # the token plus another use of the output
    _same(cls.backward(node, g), _expected(BASE * g.sum() + payload * torch.tensor(2.0), cls.LEAD))
    assert cls.calls[1:] == [(False, 0, 0.0)]
    # a zero-stride tensor that is not the token runs the usual way too
    out, eff = call()
    node = out.grad_fn
    payload, _, token = _fold(node, out, hr, torch.tensor(2.0))
    zeros = torch.zeros(1).expand(out.shape)
    _same(cls.backward(node, zeros), _expected(BASE * 0.0 + payload * torch.tensor(2.0), cls.LEAD))
    assert len(cls.calls) == 4


@LEADS
def test_can_fold_is_false_after_fold_started_ran_and_folded(toy):
    cls, call = toy
    hr = torch.rand(2, 3, 3, 8, 12)
    out, _ = call()
    node = out.grad_fn
    assert LF.can_fold(node, out, hr)
    LF.fold(node, out, hr, "charbonnier")
    assert node.fold_started and cls.calls[-1][1] == 2 and not LF.can_fold(node, out, hr)      # fold_started
    out, _ = call()
    node = out.grad_fn
    cls.backward(node, torch.ones(out.shape))
    assert node.ran and not node.fold_started and node.folded is None and not LF.can_fold(node, out, hr)       # ran
    out, _ = call()
    node = out.grad_fn
    node.folded = (torch.zeros(15), torch.tensor(1.0), 0)
    assert not node.ran and not node.fold_started and not LF.can_fold(node, out, hr)           # folded
