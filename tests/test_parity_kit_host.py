"""tests/parity_kit.py on the CPU: the lattice helpers, the 2^24 rule, the seed recipe, the accuracy bound and the two comparisons
that every parity suite stands on."""
import pytest
import torch

from tests import parity_kit as K


def test_lowbit():
    t = torch.tensor([0.0, 3 * 2.0 ** -5, -1.0, 12.0, 2.0 ** -149, 3 * 2.0 ** -148])      # the last two: fp32 denormals
    assert t.dtype == torch.float32 and float(t[4]) > 0
    assert K.lowbit(t).tolist() == [2.0 ** 200, 2.0 ** -5, 1.0, 4.0, 2.0 ** -149, 2.0 ** -148]
    assert K.BIG == 2.0 ** 200


def test_chan_quantum():
    t = torch.tensor([[[[0.75, 0.5]], [[0.0, 0.0]], [[-6.0, 4.0]]]])
    assert K.chan_quantum(t).tolist() == [0.25, K.BIG, 2.0]
    empty = K.chan_quantum(torch.zeros(2, 3, 0, 5))
    assert empty.dtype == torch.float64 and empty.tolist() == [K.BIG] * 3


def test_bf16_ties_and_rounding():
    tie, not_a, not_b = 1 + 2.0 ** -8, 1 + 2.0 ** -7, 1 + 2.0 ** -9
    t = torch.tensor([tie, not_a, not_b, -tie, 0.0, 257.0, 256.0, 3 * 2.0 ** -9 + 2.0], dtype=torch.float64)
    assert K.bf16_ties(t).tolist() == [True, False, False, True, False, True, False, False]
    assert K.count_ties(t) == 3
    assert K.bf16_round(t)[:4].tolist() == [1.0, not_a, 1.0, -1.0]          # the tie goes to the even neighbour; 1 + 2^-9 is below it
    assert K.bf16_round(torch.tensor([1 + 3 * 2.0 ** -8], dtype=torch.float64)).item() == 1 + 2.0 ** -6      # odd neighbour below: up
    assert K.bf16_round(t).dtype == torch.float64
    assert K.is_bf16(torch.tensor([not_a, -3.0])) and not K.is_bf16(torch.tensor([tie]))
    assert K.is_fp32(torch.tensor([1 + 2.0 ** -23], dtype=torch.float64)) and not K.is_fp32(torch.tensor([1 + 2.0 ** -24], dtype=torch.float64))


def test_need_sum():
    q = torch.tensor([0.25])
    assert K.need_sum("a sum", torch.tensor([(2.0 ** 24 - 1) * 0.25]), q) == 2.0 ** 24 - 1
    assert K.need_sum("a sum", torch.tensor([3.0, 1.0]), 0.5) == 6.0                # a plain number as the quantum
    with pytest.raises(ValueError, match="exact case: a sum: .*2\\^24"):
        K.need_sum("a sum", torch.tensor([2.0 ** 22]), q)
    with pytest.raises(ValueError, match="2\\^24"):
        K.need_sum("a sum", torch.tensor([1.0, float("nan")]), q)
    assert K.need_sum("a sum", torch.zeros(0, 3), torch.ones(3)) == 0.0


def test_conditions_raise():
    for call in (lambda: K.need_bf16("t", torch.tensor([1 + 2.0 ** -8])),
                 lambda: K.need_fp32("t", torch.tensor([1 + 2.0 ** -24], dtype=torch.float64)),
                 lambda: K.need_half_nonzero("t", torch.tensor([1.0, 0.0, 0.0])),
                 lambda: K.need_half_nonzero("t", torch.tensor([1.0, 0.0, 0.0, 0.0]), torch.tensor([1.0, 1.0, 1.0, 0.0])),
                 lambda: K.need_half_nonzero("t", torch.zeros(2), torch.zeros(2)),
                 lambda: K.need_biases("b", torch.tensor([1.0, 0.0])),
                 lambda: K.need_biases("b", torch.tensor([1.0, 2.0, 1.0]))):
        with pytest.raises(ValueError, match="exact case: "):
            call()
    K.need_bf16("t", torch.tensor([1.5]))
    K.need_half_nonzero("t", torch.tensor([1.0, 0.0]))
    K.need_half_nonzero("t", torch.tensor([1.0, 0.0, 0.0, 0.0]), torch.tensor([1.0, 1.0, 0.0, 0.0]))
    K.need_biases("b", torch.tensor([1.0, -1.0]))


def test_tap_symmetries():
    w = torch.arange(18.0).view(1, 2, 3, 3)
    assert len(K.tap_symmetries(w)) == 7 and len(K.tap_symmetries(w, 1, 5)) == 1 and K.tap_symmetries(w, 1, 1) == []
    K.need_taps("w", w)
    sym = w + w.transpose(2, 3)
    mirrored = torch.tensor([[1.0, 2.0, 1.0], [3.0, 4.0, 3.0], [5.0, 6.0, 5.0]]).view(1, 1, 3, 3)      # left-right only
    for bad, geom in ((sym, (3, 3)), (mirrored, (3, 3)), (mirrored, (1, 5))):
        with pytest.raises(ValueError, match="symmetric"):
            K.need_taps("w", bad, *geom)
    K.need_taps("w", mirrored, 5, 1)                          # a 1-pixel-wide image forces that symmetry: not asked


def test_seed_reproduces_the_modules_recorded_values():
    key = (1, 24, 3, 13, 25)
    for start, step, want in ((13579, 7, 1623700712), (12345, 7, 563751762), (24680, 7, 1396075132), (24680, 11, 541137056), (0, 17, 1682071059)):
        assert K.seed(start, step, *key) == want
        assert K.seed(start, step) == start


def test_modules_bind_their_own_seed_constants():
    from tests import block_ref, conv_ref, ends_ref, frame_net_ref, trunk_ref
    key = (1, 24, 3, 13, 25)
    got = [m._seed(*key) for m in (block_ref, trunk_ref, ends_ref, conv_ref, frame_net_ref)]
    assert got == [1623700712, 563751762, 1396075132, 541137056, 1682071059]


def test_bound():
    assert K.bound("fp32", 0.5) == 8 * 0.5 + 1e-6 and K.bound("bf16", 0.5) == 4 * 0.5
    assert K.bound("fp32", 0.0) == 1e-6 and K.bound("bf16", 0.0) == 0.0
    assert K.bound("fp32", 0.5, slack=0.0) == 4.0


def test_rel_max():
    ref = torch.tensor([2.0, -4.0])
    assert K.rel_max(torch.tensor([2.5, -4.0]), ref) == 0.125
    assert K.rel_max(torch.tensor([0.5, 0.0]), torch.zeros(2)) == 0.5          # nothing to scale by: the plain distance
    assert K.rel_max(torch.zeros(0), torch.zeros(0)) == 0.0
    assert K.rel_max(torch.tensor([float("nan"), -4.0]), ref) != K.rel_max(torch.tensor([float("nan"), -4.0]), ref)   # NaN


def test_hold_rounded(capsys):
    ref = torch.tensor([1.0, 0.0, -0.25], dtype=torch.float64)
    off = lambda d: ref + torch.tensor([0.0, d, 0.0], dtype=torch.float64)       # (onto a zero: the error is d exactly)
    e_ref = 2.0 ** -10                                       # bf16: the bound is 2^-8, and max |ref| = 1
    K.hold_rounded("kit parity", "a tag", "bf16", [("y", off(2.0 ** -8), ref, e_ref)])           # err == tol passes
    assert capsys.readouterr().out == "kit parity | a tag | y | yardstick 9.77e-04 | kernel 3.91e-03 | ratio 4.00 | bound 3.91e-03\n"
    with pytest.raises(AssertionError):
        K.hold_rounded("kit parity", "a tag", "bf16", [("y", off(2.0 ** -8 + 2.0 ** -40), ref, e_ref)])
    K.hold_rounded("kit parity", "a tag", "fp32", [("y", off(2.0 ** -7 + 1e-6), ref, e_ref)])    # 8 x, + 1e-6
    with pytest.raises(AssertionError):
        K.hold_rounded("kit parity", "a tag", "fp32", [("y", off(2.0 ** -7 + 2e-6), ref, e_ref)])
    with pytest.raises(AssertionError):
        K.hold_rounded("kit parity", "a tag", "fp32", [("y", off(float("nan")), ref, 1.0)])
    K.hold_rounded("kit parity", "a tag", "bf16", [("y", ref.float(), ref, 0.0)])                # no yardstick error: equality
    assert "ratio nan" in capsys.readouterr().out
    with pytest.raises(AssertionError):
        K.hold_rounded("kit parity", "a tag", "bf16", [("y", off(2.0 ** -60), ref, 0.0)])
    with pytest.raises(AssertionError) as e:                  # every row is judged, the good ones too
        K.hold_rounded("kit parity", "a tag", "bf16", [("bad", off(1.0), ref, e_ref), ("good", ref, ref, e_ref)])
    assert "bad" in str(e.value) and "good" not in str(e.value) and "| good |" in capsys.readouterr().out


def test_first_diff_and_hold_exact():
    nan = float("nan")
    a = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    assert K.first_diff("a", a, a.clone()) is None
    assert K.first_diff("a", a.bfloat16(), a.double()) is None                  # exp is cast to got's dtype ...
    assert K.first_diff("a", torch.tensor([1.0]).bfloat16(), torch.tensor([1 + 2.0 ** -9])) is None     # ... so it is rounded as got was
    msg = K.first_diff("a", torch.tensor([[1.0, 2.0], [5.0, nan]]), a)
    assert msg == "a: 2 of 4 differ, first at [1, 0]: got 5.0 expected 3.0"
    # an output buffer is pre-filled with NaN: an element that was never written differs from any expectation, NaN included
    msg = K.first_diff("buf", torch.tensor([1.0, nan]), torch.tensor([1.0, nan]))
    assert msg is not None and msg.startswith("buf: 1 of 2 differ, first at [1]")
    with pytest.raises(AssertionError):
        K.first_diff("a", a, a[:1])
    K.hold_exact("tag", [("a", a, a.double()), ("b", a[0], a[0])])
    K.hold_exact("tag", iter([]))
    with pytest.raises(AssertionError) as e:
        K.hold_exact("tag", [("a", a, a), ("b", a + 1, a), ("c", torch.tensor([nan]), torch.tensor([nan]))])
    assert "b: 4 of 4 differ" in str(e.value) and "c: 1 of 1 differ" in str(e.value) and "a: " not in str(e.value)
