"""What the parity suites share: the roundings, the lattice helpers, the exactness conditions, the seed recipe and the accuracy
bound.  Plain torch on the CPU, nothing of the package.  The reference modules (block_ref, ends_ref, conv_ref, trunk_ref, nas_ref,
frame_net_ref) build their check_exact() and their case generators on it, the test_gpu_* files of those families hold the kernels
to the references with hold_exact() / hold_rounded(), and tests/test_parity_kit_host.py pins every function below.

An EXACT case is dyadic data on which every operand a kernel holds in the hot dtype is its own bf16 rounding and every reduction
satisfies sum |terms| < 2^24 quanta of its lattice (need_sum): fp32 accumulation is then exact in any order, so a kernel must
return the float64 reference bit for bit.  A ROUNDED case is random data; the kernel's distance from the float64 reference, in
rel_max's metric, must stay within bound() of the same distance of a CPU emulation of the kernel's precision (the yardstick).
"""
import torch


# ---- rounding ----------------------------------------------------------------------------------------------------------------
def bf16_round(t):
    """to bf16 (nearest even) and back to t's dtype"""
    return t.bfloat16().to(t.dtype)


class RoundForward(torch.autograd.Function):
    """value rounded on the way forward, gradient passed through (a tensor the kernels hold in bf16)"""

    @staticmethod
    def forward(ctx, x, rnd):
        return rnd(x)

    @staticmethod
    def backward(ctx, g):
        return g, None


class RoundBackward(torch.autograd.Function):
    """identity forward, gradient rounded on the way back (a gradient the kernels hold in bf16)"""

    @staticmethod
    def forward(ctx, x, rnd):
        ctx.rnd = rnd
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.rnd(g), None


def leaf(t, dtype=torch.float64):
    return t.detach().to(dtype, copy=True).requires_grad_(True)


# ---- lattices ----------------------------------------------------------------------------------------------------------------
BIG = 2.0 ** 200


def lowbit(t):
    """per element, the largest power of two that divides it (2^200 for 0)"""
    mant, exp = torch.frexp(t.double())                    # t = mant 2^exp, mant a 53-bit fraction
    i = (mant * 2.0 ** 53).long()
    low = torch.ldexp((i & -i).double(), exp - 53)
    return torch.where(i == 0, torch.full_like(low, BIG), low)


def chan_quantum(t):
    """(C,) of an (N, C, H, W) tensor: the lattice each channel lives on (2^200 for a channel without elements)"""
    return lowbit(t).amin((0, 2, 3)) if t.numel() else torch.full((t.shape[1],), BIG, dtype=torch.float64)


def is_bf16(t):
    return torch.equal(t.double(), t.double().bfloat16().double())


def is_fp32(t):
    return torch.equal(t.double(), t.double().float().double())


def bf16_ties(t):
    """bool: elements exactly half way between two bf16 neighbours (nine significant bits, the last one set)"""
    mant, _ = torch.frexp(t.double())
    m9 = mant.abs() * 512.0
    return (m9 == m9.floor()) & (m9.floor() % 2 == 1)


def count_ties(t):
    return int(bf16_ties(t).sum())


# ---- conditions of an exact case ---------------------------------------------------------------------------------------------
def fail(msg):
    raise ValueError("exact case: " + msg)


def need_bf16(name, t):
    if not is_bf16(t):
        fail(f"{name} is not its own bf16 rounding")


def need_fp32(name, t):
    if not is_fp32(t):
        fail(f"{name} is not representable in fp32")


def need_sum(name, abs_sum, quantum):
    """sum |terms| < 2^24 quanta: every partial sum, in any order, is a whole number of quanta below 2^24, i.e. exact in fp32.
    abs_sum and quantum broadcast against each other (one quantum per accumulator).  Returns the worst ratio (0.0 for an empty
    sum); a NaN raises."""
    if abs_sum.numel() == 0:
        return 0.0
    worst = float((abs_sum / quantum).max())
    if not worst < 2.0 ** 24:
        fail(f"{name}: sum |terms| = {worst} quanta >= 2^24")
    return worst


def need_half_nonzero(name, t, reach=None):
    """at least half of the tensor -- of what the geometry lets be nonzero (reach: the same sum over |terms|) -- is nonzero"""
    n_reach, n_nz = t.numel() if reach is None else int((reach > 0).sum()), int((t != 0).sum())
    if n_reach == 0 or 2 * n_nz < n_reach:
        fail(f"{name}: {n_nz} of {n_reach} reachable elements are nonzero")


def need_biases(name, b):
    if bool((b == 0).any()) or torch.unique(b).numel() != b.numel():
        fail(f"{name}: biases must be nonzero and differ per channel")


def tap_symmetries(w, h=3, w_img=3):
    """the tap transpositions / reversals under which a (.., k, k) tensor over an h x w_img image is NOT symmetric by
    construction (a 1-pixel-high image reaches one tap row only)"""
    if h < 2 and w_img < 2:
        return []
    if h < 2:
        return [w.flip(-1)]
    if w_img < 2:
        return [w.flip(-2)]
    wt = w.transpose(-1, -2)
    return [wt, w.flip(-2), w.flip(-1), w.flip(-2, -1), wt.flip(-2), wt.flip(-1), wt.flip(-2, -1)]


def need_taps(name, w, h=3, w_img=3):
    if any(torch.equal(sym, w) for sym in tap_symmetries(w, h, w_img)):
        fail(f"{name}: symmetric under a transposition or reversal of the taps")


# ---- seeds -------------------------------------------------------------------------------------------------------------------
def seed(start, step, *key):
    """the generators' seed of a case key; every reference module binds its own (start, step)"""
    s = start
    for v in key:
        s = (s * 1000003 + int(v) + step) % (2 ** 31 - 1)
    return s


# ---- distances and bounds ----------------------------------------------------------------------------------------------------
def rel_max(got, ref):
    """max |got - ref| / max |ref| (the plain max |got - ref| where ref vanishes; 0 for empty tensors)"""
    if ref.numel() == 0:
        return 0.0
    ref = ref.double()
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    return err / scale if scale > 0 else err


def bound(mode, e_ref, slack=1e-6):
    """THE accuracy rule of the rounded cases: a kernel may be 8 x (fp32, plus `slack`) or 4 x (bf16) as far from the float64
    reference as the yardstick e_ref is"""
    return 8 * e_ref + slack if mode == "fp32" else 4 * e_ref


def first_diff(name, got, exp):
    """None if got equals exp (cast to got's dtype) bit for bit, else a line that names the first difference; an element that is
    NaN in got counts as different, so an output buffer pre-filled with NaN shows what was not written"""
    got, exp = got.detach().cpu(), exp.to(got.dtype).cpu()
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    if torch.equal(got, exp):
        return None
    ne = (got != exp) | (got != got)
    idx = ne.nonzero()[0].tolist()
    return f"{name}: {int(ne.sum())} of {got.numel()} differ, first at {idx}: got {got[tuple(idx)].item()} expected {exp[tuple(idx)].item()}"


def hold_exact(tag, pairs):
    """pairs: (name, got, expected) triples; every got must equal its expected bit for bit"""
    bad = [m for m in (first_diff(*p) for p in pairs) if m]
    assert not bad, (tag, bad[:8], len(bad))


def hold_rounded(prefix, tag, mode, rows):
    """rows: (label, got, float64 reference, yardstick) per tensor; every rel_max(got, reference) must stay within
    bound(mode, yardstick).  Prints one line per row (DESIGN.md's tables are made from them)."""
    bad = []
    for label, got, ref, e_ref in rows:
        err = rel_max(got.detach().cpu(), ref)
        tol = bound(mode, e_ref)
        ratio = err / e_ref if e_ref > 0 else float("nan")
        print(f"{prefix} | {tag} | {label} | yardstick {e_ref:.2e} | kernel {err:.2e} | ratio {ratio:.2f} | bound {tol:.2e}")
        if not err <= tol:
            bad.append((label, err, tol))
    assert not bad, (tag, bad)
