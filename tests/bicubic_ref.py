"""numpy restatement of the reference's `imresize(I, scalar_scale=1/scale)` for uint8 input
(third_party/matlab_imresize/imresize.py:104-136), the arithmetic csrc/bicubic.h reproduces: two passes, rows (dim 0) first;
each pass forms  ((w0 p0 + w1 p1) + w2 p2) + ...  in float64, one tap after another in tap order (separately rounded
products and sums: numpy never fuses them), clips to [0, 255], rounds half to even (`np.around`) and goes back to uint8.
tests/test_bicubic_host.py pins it to the reference's own outputs (fixture G20) with `np.array_equal`; the GPU tests use it at
shapes the fixture does not hold.  The tables are packing.bicubic_tables, themselves pinned bitwise to the fixture."""
import numpy as np

from mobilesuperresolution_amd.packing import bicubic_tables


def pass_float(a, weights, indices, axis):
    """one pass along `axis` (0 or 1) of an H x W x C uint8 image, before clip and rounding: float64"""
    a = np.moveaxis(np.asarray(a), axis, 0)
    assert a.dtype == np.uint8
    acc = weights[:, 0, None, None] * a[indices[:, 0]].astype(np.float64)
    for t in range(1, weights.shape[1]):
        acc = acc + weights[:, t, None, None] * a[indices[:, t]].astype(np.float64)
    return np.moveaxis(acc, 0, axis)


def to_u8(v):
    return np.around(np.clip(v, 0, 255)).astype(np.uint8)


def downscale(img, scale):
    """H x W x 3 uint8 -> ceil(H / scale) x ceil(W / scale) x 3 uint8"""
    img = np.asarray(img)
    mid = to_u8(pass_float(img, *bicubic_tables(img.shape[0], scale), axis=0))
    return to_u8(pass_float(mid, *bicubic_tables(img.shape[1], scale), axis=1))


def half_even_ties(img, scale):
    """number of first-pass values that are exact .5 ties at which round-half-even and round-half-up differ (even floor)"""
    v = np.clip(pass_float(img, *bicubic_tables(np.asarray(img).shape[0], scale), axis=0), 0, 255)
    f = np.floor(v)
    return int(np.count_nonzero((v - f == 0.5) & (f % 2 == 0)))


def augment(a, flags):
    """the reference's `_augment` (datasets/_isr.py:109-121) on an H x W x C array: 1 flip rows, 2 flip columns, 4 swap axes"""
    if flags & 1:
        a = a[::-1]
    if flags & 2:
        a = a[:, ::-1]
    if flags & 4:
        a = np.swapaxes(a, 0, 1)
    return a


def train_item(hr, x, y, flags, P, scale, ig):
    """TRAIN-mode item of ImageSuperResolutionBicubicDataset (datasets/_isr.py:197-214, then `_augment`) for the draws
    (x, y, flags): (lr 3 x P x P, hr 3 x P scale x P scale) uint8"""
    S, b = (P + 2 * ig) * scale, ig * scale
    crop = np.asarray(hr)[x:x + S, y:y + S]
    lr = downscale(crop, scale)[ig:-ig, ig:-ig]
    ctr = crop[b:-b, b:-b]
    return (np.ascontiguousarray(augment(lr, flags).transpose(2, 0, 1)),
            np.ascontiguousarray(augment(ctr, flags).transpose(2, 0, 1)))
