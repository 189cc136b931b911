#!/usr/bin/env python3
"""Write fixture G20 (tests/golden/g20_bicubic.npz, data only) by running the REFERENCE's own MATLAB-compatible resize and its
HR-only dataset class on the CPU:

    SR_REFERENCE_ROOT=<reference checkout> python tools/make_golden_bicubic.py

`imresize`, `contributions` and `cubic` are imported from the reference's third_party/matlab_imresize/imresize.py, and
`datasets._isr` with the absent third-party modules stubbed (oracle/make_golden.py's stubs), so the reference's own
ImageSuperResolutionBicubicDataset runs unchanged: `_load_item` through PIL on PNG files written here, `_sample_patch`
(`imresize` of the HR crop), `_augment`, `to_tensor`, under a seeded `random`.  Nothing of the item path is restated here.

Stored, for scale 2, 3 and 4:
  * four uint8 images and the reference's `imresize(img, scalar_scale=1 / scale)` of each: random 48s x 52s; a 0 / 255 binary
    image of 37 x 50 (clip and overshoot, no multiple of the scale); a random 4s x 4s (smaller than the filter support); a
    low-amplitude image (values 0..3) of 16s x 20s whose seed is searched so that, where the weights are dyadic (x2, x4), at
    least one first-pass value is an exact .5 tie at which round-half-even and round-half-up differ (count stored; x3 has no
    exact ties);
  * the reference's `contributions` tables for every source length used anywhere in the fixture;
  * the EVAL-mode item of a 37 x 50 image (HR cropped to multiples of the scale).
For two TRAIN configurations (ignored_boundary_size 1: the centre outputs reach the crop's reflection; ignored_boundary_size 2
with num_patches 2): the HR images, every item (LR / HR as uint8: `to_tensor` only divides by 255), the values the reference's
`random.randrange` / `random.random` calls returned item by item, and `random.random()` drawn right after the last item.  The
seed of each is searched so that the items cover all eight flip / transpose combinations."""
import argparse
import importlib
import os
import random
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SR_REFERENCE_ROOT", "")
OUT = os.path.join(ROOT, "tests", "golden", "g20_bicubic.npz")
SCALES = (2, 3, 4)
# (scale, lr_patch_size, ignored_boundary_size, num_patches, n_images, n_items)
CFGS = [(4, 8, 1, 1, 3, 32), (3, 12, 2, 2, 2, 32)]


def _images(scale):
    g = np.random.default_rng(200 + scale)
    return [g.integers(0, 256, (48 * scale, 52 * scale, 3), dtype=np.uint8),
            (g.integers(0, 2, (37, 50, 3)) * 255).astype(np.uint8),
            g.integers(0, 256, (4 * scale, 4 * scale, 3), dtype=np.uint8)]


def _low_amplitude(scale, BR):
    """(image, seed, ties): the first seed whose image has a first-pass tie that tells half-to-even from half-up"""
    for seed in range(2000):
        img = np.random.default_rng(seed).integers(0, 4, (16 * scale, 20 * scale, 3), dtype=np.uint8)
        ties = BR.half_even_ties(img, scale)
        if ties or scale == 3:
            return img, seed, ties
    sys.exit(f"no tie image found for scale {scale}")


def main():
    if not os.path.isfile(os.path.join(REF, "third_party", "matlab_imresize", "imresize.py")):
        sys.exit("set SR_REFERENCE_ROOT to a checkout of the reference (third_party/matlab_imresize/imresize.py not found)")
    sys.path.insert(0, ROOT)
    from oracle.make_golden import _absent_third_party_stubs
    from tests import bicubic_ref as BR
    from PIL import Image
    _absent_third_party_stubs()
    sys.path.insert(0, REF)
    mi = importlib.import_module("third_party.matlab_imresize.imresize")
    isr = importlib.import_module("datasets._isr")
    modes = importlib.import_module("common.modes")

    d = {"scales": np.array(SCALES, dtype=np.int64), "cfgs": np.array([c[:4] for c in CFGS], dtype=np.int64)}
    lengths = set()

    def resize(img, scale):
        out = mi.imresize(img, scalar_scale=1 / scale)
        assert out.dtype == np.uint8
        assert np.array_equal(out, BR.downscale(img, scale)), "tests/bicubic_ref.py disagrees with the reference"
        lengths.update((scale, n) for n in img.shape[:2])
        return out

    for scale in SCALES:
        low, seed, ties = _low_amplitude(scale, BR)
        assert ties >= 1 or scale == 3
        imgs = _images(scale) + [low]
        for k, img in enumerate(imgs):
            d[f"s{scale}_img{k}"], d[f"s{scale}_out{k}"] = img, resize(img, scale)
        d[f"s{scale}_n_img"], d[f"s{scale}_tie_seed"], d[f"s{scale}_ties"] = np.int64(len(imgs)), np.int64(seed), np.int64(ties)
        print(f"G20 x{scale}: {[i.shape[:2] for i in imgs]}, low-amplitude seed {seed}: {ties} half-even ties in pass 1")

    with tempfile.TemporaryDirectory() as tmp:
        def dataset(mode, params, images, tag):
            files = []
            for k, img in enumerate(images):
                p = os.path.join(tmp, f"{tag}_{k}.png")
                Image.fromarray(img).save(p)
                files.append((f"{k}.png", p))
            return isr.ImageSuperResolutionBicubicDataset(mode, params, files)

        d["eval_img"] = np.random.default_rng(209).integers(0, 256, (37, 50, 3), dtype=np.uint8)
        for scale in SCALES:
            ds = dataset(modes.EVAL, argparse.Namespace(scale=scale), [d["eval_img"]], f"e{scale}")
            _, lr, hr = ds[0]
            d[f"eval_s{scale}_lr"], d[f"eval_s{scale}_hr"] = (lr * 255).round().to(torch.uint8).numpy(), (hr * 255).round().to(torch.uint8).numpy()
            assert torch.equal(torch.from_numpy(d[f"eval_s{scale}_lr"]).float().div(255), lr)
            lengths.update((scale, n) for n in hr.shape[1:])

        for ci, (scale, P, ig, num_patches, n_img, n_items) in enumerate(CFGS):
            S = (P + 2 * ig) * scale
            g = np.random.default_rng(2000 + ci)
            images = [g.integers(0, 256, (S + int(g.integers(0, 24)), S + int(g.integers(0, 24)), 3), dtype=np.uint8) for _ in range(n_img)]
            images[0] = images[0][:S]                                  # one image exactly S high: randrange(0, 1)
            params = argparse.Namespace(scale=scale, lr_patch_size=P, ignored_boundary_size=ig, num_patches=num_patches)
            ds = dataset(modes.TRAIN, params, images, f"c{ci}")
            idx = (list(range(len(ds))) * n_items)[:n_items]
            real_randrange, real_random = random.randrange, random.random
            for seed in range(20000 + 100 * ci, 20100 + 100 * ci):
                drawn = []
                random.randrange = lambda *a: drawn.append(real_randrange(*a)) or drawn[-1]
                random.random = lambda: drawn.append(real_random()) or drawn[-1]
                try:
                    random.seed(seed)
                    items = [ds[i] for i in idx]
                finally:
                    random.randrange, random.random = real_randrange, real_random
                draws = np.array(drawn, dtype=np.float64).reshape(n_items, 5)
                combos = {tuple(r) for r in (draws[:, 2:] < 0.5).tolist()}
                if len(combos) == 8:
                    break
            else:
                sys.exit(f"cfg {ci}: no seed covers all flag combinations")
            lrs = [(a * 255).round().to(torch.uint8).numpy() for a, _ in items]
            hrs = [(b * 255).round().to(torch.uint8).numpy() for _, b in items]
            for (a, b), l, h in zip(items, lrs, hrs):
                assert a.shape == (3, P, P) and b.shape == (3, P * scale, P * scale)
                assert torch.equal(torch.from_numpy(l).float().div(255), a) and torch.equal(torch.from_numpy(h).float().div(255), b)
            for k, img in enumerate(images):
                d[f"c{ci}_hr{k}"] = img
            d[f"c{ci}_n_img"], d[f"c{ci}_seed"] = np.int64(n_img), np.int64(seed)
            d[f"c{ci}_idx"], d[f"c{ci}_draws"] = np.array(idx, dtype=np.int64), draws
            d[f"c{ci}_lr_items"], d[f"c{ci}_hr_items"] = np.stack(lrs), np.stack(hrs)
            d[f"c{ci}_next_random"] = np.float64(random.random())
            lengths.add((scale, S))
            print(f"G20 cfg {ci} (scale {scale}, P {P}, ignored {ig}, num_patches {num_patches}): {n_img} images, {n_items} items, seed {seed}")

    keys = sorted(lengths)
    d["table_keys"] = np.array(keys, dtype=np.int64)
    for scale, n in keys:
        w, i = mi.contributions(n, int(np.ceil(n * (1 / scale))), 1 / scale, mi.cubic, 4.0)
        d[f"tab_s{scale}_n{n}_w"], d[f"tab_s{scale}_n{n}_i"] = np.ascontiguousarray(w.squeeze(1)), np.ascontiguousarray(i.squeeze(1))
        assert d[f"tab_s{scale}_n{n}_w"].dtype == np.float64 and d[f"tab_s{scale}_n{n}_i"].dtype == np.int32
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(keys), "tables")


if __name__ == "__main__":
    main()
