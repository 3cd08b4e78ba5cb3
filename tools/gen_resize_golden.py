#!/usr/bin/env python3
"""Writes tests/golden/resize_kat.npz and resize_kat_2.npz: known answers of the input pipeline's resize (qat-vit_amd/csrc/image.hip), made with Pillow.

For every source size S and image kind: the uint8 input [S, S, 3] and what ``Image.fromarray(a).resize((D, D), Image.BICUBIC)`` returns for it,
which is what ``transforms.Resize(D, BICUBIC)`` does to a square PIL image.  Next to them the coefficient tables of every S as this file's NumPy
restatement of Pillow's 8-bit resample computes them (``coeffs``); the restatement's two-pass result (``resize``) is checked against Pillow here,
for every stored image, before anything is written.  An expected output that equals another stored array byte for byte (S = D: Pillow returns
the input) is stored once, as ``same_as`` naming that array.  The outputs are 150 KB each and do not compress, so the images of the two larger
sizes go to a second file: each stays under the 1 MiB a committed file may have.  tests/resize_kat.py reads both back as one table.

    python tools/gen_resize_golden.py            # needs Pillow; rewrites the fixture
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "resize_kat.npz")        # settings, the tables of every size, the images of FILE_OF[...] == 0
OUT2 = os.path.join(ROOT, "tests", "golden", "resize_kat_2.npz")
D = 224
SIZES = (32, 64, 96, 224)
FILE_OF = {32: 0, 64: 0, 96: 1, 224: 1}
KINDS = ("uniform", "binary", "white", "gauss")
BITS = 22


def cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(src, dst):
    """xmin [dst], ntaps [dst], coef [dst, 4] (int32; unused taps 0) for src <= dst."""
    assert src <= dst
    scale, support = src / dst, 2.0
    xmin_a, n_a, kk = np.zeros(dst, np.int32), np.zeros(dst, np.int32), np.zeros((dst, 4), np.int32)
    for xx in range(dst):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), src) - xmin
        w = [cubic(i + xmin - center + 0.5) for i in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for i, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            kk[xx, i] = int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS))
        xmin_a[xx], n_a[xx] = xmin, n
    return xmin_a, n_a, kk


def one_pass(img, xmin, ntaps, kk, axis):
    """Resample `axis` (0 or 1) of img [H, W, C] uint8 with the tables; int32 accumulators, uint8 result."""
    img = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((len(xmin),) + img.shape[1:], np.uint8)
    for xx in range(len(xmin)):
        acc = np.full(img.shape[1:], 1 << (BITS - 1), np.int32)
        for i in range(int(ntaps[xx])):
            acc += img[xmin[xx] + i] * np.int32(kk[xx, i])
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, dst, tables=None):
    xmin, ntaps, kk = tables if tables is not None else coeffs(img.shape[0], dst)
    return one_pass(one_pass(img, xmin, ntaps, kk, 1), xmin, ntaps, kk, 0)   # horizontal first; its uint8 rounding is part of the result


def make_image(kind, s, rng):
    if kind == "uniform":
        return rng.integers(0, 256, (s, s, 3), dtype=np.uint8)
    if kind == "binary":                                   # 0 / 255 noise: the cubic overshoots and both passes clip
        return (rng.integers(0, 2, (s, s, 3)) * 255).astype(np.uint8)
    if kind == "white":
        return np.full((s, s, 3), 255, np.uint8)
    return np.clip(rng.normal(128, 60, (s, s, 3)), 0, 255).astype(np.uint8)


def main():
    import PIL
    from PIL import Image

    rng = np.random.default_rng(20240)
    d2 = {}
    d = {"dst": np.int32(D), "sizes": np.array(SIZES, np.int32), "kinds": np.array(KINDS), "pillow_version": np.array(PIL.__version__)}
    for s in SIZES:
        xmin, ntaps, kk = coeffs(s, D)
        d[f"xmin_{s}"], d[f"ntaps_{s}"], d[f"coef_{s}"] = xmin, ntaps, kk
        for kind in KINDS:
            a = make_image(kind, s, rng)
            ref = np.asarray(Image.fromarray(a).resize((D, D), Image.BICUBIC))
            assert np.array_equal(ref, resize(a, D)), (s, kind)
            f = d2 if FILE_OF[s] else d
            f[f"in_{s}_{kind}"] = a
            if np.array_equal(ref, a):
                f[f"same_as_{s}_{kind}"] = np.array(f"in_{s}_{kind}")
            else:
                f[f"out_{s}_{kind}"] = ref
    for path, f in ((OUT, d), (OUT2, d2)):
        np.savez_compressed(path, **f)
        assert os.path.getsize(path) < (1 << 20), path
        print(f"{path}: {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
