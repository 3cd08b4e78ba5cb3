#!/usr/bin/env python3
"""Writes tests/golden/blur_kat.npz: known answers of the input pipeline's blur record (qatvit_image_batch_blur), made with Pillow.

Four uint8 images [36, 36, 3] (the kinds of tools/gen_resize_golden.py) and one [224, 224, 3]; per size a list of Gaussian radii, the image
each is applied to, the (box radius, ww, fw) the record holds for it and what ``Image.fromarray(a).filter(ImageFilter.GaussianBlur(r))`` returns,
which is what DeiT-III's and timm's GaussianBlur call.  The radii: 0.1, 0.5, 1.0, 2.0 and the two fp32 radii just either side of the step of
the box radius from 0 to 1 (found by bisection; near sqrt(2)).  At D = 224 two radii, to keep the file near half a megabyte.  ``special_*``
at D = 36: the constant images 0 and 255, an impulse in each corner, and impulses on rows 7 and 8 and on rows 15 and 16 (either side of a seam
between two bands of the kernel), each at 0.5, 2.0 and both sides of the step.
The host restatement (tests/blur_ref.py) is checked against Pillow here, byte for byte, for every stored case and for 400 random images of sizes
3 .. 224 at random radii, before anything is written.

    python tools/gen_blur_golden.py            # needs Pillow; rewrites the fixture
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import blur_ref  # noqa: E402
from tools.gen_resize_golden import KINDS, make_image  # noqa: E402

D_SMALL, D_LARGE = 36, 224


def radius_step():
    """(below, above): neighbouring fp32 Gaussian radii whose box radii are 0 and 1."""
    lo, hi = np.float32(1.0), np.float32(2.0)
    assert blur_ref.weights(lo)[0] == 0 and blur_ref.weights(hi)[0] == 1
    while np.nextafter(lo, hi) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        lo, hi = (mid, hi) if blur_ref.weights(mid)[0] == 0 else (lo, mid)
    return float(lo), float(hi)


def pillow_blur(arr, r):
    from PIL import Image, ImageFilter

    return np.asarray(Image.fromarray(arr).filter(ImageFilter.GaussianBlur(radius=float(r))))


def check(arr, r):
    want = pillow_blur(arr, r)
    got = blur_ref.blur(arr, *blur_ref.weights(r))
    assert np.array_equal(got, want), (r, blur_ref.weights(r), np.argwhere(got != want)[:4])
    return want


def special_images():
    imgs = [np.zeros((D_SMALL, D_SMALL, 3), np.uint8), np.full((D_SMALL, D_SMALL, 3), 255, np.uint8)]
    last = D_SMALL - 1
    for y, x in ((0, 0), (0, last), (last, 0), (last, last), (7, 11), (8, 20), (15, 5), (16, 30)):
        a = np.zeros((D_SMALL, D_SMALL, 3), np.uint8)
        a[y, x] = (255, 200, 90)
        imgs.append(a)
    return np.stack(imgs)


def main():
    import PIL

    below, above = radius_step()
    radii = [0.1, 0.5, 1.0, 2.0, below, above]
    rng = np.random.default_rng(20243)
    for _ in range(400):                                             # the restatement against Pillow, beyond what is stored
        h, w = (int(v) for v in rng.integers(3, 225, 2))
        arr = make_image(KINDS[int(rng.integers(0, len(KINDS)))], max(h, w), rng)[:h, :w]
        check(np.ascontiguousarray(arr), float(rng.choice(radii + [float(np.float32(rng.uniform(0.1, 2.0)))] * 6)))
    d = {"pillow_version": np.array(PIL.__version__), "sizes": np.array([D_SMALL, D_LARGE], np.int32), "step": np.array([below, above], np.float32)}
    for D, images, rs in ((D_SMALL, np.stack([make_image(k, D_SMALL, rng) for k in KINDS]), radii * 2),
                          (D_LARGE, make_image("gauss", D_LARGE, rng)[None], [0.5, 2.0])):
        image_of = np.arange(len(rs), dtype=np.int64) % len(images)
        d[f"images_{D}"], d[f"radii_{D}"], d[f"image_of_{D}"] = images, np.array(rs, np.float32), image_of
        d[f"weights_{D}"] = np.array([blur_ref.weights(r) for r in rs], np.int32)
        d[f"out_{D}"] = np.stack([check(images[k], r) for k, r in zip(image_of, rs)])
    sp, sr = special_images(), [0.5, 2.0, below, above]
    d["special_images"], d["special_radii"] = sp, np.array(sr, np.float32)
    d["special_out"] = np.stack([np.stack([check(a, r) for r in sr]) for a in sp])           # [image][radius]
    np.savez_compressed(blur_ref.GOLDEN, **d)
    assert os.path.getsize(blur_ref.GOLDEN) < (1 << 20)
    print(f"{blur_ref.GOLDEN}: {os.path.getsize(blur_ref.GOLDEN)} bytes, step {below!r} / {above!r} -> {blur_ref.weights(below)} / {blur_ref.weights(above)}, "
          f"Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
