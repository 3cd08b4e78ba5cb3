#!/usr/bin/env python3
"""Writes tests/golden/color_kat.npz: known answers of the input pipeline's colour record (qatvit_image_batch_color), made with Pillow.

Four uint8 images [36, 36, 3] (the kinds of tools/gen_resize_golden.py) and one [224, 224, 3], and per size a list of records
(include/qatvit.h: jitter ops in slot order, grayscale, solarize, three factors), the image each record is applied to, what Pillow returns for it
and the mean Pillow's ImageEnhance.Contrast used (-1 where the record has no contrast op).  The Pillow side is what torchvision's transforms call
on a PIL image: ``convert("L")`` (three equal channels) for RandomGrayscale, ``ImageOps.solarize``, ``ImageEnhance.Brightness / Contrast / Color``
``.enhance(f)``, and ``ImageStat.Stat(convert("L")).mean`` for the contrast mean.  At D = 36: each op alone at the factors 0, 0.5, 1, 1.7, 2,
grayscale and solarize alone, all six orders of the three ops, contrast in front of and behind brightness, and grayscale + solarize + three ops.
At D = 224 two records, to keep the file near half a megabyte.  ``tie_*``: grey images of D = 36 whose luma sum s makes s / (D * D) end in
exactly .5 and lie just either side of it, next to 0 and next to 255, and the constant images 0 and 255, through contrast at the factors 0 and 2.
The host restatement (tests/color_ref.py) is checked against Pillow here, byte for byte and mean for mean, for every stored case and for 400
random images of sizes 8 .. 224, before anything is written.

    python tools/gen_color_golden.py            # needs Pillow; rewrites the fixture
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import color_ref  # noqa: E402
from tests.color_ref import BRIGHTNESS as B, CONTRAST as C, SATURATION as S, pack  # noqa: E402
from tools.gen_resize_golden import KINDS, make_image  # noqa: E402

D_SMALL, D_LARGE = 36, 224
FACTORS = (0.0, 0.5, 1.0, 1.7, 2.0)


def records_small():
    recs = [pack((op,), **{name: f}) for op, name in ((B, "brightness"), (C, "contrast"), (S, "saturation")) for f in FACTORS]
    recs += [pack(gray=True), pack(solarize=128), pack(solarize=0), pack(solarize=255)]
    recs += [pack(order, 1.7, 0.5, 2.0) for order in itertools.permutations((B, C, S))]
    recs += [pack((B, C), 1.7, 2.0), pack((C, B), 1.7, 2.0), pack((S, C), contrast=1.7, saturation=0.0)]
    recs += [pack((C, S, B), 0.5, 1.7, 2.0, gray=True, solarize=100), pack((S, B, C), 2.0, 0.5, 1.7, gray=True, solarize=200)]
    return recs


RECORDS_LARGE = [pack((B, S, C), 1.7, 2.0, 0.5, gray=False, solarize=160), pack((C,), contrast=1.7)]


def tie_cases():
    """(image, record) pairs: s = n * k + m of a grey image of n = 36 * 36 pixels, m of them k + 1 and the rest k."""
    n = D_SMALL * D_SMALL
    out = []
    for k, ms in ((0, (0, n // 2 - 1, n // 2, n // 2 + 1)), (254, (n // 2 - 1, n // 2, n // 2 + 1, n)), (127, (n // 2 - 1, n // 2, n // 2 + 1))):
        for m in ms:
            flat = np.full(n, k, np.uint8)
            flat[np.random.default_rng(m).permutation(n)[:m]] = k + 1
            img = np.repeat(flat.reshape(D_SMALL, D_SMALL, 1), 3, axis=2)
            out += [(img, pack((C,), contrast=f)) for f in (0.0, 2.0)]
    return out


def pillow_apply(arr, rec):
    """(bytes, mean) by Pillow, for a VALID record."""
    from PIL import Image, ImageEnhance, ImageOps, ImageStat

    slots, gray, sol, thr, (fb, fc, fs) = color_ref.unpack(rec)
    img, mean = Image.fromarray(arr), -1
    if gray:
        img = img.convert("L").convert("RGB")
    if sol:
        img = ImageOps.solarize(img, thr)
    for op in slots:
        if op == B:
            img = ImageEnhance.Brightness(img).enhance(float(fb))
        elif op == C:
            mean = int(ImageStat.Stat(img.convert("L")).mean[0] + 0.5)
            img = ImageEnhance.Contrast(img).enhance(float(fc))
        elif op == S:
            img = ImageEnhance.Color(img).enhance(float(fs))
    return np.asarray(img), mean


def check(arr, rec):
    got, s = color_ref.apply(arr, rec)
    want, mean = pillow_apply(arr, rec)
    assert np.array_equal(got, want), (rec, np.argwhere(got != want)[:4])
    has = color_ref.CONTRAST in color_ref.unpack(color_ref.cleaned(rec))[0]
    assert (mean >= 0) == has and (not has or color_ref.mean_of(s, arr.shape[0] * arr.shape[1]) == mean), (rec, s, mean)
    return want, mean


def main():
    import PIL

    rng = np.random.default_rng(20242)
    for _ in range(400):                                             # the restatement against Pillow, beyond what is stored
        d = int(rng.integers(8, 225))
        arr = make_image(KINDS[int(rng.integers(0, len(KINDS)))], d, rng)
        f = [float(rng.choice([0.0, 1.0, float(rng.uniform(0, 2))], p=[0.1, 0.1, 0.8])) for _ in range(3)]
        ops = tuple(rng.permutation([B, C, S])[:int(rng.integers(1, 4))].tolist())
        check(arr, pack(ops, *f, gray=bool(rng.integers(0, 4) == 0), solarize=int(rng.integers(0, 256)) if rng.integers(0, 4) == 0 else None))
    d = {"pillow_version": np.array(PIL.__version__), "sizes": np.array([D_SMALL, D_LARGE], np.int32)}
    for D, images, recs in ((D_SMALL, np.stack([make_image(k, D_SMALL, rng) for k in KINDS]), records_small()),
                            (D_LARGE, make_image("gauss", D_LARGE, rng)[None], RECORDS_LARGE)):
        image_of = np.arange(len(recs), dtype=np.int64) % len(images)
        res = [check(images[k], r) for k, r in zip(image_of, recs)]
        d[f"images_{D}"], d[f"records_{D}"], d[f"image_of_{D}"] = images, np.array(recs, np.int32), image_of
        d[f"out_{D}"], d[f"means_{D}"] = np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32)
    ties = tie_cases()
    res = [check(a, r) for a, r in ties]
    d["tie_images"], d["tie_records"] = np.stack([a for a, _ in ties]), np.array([r for _, r in ties], np.int32)
    d["tie_out"], d["tie_means"] = np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32)
    np.savez_compressed(color_ref.GOLDEN, **d)
    assert os.path.getsize(color_ref.GOLDEN) < (1 << 20)
    print(f"{color_ref.GOLDEN}: {os.path.getsize(color_ref.GOLDEN)} bytes, {len(records_small())} + {len(RECORDS_LARGE)} records, {len(ties)} tie cases, "
          f"tie means {d['tie_means'].tolist()}, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
