#!/usr/bin/env python3
"""Writes tests/golden/randaug_kat.npz: known answers of the RandAugment stage (qatvit_image_bytes_randaug), made with Pillow.

Per size D in 8, 20, 36: three images built from a seed (tests/randaug_ref.images: random bytes, a narrow-range ramp, a constant channel), a
list of one-layer cases (every op of include/qatvit.h; both resample filters and both signs of every geometric op, a translation beyond the
image, rotations by 0 and 90; the enhance factors 0.1 and 1.9) with their records, and Pillow's bytes of every case on every image, made with
the calls timm makes: ImageOps.*, ImageEnhance.*(img).enhance(f), img.transform(size, AFFINE, m, resample, fillcolor=fill) and
img.rotate(deg, resample, fillcolor=fill).  Chains of two and three layers at D = 36.  At D = 224 four images, the records that
RandAugment.from_config("rand-m9-mstd0.5-inc1").draw gives for a seed, and the SHA-256 of Pillow's bytes.
The host restatement (tests/randaug_ref.py) is checked against Pillow here, byte for byte, for every stored case and for 300 random images
of sizes 8 .. 64 under drawn records, before anything is written.

    python tools/gen_randaug_golden.py            # needs Pillow; rewrites the fixture
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qat_vit_amd  # noqa: E402
from qat_vit_amd.data import RANDAUG_FILL, RANDAUG_OPS, randaug_record  # noqa: E402
from tests import randaug_ref as ref  # noqa: E402

GEOMETRIC = {"ShearX": 0.27, "ShearY": 0.21, "TranslateX": 0.4, "TranslateY": 0.33, "Rotate": 27.0}   # translations: a fraction of D


def cases(D):
    """[(op, value, resample)]: one layer each."""
    out = [("AutoContrast", 0, None), ("Equalize", 0, None), ("Invert", 0, None), ("Posterize", 0, None), ("Posterize", 3, None),
           ("Solarize", 0, None), ("Solarize", 100, None), ("SolarizeAdd", 60, None)]
    out += [(op, f, None) for op in ("Color", "Contrast", "Brightness", "Sharpness") for f in (0.1, 1.9)]
    for op, v in GEOMETRIC.items():
        v = v * D if op.startswith("Translate") else v
        out += [(op, v, "bilinear"), (op, -v, "bicubic")]
    return out + [("TranslateX", 1.5 * D, "bicubic"), ("Rotate", 0.0, "bicubic"), ("Rotate", 90.0, "bilinear")]


def pillow(arr, op, value, resample, matrix=None):
    """What timm's op gives for one uint8 [D, D, 3] image; with `matrix`, a geometric op as the transform of that matrix."""
    from PIL import Image, ImageEnhance, ImageOps

    img = Image.fromarray(arr)
    if op in ("AutoContrast", "Equalize", "Invert"):
        img = getattr(ImageOps, op.lower())(img)
    elif op in ("Posterize", "Solarize"):
        img = getattr(ImageOps, op.lower())(img, int(value))
    elif op == "SolarizeAdd":
        img = img.point([min(255, i + int(value)) if i < 128 else i for i in range(256)] * 3)
    elif op in ("Color", "Contrast", "Brightness", "Sharpness"):
        img = getattr(ImageEnhance, op)(img).enhance(float(value))
    else:
        kw = dict(resample={"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[resample], fillcolor=RANDAUG_FILL)
        if matrix is not None:
            img = img.transform(img.size, Image.AFFINE, tuple(matrix), **kw)
        elif op == "Rotate":
            img = img.rotate(value, **kw)
        else:
            m = {"ShearX": (1, value, 0, 0, 1, 0), "ShearY": (1, 0, 0, value, 1, 0), "TranslateX": (1, 0, value, 0, 1, 0), "TranslateY": (1, 0, 0, 0, 1, value)}[op]
            img = img.transform(img.size, Image.AFFINE, m, **kw)
    return np.asarray(img)


def pillow_records(imgs, records):
    """Pillow on uint8 [B, D, D, 3] under drawn records [B, layers, 16], read back word by word."""
    out = []
    for a, layers in zip(imgs, records):
        for rec in layers:
            if rec[0]:
                op = RANDAUG_OPS[rec[0] - 1]
                value = rec[2:3].view(np.float32)[0] if 7 <= rec[0] <= 10 else rec[1]
                resample = {2: "bilinear", 3: "bicubic"}.get(int(rec[1]))
                a = pillow(a, op, value, resample, rec[4:16].view(np.float64) if rec[0] >= 11 else None)
        out.append(a)
    return np.stack(out)


def main():
    store = {}
    for D in ref.SIZES:
        imgs = ref.images(3, D, 900 + D)
        recs = np.stack([randaug_record(op, v, D, r or "bilinear") for op, v, r in cases(D)])
        want = np.stack([np.stack([pillow(a, op, v, r) for a in imgs]) for op, v, r in cases(D)])
        for k, rec in enumerate(recs):
            got = ref.apply_batch(imgs, np.broadcast_to(rec, (3, 1, 16)))
            assert np.array_equal(got, want[k]), (D, cases(D)[k], np.argwhere(got != want[k])[:4])
        assert cases(D)[1][0] == "Equalize" and np.array_equal(want[1], imgs) == (D == 8)    # 64 pixels: step == 0, the identity
        store.update({f"seed_{D}": 900 + D, f"records_{D}": recs, f"out_{D}": want})
    D = 36
    imgs = ref.images(3, D, 900 + D)
    none = randaug_record(None)
    r = lambda *a: randaug_record(*a[:2], D, *a[2:])   # noqa: E731
    chains = np.stack([np.stack([r("Rotate", 20.0, "bicubic"), r("Equalize"), none]), np.stack([r("AutoContrast"), r("ShearX", -0.2), none]),
                       np.stack([r("Sharpness", 1.7), r("TranslateY", 7.0, "bicubic"), r("Contrast", 1.5)]),
                       np.stack([r("Equalize"), none, r("Color", 0.3)])])
    chain_records = np.stack([chains[(np.arange(3) + s) % 4] for s in range(4)])          # per batch: three samples on three different chains
    chain_out = np.stack([pillow_records(imgs, cr) for cr in chain_records])
    for cr, want in zip(chain_records, chain_out):
        assert np.array_equal(ref.apply_batch(imgs, cr), want)
    store.update(chain_records=chain_records, chain_out=chain_out)

    aug = qat_vit_amd.RandAugment.from_config("rand-m9-mstd0.5-inc1")
    g = torch.Generator().manual_seed(228)                     # an untouched sample, two chains, a bicubic shear
    records = aug.draw(4, 224, g).numpy()
    assert (records[..., 0] > 0).sum() >= 4 and (records[..., 0] >= 11).any() and (records[..., 0] == 0).any()
    big = ref.images(4, 224, 224)
    want = pillow_records(big, records)
    assert np.array_equal(ref.apply_batch(big, records), want)
    store.update(seed_224=224, records_224=records, sha_224=hashlib.sha256(want.tobytes()).hexdigest())

    rng = np.random.default_rng(5)
    three = qat_vit_amd.RandAugment(num_layers=3, prob=0.9, mstd=2.0)
    for k in range(300):
        d = int(rng.integers(2, 17)) * 4
        a = rng.integers(0, 256, (1, d, d, 3), dtype=np.uint8) if k % 3 else ref.images(3, d, k)[1 + k % 2:][:1]
        recs = three.draw(1, d, g).numpy()
        assert np.array_equal(ref.apply_batch(a, recs), pillow_records(a, recs)), (k, d, recs[0, :, :4])
    np.savez_compressed(ref.GOLDEN, **store)
    print(f"{ref.GOLDEN}: {os.path.getsize(ref.GOLDEN)} bytes, {len(cases(8))} cases per size")


if __name__ == "__main__":
    main()
