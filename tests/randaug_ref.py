"""NumPy restatement of the RandAugment stage (qatvit_image_bytes_randaug, include/qatvit.h): Pillow's ImageOps / ImageEnhance / Image.transform
on one uint8 [D, D, 3] image, per 16-word record.  tools/gen_randaug_golden.py checks it against Pillow byte for byte; the tests check it and
the kernel against the fixture that tool writes (tests/golden/randaug_kat.npz)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "randaug_kat.npz")
SIZES = (8, 20, 36)
(AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y,
 ROTATE) = range(1, 16)
BILINEAR, BICUBIC = 2, 3


def images(B, D, seed):
    """uint8 [B, D, D, 3], distinct: random bytes; a ramp with noise in a narrow range (a non-trivial AutoContrast); an image whose green channel
    is constant (the identity branches of AutoContrast and Equalize), then random bytes again."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (B, D, D, 3), dtype=np.uint8)
    if B > 1:
        ramp = np.add.outer(np.arange(D) * 3, np.arange(D) * 2)[..., None] % 120
        a[1] = (40 + ramp + rng.integers(0, 30, (D, D, 3))).astype(np.uint8)
    if B > 2:
        a[2, ..., 1] = 77
    return a


def cleaned(rec):
    """(op, integer argument, np.float32 factor, fill bytes, matrix) of a 16-word record as the kernel cleans it, or None: the identity."""
    rec = np.asarray(rec, dtype=np.int32)
    op, arg = int(rec[0]), int(rec[1])
    factor, matrix = rec[2:3].view(np.float32)[0], rec[4:16].view(np.float64)
    if not 1 <= op <= 15 or (COLOR <= op <= SHARPNESS and not np.isfinite(factor)):
        return None
    if op >= SHEAR_X and (arg not in (BILINEAR, BICUBIC) or not np.isfinite(matrix).all()):
        return None
    arg = min(max(arg, 0), {POSTERIZE: 8, SOLARIZE: 256, SOLARIZE_ADD: 255}.get(op, 1 << 30))
    return op, arg, factor, [int(rec[3]) >> s & 255 for s in (0, 8, 16)], matrix


def luma(a):
    a = a.astype(np.int64)
    return (a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16


def blend(base, a, f):
    """Image.blend(base, a, f): fp32, the product and the sum rounded one by one, clipped, truncated."""
    base, a = np.asarray(base).astype(np.float32), a.astype(np.float32)
    return np.clip(base + np.float32(f) * (a - base), 0, 255).astype(np.uint8)


def lut_of(op, arg, a):
    """int64 [3, 256]: the table of a histogram or pointwise op for image a."""
    i = np.arange(256)
    if op == INVERT:
        return np.tile(255 - i, (3, 1))
    if op == POSTERIZE:
        return np.tile(i & ~(2 ** (8 - arg) - 1) & 255, (3, 1))
    if op == SOLARIZE:
        return np.tile(np.where(i < arg, i, 255 - i), (3, 1))
    if op == SOLARIZE_ADD:
        return np.tile(np.where(i < 128, np.minimum(255, i + arg), i), (3, 1))
    lut = np.tile(i, (3, 1))
    for c in range(3):
        h = np.bincount(a[..., c].ravel(), minlength=256)
        nz = np.nonzero(h)[0]
        if op == AUTOCONTRAST and nz[-1] > nz[0]:
            scale = 255.0 / (nz[-1] - nz[0])
            lut[c] = np.clip((i * scale + -nz[0] * scale).astype(np.int64), 0, 255)
        step = (h.sum() - h[nz[-1]]) // 255
        if op == EQUALIZE and len(nz) > 1 and step:
            lut[c] = np.minimum((step // 2 + np.cumsum(h) - h) // step, 255)
    return lut


def smooth(a):
    """ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13 on the interior, the one-pixel border copied."""
    s = a.astype(np.int64)
    box = sum(s[1 + dy:s.shape[0] - 1 + dy, 1 + dx:s.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    out = a.copy()
    out[1:-1, 1:-1] = np.floor((box + 4 * s[1:-1, 1:-1]) / 13.0 + 0.5)
    return out


def affine(a, m, resample, fill):
    """Image.transform(size, AFFINE, m, resample, fillcolor=fill) in double, one operation at a time."""
    D = a.shape[0]
    y, x = np.meshgrid(np.arange(D) + 0.5, np.arange(D) + 0.5, indexing="ij")
    with np.errstate(all="ignore"):
        xin, yin = (m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5]
        inside = (xin >= 0) & (xin < D) & (yin >= 0) & (yin < D)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x0, y0 = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    src = a.astype(np.float64)
    clip = lambda v: np.clip(v, 0, D - 1)   # noqa: E731
    if resample == BILINEAR:
        line = lambda r: src[r, clip(x0)] + (src[r, clip(x0 + 1)] - src[r, clip(x0)]) * dx   # noqa: E731
        v1 = line(clip(y0))
        v2 = np.where((y0 + 1 < D)[..., None], line(clip(y0 + 1)), v1)
        v = v1 + (v2 - v1) * dy
    else:
        x0, y0 = x0 - 1, y0 - 1

        def cubic(v1, v2, v3, v4, d):
            p2, p3, p4 = -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
            return v2 + d * (p2 + d * (p3 + d * p4))

        line = lambda r: cubic(*(src[r, clip(x0 + k)] for k in range(4)), dx)   # noqa: E731
        rows = [line(clip(y0))]
        for k in (1, 2, 3):
            ok = ((y0 + k >= 0) & (y0 + k < D))[..., None]
            rows.append(np.where(ok, line(clip(y0 + k)), rows[-1]))
        v = np.clip(cubic(*rows, dy), 0, 255)
    return np.where(inside[..., None], v.astype(np.uint8), np.asarray(fill, np.uint8))


def apply(a, rec):
    """One layer on one uint8 [D, D, 3] image."""
    c = cleaned(rec)
    if c is None:
        return a.copy()
    op, arg, f, fill, m = c
    if op >= SHEAR_X:
        return affine(a, m, arg, fill)
    if op == COLOR:
        return blend(luma(a)[..., None], a, f)
    if op == CONTRAST:
        return blend(int(luma(a).sum() / (a.shape[0] * a.shape[1]) + 0.5), a, f)
    if op == BRIGHTNESS:
        return blend(0, a, f)
    if op == SHARPNESS:
        return blend(smooth(a), a, f)
    lut = lut_of(op, arg, a)
    return np.stack([lut[ch][a[..., ch]] for ch in range(3)], -1).astype(np.uint8)


def apply_batch(imgs, records):
    """uint8 [B, D, D, 3] through int32 records [B, layers, 16], the layers in order."""
    out = []
    for a, layers in zip(imgs, np.asarray(records)):
        for rec in layers:
            a = apply(a, rec)
        out.append(a)
    return np.stack(out)
