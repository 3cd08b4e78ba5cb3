"""Host restatement of the blur record (include/qatvit.h, qatvit_image_batch_blur): the four words, their cleaning rule, and Pillow's
ImageFilter.GaussianBlur on a uint8 RGB image in NumPy - three box passes along the rows, then three along the columns, every pass rounded to uint8
in 32-bit unsigned integers, the edge pixel replicated.  tools/gen_blur_golden.py holds it equal to Pillow before it writes
tests/golden/blur_kat.npz; tests/test_blur_abi.py and tests/test_gpu_blur.py build their expectations with it.  It composes with tests/color_ref.py
by splitting a colour record around the blur: grayscale / solarize in front of it, the jitter ops behind it."""
import os

import numpy as np

from tests import color_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blur_kat.npz")
MAX_RADIUS = 1
NONE = [0, 0, 0, 0]
MASK = 0xFFFFFFFF


def weights(r):
    """(box radius, ww, fw) of the Gaussian radius r, in np.float32 arithmetic as Pillow's C float code."""
    f = np.float32
    r, passes = f(r), f(3)
    sigma2 = r * r / passes
    L = np.sqrt(f(12) * sigma2 + f(1))
    l = np.floor((L - f(1)) / f(2))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2) / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    box = l + a
    assert all(v.dtype == np.float32 for v in (sigma2, L, l, a, box))
    radius = int(box)
    ww = int(f(1 << 24) / (box * f(2) + f(1)))
    return radius, ww, ((1 << 24) - (2 * radius + 1) * ww) // 2


def pack(r):
    """The four int32 words of a sample blurred with the Gaussian radius r."""
    radius, ww, fw = weights(r)
    return [1 | radius << 8, ww, fw, 0]


def cleaned(rec):
    """The record the kernels act on: (radius, ww, fw), or None for "no blur".  Only bit 0 and bits 8..15 of word 0 are read; word 3 is not."""
    w0, ww, fw = int(rec[0]) & MASK, int(rec[1]), int(rec[2])        # ww and fw are signed words
    radius = w0 >> 8 & 255
    ok = w0 & 1 and radius <= MAX_RADIUS and 1 <= ww <= 1 << 24 and fw >= 0 and (2 * radius + 1) * ww + 2 * fw <= 1 << 24
    return (radius, ww, fw) if ok else None


def box_pass(a, radius, ww, fw, axis):
    """One pass along `axis` of uint8 [H, W, C]: out = (ww * sum(|d| <= radius) + fw * (the two at radius + 1) + 2^23) >> 24, taps clamped."""
    n = a.shape[axis]
    v = np.moveaxis(a.astype(np.uint64), axis, 0)
    at = lambda d: v[np.clip(np.arange(n) + d, 0, n - 1)]            # noqa: E731
    inner = sum(at(d) for d in range(-radius, radius + 1))
    acc = ww * inner + fw * (at(-radius - 1) + at(radius + 1)) + (1 << 23)
    assert int(acc.max()) < 1 << 32                                   # fits 32 unsigned bits
    out = acc >> 24
    assert int(out.max()) <= 255
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def blur(image_u8, radius, ww, fw):
    """uint8 [H, W, C] through the six passes."""
    a = np.ascontiguousarray(image_u8, dtype=np.uint8)
    for axis in (1, 1, 1, 0, 0, 0):
        a = box_pass(a, radius, ww, fw, axis)
    return a


def split(color_rec):
    """(front, back) of a colour record: its grayscale / solarize part and its jitter part."""
    w0 = int(color_rec[0]) & MASK
    front = [color_ref._i32(w0 & ~0x3F), 0, 0, 0]
    back = [color_ref._i32(w0 & 0x3F)] + [int(v) for v in color_rec[1:4]]
    return front, back


def apply(image_u8, color_rec, blur_rec, contrast=True):
    """(uint8 [D, D, 3], s) of one image through one colour record and one blur record: grayscale, solarize, blur, the jitter ops.  s = the luma
    sum in front of the contrast op (of the blurred image), or 0."""
    front, back = split(color_rec if color_rec is not None else color_ref.pack())
    img, _ = color_ref.apply(image_u8, front, contrast)
    c = cleaned(blur_rec) if blur_rec is not None else None
    if c is not None:
        img = blur(img, *c)
    return color_ref.apply(img, back, contrast)


def apply_batch(images_u8, color_records, blur_records, contrast=True):
    """(uint8 [B, D, D, 3], int64 [B]): image b through colour record b and blur record b; either list may be None."""
    n = len(images_u8)
    cols = np.asarray(color_records).tolist() if color_records is not None else [None] * n
    blurs = np.asarray(blur_records).tolist() if blur_records is not None else [None] * n
    assert len(cols) == len(blurs) == n
    out = [apply(a, c, b, contrast) for a, c, b in zip(images_u8, cols, blurs)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int64)


def load():
    """The fixture: images_36 / images_224, per size radii_*, image_of_*, weights_* (radius, ww, fw) and out_* = Pillow's bytes; special_images,
    special_radii, special_out: the constant images, the corner impulses and the impulses on rows 15 and 16."""
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}
