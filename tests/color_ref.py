"""Host restatement of the colour record (include/qatvit.h, qatvit_image_batch_color): the four words, their cleaned form, and the chain grayscale,
solarize, jitter ops on a uint8 RGB image in NumPy, every float product and sum rounded to fp32 one by one.  tools/gen_color_golden.py holds it
equal to Pillow (ImageOps.solarize, convert("L"), ImageEnhance.Brightness / Contrast / Color, ImageStat) before it writes
tests/golden/color_kat.npz; tests/test_color_abi.py and tests/test_gpu_color.py build their expectations with it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_kat.npz")
NONE, BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2, 3
MASK = 0xFFFFFFFF


def f32_bits(v):
    return int(np.float32(v).view(np.int32))


def _i32(v):
    return int(np.uint32(v & MASK).view(np.int32))


def pack(ops=(), brightness=0.0, contrast=0.0, saturation=0.0, gray=False, solarize=None):
    """The four int32 words of one batch position: `ops` the op codes of slots 0 .. 2 in order, the three factors (fp32), the grayscale bit and
    the solarize threshold (None: off)."""
    assert len(ops) <= 3 and all(0 <= o <= 3 for o in ops) and (solarize is None or 0 <= solarize <= 255)
    w0 = sum(o << 2 * k for k, o in enumerate(ops)) | int(bool(gray)) << 8
    if solarize is not None:
        w0 |= 1 << 9 | int(solarize) << 16
    return [_i32(w0), f32_bits(brightness), f32_bits(contrast), f32_bits(saturation)]


def unpack(rec):
    """((slot 0, slot 1, slot 2), gray, solarize, threshold, (fb, fc, fs) as np.float32) of a record as stored, nothing cleaned."""
    w = [int(v) & MASK for v in rec]
    factors = tuple(np.uint32(v).view(np.float32) for v in w[1:4])
    return (w[0] & 3, w[0] >> 2 & 3, w[0] >> 4 & 3), bool(w[0] >> 8 & 1), bool(w[0] >> 9 & 1), w[0] >> 16 & 255, factors


def _usable(f):
    return bool(f >= 0) and bool(f < np.inf)                       # false for a negative factor, an infinity and a NaN; -0.0 is 0


def cleaned(rec, contrast=True):
    """The record the kernels act on.  A slot whose op code an earlier slot held, and a slot whose op has a negative or non-finite factor, holds
    `none`; so does a contrast slot with contrast=False (the call without sums).  The factor of an op that no slot holds, the threshold without
    the solarize bit and every other bit are zero."""
    slots, gray, sol, thr, factors = unpack(rec)
    seen, out = set(), []
    for op in slots:
        keep = op != NONE and op not in seen and _usable(factors[op - 1]) and (op != CONTRAST or contrast)
        seen.add(op)
        out.append(op if keep else NONE)
    w0 = sum(o << 2 * k for k, o in enumerate(out)) | int(gray) << 8 | (1 << 9 | thr << 16 if sol else 0)
    return [_i32(w0)] + [int(np.float32(f).view(np.int32)) if k + 1 in out else 0 for k, f in enumerate(factors)]


def luma(img):
    """Pillow's convert("L") of uint8 [..., 3] as int32."""
    v = img.astype(np.int32)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def blend(in1, img, a):
    """Pillow's Image.blend(in1, img, a) as ImageEnhance calls it, per channel: in1 an int or an int array that broadcasts against img."""
    a = np.float32(a)
    in1 = np.asarray(in1, dtype=np.int32)
    prod = a * (img.astype(np.int32) - in1).astype(np.float32)       # fl32(a * fl32(in2 - in1))
    t = in1.astype(np.float32) + prod                                 # fl32(fl32(in1) + ...)
    assert prod.dtype == np.float32 and t.dtype == np.float32
    if 0 <= a <= 1:
        return np.trunc(t).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def mean_of(s, pixels):
    """Python's int(s / pixels + 0.5) in integers."""
    return (2 * int(s) + pixels) // (2 * pixels)


def apply(image_u8, rec, contrast=True):
    """(uint8 [D, D, 3], s) of one uint8 [D, D, 3] image through one record: grayscale, solarize, then the cleaned record's ops in slot order.
    s = the sum of the luma over the image as it stands right in front of the contrast op, or 0 where the cleaned record has none."""
    slots, gray, sol, thr, factors = unpack(cleaned(rec, contrast))
    img = np.ascontiguousarray(image_u8, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3
    s = 0
    if gray:
        img = np.repeat(luma(img).astype(np.uint8)[..., None], 3, axis=2)
    if sol:
        img = np.where(img < thr, img, 255 - img).astype(np.uint8)
    for op in slots:
        if op == BRIGHTNESS:
            img = blend(0, img, factors[0])
        elif op == CONTRAST:
            s = int(luma(img).sum())
            img = blend(mean_of(s, img.shape[0] * img.shape[1]), img, factors[1])
        elif op == SATURATION:
            img = blend(luma(img)[..., None], img, factors[2])
    return img, s


def apply_batch(images_u8, records, contrast=True):
    """(uint8 [B, D, D, 3], int64 [B]): image b through record b."""
    records = np.asarray(records).tolist()
    assert len(images_u8) == len(records)
    out = [apply(a, r, contrast) for a, r in zip(images_u8, records)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int64)


def normalized(images_u8, table):
    """fp32 [B, 3, D, D]: the value table [3, 256] (ToTensor() + Normalize()) of uint8 [B, D, D, 3]."""
    table = np.asarray(table, dtype=np.float32)
    return np.stack([table[c][images_u8[..., c]] for c in range(3)], 1)


def load():
    """The fixture: a dict of its arrays (images_36 / images_224, records_*, image_of_*, out_* = Pillow's bytes, means_* = Pillow's int(mean + 0.5)
    in front of the contrast op or -1, and the crafted tie cases tie_*)."""
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}
