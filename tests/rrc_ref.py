"""Host restatement of the resized crop (include/qatvit.h, qatvit_image_batch_rrc): the record's fields, the clamps the kernel applies to a
malformed record, and the result bytes by crop, optional mirror and the NumPy two-pass with one table per axis (tools/gen_resize_golden.py's
``coeffs``).  tools/gen_rrc_golden.py holds it equal to Pillow's crop-then-resize before it writes tests/golden/rrc_kat.npz;
tests/test_rrc_abi.py and tests/test_gpu_rrc.py build their expectations with it."""
import functools
import os

import numpy as np

from tools.gen_resize_golden import BITS, coeffs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rrc_kat.npz")


def pack(top, left, h, w, flip):
    """The two int32 words of one sample: top | left << 16, h | w << 15 | flip << 30."""
    assert 0 <= top <= 0xffff and 0 <= left <= 0xffff and 0 <= h <= 0x7fff and 0 <= w <= 0x7fff
    w0 = np.uint32(top | left << 16).view(np.int32)
    return [int(w0), h | w << 15 | int(bool(flip)) << 30]


def unpack(rec):
    """(top, left, h, w, flip) of a record as stored: every field unsigned, bit 31 of word 1 ignored."""
    w0, w1 = (int(v) & 0xffffffff for v in rec)
    return w0 & 0xffff, w0 >> 16, w1 & 0x7fff, w1 >> 15 & 0x7fff, bool(w1 >> 30 & 1)


def clamped(rec, S):
    """The record the kernel makes of any two words: h, w to [1, S], then top to [0, S - h] and left to [0, S - w]."""
    top, left, h, w, flip = unpack(rec)
    h, w = max(1, min(h, S)), max(1, min(w, S))
    return pack(min(top, S - h), min(left, S - w), h, w, flip)


@functools.lru_cache(maxsize=None)
def _table(n, D):
    return coeffs(n, D)


def _pass(a, n, D):
    """Resample axis 0 of a [n, ...] (uint8) to D with the table of n -> D: int32 accumulators, rounded, shifted and clipped as Pillow does.
    All four taps are taken from a clamped position; a tap the table does not use has coefficient 0."""
    xmin, _, kk = _table(n, D)
    idx = np.minimum(xmin[:, None].astype(np.int64) + np.arange(4), n - 1)                        # [D, 4]
    acc = (a.astype(np.int32)[idx] * kk.reshape(D, 4, *([1] * (a.ndim - 1)))).sum(1, dtype=np.int32) + np.int32(1 << (BITS - 1))
    return np.clip(acc >> BITS, 0, 255).astype(np.uint8)


def resized_crop(image, rec, D):
    """uint8 [D, D, 3] of one uint8 [S, S, 3] image and one VALID record: crop, mirror, horizontal pass (table of w), vertical pass (table of h)."""
    S = image.shape[0]
    top, left, h, w, flip = unpack(rec)
    assert 1 <= h <= S and 1 <= w <= S and top <= S - h and left <= S - w, (rec, S)
    win = image[top:top + h, left:left + w]
    win = win[:, ::-1] if flip else win
    horizontal = np.swapaxes(_pass(np.swapaxes(win, 0, 1), w, D), 0, 1)                           # [h, D, 3]
    return _pass(horizontal, h, D)


def host_rrc(images, records, D):
    """uint8 [B, D, D, 3]: image b through record b."""
    records = np.asarray(records).tolist()
    assert len(images) == len(records)
    return np.stack([resized_crop(a, r, D) for a, r in zip(images, records)])


def load():
    """(images uint8 [K, 32, 32, 3], groups): groups is a list of (D, records int32 [n, 2], image_of int64 [n], pillow uint8 [n, D, D, 3])."""
    with np.load(GOLDEN) as f:
        z = {k: f[k] for k in f.files}
    return z["images"], [(int(d), z[f"records_{d}"], z[f"image_of_{d}"], z[f"out_{d}"]) for d in z["dsts"].tolist()]
