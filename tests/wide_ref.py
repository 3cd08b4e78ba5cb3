"""Host restatement of the window stage (include/qatvit.h, qatvit_image_window_u8): Pillow's 8-bit bicubic tables for any n -> D with the
filter stretched where n > D, the clamps the kernel applies to a malformed record of an H x W source, and the result bytes by crop, optional
mirror and the NumPy two-pass with one table per axis.  tools/gen_wide_golden.py holds it equal to Pillow's crop-then-resize for every stored
case (and more) before it writes tests/golden/wide_kat.npz; tests/test_wide_abi.py and tests/test_gpu_wide.py build their expectations with it."""
import functools
import os

import numpy as np

from tests.rrc_ref import pack, unpack  # noqa: F401  (the record is qatvit_image_batch_rrc's)
from tools.gen_resize_golden import BITS, cubic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_kat.npz")
K = 17                                                               # taps per output at n <= 4 D: support <= 8
SMALL = ((64, 48), (37, 128), (20, 100), (128, 128), (33, 31))       # (H, W) of the D = 32 cases
D_SMALL = 32
BIG = ((256, 256), 224)
TABLE_SIDES = {32: (1, 8, 31, 32, 33, 64, 100, 128), 224: (223, 224, 225, 448, 896)}
# RandomResizedCrop.draw(n, S) for a number S, pinned: (name, n, S, seed, scale, ratio)
DRAW_CASES = (("default", 64, 32, 1, (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)), ("wide_ratio", 64, 37, 2, (0.5, 1.0), (2.0, 3.0)),
              ("tall_ratio", 64, 224, 3, (0.6, 1.0), (0.2, 0.4)), ("big", 48, 224, 4, (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)))


@functools.lru_cache(maxsize=None)
def tables(n, D):
    """xmin [D], ntaps [D], coef [D, 17] (int32; unused taps 0) of n -> D, 1 <= n <= 4 D: the recipe of include/qatvit.h, all in double."""
    assert 1 <= n <= 4 * D
    scale = n / D
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    xmin_a, n_a, kk = np.zeros(D, np.int32), np.zeros(D, np.int32), np.zeros((D, K), np.int32)
    for xx in range(D):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        nt = min(int(center + support + 0.5), n) - xmin
        assert 1 <= nt <= K
        w = [cubic((i + xmin - center + 0.5) * ss) for i in range(nt)]
        ww = 0.0
        for v in w:
            ww += v
        for i, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            kk[xx, i] = int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS))
        xmin_a[xx], n_a[xx] = xmin, nt
    return xmin_a, n_a, kk


def flat_table(n, D):
    """int32 [19 * D]: the table of n -> D as qatvit_image_window_coeffs lays it out."""
    return np.concatenate([t.reshape(-1) for t in tables(n, D)])


def clamped(rec, H, W):
    """The record the kernel makes of any two words: h to [1, H], w to [1, W], then top to [0, H - h] and left to [0, W - w]."""
    top, left, h, w, flip = unpack(rec)
    h, w = max(1, min(h, H)), max(1, min(w, W))
    return pack(min(top, H - h), min(left, W - w), h, w, flip)


def _pass(a, n, D):
    """Resample axis 0 of a [n, ...] (uint8) to D with the table of n -> D: every tap from a clamped position (a tap the table does not use has
    coefficient 0), the sum checked to stay inside int32, rounded, shifted and clipped as Pillow does."""
    xmin, _, kk = tables(n, D)
    idx = np.minimum(xmin[:, None].astype(np.int64) + np.arange(K), n - 1)                        # [D, K]
    acc = (a.astype(np.int64)[idx] * kk.astype(np.int64).reshape(D, K, *([1] * (a.ndim - 1)))).sum(1) + (1 << (BITS - 1))
    assert acc.min() >= -(1 << 31) and acc.max() < (1 << 31)
    return np.clip(acc >> BITS, 0, 255).astype(np.uint8)


def resized_window(image, rec, D):
    """uint8 [D, D, 3] of one uint8 [H, W, 3] image and one VALID record: crop, mirror, horizontal pass (table of w), vertical pass (table of h)."""
    H, W = image.shape[:2]
    top, left, h, w, flip = unpack(rec)
    assert 1 <= h <= H and 1 <= w <= W and top <= H - h and left <= W - w, (rec, H, W)
    win = image[top:top + h, left:left + w]
    win = win[:, ::-1] if flip else win
    horizontal = np.swapaxes(_pass(np.swapaxes(win, 0, 1), w, D), 0, 1)                           # [h, D, 3]
    return _pass(horizontal, h, D)


def host_window(images, records, D):
    """uint8 [B, D, D, 3]: image b through record b."""
    records = np.asarray(records).tolist()
    assert len(images) == len(records)
    return np.stack([resized_window(a, r, D) for a, r in zip(images, records)])


def side_values(side, D):
    """The window sides of the corner records on an axis of `side` pixels: 1, 2, 3, around D, 2 D and the two largest, where they fit."""
    return sorted({v for v in (1, 2, 3, D - 1, D, D + 1, 2 * D, side - 1, side) if 1 <= v <= side})


def corner_records(H, W, D, rotations=(0, 2, 5)):
    """Per rotation one record for every value of the longer of the two value lists, every h with changing w: the window in the four corners
    (top and left at 0 and at their maximum) and both flip values in turn."""
    hv, wv = side_values(H, D), side_values(W, D)
    out = []
    for j in rotations:
        for i in range(max(len(hv), len(wv))):
            h, w, k = hv[i % len(hv)], wv[(i + j) % len(wv)], len(out)
            out.append(pack((H - h) * (k & 1), (W - w) * (k >> 1 & 1), h, w, bool(k >> 2 & 1)))
    return out


def images(n, H, W, seed):
    """n uint8 [H, W, 3] images, three kinds in turn: uniform noise, 0 / 255 noise (both passes clip), clipped gaussian."""
    rng = np.random.default_rng(seed)
    kinds = (lambda: rng.integers(0, 256, (H, W, 3), dtype=np.uint8), lambda: (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8),
             lambda: np.clip(rng.normal(128, 60, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack([kinds[i % 3]() for i in range(n)])


def load():
    """The fixture as a dict of arrays.  Per case `H_W_D`: ``image_*`` uint8 [H, W, 3], ``records_*`` int32 [n, 2], ``out_*`` uint8 [n, D, D, 3]
    (Pillow's); ``table_D_n`` int32 [19 * D]; ``draw_<name>`` int32 [n, 2]."""
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}
