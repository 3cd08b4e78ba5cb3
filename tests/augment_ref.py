"""Host restatement of the input pipeline's augmentation (include/qatvit.h, qatvit_image_batch_aug): the augmented uint8 image by the coordinate
formula, word by word.  tests/test_augment_abi.py holds it equal to np.pad + crop + flip; tests/test_gpu_augment.py builds its expectations with it."""
import numpy as np


def pack(oy, ox, flip):
    """The int32 word of one sample: bits 0..7 oy, bits 8..15 ox (both signed bytes), bit 16 flip."""
    assert -128 <= oy <= 127 and -128 <= ox <= 127
    return (oy & 255) | (ox & 255) << 8 | int(bool(flip)) << 16


def unpack(word):
    """(oy, ox, flip) of a word."""
    word = int(word)
    signed = lambda v: v - 256 if v >= 128 else v   # noqa: E731
    return signed(word & 255), signed(word >> 8 & 255), bool(word >> 16 & 1)


def corner_words(p):
    """The 18 words {-p, 0, p}^2 x flip."""
    return [pack(oy, ox, f) for oy in (-p, 0, p) for ox in (-p, 0, p) for f in (False, True)]


def augmented(image, word, padding_mode="constant", fill=0):
    """A[y][x][c] = E[y + oy][xf + ox][c], xf = flip ? S-1-x : x, of one uint8 [S, S, 3] image.  E: constant -> `fill` outside [0, S);
    reflect -> u < 0: -u, u > S-1: 2(S-1) - u, then clamped to [0, S-1]."""
    S = image.shape[0]
    oy, ox, flip = unpack(word)
    x = np.arange(S)
    sy, sx = x + oy, (S - 1 - x if flip else x) + ox
    if padding_mode == "constant":
        inside = ((sy >= 0) & (sy < S))[:, None] & ((sx >= 0) & (sx < S))[None, :]
        out = image[np.clip(sy, 0, S - 1)][:, np.clip(sx, 0, S - 1)].copy()
        out[~inside] = fill
        return out
    assert padding_mode == "reflect"

    def reflect(u):
        u = np.where(u < 0, -u, u)
        u = np.where(u > S - 1, 2 * (S - 1) - u, u)
        return np.clip(u, 0, S - 1)

    return image[reflect(sy)][:, reflect(sx)].copy()


def host_augmented(images, words, padding_mode="constant", fill=0):
    """uint8 [B, S, S, 3]: image b augmented by word b."""
    assert len(images) == len(words)
    return np.stack([augmented(a, w, padding_mode, fill) for a, w in zip(images, np.asarray(words).tolist())])
