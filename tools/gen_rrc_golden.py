#!/usr/bin/env python3
"""Writes tests/golden/rrc_kat.npz: known answers of the input pipeline's resized crop (qatvit_image_batch_rrc), made with Pillow.

Four uint8 source images [32, 32, 3] (the kinds of tools/gen_resize_golden.py), and per output size D a list of records (include/qatvit.h:
top | left << 16, h | w << 15 | flip << 30), the image each record is applied to, and what Pillow returns for it:
``Image.fromarray(hflip?(I[top:top+h, left:left+w])).resize((D, D), Image.BICUBIC)`` - crop, THEN resize, which is torchvision's resized_crop
(``resize(box=...)`` of the whole image is another function).  A few records at D = 224, a few dozen at D = 64, so that the file stays under the
1 MiB a committed file may have.  The host restatement (tests/rrc_ref.py) is checked against Pillow here, for every stored case, before anything is
written.

    python tools/gen_rrc_golden.py            # needs Pillow; rewrites the fixture
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import rrc_ref  # noqa: E402
from tools.gen_resize_golden import KINDS, make_image  # noqa: E402

S = 32
# (image, top, left, h, w, flip)
CASES_224 = [(0, 0, 0, 32, 32, False), (1, 7, 20, 17, 9, True), (2, 27, 1, 5, 30, False), (3, 13, 31, 19, 1, True)]


def cases_64(rng):
    """36 records: sides from {1, 2, 3, 4, 5, 31, 32} in 21 pairs with the window in a corner, then 15 drawn ones."""
    vals = (1, 2, 3, 4, 5, S - 1, S)
    out = []
    for j in (0, 2, 5):
        for i, h in enumerate(vals):
            w, k = vals[(i + j) % 7], len(out)
            out.append((k % 4, (S - h) * (k & 1), (S - w) * (k >> 1 & 1), h, w, bool(k >> 2 & 1)))
    for _ in range(15):
        h, w = (int(v) for v in rng.integers(1, S + 1, 2))
        out.append((int(rng.integers(0, 4)), int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w, bool(rng.integers(0, 2))))
    return out


def main():
    import PIL
    from PIL import Image

    rng = np.random.default_rng(20241)
    images = np.stack([make_image(kind, S, rng) for kind in KINDS])
    d = {"images": images, "dsts": np.array([224, 64], np.int32), "pillow_version": np.array(PIL.__version__)}
    for D, cases in ((224, CASES_224), (64, cases_64(rng))):
        records = np.array([rrc_ref.pack(*c[1:]) for c in cases], np.int32)
        image_of = np.array([c[0] for c in cases], np.int64)
        out = []
        for k, top, left, h, w, flip in cases:
            win = images[k][top:top + h, left:left + w]
            win = np.ascontiguousarray(win[:, ::-1] if flip else win)
            out.append(np.asarray(Image.fromarray(win).resize((D, D), Image.BICUBIC)))
        out = np.stack(out)
        assert np.array_equal(out, rrc_ref.host_rrc(images[image_of], records, D)), D
        d[f"records_{D}"], d[f"image_of_{D}"], d[f"out_{D}"] = records, image_of, out
    np.savez_compressed(rrc_ref.GOLDEN, **d)
    assert os.path.getsize(rrc_ref.GOLDEN) < (1 << 20)
    print(f"{rrc_ref.GOLDEN}: {os.path.getsize(rrc_ref.GOLDEN)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
