#!/usr/bin/env python3
"""Writes tests/golden/wide_kat.npz: known answers of the input pipeline's window stage (qatvit_image_window_u8), made with Pillow.

Per case (H, W) -> D one uint8 source image, a list of records (include/qatvit.h: top | left << 16, h | w << 15 | flip << 30) and what Pillow
returns for each: ``Image.fromarray(hflip?(I[top:top+h, left:left+w])).resize((D, D), Image.BICUBIC)`` - crop, THEN resize, torchvision's
resized_crop.  The small cases are at D = 32 with corner records whose sides lie around D, 2 D and the source's own; one case is 256 x 256 -> 224
(a 0 / 255 noise source, which compresses).  Next to them the tables of a few sides, among them D - 1, D, D + 1, 2 D and 4 D.  The host restatement
(tests/wide_ref.py) is checked against Pillow here for every stored case, for the drawn records the GPU test adds, and for further shapes that
are not stored, before anything is written.

The ``draw_*`` arrays pin ``RandomResizedCrop.draw(n, S)`` for a number S to what it returned BEFORE it learned to take a pair (H, W).  This
tool computes them with that older code: it reads ``qat-vit_amd/data.py`` of the commit DRAW_COMMIT out of git (``git show``), runs the text as a
module of its own and calls its ``RandomResizedCrop`` on tests/wide_ref.py's DRAW_CASES - never with the code under test, which is only
compared.  Where the commit cannot be read (no git history), the arrays of the fixture that exists are carried over, and the tool says so.

    python tools/gen_wide_golden.py [--draw-commit REV]              # needs Pillow; rewrites the fixture
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import wide_ref  # noqa: E402

EXTRA = (((320, 480), 224), ((512, 384), 224), ((225, 223), 224), ((500, 375), 192), ((64, 300), 224), ((896, 640), 224))   # checked, not stored


def pillow(image, rec, D):
    from PIL import Image

    top, left, h, w, flip = wide_ref.unpack(rec)
    win = image[top:top + h, left:left + w]
    win = np.ascontiguousarray(win[:, ::-1] if flip else win)
    return np.asarray(Image.fromarray(win).resize((D, D), Image.BICUBIC))


def drawn_records(H, W, n=16):
    import torch

    import qat_vit_amd

    return qat_vit_amd.RandomResizedCrop().draw(n, (H, W), torch.Generator().manual_seed(1000 * H + W)).tolist()


DRAW_COMMIT = "e62cc61"    # the last commit whose RandomResizedCrop.draw takes a number only


def old_draw_arrays(rev):
    """draw_<name> of every DRAW_CASE from `rev`'s data.py, or None where git cannot show it.  The module's one relative import (the binding of
    the native library, which draw never touches) is replaced by a name that holds nothing."""
    import subprocess
    import types

    import torch

    r = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:qat-vit_amd/data.py"], capture_output=True, text=True)
    if r.returncode != 0:
        return None
    text = r.stdout.replace("from . import native\n", "native = None\n")
    assert "def draw(self, n, src_size, generator=None)" in text and "isinstance(src_size, (tuple, list))" not in text, f"{rev} is not the older code"
    old = types.ModuleType("data_at_" + rev)
    exec(compile(text, f"{rev}:qat-vit_amd/data.py", "exec"), old.__dict__)
    return {f"draw_{name}": old.RandomResizedCrop(scale, ratio).draw(n, S, torch.Generator().manual_seed(seed)).numpy()
            for name, n, S, seed, scale, ratio in wide_ref.DRAW_CASES}


def kept_draw_arrays(path):
    with np.load(path) as f:
        d = {k: f[k] for k in f.files if k.startswith("draw_")}
    missing = [f"draw_{c[0]}" for c in wide_ref.DRAW_CASES if f"draw_{c[0]}" not in d]
    if missing:
        raise SystemExit(f"{path} lacks {missing}, and git cannot show the older code")
    return d


def main():
    import PIL

    ap = argparse.ArgumentParser()
    ap.add_argument("--draw-commit", default=DRAW_COMMIT)
    args = ap.parse_args()
    d = {"pillow_version": np.array(PIL.__version__), "draw_commit": np.array(args.draw_commit)}
    drawn = old_draw_arrays(args.draw_commit)
    if drawn is None:
        print(f"git cannot show {args.draw_commit}: the draw_* arrays of the existing fixture are carried over")
        drawn = kept_draw_arrays(wide_ref.GOLDEN)
    d.update(drawn)
    for (H, W) in wide_ref.SMALL:
        D = wide_ref.D_SMALL
        imgs = wide_ref.images(3, H, W, 100 * H + W)
        stored = wide_ref.corner_records(H, W, D, rotations=(0, 4))
        for k, image in enumerate(imgs):                             # every record the GPU test uses, on every kind of image
            for rec in wide_ref.corner_records(H, W, D) + drawn_records(H, W) + stored:
                assert np.array_equal(pillow(image, rec, D), wide_ref.resized_window(image, rec, D)), (H, W, k, rec)
        d[f"image_{H}_{W}_{D}"], d[f"records_{H}_{W}_{D}"] = imgs[0], np.array(stored, np.int32)
        d[f"out_{H}_{W}_{D}"] = np.stack([pillow(imgs[0], r, D) for r in stored])
    (H, W), D = wide_ref.BIG
    image = wide_ref.images(2, H, W, 7)[1]                           # the 0 / 255 kind
    rec = wide_ref.pack(0, 0, H, W, False)
    d[f"image_{H}_{W}_{D}"], d[f"records_{H}_{W}_{D}"], d[f"out_{H}_{W}_{D}"] = image, np.array([rec], np.int32), pillow(image, rec, D)[None]
    assert np.array_equal(d[f"out_{H}_{W}_{D}"][0], wide_ref.resized_window(image, rec, D))
    for (H, W), D in EXTRA:
        imgs = wide_ref.images(2, H, W, H + W)
        for image, rec in ((imgs[0], wide_ref.pack(0, 0, H, W, False)), (imgs[1], wide_ref.pack(H // 9, W // 7, H - H // 5, W - W // 4, True))):
            assert np.array_equal(pillow(image, rec, D), wide_ref.resized_window(image, rec, D)), (H, W, D, rec)
    for D, sides in wide_ref.TABLE_SIDES.items():
        for n in sides:
            d[f"table_{D}_{n}"] = wide_ref.flat_table(n, D)
    np.savez_compressed(wide_ref.GOLDEN, **d)
    assert os.path.getsize(wide_ref.GOLDEN) < (1 << 20)
    print(f"{wide_ref.GOLDEN}: {os.path.getsize(wide_ref.GOLDEN)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
