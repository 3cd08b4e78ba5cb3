"""CPU-side checks of the augmenting input pipeline (qatvit_image_batch_aug, qat_vit_amd.RandomCropFlip): the symbol in the header, the binding and
the library; every argument error as a string without a HIP call; the drawing rule; the coordinate formula of include/qatvit.h against
np.pad + crop + flip."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from tests import augment_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qatvit_image_batch_aug"


def test_symbol_in_header_signatures_and_exports(native_lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert decl, "not declared in include/qatvit.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 13 and params[8] == "const int32_t* aug" and params[9] == "int32_t padding_mode" and params[10] == "int32_t fill"
    res, args = native.SIGNATURES[NAME]
    assert res is native.c_int and len(args) == len(params)
    for p, a in zip(params, args):                                   # pointers as c_void_p, int32_t as c_int32
        assert a is (native.c_void_p if "*" in p else native.c_int32), p
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4                      # an added symbol: the version stays
    assert "RandomCropFlip" in qat_vit_amd.__all__


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def refused(msg, data=p, index=None, B=1, N=1, S=32, D=224, coeffs=p, table=p, aug=p, mode=0, fill=0, out=p):
        assert L.qatvit_image_batch_aug(data, index, B, N, S, D, coeffs, table, aug, mode, fill, out, None) != 0
        assert msg in L.qatvit_last_error() and NAME.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    # qatvit_image_batch's checks
    for name in ("data", "coeffs", "table", "out"):
        refused(b"null pointer", **{name: None})
    refused(b"downscaling is not supported", S=256)
    refused(b"outside 8", S=4)
    refused(b"multiple of 4", D=222)
    refused(b"at most 384", S=384, D=512)
    refused(b"batch 0", B=0)
    refused(b"batch 65536", B=65536, index=p)
    refused(b"not empty", N=0)
    refused(b"needs an index", B=8, N=4)
    refused(b"misaligned", out=p + 4)
    refused(b"misaligned", coeffs=p + 2)
    refused(b"misaligned", table=p + 1)
    # and its own
    refused(b"misaligned", aug=p + 2)
    refused(b"misaligned", aug=p + 1)
    for mode in (-1, 2, 7):
        refused(b"unknown padding_mode %d" % mode, mode=mode)
    for fill in (-1, 256, 1 << 20):
        refused(b"fill %d is outside 0 .. 255" % fill, fill=fill)
    for aug in (p, None):                                            # a bad mode or fill is refused with and without words
        refused(b"unknown padding_mode", aug=aug, mode=2)
        refused(b"fill 300", aug=aug, fill=300)


def test_python_wrapper_refuses_cpu_tensors():
    tr = object.__new__(qat_vit_amd.GpuResizeNormalize)               # the constructor needs the GPU; the refusal does not
    tr.src_size, tr.out_size, tr.device = 32, 224, torch.device("cuda", 0)
    imgs, words = torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(imgs, aug=words)
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(imgs, aug=words, padding_mode="reflect", fill=3)


def test_random_crop_flip_refusals():
    R = qat_vit_amd.RandomCropFlip
    for kw in ({"padding": -1}, {"padding": 128}, {"padding": 1.5}, {"padding": True}):
        with pytest.raises(ValueError, match="padding must be"):
            R(**kw)
    for kw in ({"flip": -0.1}, {"flip": 1.5}, {"flip": "half"}, {"flip": float("nan")}):
        with pytest.raises(ValueError, match="flip must be"):
            R(**kw)
    for mode in ("edge", "symmetric", 1, None):
        with pytest.raises(ValueError, match="padding_mode must be"):
            R(padding_mode=mode)
    for fill in (-1, 256, 0.5, (0, 0, 0)):
        with pytest.raises(ValueError, match="fill must be"):
            R(fill=fill)
    a = R()
    assert (a.padding, a.flip, a.padding_mode, a.fill) == (4, 0.5, "constant", 0)
    b = R(padding=127, flip=1, padding_mode="reflect", fill=255)
    assert (b.padding, b.flip, b.padding_mode, b.fill) == (127, 1.0, "reflect", 255)
    assert R(padding=0, flip=0).padding == 0


def _fields(words):
    w = words.to(torch.int64)
    signed = lambda v: torch.where(v >= 128, v - 256, v)   # noqa: E731
    return signed(w & 255), signed(w >> 8 & 255), w >> 16 & 1, w >> 17


def test_draw_follows_the_stated_rule():
    R = qat_vit_amd.RandomCropFlip
    n, p = 4096, 4
    a = R(padding=p)
    w1, w2 = a.draw(n, torch.Generator().manual_seed(5)), a.draw(n, torch.Generator().manual_seed(5))
    assert w1.dtype == torch.int32 and w1.shape == (n,) and not w1.is_cuda and w1.is_contiguous() and torch.equal(w1, w2)
    assert not torch.equal(w1, a.draw(n, torch.Generator().manual_seed(6)))
    oy, ox, flip, rest = _fields(w1)
    assert int(oy.min()) == -p == int(ox.min()) and int(oy.max()) == p == int(ox.max())            # both ends occur
    assert 0 < int(flip.sum()) < n and not rest.any() and int(w1.min()) >= 0                      # the unused bits are zero
    # the rule itself: randint for the offsets (row k = [oy, ox]), then rand for the flips
    g = torch.Generator().manual_seed(5)
    off = torch.randint(0, 2 * p + 1, (n, 2), generator=g) - p
    fl = torch.rand(n, generator=g) < 0.5
    assert torch.equal(oy, off[:, 0]) and torch.equal(ox, off[:, 1]) and torch.equal(flip.bool(), fl)
    assert w1.tolist()[:64] == [augment_ref.pack(int(y), int(x), bool(f)) for y, x, f in zip(off[:64, 0], off[:64, 1], fl[:64])]
    assert [augment_ref.unpack(v) for v in w1.tolist()[:64]] == [(int(y), int(x), bool(f)) for y, x, f in zip(off[:64, 0], off[:64, 1], fl[:64])]
    # flip = 0: never; flip = 1: always; p = 0: no offsets; p = 127: the whole signed byte but -128
    for prob, count in ((0, 0), (1, n)):
        _, _, f, rest = _fields(R(padding=p, flip=prob).draw(n, torch.Generator().manual_seed(1)))
        assert int(f.sum()) == count and not rest.any()
    oy, ox, _, rest = _fields(R(padding=0).draw(n, torch.Generator().manual_seed(1)))
    assert not oy.any() and not ox.any() and not rest.any()
    oy, ox, _, rest = _fields(R(padding=127).draw(n, torch.Generator().manual_seed(1)))
    assert -127 <= int(oy.min()) < -100 and 100 < int(ox.max()) <= 127 and not rest.any()
    # the generator advances identically whatever the settings: the next draw from it is the same
    after = []
    for kw in ({"padding": 0}, {"padding": 4}, {"padding": 4, "flip": 0}, {"padding": 127, "flip": 1, "padding_mode": "reflect"}):
        g = torch.Generator().manual_seed(9)
        R(**kw).draw(100, g)
        after.append(torch.rand(8, generator=g))
    assert all(torch.equal(after[0], t) for t in after[1:])
    assert R().draw(0).shape == (0,)
    # no generator: torch's default one
    torch.manual_seed(3)
    d1 = R().draw(50)
    torch.manual_seed(3)
    assert torch.equal(d1, R().draw(50))


@pytest.mark.parametrize("S,p", [(8, 7), (32, 4), (37, 5)])
@pytest.mark.parametrize("mode", ["constant", "reflect"])
def test_coordinate_formula_equals_pad_crop_flip(S, p, mode):
    rng = np.random.default_rng(S)
    img = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    words = augment_ref.corner_words(p)
    assert len(set(words)) == 18
    for fill in ((0, 77) if mode == "constant" else (0,)):
        padded = np.pad(img, ((p, p), (p, p), (0, 0)), mode, **({"constant_values": fill} if mode == "constant" else {}))
        for w in words:
            oy, ox, flip = augment_ref.unpack(w)
            want = padded[oy + p:oy + p + S, ox + p:ox + p + S]
            want = want[:, ::-1] if flip else want
            assert np.array_equal(augment_ref.augmented(img, w, mode, fill), want), (oy, ox, flip, fill)
    batch = augment_ref.host_augmented(np.stack([img] * 18), words, mode, 0)
    assert batch.shape == (18, S, S, 3) and batch.dtype == np.uint8
    assert np.array_equal(batch[8], img) and np.array_equal(batch[9], img[:, ::-1])            # the zero offset: the image, and its mirror


def test_formula_is_defined_for_every_word():
    """Constant mode: a window wholly off the image is all fill.  Reflect mode: the clamp keeps any offset inside the image."""
    img = np.random.default_rng(0).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    for w in (augment_ref.pack(127, 0, False), augment_ref.pack(0, -128, True), augment_ref.pack(-128, 127, False)):
        assert (augment_ref.augmented(img, w, "constant", 77) == 77).all()
        out = augment_ref.augmented(img, w, "reflect")
        assert out.shape == img.shape
    assert np.array_equal(augment_ref.augmented(img, augment_ref.pack(127, 0, False), "reflect"), np.broadcast_to(img[0], (8, 8, 3)))
