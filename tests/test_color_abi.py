"""CPU-side checks of the colour augmentations inside the batch launch (qatvit_image_batch_color, qatvit_image_batch_rrc_color,
qat_vit_amd.ColorJitter): the symbols in the header, the binding and the library; every argument error as a string without a HIP call; the host
restatement tests/color_ref.py against Pillow's bytes and means in tests/golden/color_kat.npz; the clean-up rule of a malformed record; the
refusals and the drawing rule of the Python class."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from tests import color_ref
from tests.color_ref import BRIGHTNESS, CONTRAST, SATURATION, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOR, RRC_COLOR = "qatvit_image_batch_color", "qatvit_image_batch_rrc_color"


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert decl, f"{name} is not declared in include/qatvit.h"
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_symbols_in_header_signatures_and_exports(native_lib):
    co, rrc = _params(COLOR), _params(RRC_COLOR)
    er, rrc_er = _params("qatvit_image_batch_erase"), _params("qatvit_image_batch_rrc_erase")
    tail = ["const int32_t* color", "uint32_t* sums", "float* out", "void* stream"]
    assert co == er[:13] + tail and er[12] == "const int32_t* erase" and len(co) == 17          # the erase entry's arguments up to erase, then these
    assert rrc == rrc_er[:11] + tail and rrc_er[10] == "const int32_t* erase" and len(rrc) == 15
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name, params in ((COLOR, co), (RRC_COLOR, rrc)):
        res, args = native.SIGNATURES[name]
        assert res is native.c_int and len(args) == len(params)
        for p, a in zip(params, args):
            assert a is (native.c_void_p if "*" in p else native.c_int32), (name, p)
        assert name in exported
    assert native_lib.qatvit_abi_version() == 4                      # added symbols: the version stays
    assert "ColorJitter" in qat_vit_amd.__all__ and qat_vit_amd.data.COLOR_WORDS == 4
    hdr = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    assert "fused multiply-add is forbidden" in hdr and "CALLER'S PROMISE THAT NO RECORD HOLDS A CONTRAST OP" in hdr


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def refused(msg, who=None, data=p, index=None, B=1, N=1, S=32, D=224, coeffs=p, table=p, aug=p, mode=0, fill=0, mix=p, erase=p, color=p, sums=p,
                out=p):
        assert L.qatvit_image_batch_color(data, index, B, N, S, D, coeffs, table, aug, mode, fill, mix, erase, color, sums, out, None) != 0
        assert msg in L.qatvit_last_error() and (who or COLOR).encode() in L.qatvit_last_error(), L.qatvit_last_error()

    def refused_rrc(msg, who=None, data=p, index=None, B=1, N=1, S=32, D=224, windows=p, table=p, rrc=p, mix=p, erase=p, color=p, sums=p, out=p):
        assert L.qatvit_image_batch_rrc_color(data, index, B, N, S, D, windows, table, rrc, mix, erase, color, sums, out, None) != 0
        assert msg in L.qatvit_last_error() and (who or RRC_COLOR).encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for color, sums in ((p, p), (p, None), (None, None)):               # with records and a workspace, without the workspace, without records
        for erase in (p, None):
            for mix in (p, None):
                kw = dict(mix=mix, erase=erase, color=color, sums=sums)
                for fn, tab in ((refused, "coeffs"), (refused_rrc, "windows")):
                    for name in ("data", tab, "table", "out"):
                        fn(b"null pointer", **{name: None}, **kw)
                    fn(b"downscaling is not supported", S=256, **kw)
                    fn(b"outside 8", S=4, **kw)
                    fn(b"multiple of 4", D=222, **kw)
                    fn(b"at most 384", S=384, D=512, **kw)
                    fn(b"batch 0", B=0, **kw)                        # color given with a bad B
                    fn(b"batch 65536", B=65536, index=p, **kw)
                    fn(b"not empty", N=0, **kw)
                    fn(b"needs an index", B=8, N=4, **kw)
                    fn(b"misaligned", out=p + 4, **kw)
                    fn(b"misaligned", **{tab: p + 2}, **kw)
                    fn(b"misaligned", table=p + 1, **kw)
                refused(b"unknown padding_mode 2", mode=2, **kw)
                refused(b"fill 256", fill=256, **kw)
                refused(b"fill -1", fill=-1, **kw)
                refused_rrc(b"rrc is NULL", rrc=None, **kw)
                for off in (1, 2, 3):
                    refused(b"misaligned", aug=p + off, **kw)
                    refused_rrc(b"misaligned", rrc=p + off, **kw)
            for off in (1, 2, 3):
                refused(b"misaligned", mix=p + off, erase=erase, color=color, sums=sums)
                refused_rrc(b"misaligned", mix=p + off, erase=erase, color=color, sums=sums)
        for off in (1, 2, 3):
            for mix in (p, None):
                refused(b"misaligned", erase=p + off, mix=mix, color=color, sums=sums)
                refused_rrc(b"misaligned", erase=p + off, mix=mix, color=color, sums=sums)
    for off in (1, 2, 3):                                            # a misaligned color, a misaligned sums
        for fn in (refused, refused_rrc):
            for sums in (p, None):
                fn(b"misaligned", color=p + off, sums=sums)
            fn(b"misaligned", sums=p + off)
            fn(b"misaligned", sums=p + off, color=None)
    # two plane sets of a large source do not fit 64 KB of LDS: an error string, not a launch; without colour records the sibling's own refusal
    refused(b"bytes of LDS", S=384, D=384)
    refused(b"bytes of LDS", S=300, D=384, aug=None, erase=None, sums=None)
    refused(b"bytes of LDS", who="qatvit_image_batch_erase", S=384, D=384, color=None)
    refused(b"bytes of LDS", who="qatvit_image_batch_mix", S=384, D=384, color=None, erase=None)
    refused_rrc(b"bytes of LDS", S=384, D=384)
    refused_rrc(b"bytes of LDS", S=300, D=384, erase=None)
    refused_rrc(b"bytes of LDS", who="qatvit_image_batch_rrc_erase", S=384, D=384, color=None)
    refused_rrc(b"bytes of LDS", who="qatvit_image_batch_rrc", S=384, D=384, color=None, erase=None)


def test_color_ref_equals_pillows_bytes_and_means():
    z = color_ref.load()
    assert z["sizes"].tolist() == [36, 224] and len(z["records_36"]) >= 28 and len(z["records_224"]) >= 1
    seen_orders, seen_factors = set(), set()
    for d in (36, 224):
        images, recs, image_of = z[f"images_{d}"], z[f"records_{d}"].tolist(), z[f"image_of_{d}"]
        assert images.shape[1:] == (d, d, 3) and images.dtype == np.uint8
        for k, rec in enumerate(recs):
            assert color_ref.cleaned(rec) == rec                     # the fixture's records are valid
            got, s = color_ref.apply(images[image_of[k]], rec)
            assert np.array_equal(got, z[f"out_{d}"][k]), (d, k)
            slots, gray, sol, thr, f = color_ref.unpack(rec)
            if CONTRAST in slots:
                assert color_ref.mean_of(s, d * d) == int(z[f"means_{d}"][k]), (d, k)
            else:
                assert s == 0 and int(z[f"means_{d}"][k]) == -1
            ops = tuple(o for o in slots if o)
            if len(ops) == 3:
                seen_orders.add(ops)
            if len(ops) == 1:
                seen_factors.add((ops[0], float(f[ops[0] - 1])))
    assert seen_orders == set(itertools.permutations((BRIGHTNESS, CONTRAST, SATURATION)))
    assert seen_factors == {(op, float(np.float32(f))) for op in (1, 2, 3) for f in (0, 0.5, 1, 1.7, 2)}
    # the crafted ties: s / (D * D) exactly .5 and either side of it, next to 0, 127 and 255, at the factors 0 and 2
    n, fracs = 36 * 36, set()
    for img, rec, want, mean in zip(z["tie_images"], z["tie_records"].tolist(), z["tie_out"], z["tie_means"].tolist()):
        got, s = color_ref.apply(img, rec)
        assert np.array_equal(got, want) and color_ref.mean_of(s, n) == mean == int(s / n + 0.5)
        fracs.add((s // n, s % n))
        if color_ref.unpack(rec)[4][1] == 0:
            assert bool((got == mean).all())                         # factor 0: the mean itself, everywhere
    assert {(0, 0), (0, n // 2 - 1), (0, n // 2), (0, n // 2 + 1), (254, n // 2), (254, n // 2 - 1), (254, n // 2 + 1), (255, 0), (127, n // 2)} <= fracs


def test_formulas_at_single_pixels():
    px = lambda r, g, b: np.array([[[r, g, b]]], np.uint8)   # noqa: E731
    assert int(color_ref.luma(px(255, 255, 255))[0, 0]) == 255 and int(color_ref.luma(px(255, 0, 0))[0, 0]) == 76
    assert color_ref.apply(px(10, 200, 128), pack(solarize=128))[0].tolist() == [[[10, 55, 127]]]
    assert color_ref.apply(px(10, 200, 30), pack(gray=True))[0].tolist() == [[[124, 124, 124]]]
    assert color_ref.apply(px(10, 200, 30), pack((BRIGHTNESS,), 2.0))[0].tolist() == [[[20, 255, 60]]]
    assert color_ref.apply(px(10, 200, 30), pack((SATURATION,), saturation=0.0))[0].tolist() == [[[124, 124, 124]]]
    out, s = color_ref.apply(px(10, 200, 30), pack((CONTRAST,), contrast=0.0))
    assert s == 124 and out.tolist() == [[[124, 124, 124]]]
    # the two roundings, one by one: a = 1.7, in1 = 37, v = 172: fl(1.7f * 135) = 229.5 exactly after rounding, + 37 = 266.5 -> clipped
    assert color_ref.blend(37, px(172, 38, 0), 1.7).tolist() == [[[255, 38, 0]]]
    assert color_ref.mean_of(648, 1296) == 1 and color_ref.mean_of(647, 1296) == 0 and color_ref.mean_of(255 * 384 * 384, 384 * 384) == 255


def test_a_malformed_record_is_cleaned():
    f = color_ref.f32_bits
    good = pack((CONTRAST, BRIGHTNESS, SATURATION), 1.5, 0.5, 2.0, gray=True, solarize=77)
    assert color_ref.cleaned(good) == good
    # repeated op codes: the later slot is skipped, the earlier one stays
    assert color_ref.cleaned(pack((BRIGHTNESS, BRIGHTNESS, CONTRAST), 1.5, 0.5)) == pack((BRIGHTNESS, 0, CONTRAST), 1.5, 0.5)
    assert color_ref.cleaned(pack((SATURATION, CONTRAST, SATURATION), 0, 0.5, 2.0)) == pack((SATURATION, CONTRAST, 0), 0, 0.5, 2.0)
    assert color_ref.cleaned(pack((CONTRAST, CONTRAST, CONTRAST), contrast=0.5)) == pack((CONTRAST,), contrast=0.5)
    # stray bits: bits 6-7, 10-15 and 24-31 of word 0, the threshold without the solarize bit, the factor of an op that no slot holds
    stray = [good[0] | 0xC0 | 0xFC00 | -(1 << 24), good[1], good[2], good[3]]
    assert color_ref.cleaned(stray) == good
    assert color_ref.cleaned([200 << 16, f(3.0), f(-1.0), f(float("nan"))]) == [0, 0, 0, 0]
    # negative, infinite and NaN factors: the op is the identity, its neighbours stay
    for bad in (-0.5, float("inf"), float("-inf"), float("nan")):
        assert color_ref.cleaned(pack((BRIGHTNESS, CONTRAST, SATURATION), 1.5, bad, 2.0)) == pack((BRIGHTNESS, 0, SATURATION), 1.5, 0.0, 2.0)
        assert color_ref.cleaned(pack((BRIGHTNESS,), bad)) == [0, 0, 0, 0]
    assert color_ref.cleaned([-1, -1, -1, -1]) == [color_ref._i32(1 << 8 | 1 << 9 | 255 << 16), 0, 0, 0]     # all bits set: op 3 thrice, factors NaN
    assert color_ref.cleaned(pack((BRIGHTNESS,), -0.0)) == pack((BRIGHTNESS,), -0.0)                          # -0.0 is 0, not negative
    # without a workspace (sums == NULL) contrast is the identity
    assert color_ref.cleaned(good, contrast=False) == pack((0, BRIGHTNESS, SATURATION), 1.5, 0.0, 2.0, gray=True, solarize=77)
    img = np.random.default_rng(3).integers(0, 256, (12, 12, 3), dtype=np.uint8)
    for rec in (stray, [-1] * 4, pack((BRIGHTNESS, BRIGHTNESS, CONTRAST), 1.5, 0.5), pack((SATURATION, CONTRAST), 0, float("nan"), 0.3)):
        a, b = color_ref.apply(img, rec), color_ref.apply(img, color_ref.cleaned(rec))
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert color_ref.apply(img, pack((SATURATION, CONTRAST), 0, float("nan"), 0.3))[1] == 0
    assert np.array_equal(color_ref.apply(img, [0] * 4)[0], img) and np.array_equal(color_ref.apply(img, pack((1, 2, 3), 1, 1, 1))[0], img)


def test_color_jitter_refusals_and_ranges():
    J = qat_vit_amd.ColorJitter
    for hue in (0.1, (0, 0), (-0.1, 0.1), "0", None, True):
        with pytest.raises(ValueError, match="hue is not supported"):
            J(hue=hue)
    for name in ("brightness", "contrast", "saturation"):
        for bad in (-0.1, (0.5,), (1.2, 0.8), (-0.1, 1.0), (0.5, float("inf")), float("nan"), "0.4", None, True, (0.5, "a"), (1, 2, 3)):
            with pytest.raises(ValueError, match=f"{name} must be"):
                J(**{name: bad})
    for name in ("grayscale", "solarize"):
        for bad in (-0.1, 1.5, "half", float("nan"), True, None):
            with pytest.raises(ValueError, match=f"{name} must be a probability"):
                J(**{name: bad})
    for bad in (-1, 256, 128.0, True, None):
        with pytest.raises(ValueError, match="solarize_threshold must be"):
            J(solarize_threshold=bad)
    a = J()
    assert (a.brightness, a.contrast, a.saturation, a.grayscale, a.solarize, a.solarize_threshold) == (None, None, None, 0.0, 0.0, 128)
    assert not a.draw(64, torch.Generator().manual_seed(1)).any()    # nothing enabled: identity records
    assert J(0.4).brightness == (0.6, 1.4) and J(contrast=1.5).contrast == (0.0, 2.5) and J(saturation=(0.2, 0.3)).saturation == (0.2, 0.3)
    assert J(brightness=(1, 1)).brightness is None and J(brightness=(0, 0)).brightness == (0.0, 0.0) and J(hue=0.0).contrast is None
    assert J().draw(0).shape == (0, 4)


def test_draw_gives_records_by_the_stated_rule():
    J = qat_vit_amd.ColorJitter
    n = 4096
    a = J(0.4, (0.5, 0.5), 1.5, grayscale=0.1, solarize=0.2, solarize_threshold=130)
    r1, r2 = a.draw(n, torch.Generator().manual_seed(5)), a.draw(n, torch.Generator().manual_seed(5))
    assert r1.dtype == torch.int32 and r1.shape == (n, 4) and not r1.is_cuda and r1.is_contiguous() and torch.equal(r1, r2)
    assert not torch.equal(r1, a.draw(n, torch.Generator().manual_seed(6)))
    assert [color_ref.cleaned(r) for r in r1[:256].tolist()] == r1[:256].tolist()
    # the rule itself, restated sample by sample
    g = torch.Generator().manual_seed(5)
    order = torch.rand(n, 3, dtype=torch.float64, generator=g).argsort(1)
    f = torch.rand(n, 3, dtype=torch.float64, generator=g)
    p = torch.rand(n, 2, dtype=torch.float64, generator=g)
    lo, hi = (0.6, 0.5, 0.0), (1.4, 0.5, 2.5)
    for s in range(256):
        fac = [np.float32(lo[j] + float(f[s, j]) * (hi[j] - lo[j])) for j in range(3)]
        want = pack(tuple(int(o) + 1 for o in order[s]), *fac, gray=bool(p[s, 0] < 0.1), solarize=130 if bool(p[s, 1] < 0.2) else None)
        assert r1[s].tolist() == want, s
    orders, gray, sol = {}, 0, 0
    for rec in r1.tolist():
        slots, gy, so, thr, fac = color_ref.unpack(rec)
        orders[slots] = orders.get(slots, 0) + 1
        gray, sol = gray + gy, sol + so
        assert 0.6 <= fac[0] <= 1.4 and fac[1] == 0.5 and 0 <= fac[2] <= 2.5 and thr == (130 if so else 0)
    assert set(orders) == set(itertools.permutations((1, 2, 3)))     # every order of the enabled ops appears, each near n / 6
    assert all(abs(c - n / 6) < 5 * math.sqrt(n * (1 / 6) * (5 / 6)) for c in orders.values())
    assert abs(gray - 0.1 * n) < 5 * math.sqrt(n * 0.1 * 0.9) and abs(sol - 0.2 * n) < 5 * math.sqrt(n * 0.2 * 0.8)
    fb = r1[:, 1].contiguous().view(torch.float32).double()
    assert abs(float(fb.mean()) - 1.0) < 5 * 0.8 / math.sqrt(12 * n) and float(fb.min()) < 0.61 and float(fb.max()) > 1.39
    # two ops enabled: both orders, in the first two slots, the third slot and the disabled op's factor word zero
    two = J(brightness=0.4, saturation=0.4).draw(n, torch.Generator().manual_seed(7))
    got = {}
    for rec in two.tolist():
        slots = color_ref.unpack(rec)[0]
        got[slots] = got.get(slots, 0) + 1
        assert rec[2] == 0
    assert set(got) == {(1, 3, 0), (3, 1, 0)} and all(abs(c - n / 2) < 5 * math.sqrt(n / 4) for c in got.values())
    assert bool((J(grayscale=1, solarize=1).draw(50)[:, 0] == (1 << 8 | 1 << 9 | 128 << 16)).all())
    # the generator advances identically whatever the settings: its position depends on n only
    after = []
    for kw in ({}, {"brightness": 0.4}, {"contrast": 0.3, "grayscale": 1.0}, {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4, "solarize": 0.5}):
        g = torch.Generator().manual_seed(9)
        J(**kw).draw(100, g)
        after.append(torch.rand(8, generator=g))
    assert all(torch.equal(after[0], t) for t in after[1:])
    g = torch.Generator().manual_seed(9)
    J().draw(101, g)
    assert not torch.equal(after[0], torch.rand(8, generator=g))
    torch.manual_seed(3)                                             # no generator: torch's default one
    d1 = a.draw(50)
    torch.manual_seed(3)
    assert torch.equal(d1, a.draw(50))


def test_wrapper_and_loader_refusals_without_a_gpu():
    tr = object.__new__(qat_vit_amd.GpuResizeNormalize)               # the constructor needs the GPU; these refusals do not
    tr.src_size, tr.out_size, tr.device = 32, 224, torch.device("cuda", 0)
    imgs, recs = torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 4, dtype=torch.int32)
    for kw in ({}, {"aug": torch.zeros(2, dtype=torch.int32)}, {"rrc": torch.zeros(2, 2, dtype=torch.int32)}, {"erase": torch.zeros(2, 8, dtype=torch.int32)}):
        with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
            tr(imgs, color=recs, **kw)
    tr.device = torch.device("cpu")
    np_imgs, labels = np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64)
    tr.src_size = 8
    for bad in ("jitter", 0.4, qat_vit_amd.RandomErasing(), (0.4, 0.4, 0.4)):
        with pytest.raises(TypeError, match="color must be a ColorJitter"):
            qat_vit_amd.GpuImageLoader(np_imgs, labels, 2, transform=tr, color=bad)
    ok = qat_vit_amd.GpuImageLoader(np_imgs, labels, 2, transform=tr, color=qat_vit_amd.ColorJitter(0.4, 0.4, 0.4), erase=qat_vit_amd.RandomErasing(),
                                    mix=qat_vit_amd.MixupCutmix(), crop=qat_vit_amd.RandomResizedCrop())
    assert isinstance(ok.color, qat_vit_amd.ColorJitter) and len(ok) == 2
