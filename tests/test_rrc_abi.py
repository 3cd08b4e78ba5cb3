"""CPU-side checks of the resized crop (qatvit_image_resize_coeffs_windows, qatvit_image_batch_rrc, qat_vit_amd.RandomResizedCrop): the symbols in
the header, the binding and the library; the window tables against the restatement; the restatement against the fixture and, where it is installed,
Pillow; every argument error as a string without a HIP call; the refusals of the Python classes; the drawing rule."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data, native
from tests import rrc_ref
from tools.gen_resize_golden import coeffs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS, BATCH = "qatvit_image_resize_coeffs_windows", "qatvit_image_batch_rrc"


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert decl, f"{name} is not declared in include/qatvit.h"
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_symbols_in_header_signatures_and_exports(native_lib):
    win, batch = _params(WINDOWS), _params(BATCH)
    assert win == ["int32_t src", "int32_t dst", "int32_t* out_host"]
    assert len(batch) == 12 and batch[6:11] == ["const int32_t* windows", "const float* table", "const int32_t* rrc", "const int32_t* mix", "float* out"]
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name, params in ((WINDOWS, win), (BATCH, batch)):
        res, args = native.SIGNATURES[name]
        assert res is native.c_int and len(args) == len(params)
        for p, a in zip(params, args):
            assert a is (native.c_void_p if "*" in p else native.c_int32), (name, p)
        assert name in exported
    assert native_lib.qatvit_abi_version() == 4                      # added symbols: the version stays
    assert "RandomResizedCrop" in qat_vit_amd.__all__


@pytest.mark.parametrize("S,D", [(8, 224), (32, 224), (37, 224), (96, 384)])
def test_window_tables_equal_the_restatement_for_every_side(S, D):
    w = data.resize_window_tables(S, D)
    assert w.dtype == torch.int32 and w.shape == (S, 6 * D) and w.is_contiguous()
    w = w.numpy()
    for n in range(1, S + 1):
        xmin, ntaps, kk = coeffs(n, D)
        assert np.array_equal(w[n - 1, :D], xmin) and np.array_equal(w[n - 1, D:2 * D], ntaps) and np.array_equal(w[n - 1, 2 * D:], kk.ravel()), n
        assert ntaps.max() <= 4 and ntaps.min() >= 1
    assert np.array_equal(w[S - 1], torch.cat([t.flatten() for t in data.resize_tables(S, D)]).numpy())
    # a band of 16 output rows stays within the kernel's row budget for every window height
    budget = (16 * S + D - 1) // D + 5
    for n in range(1, S + 1):
        xmin, ntaps = w[n - 1, :D], w[n - 1, D:2 * D]
        for y0 in range(0, D, 16):
            y1 = min(y0 + 16, D) - 1
            assert xmin[y1] + ntaps[y1] - xmin[y0] <= budget


def test_window_tables_refusals(native_lib):
    L = native_lib
    buf = torch.empty(16, dtype=torch.int32)

    def refused(msg, S, D, out=buf.data_ptr()):
        assert L.qatvit_image_resize_coeffs_windows(S, D, out) != 0
        assert msg in L.qatvit_last_error() and WINDOWS.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    refused(b"null pointer", 32, 224, out=None)
    refused(b"outside 8", 4, 224)
    refused(b"downscaling is not supported", 256, 224)
    refused(b"multiple of 4", 32, 222)
    refused(b"at most 384", 32, 512)
    # the single-table entry keeps its own refusal of a source below 8
    x = torch.empty(224 * 6, dtype=torch.int32)
    assert L.qatvit_image_resize_coeffs(4, 224, x.data_ptr(), x.data_ptr(), x.data_ptr()) != 0 and b"outside 8" in L.qatvit_last_error()
    with pytest.raises(RuntimeError, match="outside 8"):
        data.resize_window_tables(4, 224)


def test_fixture_equals_the_restatement():
    images, groups = rrc_ref.load()
    assert images.shape == (4, 32, 32, 3) and images.dtype == np.uint8 and [g[0] for g in groups] == [224, 64]
    for D, records, image_of, pillow in groups:
        assert records.dtype == np.int32 and records.shape == (len(pillow), 2) and pillow.shape[1:] == (D, D, 3)
        assert np.array_equal(rrc_ref.host_rrc(images[image_of], records, D), pillow)
        for r in records.tolist():
            assert rrc_ref.clamped(r, 32) == r and rrc_ref.pack(*rrc_ref.unpack(r)) == r
    sides = {rrc_ref.unpack(r)[2:4] for r in groups[1][1].tolist()}
    assert len(groups[1][1]) >= 36 and {1, 2, 3, 4, 5, 31, 32} <= {h for h, _ in sides} and {1, 2, 3, 4, 5, 31, 32} <= {w for _, w in sides}


def test_restatement_equals_pillow_crop_then_resize_for_every_window_size():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    for h in range(1, 33):
        for w in range(1, 33):
            top, left, flip = int(rng.integers(0, 33 - h)), int(rng.integers(0, 33 - w)), bool((h + w) & 1)
            win = img[top:top + h, left:left + w]
            win = np.ascontiguousarray(win[:, ::-1] if flip else win)
            want = np.asarray(Image.fromarray(win).resize((224, 224), Image.BICUBIC))
            assert np.array_equal(rrc_ref.resized_crop(img, rrc_ref.pack(top, left, h, w, flip), 224), want), (top, left, h, w, flip)


def test_record_fields_and_clamps():
    assert rrc_ref.pack(3, 5, 7, 9, True) == [3 | 5 << 16, 7 | 9 << 15 | 1 << 30]
    assert rrc_ref.unpack([-1, -1]) == (0xffff, 0xffff, 0x7fff, 0x7fff, True)
    assert rrc_ref.clamped([-1, -1], 32) == rrc_ref.pack(0, 0, 32, 32, True)
    assert rrc_ref.clamped([0, 0], 32) == rrc_ref.pack(0, 0, 1, 1, False)
    assert rrc_ref.clamped(rrc_ref.pack(40, 31, 3, 4, False), 32) == rrc_ref.pack(29, 28, 3, 4, False)
    assert rrc_ref.clamped(rrc_ref.pack(2, 2, 37, 0x7fff, True), 32) == rrc_ref.pack(0, 0, 32, 32, True)


def test_batch_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def refused(msg, data=p, index=None, B=1, N=1, S=32, D=224, windows=p, table=p, rrc=p, mix=p, out=p):
        assert L.qatvit_image_batch_rrc(data, index, B, N, S, D, windows, table, rrc, mix, out, None) != 0
        assert msg in L.qatvit_last_error() and BATCH.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for mix in (p, None):                                            # the sibling entries' checks, with and without mix records
        for name in ("data", "windows", "table", "out"):
            refused(b"null pointer", mix=mix, **{name: None})
        refused(b"rrc is NULL", rrc=None, mix=mix)
        refused(b"downscaling is not supported", S=256, mix=mix)
        refused(b"outside 8", S=4, mix=mix)
        refused(b"multiple of 4", D=222, mix=mix)
        refused(b"at most 384", S=384, D=512, mix=mix)
        refused(b"batch 0", B=0, mix=mix)
        refused(b"batch 65536", B=65536, index=p, mix=mix)
        refused(b"not empty", N=0, mix=mix)
        refused(b"needs an index", B=8, N=4, mix=mix)
        refused(b"misaligned", out=p + 4, mix=mix)
        refused(b"misaligned", windows=p + 2, mix=mix)
        refused(b"misaligned", table=p + 1, mix=mix)
        for off in (1, 2, 3):
            refused(b"misaligned", rrc=p + off, mix=mix)
    for off in (1, 2, 3):
        refused(b"misaligned", mix=p + off)
    # two plane sets of a large source do not fit 64 KB of LDS: an error string, not a launch
    refused(b"bytes of LDS", S=384, D=384)
    refused(b"bytes of LDS", S=300, D=384)


def test_python_wrapper_refusals_without_a_gpu():
    tr = object.__new__(qat_vit_amd.GpuResizeNormalize)               # the constructor needs the GPU; these refusals do not
    tr.src_size, tr.out_size, tr.device = 32, 224, torch.device("cuda", 0)
    imgs, recs = torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(imgs, rrc=recs)
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(imgs, rrc=recs, mix=torch.zeros(2, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="rrc and aug are mutually exclusive"):
        tr(imgs, rrc=recs, aug=torch.zeros(2, dtype=torch.int32))


def test_random_resized_crop_refusals():
    R = qat_vit_amd.RandomResizedCrop
    for scale in ((0, 1), (-0.1, 0.5), (0.5, 0.2), (0.1,), 0.5, (0.1, float("inf")), (float("nan"), 1), ("a", 1), (True, 1), (0.1, 0.5, 1)):
        with pytest.raises(ValueError, match="scale must be"):
            R(scale=scale)
    for ratio in ((0, 1), (2, 1), (1, float("inf")), None, (1, "b"), (0.5, False)):
        with pytest.raises(ValueError, match="ratio must be"):
            R(ratio=ratio)
    for flip in (-0.1, 1.5, "half", float("nan"), True, None):
        with pytest.raises(ValueError, match="flip must be"):
            R(flip=flip)
    a = R()
    assert (a.scale, a.ratio, a.flip) == ((0.08, 1.0), (0.75, 4.0 / 3.0), 0.5)
    b = R(scale=[1, 1], ratio=(1, 1), flip=1)
    assert (b.scale, b.ratio, b.flip) == ((1.0, 1.0), (1.0, 1.0), 1.0)
    for s in (0, -3, 0x8000):
        with pytest.raises(ValueError, match="src_size must be"):
            a.draw(4, s)


def _fields(rec):
    r = rec.to(torch.int64) & 0xffffffff
    return r[:, 0] & 0xffff, r[:, 0] >> 16, r[:, 1] & 0x7fff, r[:, 1] >> 15 & 0x7fff, r[:, 1] >> 30 & 1, r[:, 1] >> 31


@pytest.mark.parametrize("S", [8, 32, 37, 96])
def test_draw_gives_valid_records_by_the_stated_rule(S):
    R = qat_vit_amd.RandomResizedCrop
    n, a = 4096, R()
    r1, r2 = a.draw(n, S, torch.Generator().manual_seed(5)), a.draw(n, S, torch.Generator().manual_seed(5))
    assert r1.dtype == torch.int32 and r1.shape == (n, 2) and not r1.is_cuda and r1.is_contiguous() and torch.equal(r1, r2)
    assert not torch.equal(r1, a.draw(n, S, torch.Generator().manual_seed(6)))
    top, left, h, w, flip, rest = _fields(r1)
    assert bool(((h >= 1) & (h <= S) & (w >= 1) & (w <= S) & (top <= S - h) & (left <= S - w)).all()) and not rest.any() and int(r1.min()) >= 0
    assert 0 < int(flip.sum()) < n and int(h.max()) == S and int(w.max()) == S and int(h.min()) < S // 2 and len(set(zip(h.tolist(), w.tolist()))) > 10
    assert [rrc_ref.clamped(r, S) for r in r1[:64].tolist()] == r1[:64].tolist()
    # the rule itself, restated sample by sample with Python floats
    g = torch.Generator().manual_seed(5)
    u, v = torch.rand(n, 10, 2, dtype=torch.float64, generator=g), torch.rand(n, 3, dtype=torch.float64, generator=g)
    for k in range(256):
        want = None
        for t in range(10):
            area = float(S * S) * (0.08 + float(u[k, t, 0]) * (1.0 - 0.08))
            aspect = float(torch.exp(math.log(0.75) + u[k, t, 1] * (math.log(4.0 / 3.0) - math.log(0.75))))
            ww, hh = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 1 <= ww <= S and 1 <= hh <= S:
                want = (int(math.floor(float(v[k, 0]) * (S - hh + 1))), int(math.floor(float(v[k, 1]) * (S - ww + 1))), hh, ww)
                break
        if want is None:
            want = (0, 0, S, S)
        assert (int(top[k]), int(left[k]), int(h[k]), int(w[k]), bool(flip[k])) == want + (bool(v[k, 2] < 0.5),), k


def test_draw_settings():
    R = qat_vit_amd.RandomResizedCrop
    n, S = 2048, 32
    whole = R(scale=(1, 1), ratio=(1, 1)).draw(n, S, torch.Generator().manual_seed(1))
    top, left, h, w, flip, _ = _fields(whole)
    assert bool(((top == 0) & (left == 0) & (h == S) & (w == S)).all()) and 0 < int(flip.sum()) < n
    for prob, count in ((0, 0), (1, n)):
        assert int(_fields(R(flip=prob).draw(n, S, torch.Generator().manual_seed(1)))[4].sum()) == count
    # a ratio that excludes 1 with a scale no window of that ratio reaches: every try fails, the fallback is the largest centred window of the
    # nearest ratio
    top, left, h, w, _, _ = _fields(R(scale=(0.9, 1.0), ratio=(2.0, 3.0)).draw(n, S, torch.Generator().manual_seed(2)))
    assert bool(((w == S) & (h == 16) & (top == 8) & (left == 0)).all())
    top, left, h, w, _, _ = _fields(R(scale=(0.9, 1.0), ratio=(0.25, 0.4)).draw(n, 37, torch.Generator().manual_seed(2)))
    assert bool(((h == 37) & (w == 15) & (left == 11) & (top == 0)).all())            # round(37 * 0.4) = 15 (14.8)
    # the same ratio with a scale that such a window reaches: tries succeed, and h / w follows the ratio
    top, left, h, w, _, _ = _fields(R(scale=(0.1, 0.3), ratio=(2.0, 3.0)).draw(n, S, torch.Generator().manual_seed(2)))
    assert bool((w > h).all()) and len(set(top.tolist())) > 8
    # the generator advances identically whatever the settings: the next draw from it is the same
    after = []
    for kw in ({}, {"scale": (1, 1), "ratio": (1, 1)}, {"flip": 0}, {"scale": (0.9, 1.0), "ratio": (2.0, 3.0), "flip": 1}):
        g = torch.Generator().manual_seed(9)
        R(**kw).draw(100, S, g)
        after.append(torch.rand(8, generator=g))
    assert all(torch.equal(after[0], t) for t in after[1:])
    assert R().draw(0, S).shape == (0, 2)
    torch.manual_seed(3)                                             # no generator: torch's default one
    d1 = R().draw(50, S)
    torch.manual_seed(3)
    assert torch.equal(d1, R().draw(50, S))


def test_loader_refusals_without_a_gpu():
    tr = object.__new__(qat_vit_amd.GpuResizeNormalize)
    tr.src_size, tr.out_size, tr.device = 8, 224, torch.device("cpu")
    imgs, labels = np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64)
    with pytest.raises(TypeError, match="RandomResizedCrop"):
        qat_vit_amd.GpuImageLoader(imgs, labels, 2, transform=tr, crop="rrc")
    with pytest.raises(ValueError, match="crop and augment are mutually exclusive"):
        qat_vit_amd.GpuImageLoader(imgs, labels, 2, transform=tr, crop=qat_vit_amd.RandomResizedCrop(), augment=qat_vit_amd.RandomCropFlip(2))
