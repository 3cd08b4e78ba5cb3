"""CPU-side checks of the window stage (qatvit_image_window_coeffs, qatvit_image_window_u8, GpuWindowResize / GpuWideResizeNormalize): the
symbols; the host builder against the restatement (tests/wide_ref.py), the stored tables and, for n <= D, qatvit_image_resize_coeffs; the
restatement against the stored Pillow bytes; every argument error as a string without a HIP call; RandomResizedCrop.draw for a number S pinned
to the tensor it gave before it took a pair, and the rule for a pair; center_crop_window; the wide transform's refusals."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data, distill, native
from tests import wide_ref
from tests.test_rrc_abi import _fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFFS, BYTES, WINDOW = "qatvit_image_window_coeffs", "qatvit_image_window_coeffs_bytes", "qatvit_image_window_u8"
K = wide_ref.K


def test_symbols_in_header_signatures_and_exports(native_lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name, res, count in ((COEFFS, "int", 3), (BYTES, "int64_t", 2), (WINDOW, "int", 12)):
        decl = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), hdr)
        assert decl, name
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        r, args = native.SIGNATURES[name]
        assert len(params) == len(args) == count and r is (native.c_int64 if res == "int64_t" else native.c_int)
        for p, a in zip(params, args):
            assert a is (native.c_void_p if "*" in p else native.c_int32), (name, p)
        assert name in exported
    assert native_lib.qatvit_abi_version() == 4                      # added symbols: the version stays
    assert {"GpuWindowResize", "GpuWideResizeNormalize", "center_crop_window"} <= set(qat_vit_amd.__all__)
    assert data.WINDOW_TAPS == K and data.RRC_WORDS == 2


@pytest.mark.parametrize("max_side,D", [(128, 32), (96, 24), (260, 224)])
def test_builder_equals_the_restatement_for_every_side(max_side, D):
    t = data.window_stage_tables(max_side, D)
    assert t.dtype == torch.int32 and t.shape == (max_side, (2 + K) * D) and t.is_contiguous()
    assert native.lib().qatvit_image_window_coeffs_bytes(max_side, D) == t.numel() * 4
    t = t.numpy()
    for n in (range(1, max_side + 1) if D < 224 else (1, 2, 7, 8, 100, 223, 224, 225, 256, 260)):
        xmin, ntaps, kk = wide_ref.tables(n, D)
        assert np.array_equal(t[n - 1], wide_ref.flat_table(n, D)), n
        coef = t[n - 1, 2 * D:].reshape(D, K)
        assert all(not coef[x, ntaps[x]:].any() for x in range(D))                       # coefficients past ntaps are zero
        bound = _tap_bound(n, D)                                                       # the taps the kernel takes: nothing behind them
        assert ntaps.max() <= min(K, bound + 1) and ntaps.min() >= 1 and not coef[:, bound:].any(), n
        assert np.abs(kk).max() < 1 << 23
        assert 255 * np.maximum(kk, 0).sum(1).max() + (1 << 21) < 1 << 31 and 255 * np.maximum(-kk, 0).sum(1).max() < 1 << 31
        # a band of 8 output rows stays within the rows the kernel keeps for a window of this height
        scale = n / D
        budget = min(n, math.ceil(7 * scale + 4.0 * max(scale, 1.0)) + 2)
        assert budget <= 50
        for y0 in range(0, D, 8):
            y1 = min(y0 + 8, D) - 1
            assert xmin[y1] + ntaps[y1] - xmin[y0] <= budget, (n, y0)


@pytest.mark.parametrize("D", [32, 224])
def test_builder_equals_the_stored_tables_and_the_four_tap_builder(D):
    z = wide_ref.load()
    sides = wide_ref.TABLE_SIDES[D]
    assert {D - 1, D, D + 1, 2 * D, 4 * D} <= set(sides)
    t = data.window_stage_tables(4 * D, D).numpy()
    for n in sides:
        assert np.array_equal(t[n - 1], z[f"table_{D}_{n}"]), n
    taps = {n: int(z[f"table_{D}_{n}"][D:2 * D].max()) for n in sides}
    assert taps[D] == 4 and taps[2 * D] in (8, 9) and taps[4 * D] in (16, 17)      # 2 * support taps, one more where the window straddles
    for n in range(8, D + 1, 1 if D == 32 else 27):                   # n <= D: xmin, ntaps and the first four coefficients are the existing table
        xmin, ntaps, coef = data.resize_tables(n, D)
        assert np.array_equal(t[n - 1, :D], xmin.numpy()) and np.array_equal(t[n - 1, D:2 * D], ntaps.numpy())
        full = t[n - 1, 2 * D:].reshape(D, K)
        assert np.array_equal(full[:, :4], coef.numpy()) and not full[:, 4:].any()
    # n = D is the identity: the one coefficient on the output's own pixel is 2^22, which is why the batch launch at S = D changes nothing
    xmin, coef = t[D - 1, :D], t[D - 1, 2 * D:].reshape(D, K)
    assert all(coef[x, x - xmin[x]] == 1 << 22 and np.abs(coef[x]).sum() == 1 << 22 for x in range(D))


def _tap_bound(n, D):
    return 4 if n <= D else min(K, 4 * n // D + 1)


def test_every_admitted_output_size_builds_tables_for_every_admitted_side():
    """D = 8 .. 384 in steps of 4, sides 1 .. 4 D.  Some (n, D) have an output with one tap more than ceil(2 * support), from the rounding of the
    doubles (five at 12 -> 44); its coefficient is 0, and the builder keeps it."""
    extra = {}
    for D in range(8, 385, 4):
        t = data.window_stage_tables(4 * D, D).numpy()
        ntaps, coef = t[:, D:2 * D], t[:, 2 * D:].reshape(4 * D, D, K)
        n = np.arange(1, 4 * D + 1)
        bound = np.where(n <= D, 4, np.minimum(K, 4 * n // D + 1))
        assert ntaps.min() >= 1 and bool((ntaps.max(1) <= np.minimum(K, bound + 1)).all()), D
        assert not (coef * (np.arange(K)[None, None, :] >= bound[:, None, None])).any(), D            # nothing behind the taps the kernel takes
        assert not (coef * (np.arange(K)[None, None, :] >= ntaps[:, :, None])).any(), D               # nothing behind an output's own taps
        over = n[ntaps.max(1) > bound]
        if len(over):
            extra[D] = over.tolist()
    assert 12 in extra[44] and 176 in extra[240] and 96 in extra[352]
    assert all(k not in extra for k in (32, 192, 224, 256, 320, 384))
    for D, sides in ((44, extra[44]), (240, [176])):                  # such a table equals the restatement, and the four-tap entry refuses it
        for n in sides:
            assert np.array_equal(data.window_stage_tables(max(n, 8), D).numpy()[n - 1], wide_ref.flat_table(n, D)), (n, D)
            if 8 <= n <= D:
                with pytest.raises(RuntimeError, match="5 taps"):
                    data.resize_tables(n, D)


def test_the_restatement_with_a_five_tap_row_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(44)
    img = rng.integers(0, 256, (48, 20, 3), dtype=np.uint8)
    assert wide_ref.tables(12, 44)[1].max() == 5
    for rec in (wide_ref.pack(3, 2, 12, 12, False), wide_ref.pack(0, 8, 40, 12, True), wide_ref.pack(36, 0, 12, 20, False)):
        top, left, h, w, flip = wide_ref.unpack(rec)
        win = img[top:top + h, left:left + w]
        win = np.ascontiguousarray(win[:, ::-1] if flip else win)
        assert np.array_equal(wide_ref.resized_window(img, rec, 44), np.asarray(Image.fromarray(win).resize((44, 44), Image.BICUBIC))), rec


def test_tap_counts_at_the_issue_sizes():
    assert [int(wide_ref.tables(n, 224)[1].max()) for n in (256, 512, 896)] == [5, 10, 16]


def test_fixture_equals_the_restatement():
    z = wide_ref.load()
    cases = [(H, W, wide_ref.D_SMALL) for H, W in wide_ref.SMALL] + [wide_ref.BIG[0] + (wide_ref.BIG[1],)]
    for H, W, D in cases:
        image, records, out = z[f"image_{H}_{W}_{D}"], z[f"records_{H}_{W}_{D}"], z[f"out_{H}_{W}_{D}"]
        assert image.shape == (H, W, 3) and image.dtype == np.uint8 and records.dtype == np.int32 and out.shape == (len(records), D, D, 3)
        assert np.array_equal(wide_ref.host_window([image] * len(records), records, D), out), (H, W)
        for r in records.tolist():
            assert wide_ref.clamped(r, H, W) == r
    sides = {wide_ref.unpack(r)[2:4] for r in z["records_64_48_32"].tolist()}
    assert {1, 2, 3, 31, 32, 33, 63, 64} <= {h for h, _ in sides} and {1, 2, 3, 31, 32, 33, 47, 48} <= {w for _, w in sides}


def test_restatement_equals_pillow_where_it_is_installed():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (150, 131, 3), dtype=np.uint8)
    for D in (32, 40):
        for k in range(40):
            h, w = int(rng.integers(1, min(150, 4 * D) + 1)), int(rng.integers(1, min(131, 4 * D) + 1))
            top, left, flip = int(rng.integers(0, 151 - h)), int(rng.integers(0, 132 - w)), bool(k & 1)
            win = img[top:top + h, left:left + w]
            win = np.ascontiguousarray(win[:, ::-1] if flip else win)
            want = np.asarray(Image.fromarray(win).resize((D, D), Image.BICUBIC))
            assert np.array_equal(wide_ref.resized_window(img, wide_ref.pack(top, left, h, w, flip), D), want), (top, left, h, w, flip, D)


def test_record_clamps():
    H, W = 64, 48
    assert wide_ref.clamped([-1, -1], H, W) == wide_ref.pack(0, 0, H, W, True)
    assert wide_ref.clamped([0, 0], H, W) == wide_ref.pack(0, 0, 1, 1, False)
    assert wide_ref.clamped(wide_ref.pack(70, 47, 3, 4, False), H, W) == wide_ref.pack(61, 44, 3, 4, False)
    assert wide_ref.clamped(wide_ref.pack(2, 2, 60, 0x7fff, True), H, W) == wide_ref.pack(2, 0, 60, W, True)


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths
    buf = torch.empty(16, dtype=torch.int32)

    def refused_tables(msg, max_side, D, out=buf.data_ptr()):
        assert L.qatvit_image_window_coeffs(max_side, D, out) != 0
        assert msg in L.qatvit_last_error() and COEFFS.encode() in L.qatvit_last_error(), L.qatvit_last_error()
        if out is not None:
            assert L.qatvit_image_window_coeffs_bytes(max_side, D) == -1 and msg in L.qatvit_last_error()

    refused_tables(b"null pointer", 64, 32, out=None)
    refused_tables(b"outside 8 .. 128", 129, 32)
    refused_tables(b"outside 8 .. 896", 897, 224)
    refused_tables(b"outside 8", 4, 32)
    refused_tables(b"multiple of 4", 64, 30)
    refused_tables(b"8 .. 384", 64, 4)
    refused_tables(b"8 .. 384", 512, 388)
    with pytest.raises(RuntimeError, match="outside 8 .. 896"):
        data.window_stage_tables(1024, 224)

    def refused(msg, data=p, index=None, B=1, N=1, H=64, W=48, D=32, tables=p, max_side=64, rrc=p, out=p):
        assert L.qatvit_image_window_u8(data, index, B, N, H, W, D, tables, max_side, rrc, out, None) != 0
        assert msg in L.qatvit_last_error() and WINDOW.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for name in ("data", "tables", "rrc", "out"):
        refused(b"null pointer", **{name: None})
    refused(b"source height 129 is outside 8 .. 128", H=129, max_side=129)
    refused(b"source width 897 is outside 8 .. 896", W=897, D=224, max_side=897)
    refused(b"source height 4 is outside 8", H=4)
    refused(b"source width 7 is outside 8", W=7)
    refused(b"multiple of 4", D=34)
    refused(b"8 .. 384", D=512, H=512, W=512, max_side=512)
    refused(b"8 .. 384", D=4, H=8, W=8)
    refused(b"tables of 48 sides", max_side=48)
    refused(b"batch 0", B=0)
    refused(b"batch 65536", B=65536, index=p)
    refused(b"not empty", N=0)
    refused(b"needs an index", B=8, N=4)
    for off in (1, 2, 3):
        refused(b"misaligned", tables=p + off)
        refused(b"misaligned", rrc=p + off)
        refused(b"misaligned", out=p + off)
    refused(b"misaligned", index=p + 4, B=1)


def test_draw_for_a_number_is_the_tensor_it_was_before_the_pair_form():
    z = wide_ref.load()
    for name, n, S, seed, scale, ratio in wide_ref.DRAW_CASES:
        got = qat_vit_amd.RandomResizedCrop(scale, ratio).draw(n, S, torch.Generator().manual_seed(seed))
        assert got.dtype == torch.int32 and torch.equal(got, torch.from_numpy(z[f"draw_{name}"])), name
        assert torch.equal(got, qat_vit_amd.RandomResizedCrop(scale, ratio).draw(n, (S, S), torch.Generator().manual_seed(seed))), name
    fallback = _fields(torch.from_numpy(z["draw_wide_ratio"]))       # the pinned cases do reach the fallbacks
    assert bool((fallback[3] == 37).all()) and len(set(_fields(torch.from_numpy(z["draw_tall_ratio"]))[2].tolist())) == 1


@pytest.mark.parametrize("H,W", [(64, 48), (37, 128), (320, 480)])
def test_draw_for_a_pair_follows_the_stated_rule(H, W):
    n, a = 2048, qat_vit_amd.RandomResizedCrop()
    r = a.draw(n, (H, W), torch.Generator().manual_seed(5))
    assert r.dtype == torch.int32 and r.shape == (n, 2) and torch.equal(r, a.draw(n, [H, W], torch.Generator().manual_seed(5)))
    top, left, h, w, flip, rest = _fields(r)
    assert bool(((h >= 1) & (h <= H) & (w >= 1) & (w <= W) & (top <= H - h) & (left <= W - w)).all()) and not rest.any()
    assert [wide_ref.clamped(v, H, W) for v in r[:64].tolist()] == r[:64].tolist()
    assert int(top.max()) > 0 and int(left.max()) > 0 and 0 < int(flip.sum()) < n
    g = torch.Generator().manual_seed(5)
    u, v = torch.rand(n, 10, 2, dtype=torch.float64, generator=g), torch.rand(n, 3, dtype=torch.float64, generator=g)
    in_ratio, whole = W / H, 0
    for k in range(256):
        want = None
        for t in range(10):
            area = float(H * W) * (0.08 + float(u[k, t, 0]) * (1.0 - 0.08))
            aspect = float(torch.exp(math.log(0.75) + u[k, t, 1] * (math.log(4.0 / 3.0) - math.log(0.75))))
            ww, hh = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 1 <= ww <= W and 1 <= hh <= H:
                want = (int(math.floor(float(v[k, 0]) * (H - hh + 1))), int(math.floor(float(v[k, 1]) * (W - ww + 1))), hh, ww)
                break
        if want is None:                                             # torchvision's fallback for a rectangle, centred
            if in_ratio < 0.75:
                ww, hh = W, int(round(W / 0.75))
            elif in_ratio > 4.0 / 3.0:
                hh, ww = H, int(round(H * (4.0 / 3.0)))
            else:
                ww, hh = W, H
            want, whole = ((H - hh) // 2, (W - ww) // 2, hh, ww), whole + 1
        assert (int(top[k]), int(left[k]), int(h[k]), int(w[k]), bool(flip[k])) == want + (bool(v[k, 2] < 0.5),), k


def test_draw_for_a_pair_takes_all_three_fallback_branches():
    R = qat_vit_amd.RandomResizedCrop
    n = 256
    # a scale that no window of the ratio range reaches inside the image: every try fails
    top, left, h, w, _, _ = _fields(R(scale=(0.95, 1.0), ratio=(1.0, 1.0)).draw(n, (40, 100), torch.Generator().manual_seed(1)))
    assert bool(((h == 40) & (w == 40) & (top == 0) & (left == 30)).all())                 # in_ratio 2.5 > r1: h = H, w = round(H * r1)
    top, left, h, w, _, _ = _fields(R(scale=(0.95, 1.0), ratio=(1.0, 1.0)).draw(n, (100, 40), torch.Generator().manual_seed(1)))
    assert bool(((h == 40) & (w == 40) & (top == 30) & (left == 0)).all())                 # in_ratio 0.4 < r0: w = W, h = round(W / r0)
    top, left, h, w, _, _ = _fields(R(scale=(0.99, 1.0), ratio=(0.3, 3.0)).draw(n, (60, 90), torch.Generator().manual_seed(1)))
    whole = (h == 60) & (w == 90)
    assert bool(whole.any()) and bool(((top == 0) & (left == 0))[whole].all())                 # r0 <= in_ratio <= r1: the whole image
    top, left, h, w, _, _ = _fields(R(scale=(0.9, 1.0), ratio=(2.0, 3.0)).draw(n, (50, 60), torch.Generator().manual_seed(2)))
    assert bool(((w == 60) & (h == 30) & (top == 10) & (left == 0)).all())                 # in_ratio 1.2 < r0 = 2
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)              # the generator ends where it ends for a number
    R().draw(100, 32, g1), R(scale=(0.95, 1.0), ratio=(1.0, 1.0)).draw(100, (40, 100), g2)
    assert torch.equal(torch.rand(8, generator=g1), torch.rand(8, generator=g2))
    for bad in ((0, 5), (5, 0x8000), (1, 2, 3), (4,)):
        with pytest.raises(ValueError, match="src_size must be"):
            R().draw(4, bad)


def test_center_crop_window():
    c = qat_vit_amd.center_crop_window
    assert c(256, 256) == (0, 0, 256, 256) and c(320, 480) == (0, 80, 320, 320) and c(480, 320) == (80, 0, 320, 320)
    assert c(256, 256, 0.875) == (16, 16, 224, 224) and c(375, 500, 0.875) == (24, 86, 328, 328)    # round(23.5) = 24 and round(86.0)
    assert c(33, 31) == (1, 0, 31, 31) and c(10, 13) == (0, 2, 10, 10) and c(9, 10) == (0, 0, 9, 9)    # Python's round: 1.5 -> 2, 0.5 -> 0
    assert c(8, 8, 0.01) == (4, 4, 1, 1)
    for bad in ((0, 8, 1.0), (8, 8, 0.0), (8, 8, 1.5)):
        with pytest.raises(ValueError):
            c(*bad)


def _bare_wide(H, W, D):
    tr = object.__new__(qat_vit_amd.GpuWideResizeNormalize)           # the constructor needs the GPU; these refusals do not
    tr.src_size, tr.out_size, tr.device, tr.window = (H, W), D, torch.device("cuda", 0), (0, 0, H, W)
    tr.mean, tr.std = data.IMAGENET_MEAN, data.IMAGENET_STD
    return tr


def test_wide_transform_refusals_without_a_gpu():
    tr = _bare_wide(64, 48, 32)
    imgs = torch.zeros(2, 64, 48, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="aug does not apply to a wide source"):
        tr(imgs, aug=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="cap of 65536 bytes"):
        tr(imgs, blur=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(imgs)
    labels = np.zeros(4, np.int64)
    L = qat_vit_amd.GpuImageLoader
    with pytest.raises(ValueError, match=r"images must be uint8 \[N, 64, 48, 3\]"):
        L(np.zeros((4, 48, 64, 3), np.uint8), labels, 2, transform=tr)
    with pytest.raises(ValueError, match="aug does not apply"):
        L(np.zeros((4, 64, 48, 3), np.uint8), labels, 2, transform=tr, augment=qat_vit_amd.RandomCropFlip(2))
    for kw in ({"blur": qat_vit_amd.GaussianBlur()}, {"three_augment": qat_vit_amd.ThreeAugment()}):
        with pytest.raises(NotImplementedError, match="cap of 65536 bytes"):
            L(np.zeros((4, 64, 48, 3), np.uint8), labels, 2, transform=tr, **kw)
    # with any other transform the loader's shape refusal is what it was
    sq = object.__new__(qat_vit_amd.GpuResizeNormalize)
    sq.src_size, sq.out_size, sq.device = 8, 224, torch.device("cpu")
    with pytest.raises(ValueError, match=r"images must be uint8 \[N, S, S, 3\]"):
        L(np.zeros((4, 64, 48, 3), np.uint8), labels, 2, transform=sq)
    for src, window in (((64, 48), (0, 0, 65, 48)), ((64, 48), (60, 0, 8, 8)), ((64, 48), (0, 0, 0, 4)), (64, None), ((64, 48), (0, 0, 8.0, 8))):
        with pytest.raises(ValueError, match="window|src_size must be a pair"):      # refused before the device is touched
            qat_vit_amd.GpuWindowResize(src, 32, window=window)
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.GpuWindowResize((64, 48), 32, device="cpu")


def test_teacher_table_record_of_a_wide_transform():
    tr = _bare_wide(64, 48, 32)
    rec = distill.transform_tuple(tr)
    assert rec == ((64, 48), 32, data.IMAGENET_MEAN, data.IMAGENET_STD, (0, 0, 64, 48)) and distill.transform_tuple(rec) == rec
    tr.window = (8, 0, 48, 48)
    assert distill.transform_tuple(tr)[4] == (8, 0, 48, 48) and distill.transform_tuple(tr) != rec
    sq = object.__new__(qat_vit_amd.GpuResizeNormalize)               # the record of a GpuResizeNormalize is what it was
    sq.src_size, sq.out_size, sq.mean, sq.std = 32, 224, data.IMAGENET_MEAN, data.IMAGENET_STD
    assert distill.transform_tuple(sq) == (32, 224, data.IMAGENET_MEAN, data.IMAGENET_STD)
