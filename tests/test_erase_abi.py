"""CPU-side checks of RandomErasing inside the batch launch (qatvit_image_batch_erase, qatvit_image_batch_rrc_erase, qat_vit_amd.RandomErasing): the
symbols in the header, the binding and the library; every argument error as a string without a HIP call, with and without records; the refusals
of the Python classes; the drawing rule restated per sample; Philox4x32-10 of tests/erase_ref.py against the published known-answer vectors."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from tests import erase_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERASE, RRC_ERASE = "qatvit_image_batch_erase", "qatvit_image_batch_rrc_erase"


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert decl, f"{name} is not declared in include/qatvit.h"
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_symbols_in_header_signatures_and_exports(native_lib):
    er, rrc = _params(ERASE), _params(RRC_ERASE)
    assert len(er) == 15 and er[6:14] == ["const int32_t* coeffs", "const float* table", "const int32_t* aug", "int32_t padding_mode", "int32_t fill",
                                          "const int32_t* mix", "const int32_t* erase", "float* out"]
    assert len(rrc) == 13 and rrc[6:12] == ["const int32_t* windows", "const float* table", "const int32_t* rrc", "const int32_t* mix",
                                            "const int32_t* erase", "float* out"]
    assert er[:6] == rrc[:6] == ["const uint8_t* data", "const int64_t* index", "int32_t B", "int32_t N", "int32_t S", "int32_t D"]
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name, params in ((ERASE, er), (RRC_ERASE, rrc)):
        res, args = native.SIGNATURES[name]
        assert res is native.c_int and len(args) == len(params)
        for p, a in zip(params, args):
            assert a is (native.c_void_p if "*" in p else native.c_int32), (name, p)
        assert name in exported
    assert native_lib.qatvit_abi_version() == 4                      # added symbols: the version stays
    assert "RandomErasing" in qat_vit_amd.__all__ and qat_vit_amd.data.ERASE_WORDS == 8


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert tuple(int(v) for v in erase_ref.philox4x32_10(counter, key)) == want
    # vectorised: the three counters in one call per key give the single calls' words; a key given as int32 words is the same key
    c = np.array([k[0] for k in kat], dtype=np.uint32).T
    got = erase_ref.philox4x32_10(tuple(c), kat[2][1])
    assert tuple(int(v[2]) for v in got) == kat[2][2] and got[0].dtype == np.uint32
    assert tuple(int(v) for v in erase_ref.philox4x32_10(kat[1][0], (-1, -1))) == kat[1][2]


def test_noise_field_is_standard_normal_and_a_function_of_the_key():
    z = erase_ref.noise((1, 2), 36)
    assert z.shape == (3, 36, 36) and z.dtype == np.float64 and np.isfinite(z).all() and np.abs(z).max() <= math.sqrt(46 * math.log(2))
    n = z.size
    assert abs(z.mean()) < 5 / math.sqrt(n) and abs(z.std() - 1) < 5 / math.sqrt(2 * n)
    assert np.array_equal(z, erase_ref.noise((1, 2), 36)) and not np.array_equal(z, erase_ref.noise((2, 1), 36))
    # element (c, y, x) comes from counter (y * (D / 4) + x / 4, c, 0, 0): the pair (r0, r1) gives x & 3 = 0, 1
    r = [int(v) for v in erase_ref.philox4x32_10((5 * 9 + 3, 2, 0, 0), (1, 2))]
    u, t = ((r[0] >> 9) + 1) * 2.0 ** -23, (r[1] >> 8) * 2.0 ** -23
    assert z[2, 5, 12] == math.sqrt(-2 * math.log(u)) * np.cos(np.pi * t) and z[2, 5, 13] == math.sqrt(-2 * math.log(u)) * np.sin(np.pi * t)


def test_record_fields_clamps_and_the_erased_batch():
    r = erase_ref.pack(3, 7, 250, 9, (1.5, -2.0, -0.0), 0)
    assert r[:2] == [3 | 7 << 16, 250 | 9 << 16] and r[4] == -(1 << 31) and r[5:] == [0, 0, 0]
    assert erase_ref.unpack([-1] * 8)[:4] == (0xffff,) * 4 and erase_ref.unpack([-1] * 8)[5:] == (1, (0xffffffff, 0xffffffff))
    assert erase_ref.clamped([-1] * 8, 224)[:2] == erase_ref.pack(224, 224, 224, 224)[:2] and erase_ref.clamped([-1] * 8, 224)[5] == 1
    assert erase_ref.clamped(erase_ref.pack(0, 40000, 10, 230, mode=6), 224) == erase_ref.pack(0, 224, 10, 224, mode=0)
    X = np.arange(2 * 3 * 8 * 8, dtype=np.float32).reshape(2, 3, 8, 8)
    E = erase_ref.erased(X, [erase_ref.pack(1, 3, 2, 9, (1.5, -2.0, -0.0)), [0] * 8])
    assert np.array_equal(E[1], X[1]) and np.array_equal(E[0, :, 1:3, 2:], np.broadcast_to(np.float32([1.5, -2.0, -0.0])[:, None, None], (3, 2, 6)))
    mask = erase_ref.box_mask([erase_ref.pack(1, 3, 2, 9), [0] * 8], 8)
    assert mask.sum() == 3 * 2 * 6 and np.array_equal(E[~mask], X[~mask])
    N = erase_ref.erased(X, [erase_ref.pack(0, 8, 0, 8, mode=1, key=(7, 9))] * 2)
    assert np.array_equal(N[0], erase_ref.noise((7, 9), 8).astype(np.float32)) and np.array_equal(N[0], N[1])


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def refused(msg, who=None, data=p, index=None, B=1, N=1, S=32, D=224, coeffs=p, table=p, aug=p, mode=0, fill=0, mix=p, erase=p, out=p):
        assert L.qatvit_image_batch_erase(data, index, B, N, S, D, coeffs, table, aug, mode, fill, mix, erase, out, None) != 0
        assert msg in L.qatvit_last_error() and (who or ERASE).encode() in L.qatvit_last_error(), L.qatvit_last_error()

    def refused_rrc(msg, who=None, data=p, index=None, B=1, N=1, S=32, D=224, windows=p, table=p, rrc=p, mix=p, erase=p, out=p):
        assert L.qatvit_image_batch_rrc_erase(data, index, B, N, S, D, windows, table, rrc, mix, erase, out, None) != 0
        assert msg in L.qatvit_last_error() and (who or RRC_ERASE).encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for erase in (p, None):                                          # with and without erase records
        for mix in (p, None):
            kw = dict(mix=mix, erase=erase)
            for fn, tab in ((refused, "coeffs"), (refused_rrc, "windows")):
                for name in ("data", tab, "table", "out"):
                    fn(b"null pointer", **{name: None}, **kw)
                fn(b"downscaling is not supported", S=256, **kw)
                fn(b"outside 8", S=4, **kw)
                fn(b"multiple of 4", D=222, **kw)
                fn(b"at most 384", S=384, D=512, **kw)
                fn(b"batch 0", B=0, **kw)
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
            refused(b"misaligned", mix=p + off, erase=erase)
            refused_rrc(b"misaligned", mix=p + off, erase=erase)
    for off in (1, 2, 3):                                            # a misaligned erase, with and without mix records
        for mix in (p, None):
            refused(b"misaligned", erase=p + off, mix=mix)
            refused_rrc(b"misaligned", erase=p + off, mix=mix)
    # two plane sets of a large source do not fit 64 KB of LDS: an error string, not a launch; without erase records the sibling's own
    refused(b"bytes of LDS", S=384, D=384)
    refused(b"bytes of LDS", S=300, D=384, aug=None)
    refused(b"bytes of LDS", who="qatvit_image_batch_mix", S=384, D=384, erase=None)
    refused_rrc(b"bytes of LDS", S=384, D=384)
    refused_rrc(b"bytes of LDS", S=300, D=384)
    refused_rrc(b"bytes of LDS", who="qatvit_image_batch_rrc", S=384, D=384, erase=None)


def test_python_wrapper_refusals_without_a_gpu():
    tr = object.__new__(qat_vit_amd.GpuResizeNormalize)               # the constructor needs the GPU; these refusals do not
    tr.src_size, tr.out_size, tr.device = 32, 224, torch.device("cuda", 0)
    imgs, recs = torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.int32)
    for kw in ({}, {"aug": torch.zeros(2, dtype=torch.int32)}, {"rrc": torch.zeros(2, 2, dtype=torch.int32)}, {"mix": torch.zeros(2, 6, dtype=torch.int32)}):
        with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
            tr(imgs, erase=recs, **kw)
    with pytest.raises(ValueError, match="rrc and aug are mutually exclusive"):
        tr(imgs, erase=recs, rrc=torch.zeros(2, 2, dtype=torch.int32), aug=torch.zeros(2, dtype=torch.int32))


def test_random_erasing_refusals():
    R = qat_vit_amd.RandomErasing
    for p in (-0.1, 1.5, "half", float("nan"), True, None):
        with pytest.raises(ValueError, match="p must be"):
            R(p=p)
    for scale in ((0, 1), (-0.1, 0.5), (0.5, 0.2), (0.1,), 0.5, (0.1, float("inf")), (float("nan"), 1), ("a", 1), (True, 1)):
        with pytest.raises(ValueError, match="scale must be"):
            R(scale=scale)
    for ratio in ((0, 1), (2, 1), (1, float("inf")), None, (1, "b")):
        with pytest.raises(ValueError, match="ratio must be"):
            R(ratio=ratio)
    for value in ("noise", (1, 2), (1, 2, 3, 4), float("nan"), (0, float("inf"), 0), None, True, (1, "a", 2)):
        with pytest.raises(ValueError, match="value must be"):
            R(value=value)
    for mode in ("noise", 1, "Pixel"):
        with pytest.raises(ValueError, match="mode must be"):
            R(mode=mode)
    for kw in ({"value": "random", "mode": "const"}, {"value": "random", "mode": "rand"}):
        with pytest.raises(ValueError, match="value='random' is mode='pixel'"):
            R(**kw)
    for kw in ({"value": 0.5, "mode": "rand"}, {"value": (0, 0, 1), "mode": "pixel"}):
        with pytest.raises(ValueError, match="draws its own fill"):
            R(**kw)
    a = R()
    assert (a.p, a.scale, a.ratio, a.value, a.mode) == (0.25, (0.02, 0.33), (0.3, 3.3), (0.0, 0.0, 0.0), "const")
    assert R(value="random").mode == "pixel" and R(value="random", mode="pixel").mode == "pixel" and R(mode="rand").mode == "rand"
    assert R(value=(1, -2.5, 0)).value == (1.0, -2.5, 0.0) and R(value=-1).value == (-1.0,) * 3 and R(p=1).p == 1.0
    for d in (0, -3, 0x10000):
        with pytest.raises(ValueError, match="out_size must be"):
            a.draw(4, d)


def _boxes(rec):
    r = rec.to(torch.int64) & 0xffffffff
    return r[:, 0] & 0xffff, r[:, 0] >> 16, r[:, 1] & 0xffff, r[:, 1] >> 16


@pytest.mark.parametrize("D", [36, 224])
@pytest.mark.parametrize("mode", ["const", "rand", "pixel"])
def test_draw_gives_records_by_the_stated_rule(D, mode):
    R = qat_vit_amd.RandomErasing
    n, fill = 2048, (0.5, -1.25, -0.0)
    a = R(p=1, value=fill if mode == "const" else 0, mode=mode)
    r1, r2 = a.draw(n, D, torch.Generator().manual_seed(5)), a.draw(n, D, torch.Generator().manual_seed(5))
    assert r1.dtype == torch.int32 and r1.shape == (n, 8) and not r1.is_cuda and r1.is_contiguous() and torch.equal(r1, r2)
    assert not torch.equal(r1, a.draw(n, D, torch.Generator().manual_seed(6)))
    y0, y1, x0, x1 = _boxes(r1)
    assert bool(((y1 <= D) & (x1 <= D) & (y1 - y0 < D) & (x1 - x0 < D)).all()) and len(set((y1 - y0).tolist())) > 10
    assert [erase_ref.clamped(r, D) for r in r1[:64].tolist()] == r1[:64].tolist()
    # the rule itself, restated sample by sample with Python floats
    g = torch.Generator().manual_seed(5)
    gg = torch.rand(n, dtype=torch.float64, generator=g)
    u, v = torch.rand(n, 10, 2, dtype=torch.float64, generator=g), torch.rand(n, 2, dtype=torch.float64, generator=g)
    z = torch.randn(n, 3, dtype=torch.float32, generator=g)
    k = torch.randint(-(1 << 31), 1 << 31, (n, 2), dtype=torch.int64, generator=g)
    assert bool((gg < 1).all())
    erased = 0
    for s in range(256):
        want = [0] * 8
        for t in range(10):
            area = float(D * D) * (0.02 + float(u[s, t, 0]) * (0.33 - 0.02))
            aspect = float(torch.exp(math.log(0.3) + u[s, t, 1] * (math.log(3.3) - math.log(0.3))))
            h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if h < D and w < D:
                top, left = int(math.floor(float(v[s, 0]) * (D - h + 1))), int(math.floor(float(v[s, 1]) * (D - w + 1)))
                if mode == "pixel":
                    want = erase_ref.pack(top, top + h, left, left + w, mode=1, key=(int(k[s, 0]), int(k[s, 1])))
                else:
                    want = erase_ref.pack(top, top + h, left, left + w, fill if mode == "const" else z[s].tolist())
                erased += 1
                break
        assert r1[s].tolist() == want, s
    assert erased > 250
    if mode == "rand":                                               # one normal per channel and sample, not one per record
        f = r1[:, 2:5].contiguous().view(torch.float32)
        assert len(set(f.flatten().tolist())) > 3 * n - 8 and abs(float(f.mean())) < 5 / math.sqrt(3 * n)


def test_draw_settings():
    R = qat_vit_amd.RandomErasing
    n, D = 4096, 224
    for kw in ({}, {"mode": "rand"}, {"value": "random"}):
        assert not R(p=0, **kw).draw(n, D, torch.Generator().manual_seed(1)).any()             # p = 0: every record is the identity
        # a scale and ratio that only the whole image meets: h = w = D does not fit (h < D is asked), so no try fits: the identity
        assert not R(p=1, scale=(1, 1), ratio=(1, 1), **kw).draw(n, D, torch.Generator().manual_seed(1)).any()
    quarter = R().draw(n, D, torch.Generator().manual_seed(2))
    hit = quarter.any(1)
    assert abs(int(hit.sum()) - n // 4) < 5 * math.sqrt(n * 0.25 * 0.75)
    g = torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    assert torch.equal(hit, g < 0.25)                                # the default scale and ratio always fit within ten tries here
    y0, y1, x0, x1 = _boxes(quarter[hit])
    area = ((y1 - y0) * (x1 - x0)).double() / (D * D)
    assert 0.015 < float(area.min()) and float(area.max()) < 0.34 and 0.15 < float(area.mean()) < 0.20
    assert not quarter[:, 2:].any()                                  # const with value 0: nothing but the box
    pix = R(value="random").draw(n, D, torch.Generator().manual_seed(2))
    assert torch.equal(pix[:, :2], quarter[:, :2]) and bool((pix[hit][:, 5] == 1).all()) and not pix[:, 2:5].any()
    assert len({tuple(r) for r in pix[hit][:, 6:].tolist()}) == int(hit.sum())
    # the generator advances identically whatever the settings: its position depends on n only
    after = []
    for kw in ({}, {"p": 0}, {"p": 1, "mode": "rand"}, {"value": "random", "scale": (1, 1), "ratio": (1, 1)}, {"value": (1, 2, 3), "ratio": (2.0, 3.0)}):
        g = torch.Generator().manual_seed(9)
        R(**kw).draw(100, D, g)
        after.append(torch.rand(8, generator=g))
    assert all(torch.equal(after[0], t) for t in after[1:])
    g = torch.Generator().manual_seed(9)
    R().draw(101, D, g)
    assert not torch.equal(after[0], torch.rand(8, generator=g))
    assert R().draw(0, D).shape == (0, 8)
    torch.manual_seed(3)                                             # no generator: torch's default one
    d1 = R(p=1).draw(50, D)
    torch.manual_seed(3)
    assert torch.equal(d1, R(p=1).draw(50, D))


def test_loader_refusals_without_a_gpu():
    tr = object.__new__(qat_vit_amd.GpuResizeNormalize)
    tr.src_size, tr.out_size, tr.device = 8, 224, torch.device("cpu")
    imgs, labels = np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64)
    for bad in ("pixel", 0.25, qat_vit_amd.RandomCropFlip(2), qat_vit_amd.MixupCutmix()):
        with pytest.raises(TypeError, match="erase must be a RandomErasing"):
            qat_vit_amd.GpuImageLoader(imgs, labels, 2, transform=tr, erase=bad)
    with pytest.raises(ValueError, match="crop and augment are mutually exclusive"):
        qat_vit_amd.GpuImageLoader(imgs, labels, 2, transform=tr, crop=qat_vit_amd.RandomResizedCrop(), augment=qat_vit_amd.RandomCropFlip(2),
                                   erase=qat_vit_amd.RandomErasing())
    ok = qat_vit_amd.GpuImageLoader(imgs, labels, 2, transform=tr, erase=qat_vit_amd.RandomErasing(), mix=qat_vit_amd.MixupCutmix(),
                                    augment=qat_vit_amd.RandomCropFlip(2))
    assert isinstance(ok.erase, qat_vit_amd.RandomErasing) and len(ok) == 2
