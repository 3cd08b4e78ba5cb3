"""CPU-side checks of the bytes-in blur form (qatvit_image_bytes_blur, qat_vit_amd.GpuBytesBlurNormalize, GpuWideResizeNormalize(blur=True)):
the symbol in the header, the binding and the library; every refusal of the entry, under its name and before any HIP call; the LDS figures of
the layout include/qatvit.h states, restated here; the switch of the wide transform and what stays without it; the loader with a wide transform
whose switch is on.  Nothing here needs a GPU: every library call ends in an error string before any HIP call."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data, native
from tests.test_wide_abi import _bare_wide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096                                                             # non-null, 4096-aligned; never dereferenced on these paths
NAME = "qatvit_image_bytes_blur"
CAP = 65536


def _call(L, **kw):
    a = dict(bytes=P, B=1, D=224, table=P, mix=None, erase=None, color=None, sums=None, blur=P, out=P)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(L, NAME)(a["bytes"], a["B"], a["D"], a["table"], a["mix"], a["erase"], a["color"], a["sums"], a["blur"], a["out"], None)
    return rc, L.qatvit_last_error().decode()


def _refused(L, text, **kw):
    rc, err = _call(L, **kw)
    assert rc != 0 and err.startswith(NAME + ": ") and text in err, (kw, err)
    return err


def _lds(D, mixed):
    """(bytes, band) of the layout: the value table, then (sides + 1) image buffers of band + 12 rows of 3 * D bytes; the band is 16 rows
    without mix records where that stays within the cap, else 8; 8 with them."""
    sides = 2 if mixed else 1
    request = lambda band: 3072 + (sides + 1) * (band + 12) * 3 * D   # noqa: E731
    band = 16 if not mixed and request(16) <= CAP else 8
    return request(band), band


def test_symbol_in_header_signature_and_export(native_lib):
    hdr = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert decl, f"{NAME} is not declared in include/qatvit.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const uint8_t* bytes", "int32_t B", "int32_t D", "const float* table", "const int32_t* mix", "const int32_t* erase",
                      "const int32_t* color", "uint32_t* sums", "const int32_t* blur", "float* out", "void* stream"]
    res, args = native.SIGNATURES[NAME]
    assert res is native.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        assert a is (native.c_void_p if "*" in p else native.c_int32), p
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4                      # an added symbol: the version stays
    assert "GpuBytesBlurNormalize" in qat_vit_amd.__all__
    for text in ("qatvit_image_bytes_blur:", "40,704 bytes, 43,392 with mix records", "(band + 12) * 3 * D bytes", "BITWISE"):
        assert text in hdr, text
    assert "image_bytes_blur.hip" in open(os.path.join(ROOT, "qat-vit_amd", "csrc", "Makefile")).read()


def test_every_refusal_is_a_string_under_the_entrys_name(native_lib):
    L = native_lib
    for arg in ("bytes", "table", "blur", "out"):
        _refused(L, "null pointer argument", **{arg: None})
    _refused(L, "output size 222 must be a multiple of 4", D=222)
    _refused(L, "output size 4 must be a multiple of 4 in 8 .. 384", D=4)
    _refused(L, "output size 388 must be a multiple of 4 in 8 .. 384", D=388)
    _refused(L, "output size 0 ", D=0)
    _refused(L, "output size -224 ", D=-224)
    _refused(L, "batch 0 must be 1 .. 65535", B=0)
    _refused(L, "batch -3 must be 1 .. 65535", B=-3)
    _refused(L, "batch 65536 must be 1 .. 65535", B=65536)
    for off in (4, 8, 12):
        _refused(L, "misaligned pointer", out=P + off)
    for arg in ("bytes", "table", "mix", "erase", "color", "sums", "blur"):
        for off in (1, 2, 3):
            _refused(L, "misaligned pointer", **{arg: P + off})
    # the LDS limit, before any HIP call, with the byte count: mix records above D = 344
    assert _lds(384, True) == (72192, 8) and _lds(348, True) == (65712, 8)
    for D in (348, 384):
        err = _refused(L, f"output {D} needs {_lds(D, True)[0]} bytes of LDS", D=D, mix=P)
        assert "3 image buffers of 20 rows" in err and err.endswith(f"more than {CAP}")
        _refused(L, "bytes of LDS", D=D, mix=P, erase=P, color=P, sums=P)


def test_the_lds_figures_of_the_layout():
    assert _lds(224, False) == (40704, 16) and _lds(224, True) == (43392, 8)
    assert _lds(368, False) == (64896, 16) and _lds(372, False) == (47712, 8) and _lds(384, False) == (49152, 8)
    assert _lds(344, True) == (64992, 8)
    for D in range(8, 385, 4):
        plain, mixed = _lds(D, False)[0], _lds(D, True)[0]
        assert plain <= CAP, D                                       # the forms without mix records: every admitted D
        assert (mixed <= CAP) == (D <= 344), D
        if D <= 224:
            assert mixed <= CAP and _lds(D, False)[1] == 16, D       # every form for every D <= 224


def test_the_library_admits_and_refuses_as_the_layout_says(native_lib):
    """The launcher's refusal is the only thing between an admitted request and a HIP call, so only refused shapes are called here: every D
    with mix records above 344, with the layout's byte count in the text; the admitted ones are launched on the GPU (tests/test_gpu_bytes_blur.py)."""
    for D in range(348, 385, 4):
        _refused(native_lib, f"needs {_lds(D, True)[0]} bytes of LDS", D=D, mix=P)
    src = open(os.path.join(ROOT, "qat-vit_amd", "csrc", "image_bytes_blur.hip")).read()
    assert "kImgBytesTable + (int64_t)(sides + 1) * (band + 2 * kImgBlurHalo) * 3 * D" in src        # the formula restated above
    kernels = open(os.path.join(ROOT, "qat-vit_amd", "csrc", "qv_kernels.h")).read()
    assert "kImgBlurHalo = 3 * (kImgBlurMaxRadius + 1), kImgBlurBand = 16, kImgBlurMixBand = 8" in kernels and "kImgMixMaxLds = 64 * 1024" in kernels


def test_without_the_switch_everything_stays():
    tr = _bare_wide(64, 48, 32)                                      # never ran the constructor: the switch reads as off
    imgs = torch.zeros(2, 64, 48, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError) as e:
        tr(imgs, blur=torch.zeros(2, 4, dtype=torch.int32))
    assert str(e.value) == ("blur is not served on a wide source: the blur forms stage source rows plus planes in LDS, and at S = D = 224 they ask for "
                            "89,536 bytes, above the cap of 65536 bytes")
    labels = np.zeros(4, np.int64)
    for kw in ({"blur": qat_vit_amd.GaussianBlur()}, {"three_augment": qat_vit_amd.ThreeAugment()}):
        with pytest.raises(NotImplementedError, match="cap of 65536 bytes"):
            qat_vit_amd.GpuImageLoader(np.zeros((4, 64, 48, 3), np.uint8), labels, 2, transform=tr, **kw)
    tr.blur = False
    with pytest.raises(NotImplementedError, match="cap of 65536 bytes"):
        tr.refuse(None, object())
    tr.blur = True                                                   # on: blur passes, aug stays refused
    tr.refuse(None, object())
    with pytest.raises(ValueError, match="aug does not apply to a wide source"):
        tr.refuse(object(), object())
    with pytest.raises(ValueError, match="aug does not apply to a wide source"):
        tr(imgs, aug=torch.zeros(2, dtype=torch.int32), blur=torch.zeros(2, 4, dtype=torch.int32))


def test_the_constructors_and_calls_take_the_keywords():
    sig = inspect.signature(qat_vit_amd.GpuWideResizeNormalize.__init__)
    assert list(sig.parameters) == ["self", "src_size", "out_size", "mean", "std", "device", "window", "blur"] and sig.parameters["blur"].default is False
    sig = inspect.signature(qat_vit_amd.GpuBytesBlurNormalize.__init__)
    assert list(sig.parameters) == ["self", "out_size", "mean", "std", "device"] and sig.parameters["out_size"].default == 224
    sig = inspect.signature(qat_vit_amd.GpuBytesBlurNormalize.__call__)
    assert list(sig.parameters) == ["self", "bytes_u8", "out", "mix", "erase", "color", "contrast", "blur"] and sig.parameters["contrast"].default is True
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.GpuBytesBlurNormalize(32, device="cpu")
    tr = object.__new__(qat_vit_amd.GpuBytesBlurNormalize)           # the constructor needs the GPU; these refusals do not
    tr.out_size, tr.device = 32, torch.device("cuda", 0)
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), blur=torch.zeros(2, 4, dtype=torch.int32))


class _WideRecorder(qat_vit_amd.GpuWideResizeNormalize):
    """A stand-in wide transform with the switch on: keeps what the loader hands to every call."""

    def __init__(self, H, W, D):
        self.src_size, self.out_size, self.device, self.window, self.blur = (H, W), D, torch.device("cpu"), (0, 0, H, W), True
        self.calls = []

    def __call__(self, images, index, **kw):
        self.calls.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in dict(kw, index=index).items()})
        return torch.zeros(index.shape[0], 3, 1, 1)


@pytest.mark.parametrize("option", ["three_augment", "blur"])
def test_the_loader_takes_blur_options_with_a_wide_transform_whose_switch_is_on(monkeypatch, option):
    empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **k: empty(*a, **k))       # no accelerator here: the block is not pinned
    H, W, D, n, bs, seed = 64, 48, 32, 20, 8, 12
    rng = np.random.default_rng(3)
    imgs, labels = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), rng.integers(0, 10, n)
    tr = _WideRecorder(H, W, D)
    c, m, e = qat_vit_amd.RandomResizedCrop(), qat_vit_amd.MixupCutmix(mode="elem"), qat_vit_amd.RandomErasing(p=0.6)
    aug = qat_vit_amd.ThreeAugment() if option == "three_augment" else qat_vit_amd.GaussianBlur(p=0.5)
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, generator=torch.Generator().manual_seed(seed), transform=tr, crop=c, mix=m,
                                        erase=e, **{option: aug})
    tuples = list(loader)
    g = torch.Generator().manual_seed(seed)                          # the documented order: plan, windows of (H, W), mix, erase, colour and blur
    plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
    want = {"rrc": c.draw(n, (H, W), g), "mix": m.draw([len(b) for b in plan], D, g), "erase": e.draw(n, D, g)}
    if option == "three_augment":
        want["color"], want["blur"] = aug.draw(n, g)
    else:
        want["blur"] = aug.draw(n, g)
    assert len(tr.calls) == len(tuples) == len(plan) == 3
    for key, records in want.items():
        assert torch.equal(torch.cat([call[key] for call in tr.calls]), records), key
    assert 0 < int((want["blur"][:, 0] & 1).sum()) < n                # the blur section arrives as blur=, some samples on and some off
    for call, b in zip(tr.calls, plan):
        assert torch.equal(call["index"], b) and call["blur"].shape == (len(b), 4) and call["blur"].dtype == torch.int32
        assert call["contrast"] is (option == "three_augment") and "aug" not in call
        if option == "blur":
            assert call["color"] is None
    with pytest.raises(ValueError, match="aug does not apply"):
        qat_vit_amd.GpuImageLoader(imgs, labels, bs, transform=tr, augment=qat_vit_amd.RandomCropFlip(2), **{option: aug})
