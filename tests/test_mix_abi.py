"""CPU-side checks of mixup / cutmix (qatvit_image_batch_mix, qatvit_kd_ce_loss_mix, qat_vit_amd.MixupCutmix): the symbols in the header, the
binding and the library; every argument error as a string without a HIP call; the wrappers' refusal of CPU tensors; the drawing rule."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native
from tests import mix_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE, LOSS = "qatvit_image_batch_mix", "qatvit_kd_ce_loss_mix"
CTYPE = {"int32_t": native.c_int32, "int64_t": native.c_int64, "float": native.c_float}


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert decl, f"{name} is not declared in include/qatvit.h"
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_symbols_in_header_signatures_and_exports(native_lib):
    img, loss = _params(IMAGE), _params(LOSS)
    assert len(img) == 14 and img[8:12] == ["const int32_t* aug", "int32_t padding_mode", "int32_t fill", "const int32_t* mix"]
    assert len(loss) == 15 and loss[1:7] == ["const float* teacher", "const float* table", "int64_t table_rows", "const int64_t* index",
                                             "const int64_t* labels", "const int32_t* mix"]
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name, params in ((IMAGE, img), (LOSS, loss)):
        res, args = native.SIGNATURES[name]
        assert res is native.c_int and len(args) == len(params)
        for p, a in zip(params, args):
            assert a is (native.c_void_p if "*" in p else CTYPE[p.split()[0]]), (name, p)
        assert name in exported
    assert native_lib.qatvit_abi_version() == 4                      # added symbols: the version stays
    assert "MixupCutmix" in qat_vit_amd.__all__


def test_image_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def refused(msg, data=p, index=None, B=1, N=1, S=32, D=224, coeffs=p, table=p, aug=p, mode=0, fill=0, mix=p, out=p):
        assert L.qatvit_image_batch_mix(data, index, B, N, S, D, coeffs, table, aug, mode, fill, mix, out, None) != 0
        assert msg in L.qatvit_last_error() and IMAGE.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for mix in (p, None):                                            # the aug entry's checks, with and without records
        for name in ("data", "coeffs", "table", "out"):
            refused(b"null pointer", mix=mix, **{name: None})
        refused(b"downscaling is not supported", S=256, mix=mix)
        refused(b"outside 8", S=4, mix=mix)
        refused(b"multiple of 4", D=222, mix=mix)
        refused(b"at most 384", S=384, D=512, mix=mix)
        refused(b"batch 0", B=0, mix=mix)
        refused(b"batch 65536", B=65536, index=p, mix=mix)
        refused(b"not empty", N=0, mix=mix)
        refused(b"needs an index", B=8, N=4, mix=mix)
        refused(b"misaligned", out=p + 4, mix=mix)
        refused(b"misaligned", coeffs=p + 2, mix=mix)
        refused(b"misaligned", table=p + 1, mix=mix)
        refused(b"misaligned", aug=p + 2, mix=mix)
        refused(b"unknown padding_mode 2", mode=2, mix=mix)
        refused(b"fill 256 is outside 0 .. 255", fill=256, mix=mix)
        refused(b"fill 300", aug=None, fill=300, mix=mix)
    # its own
    for off in (1, 2, 3):
        refused(b"misaligned", mix=p + off)
        refused(b"misaligned", mix=p + off, aug=None)
    # two plane sets of a large source do not fit 64 KB of LDS: an error string, not a launch
    refused(b"bytes of LDS", S=384, D=384)
    refused(b"bytes of LDS", S=300, D=384, aug=None)


def test_loss_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096

    def refused(msg, student=p, teacher=None, table=None, rows=0, index=None, labels=p, mix=p, B=8, C=10, T=4.0, out3=p, dlogits=p):
        assert L.qatvit_kd_ce_loss_mix(student, teacher, table, rows, index, labels, mix, B, C, T, 0.5, 0.1, out3, dlogits, None) != 0
        assert msg in L.qatvit_last_error() and LOSS.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for mix in (p, None):
        for name in ("student", "labels", "out3", "dlogits"):
            refused(b"null pointer", mix=mix, **{name: None})
        refused(b"mutually exclusive", teacher=p, table=p, rows=4, index=p, mix=mix)
        refused(b"needs an index", table=p, rows=4, mix=mix)
        refused(b"table_rows 0", table=p, rows=0, index=p, mix=mix)
        refused(b"bad shape", B=0, mix=mix)
        refused(b"bad shape", C=1, mix=mix)
        refused(b"bad shape", C=4097, mix=mix)
        refused(b"kd_temp", T=0.0, mix=mix)
    for off in (1, 2, 3):
        refused(b"misaligned mix", mix=p + off)
        refused(b"misaligned mix", mix=p + off, teacher=p)
        refused(b"misaligned mix", mix=p + off, table=p, rows=4, index=p)


def test_python_wrappers_refuse_cpu_tensors():
    tr = object.__new__(qat_vit_amd.GpuResizeNormalize)               # the constructor needs the GPU; the refusal does not
    tr.src_size, tr.out_size, tr.device = 32, 224, torch.device("cuda", 0)
    imgs, recs = torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 6, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(imgs, mix=recs)
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(imgs, aug=torch.zeros(2, dtype=torch.int32), mix=recs)
    s, t, y = torch.zeros(2, 10), torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="kd_ce_loss_mix: qat-vit_amd ops run on MI355X only"):
        F.kd_ce_loss_mix(s, t, y, recs)
    with pytest.raises(RuntimeError, match="kd_ce_loss_mix: qat-vit_amd ops run on MI355X only"):
        F.kd_ce_loss_mix(s, None, y, recs)
    with pytest.raises(RuntimeError, match="kd_ce_loss_table_mix: qat-vit_amd ops run on MI355X only"):
        F.kd_ce_loss_table_mix(s, torch.zeros(5, 10), y, y, recs)
    table = object.__new__(qat_vit_amd.TeacherLogitTable)           # a table on the host: refused before anything else is looked at
    table.logits = torch.zeros(5, 10)
    with pytest.raises(RuntimeError, match="MI355X only"):
        table.loss(s, y, y, mix=recs)


def test_mixup_cutmix_refusals():
    M = qat_vit_amd.MixupCutmix
    for kw in ({"mixup_alpha": -0.1}, {"cutmix_alpha": -1}, {"mixup_alpha": float("nan")}, {"cutmix_alpha": float("inf")}, {"mixup_alpha": "a"},
               {"cutmix_alpha": True}):
        with pytest.raises(ValueError, match="alpha must be"):
            M(**kw)
    for kw in ({"prob": -0.1}, {"prob": 1.5}, {"switch_prob": 2}, {"switch_prob": -1e-9}, {"prob": float("nan")}, {"prob": None}):
        with pytest.raises(ValueError, match="prob must be"):
            M(**kw)
    for mode in ("pair", "half", None, 0):
        with pytest.raises(ValueError, match="mode must be"):
            M(mode=mode)
    m = M()
    assert (m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob, m.mode) == (0.8, 1.0, 1.0, 0.5, "batch")
    assert M(0, 0, 0, 0, "elem").mode == "elem"
    with pytest.raises(ValueError, match="out_size"):
        m.draw([4], 0)


def _columns(rec, D):
    rows = [mix_ref.fields(r, None, None) for r in rec.tolist()]
    partner = [r[0] for r in rows]
    ws, wp, lam = (np.array([r[k] for r in rows], dtype=np.float32) for k in (1, 2, 4))
    box = np.array([r[3] for r in rows])
    assert box.min() >= 0 and box.max() <= D
    return partner, ws, wp, box, lam


def _flip_partners(sizes):
    return [m - 1 - b for m in sizes for b in range(m)]


SIZES = [16, 16, 7]                                                  # an odd last batch


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_draw_is_reproducible_and_typed(mode):
    m = qat_vit_amd.MixupCutmix(mode=mode)
    r1, r2 = m.draw(SIZES, 224, torch.Generator().manual_seed(5)), m.draw(SIZES, 224, torch.Generator().manual_seed(5))
    assert r1.dtype == torch.int32 and r1.shape == (39, 6) and not r1.is_cuda and r1.is_contiguous() and torch.equal(r1, r2)
    assert not torch.equal(r1, m.draw(SIZES, 224, torch.Generator().manual_seed(6)))
    assert r1[:, 0].tolist() == _flip_partners(SIZES)
    per_batch = [len({tuple(r[1:]) for r in r1[o:o + n].tolist()}) for o, n in ((0, 16), (16, 16), (32, 7))]
    assert per_batch == [1, 1, 1] if mode == "batch" else min(per_batch) > 1
    assert m.draw([], 224).shape == (0, 6)
    torch.manual_seed(3)                                             # no generator: torch's default one
    d1 = m.draw([5], 32)
    torch.manual_seed(3)
    assert torch.equal(d1, m.draw([5], 32))


def test_prob_zero_gives_identity_records():
    for kw in ({"prob": 0}, {"mixup_alpha": 0, "cutmix_alpha": 0}):
        rec = qat_vit_amd.MixupCutmix(mode="elem", **kw).draw(SIZES, 224, torch.Generator().manual_seed(1))
        want = [mix_ref.record(p) for p in _flip_partners(SIZES)]
        assert rec.tolist() == want
        assert want[0][1:] == [0x3f800000, 0, 0, 0, 0x3f800000]


def test_mixup_only_rows():
    D = 224
    rec = qat_vit_amd.MixupCutmix(mixup_alpha=0.8, cutmix_alpha=0, mode="elem").draw([256], D, torch.Generator().manual_seed(2))
    partner, ws, wp, box, lam = _columns(rec, D)
    assert partner == _flip_partners([256])
    assert not box.any()                                             # the empty box
    assert ((ws >= 0) & (ws <= 1)).all() and len(set(ws.tolist())) > 200
    assert np.array_equal(wp, np.float32(1) - ws) and np.array_equal(lam, ws)
    assert (np.abs(ws.astype(np.float64) + wp.astype(np.float64) - 1.0) <= 2.0 ** -24).all()     # w_self + w_partner == 1 to fp32 rounding
    # the rule itself, restated: rand(2) float64, then the gamma pair
    g = torch.Generator().manual_seed(2)
    for k in range(8):
        torch.rand(2, dtype=torch.float64, generator=g)
        x = torch._standard_gamma(torch.full((2,), 0.8, dtype=torch.float64), generator=g)
        assert ws[k] == np.float32(float(x[0] / (x[0] + x[1])))


def test_cutmix_only_rows():
    D = 224
    rec = qat_vit_amd.MixupCutmix(mixup_alpha=0, cutmix_alpha=1.0, mode="elem").draw([256], D, torch.Generator().manual_seed(4))
    partner, ws, wp, box, lam = _columns(rec, D)
    assert partner == _flip_partners([256])
    assert (ws == 1).all() and (wp == 0).all()
    area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
    assert (box[:, 1] >= box[:, 0]).all() and (box[:, 3] >= box[:, 2]).all() and (area > 0).sum() > 200
    assert np.array_equal(lam, (1.0 - area / float(D * D)).astype(np.float32))
    assert ((box == 0) | (box == D)).any()                           # some box was clamped at an edge
    g = torch.Generator().manual_seed(4)
    for k in range(8):
        torch.rand(2, dtype=torch.float64, generator=g)
        x = torch._standard_gamma(torch.full((2,), 1.0, dtype=torch.float64), generator=g)
        cy, cx = torch.randint(0, D, (2,), generator=g).tolist()
        h = int(D * float(np.sqrt(1.0 - float(x[0] / (x[0] + x[1])))))
        clip = lambda v: min(max(v, 0), D)   # noqa: E731
        assert tuple(box[k]) == (clip(cy - h // 2), clip(cy + h // 2), clip(cx - h // 2), clip(cx + h // 2))


def test_switching_and_probability():
    D, n = 224, 400
    rec = qat_vit_amd.MixupCutmix(prob=0.5, switch_prob=0.5, mode="elem").draw([n], D, torch.Generator().manual_seed(9))
    _, ws, wp, box, lam = _columns(rec, D)
    ident = (ws == 1) & (wp == 0) & ~box.any(1)
    cut = (ws == 1) & (wp == 0) & box.any(1)
    mixup = ~ident & ~cut
    assert 120 < ident.sum() < 280 and 50 < cut.sum() < 150 and 50 < mixup.sum() < 150
    assert (lam[ident] == 1).all() and not box[mixup].any()
    # one decision per batch in "batch" mode, the partners still flipped per batch
    rec = qat_vit_amd.MixupCutmix(mode="batch").draw([4, 4, 3], D, torch.Generator().manual_seed(9))
    assert rec[:, 0].tolist() == [3, 2, 1, 0, 3, 2, 1, 0, 2, 1, 0]
