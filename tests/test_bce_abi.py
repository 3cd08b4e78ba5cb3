"""CPU-side checks of the binary cross-entropy objective (qatvit_kd_bce_loss, F.kd_bce_loss, qat_vit_amd.BinaryCrossEntropy,
TeacherLogitTable.bce_loss): the symbol in the header, the binding and the library; every argument error as a string without a HIP call; the fp64
reference of tests/bce_ref.py against an independent construction of timm's target; the wrappers' refusal of CPU tensors."""
import os
import re
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native
from tests import bce_ref, mix_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qatvit_kd_bce_loss"
CTYPE = {"int32_t": native.c_int32, "int64_t": native.c_int64, "float": native.c_float}


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert decl, f"{name} is not declared in include/qatvit.h"
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_symbol_in_header_signatures_and_exports(native_lib):
    params = _params(NAME)
    assert params == ["const float* student", "const float* teacher", "const float* table", "int64_t table_rows", "const int64_t* index",
                      "const int64_t* labels", "const int32_t* mix", "int64_t batch", "int64_t classes", "float kd_temp", "float kd_alpha",
                      "float label_smoothing", "float target_threshold", "int32_t sum_classes", "float* partials", "float* out3", "float* dlogits",
                      "void* stream"]
    res, args = native.SIGNATURES[NAME]
    assert res is native.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        assert a is (native.c_void_p if "*" in p else CTYPE[p.split()[0]]), p
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4                      # an added symbol: the version stays
    assert "BinaryCrossEntropy" in qat_vit_amd.__all__ and issubclass(qat_vit_amd.BinaryCrossEntropy, torch.nn.Module)
    assert callable(F.kd_bce_loss) and callable(qat_vit_amd.TeacherLogitTable.bce_loss)


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def refused(msg, student=p, teacher=None, table=None, rows=0, index=None, labels=p, mix=p, B=8, C=10, T=4.0, eps=0.1, partials=p, out3=p,
                dlogits=p):
        assert L.qatvit_kd_bce_loss(student, teacher, table, rows, index, labels, mix, B, C, T, 0.5, eps, -1.0, 0, partials, out3, dlogits, None) != 0
        assert msg in L.qatvit_last_error() and NAME.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for mix in (p, None):
        for name in ("student", "labels", "partials", "out3", "dlogits"):
            refused(b"null pointer", mix=mix, **{name: None})
        refused(b"mutually exclusive", teacher=p, table=p, rows=4, index=p, mix=mix)
        refused(b"needs an index", table=p, rows=4, mix=mix)
        refused(b"table_rows 0", table=p, rows=0, index=p, mix=mix)
        refused(b"table_rows -3", table=p, rows=-3, index=p, mix=mix)
        refused(b"bad shape", B=0, mix=mix)
        refused(b"bad shape", B=-1, mix=mix)
        refused(b"bad shape", C=1, mix=mix)
        refused(b"bad shape", C=4097, mix=mix)
        refused(b"kd_temp", T=0.0, mix=mix)
        refused(b"kd_temp", T=-1.0, mix=mix)
        refused(b"label_smoothing", eps=1.0, mix=mix)
        refused(b"label_smoothing", eps=-0.01, mix=mix)
        refused(b"label_smoothing", eps=float("nan"), mix=mix)
    for off in (1, 2, 3):
        refused(b"misaligned mix", mix=p + off)
        refused(b"misaligned mix", mix=p + off, teacher=p)
        refused(b"misaligned mix", mix=p + off, table=p, rows=4, index=p)


PAIRS = [(thr, sc) for thr in (None, 0.2) for sc in (False, True)]


@pytest.mark.parametrize("C", [3, 10])
def test_reference_equals_the_timm_target_construction(C):
    """full(off).scatter_(on), mixed with the partner rows as timm's Mixup mixes them - one lam per batch with the flipped batch as partners
    ("batch" mode) and one lam per row ("elem" mode) - with and without threshold and sum_classes.  The lams are exact in fp32, so 1 - lam is the
    same number in both constructions."""
    B = 6
    g = torch.Generator().manual_seed(C)
    y, s = torch.randint(0, C, (B,), generator=g), 3 * torch.randn(B, C, generator=g, dtype=torch.float64)
    flip = list(range(B - 1, -1, -1))
    arms = [([0.75] * B, flip), ([1.0, 0.0, 0.5, 0.25, 0.875, 0.75], flip), ([0.5, 0.25, 1.0, 0.75, 0.0, 0.5], [2, 2, 0, 5, 1, 5]), ([1.0] * B, flip)]
    for eps in (0.0, 0.1):
        for lams, part in arms:
            recs = torch.tensor([mix_ref.mixup(p, l) for p, l in zip(part, lams)], dtype=torch.int32)
            for thr, sc in PAIRS:
                want_t = bce_ref.timm_target(y, C, lams, None if part == flip else part, eps, thr)
                got_t = bce_ref.targets(y, C, recs, eps, thr)
                assert torch.allclose(got_t, want_t, rtol=0, atol=1e-15)
                per = torch.nn.functional.binary_cross_entropy_with_logits(s, want_t, reduction="none")     # timm: .sum(-1).mean() or the mean
                want = per.sum(-1).mean() if sc else per.mean()
                got = bce_ref.loss(s, y, recs, label_smoothing=eps, target_threshold=thr, sum_classes=sc)
                assert abs(float(got[0]) - float(want)) < 1e-13 * max(1.0, abs(float(want))) and float(got[2]) == 0.0
                assert torch.equal(got[0], got[1])
                dev = bce_ref.composition(s, y, recs, label_smoothing=eps, target_threshold=thr, sum_classes=sc)
                assert abs(float(dev[0]) - float(want)) < 1e-13 * max(1.0, abs(float(want)))
    # no records: lam = 1 everywhere; the smoothed one-hot itself at eps = 0.1
    assert torch.equal(bce_ref.targets(y, C), bce_ref.timm_target(y, C))
    assert float(bce_ref.targets(y, C).sum()) == pytest.approx(B)
    # the threshold applies after smoothing and mixing: with eps = 0.1 and lam = 0.75 the partner's 0.225 + eps / C passes 0.2, the off value does not
    t = bce_ref.targets(torch.tensor([0, 1]), C, torch.tensor([mix_ref.mixup(1, 0.75), mix_ref.mixup(0, 0.75)], dtype=torch.int32), 0.1, 0.2)
    assert t[0].tolist() == [1.0, 1.0] + [0.0] * (C - 2)


def test_reference_kd_part_and_composition_agree():
    B, C = 5, 7
    g = torch.Generator().manual_seed(4)
    s, t, table = (3 * torch.randn(n, C, generator=g, dtype=torch.float64) for n in (B, B, B + 3))
    y, index = torch.randint(0, C, (B,), generator=g), torch.randperm(B + 3, generator=g)[:B]
    recs = torch.tensor([mix_ref.mixup(1, 1.0), mix_ref.mixup(3, 0.0), mix_ref.mixup(2, 0.3), mix_ref.mixup(B, 0.25), mix_ref.mixup(0, 0.5)],
                        dtype=torch.int32)
    for kw in ({"teacher": t}, {"table": table, "index": index}):
        for r in (recs, None):
            want = bce_ref.loss(s, y, r, kd_temp=3.0, kd_alpha=0.3, **kw)
            ce = mix_ref.loss(s, y, r, kd_temp=3.0, kd_alpha=0.3, **kw)
            assert float(want[2]) == float(ce[2]) and float(want[2]) > 0                           # the KD term is mix_ref's
            assert float(want[0]) == pytest.approx(0.3 * float(want[2]) + 0.7 * float(want[1]), rel=1e-14)
            got = bce_ref.composition(s, y, r, kd_temp=3.0, kd_alpha=0.3, **kw)
            for a, b in zip(got, want):
                assert float(a) == pytest.approx(float(b), rel=1e-12)


def test_python_wrappers_refuse_cpu_tensors():
    s, t, y = torch.zeros(2, 10), torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64)
    recs = torch.zeros(2, 6, dtype=torch.int32)
    for kw in ({}, {"teacher": t}, {"mix": recs}, {"table": torch.zeros(5, 10), "index": y}):
        with pytest.raises(RuntimeError, match="kd_bce_loss: qat-vit_amd ops run on MI355X only"):
            F.kd_bce_loss(s, y, **kw)
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.BinaryCrossEntropy()(s, y)
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.BinaryCrossEntropy(smoothing=0.0, target_threshold=0.2, sum_classes=True)(s, y, mix=recs)
    with pytest.raises(RuntimeError, match="target_threshold"):
        F.kd_bce_loss(s, y, target_threshold=torch.tensor(0.2))
    table = object.__new__(qat_vit_amd.TeacherLogitTable)           # a table on the host: refused before anything else is looked at
    table.logits = torch.zeros(5, 10)
    with pytest.raises(RuntimeError, match="MI355X only"):
        table.bce_loss(s, y, y, mix=recs)


def test_criterion_arguments():
    c = qat_vit_amd.BinaryCrossEntropy()
    assert (c.smoothing, c.target_threshold, c.sum_classes) == (0.1, None, False)
    c = qat_vit_amd.BinaryCrossEntropy(0.0, 0.2, True)
    assert (c.smoothing, c.target_threshold, c.sum_classes) == (0.0, 0.2, True) and "target_threshold=0.2" in repr(c)
    for kw in ({"smoothing": 1.0}, {"smoothing": -0.1}, {"smoothing": float("nan")}, {"target_threshold": 1.0}, {"target_threshold": -0.5},
               {"target_threshold": float("nan")}):
        with pytest.raises(ValueError):
            qat_vit_amd.BinaryCrossEntropy(**kw)
