"""CPU-side checks of qatvit_kd_bce_loss_topk (F.kd_bce_loss_topk, TeacherTopKTable.bce_loss): the symbol in the header, the binding and the library;
the argument errors as strings without a HIP call; the wrappers' refusal of CPU tensors."""
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native
from tests.test_bce_abi import CTYPE, _params

NAME = "qatvit_kd_bce_loss_topk"


def test_symbol_in_header_signatures_and_exports(native_lib):
    params = _params(NAME)
    assert params == ["const float* student", "const int16_t* idx", "const float* val", "const float* tail", "int64_t table_rows", "int32_t k",
                      "const int64_t* index", "const int64_t* labels", "const int32_t* mix", "int64_t batch", "int64_t classes", "float kd_temp",
                      "float kd_alpha", "float label_smoothing", "float target_threshold", "int32_t sum_classes", "float* partials", "float* out3",
                      "float* dlogits", "void* stream"]
    res, args = native.SIGNATURES[NAME]
    assert res is native.c_int and [a is (native.c_void_p if "*" in p else CTYPE[p.split()[0]]) for p, a in zip(params, args)] == [True] * len(params)
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4                      # an added symbol: the version stays


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def refused(msg, table=True, student=p, val=p, tail=p, rows=4, k=3, index=p, labels=p, mix=None, C=10, T=4.0, eps=0.1, partials=p):
        assert L.qatvit_kd_bce_loss_topk(student, p if table else None, val, tail, rows, k, index, labels, mix, 8, C, T, 0.5, eps, -1.0, 0, partials, p, p, None) != 0
        assert msg in L.qatvit_last_error() and NAME.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for table in (True, False):
        for name in ("student", "labels", "partials"):
            refused(b"null pointer", table, **{name: None})
        for C in (1, 32769):
            refused(b"bad shape", table, C=C, k=1)
        refused(b"kd_temp", table, T=0.0)
        refused(b"label_smoothing", table, eps=1.0)
        for off in (1, 2, 3):
            refused(b"misaligned mix", table, mix=p + off)
    for k, C in ((0, 10), (10, 10), (65, 1000)):                     # k = 0, k = C, k past a wave
        refused(b"is outside 1 .. min(64, C - 1)", k=k, C=C)
    for name in ("val", "tail", "index"):
        refused(b"needs val, tail and an index", **{name: None})
    refused(b"table_rows 0", rows=0)
    refused(b"misaligned table", val=p + 2)


def test_python_wrappers_refuse_cpu_tensors():
    s, y = torch.zeros(2, 5000), torch.zeros(2, dtype=torch.int64)
    for fn, who in ((F.kd_bce_loss, "kd_bce_loss"), (F.kd_bce_loss_topk, "kd_bce_loss_topk")):   # above 4096 classes both are the new entry's wrapper
        with pytest.raises(RuntimeError, match=who + ": qat-vit_amd ops run on MI355X only"):
            fn(s, y)
    with pytest.raises(RuntimeError, match="target_threshold"):
        F.kd_bce_loss_topk(s, y, target_threshold=torch.tensor(0.2))
    assert callable(qat_vit_amd.TeacherTopKTable.bce_loss)
