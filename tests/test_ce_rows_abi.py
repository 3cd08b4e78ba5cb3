"""CPU-side checks of the class-parallel KD + CE loss (qatvit_kd_ce_loss_rows, the class_parallel keyword of F.kd_ce_loss and its siblings): the
symbol in the header, the binding and the library; every argument error as a string without a HIP call; the wrappers' refusal of CPU tensors."""
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native
from tests.test_bce_abi import CTYPE, _params

NAME = "qatvit_kd_ce_loss_rows"


def test_symbol_in_header_signatures_and_exports(native_lib):
    params = _params(NAME)
    assert params == ["const float* student", "const float* teacher", "const float* table", "int64_t table_rows", "const int64_t* index",
                      "const int64_t* labels", "const int32_t* mix", "int64_t batch", "int64_t classes", "float kd_temp", "float kd_alpha",
                      "float label_smoothing", "float* partials", "float* out3", "float* dlogits", "void* stream"]
    res, args = native.SIGNATURES[NAME]
    assert res is native.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        assert a is (native.c_void_p if "*" in p else CTYPE[p.split()[0]]), p
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4                      # an added symbol: the version stays


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def refused(msg, student=p, teacher=None, table=None, rows=0, index=None, labels=p, mix=p, B=8, C=10, T=4.0, eps=0.1, partials=p, out3=p, dlogits=p):
        assert L.qatvit_kd_ce_loss_rows(student, teacher, table, rows, index, labels, mix, B, C, T, 0.5, eps, partials, out3, dlogits, None) != 0
        assert msg in L.qatvit_last_error() and NAME.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for mix in (p, None):
        for name in ("student", "labels", "partials", "out3", "dlogits"):
            refused(b"null pointer", mix=mix, **{name: None})
        refused(b"mutually exclusive", teacher=p, table=p, rows=4, index=p, mix=mix)
        refused(b"needs an index", table=p, rows=4, mix=mix)
        refused(b"table_rows 0", table=p, rows=0, index=p, mix=mix)
        refused(b"bad shape", B=0, mix=mix)
        refused(b"bad shape", B=2 ** 30, mix=mix)
        refused(b"bad shape", C=1, mix=mix)
        refused(b"bad shape", C=32769, mix=mix)
        refused(b"kd_temp", T=0.0, mix=mix)
        refused(b"label_smoothing", eps=1.0, mix=mix)
        refused(b"label_smoothing", eps=float("nan"), mix=mix)
    for off in (1, 2, 3):
        refused(b"misaligned mix", mix=p + off)
        refused(b"misaligned mix", mix=p + off, table=p, rows=4, index=p)


def test_python_wrappers_refuse_cpu_tensors():
    s, t, y, recs, tab = torch.zeros(2, 10), torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 6, dtype=torch.int32), torch.zeros(5, 10)
    calls = {"kd_ce_loss": lambda: F.kd_ce_loss(s, t, y, class_parallel=True),
             "kd_ce_loss_table": lambda: F.kd_ce_loss_table(s, tab, y, y, class_parallel=True),
             "kd_ce_loss_mix": lambda: F.kd_ce_loss_mix(s, None, y, recs, class_parallel=True),
             "kd_ce_loss_table_mix": lambda: F.kd_ce_loss_table_mix(s, tab, y, y, recs, class_parallel=True)}
    for who, call in calls.items():
        with pytest.raises(RuntimeError, match=who + ": qat-vit_amd ops run on MI355X only"):
            call()
    table = object.__new__(qat_vit_amd.TeacherLogitTable)           # a table on the host: refused before anything else is looked at
    table.logits = tab
    with pytest.raises(RuntimeError, match="MI355X only"):
        table.loss(s, y, y, mix=recs, class_parallel=True)
