"""CPU-side checks of the 16-bit-logit loss entries (qatvit_kd_ce_loss_rows16 / _topk16, qatvit_kd_bce_loss_topk16): each is the fp32 entry's
declaration with `const void* student, int32_t dtype`, `const float* grad_scale` in front of `partials` and `void* dlogits`; the binding and the
export; the refusals as strings without a HIP call.  (That a 16-bit student with class_parallel=False still raises "expected float32" needs a GPU
tensor - the device check comes first - and is in tests/test_gpu_loss16.py.)"""
import subprocess

import pytest

from qat_vit_amd import native
from tests.test_bce_abi import CTYPE, _params

FP32 = {"qatvit_kd_ce_loss_rows16": "qatvit_kd_ce_loss_rows", "qatvit_kd_ce_loss_topk16": "qatvit_kd_ce_loss_topk",
        "qatvit_kd_bce_loss_topk16": "qatvit_kd_bce_loss_topk"}


@pytest.mark.parametrize("name", FP32)
def test_signature_is_the_fp32_entrys_with_the_documented_changes(native_lib, name):
    want = _params(FP32[name])
    want[0:1] = ["const void* student", "int32_t dtype"]
    want[want.index("float* partials"):want.index("float* partials")] = ["const float* grad_scale"]
    want[want.index("float* dlogits")] = "void* dlogits"
    params = _params(name)
    assert params == want
    res, args = native.SIGNATURES[name]
    assert res is native.c_int and [a is (native.c_void_p if "*" in p else CTYPE[p.split()[0]]) for p, a in zip(params, args)] == [True] * len(params)
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert name in {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4   # added symbols: the version stays


REFUSALS = [("dtype", FP32), ("student", b"null pointer"), ("k", b"is outside 1 .. min(64, C - 1)"), ("C", b"bad shape"),
            ("odd", b"misaligned student or dlogits"), ("odd_out", b"misaligned student or dlogits"), ("unknown", b"unknown dtype code 3")]


@pytest.mark.parametrize("name,what,msg", [(n, w, m) for n in FP32 for w, m in REFUSALS if not (w == "k" and n == "qatvit_kd_ce_loss_rows16")],
                         ids=lambda v: v if isinstance(v, str) else "")   # (the rows entry has no k)
def test_refusals_leave_the_error_text(native_lib, name, what, msg):
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths
    student = {"student": None, "odd": p + 1}.get(what, p)
    dtype = {"dtype": 0, "unknown": 3}.get(what, 2)
    k, C = (65 if what == "k" else 3), (32769 if what == "C" else 1000)
    tail = (p, p, p, p + 1 if what == "odd_out" else p, None)   # grad_scale, partials, out3, dlogits, stream
    if name == "qatvit_kd_ce_loss_rows16":
        rc = native_lib.qatvit_kd_ce_loss_rows16(student, dtype, None, p, 4, p, p, None, 8, C, 4.0, 0.5, 0.1, *tail)
    elif name == "qatvit_kd_ce_loss_topk16":
        rc = native_lib.qatvit_kd_ce_loss_topk16(student, dtype, p, p, p, 4, k, p, p, None, 8, C, 4.0, 0.5, 0.1, *tail)
    else:
        rc = native_lib.qatvit_kd_bce_loss_topk16(student, dtype, p, p, p, 4, k, p, p, None, 8, C, 4.0, 0.5, 0.1, -1.0, 0, *tail)
    err = native_lib.qatvit_last_error()
    assert rc != 0 and name.encode() in err, err
    assert (msg[name].encode() + b",") in err if what == "dtype" else msg in err, err   # fp32 logits: the text names the fp32 entry
