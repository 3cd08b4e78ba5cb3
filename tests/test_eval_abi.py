"""CPU-side checks of on-device validation: the new symbol in the library, the header and native.py, its argument errors without a HIP call,
the refusal of CPU tensors, and the arithmetic of the result object from a hand-filled state block."""
import math
import os
import re
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.evaluate import COUNTERS, STATE_WORDS, EvalResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "qatvit_eval_accumulate"


def test_eval_symbol_in_exports_signatures_and_header(native_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert SYMBOL in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert SYMBOL in native.SIGNATURES and len(native.SIGNATURES[SYMBOL][1]) == 13
    assert native_lib.qatvit_abi_version() == 4
    text = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert SYMBOL in set(re.findall(r"\b(qatvit_[a-z0-9_]+)\s*\(", hdr))
    assert "#define QATVIT_ABI_VERSION 4" in hdr.replace("  ", " ")
    assert f"#define QATVIT_EVAL_STATE_WORDS {STATE_WORDS}" in hdr and STATE_WORDS == len(COUNTERS) + 1
    for k, name in enumerate(COUNTERS):      # the documented layout is the one the Python layer reads
        assert f"[{k}] {name}" in text, name
    assert f"[{len(COUNTERS)}] loss_sum" in text


def test_eval_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths (each call returns before any HIP call)
    ok = dict(logits=p, dtype=0, ld=10, labels=p, batch=4, classes=10, other=p, other_ld=10, index=p, rows=8, state=p, confusion=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.qatvit_eval_accumulate(a["logits"], a["dtype"], a["ld"], a["labels"], a["batch"], a["classes"], a["other"], a["other_ld"], a["index"],
                                        a["rows"], a["state"], a["confusion"], None)

    for name in ("logits", "labels", "state"):
        assert call(**{name: None}) != 0 and b"qatvit_eval_accumulate: null pointer" in L.qatvit_last_error(), name
    assert call(batch=0) != 0 and b"batch 0" in L.qatvit_last_error()
    assert call(batch=-2) != 0 and b"batch -2" in L.qatvit_last_error()
    assert call(classes=1) != 0 and b"classes 1" in L.qatvit_last_error()
    assert call(ld=9) != 0 and b"ld 9 is less than classes 10" in L.qatvit_last_error()
    for code in (3, -1):
        assert call(dtype=code) != 0 and b"unknown dtype code %d" % code in L.qatvit_last_error()
    assert call(other=None) != 0 and b"other_index given without other" in L.qatvit_last_error()
    assert call(other_ld=9) != 0 and b"other_ld 9 is less than classes 10" in L.qatvit_last_error()
    assert call(rows=0) != 0 and b"other_rows 0" in L.qatvit_last_error()
    assert call(rows=-1) != 0 and b"other_rows -1" in L.qatvit_last_error()
    assert call(state=p + 4) != 0 and b"misaligned" in L.qatvit_last_error()
    # without an index, other_rows is not looked at
    assert call(index=None, rows=0, logits=None) != 0 and b"null pointer" in L.qatvit_last_error()


def test_cpu_tensors_are_refused():
    logits, labels = torch.randn(4, 10), torch.randint(0, 10, (4,))
    acc = qat_vit_amd.EvalAccumulator(10)
    with pytest.raises(RuntimeError, match="MI355X only"):
        acc.update(logits, labels)
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.EvalAccumulator(10, device="cpu").update(logits, labels)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 10)).train()
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.evaluate(model, [(torch.randn(4, 3, 2, 2), labels)])
    assert model.training                      # refused before anything was touched
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.evaluate(lambda x: x.flatten(1)[:, :10], [(torch.randn(4, 3, 2, 2), labels)], device="cpu")
    with pytest.raises(ValueError, match="at least 2"):
        qat_vit_amd.EvalAccumulator(1)


def _state(loss_sum=0.0, **counts):
    s = torch.zeros(STATE_WORDS, dtype=torch.int64)
    for k, v in counts.items():
        s[COUNTERS.index(k)] = v
    s[len(COUNTERS):].view(torch.float64)[0] = loss_sum
    return s


def test_result_arithmetic_from_a_hand_filled_state():
    empty = qat_vit_amd.EvalAccumulator(10).result()      # nothing counted, nothing allocated: no GPU involved
    assert (empty.total, empty.correct, empty.accuracy) == (0, 0, 0.0) and math.isnan(empty.loss)
    assert empty.agree is None and empty.agreement is None and empty.other_correct is None
    assert empty.confusion.shape == (10, 10) and empty.confusion.dtype == torch.int64 and int(empty.confusion.sum()) == 0
    assert qat_vit_amd.EvalAccumulator(10, confusion=False).result().confusion is None

    conf = torch.tensor([[3, 1, 0], [0, 0, 0], [2, 0, 4]])
    r = EvalResult(_state(loss_sum=12.5, total=13, correct=7, bad_labels=2, nonfinite_rows=1, loss_rows=10), conf)
    assert r.accuracy == 100.0 * 7 / 13 and r.loss == 1.25 and r.loss_sum == 12.5
    assert (r.total, r.correct, r.bad_labels, r.nonfinite_rows, r.bad_index, r.loss_rows) == (13, 7, 2, 1, 0, 10)
    assert r.agree is None and r.agreement is None and r.other_correct is None
    pc = r.per_class_accuracy
    assert pc[0] == 75.0 and math.isnan(pc[1]) and pc[2] == 100.0 * 4 / 6 and r.confusion is conf
    assert "accuracy=" in repr(r)

    o = EvalResult(_state(total=8, correct=4, other_rows_seen=6, agree=3, other_correct=5, bad_index=2), None, had_other=True)
    assert (o.agree, o.other_correct, o.bad_index, o.agreement) == (3, 5, 2, 50.0) and o.per_class_accuracy is None and math.isnan(o.loss)
    z = EvalResult(_state(), None, had_other=True)         # a second opinion was given, but no row of it could be read
    assert z.agree == 0 and z.agreement == 0.0
    with pytest.raises(ValueError):
        EvalResult(torch.zeros(STATE_WORDS - 1, dtype=torch.int64))


def test_names_are_exported():
    assert "evaluate" in qat_vit_amd.__all__ and "EvalAccumulator" in qat_vit_amd.__all__
    assert callable(qat_vit_amd.evaluate) and isinstance(qat_vit_amd.EvalAccumulator, type)
