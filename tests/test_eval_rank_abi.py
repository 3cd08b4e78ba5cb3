"""CPU-side checks of validation at many classes (qatvit_eval_accumulate_rank; the topk / label_smoothing / per_class keywords of EvalAccumulator and
evaluate): the symbol in the library, the header and native.py; every argument error as a string without a HIP call; the keyword errors on the host;
the unchanged buffer and result with the keywords at their defaults."""
import os
import subprocess

import pytest

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.evaluate import RANK_BINS, RANK_STATE_WORDS, STATE_WORDS
from tests.test_bce_abi import CTYPE, ROOT, _params

NAME = "qatvit_eval_accumulate_rank"


def test_symbol_in_header_signatures_and_exports(native_lib):
    params = _params(NAME)
    assert params == ["const void* logits", "int32_t dtype", "int64_t ld", "const int64_t* labels", "int64_t batch", "int64_t classes",
                      "float label_smoothing", "const float* other", "int64_t other_ld", "const int64_t* other_index", "int64_t other_rows",
                      "void* state", "int64_t* class_counts", "void* stream"]
    res, args = native.SIGNATURES[NAME]
    assert res is native.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        assert a is (native.c_void_p if "*" in p else CTYPE[p.split()[0]]), p
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4                      # an added symbol: the version stays
    header = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    assert f"#define QATVIT_EVAL_RANK_BINS {RANK_BINS}\n" in header and f"#define QATVIT_EVAL_RANK_STATE_WORDS {RANK_STATE_WORDS}\n" in header
    assert RANK_STATE_WORDS == 10 + 2 * RANK_BINS


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths (each call returns before any HIP call)
    ok = dict(logits=p, dtype=0, ld=10, labels=p, batch=4, classes=10, eps=0.1, other=p, other_ld=10, index=p, rows=8, state=p, counts=p)

    def refused(msg, **kw):
        a = dict(ok, **kw)
        assert L.qatvit_eval_accumulate_rank(a["logits"], a["dtype"], a["ld"], a["labels"], a["batch"], a["classes"], a["eps"], a["other"], a["other_ld"],
                                             a["index"], a["rows"], a["state"], a["counts"], None) != 0
        assert msg in L.qatvit_last_error() and NAME.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    refused(b"null pointer", state=None)
    refused(b"classes 1 ", classes=1, ld=1)
    refused(b"classes 32769", classes=32769, ld=32769, other_ld=32769)
    refused(b"ld 9 is less than classes 10", ld=9)
    for code in (3, -1):
        refused(b"unknown dtype code %d" % code, dtype=code)
    for eps in (1.0, -0.1, float("nan")):
        refused(b"label_smoothing", eps=eps)
    refused(b"other_index given without other", other=None)
    refused(b"misaligned", counts=p + 4)


def test_keyword_errors_and_the_unchanged_default():
    for bad in ((), (0,), (32,), (1, 5.0), 5, "5", (True,), [1, -1]):
        with pytest.raises(ValueError, match="topk"):
            qat_vit_amd.EvalAccumulator(1000, topk=bad)
        with pytest.raises(ValueError, match="topk"):
            qat_vit_amd.evaluate(lambda x: x, [], device="cuda", topk=bad)
    with pytest.raises(ValueError, match="32768"):
        qat_vit_amd.EvalAccumulator(32769, confusion=False, topk=(1, 5))
    for C in (10, 1000):
        plain = qat_vit_amd.EvalAccumulator(C)
        assert plain._words() == STATE_WORDS + C * C and plain._rank_words() == 0 and qat_vit_amd.EvalAccumulator(C, confusion=False)._words() == STATE_WORDS
        r = plain.result()
        assert r.rank_hist is None and r.topk_accuracy is None and r.smoothed_loss is None and r.per_class_recall is None and r.other_rank_hist is None
        full = qat_vit_amd.EvalAccumulator(C, confusion=False, topk=[1, 31], label_smoothing=0.1, per_class=True)
        assert full._words() == STATE_WORDS and full._rank_words() == RANK_STATE_WORDS + 2 * C and full.topk == (1, 31)
