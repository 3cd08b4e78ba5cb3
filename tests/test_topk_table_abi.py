"""CPU-side checks of the compressed teacher table (qatvit_teacher_topk_rows, qatvit_kd_ce_loss_topk, qat_vit_amd.TeacherTopKTable): the symbols in
the header, the binding and the library; every argument error as a string without a HIP call; the record checks of TeacherTopKTable.load."""
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from tests.test_bce_abi import CTYPE, _params

TOPK, LOSS = "qatvit_teacher_topk_rows", "qatvit_kd_ce_loss_topk"
DECLARED = {
    TOPK: ["const float* logits", "int64_t batch", "int64_t classes", "int32_t k", "float build_temp", "int16_t* idx", "float* val", "float* tail",
           "void* stream"],
    LOSS: ["const float* student", "const int16_t* idx", "const float* val", "const float* tail", "int64_t table_rows", "int32_t k",
           "const int64_t* index", "const int64_t* labels", "const int32_t* mix", "int64_t batch", "int64_t classes", "float kd_temp", "float kd_alpha",
           "float label_smoothing", "float* partials", "float* out3", "float* dlogits", "void* stream"],
}


@pytest.mark.parametrize("name", [TOPK, LOSS])
def test_symbols_in_header_signatures_and_exports(native_lib, name):
    params = _params(name)
    assert params == DECLARED[name]
    res, args = native.SIGNATURES[name]
    assert res is native.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        assert a is (native.c_void_p if "*" in p else CTYPE[p.split()[0]]), p
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert name in {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4                      # added symbols: the version stays
    assert "TeacherTopKTable" in qat_vit_amd.__all__


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths

    def topk(msg, logits=p, B=8, C=10, k=3, Tb=4.0, idx=p, val=p, tail=p):
        assert L.qatvit_teacher_topk_rows(logits, B, C, k, Tb, idx, val, tail, None) != 0
        assert msg in L.qatvit_last_error() and TOPK.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    def loss(msg, student=p, idx=p, val=p, tail=p, rows=4, k=3, index=p, labels=p, mix=None, B=8, C=10, T=4.0, eps=0.1, partials=p, out3=p, dlogits=p):
        assert L.qatvit_kd_ce_loss_topk(student, idx, val, tail, rows, k, index, labels, mix, B, C, T, 0.5, eps, partials, out3, dlogits, None) != 0
        assert msg in L.qatvit_last_error() and LOSS.encode() in L.qatvit_last_error(), L.qatvit_last_error()

    for name in ("logits", "idx", "val", "tail"):
        topk(b"null pointer", **{name: None})
    for name in ("student", "idx", "val", "tail", "index", "labels", "partials", "out3", "dlogits"):
        loss(b"null pointer", **{name: None})
    for refused in (topk, loss):
        for k, C in ((0, 10), (-1, 10), (65, 1000), (10, 10), (64, 64), (2, 2)):
            refused(b"is outside 1 .. min(64, C - 1)", k=k, C=C)
        for C in (1, 32769):
            refused(b"bad shape", C=C, k=1)
        refused(b"bad shape", B=0)
        refused(b"misaligned", idx=p + 1)
        refused(b"misaligned", val=p + 2)
        refused(b"misaligned", tail=p + 1)
    topk(b"misaligned", logits=p + 2)
    for Tb in (0.0, -1.0, float("nan")):
        topk(b"build_temp must be > 0", Tb=Tb)
    loss(b"kd_temp", T=0.0)
    loss(b"table_rows 0", rows=0)
    loss(b"label_smoothing", eps=1.0)
    loss(b"misaligned mix", mix=p + 2)


def test_load_names_the_differing_field(tmp_path):
    meta = {"format": 101, "N": 3, "C": 10, "teacher_form": 1, "transform": (), "data_digest": "", "param_digest": "", "k": 2, "tail_temp": 4.0}
    idx, val, tail = torch.tensor([[1, 0], [9, 3], [4, 5]], dtype=torch.int16), torch.randn(3, 2), torch.randn(3)
    path = str(tmp_path / "t.pt")
    qat_vit_amd.TeacherTopKTable(idx, val, tail, meta).save(path)
    back = qat_vit_amd.TeacherTopKTable.load(path, device="cpu", k=2, tail_temp=4.0, C=10)
    assert torch.equal(back.idx, idx) and torch.equal(back.val, val) and torch.equal(back.tail, tail) and back.nbytes == 3 * (6 * 2 + 4)
    for field, kw in (("k", {"k": 3}), ("tail_temp", {"tail_temp": 2.0}), ("C", {"C": 1000})):
        with pytest.raises(ValueError, match=field + " differs"):
            qat_vit_amd.TeacherTopKTable.load(path, device="cpu", **kw)
    dense = str(tmp_path / "d.pt")
    torch.save({"logits": torch.zeros(3, 10), "meta": dict(meta, format=1)}, dense)
    with pytest.raises(ValueError, match="table format 1"):
        qat_vit_amd.TeacherTopKTable.load(dense, device="cpu")
    with pytest.raises(RuntimeError, match="MI355X only"):
        back.loss(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
