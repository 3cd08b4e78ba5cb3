"""CPU-side checks of the native float (pre-QAT) student step's boundary: the C ABI symbols, and the opt-in's behaviour off the GPU."""
import os
import re
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_SYMBOLS = {"qatvit_float_student_workspace_bytes", "qatvit_float_student_init", "qatvit_float_student_forward", "qatvit_float_student_backward"}
TINY = dict(embed_dim=128, depth=2, num_heads=2, img_size=32)


def test_float_symbols_in_header_signatures_and_exports(native_lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(qatvit_[a-z0-9_]+)\s*\(", hdr))
    assert FLOAT_SYMBOLS <= declared
    assert FLOAT_SYMBOLS <= set(native.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert FLOAT_SYMBOLS <= exported
    assert native_lib.qatvit_abi_version() == 4


def _cfg(**kw):
    c = dict(batch=8, img_size=224, patch_size=16, in_chans=3, embed_dim=384, depth=12, num_heads=6, mlp_hidden=1536, num_classes=10,
             act_qmin=0, act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, ln_eps=1e-6)
    c.update(kw)
    return native.Cfg(**c)


def test_float_workspace_size_and_shape_limits_without_a_gpu(native_lib):
    import ctypes

    ws = native_lib.qatvit_float_student_workspace_bytes
    b8, b1024, b7 = (ws(ctypes.byref(_cfg(batch=b))) for b in (8, 1024, 7))
    assert 0 < b7 < b8 < b1024          # the batch is a run-time argument: a larger workspace serves every smaller batch
    assert ws(ctypes.byref(_cfg(embed_dim=768, num_heads=12, mlp_hidden=3072))) > b8
    for bad in (dict(embed_dim=320, num_heads=5, mlp_hidden=1280), dict(num_heads=4), dict(embed_dim=896, num_heads=14), dict(img_size=256)):
        assert ws(ctypes.byref(_cfg(**bad))) == -1, bad
        assert b"float student: unsupported config" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_forward(None, None, None, None, None, None) != 0
    assert b"null argument" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_backward(None, None, None, None, None, None) != 0


def test_native_float_refuses_a_cpu_model():
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **TINY)
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        qat_vit_amd.native_float(stu)
    with pytest.raises(TypeError, match="QATWrapper"):
        qat_vit_amd.native_float(stu.model)
    assert not qat_vit_amd.float_engine.is_native_float(stu)


def test_shape_check_names_what_is_unsupported():
    from qat_vit_amd.float_engine import check_shape

    check_shape(qat_vit_amd.create_student("vit", num_classes=10, **TINY))
    with pytest.raises(RuntimeError, match="head_dim"):
        check_shape(qat_vit_amd.create_student("vit", num_classes=10, embed_dim=128, depth=1, num_heads=8, img_size=32))
    with pytest.raises(RuntimeError, match="tokens"):
        check_shape(qat_vit_amd.create_student("vit", num_classes=10, embed_dim=128, depth=1, num_heads=2, img_size=256))


def test_unprepared_wrapper_without_opt_in_is_stock_on_cpu():
    torch.manual_seed(0)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **TINY)
    x = torch.randn(3, 3, 32, 32)
    out = stu(x)
    ref = stu.model.head(stu.model.forward_features(x)[:, 0])
    assert torch.equal(out, ref) and not out.is_cuda
    out.sum().backward()
    assert all(p.grad is not None for p in stu.parameters())
