"""CPU-side checks of the fp16 (autocast) form of the native float student step: the C ABI symbols, workspace sizes, shape limits and the
opt-in off the GPU."""
import ctypes
import os
import re
import subprocess

import pytest

import qat_vit_amd
from qat_vit_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMP_SYMBOLS = {"qatvit_float_student_amp_workspace_bytes", "qatvit_float_student_amp_init", "qatvit_float_student_amp_forward",
               "qatvit_float_student_amp_backward", "qatvit_float_student_amp_attn_backward"}


def _cfg(**kw):
    c = dict(batch=8, img_size=224, patch_size=16, in_chans=3, embed_dim=384, depth=12, num_heads=6, mlp_hidden=1536, num_classes=10,
             act_qmin=0, act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, ln_eps=1e-6)
    c.update(kw)
    return native.Cfg(**c)


def test_amp_symbols_in_header_signatures_and_exports(native_lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(qatvit_[a-z0-9_]+)\s*\(", hdr))
    assert AMP_SYMBOLS <= declared
    assert AMP_SYMBOLS <= set(native.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert AMP_SYMBOLS <= exported
    assert native_lib.qatvit_abi_version() == 4


def test_amp_workspace_grows_with_batch_and_is_below_the_fp32_form(native_lib):
    ws16 = native_lib.qatvit_float_student_amp_workspace_bytes
    ws32 = native_lib.qatvit_float_student_workspace_bytes
    b7, b8, b1024 = (ws16(ctypes.byref(_cfg(batch=b))) for b in (7, 8, 1024))
    assert 0 < b7 < b8 < b1024
    for b in (8, 256, 1024):
        assert ws16(ctypes.byref(_cfg(batch=b))) < ws32(ctypes.byref(_cfg(batch=b)))
    vitb = dict(embed_dim=768, num_heads=12, mlp_hidden=3072)
    assert 0 < ws16(ctypes.byref(_cfg(**vitb))) < ws32(ctypes.byref(_cfg(**vitb)))


def test_amp_refuses_unsupported_shapes_with_a_message(native_lib):
    ws16 = native_lib.qatvit_float_student_amp_workspace_bytes
    # the fp32 form covers a 128-wide model, the fp16 form needs multiples of 384
    assert native_lib.qatvit_float_student_workspace_bytes(ctypes.byref(_cfg(embed_dim=256, num_heads=4, mlp_hidden=1024))) > 0
    for bad in (dict(embed_dim=256, num_heads=4, mlp_hidden=1024), dict(mlp_hidden=1280), dict(num_heads=4), dict(img_size=256)):
        assert ws16(ctypes.byref(_cfg(**bad))) == -1, bad
        assert b"float student amp: unsupported config" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_amp_forward(None, None, None, None, None, None) != 0
    assert b"null argument" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_amp_backward(None, None, None, None, None, None) != 0
    assert native_lib.qatvit_float_student_amp_attn_backward(None, None, None, None, 1, 197, 6, 384, None, None) != 0
    assert b"attn_bwd_f16: unsupported arguments" in native_lib.qatvit_last_error()


def test_amp_shape_check_names_the_384_limit():
    from qat_vit_amd.float_engine import check_shape

    m = qat_vit_amd.create_student("vit", num_classes=10, embed_dim=128, depth=2, num_heads=2, img_size=32)
    check_shape(m)
    with pytest.raises(RuntimeError, match="multiples of 384"):
        check_shape(m, amp=True)
    check_shape(qat_vit_amd.create_model("vit_small_patch16_224_student", pretrained=False, num_classes=10), amp=True)


def test_native_float_amp_refuses_a_cpu_model():
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=384, depth=1, num_heads=6, img_size=32)
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        qat_vit_amd.native_float(stu, amp=True)
    assert not qat_vit_amd.float_engine.is_native_float(stu)
