"""CPU-side checks of the bf16 (autocast) form of the native float student step: the C ABI symbols, workspace sizes, shape limits and the
opt-in off the GPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_SYMBOLS = {"qatvit_float_student_bf16_workspace_bytes", "qatvit_float_student_bf16_init", "qatvit_float_student_bf16_forward",
                "qatvit_float_student_bf16_backward", "qatvit_float_student_bf16_attn_backward"}


def _cfg(**kw):
    c = dict(batch=8, img_size=224, patch_size=16, in_chans=3, embed_dim=384, depth=12, num_heads=6, mlp_hidden=1536, num_classes=10,
             act_qmin=0, act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, ln_eps=1e-6)
    c.update(kw)
    return native.Cfg(**c)


def test_bf16_symbols_in_header_signatures_and_exports(native_lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(qatvit_[a-z0-9_]+)\s*\(", hdr))
    assert BF16_SYMBOLS <= declared
    assert BF16_SYMBOLS <= set(native.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert BF16_SYMBOLS <= exported
    assert native_lib.qatvit_abi_version() == 4


def test_bf16_workspace_grows_with_batch_and_is_below_the_fp32_form(native_lib):
    wsb = native_lib.qatvit_float_student_bf16_workspace_bytes
    ws32 = native_lib.qatvit_float_student_workspace_bytes
    ws16 = native_lib.qatvit_float_student_amp_workspace_bytes
    b7, b8, b1024 = (wsb(ctypes.byref(_cfg(batch=b))) for b in (7, 8, 1024))
    assert 0 < b7 < b8 < b1024
    vitb = dict(embed_dim=768, num_heads=12, mlp_hidden=3072)
    for kw in (dict(), vitb):
        for b in (8, 256, 1024):
            c = ctypes.byref(_cfg(batch=b, **kw))
            assert 0 < wsb(c) < ws32(c)
            assert wsb(c) <= ws16(c)   # the fp16 form's planes without its amax slots


def test_bf16_refuses_unsupported_shapes_with_a_message(native_lib):
    wsb = native_lib.qatvit_float_student_bf16_workspace_bytes
    assert native_lib.qatvit_float_student_workspace_bytes(ctypes.byref(_cfg(embed_dim=256, num_heads=4, mlp_hidden=1024))) > 0
    for bad in (dict(embed_dim=256, num_heads=4, mlp_hidden=1024), dict(mlp_hidden=1280), dict(num_heads=4), dict(img_size=256),
                dict(depth=13), dict(embed_dim=1152, num_heads=18, mlp_hidden=4608)):
        assert wsb(ctypes.byref(_cfg(**bad))) == -1, bad
        assert b"float student bf16: unsupported config" in native_lib.qatvit_last_error()
    assert wsb(None) == -1
    assert b"null argument" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_bf16_init(None, None, None) != 0
    assert b"null argument" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_bf16_forward(None, None, None, None, None, None) != 0
    assert b"null argument" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_bf16_backward(None, None, None, None, None, None) != 0
    assert b"null argument" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_bf16_attn_backward(None, None, None, None, 1, 197, 6, 384, None, None) != 0
    assert b"attn_bwd_bf16: unsupported arguments" in native_lib.qatvit_last_error()
    # the other forms keep their own messages
    assert native_lib.qatvit_float_student_amp_workspace_bytes(ctypes.byref(_cfg(mlp_hidden=1280))) == -1
    assert b"float student amp: unsupported config" in native_lib.qatvit_last_error()


def test_amp_argument_selects_the_autocast_dtypes():
    from qat_vit_amd.float_engine import autocast_dtypes

    assert autocast_dtypes(False) == () and autocast_dtypes(True) == (torch.float16,)
    assert autocast_dtypes(torch.bfloat16) == (torch.bfloat16,)
    assert autocast_dtypes((torch.float16, torch.bfloat16)) == (torch.float16, torch.bfloat16)
    with pytest.raises(ValueError, match="autocast dtypes"):
        autocast_dtypes(torch.float32)


def test_native_float_bf16_refuses_a_cpu_model():
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=384, depth=1, num_heads=6, img_size=32)
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        qat_vit_amd.native_float(stu, amp=torch.bfloat16)
    assert not qat_vit_amd.float_engine.is_native_float(stu)
