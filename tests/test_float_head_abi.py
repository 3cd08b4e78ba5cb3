"""CPU-side checks of the float steps' head entries (qatvit_float_head_forward / _backward / _scratch_bytes, qatvit_float_student_head_mfma; include/qatvit.h):
the symbols in the header, the binding and the library; every form-1 refusal as a string before any HIP call; the one decision; workspaces below 128 classes."""
import ctypes
import os
import subprocess
import sys

import pytest

from qat_vit_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qatvit_float_head_forward", "qatvit_float_head_backward", "qatvit_float_head_scratch_bytes", "qatvit_float_student_head_mfma")
P = 4096   # a non-null, 16-byte aligned stand-in; never dereferenced on these paths
WS = ("qatvit_float_student_workspace_bytes", "qatvit_float_student_amp_workspace_bytes", "qatvit_float_student_bf16_workspace_bytes")
CFG = ("dict(batch=8, img_size=224, patch_size=16, in_chans=3, embed_dim=384, depth=12, num_heads=6, mlp_hidden=1536, num_classes={}, act_qmin=0, act_qmax=255, "
       "w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, ln_eps=1e-6)")


def _fwd(L, B=4, D=128, T=1, C=200, dtype=0, form=1):
    return L.qatvit_float_head_forward(P, P, P, P, P, P, P, P, P, None, B, D, T, C, dtype, form, None)


def _bwd(L, B=4, D=128, C=200, dtype=0, form=1, scratch=P, scratch_bytes=1 << 40):
    return L.qatvit_float_head_backward(P, P, P, P, P, P, scratch, scratch_bytes, B, D, C, dtype, form, None)


def test_symbols_scratch_and_the_decision(native_lib):
    L = native_lib
    hdr = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for n in NAMES:
        assert n + "(" in hdr and n in native.SIGNATURES and n in exported, n
    assert L.qatvit_abi_version() == 4                                   # added symbols: the version stays
    for shape in ((4, 128, 10), (4, 128, 127), (4, 96, 200), (4, 832, 200), (4, 128, 32769), (0, 128, 200)):
        assert L.qatvit_float_head_scratch_bytes(*shape) == 0, shape     # shapes form 1 does not cover
    n = L.qatvit_float_head_scratch_bytes(4, 128, 4099)
    assert n >= 2 * 32 * 128 * 4 and n % (32 * 128 * 4) == 0             # more than one class range of [32 rows, D] fp32 partial tiles
    cfg = lambda classes: ctypes.byref(native.Cfg(**eval(CFG.format(classes))))
    assert (L.qatvit_float_student_head_mfma(cfg(10)), L.qatvit_float_student_head_mfma(cfg(1000))) == (0, 1)


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_form_1_refusals_are_strings_without_a_gpu(native_lib, call):
    L = native_lib
    who = b"qatvit_float_head_forward" if call is _fwd else b"qatvit_float_head_backward"
    for kw, msg in (({"D": 96}, b"form 1 (MFMA) needs D % 64 == 0"), ({"D": 832}, b"D <= 768"), ({"C": 127}, b"128 <= C <= 32768"), ({"C": 32769}, b"C <= 32768"),
                    ({"form": 2}, b"form 2"), ({"dtype": 3}, b"dtype 3"), ({"B": 0}, b"all >= 1")):
        assert call(L, **kw) != 0
        assert msg in L.qatvit_last_error() and who in L.qatvit_last_error(), (kw, L.qatvit_last_error())
    need = L.qatvit_float_head_scratch_bytes(4, 128, 200)
    assert need > 0
    for kw in ({"scratch_bytes": need - 1}, {"scratch": None}):
        assert _bwd(L, **kw) != 0
        assert b"bytes of scratch" in L.qatvit_last_error(), L.qatvit_last_error()


def test_workspaces_below_128_classes_do_not_depend_on_the_knob():
    code = ("import ctypes; from qat_vit_amd import native; L = native.lib()\n"
            f"print([getattr(L, n)(ctypes.byref(native.Cfg(**{CFG.format('c')}))) for c in (10, 1000) for n in {WS!r}])")
    sizes = {}
    for knob in (None, "0"):
        env = {k: v for k, v in os.environ.items() if k != "QATVIT_FLOAT_HEAD_MFMA"}
        if knob is not None:
            env["QATVIT_FLOAT_HEAD_MFMA"] = knob
        sizes[knob] = eval(subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True, cwd=ROOT).stdout)
    assert all(n > 0 for n in sizes["0"]) and sizes[None][:3] == sizes["0"][:3]     # 10 classes: the same numbers
    assert all(a > b for a, b in zip(sizes[None][3:], sizes["0"][3:]))             # 1000 classes: the dgrad scratch at the end
