"""CPU-side checks of the head entries (qatvit_head_forward / qatvit_head_backward / qatvit_head_scratch_bytes, include/qatvit.h): the symbols in the
header, the binding and the library, and every shape refusal as a string before any HIP call - form 1 (MFMA, head_mfma.hip) states its own limits."""
import subprocess

import pytest

from qat_vit_amd import native

NAMES = ("qatvit_head_forward", "qatvit_head_backward", "qatvit_head_scratch_bytes", "qatvit_student_head_mfma")
P = 4096   # a non-null, 16-byte aligned stand-in; never dereferenced on these paths


def _fwd(L, B=4, D=128, T=1, C=200, form=1, levels=256):
    return L.qatvit_head_forward(P, P, P, P, P, P, 0, levels - 1, P, P, 0, P, P, P, P, P, B, D, T, C, form, None)


def _bwd(L, B=4, D=128, C=200, form=1, scratch=P, scratch_bytes=1 << 40):
    return L.qatvit_head_backward(P, P, P, 0, 255, P, P, P, P, P, P, P, 0, -128, 127, P, P, P, scratch, scratch_bytes, B, D, C, form, None)


def test_symbols_in_header_signatures_and_exports(native_lib):
    hdr = open(native.CSRC + "/../../include/qatvit.h").read()
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for n in NAMES:
        assert n + "(" in hdr and n in native.SIGNATURES and n in exported, n
    assert native_lib.qatvit_abi_version() == 4                      # added symbols: the version stays
    assert native_lib.qatvit_head_scratch_bytes(4, 128, 10) == 0     # form 0 needs none
    n = native_lib.qatvit_head_scratch_bytes(4, 128, 4099)
    assert n >= 2 * 32 * 128 * 4 and n % (32 * 128 * 4) == 0          # more than one class range of [32 rows, D] fp32 partial tiles


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_shape_refusals_are_strings_without_a_gpu(native_lib, call):
    L = native_lib
    who = b"qatvit_head_forward" if call is _fwd else b"qatvit_head_backward"
    for kw, msg in (({"C": 32769}, b"C <= 32768"), ({"C": 32769, "form": 0}, b"C <= 32768"), ({"D": 96}, b"form 1 (MFMA) needs D % 64 == 0"),
                    ({"C": 127}, b"128 <= C <= 32768"), ({"form": 2}, b"form 2"), ({"B": 0}, b"all >= 1")):
        assert call(L, **kw) != 0
        assert msg in L.qatvit_last_error() and who in L.qatvit_last_error(), (kw, L.qatvit_last_error())
    assert _fwd(L, levels=65536) != 0 and b"256 activation levels" in L.qatvit_last_error()
    need = L.qatvit_head_scratch_bytes(4, 128, 200)
    assert need > 0
    for kw in ({"scratch_bytes": need - 1}, {"scratch": None}):
        assert _bwd(L, **kw) != 0
        assert b"bytes of scratch" in L.qatvit_last_error(), L.qatvit_last_error()
