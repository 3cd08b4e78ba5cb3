"""CPU-side checks of the weight-gradient (TN) requests at the C ABI: every per-GEMM entry point and the stream launcher refuse a bad request with a
non-zero return and a message, before any HIP call.  The pointers are non-null stand-ins that are never dereferenced (the item array of the stream
call is real host memory: it is copied before it is checked)."""
import ctypes

import pytest

import qat_vit_amd  # noqa: F401
from qat_vit_amd import native

p = 4096                     # stand-in device pointer
M, N, Kw = 640, 256, 384     # a supported request; every case below breaks one thing
TAIL = (None, None, None, 0, -128, 127, None, None, None, 0, None)   # W, w_scale, w_zp, w_per_channel, w_qmin, w_qmax, dbias, row_div, scratch, scratch_bytes, stream
W_ONLY = (p,) + TAIL[1:]


def _tn(L, Kw, ldq, tail):
    return L.qatvit_gemm_tn(p, p, p, None, p, M, N, Kw, N, ldq, Kw, None, *tail)


def _tn_codes(L, Kw, ldq, tail):
    return L.qatvit_gemm_tn_codes(p, p, p, p, p, M, N, Kw, N, ldq, Kw, None, *tail)


def _tn_dy16_plane(L, Kw, ldq, tail):
    return L.qatvit_gemm_tn_dy16(p, p, None, None, None, p, M, N, Kw, N, ldq, Kw, p, p, *tail)


def _tn_dy16_codes(L, Kw, ldq, tail):
    return L.qatvit_gemm_tn_dy16(p, None, None, p, p, p, M, N, Kw, N, ldq, Kw, p, p, *tail)


def _tn_q8(L, Kw, ldq, tail):
    return L.qatvit_gemm_tn_q8_dy16(p, p, p, 128, p, M, N, Kw, N, ldq, Kw, p, *tail)


# entry point, its shape message, an ldq its operand form does not take (planes: elements % 8, bytes: % 16)
ENTRIES = [(_tn, b"gemm_tn: unsupported shape", 388), (_tn_codes, b"gemm_tn_codes: unsupported arguments", 392),
           (_tn_dy16_plane, b"gemm_tn: unsupported shape", 388), (_tn_dy16_codes, b"gemm_tn_codes: unsupported arguments", 392),
           (_tn_q8, b"gemm_tn_q8: unsupported arguments", 392)]


@pytest.mark.parametrize("call,shape_msg,bad_ldq", ENTRIES, ids=[e[0].__name__.lstrip("_") for e in ENTRIES])
def test_per_gemm_entry_points_refuse_bad_requests_without_a_gpu(native_lib, call, shape_msg, bad_ldq):
    L = native_lib
    assert call(L, 100, 100, TAIL) != 0          # a Kw no tile covers
    assert shape_msg in L.qatvit_last_error(), L.qatvit_last_error()
    assert call(L, Kw, bad_ldq, TAIL) != 0       # a misaligned Q row
    assert shape_msg in L.qatvit_last_error(), L.qatvit_last_error()
    assert call(L, Kw, Kw, W_ONLY) != 0          # a weight mask without its qparams
    assert b"weight mask needs w_scale and w_zp" in L.qatvit_last_error(), L.qatvit_last_error()


def test_tn_dy16_refuses_planes_together_with_codes(native_lib):
    L = native_lib
    assert L.qatvit_gemm_tn_dy16(p, p, None, p, p, p, M, N, Kw, N, Kw, Kw, p, p, *TAIL) != 0
    assert b"qatvit_gemm_tn_dy16: Q is either planes" in L.qatvit_last_error(), L.qatvit_last_error()


def test_tn_stream_refuses_no_items_and_an_unknown_mode(native_lib):
    L = native_lib
    items = (native.TNItem * 1)()
    it = items[0]
    it.P = it.Q = it.lut = it.s1 = it.s2 = it.C = p
    it.N, it.Kw, it.ldp, it.ldq, it.ldc = N, Kw, N, Kw, Kw
    ip = ctypes.cast(items, ctypes.c_void_p)
    assert L.qatvit_gemm_tn_stream_dy16(0, ip, 0, M, 128, 0, -128, 127, p, 1 << 30, None) != 0
    assert b"qatvit_gemm_tn_stream_dy16: null / empty argument" in L.qatvit_last_error(), L.qatvit_last_error()
    assert L.qatvit_gemm_tn_stream_dy16(3, ip, 1, M, 128, 0, -128, 127, p, 1 << 30, None) != 0
    assert b"tn_stream: bad arguments (n=1, mode=3)" in L.qatvit_last_error(), L.qatvit_last_error()
