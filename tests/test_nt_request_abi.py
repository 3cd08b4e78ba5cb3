"""CPU-side checks of the NT GEMM requests at the C ABI: every qatvit_gemm_nt* entry point and the two strip entry points refuse a bad request with a
non-zero return and a message, before any HIP call.  The pointers are non-null stand-ins that are never dereferenced.  Each case breaks one thing on an
otherwise supported request; every message is asserted, so a case that stopped being refused fails here and never reaches a launch."""
import pytest

import qat_vit_amd  # noqa: F401

p = 4096                      # stand-in device pointer
M, N, K = 640, 384, 384       # a supported request of the general tiles
NS = 1152                     # ... and of the strip kernels (three column tiles per workgroup)
TAIL = (None, None, None, None, None)   # s2, col_scale, bias, stats, stream


def _nt(L, M=M, N=N, K=K, lda=None, A=p):
    return L.qatvit_gemm_nt(A, p, p, p, M, N, K, lda or K, K, N, None, *TAIL)


def _nt_f16(L, M=M, N=N, K=K, lda=None, A=p):
    return L.qatvit_gemm_nt_f16(A, p, p, p, M, N, K, lda or K, K, N, None, *TAIL)


def _nt_i8(L, M=M, N=N, K=K, lda=None, wsum=p, a_qp=p):
    return L.qatvit_gemm_nt_i8(p, p, wsum, a_qp, 128, p, M, N, K, lda or K, K, N, p, *TAIL)


def _nt_i8_minmax(L, M=M, N=N, K=K, lda=None, wsum=p, a_qp=p):
    return L.qatvit_gemm_nt_i8_minmax(p, p, wsum, a_qp, 128, M, N, K, lda or K, K, p, None, None, None, p, None)


def _nt_codes(L, M=M, N=N, K=K, lda=None, lut=p):
    return L.qatvit_gemm_nt_codes(p, lut, p, p, M, N, K, lda or K, K, N, None, *TAIL)


def _nt_dy16(L, M=M, N=N, K=K, lda=None, A=p):
    return L.qatvit_gemm_nt_dy16(A, p, p, M, N, K, lda or K, K, N, p, p, None)


def _strip(L, M=M, N=NS, K=K, lda=None, wsum=p):   # the statistics pass
    return L.qatvit_i8_strip(3, p, p, wsum, p, 128, M, N, K, lda or K, p, None, None, None, p, None, 0, 255, None, None, 197, None, None, None, None)


def _strip_ln(L, M=M, N=NS, K=K, lda=None, wsum=p):
    return L.qatvit_i8_strip_ln(p, p, p, p, p, 0, 255, p, p, wsum, p, 128, M, N, K, lda or K, None, None, None, p, None)


def refused(L, rc, msg):
    assert rc != 0
    assert msg in L.qatvit_last_error(), L.qatvit_last_error()


# entry point, its refusal, a K that is no multiple of the form's k-step, an lda the form does not take (planes: elements % 8, byte forms: % 16)
ENTRIES = [(_nt, b"gemm_nt: unsupported shape", 96, 388), (_nt_f16, b"gemm_nt: unsupported shape", 96, 388),
           (_nt_i8, b"gemm_nt_i8: unsupported shape", 96, 392), (_nt_i8_minmax, b"gemm_nt_i8: unsupported shape", 96, 392),
           (_nt_codes, b"gemm_nt_codes: unsupported arguments", 96, 392), (_nt_dy16, b"gemm_nt_dy16: unsupported arguments", 48, 388),
           (_strip, b"qatvit_i8_strip: unsupported arguments", 320, 392), (_strip_ln, b"qatvit_i8_strip_ln: unsupported arguments", 320, 392)]


@pytest.mark.parametrize("call,msg,bad_k,bad_lda", ENTRIES, ids=[e[0].__name__.lstrip("_") for e in ENTRIES])
def test_entry_points_refuse_bad_shapes_without_a_gpu(native_lib, call, msg, bad_k, bad_lda):
    L = native_lib
    # an N no tile covers (the fp16 pair form names its own N rule first)
    refused(L, call(L, N=100), b"gemm_nt: the fp16 form takes N % 384 == 0" if call is _nt_f16 else msg)
    refused(L, call(L, K=bad_k), msg)
    refused(L, call(L, lda=bad_lda), msg)
    if call is not _strip:   # (qatvit_i8_strip has no check of M: an empty grid is refused by the launch, not before it)
        refused(L, call(L, M=0), msg)


NULLS = [(_nt_i8, "wsum", b"gemm_nt_i8: null pointer argument"), (_nt_i8, "a_qp", b"gemm_nt_i8: null pointer argument"),
         (_nt_i8_minmax, "wsum", b"gemm_nt_i8_minmax: null pointer argument"), (_nt_i8_minmax, "a_qp", b"gemm_nt_i8_minmax: null pointer argument"),
         (_nt_codes, "lut", b"gemm_nt_codes: null pointer argument"), (_nt_dy16, "A", b"gemm_nt_dy16: null pointer argument"),
         (_strip, "wsum", b"qatvit_i8_strip: null pointer argument"), (_strip_ln, "wsum", b"qatvit_i8_strip_ln: null pointer argument")]


@pytest.mark.parametrize("call,operand,msg", NULLS, ids=["%s-%s" % (e[0].__name__.lstrip("_"), e[1]) for e in NULLS])
def test_entry_points_refuse_a_null_required_operand(native_lib, call, operand, msg):
    refused(native_lib, call(native_lib, **{operand: None}), msg)
