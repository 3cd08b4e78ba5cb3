"""CPU-side checks of the integer forward under LayerScale: the two entry points exist and refuse a bad request with a message before any HIP call
(``qatvit_infer_forward_ls``: a null entry among the gammas; ``qatvit_gemm_nt_resid_fq``: a form without a residual epilogue, an N no tile covers, a null
``resid`` - the refusals are launch_gemm_nt's own, the wrapper adds none), and ``Int8Student`` decides on the gammas of an export on the host: the
``layer_scale`` keyword is opt-in, a partial, mis-sized or non-fp32 set is a ``ValueError``.  Pointers are non-null stand-ins that are never dereferenced."""
import ctypes

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.export import Int8Student, export_int8
from tests.util import prepare

p = 4096                       # stand-in device pointer
M, N, K = 417, 384, 384
F16, CODES = 1, 3              # kNTF16, kNTCodes (csrc/qv_kernels.h)
DEPTH = 2


def _cfg():
    return native.Cfg(batch=2, img_size=32, patch_size=16, in_chans=3, embed_dim=384, depth=DEPTH, num_heads=6, mlp_hidden=1536, num_classes=10, act_qmin=0,
                      act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, ln_eps=1e-6)


def _resid(L, form, N=N, resid=p, gamma=None):
    return L.qatvit_gemm_nt_resid_fq(form, p, p, p, resid, p, M, N, K, K, K, N, p, None, None, None, p, 0, 255, gamma, None)


def refused(L, rc, msg):
    assert rc != 0
    assert msg in L.qatvit_last_error(), L.qatvit_last_error()


def test_both_symbols_resolve(native_lib):
    for name in ("qatvit_infer_forward_ls", "qatvit_gemm_nt_resid_fq"):
        assert name in native.SIGNATURES
        assert getattr(native_lib, name) is not None


def test_infer_forward_ls_refuses_a_null_gamma_entry(native_lib):
    L = native_lib
    c = _cfg()
    tab = (ctypes.c_void_p * 64)(*([p] * 64))               # params / w8 / w_scale: more entries than any of them has
    for hole in (0, 3):
        gam = (ctypes.c_void_p * (2 * DEPTH))(*[None if k == hole else p for k in range(2 * DEPTH)])
        refused(L, L.qatvit_infer_forward_ls(ctypes.byref(c), tab, tab, tab, gam, p, p, p, None),
                b"qatvit_infer_forward_ls: ls_gamma[%d] (block %d, ls%d) is null" % (hole, hole // 2, hole % 2 + 1))
    # the shared body names the entry point that was called
    refused(L, L.qatvit_infer_forward_ls(ctypes.byref(c), tab, tab, tab, None, None, p, p, None), b"qatvit_infer_forward_ls: null argument")
    refused(L, L.qatvit_infer_forward(ctypes.byref(c), tab, tab, tab, None, p, p, None), b"qatvit_infer_forward: null argument")


@pytest.mark.parametrize("gamma", [None, p], ids=["mode6", "layer-scale"])
def test_resid_fq_refuses_other_forms(native_lib, gamma):
    L = native_lib
    mode = b"11" if gamma else b"6"
    refused(L, _resid(L, 0, gamma=gamma), b"gemm_nt: incomplete arguments for epilogue mode " + mode)          # kNTBf16: the bf16 pair form has no residual epilogue
    refused(L, _resid(L, 2, gamma=gamma), b"gemm_nt_i8: unsupported shape")                                     # kNTI8: not without its row sums and A quantizer
    refused(L, _resid(L, 4, gamma=gamma), b"gemm_nt_dy16: epilogue mode " + mode)                               # kNTPlaneF16
    refused(L, _resid(L, 5, gamma=gamma), b"gemm_nt_dy16: the bf16 form has the plain epilogue only")           # kNTPlaneBf16
    refused(L, _resid(L, 6, gamma=gamma), b"gemm_nt: no operand form 6")
    refused(L, _resid(L, -1, gamma=gamma), b"gemm_nt: no operand form -1")


@pytest.mark.parametrize("gamma", [None, p], ids=["mode6", "layer-scale"])
def test_resid_fq_refuses_bad_n_and_null_resid(native_lib, gamma):
    L = native_lib
    for n in (256, 400):
        refused(L, _resid(L, F16, N=n, gamma=gamma), b"gemm_nt: the fp16 form takes N % 384 == 0")
        refused(L, _resid(L, CODES, N=n, gamma=gamma), b"gemm_nt_codes: unsupported arguments")
    refused(L, _resid(L, F16, resid=None, gamma=gamma), b"gemm_nt: incomplete arguments for epilogue mode " + (b"11" if gamma else b"6"))
    refused(L, _resid(L, CODES, resid=None, gamma=gamma), b"gemm_nt_codes: only the residual epilogue")


@pytest.fixture(scope="module")
def ls_export():
    """The export of an untrained LayerScale student, made on the CPU (nothing in export_int8 needs a device)."""
    torch.manual_seed(0)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, init_values=0.5, embed_dim=384, depth=DEPTH, num_heads=6, img_size=32)
    return export_int8(prepare(stu, "qnnpack"))


def _variant(export, edit):
    e = dict(export)
    e["float"] = dict(export["float"])
    edit(e["float"])
    return e


def test_int8_student_default_still_refuses_an_export_with_gammas(ls_export):
    assert sum(n.endswith(".gamma") for n in ls_export["float"]) == 2 * DEPTH
    with pytest.raises(NotImplementedError, match="LayerScale"):
        Int8Student(ls_export)
    with pytest.raises(NotImplementedError, match="LayerScale"):
        Int8Student(ls_export, layer_scale=False)


def test_int8_student_refuses_partial_or_malformed_gammas_on_the_host(ls_export):
    name = "model.blocks.1.ls2.gamma"
    with pytest.raises(ValueError, match="some branches only"):
        Int8Student(_variant(ls_export, lambda f: f.pop(name)), layer_scale=True)
    with pytest.raises(ValueError, match="some branches only"):
        Int8Student(_variant(ls_export, lambda f: [f.pop(n) for n in list(f) if n.endswith(".gamma") and n != name]), layer_scale=True)
    with pytest.raises(ValueError, match="some branches only"):
        Int8Student(_variant(ls_export, lambda f: f.__setitem__("model.blocks.7.ls1.gamma", f[name])), layer_scale=True)
    with pytest.raises(ValueError, match="shape"):
        Int8Student(_variant(ls_export, lambda f: f.__setitem__(name, f[name][:383])), layer_scale=True)
    with pytest.raises(ValueError, match="shape"):
        Int8Student(_variant(ls_export, lambda f: f.__setitem__(name, f[name].reshape(1, 384))), layer_scale=True)
    with pytest.raises(ValueError, match="fp32"):
        Int8Student(_variant(ls_export, lambda f: f.__setitem__(name, f[name].double())), layer_scale=True)
    # the partial set is refused without the keyword too, as any export with gammas is
    with pytest.raises(NotImplementedError, match="LayerScale"):
        Int8Student(_variant(ls_export, lambda f: f.pop(name)))
