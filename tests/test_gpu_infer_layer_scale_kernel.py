"""The residual epilogue of the inference GEMMs on its own (``qatvit_gemm_nt_resid_fq``), without and with LayerScale gammas, on guarded operands.

The reference holds none of the new code: ``C0`` is the product as the plain entry of the same form stores it (``qatvit_gemm_nt_f16`` /
``qatvit_gemm_nt_codes``, same operands - the residual kernels stage the same values), then ``resid + fq(C0) * gamma`` in separate fp32 torch operations,
each rounded on its own: ``fq(v) = (clamp(round(v * inv) + zp, qmin, qmax) - zp) * scale``, the fake-quantize formula with the ``inv`` the kernel is given.
Every comparison is bitwise:
 (a) without gammas the entry gives ``resid + fq(C0)`` - a control of the existing epilogue (mode 6);
 (b) with gammas (mixed signs, magnitudes 0.5 .. 2, exactly 0 in column N - 1 and in one other) it gives ``resid + fq(C0) * gamma``;
 (c) with all-ones gammas it gives the bits of (a);
 (d) the guard bands around C (rows < 0 and >= M), its columns >= N where ldc > N, and ``resid`` are untouched.
Shapes: M = a sliver, 15 rows, one full 208-row tile, one row into the second, a ragged third; both N; a one-step and a six-step k-loop of the codes
kernel's two-step unroll; ldc = N and N + 8 (``resid`` shares it)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.kernel_check import guarded, guarded_copy  # noqa: E402

DEV = "cuda"
F16, CODES = 1, 3              # kNTF16, kNTCodes (csrc/qv_kernels.h)
QMIN, QMAX = 0, 255
SENTINEL = 0x7FC0BEEF          # tests/kernel_check.py, fp32


def _st():
    return torch.cuda.current_stream().cuda_stream


def split_h(x):
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi, lo


def _operands(form, M, N, K):
    """(A, A_lo or lut) of the form, the weight integers as fp16, the scalars, column scale and bias of the product."""
    if form == CODES:
        idx = (torch.randn(M, K, device=DEV).abs() * 40).clamp(0, 255).to(torch.uint8)           # skewed like GELU codes, every entry used somewhere
        idx[::5, ::3] = torch.randint(0, 256, idx[::5, ::3].shape, device=DEV, dtype=torch.uint8)
        vals = torch.randn(256, device=DEV) * 2.0 ** torch.randint(-4, 9, (256,), device=DEV).float()
        hi_t, lo_t = split_h(vals)
        a0 = idx
        a1 = ((hi_t.view(torch.int16).int() & 0xffff) | (lo_t.view(torch.int16).int() << 16)).contiguous()
    else:
        A = torch.randn(M, K, device=DEV).abs() * 3 * torch.rand(M, K, device=DEV)
        A[::7] *= -0.05
        a0, a1 = split_h(A * 2.0 ** 9)
    B = torch.randint(-128, 128, (N, K), device=DEV).float().to(torch.float16)
    s1 = torch.tensor([2.0 ** -9], device=DEV)
    s2 = torch.tensor([0.0045], device=DEV)
    cs = torch.rand(N, device=DEV) + 0.5
    bias = torch.randn(N, device=DEV)
    return a0, a1, B, s1, s2, cs, bias


def _gammas(N):
    g = (0.5 + 1.5 * torch.rand(N, device=DEV)) * torch.where(torch.rand(N, device=DEV) < 0.5, -1.0, 1.0)
    g[N - 1] = 0.0
    g[(37 * 3 + 5) % (N - 1)] = 0.0
    assert (g == 0).sum().item() == 2 and g.abs()[g != 0].min().item() >= 0.5 and g.abs().max().item() <= 2.0 and (g < 0).any() and (g > 0).any()
    return g


@pytest.mark.parametrize("pad", [0, 8], ids=["ldc=N", "ldc=N+8"])
@pytest.mark.parametrize("K", [64, 384])
@pytest.mark.parametrize("N", [384, 768])
@pytest.mark.parametrize("M", [1, 15, 208, 209, 417])
@pytest.mark.parametrize("form", [F16, CODES], ids=["f16", "codes"])
def test_residual_epilogue_with_and_without_gammas(native_lib, form, M, N, K, pad):
    L = native_lib
    torch.manual_seed(1000 * form + M + N + K + pad)
    ldc = N + pad
    a0, a1, B, s1, s2, cs, bias = _operands(form, M, N, K)
    (a0, chk_a0), (B, chk_b) = guarded_copy(a0), guarded_copy(B)
    plain = L.qatvit_gemm_nt_codes if form == CODES else L.qatvit_gemm_nt_f16

    # C0: the plain entry on the same operands (dense)
    C0, chk_c0 = guarded(M, N, torch.float32, DEV)
    assert plain(a0.data_ptr(), a1.data_ptr(), B.data_ptr(), C0.data_ptr(), M, N, K, K, K, N, s1.data_ptr(), s2.data_ptr(), cs.data_ptr(), bias.data_ptr(), None,
                 _st()) == 0, L.qatvit_last_error()
    chk_c0("plain C0")
    assert torch.isfinite(C0).all()

    # a frozen quantizer that saturates a little on both sides, with a zero point off the middle
    scale = (C0.abs().max() * 0.8 / 127).cpu().reshape(1)
    inv = torch.ones(1) / scale                               # fp32 on the host: the qparams' reciprocal, rounded once
    zp = 131.0
    qp = torch.cat([scale, inv, torch.tensor([zp, 1.0])]).to(DEV)
    scale_d, inv_d = qp[0], qp[1]
    t = torch.round(C0 * inv_d) + zp
    assert (t < QMIN).any() or (t > QMAX).any()
    fq = (t.clamp(QMIN, QMAX) - zp) * scale_d
    resid0 = torch.randn(M, ldc, device=DEV) * (3 * scale_d * 40)
    resid, chk_r = guarded_copy(resid0)
    gam = _gammas(N)
    ones = torch.ones(N, device=DEV)
    ref_a = resid0[:, :N] + fq
    ref_b = resid0[:, :N] + fq * gam                          # two torch kernels: product and sum rounded separately

    def run(gamma):
        C, chk = guarded(M, ldc, torch.float32, DEV)
        assert L.qatvit_gemm_nt_resid_fq(form, a0.data_ptr(), a1.data_ptr(), B.data_ptr(), resid.data_ptr(), C.data_ptr(), M, N, K, K, K, ldc, s1.data_ptr(),
                                         s2.data_ptr(), cs.data_ptr(), bias.data_ptr(), qp.data_ptr(), QMIN, QMAX, None if gamma is None else gamma.data_ptr(),
                                         _st()) == 0, L.qatvit_last_error()
        torch.cuda.synchronize()
        what = f"resid_fq form {form} M={M} N={N} K={K} ldc={ldc} gamma={'none' if gamma is None else 'set'}"
        chk(what)                                                                                  # (d) rows outside 0 .. M - 1
        assert (C[:, N:].contiguous().view(torch.int32) == SENTINEL).all(), what + ": columns >= N"
        assert torch.equal(resid, resid0), what + ": resid changed"
        return C[:, :N]

    out_a, out_b, out_c = run(None), run(gam), run(ones)
    chk_r("resid"), chk_a0("A"), chk_b("B")
    assert torch.equal(out_a, ref_a), ("(a) mode 6 against resid + fq(C0)", (out_a - ref_a).abs().max().item())
    assert torch.equal(out_b, ref_b), ("(b) gammas against resid + fq(C0) * gamma", (out_b - ref_b).abs().max().item())
    assert torch.equal(out_c, out_a), ("(c) all-ones gammas against mode 6", (out_c - out_a).abs().max().item())
    zero = (gam == 0).nonzero().flatten()
    assert torch.equal(out_b[:, zero], resid0[:, zero])                                            # a zero gamma leaves the residual stream as it is
    assert not torch.equal(out_b, out_a)
