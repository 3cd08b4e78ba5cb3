"""Every exported kernel launcher at its smallest edge shapes, with every operand and output inside guarded padding (tests/kernel_check.py): an input's
padding is poison (NaN / 0x80 / 0xFF in the rows before and past the extent), an output's is a canary.  Each result is compared with the fp64
reference of the launcher's existing test, at that test's tolerance, over the whole tensor AND per 16 x 16 tile; pairs that must be bit-identical
keep torch.equal.  Shapes: one row, one row less than / exactly / one row more than the row tile of the form (128-row tiles, 208-row tall tiles
and strips), the 64-token reduction step of the weight gradients and their first two-split size, the attention key-tile forms exactly full and
one past.  Measured values: profiles/kernel_tile_errors.txt."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from qat_vit_amd import native  # noqa: E402
from tests.kernel_check import assert_tiles_close, guarded, guarded_copy, ord2f, rel_l2_t, tile_errors  # noqa: E402
from tests.test_gpu_attn import _emulate as attn_emulate  # noqa: E402
from tests.test_gpu_attn import _ref as attn_ref  # noqa: E402
from tests.test_gpu_gemm import _unpack_bits, split, split_h  # noqa: E402

DEV = "cuda"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class Guards:
    """Collects the checks of one test's guarded operands."""

    def __init__(self):
        self.checks = []

    def inp(self, x):
        if x is None:
            return None
        t, c = guarded_copy(x)
        self.checks.append(c)
        return t

    def out(self, rows, cols, dtype, fill=None, pad=224):
        t, c = guarded(rows, cols, dtype, DEV, pad=pad, fill=fill)
        self.checks.append(c)
        return t

    def inps(self, *xs):
        return tuple(self.inp(x) for x in xs)

    def check(self, what):
        torch.cuda.synchronize()
        for c in self.checks:
            c(what)


def _fresh_stats(g):
    """The caller-initialised {min, max} accumulator, guarded like every other operand."""
    return g.inp(torch.tensor([0xFF800000 - (1 << 32), 0x007FFFFF], dtype=torch.int32, device=DEV))


def _report(what, got, ref, tol, tile=(16, 16), emu=None):
    """Both bounds: whole tensor and per tile (assert_tiles_close prints the figures).  emu: a stock-torch emulation of the kernel (the operand planes as
    given, fp32 accumulation) where a correct kernel's worst tile is known to come out above half of tol: the tile bound is then twice the emulation's
    worst tile against the same reference - it shares every rounding with the kernel and differs in summation order only."""
    whole = rel_l2_t(got, ref)
    tile_tol = tol
    if emu is not None:
        e_worst = tile_errors(emu.to(ref.device), ref, tile)[1]
        tile_tol = 2 * e_worst
        print(f"EMU {what}: emulation worst_tile {e_worst:.3e}")
    assert_tiles_close(got, ref, tile_tol, tile, what)
    assert whole < tol, (what, whole)


# ---------------------------------------------------------------------------------------------------------------- NT
NT_SHAPES = [(M, 128, K) for K in (64, 384) for M in (1, 127, 128, 129)] + [(M, 384, K) for K in (64, 384) for M in (1, 207, 208, 209, 417)]


@pytest.mark.parametrize("a_f32", [0, 1], ids=["gridA", "splitA"])
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_edges(native_lib, M, N, K, a_f32):
    """qatvit_gemm_nt on the 128 x 128 tile (N = 128) and the 208 x 384 tall tile (N = 384), with and without col_scale / bias / stats: the fp64
    reference and tolerance of test_gemm_nt; stats = the min / max over the valid rows only."""
    torch.manual_seed(M + N + K + a_f32)
    g = Guards()
    B = torch.randint(-128, 128, (N, K), device=DEV).float()
    Bh = g.inp(B.to(torch.bfloat16))
    if a_f32:
        A = torch.randn(M, K, device=DEV) * 3
        Ah, Al = (g.inp(x) for x in split(A))
    else:
        A = torch.randint(-255, 256, (M, K), device=DEV).float()
        Ah, Al = g.inp(A.to(torch.bfloat16)), None
    s1, s2, cs, bias = g.inps(torch.tensor([0.0123], device=DEV), torch.tensor([0.0045], device=DEV), torch.rand(N, device=DEV) + 0.5, torch.randn(N, device=DEV))
    for extras in (True, False):
        stats = _fresh_stats(g) if extras else None
        C = g.out(M, N, torch.float32)
        st = native_lib.qatvit_gemm_nt(Ah.data_ptr(), _ptr(Al), Bh.data_ptr(), C.data_ptr(), M, N, K, K, K, N, s1.data_ptr(), s2.data_ptr(),
                                       cs.data_ptr() if extras else None, bias.data_ptr() if extras else None, _ptr(stats), _st())
        assert st == 0, native_lib.qatvit_last_error()
        g.check(f"gemm_nt M={M} N={N} K={K}")
        ref = (A.double() @ B.double().t()) * (s1.double() * s2.double())
        if extras:
            ref = ref * cs.double() + bias.double()
        assert not torch.isnan(C).any()
        _report(f"gemm_nt[{M}-{N}-{K}-{'splitA' if a_f32 else 'gridA'}-{'extras' if extras else 'plain'}]", C, ref, 2e-5)
        if extras:
            assert ord2f(stats[0]) == C.min().item() and ord2f(stats[1]) == C.max().item()


F16_SHAPES = [(M, 384, K) for K in (64, 384) for M in (1, 208, 209)]     # (the launcher shares qatvit_gemm_nt's K % 64 == 0 check: K = 32 is refused)
DY16_SHAPES = [(M, 384, K) for K in (32, 64, 384) for M in (1, 208, 209)] + [(209, 384, 96)]      # 96: one 64-wide k-step and a 32-wide rest


@pytest.mark.parametrize("M,N,K", F16_SHAPES)
def test_gemm_nt_f16_and_codes_edges(native_lib, M, N, K):
    """qatvit_gemm_nt_f16 against fp64 on the original operand (1e-6, as test_gemm_nt_f16_pair) and, where K % 64 == 0, qatvit_gemm_nt_codes on the
    same operand as codes + table: the same bits, incl. the statistics."""
    torch.manual_seed(M + N + K)
    g = Guards()
    idx = (torch.randn(M, K, device=DEV).abs() * 40).clamp(0, 255).to(torch.uint8)
    idx[::5, ::3] = torch.randint(0, 256, idx[::5, ::3].shape, device=DEV, dtype=torch.uint8)
    vals = torch.randn(256, device=DEV).abs() * 3 * torch.rand(256, device=DEV)        # the operand of test_gemm_nt_f16_pair, on a 256-entry table
    vals[::7] *= -0.05
    pre = 2.0 ** 9
    hi_t, lo_t = split_h(vals * pre)
    lut = g.inp((hi_t.view(torch.int16).int() & 0xffff) | (lo_t.view(torch.int16).int() << 16))
    A = vals[idx.long()]
    Ah, Al = g.inp(hi_t[idx.long()]), g.inp(lo_t[idx.long()])
    Bi = torch.randint(-128, 128, (N, K), device=DEV).float()
    Bh = g.inp(Bi.to(torch.float16))
    s1, s2, cs, bias = g.inps(torch.tensor([0.0123 / pre], device=DEV), torch.tensor([0.0045], device=DEV), torch.rand(N, device=DEV) + 0.5, torch.randn(N, device=DEV))
    st_a, st_b = _fresh_stats(g), _fresh_stats(g)
    Ca = g.out(M, N, torch.float32)
    assert native_lib.qatvit_gemm_nt_f16(Ah.data_ptr(), Al.data_ptr(), Bh.data_ptr(), Ca.data_ptr(), M, N, K, K, K, N, s1.data_ptr(), s2.data_ptr(),
                                         cs.data_ptr(), bias.data_ptr(), st_a.data_ptr(), _st()) == 0, native_lib.qatvit_last_error()
    g.check(f"gemm_nt_f16 M={M} K={K}")
    ref = (A.double() @ Bi.double().t()) * (0.0123 * 0.0045) * cs.double() + bias.double()
    assert not torch.isnan(Ca).any()
    _report(f"gemm_nt_f16[{M}-{N}-{K}]", Ca, ref, 1e-6)
    assert ord2f(st_a[0]) == Ca.min().item() and ord2f(st_a[1]) == Ca.max().item()
    if K % 64 == 0:
        A8 = g.inp(idx)
        Cb = g.out(M, N, torch.float32)
        assert native_lib.qatvit_gemm_nt_codes(A8.data_ptr(), lut.data_ptr(), Bh.data_ptr(), Cb.data_ptr(), M, N, K, K, K, N, s1.data_ptr(), s2.data_ptr(),
                                               cs.data_ptr(), bias.data_ptr(), st_b.data_ptr(), _st()) == 0, native_lib.qatvit_last_error()
        g.check(f"gemm_nt_codes M={M} K={K}")
        assert torch.equal(Ca, Cb) and torch.equal(st_a, st_b)


@pytest.mark.parametrize("M,N,K", [(M, 384, K) for K in (64, 384) for M in (1, 208, 209)])
def test_gemm_nt_i8_edges(native_lib, M, N, K):
    """qatvit_gemm_nt_i8 == qatvit_gemm_nt on the bf16 integers, bit for bit (test_gemm_nt_i8_equals_bf16_path), and both against fp64 at 1e-6."""
    torch.manual_seed(M + N + K)
    g = Guards()
    zp, center = 131, 128
    q = torch.randint(0, 256, (M, K), device=DEV)
    W = torch.randint(-128, 128, (N, K), device=DEV)
    A16, B16 = g.inp((q - zp).to(torch.bfloat16)), g.inp(W.to(torch.bfloat16))
    A8, B8 = g.inp((q - center).to(torch.int8)), g.inp(W.to(torch.int8))
    wsum, aqp = g.inps(W.sum(1).to(torch.int32), torch.tensor([0.0173, 1 / 0.0173, float(zp), 1.0], device=DEV))
    s1, s2, bias = g.inps(torch.tensor([0.0173], device=DEV), torch.tensor([0.0041], device=DEV), torch.randn(N, device=DEV))
    C16, C8 = g.out(M, N, torch.float32), g.out(M, N, torch.float32)
    st16, st8 = _fresh_stats(g), _fresh_stats(g)
    assert native_lib.qatvit_gemm_nt(A16.data_ptr(), None, B16.data_ptr(), C16.data_ptr(), M, N, K, K, K, N, s1.data_ptr(), s2.data_ptr(), None,
                                     bias.data_ptr(), st16.data_ptr(), _st()) == 0, native_lib.qatvit_last_error()
    assert native_lib.qatvit_gemm_nt_i8(A8.data_ptr(), B8.data_ptr(), wsum.data_ptr(), aqp.data_ptr(), center, C8.data_ptr(), M, N, K, K, K, N,
                                        s1.data_ptr(), s2.data_ptr(), None, bias.data_ptr(), st8.data_ptr(), _st()) == 0, native_lib.qatvit_last_error()
    g.check(f"gemm_nt_i8 M={M} K={K}")
    assert torch.equal(C8, C16) and torch.equal(st8, st16)
    assert ord2f(st8[0]) == C8.min().item() and ord2f(st8[1]) == C8.max().item()
    ref = ((q - zp).double() @ W.double().t()) * (0.0173 * 0.0041) + bias.double()
    _report(f"gemm_nt_i8[{M}-{N}-{K}]", C8, ref, 1e-6)


@pytest.mark.parametrize("M,N,K", DY16_SHAPES)
def test_gemm_nt_dy16_edges(native_lib, M, N, K):
    """qatvit_gemm_nt_dy16 against fp64 on the rounded plane (2e-5, as test_dgrad_one_plane_vs_fp64)."""
    gen = torch.Generator(device=DEV).manual_seed(M + N + K)
    g = Guards()
    dy = torch.randn(M, K, generator=gen, device=DEV) * 3e-6 * torch.exp(torch.randn(M, K, generator=gen, device=DEV))
    wt = torch.randint(-127, 128, (N, K), generator=gen, device=DEV).float()
    e = 8 - int(np.floor(np.log2(dy.abs().max().item())) + 1)
    plane = (dy * 2.0 ** e).to(torch.float16)
    P16, W16 = g.inp(plane), g.inp(wt.to(torch.float16))
    C = g.out(M, N, torch.float32)
    s1, s2 = g.inps(torch.tensor([0.0123], device=DEV), torch.tensor([2.0 ** -e], device=DEV))
    assert native_lib.qatvit_gemm_nt_dy16(P16.data_ptr(), W16.data_ptr(), C.data_ptr(), M, N, K, K, K, N, s1.data_ptr(), s2.data_ptr(), _st()) == 0, \
        native_lib.qatvit_last_error()
    g.check(f"gemm_nt_dy16 M={M} K={K}")
    _report(f"gemm_nt_dy16[{M}-{N}-{K}]", C, (plane.double() @ wt.double().T) * (0.0123 * 2.0 ** -e), 2e-5)


# ---------------------------------------------------------------------------------------------------------------- int8 strip
def _strip_tm():
    """The strip height in 16-row fragments that i8strip.hip instantiates for K = 384, N = 1152: strip_launch_shape launches strip_launch<MODE, 3> there, with
    the template's default TM - read from the source, so a changed instantiation moves the edge shapes with it (or fails here)."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(native.__file__), "csrc", "i8strip.hip")).read()
    m = re.search(r"template <int MODE, int NTL, int TM = (\d+), int KT = \d+>\s*static void strip_launch\(", src)
    assert m and "else strip_launch<MODE, 3>(a, st);" in src, "i8strip.hip: the K = 384 instantiation is no longer strip_launch<MODE, 3> with the default TM"
    return int(m.group(1))


STRIP_TM = _strip_tm()      # 13: 208-row strips


@pytest.mark.parametrize("per_channel", [0, 1])
@pytest.mark.parametrize("qrange", [(0, 255), (0, 127)])
@pytest.mark.parametrize("M", [1, 16 * STRIP_TM - 1, 16 * STRIP_TM, 16 * STRIP_TM + 1])
def test_i8_strip_edges(native_lib, M, per_channel, qrange):
    """qatvit_i8_strip (K = 384, N = 1152) against qatvit_gemm_nt_i8 as test_i8_strip_kernel_equals_general_kernel does it - statistics (mode 3),
    row-major codes + mask bits (mode 4), attention-layout codes + mask bits (mode 7): torch.equal throughout."""
    N, K, B, T = 1152, 384, 1, M
    torch.manual_seed(M + N + per_channel + qrange[1])
    g = Guards()
    zp, center = 131, 128
    q = torch.randint(0, 256, (M, K), device=DEV)
    W = torch.randint(-128, 128, (N, K), device=DEV)
    A8 = g.inp((q - center).to(torch.int8))
    B8 = g.inp(W.to(torch.int8))
    B8f = g.out(N, K, torch.int8)
    assert native_lib.qatvit_w8_fragment_order(B8.data_ptr(), B8f.data_ptr(), N, K, _st()) == 0, native_lib.qatvit_last_error()
    wsum, aqp = g.inps(W.sum(1).to(torch.int32), torch.tensor([0.0173, 1 / 0.0173, float(zp), 1.0], device=DEV))
    s1, s2, bias = g.inps(torch.tensor([0.0173], device=DEV), torch.tensor([0.0041], device=DEV), torch.randn(N, device=DEV))
    cs = g.inp(torch.rand(N, device=DEV) * 0.01 + 0.001) if per_channel else None
    s2p, csp = (None, cs.data_ptr()) if per_channel else (s2.data_ptr(), None)
    C = g.out(M, N, torch.float32)
    st_full, st_gen, st_strip = _fresh_stats(g), _fresh_stats(g), _fresh_stats(g)
    assert native_lib.qatvit_gemm_nt_i8(A8.data_ptr(), B8.data_ptr(), wsum.data_ptr(), aqp.data_ptr(), center, C.data_ptr(), M, N, K, K, K, N, s1.data_ptr(),
                                        s2p, csp, bias.data_ptr(), st_full.data_ptr(), _st()) == 0, native_lib.qatvit_last_error()
    assert native_lib.qatvit_gemm_nt_i8_minmax(A8.data_ptr(), B8.data_ptr(), wsum.data_ptr(), aqp.data_ptr(), center, M, N, K, K, K, s1.data_ptr(), s2p, csp,
                                               bias.data_ptr(), st_gen.data_ptr(), _st()) == 0, native_lib.qatvit_last_error()

    def strip(mode, stats=None, qp=None, out8=None, mask=None, code_T=0, lut=None, lutq=None, sc=None):
        assert native_lib.qatvit_i8_strip(mode, A8.data_ptr(), B8f.data_ptr(), wsum.data_ptr(), aqp.data_ptr(), center, M, N, K, K, s1.data_ptr(), s2p, csp,
                                          bias.data_ptr(), _ptr(stats), _ptr(qp), qrange[0], qrange[1], _ptr(out8), _ptr(mask), code_T, _ptr(lut), _ptr(lutq),
                                          _ptr(sc), _st()) == 0, native_lib.qatvit_last_error()

    strip(3, stats=st_strip)
    g.check(f"i8 statistics M={M}")
    assert not torch.isnan(C).any()
    assert torch.equal(st_gen, st_full) and torch.equal(st_strip, st_full)
    assert ord2f(st_strip[0]) == C.min().item() and ord2f(st_strip[1]) == C.max().item()

    lo, hi = torch.quantile(C.flatten(), torch.tensor([0.1, 0.9], device=DEV)).tolist()
    scale = torch.tensor([(hi - lo) / (qrange[1] - qrange[0])], device=DEV, dtype=torch.float32)
    inv = torch.ones(1, device=DEV) / scale
    zpo = float(round(qrange[0] - lo / scale.item()))
    qp = g.inp(torch.cat([scale, inv, torch.tensor([zpo, 1.0], device=DEV)]))
    t = torch.round(C * inv) + zpo
    tc = t.clamp(qrange[0], qrange[1])
    want_code = (tc - qrange[0]).to(torch.uint8)
    want_mask = t == tc
    assert 0.02 < (~want_mask).float().mean().item() < 0.5

    out8 = g.out(M, N, torch.uint8)
    mask = g.out(M, N // 8, torch.uint8)
    lut, lutq, sc = g.inps(torch.zeros(256, dtype=torch.int32, device=DEV), torch.zeros(256, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV))
    strip(4, qp=qp, out8=out8, mask=mask, lut=lut, lutq=lutq, sc=sc)
    g.check(f"i8 strip mode 4 M={M}")
    assert torch.equal(out8, want_code)
    assert torch.equal(_unpack_bits(mask, M * N).view(M, N), want_mask)

    D, H = N // 3, N // 3 // 64
    out8 = g.out(B * H * 3 * T, 64, torch.uint8)
    mask = g.out(B * H * 3 * T, 8, torch.uint8)
    strip(7, qp=qp, out8=out8, mask=mask, code_T=T)
    g.check(f"i8 strip mode 7 M={M}")
    want = want_code.view(B, T, 3, H, 64).permute(0, 3, 2, 1, 4).contiguous()
    assert torch.equal(out8.view(B, H, 3, T, 64), want)
    wm = want_mask.view(B, T, 3, H, 64).permute(0, 3, 2, 1, 4).contiguous()
    assert torch.equal(_unpack_bits(mask, M * N).view(B, H, 3, T, 64), wm)


# ---------------------------------------------------------------------------------------------------------------- TN
def _two_splits(bk):
    """gemm.hip tn_plan: splits = min(256 / tiles, steps / (256 / bk)) with steps = ceil(M / bk) - the smallest M with two splits."""
    return (2 * (256 // bk) - 1) * bk + 1


TN_M = [1, 63, 64, 65, _two_splits(64), _two_splits(32)]        # 449 (64-token steps), 481 (32-token steps)


def _ste_mask(W, w_scale):
    qv = torch.round(W * (torch.ones(1, device=DEV) / w_scale))
    return ((qv >= -128) & (qv <= 127)).double()


def _tn_check(what, C, db, ref, dbref, tol=2e-5, emu=(None, None)):
    _report(what, C, ref, tol, emu=emu[0])
    _report(what + "-dbias", db[None, :], dbref[None, :], tol, tile=(1, 1), emu=None if emu[1] is None else emu[1][None, :])


@pytest.mark.parametrize("two_phase", [0, 1])
@pytest.mark.parametrize("form", ["grid", "pair", "codes"])
@pytest.mark.parametrize("M", TN_M)
def test_gemm_tn_edges(native_lib, M, form, two_phase):
    """qatvit_gemm_tn (Q on the grid / as a pair, N = Kw = 128) and qatvit_gemm_tn_codes (Kw = 384), M around the 64-token step: the token tail IS the
    reduction tail.  The reference and tolerance of test_gemm_tn; dbias per element.
    M = 1: nothing averages the operands' own (hi, lo) rounding (2^-18 per element) - measured, the worst tile and the worst dbias element of a correct
    kernel are 1.2e-5 .. 1.6e-5, above half of 2e-5 - so the tile bound there is twice the worst tile of the CPU emulation (see _report); the whole-tensor
    bound stays 2e-5."""
    N, Kw = 128, (384 if form == "codes" else 128)
    torch.manual_seed(M + N + Kw + len(form))
    g = Guards()
    P = torch.randn(M, N, device=DEV) * 1e-3
    Ph, Pl = (g.inp(x) for x in split(P))
    Qh = Ql = Qc = lut = None
    if form == "grid":
        Q = torch.randint(-255, 256, (M, Kw), device=DEV).float()
        Qh = g.inp(Q.to(torch.bfloat16))
        planes_q = (Qh.float().cpu(), None)
    elif form == "pair":
        Q = torch.randn(M, Kw, device=DEV)
        Qh, Ql = (g.inp(x) for x in split(Q))
        planes_q = (Qh.float().cpu(), Ql.float().cpu())
    else:
        idx = torch.randint(0, 256, (M, Kw), device=DEV, dtype=torch.uint8)
        vals = torch.randn(256, device=DEV) * 2.0 ** torch.randint(-6, 3, (256,), device=DEV).float()
        th, tl = split(vals)
        lut = g.inp((th.view(torch.int16).int() & 0xffff) | (tl.view(torch.int16).int() << 16))
        Q = (th.double() + tl.double())[idx.long()]
        Qc = g.inp(idx)
        planes_q = (th.float()[idx.long()].cpu(), tl.float()[idx.long()].cpu())
    W, s1, w_scale, w_zp = g.inps(torch.randn(N, Kw, device=DEV), torch.tensor([0.031], device=DEV), torch.tensor([2.0 / 127], device=DEV),
                                  torch.zeros(1, dtype=torch.int32, device=DEV))
    C = g.out(N, Kw, torch.float32, fill=0.0)
    db = g.out(1, N, torch.float32, fill=0.0)
    nb = native_lib.qatvit_gemm_tn_scratch_bytes()
    scratch = torch.empty(nb if two_phase else 16, dtype=torch.uint8, device=DEV)
    sp, sn = (scratch.data_ptr(), nb) if two_phase else (None, 0)
    if form == "codes":
        st = native_lib.qatvit_gemm_tn_codes(Ph.data_ptr(), Pl.data_ptr(), Qc.data_ptr(), lut.data_ptr(), C.data_ptr(), M, N, Kw, N, Kw, Kw, s1.data_ptr(),
                                             W.data_ptr(), w_scale.data_ptr(), w_zp.data_ptr(), 0, -128, 127, db.data_ptr(), None, sp, sn, _st())
    else:
        st = native_lib.qatvit_gemm_tn(Ph.data_ptr(), Pl.data_ptr(), Qh.data_ptr(), _ptr(Ql), C.data_ptr(), M, N, Kw, N, Kw, Kw, s1.data_ptr(),
                                       W.data_ptr(), w_scale.data_ptr(), w_zp.data_ptr(), 0, -128, 127, db.data_ptr(), None, sp, sn, _st())
    assert st == 0, native_lib.qatvit_last_error()
    g.check(f"gemm_tn {form} M={M}")
    mask = _ste_mask(W, w_scale)
    assert 0.01 < 1 - mask.mean().item() < 0.2
    ref = (P.double().t() @ Q.double()) * s1.double() * mask
    emu = (None, None)
    if M == 1:
        ph, pl, (qh, ql) = Ph.float().cpu(), Pl.float().cpu(), planes_q
        acc = ph.t() @ qh + pl.t() @ qh + (ph.t() @ ql if ql is not None else 0.0)
        emu = (acc * s1.cpu() * mask.float().cpu(), (ph + pl).sum(0))
    _tn_check(f"gemm_tn[{M}-{form}-{two_phase}]", C, db[0], ref, P.double().sum(0), emu=emu)


@pytest.mark.parametrize("two_phase", [0, 1])
@pytest.mark.parametrize("kind", ["grid", "pair", "codes", "q8"])
@pytest.mark.parametrize("M", TN_M)
def test_gemm_tn_dy16_edges(native_lib, M, kind, two_phase):
    """qatvit_gemm_tn_dy16 (grid and pair at Kw = 128, codes at Kw = 384) and qatvit_gemm_tn_q8_dy16 (Kw = 384): fp64 on the rounded plane, 2e-5, as
    test_wgrad_one_plane_vs_fp64 / test_wgrad_one_plane_byte_grid_vs_fp64."""
    N, Kw = 128, (384 if kind in ("codes", "q8") else 128)
    gen = torch.Generator(device=DEV).manual_seed(N + Kw + M + len(kind))
    g = Guards()
    dy = torch.randn(M, N, generator=gen, device=DEV) * 2e-6 * torch.exp(torch.randn(M, N, generator=gen, device=DEV))
    e = 8 - int(np.floor(np.log2(dy.abs().max().item())) + 1)
    plane = (dy * 2.0 ** e).to(torch.float16)
    P16 = g.inp(plane)
    sx, center, zp = 0.0371, 128, 131
    qh = ql = qc = lut = q8 = None
    if kind == "grid":
        xv = torch.randint(-255, 256, (M, Kw), generator=gen, device=DEV).float()
        qh = g.inp(xv.to(torch.float16))
    elif kind == "pair":
        xv = torch.randn(M, Kw, generator=gen, device=DEV) * 300.0
        h = xv.to(torch.float16)
        lo = (xv - h.float()).to(torch.float16)
        xv = h.float() + lo.float()
        qh, ql = g.inp(h), g.inp(lo)
    elif kind == "codes":
        tab = torch.randn(256, generator=gen, device=DEV) * 400.0
        th = tab.to(torch.float16)
        tl = (tab - th.float()).to(torch.float16)
        lut = g.inp(((th.view(torch.int16).int() & 0xffff) | (tl.view(torch.int16).int() << 16)).contiguous())
        idx = torch.randint(0, 256, (M, Kw), generator=gen, device=DEV).to(torch.uint8)
        xv = th.float()[idx.long()]
        qc = g.inp(idx)
    else:
        q = torch.randint(0, 256, (M, Kw), generator=gen, device=DEV)
        q8 = g.inp((q - center).to(torch.int8))
        xv = (q - zp).float()
    W, w_scale, w_zp = g.inps(torch.randn(N, Kw, generator=gen, device=DEV), torch.tensor([2.0 / 127], device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    dW = g.out(N, Kw, torch.float32, fill=0.0)
    db = g.out(1, N, torch.float32, fill=0.0)
    scratch = torch.empty(native_lib.qatvit_gemm_tn_scratch_bytes() if two_phase else 16, dtype=torch.uint8, device=DEV)
    sp, sn = (scratch.data_ptr(), scratch.numel()) if two_phase else (None, 0)
    s1, s2, a_qp = g.inps(torch.tensor([sx], device=DEV), torch.tensor([2.0 ** -e], device=DEV),
                          torch.tensor([sx, 1.0 / sx, float(zp), 1.0], dtype=torch.float32, device=DEV))
    tail = (W.data_ptr(), w_scale.data_ptr(), w_zp.data_ptr(), 0, -128, 127, db.data_ptr(), None, sp, sn, _st())
    if kind == "q8":
        rc = native_lib.qatvit_gemm_tn_q8_dy16(P16.data_ptr(), q8.data_ptr(), a_qp.data_ptr(), center, dW.data_ptr(), M, N, Kw, N, Kw, Kw, s2.data_ptr(), *tail)
    else:
        rc = native_lib.qatvit_gemm_tn_dy16(P16.data_ptr(), _ptr(qh), _ptr(ql), _ptr(qc), _ptr(lut), dW.data_ptr(), M, N, Kw, N, Kw, Kw, s1.data_ptr(), s2.data_ptr(), *tail)
    assert rc == 0, native_lib.qatvit_last_error()
    g.check(f"gemm_tn_dy16 {kind} M={M}")
    ref = (plane.double().T @ xv.double()) * (sx * 2.0 ** -e) * _ste_mask(W, w_scale)
    _tn_check(f"gemm_tn_dy16[{M}-{kind}-{two_phase}]", dW, db[0], ref, plane.double().sum(0) * 2.0 ** -e)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_tn_stream_edges(native_lib, mode):
    """qatvit_gemm_tn_stream_dy16: one batch of three items over M = 65 token rows (one full 64-token step and a one-row tail), every X form, guards
    around every item's operands and its C: each item against fp64 on the rounded plane as test_wgrad_stream_batch_vs_fp64 (3e-5; dbias 2e-5)."""
    M, shapes = 65, [(128, 384), (256, 384), (128, 768)]
    gen = torch.Generator(device=DEV).manual_seed(100 * mode + M)
    g = Guards()
    items = (native.TNItem * len(shapes))()
    keep, refs = [], []
    center, zp = 128, 131.0
    for k, (N, Kw) in enumerate(shapes):
        dy = torch.randn(M, N, generator=gen, device=DEV) * 2e-6 * torch.exp(torch.randn(M, N, generator=gen, device=DEV))
        e = 8 - int(np.floor(np.log2(dy.abs().max().item())) + 1)
        plane = (dy * 2.0 ** e).to(torch.float16)
        sx = 0.02 + 0.01 * k
        lut = None
        if mode == 0:
            q = torch.randint(0, 256, (M, Kw), generator=gen, device=DEV)
            Q = (q - center).to(torch.int8)
            xv = (q - zp).double()
            s1 = torch.tensor([sx, 1.0 / sx, zp, 1.0], dtype=torch.float32, device=DEV)
        elif mode == 1:
            tab = (torch.randn(256, generator=gen, device=DEV) * 400.0).to(torch.float16)
            lut = g.inp((tab.view(torch.int16).int() & 0xffff).contiguous())
            Q = torch.randint(0, 256, (M, Kw), generator=gen, device=DEV).to(torch.uint8)
            xv = tab.double()[Q.long()]
            s1 = torch.tensor([sx], device=DEV)
        else:
            Q = (torch.randn(M, Kw, generator=gen, device=DEV) * 300.0).to(torch.float16)
            xv = Q.double()
            s1 = torch.tensor([sx], device=DEV)
        s1, s2 = g.inps(s1, torch.tensor([2.0 ** -e], device=DEV))
        Pg, Qg = g.inp(plane), g.inp(Q)
        W, wsc, wzp = g.inps(torch.randn(N, Kw, generator=gen, device=DEV), torch.full((N,), 0.01, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV))
        C = g.out(N, Kw, torch.float32, fill=0.0)
        db = g.out(1, N, torch.float32, fill=0.0)
        it = items[k]
        it.P, it.Q, it.lut, it.s1, it.s2, it.C = Pg.data_ptr(), Qg.data_ptr(), _ptr(lut), s1.data_ptr(), s2.data_ptr(), C.data_ptr()
        it.W, it.w_scale, it.w_zp, it.dbias, it.row_div = W.data_ptr(), wsc.data_ptr(), wzp.data_ptr(), db.data_ptr(), None
        it.N, it.Kw, it.ldp, it.ldq, it.ldc = N, Kw, N, Kw, Kw
        qq = torch.round(W * (1.0 / wsc)[:, None])
        ref = (plane.double().T @ xv) * (sx * 2.0 ** -e)
        ref = torch.where((qq >= -128) & (qq <= 127), ref, torch.zeros_like(ref))
        keep.append((Pg, Qg, lut, s1, s2, W, wsc, wzp, C, db))
        refs.append((ref, plane.double().sum(0) * 2.0 ** -e))
    scratch = torch.empty(native_lib.qatvit_gemm_tn_stream_scratch_bytes(), dtype=torch.uint8, device=DEV)
    native.check(native_lib.qatvit_gemm_tn_stream_dy16(mode, ctypes.cast(items, ctypes.c_void_p), len(shapes), M, center, 1, -128, 127, scratch.data_ptr(),
                                                       scratch.numel(), ctypes.c_void_p(_st())), "tn_stream_dy16")
    g.check(f"tn_stream mode {mode}")
    for k, ((*_, C, db), (ref, bref)) in enumerate(zip(keep, refs)):
        _report(f"gemm_tn_stream[{mode}-item{k}]", C, ref, 3e-5)
        _report(f"gemm_tn_stream[{mode}-item{k}]-dbias", db, bref[None, :], 2e-5, tile=(1, 1))


# ---------------------------------------------------------------------------------------------------------------- attention
ATTN_SHAPES = [(1, 1, 1, 64), (2, 16, 1, 64), (2, 32, 2, 128), (2, 33, 1, 64), (1, 224, 1, 64), (2, 50, 2, 64), (1, 197, 2, 64)]


def _lse_delta_ref(qkv, qp, zp, qmin, qmax, B, T, H, D, dO, ro):
    """lse = log sum exp of the scaled scores per query (natural log); delta = rowsum(dO . O) per head: [B * H, T]."""
    q = torch.round(qkv * qp[1]) + zp
    fq = ((q.clamp(qmin, qmax) - zp) * qp[0]).double()
    hd = D // H
    x = fq.view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    lse = torch.logsumexp((x[0] * hd ** -0.5) @ x[1].transpose(-2, -1), dim=-1).reshape(B * H, T)
    delta = (dO.double() * ro).view(B, T, H, hd).sum(-1).permute(0, 2, 1).reshape(B * H, T)
    return lse, delta


def _check_dqkv(what, dqkv, rg, qkv, qp, zp, dO, B, T, H, D, cs, tol=3e-5):
    assert not torch.isnan(dqkv).any(), what
    emu = None
    for name, c0, c1 in (("dQ", 0, D), ("dK", D, 2 * D), ("dV", 2 * D, 3 * D)):
        if T == 1 and name != "dV":
            # one token: softmax is the constant 1, the reference dQ and dK are exactly zero (tile_errors then normalises by 1: absolute RMS per tile) and what
            # a correct kernel leaves there is the rounding of dS = P (dP - delta), two numbers that cancel - no tolerance of the module says how much.  The bound
            # is twice the worst tile of the CPU emulation with the module's rounding points (tests/test_gpu_attn.py:_emulate), as for every derived bound
            if emu is None:
                emu = attn_emulate(qkv, qp[0].item(), zp, 0, 255, B, T, H, D, dO, cs)[1].to(rg.device)
            e_worst = tile_errors(emu[:, c0:c1], rg[:, c0:c1])[1]
            print(f"EMU {what}-{name}: emulation worst_tile {e_worst:.3e}")
            assert_tiles_close(dqkv[:, c0:c1], rg[:, c0:c1], 2 * e_worst, what=f"{what}-{name}")
            continue
        _report(f"{what}-{name}", dqkv[:, c0:c1], rg[:, c0:c1], tol)


@pytest.mark.parametrize("B,T,H,D", ATTN_SHAPES)
def test_attention_edges(native_lib, B, T, H, D):
    """The attention launchers at one token, at the 2-key-tile form half full, exactly full (32) and one past (33: the 14-tile form), at 224 tokens (every tile full)
    and at head_dim 32 on the 14-tile form: qatvit_attn_forward + the re-quantising backward, qatvit_attn_forward_f16 without and with saved codes, and the backward
    from the codes (two kernels at T <= 32 or head_dim 32, the fused kernel otherwise) - against the fp64 reference of tests/test_gpu_attn.py at its tolerances
    (O, dQ, dK, dV, delta 3e-5; the fp16 pair 2e-6), whole tensor and per 16 x 16 tile; lse and delta in the columns < T."""
    torch.manual_seed(B * T + D)
    g = Guards()
    hd = D // H
    qkv0 = torch.randn(B * T, 3 * D, device=DEV) * 1.5
    qkv0[0, :7] = 40.0      # clipped elements -> masked gradient
    qkv = g.inp(qkv0)
    scale, zp, qmin, qmax = 8.0 / 255, 120, 0, 255
    qp = torch.tensor([scale, 1.0, float(zp), 1.0], device=DEV)
    qp[1] = torch.ones(1, device=DEV)[0] / qp[0]
    qp = g.inp(qp)
    TP = native_lib.qatvit_attn_padded_tokens(T)
    dO0 = torch.randn(B * T, D, device=DEV)
    dO = g.inp(dO0)
    cs = g.inp(torch.rand(3 * D, device=DEV) + 0.5)
    ro, rg = attn_ref(qkv0, qp[0], zp, qmin, qmax, B, T, H, D, dO0)
    rg = rg * cs.double()[None, :]
    lse_ref, delta_ref = _lse_delta_ref(qkv0, qp, zp, qmin, qmax, B, T, H, D, dO0, ro)
    tag = f"attn[{B}-{T}-{H}-{D}]"
    st = _st()

    # ---- forward (bf16 pair) + the re-quantising backward
    Oh, Ol = g.out(B * T, D, torch.bfloat16), g.out(B * T, D, torch.bfloat16)
    lse = g.out(B * H, TP, torch.float32, fill=0.0)
    assert native_lib.qatvit_attn_forward(qkv.data_ptr(), qp.data_ptr(), qmin, qmax, B, T, H, D, Oh.data_ptr(), Ol.data_ptr(), lse.data_ptr(), st) == 0, \
        native_lib.qatvit_last_error()
    g.check(tag + " forward")
    _report(tag + "-fwd-O", Oh.float() + Ol.float(), ro, 3e-5)
    _report(tag + "-fwd-lse", lse[:, :T], lse_ref, 3e-5, tile=(1, 16))
    delta = g.out(B * H, TP, torch.float32, fill=0.0)
    gh, gl = g.out(B * T, 3 * D, torch.bfloat16), g.out(B * T, 3 * D, torch.bfloat16)
    assert native_lib.qatvit_attn_backward(qkv.data_ptr(), qp.data_ptr(), qmin, qmax, B, T, H, D, Oh.data_ptr(), Ol.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                           dO.data_ptr(), gh.data_ptr(), gl.data_ptr(), cs.data_ptr(), None, None, st) == 0, native_lib.qatvit_last_error()
    g.check(tag + " re-quantising backward")
    dqkv = gh.float() + gl.float()
    _check_dqkv(tag + "-bwd-requant", dqkv, rg, qkv0, qp, zp, dO0, B, T, H, D, cs)
    _report(tag + "-bwd-requant-delta", delta[:, :T], delta_ref, 3e-5, tile=(1, 16))
    assert (dqkv[0, :7] == 0).all()

    # ---- forward with the fp16 pair, without saved codes
    Oh1, Ol1 = g.out(B * T, D, torch.bfloat16), g.out(B * T, D, torch.bfloat16)
    O16h, O16l = g.out(B * T, D, torch.float16), g.out(B * T, D, torch.float16)
    osc = g.inp(torch.zeros(1, device=DEV))
    lse1 = g.out(B * H, TP, torch.float32, fill=0.0)
    assert native_lib.qatvit_attn_forward_f16(qkv.data_ptr(), qp.data_ptr(), qmin, qmax, B, T, H, D, Oh1.data_ptr(), Ol1.data_ptr(), lse1.data_ptr(),
                                              O16h.data_ptr(), O16l.data_ptr(), osc.data_ptr(), None, None, st) == 0, native_lib.qatvit_last_error()
    g.check(tag + " forward_f16")
    assert osc.item() == qp[0].item() / 64
    O16 = (O16h.double() + O16l.double()) * osc.double()
    assert not torch.isnan(O16).any() and O16h.float().abs().max().item() < 65504
    _report(tag + "-fwd16-O16", O16, ro, 2e-6)
    _report(tag + "-fwd16-O", Oh1.float() + Ol1.float(), ro, 3e-5)
    _report(tag + "-fwd16-lse", lse1[:, :T], lse_ref, 3e-5, tile=(1, 16))

    # ---- forward with the fp16 pair, saving the codes: the same bits, and the code / mask planes of test_attention_backward_from_saved_codes
    Oh2, Ol2 = g.out(B * T, D, torch.bfloat16), g.out(B * T, D, torch.bfloat16)
    O16h2, O16l2 = g.out(B * T, D, torch.float16), g.out(B * T, D, torch.float16)
    lse2 = g.out(B * H, TP, torch.float32, fill=0.0)
    codes = g.out(B * H * 3 * T, hd, torch.uint8)
    cmask = g.out(B * H * 3 * T, hd // 8, torch.uint8, pad=448)       # (4-byte rows at head_dim 32: twice the rows keep the 256-byte alignment)
    assert native_lib.qatvit_attn_forward_f16(qkv.data_ptr(), qp.data_ptr(), qmin, qmax, B, T, H, D, Oh2.data_ptr(), Ol2.data_ptr(), lse2.data_ptr(),
                                              O16h2.data_ptr(), O16l2.data_ptr(), osc.data_ptr(), codes.data_ptr(), cmask.data_ptr(), st) == 0, native_lib.qatvit_last_error()
    g.check(tag + " forward_f16 saving codes")
    for a, b in ((Oh1, Oh2), (Ol1, Ol2), (O16h, O16h2), (O16l, O16l2)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(lse1[:, :T], lse2[:, :T])
    t = (torch.round(qkv0 * qp[1]) + zp).view(B, T, 3, H, hd).permute(0, 3, 2, 1, 4).contiguous()
    assert torch.equal(codes.view(B, H, 3, T, hd).float(), t.clamp(qmin, qmax) - qmin)
    bits = ((t >= qmin) & (t <= qmax)).view(B, H, 3, T, hd // 8, 8).to(torch.uint8)
    want = (bits << torch.arange(8, device=DEV, dtype=torch.uint8)).sum(-1).to(torch.uint8)
    assert torch.equal(cmask.view(B, H, 3, T, hd // 8), want)

    # ---- backward from the saved codes (qkv = NULL): two kernels, or the fused kernel at head_dim 64 / 33..224 tokens
    delta2 = g.out(B * H, TP, torch.float32, fill=0.0)
    gh2, gl2 = g.out(B * T, 3 * D, torch.bfloat16), g.out(B * T, 3 * D, torch.bfloat16)
    assert native_lib.qatvit_attn_backward(None, qp.data_ptr(), qmin, qmax, B, T, H, D, Oh2.data_ptr(), Ol2.data_ptr(), lse2.data_ptr(), delta2.data_ptr(),
                                           dO.data_ptr(), gh2.data_ptr(), gl2.data_ptr(), cs.data_ptr(), codes.data_ptr(), cmask.data_ptr(), st) == 0, \
        native_lib.qatvit_last_error()
    g.check(tag + " backward from codes")
    dqkv2 = gh2.float() + gl2.float()
    fused = hd == 64 and 32 < T <= 224
    _check_dqkv(tag + ("-bwd-fused" if fused else "-bwd-codes"), dqkv2, rg, qkv0, qp, zp, dO0, B, T, H, D, cs)
    _report(tag + ("-bwd-fused" if fused else "-bwd-codes") + "-delta", delta2[:, :T], delta_ref, 3e-5, tile=(1, 16))
    assert (dqkv2[0, :7] == 0).all()
    c0 = 2 * D if fused else 0      # dV (every column in the two-kernel form): the bits of the re-quantising backward
    assert torch.equal(gh[:, c0:].view(torch.int16), gh2[:, c0:].view(torch.int16)) and torch.equal(gl[:, c0:].view(torch.int16), gl2[:, c0:].view(torch.int16))
