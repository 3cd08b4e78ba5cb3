"""The one-plane backward (include/qatvit.h QATVIT_BWD_DY16): every gradient that feeds a dgrad / wgrad GEMM pair is ONE fp16 plane scaled by a
power of two predicted from the previous backward, instead of a bf16 (hi, lo) pair.  Replaces the same `loss.backward()`
(/root/reference/src/training/qat_trainer.py:359); tolerance 1e-3 relative L2 per gradient tensor against the pair form / the fp64 product.

* kernels on identical inputs: the one-plane dgrad and the three weight-gradient forms against fp64 on the ROUNDED plane (what the kernel is
  asked to compute: <= 2e-5) and against the unrounded gradient (what the form costs: ~1.5e-4);
* the protocol: first step calibrates (bit-identical to a pair-form engine), later steps run one-plane (logits and observer state still
  bit-identical - the forward's arithmetic does not change - every parameter gradient within 1e-3 of the pair form);
* a loss scaled by 2^10 between two steps is followed by the max |dlogits| ratio (no fallback);
* a scale history that no longer holds raises the overflow flag; the step is repeated in the pair form and equals a pair-form step."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import qat_vit_amd  # noqa: E402
from qat_vit_amd import engine as E  # noqa: E402
from qat_vit_amd import functional as F  # noqa: E402
from qat_vit_amd import native  # noqa: E402
from tests.kernel_check import assert_tiles_close, guarded, tile_errors  # noqa: E402
from tests.util import prepare, rel_l2  # noqa: E402

P = ctypes.c_void_p


def _ptr(t):
    return P(t.data_ptr()) if t is not None else None


def _scalar(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("M,N,K", [(1576, 384, 1536), (50432, 384, 1152), (1000, 1536, 384)])
def test_dgrad_one_plane_vs_fp64(native_lib, M, N, K):
    """C[M,N] = dY16[M,K] . Wt16[N,K]^T * s1 * 2^-e (proj / fc1 / qkv / fc2 dgrad shapes)."""
    g = torch.Generator(device="cuda").manual_seed(M + N)
    dy = torch.randn(M, K, generator=g, device="cuda") * 3e-6 * torch.exp(torch.randn(M, K, generator=g, device="cuda"))   # heavy-tailed, gradient-sized
    wt = torch.randint(-127, 128, (N, K), generator=g, device="cuda").float()
    e = 8 - int(np.floor(np.log2(dy.abs().max().item())) + 1)
    plane = (dy * 2.0 ** e).to(torch.float16)
    assert torch.isfinite(plane).all()
    C, canary = guarded(M, N, torch.float32, "cuda")
    s1, s2 = _scalar(0.0123), _scalar(2.0 ** -e)
    native.check(native_lib.qatvit_gemm_nt_dy16(_ptr(plane), _ptr(wt.to(torch.float16)), _ptr(C), M, N, K, K, K, N, _ptr(s1), _ptr(s2), P(native.stream_ptr())), "nt_dy16")
    ref_rounded = (plane.double() @ wt.double().T) * (0.0123 * 2.0 ** -e)
    ref_exact = (dy.double() @ wt.double().T) * 0.0123
    canary("gemm_nt_dy16 C")
    assert rel_l2(C.cpu().numpy(), ref_rounded.cpu().numpy()) < 2e-5
    assert_tiles_close(C, ref_rounded, 2e-5, what="gemm_nt_dy16 against the rounded plane")
    assert rel_l2(C.cpu().numpy(), ref_exact.cpu().numpy()) < 4e-4
    # what the form costs, per tile: the gradient is heavy-tailed, a tile that holds one of its largest rows carries that row's fp16 rounding (2^-12 of a value
    # many times the RMS) - measured 5.4e-4 at M = 50,432 for a correct kernel.  The bound is therefore not 4e-4 but twice the worst tile of the emulation: the
    # exact fp64 product on the ROUNDED plane (ref_rounded, stock torch) against the same reference - every rounding the kernel is asked to make, and no other
    cost = tile_errors(ref_rounded, ref_exact)[1]
    print(f"EMU gemm_nt_dy16 against the unrounded gradient: emulation worst_tile {cost:.3e}")
    assert_tiles_close(C, ref_exact, 2 * cost, what="gemm_nt_dy16 against the unrounded gradient")


@pytest.mark.parametrize("M,N,Kw,kind", [(1576, 1152, 384, "grid"), (50432, 1536, 384, "grid"), (50432, 384, 384, "pair"), (1576, 384, 1536, "codes"),
                                         (50432, 384, 1536, "codes")])
def test_wgrad_one_plane_vs_fp64(native_lib, M, N, Kw, kind):
    """dW[N,Kw] += sum_m dY16[m,N] X[m,Kw] * s_x * 2^-e, db[N] += sum_m dY16 * 2^-e: X as fp16 integers, an fp16 pair, or codes + a table of fp16 pairs."""
    g = torch.Generator(device="cuda").manual_seed(N + Kw)
    dy = torch.randn(M, N, generator=g, device="cuda") * 2e-6 * torch.exp(torch.randn(M, N, generator=g, device="cuda"))
    e = 8 - int(np.floor(np.log2(dy.abs().max().item())) + 1)
    plane = (dy * 2.0 ** e).to(torch.float16)
    sx = 0.0371
    qh = ql = qc = lut = None
    if kind == "grid":
        xv = torch.randint(-255, 256, (M, Kw), generator=g, device="cuda").float()
        qh = xv.to(torch.float16)
    elif kind == "pair":
        xv = torch.randn(M, Kw, generator=g, device="cuda") * 300.0
        qh = xv.to(torch.float16)
        ql = (xv - qh.float()).to(torch.float16)
        xv = qh.float() + ql.float()
    else:
        tab = torch.randn(256, generator=g, device="cuda") * 400.0
        th = tab.to(torch.float16)
        tl = (tab - th.float()).to(torch.float16)
        lut = ((th.view(torch.int16).int() & 0xffff) | (tl.view(torch.int16).int() << 16)).contiguous()
        qc = torch.randint(0, 256, (M, Kw), generator=g, device="cuda").to(torch.uint8)
        # (the table's lo halves are ignored: the float X operand enters the one-plane weight gradient rounded to fp16)
        xv = th.float()[qc.long()]
    dW, canary = guarded(N, Kw, torch.float32, "cuda", fill=0.0)
    db2d, canary_db = guarded(1, N, torch.float32, "cuda", fill=0.0)
    db = db2d[0]
    scratch = torch.empty(native_lib.qatvit_gemm_tn_scratch_bytes(), dtype=torch.uint8, device="cuda")
    s1, s2 = _scalar(sx), _scalar(2.0 ** -e)
    native.check(native_lib.qatvit_gemm_tn_dy16(_ptr(plane), _ptr(qh), _ptr(ql), _ptr(qc), _ptr(lut), _ptr(dW), M, N, Kw, N, Kw, Kw, _ptr(s1), _ptr(s2), None, None, None,
                                                0, -128, 127, _ptr(db), None, _ptr(scratch), scratch.numel(), P(native.stream_ptr())), "tn_dy16")
    ref_rounded = (plane.double().T @ xv.double()) * (sx * 2.0 ** -e)
    ref_exact = (dy.double().T @ xv.double()) * sx
    canary("gemm_tn_dy16 dW"), canary_db("gemm_tn_dy16 dbias")
    assert rel_l2(dW.cpu().numpy(), ref_rounded.cpu().numpy()) < 2e-5
    assert_tiles_close(dW, ref_rounded, 2e-5, what="gemm_tn_dy16 against the rounded plane")
    assert rel_l2(dW.cpu().numpy(), ref_exact.cpu().numpy()) < 4e-4     # (codes: against the table value the kernel is given, hi half)
    cost = tile_errors(ref_rounded, ref_exact)[1]      # (as in test_dgrad_one_plane_vs_fp64: twice the worst tile of the fp64 product on the rounded plane)
    print(f"EMU gemm_tn_dy16 against the unrounded gradient: emulation worst_tile {cost:.3e}")
    assert_tiles_close(dW, ref_exact, 2 * cost, what="gemm_tn_dy16 against the unrounded gradient")
    assert rel_l2(db.cpu().numpy(), (plane.double().sum(0) * 2.0 ** -e).cpu().numpy()) < 2e-5
    assert_tiles_close(db2d, (plane.double().sum(0) * 2.0 ** -e)[None, :], 2e-5, tile=(1, 16), what="gemm_tn_dy16 dbias")


@pytest.mark.parametrize("M,N,Kw,center,zp", [(1576, 1152, 384, 128, 131), (50432, 1536, 384, 128, 0), (50432, 1152, 384, 64, 127), (999, 384, 768, 128, 255)])
def test_wgrad_one_plane_byte_grid_vs_fp64(native_lib, M, N, Kw, center, zp):
    """The grid X operand as one byte per element (the forward's int8 operand, q - center): X = Q8 + center - zero_point, expanded to fp16 in registers
    after a transposed byte read (k_gemm_tn_q8).  Exact integers either way: the result must match the fp16-plane form's reference to fp32 rounding."""
    g = torch.Generator(device="cuda").manual_seed(N + Kw + zp)
    dy = torch.randn(M, N, generator=g, device="cuda") * 2e-6 * torch.exp(torch.randn(M, N, generator=g, device="cuda"))
    e = 8 - int(np.floor(np.log2(dy.abs().max().item())) + 1)
    plane = (dy * 2.0 ** e).to(torch.float16)
    qlo, qhi = (0, 255) if center == 128 else (0, 127)
    q = torch.randint(qlo, qhi + 1, (M, Kw), generator=g, device="cuda")
    q8 = (q - center).to(torch.int8)
    sx = 0.0371
    a_qp = torch.tensor([sx, 1.0 / sx, float(zp), 1.0], dtype=torch.float32, device="cuda")
    dW, canary = guarded(N, Kw, torch.float32, "cuda", fill=0.0)
    db2d, canary_db = guarded(1, N, torch.float32, "cuda", fill=0.0)
    db = db2d[0]
    scratch = torch.empty(native_lib.qatvit_gemm_tn_scratch_bytes(), dtype=torch.uint8, device="cuda")
    s2 = _scalar(2.0 ** -e)
    native.check(native_lib.qatvit_gemm_tn_q8_dy16(_ptr(plane), _ptr(q8), _ptr(a_qp), center, _ptr(dW), M, N, Kw, N, Kw, Kw, _ptr(s2), None, None, None, 0, -128, 127,
                                                   _ptr(db), None, _ptr(scratch), scratch.numel(), P(native.stream_ptr())), "tn_q8_dy16")
    ref = (plane.double().T @ (q - zp).double()) * (sx * 2.0 ** -e)
    canary("gemm_tn_q8_dy16 dW"), canary_db("gemm_tn_q8_dy16 dbias")
    assert rel_l2(dW.cpu().numpy(), ref.cpu().numpy()) < 2e-5
    assert_tiles_close(dW, ref, 2e-5, what="gemm_tn_q8_dy16 dW")
    assert rel_l2(db.cpu().numpy(), (plane.double().sum(0) * 2.0 ** -e).cpu().numpy()) < 2e-5
    assert_tiles_close(db2d, (plane.double().sum(0) * 2.0 ** -e)[None, :], 2e-5, tile=(1, 16), what="gemm_tn_q8_dy16 dbias")
    # ... and without the split scratch (atomic accumulation), on top of a non-zero dW
    dW2, canary2 = guarded(N, Kw, torch.float32, "cuda", fill=1e-4)
    native.check(native_lib.qatvit_gemm_tn_q8_dy16(_ptr(plane), _ptr(q8), _ptr(a_qp), center, _ptr(dW2), M, N, Kw, N, Kw, Kw, _ptr(s2), None, None, None, 0, -128, 127,
                                                   None, None, None, 0, P(native.stream_ptr())), "tn_q8_dy16")
    canary2("gemm_tn_q8_dy16 dW (atomics)")
    assert rel_l2((dW2.double() - 1e-4).cpu().numpy(), ref.cpu().numpy()) < 1e-4      # (fp32 atomics onto 1e-4: ~1e-5)
    assert_tiles_close(dW2.double() - 1e-4, ref, 1e-4, what="gemm_tn_q8_dy16 dW (atomics)")


@pytest.mark.parametrize("M", [70, 640])   # one split and the in-kernel tail | two splits for every form: k_tn_reduce with scratch, atomics without
@pytest.mark.parametrize("kind", ["grid", "pair", "codes", "q8"])
def test_wgrad_one_plane_mask_row_div_per_channel(native_lib, M, kind):
    """The four per-GEMM one-plane forms with the request fields no other per-GEMM test sets: W with per-channel w_scale / w_zp, row_div and dbias, on
    a non-zero dW.  fp64 on the rounded plane, divided by row_div, under the STE mask in the kernel's own fp32 arithmetic (rint(W * (1 / scale)) + zp).
    row_div, w_scale and w_zp are three different vectors, so a launcher that swaps two of them fails.  N = 256, Kw = 384: the pair form takes the
    narrow tile (2 wide tiles < 8), the others the wide one."""
    N, Kw = 256, 384
    g = torch.Generator(device="cuda").manual_seed(1000 + M + len(kind))
    dy = torch.randn(M, N, generator=g, device="cuda") * 2e-6 * torch.exp(torch.randn(M, N, generator=g, device="cuda"))
    e = 8 - int(np.floor(np.log2(dy.abs().max().item())) + 1)
    plane = (dy * 2.0 ** e).to(torch.float16)
    sx, center, zp = 0.0371, 128, 131
    qh = ql = qc = lut = q8 = None
    if kind == "grid":
        xv = torch.randint(-255, 256, (M, Kw), generator=g, device="cuda").float()
        qh = xv.to(torch.float16)
    elif kind == "pair":
        xv = torch.randn(M, Kw, generator=g, device="cuda") * 300.0
        qh = xv.to(torch.float16)
        ql = (xv - qh.float()).to(torch.float16)
        xv = qh.float() + ql.float()
    elif kind == "codes":
        tab = torch.randn(256, generator=g, device="cuda") * 400.0
        th = tab.to(torch.float16)
        tl = (tab - th.float()).to(torch.float16)
        lut = ((th.view(torch.int16).int() & 0xffff) | (tl.view(torch.int16).int() << 16)).contiguous()
        qc = torch.randint(0, 256, (M, Kw), generator=g, device="cuda").to(torch.uint8)
        xv = th.float()[qc.long()]
    else:
        q = torch.randint(0, 256, (M, Kw), generator=g, device="cuda")
        q8 = (q - center).to(torch.int8)
        xv = (q - zp).float()
    W = torch.randn(N, Kw, generator=g, device="cuda")
    wsc = 0.012 + 0.004 * torch.rand(N, generator=g, device="cuda")            # clips |W + zp * scale| > 1.5 .. 2.0: 4 - 13 % of a standard normal
    wzp = torch.randint(-8, 9, (N,), generator=g, device="cuda").to(torch.int32)
    rdiv = 0.5 + torch.rand(N, generator=g, device="cuda")
    C0 = torch.randn(N, Kw, generator=g, device="cuda") * 1e-5
    s1, s2 = _scalar(sx), _scalar(2.0 ** -e)
    a_qp = torch.tensor([sx, 1.0 / sx, float(zp), 1.0], dtype=torch.float32, device="cuda")
    scratch = torch.empty(native_lib.qatvit_gemm_tn_scratch_bytes(), dtype=torch.uint8, device="cuda")

    def run(dW, db, sc):
        tail = (_ptr(W), _ptr(wsc), _ptr(wzp), 1, -128, 127, _ptr(db), _ptr(rdiv), _ptr(sc), sc.numel() if sc is not None else 0, P(native.stream_ptr()))
        if kind == "q8":
            rc = native_lib.qatvit_gemm_tn_q8_dy16(_ptr(plane), _ptr(q8), _ptr(a_qp), center, _ptr(dW), M, N, Kw, N, Kw, Kw, _ptr(s2), *tail)
        else:
            rc = native_lib.qatvit_gemm_tn_dy16(_ptr(plane), _ptr(qh), _ptr(ql), _ptr(qc), _ptr(lut), _ptr(dW), M, N, Kw, N, Kw, Kw, _ptr(s1), _ptr(s2), *tail)
        native.check(rc, "tn_dy16 " + kind)

    qq = torch.round(W * (1.0 / wsc)[:, None]) + wzp.float()[:, None]
    keep = (qq >= -128) & (qq <= 127)
    clipped = 1.0 - keep.double().mean().item()
    ref = (plane.double().T @ xv.double()) * (sx * 2.0 ** -e) / rdiv.double()[:, None]
    ref = torch.where(keep, ref, torch.zeros_like(ref))
    bref = plane.double().sum(0) * 2.0 ** -e / rdiv.double()
    (dW, canary), (db2d, canary_db) = guarded(N, Kw, torch.float32, "cuda"), guarded(1, N, torch.float32, "cuda", fill=0.0)
    dW.copy_(C0)
    db = db2d[0]
    run(dW, db, scratch)
    canary(f"tn_dy16 {kind} dW"), canary_db(f"tn_dy16 {kind} dbias")
    err_w, err_b = rel_l2((dW.double() - C0.double()).cpu().numpy(), ref.cpu().numpy()), rel_l2(db.cpu().numpy(), bref.cpu().numpy())
    dW2, db2 = C0.clone(), torch.zeros(N, device="cuda")
    run(dW2, db2, scratch)
    (dW3, canary3), db3 = guarded(N, Kw, torch.float32, "cuda", fill=1e-4), torch.zeros(N, device="cuda")
    run(dW3, db3, None)
    canary3(f"tn_dy16 {kind} dW (atomics)")
    err_wa, err_ba = rel_l2((dW3.double() - 1e-4).cpu().numpy(), ref.cpu().numpy()), rel_l2(db3.cpu().numpy(), bref.cpu().numpy())
    print(f"{kind} M={M}: clipped {clipped:.4f}; scratch dW {err_w:.2e} db {err_b:.2e}; atomics dW {err_wa:.2e} db {err_ba:.2e}")
    assert 0.01 < clipped < 0.2
    assert err_w < 2e-5 and err_b < 2e-5
    assert_tiles_close(dW.double() - C0.double(), ref, 2e-5, what=f"tn_dy16 {kind} dW")
    assert_tiles_close(db2d, bref[None, :], 2e-5, tile=(1, 16), what=f"tn_dy16 {kind} dbias")
    assert torch.equal(dW, dW2), "with scratch the splits are summed in a fixed order: same bits on a second run"
    assert err_wa < 1e-4 and err_ba < 1e-4      # (fp32 atomics onto 1e-4: ~1e-5)
    assert_tiles_close(dW3.double() - 1e-4, ref, 1e-4, what=f"tn_dy16 {kind} dW (atomics)")
    assert_tiles_close(db3[None, :], bref[None, :], 1e-4, tile=(1, 16), what=f"tn_dy16 {kind} dbias (atomics)")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("M,shapes", [(640, [(1536, 384)] * 12 + [(1152, 384)] * 10 + [(384, 768)] * 2),      # 282 tiles of 10 steps: whole tiles in registers AND cut tiles
                                      (640, [(1536, 384)] * 24),                                                # 288 tiles: more tiles than CUs, last round 12 % full - free spans over one workgroup per CU
                                      (640, [(2560, 384)] * 24),                                                # 480 tiles: whole tiles round-robin over two rounds
                                      (1280, [(384, 1536)] * 12),                                               # 144 tiles (the fc2 batch): two aligned launches, 7 x 3 + 5 x 4 splits
                                      (6400, [(1536, 384), (1152, 384), (384, 384)]),                           # 24 tiles of 100 steps on ~256 workgroups: every tile cut ~10 times
                                      (25216, [(384, 1536), (128, 384)])])                                      # Kw tiles; a one-tile GEMM at the end
def test_wgrad_stream_batch_vs_fp64(native_lib, mode, M, shapes):
    """qatvit_gemm_tn_stream_dy16: the weight gradients of a backward call as ONE persistent stream-K launch per X form - each item against fp64 on the rounded plane,
    with and without the weight STE mask / bias gradient / per-channel division, on top of a non-zero dW; a second run gives the same bits (fixed summation order)."""
    g = torch.Generator(device="cuda").manual_seed(100 * mode + M)
    items = (native.TNItem * len(shapes))()
    keep, refs = [], []
    center, zp = 128, 131.0
    for k, (N, Kw) in enumerate(shapes):
        dy = torch.randn(M, N, generator=g, device="cuda") * 2e-6 * torch.exp(torch.randn(M, N, generator=g, device="cuda"))
        e = 8 - int(np.floor(np.log2(dy.abs().max().item())) + 1)
        plane = (dy * 2.0 ** e).to(torch.float16)
        sx = 0.02 + 0.01 * k
        lut = None
        if mode == 0:
            q = torch.randint(0, 256, (M, Kw), generator=g, device="cuda")
            Q = (q - center).to(torch.int8)
            xv = (q - zp).double()
            s1 = torch.tensor([sx, 1.0 / sx, zp, 1.0], dtype=torch.float32, device="cuda")
        elif mode == 1:
            tab = (torch.randn(256, generator=g, device="cuda") * 400.0).to(torch.float16)
            lut = (tab.view(torch.int16).int() & 0xffff).contiguous()
            Q = torch.randint(0, 256, (M, Kw), generator=g, device="cuda").to(torch.uint8)
            xv = tab.double()[Q.long()]
            s1 = _scalar(sx)
        else:
            Q = (torch.randn(M, Kw, generator=g, device="cuda") * 300.0).to(torch.float16)
            xv = Q.double()
            s1 = _scalar(sx)
        s2 = _scalar(2.0 ** -e)
        C0 = torch.randn(N, Kw, generator=g, device="cuda") * 1e-5
        C, canary = guarded(N, Kw, torch.float32, "cuda")
        C.copy_(C0)
        masked, biased, divided = k % 2 == 0, k % 3 != 1, k % 4 == 3
        W = torch.randn(N, Kw, generator=g, device="cuda") if masked else None
        wsc = torch.full((N,), 0.01, device="cuda") if masked else None
        wzp = torch.zeros(N, dtype=torch.int32, device="cuda") if masked else None
        db = torch.zeros(N, device="cuda") if biased else None
        rdiv = (0.5 + torch.rand(N, generator=g, device="cuda")) if divided else None
        it = items[k]
        it.P, it.Q, it.lut, it.s1, it.s2, it.C = plane.data_ptr(), Q.data_ptr(), (lut.data_ptr() if lut is not None else None), s1.data_ptr(), s2.data_ptr(), C.data_ptr()
        it.W, it.w_scale, it.w_zp = (W.data_ptr(), wsc.data_ptr(), wzp.data_ptr()) if masked else (None, None, None)
        it.dbias, it.row_div = (db.data_ptr() if biased else None), (rdiv.data_ptr() if divided else None)
        it.N, it.Kw, it.ldp, it.ldq, it.ldc = N, Kw, N, Kw, Kw
        ref = (plane.double().T @ xv) * (sx * 2.0 ** -e)
        if divided:
            ref = ref / rdiv.double()[:, None]
        if masked:   # per-channel scales 0.01, [-128, 127]: |W| > 1.27 .. 1.28 is clipped; the mask in the kernel's own fp32 arithmetic (rint(W * (1 / scale)))
            qq = torch.round(W * (1.0 / wsc)[:, None])
            ref = torch.where((qq >= -128) & (qq <= 127), ref, torch.zeros_like(ref))
        bref = plane.double().sum(0) * 2.0 ** -e / (rdiv.double() if divided else 1.0)
        keep.append((plane, Q, lut, s1, s2, C, W, wsc, wzp, db, rdiv, C0, canary))
        refs.append((ref, bref))
    scratch = torch.empty(native_lib.qatvit_gemm_tn_stream_scratch_bytes(), dtype=torch.uint8, device="cuda")

    def run():
        native.check(native_lib.qatvit_gemm_tn_stream_dy16(mode, ctypes.cast(items, ctypes.c_void_p), len(shapes), M, center, 1, -128, 127, _ptr(scratch), scratch.numel(),
                                                           P(native.stream_ptr())), "tn_stream_dy16")
    run()
    first = []
    for k, ((plane, Q, lut, s1, s2, C, W, wsc, wzp, db, rdiv, C0, canary), (ref, bref)) in enumerate(zip(keep, refs)):
        canary(f"tn_stream item {k} dW")
        got = (C.double() - C0.double())
        assert rel_l2(got.cpu().numpy(), ref.cpu().numpy()) < 3e-5
        assert_tiles_close(got, ref, 3e-5, what=f"tn_stream item {k} dW")
        if db is not None:
            assert rel_l2(db.cpu().numpy(), bref.cpu().numpy()) < 2e-5
            assert_tiles_close(db[None, :], bref[None, :], 2e-5, tile=(1, 16), what=f"tn_stream item {k} dbias")
        first.append(C.clone())
        C.copy_(C0)
    run()
    for (_, _, _, _, _, C, *_), f in zip(keep, first):
        assert torch.equal(C, f), "the split tiles are summed in a fixed order: same bits on a second run"


def _pair(seed=0, backend="qnnpack", **kw):
    torch.manual_seed(seed)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **kw)
    a = prepare(copy.deepcopy(stu).cuda(), backend)   # one-plane engine
    b = prepare(copy.deepcopy(stu).cuda(), backend)   # pair-form engine
    return a, b


def _step(m, x, y, scale=1.0):
    for p in m.parameters():
        p.grad = None
    out = m(x)
    (F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)[0] * scale).backward()
    return out


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_protocol_calibrate_then_one_plane(native_lib, backend):
    a, b = _pair(3, backend)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(8, 3, 224, 224, generator=g).cuda() for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), generator=g).cuda() for _ in range(3)]
    ea, eb = E.bind(a, 8), E.bind(b, 8)
    assert ea.dy16, "ViT-S at 197 tokens is a configuration the one-plane backward covers"
    eb.dy16 = False
    worst, worst_n = 0.0, ""
    for k, (x, y) in enumerate(zip(xs, ys)):
        scale = 1.0 if k < 2 else 1024.0          # the third step's loss is 2^10 times larger: the max |dlogits| ratio moves every scale with it
        oa, ob = _step(a, x, y, scale), _step(b, x, y, scale)
        assert torch.equal(oa, ob), "the forward's arithmetic does not depend on the form of the backward"
        for (n, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
            assert torch.equal(u, v), n
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            e = rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy())
            if k == 0:   # calibration IS the pair form (bias / LayerNorm gradients use fp32 atomics: 1e-6)
                assert e < 2e-6, (n, e)
            else:
                assert e < 1e-3, (k, n, e)
                if e > worst:
                    worst, worst_n = e, f"{n} (step {k})"
        assert ea._fwd_x16 == (k > 0)
    assert ea.dy16_fallbacks == 0
    assert worst > 1e-6, "the one-plane form did not run"
    print(f"one-plane vs pair form, worst parameter gradient rel L2: {worst:.2e} at {worst_n}")


def test_overflow_falls_back_to_the_pair_form(native_lib):
    a, b = _pair(4)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(8, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 10, (8,), generator=g).cuda()
    ea, eb = E.bind(a, 8), E.bind(b, 8)
    eb.dy16 = False
    _step(a, x, y); _step(b, x, y)
    # wreck the history: every tensor's previous maximum 2^-60 -> scales 2^68 -> the planes overflow
    c = ea.cfg
    off = ea.lib.qatvit_student_tensor_offset(ctypes.byref(c), b"dy16", 0)
    st = ea.workspace[off:off + 4 * (64 + 256 * 4 * c.depth)].view(torch.float32)
    for t in range(4 * c.depth):
        st[64 + 256 * t + 3] = 2.0 ** -60
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        oa = _step(a, x, y)
    ob = _step(b, x, y)
    assert ea.dy16_fallbacks == 1 and any("fp16 plane" in str(i.message) for i in w)
    assert torch.equal(oa, ob)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.isfinite(p.grad).all(), n
        assert rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy()) < 2e-6, n      # the repeated backward is the pair form
    # the fallback re-recorded the maxima: the next step is one-plane again and needs no second fallback
    oa, ob = _step(a, x, y), _step(b, x, y)
    assert ea._fwd_x16 and ea.dy16_fallbacks == 1
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy()) < 1e-3, n


def test_unsupported_configuration_keeps_the_pair_form(native_lib):
    """head_dim 64 at 5 tokens (32-pixel images): the fused attention backward - the only one with a one-plane output - does not apply."""
    a, _ = _pair(5, embed_dim=128, depth=2, num_heads=2, img_size=32)
    x = torch.randn(4, 3, 32, 32).cuda()
    y = torch.randint(0, 10, (4,)).cuda()
    _step(a, x, y); _step(a, x, y)
    ea = E.engine_of(a)
    assert not ea.dy16 and not ea._fwd_x16
    assert ea.lib.qatvit_student_dy16_supported(ctypes.byref(ea.cfg)) == 0


def test_training_trajectory_one_plane_tracks_the_pair_form(native_lib):
    """Ten optimizer steps (clip + AdamW, warm-up learning rates, a fresh batch every step, an input scale that drifts) of a ViT-S-width depth-2 student in the pair form;
    at every step a second copy with the SAME weights and observer state runs the one-plane backward with the deferred stream-K weight gradients: the delayed scales must
    follow gradients that change with the weights and the data (no fallback after the calibrating step) and every parameter gradient stays within 1e-3 of the pair form's.
    (The copy is re-synchronised after every step: fake-quant is discontinuous, two free-running trajectories separate at the first flipped code - seen: 3.6e-3 in the loss
    after ten steps in one run, 0.33 in another.)"""
    from qat_vit_amd.optim import ClipAdamW

    a, b = _pair(11, depth=2)
    g = torch.Generator().manual_seed(12)
    ea, eb = E.bind(a, 16), E.bind(b, 16)
    eb.dy16 = False
    ob = ClipAdamW(b.parameters(), lr=1e-3, weight_decay=1e-2)
    worst, worst_at = 0.0, ""
    for k in range(10):
        x = torch.randn(16, 3, 224, 224, generator=g).cuda() * (1.0 + 0.2 * k)     # the input scale drifts too
        y = torch.randint(0, 10, (16,), generator=g).cuda()
        for grp in ob.param_groups:
            grp["lr"] = 1e-3 * min(1.0, (k + 1) / 4)
        oa_, ob_ = _step(a, x, y), _step(b, x, y)
        assert torch.equal(oa_, ob_), k
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.isfinite(p.grad).all(), (k, n)
            e = rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy())
            if k > 0 and e > worst:
                worst, worst_at = e, f"{n} (step {k})"
        ob.step(max_norm=1.0)
        a.load_state_dict(b.state_dict())            # same weights, same observer state for the next step (in place: the engine keeps its pointers)
    assert ea._fwd_x16 and ea.dy16_fallbacks == 0, ea.dy16_fallbacks
    print(f"one-plane vs pair form over ten training steps, worst parameter gradient rel L2: {worst:.2e} at {worst_at}")
    assert 1e-6 < worst < 1e-3, (worst, worst_at)
