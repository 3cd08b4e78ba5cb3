"""tests/kernel_check.py on the CPU: a stock-torch emulation of qatvit_gemm_nt / qatvit_gemm_nt_f16 (the (hi, lo) planes multiplied with fp32
accumulation, then scale, column scale and bias in fp32) against the fp64 reference of tests/test_gpu_gemm.py, correct and with three planted faults
of the kind a ragged last row tile produces.  The per-tile bound at the kernel tests' own tolerance passes the correct emulation and catches every
fault; the whole-tensor relative L2 those tests asserted alone lets the first one through (the record of the gap)."""
import pytest
import torch

from tests.kernel_check import assert_tiles_close, guarded, guarded_copy, rel_l2_t, tile_errors
from tests.util import rel_l2

CASES = [(209, 384, 64, "bf16", 2e-5), (417, 128, 384, "bf16", 2e-5), (209, 384, 1536, "fp16", 1e-6)]
KSTEP = {"bf16": 16, "fp16": 32}        # the K extent of one MFMA


def _emulate(M, N, K, form):
    """(correct emulation, {fault: emulation with it}, fp64 reference)."""
    g = torch.Generator().manual_seed(M + N + K)
    B = torch.randint(-128, 128, (N, K), generator=g).float()
    if form == "bf16":
        A = torch.randn(M, K, generator=g) * 3
        pre, dt = 1.0, torch.bfloat16
    else:       # the operand of test_gemm_nt_f16_pair: wide dynamic range, pre-scaled by a power of two the scale takes out again
        A = torch.randn(M, K, generator=g).abs() * 3 * torch.rand(M, K, generator=g)
        A[::7] *= -0.05
        pre, dt = 2.0 ** 9, torch.float16
    hi = (A * pre).to(dt)
    lo = (A * pre - hi.float()).to(dt)
    s = torch.tensor(0.0123 / pre) * torch.tensor(0.0045)
    cs = torch.rand(N, generator=g) + 0.5
    bias = torch.randn(N, generator=g)
    ref = (A.double() @ B.double().t()) * (0.0123 * 0.0045) * cs.double() + bias.double()

    def post(acc):
        return acc * s * cs + bias

    acc = hi.float() @ B.t() + lo.float() @ B.t()
    good = post(acc)
    f1 = good.clone()
    f1[-1] = post(hi.float()[-1:] @ B.t())[0]
    f2 = good.clone()
    f2[M // 2, N // 3] -= bias[N // 3]
    ks = KSTEP[form]
    f3 = good.clone()
    f3[-1, :16] = post(hi.float()[-1:, :K - ks] @ B[:, :K - ks].t() + lo.float()[-1:, :K - ks] @ B[:, :K - ks].t())[0, :16]
    return good, {"lo plane dropped on the last row": f1, "bias missing on one element": f2, "last k-step lost on 16 elements of the last row": f3}, ref


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{c[3]}")
def emu(request):
    M, N, K, form, tol = request.param
    return (M, N, K, form, tol) + _emulate(M, N, K, form)


def test_correct_emulation_passes(emu):
    M, N, K, form, tol, good, _, ref = emu
    assert rel_l2(good, ref) < tol
    worst, _ = assert_tiles_close(good, ref, tol, what="correct emulation")
    assert worst < tol / 2                      # the kernel tests' tolerance is the tile bound with room: no bound of its own is needed here


@pytest.mark.parametrize("fault", ["lo plane dropped on the last row", "bias missing on one element", "last k-step lost on 16 elements of the last row"])
def test_planted_fault_fails(emu, fault):
    M, N, K, form, tol, good, faults, ref = emu
    with pytest.raises(AssertionError) as e:
        assert_tiles_close(faults[fault], ref, tol, what=fault)
    msg = str(e.value)
    _, _, (r0, c0) = tile_errors(faults[fault], ref)
    want_r0 = (M // 2) // 16 * 16 if fault.startswith("bias") else (M - 1) // 16 * 16
    assert r0 == want_r0 and f"rows {r0}.." in msg and "whole-tensor rel_l2" in msg and "tiles over the tolerance" in msg
    _, worst_good, _ = tile_errors(good, ref)
    assert tile_errors(faults[fault], ref)[1] > 50 * worst_good       # not a near miss: the metric separates them by orders of magnitude


def test_whole_tensor_l2_misses_the_dropped_lo_plane():
    """The gap this module closes: at (209, 384, 64) a last row computed without its lo plane passes rel_l2 < 2e-5, the assertion of test_gemm_nt."""
    good, faults, ref = _emulate(209, 384, 64, "bf16")
    bad = faults["lo plane dropped on the last row"]
    assert not torch.equal(bad[-1], good[-1])
    assert rel_l2(bad, ref) < 2e-5
    assert rel_l2_t(bad, ref) == pytest.approx(rel_l2(bad, ref), rel=1e-9)
    with pytest.raises(AssertionError):
        assert_tiles_close(bad, ref, 2e-5)


def test_tile_errors_ragged_edges_and_nan():
    ref = torch.ones(33, 18, dtype=torch.float64)
    got = ref.clone()
    got[32, 17] += 2.0          # the 1 x 2 corner tile: RMS over its TRUE element count = sqrt(4 / 2)
    err, worst, pos = tile_errors(got, ref)
    assert err.shape == (3, 2) and pos == (32, 16) and worst == pytest.approx(2.0 ** 0.5)
    assert (err.flatten()[:-1] == 0).all()
    got[0, 0] = float("nan")
    err, worst, pos = tile_errors(got, ref)
    assert pos == (0, 0) and worst != worst
    with pytest.raises(AssertionError, match="2 of 6 tiles"):
        assert_tiles_close(got, ref, 1e-3)
    err, worst, pos = tile_errors(torch.zeros(4, 5), torch.zeros(4, 5), tile=(1, 5))      # an all-zero reference divides by 1
    assert err.shape == (4, 1) and worst == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.int8, torch.uint8, torch.int32])
def test_guarded(dtype):
    t, check = guarded(5, 16, dtype, "cpu")
    assert t.shape == (5, 16) and t.dtype == dtype and t.is_contiguous()
    if dtype.is_floating_point:
        assert torch.isnan(t).all()             # untouched elements of an output stay NaN
    check()
    t.zero_()                                   # the whole extent may be written
    check()
    for row, where in ((5, "after"), (-1, "before")):          # one element of the row just past / just before the extent, as a kernel would reach it
        e = torch.as_strided(t, (1,), (1,), storage_offset=t.storage_offset() + row * 16 + 3)
        keep = e.clone()
        e.fill_(1)
        with pytest.raises(AssertionError, match=f"{where} the extent were overwritten, the first at row {row} .* column 3"):
            check()
        e.copy_(keep)
        check()


def test_guarded_copy_poisons_what_lies_past_the_extent():
    x = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    t, check = guarded_copy(x)
    assert torch.equal(t, x) and t.shape == x.shape
    check()
    flat = t.view(-1)
    past = torch.as_strided(flat, (4,), (1,), storage_offset=flat.storage_offset() + 24)
    before = torch.as_strided(flat, (4,), (1,), storage_offset=flat.storage_offset() - 4)
    assert torch.isnan(past).all() and torch.isnan(before).all()
    assert (past.view(torch.int32) == 0x7FC0BEEF).all()
