"""The class-parallel KD + CE loss (qatvit_kd_ce_loss_rows through class_parallel=True) on an MI355X: against the fp64 restatement of
tests/mix_ref.py and its autograd at the stride, instance and form boundaries of the wave and workgroup kernels; bit equalities of the new entry
with itself; the NaN rows of an index outside the table and of a NaN logit; guarded operands; the default path unchanged.

Inputs: tests/test_gpu_bce_loss.py's _case.  Bars.  C <= 257: the project's for this arithmetic (loss and CE 2e-6 * max(1, |v|), KD 5e-6 * max(1, |v|),
gradient rel_l2 < 1e-5).  Above: per quantity the larger of that bar and twice the error of the stock fp32 torch composition of the same loss against the
same fp64 reference, measured in the test for the case at hand; both are printed (-s).  No bar comes from the kernel under test or the serial entry."""
import importlib.util
import os

import pytest
import torch

from qat_vit_amd import functional as F
from qat_vit_amd import native
from tests import mix_ref
from tests.kernel_check import guarded, guarded_copy
from tests.test_gpu_bce_loss import _case, _errors, _kw

pytestmark = pytest.mark.gpu

KD = (4.0, 0.5, 0.1)                                                 # kd_temp, kd_alpha, label_smoothing
PROJECT = (2e-6, 2e-6, 5e-6, 1e-5)                                   # loss, CE, KD, gradient
CLASSES = [2, 63, 64, 65, 257, 1000, 1024, 1025, 4096, 4097, 21841]  # stride 64; 1 / 4 / 16 values per lane; wave / workgroup; registers / re-read
SHAPES = [(B, C) for B in (1, 5, 9) for C in CLASSES] + [(600, 10)]
FORMS = ["none", "tensor", "table"]
_spec = importlib.util.spec_from_file_location("bench_ce_rows", os.path.join(os.path.dirname(__file__), "..", "tools", "bench_ce_rows.py"))
bench = importlib.util.module_from_spec(_spec)                      # its `composition`: the stock fp32 torch form of this loss, T, alpha, eps = KD
_spec.loader.exec_module(bench)


def _run(form, s, t, table, index, y, recs, **kw):
    s = s.clone().cuda().requires_grad_(True)
    m = None if recs is None else recs.cuda()
    if form == "table":
        loss, parts = F.kd_ce_loss_table_mix(s, table.cuda(), index.cuda(), y.cuda(), m, *KD, **kw)
    else:
        loss, parts = F.kd_ce_loss_mix(s, t.cuda() if form == "tensor" else None, y.cuda(), m, *KD, **kw)
    loss.backward()
    assert torch.equal(loss.detach(), parts[0])
    return parts.detach().cpu(), s.grad.cpu()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_against_the_fp64_reference_and_its_autograd(B, C, form):
    s, t, table, index, y, recs = _case(B, C)
    for r in (recs, None):
        s64 = s.double().requires_grad_(True)
        want = mix_ref.loss(s64, y, r, kd_temp=KD[0], kd_alpha=KD[1], label_smoothing=KD[2], **_kw(form, t, table, index, dev=False))
        want[0].backward()
        want = [float(v.detach()) for v in want]
        bars = PROJECT
        if C > 257:
            s32 = s.clone().cuda().requires_grad_(True)
            got = bench.composition(s32, y.cuda(), None if r is None else r.cuda(), **_kw(form, t, table, index))
            got[0].backward()
            comp = _errors(torch.stack(got).detach().cpu(), s32.grad.cpu(), want, s64.grad)
            bars = tuple(max(p, 2 * c) for p, c in zip(PROJECT, comp))
            print(f"B={B} C={C} {form}: fp32 torch composition against fp64: " + " ".join(f"{v:.2e}" for v in comp))
        parts, grad = _run(form, s, t, table, index, y, r, class_parallel=True)
        err = _errors(parts, grad, want, s64.grad)
        print(f"B={B} C={C} {form} {'mix' if r is not None else 'plain'}: loss, ce, kd, grad", *(f"{v:.2e}" for v in err), "bars", *(f"{v:.2e}" for v in bars))
        assert bool(torch.isfinite(parts).all()) and bool(torch.isfinite(grad).all())
        assert form != "none" or (float(parts[2]) == 0.0 and torch.equal(parts[0], parts[1]))
        for e, bar, name in zip(err, bars, ("loss", "ce", "kd", "gradient")):
            assert e < bar, f"B={B} C={C} {form}: {name} error {e:.3e} is not below {bar:.3e}"


@pytest.mark.parametrize("C", [65, 1000, 4097])
def test_bit_equalities_of_the_new_entry(C):
    B = 9
    s, t, table, index, y, recs = (v.clone() for v in _case(B, C))
    ones = recs.clone()
    ones[:, 5] = mix_ref.f32_bits(1.0)                               # partners as drawn, in and out of range; only lam counts
    s[7], t[7], index[7], y[7] = s[0], t[0], index[0], y[0]          # two equal rows, in different workgroups of either form
    recs[0] = recs[7] = torch.tensor(mix_ref.mixup(3, 0.3), dtype=torch.int32)
    for form in FORMS:
        plain = _run(form, s, t, table, index, y, None, class_parallel=True)
        lam1 = _run(form, s, t, table, index, y, ones, class_parallel=True)
        assert torch.equal(plain[0], lam1[0]) and torch.equal(plain[1], lam1[1])
        parts, grad = _run(form, s, t, table, index, y, recs, class_parallel=True)
        assert torch.equal(grad[0], grad[7]) and not torch.equal(grad[0], grad[1])
        again = _run(form, s, t, table, index, y, recs, class_parallel=True)
        assert parts.view(torch.int32).tolist() == again[0].view(torch.int32).tolist() and torch.equal(grad, again[1])
    as_table = _run("table", s, t, table, index, y, None, class_parallel=True)
    as_tensor = _run("tensor", s, table[index], table, index, y, None, class_parallel=True)
    assert torch.equal(as_table[0], as_tensor[0]) and torch.equal(as_table[1], as_tensor[1])


@pytest.mark.parametrize("C", [10, 1025])
def test_index_outside_the_table_and_nan_logit(C):
    B = 7
    g = torch.Generator().manual_seed(77 + C)
    s, table, y = 3 * torch.randn(B, C, generator=g), 5 * torch.randn(B + 5, C, generator=g), torch.randint(0, C, (B,), generator=g)
    index, rows = torch.randperm(B + 5, generator=g)[:B], B + 5
    lam = [1.0 if b % 2 else 0.5 for b in range(B)]                  # even rows mix with the next row, odd rows do not
    recs = torch.tensor([mix_ref.mixup((b + 1) % B, l) for b, l in enumerate(lam)], dtype=torch.int32)
    ok_parts, ok_grad = _run("table", s, None, table, index, y, recs, class_parallel=True)
    assert bool(torch.isfinite(ok_parts).all())
    for value in (rows, -1, 2 ** 62):
        for at, want_rows in ((4, [4]), (5, [4, 5]), (3, [2, 3])):   # own index; the partner's index of a mixing row; not of an unmixed one
            bad = index.clone()
            bad[at] = value
            parts, grad = _run("table", s, None, table, bad, y, recs, class_parallel=True)
            nan = torch.isnan(grad).any(1)
            assert bool(torch.isnan(parts).all()) and nan.nonzero().flatten().tolist() == want_rows
            assert bool(torch.isnan(grad[nan]).all()) and torch.equal(grad[~nan], ok_grad[~nan])
    bad = s.clone()
    bad[6, C // 2] = float("nan")
    parts, grad = _run("table", bad, None, table, index, y, recs, class_parallel=True)
    keep = torch.arange(B) != 6
    assert bool(torch.isnan(parts).all()) and bool(torch.isnan(grad[6]).all()) and torch.equal(grad[keep], ok_grad[keep])


@pytest.mark.parametrize("B,C", [(5, 65), (5, 1025)])
def test_guarded_operands(B, C):
    s, t, table, index, y, recs = _case(B, C)                        # C odd: rows at odd 4-byte offsets; dlogits and partials hold NaN on entry
    want_parts, want_grad = _run("table", s, t, table, index, y, recs, class_parallel=True)
    sg, s_check = guarded_copy(s.cuda())
    dl, d_check = guarded_copy(torch.full((B, C), float("nan"), device="cuda"))
    pt, p_check = guarded(1, 2 * B, torch.float32, "cuda")
    out3 = torch.empty(3, device="cuda")
    tab, idx, yy, rr = table.cuda(), index.cuda(), y.cuda(), recs.cuda()
    native.check(native.lib().qatvit_kd_ce_loss_rows(sg.data_ptr(), None, tab.data_ptr(), tab.shape[0], idx.data_ptr(), yy.data_ptr(), rr.data_ptr(), B, C,
                                                     *KD, pt.data_ptr(), out3.data_ptr(), dl.data_ptr(), native.stream_ptr()), "qatvit_kd_ce_loss_rows")
    torch.cuda.synchronize()
    s_check("student"), d_check("dlogits"), p_check("partials")
    assert torch.equal(sg.cpu(), s) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(pt).all())
    assert torch.equal(out3.cpu(), want_parts) and torch.equal(dl.cpu(), want_grad)


def test_the_default_is_unchanged():
    s, t, _, _, y, _ = _case(9, 65)
    runs = []
    for kw in ({}, {"class_parallel": False}):
        sg = s.clone().cuda().requires_grad_(True)
        loss, parts = F.kd_ce_loss(sg, t.cuda(), y.cuda(), *KD, **kw)
        loss.backward()
        runs.append((parts.detach().cpu(), sg.grad.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    big, zeros = torch.zeros(2, 4097, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="bad shape"):
        F.kd_ce_loss(big, None, zeros, *KD)
    assert bool(torch.isfinite(F.kd_ce_loss(big, None, zeros, *KD, class_parallel=True)[0]))
