"""The binary cross-entropy objective (qatvit_kd_bce_loss through F.kd_bce_loss, qat_vit_amd.BinaryCrossEntropy and TeacherLogitTable.bce_loss) on
an MI355X: against the fp64 restatement of tests/bce_ref.py and its autograd at the shapes where one wave per row, four rows per workgroup and a
class loop of stride 64 can go wrong; what the mix records and the threshold do; bit equality where nothing is mixed, between equal rows and
between equal calls; wide and NaN logits; the NaN rows of an index outside the table; guarded operands; whole mixed training steps.

Bars.  C <= 129: the project's bars for this arithmetic (tests/test_gpu_loss_mix.py): loss and hard part 2e-6 * max(1, |v|), KD 5e-6 * max(1, |v|),
gradient rel_l2 < 1e-5.  C = 1000 and 4096: per quantity the larger of that bar and twice the error of the stock fp32 torch composition
(bce_ref.composition on the GPU) against the same fp64 reference, measured in the test for the case at hand; both numbers are printed (-s shows them), and
tools/bench_bce_loss.py writes the pair into profiles/bce_loss_bench.txt.  No bar comes from the kernel under test."""
import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native
from qat_vit_amd.vit import VisionTransformer
from tests import bce_ref, mix_ref
from tests.util import prepare, rel_l2

pytestmark = pytest.mark.gpu

KD = (4.0, 0.5)
PROJECT = (2e-6, 2e-6, 5e-6, 1e-5)                                   # loss, hard part, KD, gradient
SHAPES = [(B, C) for B in (1, 4, 5, 9) for C in (2, 3, 63, 64, 65, 129, 1000, 4096)] + [(600, 10)]
FORMS = ["none", "tensor", "table"]
CONFIGS = [(eps, thr, sc) for eps in (0.0, 0.1) for thr in (None, 0.2) for sc in (False, True)]     # label_smoothing, target_threshold, sum_classes
PLAIN = (0.1, None, False)
_cache, _wants, _bars_cache = {}, {}, {}


def _case(B, C):
    """Per shape, built once and never changed (host tensors): student, teacher, table, a permuted index into it, labels, records."""
    if (B, C) not in _cache:
        g = torch.Generator().manual_seed(100 * B + C)
        rows = B + 5
        s, t, table = 3 * torch.randn(B, C, generator=g), 5 * torch.randn(B, C, generator=g), 5 * torch.randn(rows, C, generator=g)
        index, y = torch.randperm(rows, generator=g)[:B], torch.randint(0, C, (B,), generator=g)
        lam = torch.rand(B, generator=g).numpy().astype(np.float32)
        part = torch.randint(0, B, (B,), generator=g).tolist()
        recs = [mix_ref.mixup(p, l) for p, l in zip(part, lam)]
        for b, l in zip(range(min(B, 4)), (1.0, 0.0, 0.5, np.float32(0.9999))):   # the ends and two fixed values in front of the drawn ones
            recs[b] = mix_ref.mixup(part[b], l)
        if B == 1:
            recs[0] = mix_ref.mixup(0, 0.3)                                       # its only partner: itself
        if B >= 9:
            recs[4] = mix_ref.cutmix(part[4], (3, 50, 10, 200), 224)              # a cutmix record: lam from the area
            recs[5] = mix_ref.mixup(5, 0.3)                                       # its own partner
        if B >= 4:
            recs[B - 1] = mix_ref.mixup(B, 0.25)                                  # a partner outside [0, B): self
        _cache[(B, C)] = (s, t, table, index, y, torch.tensor(recs, dtype=torch.int32))
    return _cache[(B, C)]


def _kw(form, t, table, index, dev=True):
    put = (lambda v: v.cuda()) if dev else (lambda v: v)
    if form == "tensor":
        return {"teacher": put(t)}
    if form == "table":
        return {"table": put(table), "index": put(index)}
    return {}


def _run(form, s, t, table, index, y, recs, cfg=PLAIN):
    """(out3, dlogits) of the entry under test."""
    s = s.clone().cuda().requires_grad_(True)
    loss, parts = F.kd_bce_loss(s, y.cuda(), mix=None if recs is None else recs.cuda(), kd_temp=KD[0], kd_alpha=KD[1], label_smoothing=cfg[0],
                                target_threshold=cfg[1], sum_classes=cfg[2], **_kw(form, t, table, index))
    loss.backward()
    assert torch.equal(loss.detach(), parts[0])
    return parts.detach().cpu(), s.grad.cpu()


def _want(form, s, t, table, index, y, recs, cfg=PLAIN, key=None):
    """((loss, bce, kd), gradient) of the fp64 reference; with a key, computed once and shared."""
    if key is not None and key in _wants:
        return _wants[key]
    s64 = s.double().requires_grad_(True)
    want = bce_ref.loss(s64, y, recs, kd_temp=KD[0], kd_alpha=KD[1], label_smoothing=cfg[0], target_threshold=cfg[1], sum_classes=cfg[2],
                        **_kw(form, t, table, index, dev=False))
    want[0].backward()
    out = ([float(v.detach()) for v in want], s64.grad)
    if key is not None:
        _wants[key] = out
    return out


def _errors(parts, grad, want, want_grad):
    return tuple(abs(float(p) - w) / max(1.0, abs(w)) for p, w in zip(parts, want)) + (float(rel_l2(grad, want_grad)),)


def _bars(form, B, C, cfg):
    """The bars of the case (B, C, form, cfg) of _case: the project's; at C >= 1000 raised to twice what the stock fp32 composition misses the
    fp64 reference by on this GPU."""
    key = (B, C, form, cfg)
    if C <= 129:
        return PROJECT
    if key not in _bars_cache:
        s, t, table, index, y, recs = _case(B, C)
        want, want_grad = _want(form, s, t, table, index, y, recs, cfg, key)
        s32 = s.clone().cuda().requires_grad_(True)
        got = bce_ref.composition(s32, y.cuda(), recs.cuda(), kd_temp=KD[0], kd_alpha=KD[1], label_smoothing=cfg[0], target_threshold=cfg[1],
                                  sum_classes=cfg[2], **_kw(form, t, table, index))
        got[0].backward()
        comp = _errors(torch.stack(got).detach().cpu(), s32.grad.cpu(), want, want_grad)
        _bars_cache[key] = tuple(max(p, 2 * c) for p, c in zip(PROJECT, comp))
        print(f"B={B} C={C} {form} {cfg}: fp32 torch composition against fp64: loss {comp[0]:.2e} bce {comp[1]:.2e} kd {comp[2]:.2e} grad {comp[3]:.2e}"
              f" -> bars {', '.join(f'{v:.2e}' for v in _bars_cache[key])}")
    return _bars_cache[key]


def _close(parts, grad, want, want_grad, bars, what):
    err = _errors(parts, grad, want, want_grad)
    print(f"{what}: loss {err[0]:.2e} bce {err[1]:.2e} kd {err[2]:.2e} grad {err[3]:.2e} (bars {', '.join(f'{v:.2e}' for v in bars)})")
    assert bool(torch.isfinite(parts).all()) and bool(torch.isfinite(grad).all())
    for e, bar, name in zip(err, bars, ("loss", "bce", "kd", "gradient")):
        assert e < bar, f"{what}: {name} error {e:.3e} is not below {bar:.3e}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_against_the_fp64_reference_and_its_autograd(B, C, form):
    s, t, table, index, y, recs = _case(B, C)
    for cfg in CONFIGS:
        parts, grad = _run(form, s, t, table, index, y, recs, cfg)
        want, want_grad = _want(form, s, t, table, index, y, recs, cfg, (B, C, form, cfg))
        if form == "none":
            assert float(parts[2]) == 0.0 and torch.equal(parts[0], parts[1])
        _close(parts, grad, want, want_grad, _bars(form, B, C, cfg), f"B={B} C={C} {form} eps={cfg[0]} thr={cfg[1]} sum_classes={cfg[2]}")


@pytest.mark.parametrize("C,sum_classes", [(3, False), (65, True)])
def test_the_mix_matters_and_the_objective_is_not_ce(C, sum_classes):
    """The mean over B * C elements dilutes what a label is worth by 1 / C: at C = 65 the sum over the classes is the number that moves by 1e-3.
    Every inequality is asserted on the host reference first: it is a property of the case, then of the kernel."""
    B, cfg = 9, (0.1, None, sum_classes)
    s, t, table, index, y, recs = _case(B, C)
    for form in FORMS:
        mixed, plain = _run(form, s, t, table, index, y, recs, cfg)[0], _run(form, s, t, table, index, y, None, cfg)[0]
        want_mixed, want_plain = _want(form, s, t, table, index, y, recs, cfg)[0], _want(form, s, t, table, index, y, None, cfg)[0]
        assert abs(want_mixed[0] - want_plain[0]) > 1e-3 and abs(want_mixed[1] - want_plain[1]) > 1e-3
        assert abs(float(mixed[0]) - float(plain[0])) > 1e-3 and abs(float(mixed[1]) - float(plain[1])) > 1e-3
    ce = F.kd_ce_loss_mix(s.cuda(), None, y.cuda(), recs.cuda(), KD[0], KD[1], 0.1)[1].cpu()
    bce = _run("none", s, t, table, index, y, recs, cfg)[0]
    assert abs(float(mix_ref.loss(s, y, recs)[1]) - _want("none", s, t, table, index, y, recs, cfg)[0][1]) > 1e-3
    assert abs(float(ce[1]) - float(bce[1])) > 1e-3
    # the threshold and sum_classes give other numbers again
    assert abs(_want("none", s, t, table, index, y, recs, (0.1, 0.2, sum_classes))[0][0] - _want("none", s, t, table, index, y, recs, cfg)[0][0]) > 1e-3
    assert abs(float(_run("none", s, t, table, index, y, recs, (0.1, 0.2, sum_classes))[0][0]) - float(bce[0])) > 1e-3
    other = float(_run("none", s, t, table, index, y, recs, (0.1, None, not sum_classes))[0][0])
    assert max(other, float(bce[0])) == pytest.approx(C * min(other, float(bce[0])), rel=1e-5)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,C", [(1, 3), (5, 64), (9, 65), (9, 1000), (600, 10)])
def test_lam_one_and_no_records_give_the_same_bits(B, C, form):
    s, t, table, index, y, recs = _case(B, C)
    ones = recs.clone()
    ones[:, 5] = mix_ref.f32_bits(1.0)                               # partners as drawn, in and out of range; only lam counts
    for cfg in (PLAIN, (0.0, 0.2, True)):
        want_parts, want_grad = _run(form, s, t, table, index, y, None, cfg)
        parts, grad = _run(form, s, t, table, index, y, ones, cfg)
        assert torch.equal(parts, want_parts) and torch.equal(grad, want_grad)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,C", [(4, 3), (5, 64), (9, 65), (9, 1000), (600, 10)])
def test_lam_zero_is_the_unmixed_call_on_the_partner(B, C, form):
    s, t, table, index, y, _ = _case(B, C)
    part = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    zeros = torch.tensor([mix_ref.mixup(int(p), 0.0) for p in part], dtype=torch.int32)
    parts, grad = _run(form, s, t, table, index, y, zeros)
    want_parts, want_grad = _run(form, s, t, table, index[part], y[part], None)      # (a teacher tensor saw the mixed images: its rows stay)
    _close(parts, grad, [float(v) for v in want_parts], want_grad, _bars(form, B, C, PLAIN), f"B={B} C={C} {form} lam=0")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C", [65, 1000])
def test_equal_rows_and_equal_calls_give_equal_bits(C, form):
    B = 9
    s, t, table, index, y, recs = (v.clone() for v in _case(B, C))
    s[7], t[7], index[7], y[7] = s[0], t[0], index[0], y[0]          # row 0: the first wave of workgroup 0; row 7: the last wave of workgroup 1
    recs[0] = recs[7] = torch.tensor(mix_ref.mixup(3, 0.3), dtype=torch.int32)
    for cfg in (PLAIN, (0.1, 0.2, True)):
        parts, grad = _run(form, s, t, table, index, y, recs, cfg)
        assert torch.equal(grad[0], grad[7]) and not torch.equal(grad[0], grad[1])
        again = _run(form, s, t, table, index, y, recs, cfg)
        assert torch.equal(parts, again[0]) and torch.equal(grad, again[1])
        assert parts.view(torch.int32).tolist() == again[0].view(torch.int32).tolist()


@pytest.mark.parametrize("form", FORMS)
def test_wide_and_nan_logits(form):
    B, C = 9, 65
    s, t, table, index, y, recs = (v.clone() for v in _case(B, C))
    for b, v in enumerate((20.0, 88.0, 104.0, 1e4)):
        cols = [int(y[b]), (int(y[b]) + 1) % C, 17, 64]              # the label's class, its neighbour, one inside, the last class
        s[b, cols] = torch.tensor([v, -v, -v, v])
    for cfg in (PLAIN, (0.0, None, True), (0.1, 0.2, False)):
        parts, grad = _run(form, s, t, table, index, y, recs, cfg)
        want, want_grad = _want(form, s, t, table, index, y, recs, cfg)
        _close(parts, grad, want, want_grad, PROJECT, f"wide logits, {form}, {cfg}")
    parts, grad = _run(form, s, t, table, index, y, recs)
    bad = s.clone()
    bad[6, 21] = float("nan")
    nan_parts, nan_grad = _run(form, bad, t, table, index, y, recs)
    assert bool(torch.isnan(nan_parts[:2]).all()) and (form == "none" or bool(torch.isnan(nan_parts[2])))
    # the hard part is per element: without a teacher the NaN stays at its element, as in the reference's autograd; the KD part's softmax takes
    # it to the whole row
    assert bool(torch.isnan(nan_grad[6, 21])) and (form == "none" or bool(torch.isnan(nan_grad[6]).all()))
    keep = torch.arange(B) != 6
    assert torch.equal(nan_grad[keep], grad[keep])
    if form == "none":
        rest = torch.arange(C) != 21
        assert torch.equal(nan_grad[6, rest], grad[6, rest])


def test_index_outside_the_table_and_partner_outside_the_batch():
    B, C = 7, 10
    g = torch.Generator().manual_seed(77)
    s, table, y = 3 * torch.randn(B, C, generator=g), 5 * torch.randn(B + 5, C, generator=g), torch.randint(0, C, (B,), generator=g)
    index, rows = torch.randperm(B + 5, generator=g)[:B], B + 5
    part = [(b + 1) % B for b in range(B)]
    lam = [1.0 if b % 2 else 0.5 for b in range(B)]                  # even rows mix, odd rows do not
    recs = torch.tensor([mix_ref.mixup(p, l) for p, l in zip(part, lam)], dtype=torch.int32)
    ok_parts, ok_grad = _run("table", s, None, table, index, y, recs)
    assert bool(torch.isfinite(ok_parts).all())

    def nan_rows(bad_index):
        parts, grad = _run("table", s, None, table, bad_index, y, recs)
        assert bool(torch.isnan(parts).all())
        rows_ = torch.isnan(grad).any(1)
        assert bool(torch.isnan(grad[rows_]).all()) and torch.equal(grad[~rows_], ok_grad[~rows_])
        return rows_.nonzero().flatten().tolist()

    for value in (rows, -1, 2 ** 62):
        bad = index.clone()
        bad[4] = value                                               # row 4 mixes with row 5; row 3 does not mix (its partner is 4)
        assert nan_rows(bad) == [4]
        bad = index.clone()
        bad[5] = value                                               # row 5's own index, and the partner's index of row 4, which mixes
        assert nan_rows(bad) == [4, 5]
        bad = index.clone()
        bad[3] = value                                               # row 2 mixes with row 3
        assert nan_rows(bad) == [2, 3]
    # a partner outside [0, B) is the sample itself: the row mixed with itself, the bits of a record that names the row as its own partner
    self_recs = torch.tensor([mix_ref.mixup(p, 0.25) for p in ([-1, B, 2 ** 31 - 1, -(2 ** 31)] * B)[:B]], dtype=torch.int32)
    parts, grad = _run("table", s, None, table, index, y, self_recs)
    want, want_grad = _want("table", s, None, table, index, y, self_recs)
    _close(parts, grad, want, want_grad, PROJECT, "partner outside the batch")
    own = torch.tensor([mix_ref.mixup(b, 0.25) for b in range(B)], dtype=torch.int32)
    own_parts, own_grad = _run("table", s, None, table, index, y, own)
    assert torch.equal(parts, own_parts) and torch.equal(grad, own_grad)


@pytest.mark.parametrize("B,C", [(5, 65), (9, 1000)])
def test_guarded_operands(B, C):
    """student, dlogits and partials as views inside larger poisoned buffers at offsets that are no multiple of 16 bytes: the bytes outside stay,
    the result is the wrapper's bit for bit, and partials' contents on entry (NaN) are ignored."""
    s, t, table, index, y, recs = _case(B, C)
    want_parts, want_grad = _run("table", s, t, table, index, y, recs)
    G = 67
    sbuf = torch.full((G + B * C + G,), float("nan")).cuda()
    sbuf[G:G + B * C] = s.flatten().cuda()
    dbuf = torch.full((G + B * C + G,), 0x7fc12345, dtype=torch.int32).view(torch.float32).cuda()      # a NaN with a payload of its own
    pbuf = torch.full((G + 2 * B + G,), float("nan")).cuda()
    before = [v.clone().view(torch.int32) for v in (sbuf, dbuf, pbuf)]
    out3 = torch.empty(3, device="cuda")
    tab, idx, yy, rr = table.cuda(), index.cuda(), y.cuda(), recs.cuda()
    native.check(native.lib().qatvit_kd_bce_loss(sbuf.data_ptr() + 4 * G, None, tab.data_ptr(), tab.shape[0], idx.data_ptr(), yy.data_ptr(), rr.data_ptr(),
                                                 B, C, KD[0], KD[1], PLAIN[0], -1.0, 0, pbuf.data_ptr() + 4 * G, out3.data_ptr(), dbuf.data_ptr() + 4 * G,
                                                 native.stream_ptr()), "qatvit_kd_bce_loss")
    torch.cuda.synchronize()
    after = [v.view(torch.int32) for v in (sbuf, dbuf, pbuf)]
    assert torch.equal(after[0], before[0])                                           # the student is read only
    for a, b, n in ((after[1], before[1], B * C), (after[2], before[2], 2 * B)):
        assert torch.equal(a[:G], b[:G]) and torch.equal(a[G + n:], b[G + n:])
    assert torch.equal(out3.cpu(), want_parts) and torch.equal(dbuf[G:G + B * C].view(B, C).cpu(), want_grad)
    assert bool(torch.isfinite(pbuf[G:G + 2 * B]).all())


def test_three_mixed_steps_of_the_tiny_student_do_not_synchronise():
    torch.manual_seed(31)
    teacher = VisionTransformer(embed_dim=128, depth=2, num_heads=2, num_classes=10, img_size=32)
    for p in teacher.parameters():
        p.requires_grad = False
    teacher = teacher.cuda().eval()
    g = torch.Generator().manual_seed(5)
    data, labels = torch.randint(0, 256, (40, 8, 8, 3), generator=g, dtype=torch.uint8).cuda(), torch.randint(0, 10, (40,), generator=g).cuda()
    tr = qat_vit_amd.GpuResizeNormalize(8, out_size=32)
    table = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16, labels=labels)
    crit = qat_vit_amd.BinaryCrossEntropy(smoothing=0.1)

    def table_loss(out, y, idx, r):
        return table.bce_loss(out, idx, y, *KD, 0.1, mix=r)

    def criterion(out, y, idx, r):
        loss = crit(out, y, mix=r)
        return loss, loss.detach().reshape(1)

    for loss_fn in (table_loss, criterion):
        torch.manual_seed(32)
        stu = qat_vit_amd.create_student("vit", qat_wrapper=True, embed_dim=128, depth=2, num_heads=2, img_size=32)
        student = prepare(stu.cuda().train(), "qnnpack").cuda().train()
        loader = qat_vit_amd.GpuImageLoader(data, labels, 8, shuffle=True, drop_last=True, transform=tr, generator=torch.Generator().manual_seed(7),
                                            return_index=True, augment=qat_vit_amd.RandomCropFlip(2), mix=qat_vit_amd.MixupCutmix(mode="elem"))
        opt = qat_vit_amd.ClipAdamW(student.parameters(), lr=1e-3)
        before = torch.cat([p.detach().flatten() for p in student.parameters()]).clone()
        losses, seen = [], []

        def step(batch):
            x, y, idx, r = batch
            opt.zero_grad(set_to_none=False)
            loss, parts = loss_fn(student(x), y, idx, r)
            loss.backward()
            opt.step(max_norm=1.0)
            losses.append(parts)
            seen.append(r)

        batches = iter(loader)
        step(next(batches))                                          # the first step builds the engine and the optimizer's tables
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            step(next(batches))
            step(next(batches))
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        torch.cuda.synchronize()
        after = torch.cat([p.detach().flatten() for p in student.parameters()])
        assert len(losses) == 3 and all(bool(torch.isfinite(p).all()) for p in losses)
        assert bool(torch.isfinite(after).all()) and float((after - before).abs().max()) > 0
        mixed = torch.cat(seen).cpu()
        assert mixed.shape == (24, 6) and (mixed[:, 5] != mix_ref.f32_bits(1.0)).any()      # something was mixed
