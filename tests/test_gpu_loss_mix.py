"""The mixed-target loss (qatvit_kd_ce_loss_mix through F.kd_ce_loss_mix, F.kd_ce_loss_table_mix and TeacherLogitTable.loss(mix=...)) on an
MI355X: against the fp64 restatement of tests/mix_ref.py with the tolerances tests/test_gpu_ops.py uses for this arithmetic, bit equality with
the two existing entries where nothing is mixed, the NaN rows of an index outside the table, and one whole mixed training step."""
import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd.vit import VisionTransformer
from tests import mix_ref
from tests.util import prepare, rel_l2

pytestmark = pytest.mark.gpu

HP = (4.0, 0.5, 0.1)
SHAPES = [(B, C) for B in (1, 7, 256) for C in (10, 100)]
FORMS = ["none", "tensor", "table"]
_cache = {}


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
        for b, l in zip(range(0, B, 5), (1.0, 0.0, 0.5, np.float32(0.9999))):      # the ends and two fixed values among the drawn ones
            recs[b] = mix_ref.mixup(part[b], l)
        if B == 1:
            recs[0] = mix_ref.mixup(0, 0.3)                                         # its only partner: itself
        if B > 2:
            recs[2] = mix_ref.cutmix(part[2], (3, 50, 10, 200), 224)                # a cutmix record: lam from the area
            recs[B - 1] = mix_ref.mixup(B, 0.25)                                    # a partner outside [0, B): self
        _cache[(B, C)] = (s, t, table, index, y, torch.tensor(recs, dtype=torch.int32))
    return _cache[(B, C)]


def _run(form, s, t, table, index, y, recs, existing=False):
    """(out3, dlogits) of the entry under test, or of the existing entry of the same form."""
    s = s.clone().cuda().requires_grad_(True)
    y, r = y.cuda(), None if recs is None else recs.cuda()
    if form == "table":
        args = (s, table.cuda(), index.cuda(), y)
        loss, parts = F.kd_ce_loss_table(*args, *HP) if existing else F.kd_ce_loss_table_mix(*args, r, *HP)
    else:
        args = (s, t.cuda() if form == "tensor" else None, y)
        loss, parts = F.kd_ce_loss(*args, *HP) if existing else F.kd_ce_loss_mix(*args, r, *HP)
    loss.backward()
    assert torch.equal(loss.detach(), parts[0])
    return parts.detach().cpu(), s.grad.cpu()


def _close(parts, grad, want, want_grad, what):
    loss, ce, kd = (float(v) for v in want)
    print(f"{what}: loss {abs(float(parts[0]) - loss) / max(1, abs(loss)):.2e} ce {abs(float(parts[1]) - ce) / max(1, abs(ce)):.2e} "
          f"kd {abs(float(parts[2]) - kd) / max(1, abs(kd)):.2e} grad {rel_l2(grad, want_grad):.2e}")
    assert abs(float(parts[0]) - loss) < 2e-6 * max(1, abs(loss))
    assert abs(float(parts[1]) - ce) < 2e-6 * max(1, abs(ce))
    assert abs(float(parts[2]) - kd) < 5e-6 * max(1, abs(kd))
    assert rel_l2(grad, want_grad) < 1e-5


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_against_the_fp64_reference_and_its_autograd(B, C, form):
    s, t, table, index, y, recs = _case(B, C)
    parts, grad = _run(form, s, t, table, index, y, recs)
    s64 = s.double().requires_grad_(True)
    want = mix_ref.loss(s64, y, recs, teacher=t if form == "tensor" else None, table=table if form == "table" else None, index=index,
                        kd_temp=HP[0], kd_alpha=HP[1], label_smoothing=HP[2])
    want[0].backward()
    _close(parts, grad, [v.detach() for v in want], s64.grad, f"B={B} C={C} {form}")
    if B > 2 and form != "none":                                     # the mix matters: the unmixed loss is another number
        assert abs(float(parts[0]) - float(_run(form, s, t, table, index, y, None)[0][0])) > 1e-3


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_lam_one_and_no_records_give_the_bits_of_the_existing_entries(B, C, form):
    s, t, table, index, y, recs = _case(B, C)
    want_parts, want_grad = _run(form, s, t, table, index, y, None, existing=True)
    ones = recs.clone()
    ones[:, 5] = mix_ref.f32_bits(1.0)                               # partners as drawn, in and out of range; only lam counts
    for r in (ones, None):
        parts, grad = _run(form, s, t, table, index, y, r)
        assert torch.equal(parts, want_parts) and torch.equal(grad, want_grad)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_lam_zero_is_the_existing_entry_on_the_partner(B, C, form):
    s, t, table, index, y, _ = _case(B, C)
    part = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    zeros = torch.tensor([mix_ref.mixup(int(p), 0.0) for p in part], dtype=torch.int32)
    parts, grad = _run(form, s, t, table, index, y, zeros)
    want_parts, want_grad = _run(form, s, t, table, index[part], y[part], None, existing=True)
    _close(parts, grad, want_parts.double(), want_grad, f"B={B} C={C} {form} lam=0")


@pytest.mark.parametrize("B", [7, 256])
def test_index_outside_the_table_and_partner_outside_the_batch(B):
    C = 10
    s, t, table, index, y, recs = _case(B, C)
    rows = table.shape[0]
    part = [(b + 1) % B for b in range(B)]
    lam = [1.0 if b % 2 else 0.5 for b in range(B)]                  # even rows mix, odd rows do not
    recs = torch.tensor([mix_ref.mixup(p, l) for p, l in zip(part, lam)], dtype=torch.int32)
    ok_parts, ok_grad = _run("table", s, t, table, index, y, recs)
    assert bool(torch.isfinite(ok_parts).all())

    def nan_rows(bad_index):
        parts, grad = _run("table", s, t, table, bad_index, y, recs)
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
    # a partner outside [0, B) is the sample itself, whatever lam says: the unmixed row
    self_recs = torch.tensor([mix_ref.mixup(p, 0.25) for p in ([-1, B, 2 ** 31 - 1, -(2 ** 31)] * B)[:B]], dtype=torch.int32)
    parts, grad = _run("table", s, t, table, index, y, self_recs)
    want_parts, want_grad = _run("table", s, t, table, index, y, None, existing=True)
    _close(parts, grad, want_parts.double(), want_grad, f"B={B} partner outside the batch")


def test_three_mixed_steps_of_the_tiny_student_do_not_synchronise():
    torch.manual_seed(31)
    teacher = VisionTransformer(embed_dim=128, depth=2, num_heads=2, num_classes=10, img_size=32)
    for p in teacher.parameters():
        p.requires_grad = False
    teacher = teacher.cuda().eval()
    torch.manual_seed(32)
    stu = qat_vit_amd.create_student("vit", qat_wrapper=True, embed_dim=128, depth=2, num_heads=2, img_size=32)
    student = prepare(stu.cuda().train(), "qnnpack").cuda().train()
    g = torch.Generator().manual_seed(5)
    data, labels = torch.randint(0, 256, (40, 8, 8, 3), generator=g, dtype=torch.uint8).cuda(), torch.randint(0, 10, (40,), generator=g).cuda()
    tr = qat_vit_amd.GpuResizeNormalize(8, out_size=32)
    table = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16, labels=labels)
    loader = qat_vit_amd.GpuImageLoader(data, labels, 8, shuffle=True, drop_last=True, transform=tr, generator=torch.Generator().manual_seed(7),
                                        return_index=True, augment=qat_vit_amd.RandomCropFlip(2), mix=qat_vit_amd.MixupCutmix(mode="elem"))
    opt = qat_vit_amd.ClipAdamW(student.parameters(), lr=1e-3)
    before = torch.cat([p.detach().flatten() for p in student.parameters()]).clone()
    losses, seen = [], []

    def step(batch):
        x, y, idx, r = batch
        opt.zero_grad(set_to_none=False)
        loss, parts = table.loss(student(x), idx, y, *HP, mix=r)
        loss.backward()
        opt.step(max_norm=1.0)
        losses.append(parts)
        seen.append(r)

    batches = iter(loader)
    step(next(batches))                                              # the first step builds the engine and the optimizer's tables
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
