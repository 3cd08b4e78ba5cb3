"""On-device validation on an MI355X (qatvit_eval_accumulate, qat_vit_amd.EvalAccumulator / evaluate): the kernel's counts
against torch on the same tensor, torch.argmax's tie and NaN rules, accumulation over launches, strided rows and guard bands, labels and indices
outside their range, the second opinion in both forms, and evaluate() against the reference's loop restated here."""
import copy

import pytest
import torch
import torch.nn.functional as TF
from torch.utils.data import DataLoader, TensorDataset

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.evaluate import COUNTERS, STATE_WORDS, EvalResult
from qat_vit_amd.vit import VisionTransformer
from tests.util import fq_modules, prepare

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
INTS = COUNTERS[:8]     # the counts that do not describe the loss sum
LOSS_RTOL = 1e-5        # per-row fp32 exp / log / subtract on max-subtracted values, a few ulp of 6e-8 each, on losses of order 1 to 10: about 10x margin
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _random(B, C, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * B + C + seed)
    return (3 * torch.randn(B, C, generator=g)).to(dtype).cuda(), torch.randint(0, C, (B,), generator=g).cuda()


def _run(logits, labels, C, other=None, index=None, confusion=True):
    acc = qat_vit_amd.EvalAccumulator(C, confusion=confusion)
    acc.update(logits, labels, other, index)
    return acc.result()


def _ints(r):
    return tuple(getattr(r, n) if getattr(r, n) is not None else 0 for n in INTS)


def _confusion(labels, pred, C):
    return torch.bincount(labels * C + pred, minlength=C * C).view(C, C).cpu()


def _close(a, b, what=""):
    err = abs(a - b) / max(abs(b), 1e-300)
    print(f"{what}: loss sum {a!r} against {b!r}, relative error {err:.2e} (bound {LOSS_RTOL:.0e})")
    assert err <= LOSS_RTOL, (what, a, b, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B,C", [(1, 2), (7, 10), (257, 10), (64, 65), (33, 1000)])
def test_kernel_counts_equal_torch(native_lib, B, C, dtype):
    logits, labels = _random(B, C, dtype)
    r = _run(logits, labels, C)
    pred = logits.argmax(1)
    assert r.total == B and r.correct == int((pred == labels).sum())
    assert torch.equal(r.confusion, _confusion(labels, pred, C))
    assert (r.bad_labels, r.nonfinite_rows, r.bad_index, r.loss_rows) == (0, 0, 0, B) and r.agree is None
    want = float(TF.cross_entropy(logits.double(), labels, reduction="sum"))
    _close(r.loss_sum, want, f"B={B} C={C} {dtype}")
    assert r.accuracy == 100.0 * r.correct / B and r.loss == r.loss_sum / B


SPECIAL_ROWS = [[1, 3, 3, 2], [float("nan"), 5, float("nan"), 1], [2, float("nan"), float("inf"), float("nan")], [float("-inf")] * 4,
                [float("inf"), 1, float("inf"), 0], [0.0, -0.0, 0.0, 0.0]]
SPECIAL_PREDS = [1, 0, 1, 0, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_ties_and_specials_follow_torch_argmax(native_lib, dtype):
    C = 10
    rows = [r + [float("-inf") if r[0] == float("-inf") else -1.0] * (C - 4) for r in SPECIAL_ROWS]   # padded with smaller values
    logits = torch.tensor(rows, dtype=torch.float32).to(dtype).cuda()
    labels = torch.arange(6).cuda()                      # one matrix row per sample: the prediction of sample b is where row b holds its 1
    r = _run(logits, labels, C)
    assert torch.equal(r.confusion.sum(1), torch.tensor([1] * 6 + [0] * 4))
    pred = r.confusion[:6].argmax(1)
    assert pred.tolist() == SPECIAL_PREDS
    assert torch.equal(pred, logits.argmax(1).cpu())
    per_row = TF.cross_entropy(logits.double(), labels, reduction="none").cpu()
    finite = torch.isfinite(per_row)
    assert not finite[1] and not finite[2] and not finite[3] and finite[0] and finite[5]     # the NaN and -inf rows have no finite loss
    assert r.nonfinite_rows == int((~finite).sum()) and r.loss_rows == int(finite.sum()) and r.total == 6
    _close(r.loss_sum, float(per_row[finite].sum()), f"specials {dtype}")
    assert r.correct == sum(int(p == b) for b, p in enumerate(SPECIAL_PREDS))


def _raw(logits, labels, C, state, confusion, other=None, index=None, rows=0):
    """One call of the C entry point on raw pointers (state / confusion are views into larger guard buffers)."""
    native.check(native.lib().qatvit_eval_accumulate(
        logits.data_ptr(), CODES[logits.dtype], logits.stride(0), labels.data_ptr(), logits.shape[0], C, None if other is None else other.data_ptr(),
        0 if other is None else other.stride(0), None if index is None else index.data_ptr(), rows, state.data_ptr(),
        None if confusion is None else confusion.data_ptr(), native.stream_ptr()), "qatvit_eval_accumulate")


def test_accumulation_strides_and_guard_bands(native_lib):
    B, C, G = 16, 10, 64
    logits, labels = _random(B, C, torch.float32, seed=3)
    one = _run(logits, labels, C)
    acc = qat_vit_amd.EvalAccumulator(C)
    for a, b in ((0, 5), (5, 13), (13, 16)):             # launches of 5, 8 and 3 rows
        acc.update(logits[a:b], labels[a:b])
    three = acc.result()
    assert _ints(three) == _ints(one) and three.loss_rows == one.loss_rows and torch.equal(three.confusion, one.confusion)
    assert abs(three.loss_sum - one.loss_sum) <= 1e-12 * abs(one.loss_sum)       # the same sixteen doubles in another order
    acc.reset()
    assert acc.result().total == 0 and int(acc.result().confusion.sum()) == 0
    # the [:, :C] view of a wider buffer whose pad is NaN: the pad is never read
    wide = torch.full((B, C + 3), float("nan"), device="cuda")
    wide[:, :C] = logits
    view = _run(wide[:, :C], labels, C)
    assert _ints(view) == _ints(one) and view.nonfinite_rows == 0 and torch.equal(view.confusion, one.confusion)
    assert abs(view.loss_sum - one.loss_sum) <= 1e-12 * abs(one.loss_sum)
    # state block and matrix inside sentinel-filled buffers
    big = torch.full((G + STATE_WORDS + G + C * C + G,), SENTINEL, dtype=torch.int64, device="cuda")
    state, conf = big[G:G + STATE_WORDS], big[2 * G + STATE_WORDS:2 * G + STATE_WORDS + C * C]
    state.zero_()
    conf.zero_()
    other = logits.flip(0).contiguous()
    for a, b in ((0, 5), (5, 13), (13, 16)):
        _raw(wide[a:b, :C], labels[a:b], C, state, conf, other=other[a:b])
    host = big.cpu()
    guard = torch.cat([host[:G], host[G + STATE_WORDS:2 * G + STATE_WORDS], host[2 * G + STATE_WORDS + C * C:]])
    assert bool((guard == SENTINEL).all())
    r = EvalResult(host[G:G + STATE_WORDS].clone(), host[2 * G + STATE_WORDS:2 * G + STATE_WORDS + C * C].clone().view(C, C), True)
    assert _ints(r)[:4] == _ints(one)[:4] and torch.equal(r.confusion, one.confusion) and r.other_rows_seen == B
    assert r.agree == int((logits.argmax(1) == other.argmax(1)).sum())
    # a null matrix pointer: nothing but the state block changes
    big.fill_(SENTINEL)
    state.zero_()
    _raw(logits, labels, C, state, None)
    host = big.cpu()
    assert bool((host[:G] == SENTINEL).all()) and bool((host[G + STATE_WORDS:] == SENTINEL).all())
    assert _ints(EvalResult(host[G:G + STATE_WORDS].clone()))[:4] == _ints(one)[:4]


def test_bad_labels_and_indices_are_counted_not_followed(native_lib):
    B, C, rows = 12, 10, 20
    logits, labels = _random(B, C, torch.float32, seed=5)
    g = torch.Generator().manual_seed(6)
    table = torch.randn(rows, C, generator=g).cuda()
    index = torch.randperm(rows, generator=g)[:B].cuda()
    labels[2], labels[5], labels[7] = -1, C, 2 ** 40
    index[3], index[9] = -1, rows
    r = _run(logits, labels, C, other=table, index=index)
    y_ok = (labels >= 0) & (labels < C)
    i_ok = (index >= 0) & (index < rows)
    pred = logits.argmax(1)
    opred = torch.full_like(pred, -7)
    opred[i_ok] = table[index[i_ok]].argmax(1)
    assert r.total == B and r.bad_labels == 3 and r.bad_index == 2
    assert r.correct == int((pred == labels)[y_ok].sum())
    assert torch.equal(r.confusion, _confusion(labels[y_ok], pred[y_ok], C)) and int(r.confusion.sum()) == B - 3
    assert r.nonfinite_rows == 0 and r.loss_rows == B - 3
    _close(r.loss_sum, float(TF.cross_entropy(logits[y_ok].double(), labels[y_ok], reduction="sum")), "bad labels left out")
    assert r.other_rows_seen == B - 2 and r.agree == int((pred == opred)[i_ok].sum())
    assert r.other_correct == int((opred == labels)[i_ok & y_ok].sum())
    # the same batch with every label and index in range counts every row
    labels[2], labels[5], labels[7] = 0, 1, 2
    index[3], index[9] = 0, 1
    ok = _run(logits, labels, C, other=table, index=index)
    assert (ok.total, ok.bad_labels, ok.bad_index, ok.other_rows_seen, ok.loss_rows) == (B, 0, 0, B, B)


@pytest.mark.parametrize("B,C", [(7, 10), (130, 65)])
def test_second_opinion_tensor_and_table_agree(native_lib, B, C):
    logits, labels = _random(B, C, torch.float16, seed=7)
    g = torch.Generator().manual_seed(8)
    other = (logits.float().cpu() + 2 * torch.randn(B, C, generator=g)).cuda()     # close enough to agree on some rows and differ on others
    rows = 3 * B + 5
    index = torch.randperm(rows, generator=g)[:B].cuda()
    table = (7 * torch.randn(rows, C, generator=g)).cuda()
    table[index] = other
    a = _run(logits, labels, C, other=other)
    b = _run(logits, labels, C, other=table, index=index)
    pred, opred = logits.argmax(1), other.argmax(1)
    want = (int((pred == opred).sum()), int((opred == labels).sum()))
    assert (a.agree, a.other_correct) == want == (b.agree, b.other_correct)
    assert 0 < want[0] < B
    assert a.other_rows_seen == b.other_rows_seen == B and a.agreement == 100.0 * want[0] / B
    assert _ints(a) == _ints(b) and torch.equal(a.confusion, b.confusion)
    same = _run(logits, labels, C, other=logits.float())
    assert same.agree == same.total == B and same.other_correct == same.correct and same.agreement == 100.0
    # a strided second opinion (column slice) is read in place
    wide = torch.full((B, C + 5), float("nan"), device="cuda")
    wide[:, :C] = other
    assert _ints(_run(logits, labels, C, other=wide[:, :C])) == _ints(a)
    with pytest.raises(ValueError, match="float32"):
        _run(logits, labels, C, other=other.half())
    with pytest.raises(ValueError, match="other_index given without other"):
        _run(logits, labels, C, index=index)
    with pytest.raises(ValueError, match=r"logits must be \[B"):
        _run(logits[:, :C - 1], labels, C)
    with pytest.raises(ValueError, match="labels must be"):
        _run(logits, labels.int(), C)


def evaluate_fp32(model, dataloader, device):
    """The reference's validation loop (qat_trainer.py:49-61), restated."""
    with torch.no_grad():
        model.eval()
        correct = 0
        total = 0
        for images, labels in dataloader:
            images = images.to(device, non_blocking=True)
            labels = labels.to(device, non_blocking=True)
            outputs = model(images)
            preds = outputs.argmax(dim=1)
            correct += (preds == labels).sum().item()
            total += labels.size(0)
        return 100.0 * correct / max(1, total)


def _loader(n, size, batch, seed):
    g = torch.Generator().manual_seed(seed)
    return DataLoader(TensorDataset(torch.randn(n, 3, size, size, generator=g), torch.randint(0, 10, (n,), generator=g)), batch_size=batch)


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_evaluate_equals_the_reference_loop(native_lib, backend):
    torch.manual_seed(11)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=128, depth=1, num_heads=2, img_size=32)
    m = prepare(stu.cuda(), backend)
    m.dequant.eval()                                     # a mixed pattern of flags to restore
    ref = copy.deepcopy(m)
    loader = _loader(20, 32, 8, 12)                      # CPU batches of 8, 8 and 4
    before = {n: s.training for n, s in m.named_modules()}
    assert any(before.values()) and not all(before.values())
    want = evaluate_fp32(ref, loader, torch.device("cuda"))
    r = qat_vit_amd.evaluate(m, loader)
    assert r.accuracy == want and r.total == 20 and r.correct == round(want * 20 / 100)
    assert r.bad_labels == 0 and r.loss_rows + r.nonfinite_rows == 20 and int(r.confusion.sum()) == 20 and r.agree is None
    moved = 0
    for (n, a), (_, b) in zip(fq_modules(m).items(), fq_modules(ref).items()):
        for (bn, x), (_, y) in zip(a.named_buffers(), b.named_buffers()):
            assert torch.equal(x, y), (n, bn)            # both moved their observers the same way
        moved += int(torch.isfinite(a.activation_post_process.min_val).all())
    assert moved == len(fq_modules(m)) > 0
    assert {n: s.training for n, s in m.named_modules()} == before
    assert all(p.grad is None for p in m.parameters())
    assert qat_vit_amd.evaluate(m, loader, max_batches=2).total == 16
    assert {n: s.training for n, s in m.named_modules()} == before
    empty = qat_vit_amd.evaluate(m, [])
    assert empty.total == 0 and empty.accuracy == 0.0


def test_int8_student_agrees_with_its_source_on_every_sample(native_lib):
    from torch.ao.quantization import disable_observer

    torch.manual_seed(13)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, depth=1)
    m = prepare(stu.cuda(), "qnnpack")
    loader = _loader(20, 224, 8, 14)
    qat_vit_amd.evaluate(m, loader, max_batches=1)       # the observers see data once
    m.apply(disable_observer)
    infer = qat_vit_amd.Int8Student(qat_vit_amd.export_int8(m))
    r = qat_vit_amd.evaluate(infer, loader, other=m)
    assert r.total == 20 and r.agree == r.total and r.other_rows_seen == 20 and r.other_correct == r.correct and r.agreement == 100.0
    assert m.training                                    # `other` is a module too: its flags are restored
    assert r.correct == qat_vit_amd.evaluate(m, loader).correct


def test_sixteen_bit_logits_of_the_autocast_forms(native_lib):
    torch.manual_seed(15)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, depth=1)
    m = qat_vit_amd.native_float(stu.cuda().eval(), amp=(torch.float16, torch.bfloat16))
    g = torch.Generator().manual_seed(16)
    x, y = torch.randn(12, 3, 224, 224, generator=g).cuda(), torch.randint(0, 10, (12,), generator=g).cuda()
    for dt in (torch.float16, torch.bfloat16):
        with torch.no_grad(), torch.autocast("cuda", dtype=dt):
            logits = m(x)
            assert logits.dtype == dt
            r = _run(logits, y, 10)
            via = qat_vit_amd.evaluate(m, [(x, y)])
        pred = logits.argmax(1)
        assert r.total == 12 and r.correct == int((pred == y).sum()) and torch.equal(r.confusion, _confusion(y, pred, 10))
        _close(r.loss_sum, float(TF.cross_entropy(logits.double(), y, reduction="sum")), f"autocast {dt}")
        assert _ints(via) == _ints(r) and torch.equal(via.confusion, r.confusion)


def test_teacher_table_as_second_opinion(native_lib):
    torch.manual_seed(17)
    teacher = VisionTransformer(embed_dim=768, depth=1, num_heads=12, num_classes=10)
    model = VisionTransformer(embed_dim=384, depth=1, num_heads=6, num_classes=10)
    for net in (teacher, model):
        for p in net.parameters():
            p.requires_grad = False
        net.cuda().eval()
    g = torch.Generator().manual_seed(18)
    data = torch.randint(0, 256, (40, 32, 32, 3), generator=g, dtype=torch.uint8).cuda()
    labels = torch.randint(0, 10, (40,), generator=g).cuda()
    tr = qat_vit_amd.GpuResizeNormalize(32)
    table = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16)
    loader = qat_vit_amd.GpuImageLoader(data, labels, 16, shuffle=True, transform=tr, generator=torch.Generator().manual_seed(19), return_index=True)
    r = qat_vit_amd.evaluate(model, loader, other=table)
    agree = other_correct = correct = 0
    with torch.no_grad():
        for images, y, index in loader:
            pred, tpred = model(images).argmax(1), table.rows(index).argmax(1)
            agree += int((pred == tpred).sum())
            other_correct += int((tpred == y).sum())
            correct += int((pred == y).sum())
    assert (r.total, r.other_rows_seen, r.bad_index) == (40, 40, 0)
    assert (r.agree, r.other_correct, r.correct) == (agree, other_correct, correct)
    plain = qat_vit_amd.GpuImageLoader(data, labels, 16, transform=tr)
    with pytest.raises(ValueError, match="return_index=True"):
        qat_vit_amd.evaluate(model, plain, other=table)
    with pytest.raises(ValueError, match="other_index"):
        qat_vit_amd.EvalAccumulator(10).update(torch.zeros(4, 10, device="cuda"), labels[:4], other=table)


def test_update_does_not_synchronise(native_lib):
    logits, labels = _random(64, 10, torch.float32, seed=21)
    other = logits.flip(0).contiguous()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            labels.sum().item()                          # the mode is honoured: a synchronising call raises
        acc = qat_vit_amd.EvalAccumulator(10)
        for _ in range(3):
            acc.update(logits, labels)
            acc.update(logits.half(), labels, other=other)
        acc.reset()
        acc.update(logits, labels)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert acc.result().total == 64
