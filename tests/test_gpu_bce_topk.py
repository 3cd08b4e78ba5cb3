"""qatvit_kd_bce_loss_topk (F.kd_bce_loss_topk, TeacherTopKTable.bce_loss, F.kd_bce_loss above 4096 classes) on an MI355X against tests/bce_ref.py
in fp64 on the rows decompressed by the header's rule, with dlogits from autograd.

Shapes: B is never a multiple of a wave-form workgroup's four rows; C sits on every form's boundary (65: past one value per lane, k = C - 1; 1025: the
first workgroup form; 4097: the first that re-reads the row) and at the top.  Bars: profiles/bce_topk_errors.txt (tools/bench_bce_topk.py --errors)
records what the entries that existed before this one miss the same reference by on these very cases - F.kd_bce_loss on the dense decompressed table
to 4096 classes, F.kd_ce_loss_topk's KD number and gradient above - and WORST holds the worst of each class range; the new entry must stay within
FACTOR times that (another summation order of zq, log Q once per row instead of per element).  No bar comes from the entry under test."""
import math

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native
from tests import bce_ref, mix_ref

pytestmark = pytest.mark.gpu

T, ALPHA, EPS = 4.0, 0.5, 0.1
SHAPES = [(5, 2, 1), (6, 65, 64), (5, 1000, 32), (3, 1025, 16), (3, 4097, 64), (3, 21841, 32), (2, 32768, 64)]
CONFIGS = [(False, False, None, False), (False, True, 0.2, True), (True, False, None, True), (True, False, 0.2, False), (True, True, None, False),
           (True, True, 0.2, True)]                                   # table, mix records, target_threshold, sum_classes
WORST = {False: (2.206e-07, 2.252e-07), True: (5.341e-07, 4.613e-07)}  # C > 4096 -> (out3, dlogits): the two `worst` lines of profiles/bce_topk_errors.txt
FACTOR = 4
_cases = {}


def decompress(idx, val, tail, C):
    """The header's rule: the tail everywhere, then the entries in order (the later of two counts); an entry outside [0, C) is ignored."""
    dense, idx = tail[:, None].repeat(1, C), idx.long()               # (an int16 tensor cannot be compared with C = 32768)
    for e in range(idx.shape[1]):
        ok = (idx[:, e] >= 0) & (idx[:, e] < C)
        dense[ok.nonzero().flatten(), idx[ok, e]] = val[ok, e]
    return dense


def case(B, C, k):
    """Per shape, built once on the host and never changed: student, the compressed table (B + 3 rows) and its decompression, index, labels, records.
    Row b's teacher is raised on k classes that half overlap those of row b ^ 1 and (where 3 k <= C) miss those of every other row.  The records: an
    overlapping partner, a disjoint one, one outside [0, B), lam == 1, and two more.  With k >= 3 the last sample's row is hand-made: entry 1 repeats
    entry 0's class (entry 1 counts), entry 2 points past the classes (int16 allows), and with k >= 4 entry 3 before them."""
    if (B, C, k) not in _cases:
        g = torch.Generator().manual_seed(1000 * B + C + k)
        s, logits = 3 * torch.randn(B, C, generator=g), 5 * torch.randn(B + 3, C, generator=g)
        index, y, perm = torch.randperm(B + 3, generator=g)[:B], torch.randint(0, C, (B,), generator=g), torch.randperm(C, generator=g)
        for b in range(B):
            logits[index[b], perm[(torch.arange(k) + (b // 2) * 2 * k + (b % 2) * (k // 2)) % C]] += 25.0
        val, idx = logits.topk(k, 1)
        rest = torch.ones_like(logits, dtype=torch.bool).scatter_(1, idx, False)
        tail = val[:, 0] + T * torch.log(torch.where(rest, ((logits - val[:, :1]) / T).exp(), 0.0).sum(1) / (C - k))
        idx = idx.to(torch.int16)
        if k >= 3:
            idx[index[B - 1], 1], idx[index[B - 1], 2] = idx[index[B - 1], 0], C if C < 32768 else -2   # (int16 ends at 32767)
        if k >= 4:
            idx[index[B - 1], 3] = -1
        recs = [mix_ref.mixup(*r) for r in ((1 % B, 0.3), (2 % B, 0.6), (B, 0.25), (0, 1.0), (2, 0.75), (5, 0.5))[:B]]
        _cases[(B, C, k)] = (s, (idx, val.contiguous(), tail), decompress(idx, val, tail, C), index, y, torch.tensor(recs, dtype=torch.int32))
    return _cases[(B, C, k)]


def want(c, table, mix, thr, sc):
    """(out3, dlogits) of the fp64 reference."""
    s, _, dense, index, y, recs = c
    s64 = s.double().requires_grad_(True)
    out = bce_ref.loss(s64, y, recs if mix else None, kd_temp=T, kd_alpha=ALPHA, label_smoothing=EPS, target_threshold=thr, sum_classes=sc,
                       **({"table": dense, "index": index} if table else {}))
    out[0].backward()
    return [float(v.detach()) for v in out], s64.grad


def errors(parts, grad, ref):
    """(the largest relative error of out3 - a zero must be met exactly -, the largest over the rows of max |dlogits - ref| / max |ref|)."""
    rel = [abs(float(p) - w) / abs(w) if w else (0.0 if float(p) == 0.0 else math.inf) for p, w in zip(parts, ref[0])]
    return max(rel), float(((grad.double() - ref[1]).abs().amax(1) / ref[1].abs().amax(1)).max())


def run(c, table, mix, thr=None, sc=False, index=None, recs=None):
    s, tab, _, index0, y, recs0 = c
    s = s.clone().cuda().requires_grad_(True)
    kw = dict(zip(("idx", "val", "tail"), (v.cuda() for v in tab)), index=(index0 if index is None else index).cuda()) if table else {}
    loss, parts = F.kd_bce_loss_topk(s, y.cuda(), mix=(recs0 if recs is None else recs).cuda() if mix else None, kd_temp=T, kd_alpha=ALPHA,
                                     label_smoothing=EPS, target_threshold=thr, sum_classes=sc, **kw)
    loss.backward()
    assert torch.equal(loss.detach(), parts[0])
    return parts.detach().cpu(), s.grad.cpu()


@pytest.mark.parametrize("table,mix,thr,sc", CONFIGS)
@pytest.mark.parametrize("B,C,k", SHAPES)
def test_against_the_fp64_reference(B, C, k, table, mix, thr, sc):
    c = case(B, C, k)
    if (B, C, k) == (5, 1000, 32):                                   # the records meet what they are meant to meet
        sets = [set(c[1][0][i].tolist()) for i in c[3]]
        assert sets[0] & sets[1] and not sets[1] & sets[2]
    parts, grad = run(c, table, mix, thr, sc)
    e_out, e_grad = errors(parts, grad, want(c, table, mix, thr, sc))
    print(f"B={B} C={C} k={k} table={table} mix={mix} thr={thr} sum_classes={sc}: out3 {e_out:.2e} dlogits {e_grad:.2e}; recorded worst {WORST[C > 4096]}")
    assert bool(torch.isfinite(parts).all()) and bool(torch.isfinite(grad).all())
    assert e_out <= FACTOR * WORST[C > 4096][0] and e_grad <= FACTOR * WORST[C > 4096][1]


@pytest.mark.parametrize("B,C,k", [(5, 1000, 32), (3, 4097, 64)])
def test_nan_row_and_equal_bits(B, C, k):
    c = case(B, C, k)
    ok = run(c, True, False)
    bad = c[3].clone()
    bad[1] = B + 3                                                   # one index outside the table: its row and out3, nothing else
    parts, grad = run(c, True, False, index=bad)
    keep = torch.arange(B) != 1
    assert bool(parts.isnan().all()) and bool(grad[1].isnan().all()) and torch.equal(grad[keep], ok[1][keep]) and bool(torch.isfinite(ok[1]).all())
    for mix in (False, True):                                        # two calls on the same inputs
        a, b = run(c, True, mix, 0.2, True), run(c, True, mix, 0.2, True)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    ones = c[5].clone()
    ones[:, 5] = mix_ref.f32_bits(1.0)                               # partners as they are; only lam counts
    a = run(c, True, True, recs=ones)
    assert torch.equal(a[0], ok[0]) and torch.equal(a[1], ok[1])


@pytest.mark.parametrize("B,C,k", [(6, 65, 64), (3, 1025, 16), (3, 4097, 64)])
def test_dlogits_inside_a_poisoned_buffer(B, C, k):
    c = case(B, C, k)
    ref, G = run(c, True, True), 67
    buf = torch.full((G + B * C + G,), 0x7fc12345, dtype=torch.int32).view(torch.float32).cuda()        # a NaN with a payload of its own
    before = buf.clone().view(torch.int32)
    s, (idx, val, tail), index, y, recs = c[0].cuda(), (v.cuda() for v in c[1]), c[3].cuda(), c[4].cuda(), c[5].cuda()
    out3, partials = torch.empty(3, device="cuda"), torch.empty(2 * B, device="cuda")
    native.check(native.lib().qatvit_kd_bce_loss_topk(s.data_ptr(), idx.data_ptr(), val.data_ptr(), tail.data_ptr(), B + 3, k, index.data_ptr(), y.data_ptr(),
                                                      recs.data_ptr(), B, C, T, ALPHA, EPS, -1.0, 0, partials.data_ptr(), out3.data_ptr(),
                                                      buf.data_ptr() + 4 * G, native.stream_ptr()), "qatvit_kd_bce_loss_topk")
    after = buf.view(torch.int32)
    assert torch.equal(after[:G], before[:G]) and torch.equal(after[G + B * C:], before[G + B * C:])
    assert torch.equal(out3.cpu(), ref[0]) and torch.equal(buf[G:G + B * C].view(B, C).cpu(), ref[1])


def test_the_public_routes_above_4096_classes():
    c = case(3, 4097, 64)
    s, y, recs = c[0].cuda(), c[4].cuda(), c[5].cuda()
    loss, parts = F.kd_bce_loss(s, y, mix=recs, label_smoothing=EPS, target_threshold=0.2, sum_classes=True)   # the parent refuses C = 4097
    assert torch.equal(parts.cpu(), run(c, False, True, 0.2, True)[0]) and float(parts[2]) == 0.0
    assert torch.equal(qat_vit_amd.BinaryCrossEntropy(EPS, 0.2, True)(s, y, mix=recs), loss)
    meta = {"format": 101, "N": 6, "C": 4097, "teacher_form": 0, "transform": (), "data_digest": "", "param_digest": "", "k": 64, "tail_temp": T}
    tab = qat_vit_amd.TeacherTopKTable(*(v.cuda() for v in c[1]), meta)
    assert torch.equal(tab.bce_loss(s, c[3].cuda(), y, T, ALPHA, EPS, mix=recs)[1].cpu(), run(c, True, True)[0])
