"""The compressed teacher table on an MI355X (qatvit_teacher_topk_rows, qatvit_kd_ce_loss_topk, TeacherTopKTable): the selection against a stable CPU
sort and the fp64 tail; the loss bit for bit against the dense class-parallel entry on the decompressed rows, and against the fp64 restatement of
tests/mix_ref.py; guarded operands with out-of-range entries; the from_dense / save / load round trip.

Shapes: B = 5 (not a multiple of a wave-form workgroup's four rows); the class counts sit on the wave / workgroup (1000 | 1025) and register / chunk
(4097) boundaries, k on C - 1 (10, 3 is plain; 65, 64 is both k = 64 and k = C - 1).  Bars: tests/test_gpu_ce_rows.py's rule, unchanged; the tail's is
the larger of 2e-6 * max(1, |u|) and twice the error of the stock fp32 torch evaluation of the same formula, measured here and printed (-s)."""
import math

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native
from tests import mix_ref
from tests.kernel_check import guarded, guarded_copy
from tests.test_gpu_bce_loss import _case, _errors
from tests.test_gpu_ce_rows import KD, PROJECT, bench

pytestmark = pytest.mark.gpu

B, TB = 5, 4.0
CASES = [(10, 3), (65, 64), (1000, 32), (1025, 8), (4097, 64), (21841, 16)]
_tables = {}


def _bits(t):
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _table(C, k):
    """Per case, built once: the compressed form of _case's dense table (B + 5 rows) on the device, and its decompressed rows."""
    if (C, k) not in _tables:
        tab = qat_vit_amd.TeacherTopKTable.from_dense(_case(B, C)[2].cuda(), k, TB)
        _tables[(C, k)] = (tab, tab.rows(torch.arange(tab.N, device="cuda")))
    return _tables[(C, k)]


def _records(C):
    s, _, _, index, y, recs = _case(B, C)
    ones = recs.clone()
    ones[:, 5] = mix_ref.f32_bits(1.0)
    return s, index, y, {"plain": None, "lam1": ones, "mix": recs}


def _sparse(tab, s, index, y, recs):
    s = s.clone().cuda().requires_grad_(True)
    loss, parts = tab.loss(s, index.cuda(), y.cuda(), *KD, mix=None if recs is None else recs.cuda())
    loss.backward()
    return parts.detach().cpu(), s.grad.cpu()


def _dense(rows, s, index, y, recs):
    s = s.clone().cuda().requires_grad_(True)
    loss, parts = F.kd_ce_loss_table_mix(s, rows, index.cuda(), y.cuda(), None if recs is None else recs.cuda(), *KD, class_parallel=True)
    loss.backward()
    return parts.detach().cpu(), s.grad.cpu()


def _same(got, want):
    """Equal bits outside the NaNs, and NaN in the same places."""
    return all(torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(g.nan_to_num(nan=0.0), w.nan_to_num(nan=0.0)) for g, w in zip(got, want))


@pytest.mark.parametrize("C,k", CASES)
def test_selection(C, k):
    g = torch.Generator().manual_seed(7 * C + k)
    t = torch.round(12 * torch.randn(B + 2, C, generator=g)) / 4      # steps of 0.25: many ties, and -0.0 next to +0.0
    t[3] = 1.25                                                       # every value equal: the classes 0 .. k - 1
    idx, val, tail = (v.cpu() for v in F.teacher_topk(t.cuda(), k, TB))
    order = torch.sort(t, dim=1, descending=True, stable=True).indices[:, :k]
    assert torch.equal(idx.long(), order)
    assert torch.equal(_bits(val), _bits(t.gather(1, order)))
    in_tail = torch.ones_like(t, dtype=torch.bool).scatter_(1, order, False)
    m = t.max(1).values
    u64 = m.double() + TB * (torch.where(in_tail, ((t - m[:, None]).double() / TB).exp(), 0.0).sum(1).log() - math.log(C - k))
    u32 = m + TB * (torch.logsumexp(torch.where(in_tail, (t - m[:, None]) / TB, -math.inf), 1) - torch.tensor(float(C - k)).log())
    stock, err = (u32.double() - u64).abs(), (tail.double() - u64).abs()
    bar = torch.maximum(2e-6 * u64.abs().clamp(min=1.0), 2 * stock)
    print(f"C={C} k={k}: tail error {err.max():.2e}, stock fp32 torch {stock.max():.2e}, bar {bar.min():.2e}")
    assert bool((err <= bar).all()), (err, bar)
    again = F.teacher_topk(t.cuda(), k, TB)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, (idx, val, tail)))
    bad = t.clone()
    bad[1, C // 2] = float("nan")
    nidx, nval, ntail = (v.cpu() for v in F.teacher_topk(bad.cuda(), k, TB))
    keep = torch.arange(B + 2) != 1
    assert nidx[1].tolist() == list(range(k)) and bool(nval[1].isnan().all()) and bool(ntail[1].isnan())
    assert torch.equal(nidx[keep], idx[keep]) and torch.equal(_bits(nval[keep]), _bits(val[keep])) and torch.equal(_bits(ntail[keep]), _bits(tail[keep]))


@pytest.mark.parametrize("C,k", CASES)
def test_loss_equals_the_dense_entry_on_the_decompressed_rows_bit_for_bit(C, k):
    tab, rows = _table(C, k)
    s, index, y, records = _records(C)
    for name, recs in records.items():
        got, want = _sparse(tab, s, index, y, recs), _dense(rows, s, index, y, recs)
        assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name
    for at in (0, 2, 4):                                              # an index outside the table: the same NaN rows as the dense entry's
        for value in (tab.N, -1):
            bad = index.clone()
            bad[at] = value
            got, want = _sparse(tab, s, bad, y, records["mix"]), _dense(rows, s, bad, y, records["mix"])
            assert bool(got[0].isnan().all()) and bool(got[1][at].isnan().all()) and _same(got, want), (at, value)


@pytest.mark.parametrize("C,k", CASES)
def test_loss_against_the_fp64_reference(C, k):
    tab, rows = _table(C, k)
    s, index, y, records = _records(C)
    for name in ("plain", "mix"):
        r = records[name]
        s64 = s.double().requires_grad_(True)
        want = mix_ref.loss(s64, y, r, table=rows.cpu(), index=index, kd_temp=KD[0], kd_alpha=KD[1], label_smoothing=KD[2])
        want[0].backward()
        want = [float(v.detach()) for v in want]
        bars = PROJECT
        if C > 257:
            s32 = s.clone().cuda().requires_grad_(True)
            comp = bench.composition(s32, y.cuda(), None if r is None else r.cuda(), table=rows, index=index.cuda())
            comp[0].backward()
            comp = _errors(torch.stack(comp).detach().cpu(), s32.grad.cpu(), want, s64.grad)
            bars = tuple(max(p, 2 * c) for p, c in zip(PROJECT, comp))
        parts, grad = _sparse(tab, s, index, y, r)
        err = _errors(parts, grad, want, s64.grad)
        print(f"C={C} k={k} {name}: loss, ce, kd, grad", *(f"{v:.2e}" for v in err), "bars", *(f"{v:.2e}" for v in bars))
        for e, bar, what in zip(err, bars, ("loss", "ce", "kd", "gradient")):
            assert e < bar, f"C={C} k={k} {name}: {what} error {e:.3e} is not below {bar:.3e}"


@pytest.mark.parametrize("C,k", [(65, 64), (1025, 8)])
def test_guarded_operands_and_entries_outside_the_classes(C, k):
    tab, _ = _table(C, k)
    s, index, y, records = _records(C)
    idx, val = torch.cat([tab.idx, tab.idx[:1]]), torch.cat([tab.val, tab.val[:1]])     # one more row: row 0 with two entries pointing outside
    idx[-1, 1], idx[-1, k - 1], idx[-1, 2] = -1, C, idx[-1, 0]           # and entry 2 names entry 0's class again: the later value counts
    wide = qat_vit_amd.TeacherTopKTable(idx, val, torch.cat([tab.tail, tab.tail[:1]]), dict(tab.meta, N=tab.N + 1))
    index = index.clone()
    index[0] = tab.N
    rows = wide.rows(torch.arange(wide.N, device="cuda"))
    assert torch.equal(rows[-1, idx[0, [1, k - 1]].long()], tab.tail[:1].expand(2))     # the classes of the ignored entries hold the tail's logit
    assert rows[-1, idx[0, 0]] == val[0, 2] != val[0, 0] and rows[-1, idx[0, 2]] == tab.tail[0]
    want = _dense(rows, s, index, y, records["mix"])
    gi, i_check = guarded(wide.N, k, torch.float16, "cuda")
    gi.view(torch.int16).copy_(idx)
    gv, v_check = guarded_copy(val)
    gt, t_check = guarded_copy(wide.tail)
    dl, d_check = guarded_copy(torch.full((B, C), float("nan"), device="cuda"))
    pt, p_check = guarded(1, 2 * B, torch.float32, "cuda")
    out3, sg = torch.empty(3, device="cuda"), s.cuda()
    ii, yy, rr = index.cuda(), y.cuda(), records["mix"].cuda()
    native.check(native.lib().qatvit_kd_ce_loss_topk(sg.data_ptr(), gi.data_ptr(), gv.data_ptr(), gt.data_ptr(), wide.N, k, ii.data_ptr(), yy.data_ptr(),
                                                     rr.data_ptr(), B, C, *KD, pt.data_ptr(), out3.data_ptr(), dl.data_ptr(), native.stream_ptr()),
                 "qatvit_kd_ce_loss_topk")
    torch.cuda.synchronize()
    i_check("idx"), v_check("val"), t_check("tail"), d_check("dlogits"), p_check("partials")
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(pt).all())
    assert torch.equal(out3.cpu(), want[0]) and torch.equal(dl.cpu(), want[1])


@pytest.mark.parametrize("C,k", [(65, 64), (1025, 8)])
def test_from_dense_round_trip(C, k, tmp_path):
    tab, rows = _table(C, k)
    dense = _case(B, C)[2].cuda()
    assert torch.equal(_bits(rows.gather(1, tab.idx.long())), _bits(dense.gather(1, tab.idx.long()))) and torch.equal(_bits(tab.val), _bits(rows.gather(1, tab.idx.long())))
    elsewhere = torch.ones_like(rows, dtype=torch.bool).scatter_(1, tab.idx.long(), False)
    assert int(elsewhere.sum()) == tab.N * (C - k) and torch.equal(_bits(rows[elsewhere]), _bits(tab.tail[:, None].expand(-1, C)[elsewhere]))
    assert tab.nbytes == tab.N * (6 * k + 4) and (tab.k, tab.C, tab.tail_temp) == (k, C, TB)
    tab.save(str(tmp_path / "t.pt"))
    back = qat_vit_amd.TeacherTopKTable.load(str(tmp_path / "t.pt"), k=k, tail_temp=TB, C=C)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in ((back.idx, tab.idx), (back.val, tab.val), (back.tail, tab.tail)))


def test_build_compresses_chunk_by_chunk_what_from_dense_compresses_at_once():
    from qat_vit_amd.vit import VisionTransformer

    torch.manual_seed(17)
    teacher = VisionTransformer(embed_dim=768, depth=1, num_heads=12, num_classes=10)
    for p in teacher.parameters():
        p.requires_grad = False
    teacher.cuda().eval()
    data = torch.randint(0, 256, (40, 32, 32, 3), generator=torch.Generator().manual_seed(18), dtype=torch.uint8).cuda()
    tr = qat_vit_amd.GpuResizeNormalize(32)
    tab = qat_vit_amd.TeacherTopKTable.build(teacher, data, transform=tr, k=3, kd_temp=TB, batch_size=16)     # 40 = 16 + 16 + 8: a padded last chunk
    want = qat_vit_amd.TeacherTopKTable.from_dense(qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16), 3, TB)
    assert (tab.N, tab.k, tab.C, tab.nbytes) == (40, 3, 10, 40 * 22) and tab.meta == want.meta and tab.meta["k"] == 3 and tab.meta["tail_temp"] == TB
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in ((tab.idx, want.idx), (tab.val, want.val), (tab.tail, want.tail)))
    teacher.head.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="replaced or modified"):
        tab.rows(torch.arange(4, device="cuda"))
