"""Validation at many classes on an MI355X (qatvit_eval_accumulate_rank; EvalAccumulator / evaluate with topk, label_smoothing, per_class; DESIGN.md
section 7zc): the label's rank from its definition on the widened stored values, the smoothed loss against fp64, ties and specials row by row,
the older entry as a control, accumulation over launches, the second opinion in both forms - each launch inside sentinel guard bands."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.evaluate import RANK_BINS, RANK_STATE_WORDS as W

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
CLASSES = [2, 5, 64, 65, 256, 257, 1000, 1024, 1025, 4096, 4097, 8193, 32768]   # every edge of a kernel form, of the register-held row, of a chunk
LOSS_RTOL = 1e-5        # tests/test_gpu_eval.py's bound for the same fp32 exp / log arithmetic per row
SENTINEL, G = 0x5A5A5A5A5A5A5A5A, 64
NAN, INF = float("nan"), float("inf")
_hist = lambda ranks: torch.bincount(ranks.clamp(max=RANK_BINS - 1), minlength=RANK_BINS)   # noqa: E731


def _launch(batches, C, eps=0.0):
    """The C entry on each (logits, labels, other, index) into one state block and one [2, C] block between guard bands -> words, loss sum, counts."""
    big = torch.full((G + W + G + 2 * C + G,), SENTINEL, dtype=torch.int64, device="cuda")
    state, counts = big[G:G + W], big[2 * G + W:2 * G + W + 2 * C]
    state.zero_()
    counts.zero_()
    for x, y, other, index in batches:
        native.check(native.lib().qatvit_eval_accumulate_rank(
            x.data_ptr(), CODES[x.dtype], x.stride(0), y.data_ptr(), x.shape[0], C, eps, None if other is None else other.data_ptr(),
            0 if other is None else other.stride(0), None if index is None else index.data_ptr(), 0 if index is None else other.shape[0],
            state.data_ptr(), counts.data_ptr(), native.stream_ptr()), "qatvit_eval_accumulate_rank")
    host = big.cpu()
    assert bool((torch.cat([host[:G], host[G + W:2 * G + W], host[2 * G + W + 2 * C:]]) == SENTINEL).all()), "a word outside the two blocks was written"
    s = host[G:G + W].clone()
    return s, float(s[8:9].view(torch.float64)[0]), host[2 * G + W:2 * G + W + 2 * C].clone().view(2, C)


def _ranks(x, y):
    """The definition, on fp32 CPU values and valid labels: columns that are larger, or equal at a lower index; NaN above every number."""
    idx, y, xl = torch.arange(x.shape[1]), y[:, None], x.gather(1, y[:, None])
    number_beats = (x > xl) | ((x == xl) & (idx < y))
    return torch.where(xl.isnan(), x.isnan() & (idx < y), x.isnan() | number_beats).sum(1)


def _close(got, want, what):
    err = abs(got - want) / max(abs(want), 1e-300)
    print(f"{what}: loss sum {got!r} against {want!r}, relative error {err:.2e} (bound {LOSS_RTOL:.0e})")
    assert err <= LOSS_RTOL, (what, got, want, err)


@functools.lru_cache(maxsize=None)
def _random(B, C, dtype, pad=0):
    """Logits (on the GPU, in a [B, C + pad] buffer whose pad is NaN), labels with one below and one above the range, and the CPU reference."""
    g = torch.Generator().manual_seed(1000 * B + C)
    x, y = 3 * torch.randn(B, C, generator=g), torch.randint(0, C, (B,), generator=g)
    odd = torch.arange(1, B, 2)                                      # every other label is lifted from the tail of its row up to its top: low and
    x[odd, y[odd]] += torch.linspace(0, 14, len(odd))                # clamped ranks; the plain rows keep the loss sum, and its relative bound, of order B
    x = x.to(dtype)
    y[1], y[2] = C, -1
    ok = (y >= 0) & (y < C)
    ranks = _ranks(x.float()[ok], y[ok])
    want = dict(hist=_hist(ranks), counts=torch.stack([torch.bincount(y[ok], minlength=C), torch.bincount(y[ok][ranks == 0], minlength=C)]),
                loss={eps: float(TF.cross_entropy(x.double()[ok], y[ok], label_smoothing=eps, reduction="sum")) for eps in (0.0, 0.1)})
    wide = torch.full((B, C + pad), NAN, dtype=dtype)
    wide[:, :C] = x
    return wide.cuda()[:, :C], y.cuda(), want


@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("B,pad", [(7, 0), (33, 0), (33, 3)])
@pytest.mark.parametrize("C", CLASSES)
def test_random_rows_equal_the_definition(native_lib, C, B, pad, dtype):
    x, y, want = _random(B, C, dtype, pad)
    for eps in (0.0, 0.1):
        s, loss, counts = _launch([(x, y, None, None)], C, eps)
        assert torch.equal(s[10:10 + RANK_BINS], want["hist"]) and torch.equal(counts, want["counts"])
        assert s[:8].tolist() == [B, 2, 0, B - 2, 0, 0, 0, 0] and s[9] == 0 and int(s[42:].sum()) == 0
        _close(loss, want["loss"][eps], f"B={B} C={C} {dtype} eps={eps}")


@pytest.mark.parametrize("C,dtype", [(5, torch.float16), (1000, torch.float16), (5, torch.float32), (65, torch.float32), (1000, torch.float32),
                                     (4097, torch.float32), (32768, torch.float32)])
def test_tie_free_rows_equal_torch_topk(native_lib, C, dtype):
    B, g = 33, torch.Generator().manual_seed(C)
    x = torch.stack([torch.randperm(C, generator=g) for _ in range(B)]).sub(C // 2).mul(0.5 if C <= 2048 else 0.01).to(dtype)   # distinct in every row
    y = torch.stack([torch.randperm(C, generator=g)[0] for _ in range(B)])
    y[::2] = x[::2].float().topk(min(C, 8)).indices[torch.arange((B + 1) // 2), torch.arange((B + 1) // 2) % min(C, 8)]   # half the labels near the top
    s, _, _ = _launch([(x.cuda(), y.cuda(), None, None)], C)
    for k in (1, 5, 31):
        assert int(s[10:10 + k].sum()) == int((x.float().topk(min(k, C)).indices == y[:, None]).any(1).sum()), k


def _specials(C):
    """(row, label, rank, finite loss with eps = 0, with eps = 0.1); a label outside [0, C) has rank None.  Columns not named hold `fill`."""
    def row(fill=-5.0, **cols):
        r = torch.full((C,), fill)
        for c, v in cols.items():
            r[int(c[1:])] = v
        return r
    above = {n: row(c35=1.0, **{f"c{c}": 3.0 for c in range(n)}) for n in (30, 31, 32)}
    return [(row(c3=2.0, c7=2.0), 7, 1, True, True), (row(c3=2.0, c7=2.0), 3, 0, True, True),            # tied with a lower / a higher index
            (row(c2=0.0, c5=-0.0), 5, 1, True, True), (row(c2=0.0, c5=-0.0), 2, 0, True, True),          # +0 == -0
            (row(c1=NAN, c4=9.0), 4, 1, False, False), (row(c4=9.0, c9=NAN), 4, 1, False, False),        # NaN before / after the label
            (row(c0=100.0, c1=NAN, c4=NAN, c9=NAN), 4, 1, False, False),                                  # NaN at the label: only the earlier NaN beats it
            (row(c4=INF), 4, 0, False, False), (row(c4=1.0, c6=INF), 4, 1, False, False), (row(fill=-INF), 4, 4, False, False),
            (row(c4=1.0, c6=-INF), 4, 0, True, False),                                                    # -inf off the label: non-finite only when smoothed
            (above[30], 35, 30, True, True), (above[31], 35, 31, True, True), (above[32], 35, 32, True, True),   # around the clamp bin
            (row(), -1, None, None, None), (row(), C, None, None, None)]


@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("C", [40, 1500, 5000, 9000])
def test_ties_and_specials_row_by_row(native_lib, C, dtype):
    for n, (row, label, rank, finite0, finite1) in enumerate(_specials(C)):
        x, y = row.to(dtype)[None], torch.tensor([label])
        for eps, finite in ((0.0, finite0), (0.1, finite1)):
            s, loss, counts = _launch([(x.cuda(), y.cuda(), None, None)], C, eps)
            if rank is None:
                assert s[:4].tolist() == [1, 1, 0, 0] and int(s[10:].sum()) == 0 and int(counts.sum()) == 0, n
                continue
            want = TF.cross_entropy(x.double(), y, label_smoothing=eps, reduction="sum")
            assert _ranks(x.float(), y).item() == rank and bool(want.isfinite()) == finite, n       # the table agrees with the definition and with torch's loss
            assert torch.equal(s[10:10 + RANK_BINS], _hist(torch.tensor([rank]))), (n, eps, s[10:42].tolist())
            assert s[:4].tolist() == [1, 0, int(not finite), int(finite)] and counts[:, label].tolist() == [1, int(rank == 0)], (n, eps)
            if finite:
                _close(loss, float(want), f"special row {n} C={C} {dtype} eps={eps}")


@pytest.mark.parametrize("C", [65, 1025, 4097])
def test_older_entry_accumulation_and_second_opinion(native_lib, C):
    B = 33
    x, y, want = _random(B, C, torch.float16)
    g = torch.Generator().manual_seed(C)
    other = (x.float().cpu() + 2 * torch.randn(B, C, generator=g)).cuda()     # agrees with x on some rows
    table, index = (7 * torch.randn(3 * B, C, generator=g)).cuda(), torch.randperm(3 * B, generator=g)[:B].cuda()
    table[index] = other
    index[5] = 3 * B                                                          # one row of the table cannot be read
    ok = ((y >= 0) & (y < C)).cpu()
    seen = ok & (torch.arange(B) != 5)
    one, loss, counts = _launch([(x, y, table, index)], C)
    three, loss3, counts3 = _launch([(x[a:b], y[a:b], table, index[a:b]) for a, b in ((0, 11), (11, 22), (22, 33))], C)
    assert torch.equal(one[:8], three[:8]) and torch.equal(one[10:], three[10:]) and torch.equal(counts, counts3) and torch.equal(counts, want["counts"])
    assert abs(loss - loss3) <= 1e-12 * abs(loss)                             # the same doubles in another order
    assert torch.equal(one[42:], _hist(_ranks(other.cpu()[seen], y.cpu()[seen]))) and torch.equal(one[10:42], want["hist"])
    tensor, _, _ = _launch([(x, y, other, None)], C)
    assert torch.equal(tensor[42:], _hist(_ranks(other.cpu()[ok], y.cpu()[ok]))) and tensor[4:7].tolist() == [B, int((x.argmax(1) == other.argmax(1)).sum()), 0]
    acc = qat_vit_amd.EvalAccumulator(C, confusion=False)                     # the older entry on the same batch
    acc.update(x, y, table, index)
    old = acc.result()
    assert (int(one[10]), int(one[5]), int(one[4]), int(one[6]), int(one[42])) == (old.correct, old.agree, old.other_rows_seen, old.bad_index, old.other_correct)
    assert (old.other_rows_seen, old.bad_index) == (B - 1, 1) and one[:4].tolist() == [old.total, old.bad_labels, old.nonfinite_rows, old.loss_rows]
    _close(loss, old.loss_sum, f"C={C}: eps = 0 against the older entry")


def test_through_the_wrapper(native_lib):
    B, C = 33, 1000
    x, y, want = _random(B, C, torch.bfloat16)
    hist, counts = want["hist"], want["counts"]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc = qat_vit_amd.EvalAccumulator(C, topk=(1, 5), label_smoothing=0.1, per_class=True, confusion=False)
        for _ in range(2):
            acc.update(x, y)
            acc.update(x, y, other=x.float())
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    r = acc.result()
    assert torch.equal(r.rank_hist, 4 * hist) and torch.equal(r.other_rank_hist, 2 * hist) and torch.equal(r.class_counts, 4 * counts)
    assert r.topk_accuracy == {k: 100.0 * int(hist[:k].sum()) / (B - 2) for k in (1, 5)} == r.other_topk_accuracy
    assert (r.total, r.correct, r.bad_labels, r.agree, r.other_correct, r.confusion) == (4 * B, 4 * int(hist[0]), 8, 2 * B, 2 * int(hist[0]), None)
    assert abs(r.smoothed_loss - want["loss"][0.1] / (B - 2)) <= LOSS_RTOL * r.smoothed_loss and r.loss != r.loss
    seen = counts[0] > 0
    assert torch.equal(r.per_class_recall[seen], 100.0 * counts[1][seen].double() / counts[0][seen]) and bool(r.per_class_recall[~seen].isnan().all())
    both = qat_vit_amd.EvalAccumulator(C, topk=(5,))                          # the default: the older entry and its matrix as well
    both.update(x, y)
    assert int(both.result().confusion.sum()) == B - 2 and both.result().correct == int(hist[0]) == int(both.result().rank_hist[0])


def test_evaluate_top5_equals_the_torch_loop(native_lib):
    torch.manual_seed(3)
    model = qat_vit_amd.create_student("vit", num_classes=1000, embed_dim=128, depth=2, num_heads=2, img_size=32).cuda()
    images = torch.randn(40, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        logits = model.eval()(images.cuda()).cpu()
    assert all(row.unique().numel() == 1000 for row in logits)                # tie-free: torch.topk's order is then the only one
    labels = logits.topk(9).indices[torch.arange(40), torch.arange(40) % 9]   # ranks 0 .. 8
    loader = [(images[a:a + 16], labels[a:a + 16]) for a in (0, 16, 32)]
    hits = {k: sum(int((model(xb.cuda()).topk(k).indices.cpu() == yb[:, None]).any(1).sum()) for xb, yb in loader) for k in (1, 5)}
    r = qat_vit_amd.evaluate(model.train(), loader, topk=(1, 5), confusion=False)
    assert r.topk_accuracy == {k: 100.0 * hits[k] / 40 for k in (1, 5)} and hits[1] < hits[5] < 40 and r.total == 40 and model.training
