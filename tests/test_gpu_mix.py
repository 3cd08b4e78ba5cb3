"""Mixup / cutmix inside the batch launch (qatvit_image_batch_mix through GpuResizeNormalize(mix=...) and GpuImageLoader(mix=...)) on an MI355X:
the batch EQUALS the composition include/qatvit.h states - what the existing entries give per position, mixed on the host by tests/mix_ref.py with
separate fp32 multiplies and an add, then the box overwrite - for every element."""
import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from tests import mix_ref

pytestmark = pytest.mark.gpu

B = 16
SIZES = [(32, 224), (37, 224), (96, 384)]                            # the template form, odd unaligned rows, run-time D
ARMS = [("constant", 131), ("reflect", 0), None]                     # words in both padding modes, and no words
_cache = {}


def _images(n, s, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, s, s, 3), dtype=np.uint8)


def _records(D):
    """One record per batch position; the comments name what each is there for."""
    r, mixup, cutmix = mix_ref.record, mix_ref.mixup, mix_ref.cutmix
    recs = [
        mixup(1, 0.3),                                               # 0 -> 1 -> 2 -> 0: a chain; the partner's source is X[p], never a mixed row
        mixup(2, 0.5),
        mixup(0, np.float32(0.9999)),
        mixup(4, 0.0),                                               # all partner
        cutmix(5, (0, D, 0, D), D),                                  # the whole image
        cutmix(6, (D // 2 + 1, D // 2 + 2, D // 2 - 3, D // 2 - 2), D),   # 1 x 1, in the middle: away from any padding of the two sources
        cutmix(7, (3, 29, 5, D - 3), D),                             # edges off the 4-column and 16-row grids
        cutmix(8, (14, 18, 6, 10), D),                               # across one band boundary
        cutmix(9, (D - 10, 65535, D - 7, 40000), D),                 # given beyond D: clamped
        cutmix(10, (50, 20, 10, 100), D),                            # y1 < y0: empty
        mixup(10, 0.3),                                              # partner == b
        mixup(-1, 0.3),                                              # outside [0, B): self
        cutmix(B, (30, 70, 30, 70), D),                              # outside [0, B): self
        r(3),                                                        # identity
        r(15, 0.5, 0.5, (40, 100, 1, 7), 0.5),                       # a blend and a box in one record
        r(0, 0.5, 0.0, lam=1.0),                                     # no partner needed, but the sample's weight is not 1
    ]
    assert len(recs) == B
    return torch.tensor(recs, dtype=torch.int32)


def _case(s, d):
    """Per size, built once and never changed: transform, images on the device, words, records (host)."""
    if (s, d) not in _cache:
        words = qat_vit_amd.RandomCropFlip(padding=4).draw(B, torch.Generator().manual_seed(s))
        _cache[(s, d)] = (qat_vit_amd.GpuResizeNormalize(s, out_size=d), torch.from_numpy(_images(B, s, s)).cuda(), words, _records(d))
    return _cache[(s, d)]


def _kw(arm, words):
    return {} if arm is None else {"aug": words.cuda(), "padding_mode": arm[0], "fill": arm[1]}


@pytest.mark.parametrize("arm", ARMS, ids=["constant", "reflect", "nowords"])
@pytest.mark.parametrize("s,d", SIZES)
def test_equals_the_composition(s, d, arm):
    tr, src, words, recs = _case(s, d)
    kw = _kw(arm, words)
    X = tr(src, **kw)
    want = torch.from_numpy(mix_ref.mixed_images(X.cpu().numpy(), recs))
    got = tr(src, mix=recs.cuda(), **kw)
    assert got.shape == (B, 3, d, d) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    Xc = X.cpu()
    assert torch.equal(want[4], Xc[5]) and torch.equal(want[3], Xc[4]) and torch.equal(want[9], Xc[9]) and torch.equal(want[13], Xc[13])
    assert not torch.equal(want[5], Xc[5]) and not torch.equal(want[0], Xc[0])            # the 1 x 1 box shows; the blend is one


@pytest.mark.parametrize("s,d", SIZES)
def test_identity_records_and_no_records_are_the_existing_calls(s, d):
    tr, src, words, _ = _case(s, d)
    ident = torch.tensor([mix_ref.record(B - 1 - b) for b in range(B)], dtype=torch.int32).cuda()
    for arm in ARMS:
        kw = _kw(arm, words)
        X = tr(src, **kw)
        assert torch.equal(tr(src, mix=ident, **kw), X)
        assert torch.equal(tr(src, mix=None, **kw), X)
        buf = torch.full_like(X, float("nan"))
        assert tr(src, out=buf, mix=ident, **kw) is buf and torch.equal(buf, X)
    # the C entry with mix == NULL launches the aug entry's kernels: words, and neither
    plain, w = tr(src), words.cuda()
    for aug, want in ((w, tr(src, aug=w, padding_mode="reflect")), (None, plain)):
        out = torch.full_like(plain, float("nan"))
        data.native.check(data.native.lib().qatvit_image_batch_mix(src.data_ptr(), None, B, B, s, d, tr.coeffs.data_ptr(), tr.table.data_ptr(),
                                                                   None if aug is None else aug.data_ptr(), 1, 200, None, out.data_ptr(),
                                                                   data.native.stream_ptr()), "mix")
        assert torch.equal(out, want)


@pytest.mark.parametrize("s,d", [(32, 224), (37, 224)])
def test_records_go_with_batch_positions_under_a_permuted_repeating_index(s, d):
    tr, src, words, recs = _case(s, d)
    g = torch.Generator().manual_seed(s)
    index = torch.cat([torch.randperm(B, generator=g)[:10], torch.randint(0, B, (6,), generator=g)])
    assert len(set(index.tolist())) < B
    kw = dict(aug=words.cuda(), padding_mode="constant", fill=7)
    X = tr(src, index.cuda(), **kw)
    want = torch.from_numpy(mix_ref.mixed_images(X.cpu().numpy(), recs))
    buf = torch.full((B, 3, d, d), float("nan"), device="cuda")
    assert tr(src, index.cuda(), out=buf, mix=recs.cuda(), **kw) is buf
    assert torch.equal(buf.cpu(), want)


def test_loader_draws_the_records_last_and_does_not_synchronise():
    n, bs = 40, 16
    imgs = _images(n, 32, 77)
    labels = np.random.default_rng(7).integers(0, 10, n)
    tr = _case(32, 224)[0]
    a, m = qat_vit_amd.RandomCropFlip(4), qat_vit_amd.MixupCutmix(mode="elem")
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, augment=a, mix=m, generator=torch.Generator().manual_seed(12),
                                        return_index=True, transform=tr)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            loader.labels.sum().item()                               # the mode is honoured: a synchronising call raises
        epochs = [list(loader) for _ in range(2)]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    g = torch.Generator().manual_seed(12)                            # the expectation: plan, then words, then records
    src, seen = torch.from_numpy(imgs).cuda(), []
    for got in epochs:
        plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
        words = a.draw(n, g)
        recs = m.draw([len(b) for b in plan], 224, g)
        seen.append(recs)
        assert len(got) == len(plan) == 3 and [len(b) for b in plan] == [16, 16, 8]
        o = 0
        for (x, y, idx, r), b in zip(got, plan):
            w, rb = words[o:o + len(b)], recs[o:o + len(b)]
            o += len(b)
            assert torch.equal(idx.cpu(), b) and torch.equal(y.cpu(), torch.from_numpy(labels)[b])
            assert r.dtype == torch.int32 and r.shape == (len(b), 6) and r.is_cuda and r.is_contiguous() and torch.equal(r.cpu(), rb)
            X = tr(src, idx, aug=w.cuda(), padding_mode=a.padding_mode, fill=a.fill)
            assert torch.equal(x.cpu(), torch.from_numpy(mix_ref.mixed_images(X.cpu().numpy(), rb)))
    assert not torch.equal(seen[0], seen[1])                         # the second epoch draws new records
    # the tuple forms: the records are the last element, with and without the index and the words
    for ret, aug, length in ((False, a, 3), (True, None, 4), (False, None, 3)):
        gen = torch.Generator().manual_seed(3)
        first = next(iter(qat_vit_amd.GpuImageLoader(imgs, labels, bs, augment=aug, mix=m, generator=gen, transform=tr, return_index=ret)))
        assert len(first) == length and first[0].shape == (16, 3, 224, 224) and first[-1].shape == (16, 6) and first[-1].dtype == torch.int32
        want = m.draw([16, 16, 8], 224, torch.Generator().manual_seed(3)) if aug is None else None
        assert want is None or torch.equal(first[-1].cpu(), want[:16])   # nothing but the records was drawn: a sequential plan, no words
    # existing seeds give existing words and plans: the records are drawn behind them
    old = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, augment=a, generator=torch.Generator().manual_seed(12), return_index=True,
                                     transform=tr)
    for (x, y, idx), (_, y2, idx2, _) in zip(list(old), epochs[0]):
        assert torch.equal(idx, idx2) and torch.equal(y, y2)


def test_refusals():
    tr, src, words, recs = _case(32, 224)
    r = recs.cuda()
    for bad in (r.long(), r[:5], recs, r[:, :5], torch.zeros(B, 12, dtype=torch.int32, device="cuda")[:, ::2], r.flatten()):
        with pytest.raises(ValueError, match="mix must be"):
            tr(src, mix=bad)
    with pytest.raises(ValueError, match="aug must be"):
        tr(src, aug=words, mix=r)
    with pytest.raises(TypeError, match="MixupCutmix"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 32, 32, 3), np.uint8), np.zeros(4, np.int64), 2, transform=tr, mix="mixup")
