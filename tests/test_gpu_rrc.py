"""The resized crop inside the batch launch (qatvit_image_batch_rrc through GpuResizeNormalize(rrc=...) and GpuImageLoader(crop=...)) on an MI355X:
the batch EQUALS ToTensor() + Normalize() of the bytes that tests/rrc_ref.py forms on the host by crop, mirror and the two-pass resample with one
table per axis, for every element; the stored Pillow answers of tests/golden/rrc_kat.npz; and, with mix records, the composition of
include/qatvit.h (tests/mix_ref.py) applied to the rrc batch."""
import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from tests import augment_ref, mix_ref, rrc_ref
from tests.rrc_ref import host_rrc, pack
from tests.test_gpu_data import _normalized
from tests.test_gpu_mix import _records as _mix_records

pytestmark = pytest.mark.gpu

SIZES = [(32, 224), (8, 224), (37, 224), (96, 384)]                  # the template form, the smallest S, odd unaligned rows, run-time D
B = 16                                                               # the batch of the mix records of tests/test_gpu_mix.py
_cache = {}


def _images(n, s, seed):
    """n uint8 [s, s, 3] images, three kinds in turn: uniform noise, 0 / 255 noise (both passes clip), clipped gaussian."""
    rng = np.random.default_rng(seed)
    kinds = (lambda: rng.integers(0, 256, (s, s, 3), dtype=np.uint8), lambda: (rng.integers(0, 2, (s, s, 3)) * 255).astype(np.uint8),
             lambda: np.clip(rng.normal(128, 60, (s, s, 3)), 0, 255).astype(np.uint8))
    return np.stack([kinds[i % 3]() for i in range(n)])


def corner_records(S):
    """21 records: h and w each from {1, 2, 3, 4, 5, S - 1, S}, every value three times on either axis, the window in the four corners
    (top and left at 0 and at their maximum) and both flip values in turn."""
    vals = (1, 2, 3, 4, 5, S - 1, S)
    out = []
    for j in (0, 2, 5):
        for i, h in enumerate(vals):
            w, k = vals[(i + j) % 7], len(out)
            out.append(pack((S - h) * (k & 1), (S - w) * (k >> 1 & 1), h, w, bool(k >> 2 & 1)))
    return out


def _case(s, d):
    """Per size, built once and never changed: transform, images (host, device), 37 records (host, device), the expected batch."""
    if (s, d) not in _cache:
        drawn = qat_vit_amd.RandomResizedCrop().draw(16, s, torch.Generator().manual_seed(s))
        recs = torch.cat([torch.tensor(corner_records(s), dtype=torch.int32), drawn])
        imgs = _images(len(recs), s, s)
        want = _normalized(host_rrc(imgs, recs, d))
        _cache[(s, d)] = (qat_vit_amd.GpuResizeNormalize(s, out_size=d), imgs, torch.from_numpy(imgs).cuda(), recs, recs.cuda(), want)
    return _cache[(s, d)]


@pytest.mark.parametrize("s,d", SIZES)
def test_equals_the_host_resized_crop(s, d):
    tr, imgs, src, recs, r, want = _case(s, d)
    corners = [rrc_ref.unpack(v) for v in recs[:21].tolist()]
    assert len(recs) == 37 and len({c[2:4] for c in corners}) == 21
    for axis in (0, 1):                                              # offsets at 0 and at their maximum S - side, on both axes
        assert any(c[axis] == 0 and c[2 + axis] < s for c in corners) and any(c[axis] == s - c[2 + axis] > 0 for c in corners)
    assert {c[4] for c in corners} == {False, True}
    got = tr(src, rrc=r)
    assert got.shape == (37, 3, d, d) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    assert tr.windows.shape == (s, 6 * d) and tr.windows.is_cuda and tr.window_tables() is tr.windows       # built once, kept on the device


def test_equals_pillows_stored_bytes_through_the_value_table():
    images, groups = rrc_ref.load()
    src, table = torch.from_numpy(images).cuda(), data.value_table()
    for d, records, image_of, pillow in groups:
        tr = _case(32, 224)[0] if d == 224 else qat_vit_amd.GpuResizeNormalize(32, out_size=d)
        got = tr(src, torch.from_numpy(image_of).cuda(), rrc=torch.from_numpy(records).cuda())
        bytes_ = torch.from_numpy(pillow).long()
        want = torch.stack([table[c][bytes_[..., c]] for c in range(3)], 1)
        assert torch.equal(got.cpu(), want), d


@pytest.mark.parametrize("s,d", SIZES)
def test_whole_image_records_are_the_plain_and_the_flipped_call(s, d):
    tr, imgs, src, _, _, _ = _case(s, d)
    n = len(imgs)
    whole = torch.tensor([pack(0, 0, s, s, False)] * n, dtype=torch.int32).cuda()
    assert torch.equal(tr(src, rrc=whole), tr(src))
    mirrored = torch.tensor([pack(0, 0, s, s, True)] * n, dtype=torch.int32).cuda()
    words = torch.tensor([augment_ref.pack(0, 0, True)] * n, dtype=torch.int32).cuda()
    assert torch.equal(tr(src, rrc=mirrored), tr(src, aug=words))


@pytest.mark.parametrize("s,d", [(32, 224), (37, 224)])
def test_record_b_goes_with_batch_position_b_and_image_index_b(s, d):
    tr, imgs, src, recs, _, _ = _case(s, d)
    g = torch.Generator().manual_seed(s)
    index = torch.cat([torch.randperm(37, generator=g)[:20], torch.randint(0, 37, (20,), generator=g)])      # permuted, then repeating
    assert len(set(index.tolist())) < 40
    br = torch.cat([recs, recs[:3].flip(0)])                                                             # 40 records, by position
    want = _normalized(host_rrc(imgs[index.numpy()], br, d))
    got = tr(src, index.cuda(), rrc=br.cuda())
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(got, tr(src, index.cuda(), rrc=br.flip(0).contiguous().cuda()))
    buf = torch.full((40, 3, d, d), float("nan"), device="cuda")     # a preallocated out= is filled completely
    assert tr(src, index.cuda(), out=buf, rrc=br.cuda()) is buf and torch.equal(buf.cpu(), want)


@pytest.mark.parametrize("s,d", SIZES)
def test_a_malformed_record_gives_the_clamped_records_result(s, d):
    tr, imgs, src, recs, _, _ = _case(s, d)
    good = recs[21].tolist()
    bad = [good,
           [0, 0],                                                   # zero sizes
           pack(1, 2, 0, 3, True),
           pack(0, 0, s + 5, 0x7fff, False),                         # sizes above S
           pack(3, 1, 0x7fff, 2, True),
           pack(0xffff, s, 3, 4, False),                             # offsets beyond the edge
           pack(s - 2, 0xffff, 3, s - 1, True),
           [-1, -1],                                                 # all bits set
           [-(1 << 31), -(1 << 31)],                                 # bit 31 of word 1 alone: ignored
           good]
    fixed = [rrc_ref.clamped(r, s) for r in bad]
    assert fixed[0] == good and fixed[1] == pack(0, 0, 1, 1, False) and fixed[7] == pack(0, 0, s, s, True) and fixed[5] == pack(s - 3, s - 4, 3, 4, False)
    sub = src[:len(bad)].contiguous()
    got = tr(sub, rrc=torch.tensor(bad, dtype=torch.int32).cuda())
    assert torch.equal(got.cpu(), _normalized(host_rrc(imgs[:len(bad)], fixed, d)))
    assert torch.equal(got, tr(sub, rrc=torch.tensor(fixed, dtype=torch.int32).cuda()))
    alone = tr(sub, rrc=torch.tensor([good] * len(bad), dtype=torch.int32).cuda())
    assert torch.equal(got[0], alone[0]) and torch.equal(got[-1], alone[-1])                     # the neighbours are unaffected


def _mix_case(s, d):
    """16 records whose partners (tests/test_gpu_mix.py: 0 -> 1 -> 2 -> 0, 3 -> 4, 4 -> 5 .. 9 -> 10, 14 -> 15, ...) differ from them in both h
    and w; position 1, the partner of position 0, is a 1 x 1 window."""
    sides = [(s, s), (1, 1), (s - 1, 3), (2, s), (5, s - 1), (3, 4), (s, 1), (4, 2), (1, s), (s - 1, 5), (3, s), (s, 2), (2, 3), (5, 5), (4, s - 1),
             (s - 1, 1)]
    rng = np.random.default_rng(s)
    recs = [pack(int(rng.integers(0, s - h + 1)), int(rng.integers(0, s - w + 1)), h, w, bool(k & 1)) for k, (h, w) in enumerate(sides)]
    return torch.tensor(recs, dtype=torch.int32)


@pytest.mark.parametrize("s,d", SIZES)
def test_mix_equals_the_composition_of_the_rrc_batch(s, d):
    tr, imgs, src, _, _, _ = _case(s, d)
    sub, r, recs = src[:B].contiguous(), _mix_case(s, d), _mix_records(d)
    X = tr(sub, rrc=r.cuda())
    assert torch.equal(X.cpu(), _normalized(host_rrc(imgs[:B], r, d)))
    assert torch.equal(tr(sub, rrc=r.cuda(), mix=None), X)
    want = torch.from_numpy(mix_ref.mixed_images(X.cpu().numpy(), recs))
    got = tr(sub, rrc=r.cuda(), mix=recs.cuda())
    assert got.shape == (B, 3, d, d) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    Xc = X.cpu()
    assert torch.equal(want[4], Xc[5]) and torch.equal(want[3], Xc[4]) and torch.equal(want[13], Xc[13])
    assert not torch.equal(want[0], Xc[0]) and not torch.equal(want[7], Xc[7])      # the blend with the 1 x 1 partner; the box across two bands
    # identity records, and a permuted repeating index under the mix
    ident = torch.tensor([mix_ref.record(B - 1 - b) for b in range(B)], dtype=torch.int32).cuda()
    buf = torch.full_like(X, float("nan"))
    assert tr(sub, out=buf, rrc=r.cuda(), mix=ident) is buf and torch.equal(buf, X)
    g = torch.Generator().manual_seed(s)
    index = torch.cat([torch.randperm(B, generator=g)[:10], torch.randint(0, B, (6,), generator=g)]).cuda()
    Xi = tr(sub, index, rrc=r.cuda())
    assert torch.equal(tr(sub, index, rrc=r.cuda(), mix=recs.cuda()).cpu(), torch.from_numpy(mix_ref.mixed_images(Xi.cpu().numpy(), recs)))


def test_loader_draws_the_records_after_the_plan_and_before_the_mix_records_and_does_not_synchronise():
    n, bs = 40, 16
    imgs = _images(n, 32, 77)
    labels = np.random.default_rng(7).integers(0, 10, n)
    tr = _case(32, 224)[0]
    c, m = qat_vit_amd.RandomResizedCrop(), qat_vit_amd.MixupCutmix(mode="elem")
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, crop=c, mix=m, generator=torch.Generator().manual_seed(12),
                                        return_index=True, transform=tr)
    tr.window_tables()                                               # (built on first use: here, not under the mode below)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            loader.labels.sum().item()                               # the mode is honoured: a synchronising call raises
        epochs = [list(loader) for _ in range(2)]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    g = torch.Generator().manual_seed(12)                            # the expectation: plan, then windows, then mix records
    seen = []
    for got in epochs:
        plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
        windows = c.draw(n, 32, g)
        recs = m.draw([len(b) for b in plan], 224, g)
        seen.append(windows)
        assert len(got) == len(plan) == 3 and [len(b) for b in plan] == [16, 16, 8]
        o = 0
        for (x, y, idx, r), b in zip(got, plan):
            w, rb = windows[o:o + len(b)], recs[o:o + len(b)]
            o += len(b)
            assert torch.equal(idx.cpu(), b) and idx.dtype == torch.int64 and torch.equal(y.cpu(), torch.from_numpy(labels)[b])
            assert r.dtype == torch.int32 and r.shape == (len(b), 6) and r.is_cuda and r.is_contiguous() and torch.equal(r.cpu(), rb)
            X = _normalized(host_rrc(imgs[b.numpy()], w, 224))
            assert torch.equal(x.cpu(), torch.from_numpy(mix_ref.mixed_images(X.numpy(), rb)))
    assert not torch.equal(seen[0], seen[1])                         # the second epoch draws new windows
    # the tuple forms, with and without the index and the mix records; without mix nothing but the plan and the windows is drawn
    for ret, mix, length in ((False, m, 3), (True, None, 3), (False, None, 2)):
        first = next(iter(qat_vit_amd.GpuImageLoader(imgs, labels, bs, crop=c, mix=mix, generator=torch.Generator().manual_seed(3), transform=tr,
                                                     return_index=ret)))
        assert len(first) == length and first[0].shape == (16, 3, 224, 224) and first[1].shape == (16,)
        w = c.draw(n, 32, torch.Generator().manual_seed(3))          # a sequential plan draws nothing
        if mix is None:
            assert torch.equal(first[0].cpu(), _normalized(host_rrc(imgs[:16], w[:16], 224)))
            assert not ret or torch.equal(first[2].cpu(), torch.arange(16))
        else:
            assert first[-1].shape == (16, 6) and first[-1].dtype == torch.int32


def test_refusals():
    tr, imgs, src, recs, r, _ = _case(32, 224)
    n = len(recs)
    for bad in (r.long(), r[:5], recs, r[:, :1], torch.zeros(n, 4, dtype=torch.int32, device="cuda")[:, ::2], r.flatten()):
        with pytest.raises(ValueError, match="rrc must be"):
            tr(src, rrc=bad)
    with pytest.raises(ValueError, match="mix must be"):
        tr(src, rrc=r, mix=torch.zeros(n, 5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="rrc and aug are mutually exclusive"):
        tr(src, rrc=r, aug=torch.zeros(n, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="crop and augment are mutually exclusive"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 32, 32, 3), np.uint8), np.zeros(4, np.int64), 2, transform=tr,
                                   crop=qat_vit_amd.RandomResizedCrop(), augment=qat_vit_amd.RandomCropFlip(4))
    with pytest.raises(TypeError, match="RandomResizedCrop"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 32, 32, 3), np.uint8), np.zeros(4, np.int64), 2, transform=tr, crop=qat_vit_amd.RandomCropFlip(4))
