"""The augmenting input pipeline (qatvit_image_batch_aug through GpuResizeNormalize(aug=...) and GpuImageLoader(augment=...)) on an MI355X: the
batch EQUALS the existing, non-augmenting path applied to the uint8 image that tests/augment_ref.py builds on the host by the coordinate formula
of include/qatvit.h, for every element; at S = 32 also the host transform of that image (Pillow or its restatement), so that the claim does not
rest on the device kernel on both sides."""
import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from tests import augment_ref
from tests.augment_ref import host_augmented, pack
from tests.test_gpu_data import _host_resize, _normalized

pytestmark = pytest.mark.gpu

MODES = [("constant", 0), ("constant", 255), ("reflect", 0)]
SIZES = [(32, 224, 4), (8, 224, 7), (37, 224, 5), (96, 384, 4)]     # S, D, p: the template form, the smallest S, odd unaligned rows, run-time D
_cache = {}


def _images(n, s, seed):
    """n uint8 [s, s, 3] images, the three kinds of tests/test_gpu_data.py in turn: uniform noise, 0 / 255 noise, clipped gaussian."""
    rng = np.random.default_rng(seed)
    kinds = (lambda: rng.integers(0, 256, (s, s, 3), dtype=np.uint8), lambda: (rng.integers(0, 2, (s, s, 3)) * 255).astype(np.uint8),
             lambda: np.clip(rng.normal(128, 60, (s, s, 3)), 0, 255).astype(np.uint8))
    return np.stack([kinds[i % 3]() for i in range(n)])


def _words(p, seed):
    """34 words: the 18 combinations {-p, 0, p}^2 x flip, then 16 drawn ones."""
    drawn = qat_vit_amd.RandomCropFlip(padding=p).draw(16, torch.Generator().manual_seed(seed))
    return torch.cat([torch.tensor(augment_ref.corner_words(p), dtype=torch.int32), drawn])


def _case(s, d, p):
    """Per size, built once and never changed: transform, images (host, device), words (host, device)."""
    if (s, d) not in _cache:
        words = _words(p, s)
        imgs = _images(len(words), s, s)
        _cache[(s, d)] = (qat_vit_amd.GpuResizeNormalize(s, out_size=d), imgs, torch.from_numpy(imgs).cuda(), words, words.cuda())
    return _cache[(s, d)]


@pytest.mark.parametrize("mode,fill", MODES)
@pytest.mark.parametrize("s,d,p", SIZES)
def test_equals_the_plain_path_on_the_host_augmented_bytes(s, d, p, mode, fill):
    tr, imgs, src, words, w = _case(s, d, p)
    assert len(words) == 34 and len(set(words[:18].tolist())) == 18
    aug_u8 = host_augmented(imgs, words, mode, fill)
    assert not np.array_equal(aug_u8, imgs)
    want = tr(torch.from_numpy(aug_u8).cuda())
    got = tr(src, aug=w, padding_mode=mode, fill=fill, padding=p)
    assert got.shape == (34, 3, d, d) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, want)
    if s == 32:                                                      # the host transform of the augmented bytes, with no device kernel behind it
        assert torch.equal(got.cpu(), _normalized(_host_resize(aug_u8, d)))


@pytest.mark.parametrize("s,d,p", SIZES)
def test_no_words_and_zero_words_are_the_plain_call(s, d, p):
    tr, imgs, src, words, w = _case(s, d, p)
    plain = tr(src)
    assert torch.equal(tr(src, aug=None), plain)
    assert torch.equal(tr(src, aug=None, padding_mode="reflect", fill=9), plain)
    zeros = torch.zeros_like(w)
    for mode, fill in MODES:
        assert torch.equal(tr(src, aug=zeros, padding_mode=mode, fill=fill), plain)
    # the C entry with aug == NULL launches the existing kernel
    out = torch.full_like(plain, float("nan"))
    data.native.check(data.native.lib().qatvit_image_batch_aug(src.data_ptr(), None, len(imgs), len(imgs), s, d, tr.coeffs.data_ptr(),
                                                               tr.table.data_ptr(), None, 1, 200, out.data_ptr(), data.native.stream_ptr()), "aug")
    assert torch.equal(out, plain)


@pytest.mark.parametrize("mode,fill", [("constant", 131), ("reflect", 0)])
@pytest.mark.parametrize("s,d,p", [(32, 224, 4), (37, 224, 5)])
def test_word_b_goes_with_batch_position_b_and_image_index_b(s, d, p, mode, fill):
    tr, imgs, src, words, w = _case(s, d, p)
    g = torch.Generator().manual_seed(s)
    index = torch.cat([torch.randperm(34, generator=g)[:20], torch.randint(0, 34, (20,), generator=g)])      # permuted, then repeating
    assert len(set(index.tolist())) < 40
    bw = torch.cat([words, words[:6].flip(0)])                                                           # 40 words, by position
    want = tr(torch.from_numpy(host_augmented(imgs[index.numpy()], bw, mode, fill)).cuda())
    got = tr(src, index.cuda(), aug=bw.cuda(), padding_mode=mode, fill=fill)
    assert torch.equal(got, want)
    assert not torch.equal(got, tr(src, index.cuda(), aug=bw.flip(0).contiguous().cuda(), padding_mode=mode, fill=fill))
    buf = torch.full((40, 3, d, d), float("nan"), device="cuda")
    assert tr(src, index.cuda(), out=buf, aug=bw.cuda(), padding_mode=mode, fill=fill) is buf and torch.equal(buf, want)


@pytest.mark.parametrize("s,d", [(32, 224), (8, 224), (96, 384)])
def test_a_window_wholly_outside_the_image_is_all_fill(s, d):
    tr, imgs, src, _, _ = _case(s, d, {32: 4, 8: 7, 96: 4}[s])
    words = torch.tensor([0, pack(127, 0, False), pack(0, 0, True), pack(3, -128, True), pack(-2, 1, False), pack(127, -128, False), 0],
                         dtype=torch.int32)
    got = tr(src[:7].contiguous(), aug=words.cuda(), padding_mode="constant", fill=77)
    table = tr.table
    for b in (1, 3, 5):
        for c in range(3):
            assert bool((got[b, c] == table[c, 77]).all()), (b, c)
    want = tr(torch.from_numpy(host_augmented(imgs[:7], words, "constant", 77)).cuda())
    assert torch.equal(got, want)                                    # the neighbours are what they are without those words
    plain = tr(src[:7].contiguous())
    assert torch.equal(got[0], plain[0]) and torch.equal(got[6], plain[6])
    # reflect mode takes the same words: the clamp keeps every read inside the image, and the result is the formula's
    got = tr(src[:7].contiguous(), aug=words.cuda(), padding_mode="reflect")
    assert torch.equal(got, tr(torch.from_numpy(host_augmented(imgs[:7], words, "reflect")).cuda()))


def test_loader_draws_the_words_after_the_plan_and_does_not_synchronise():
    n, bs = 40, 16
    imgs = _images(n, 32, 77)
    labels = np.random.default_rng(7).integers(0, 10, n)
    tr = _case(32, 224, 4)[0]
    a = qat_vit_amd.RandomCropFlip(4)
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, augment=a, generator=torch.Generator().manual_seed(12), return_index=True)
    plain = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, generator=torch.Generator().manual_seed(12), return_index=True)
    assert len(loader) == 3
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            loader.labels.sum().item()                               # the mode is honoured: a synchronising call raises
        epochs = [list(loader) for _ in range(2)]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    g = torch.Generator().manual_seed(12)                            # the expectation: plan, then words, from an equally seeded generator
    seen = []
    for got in epochs:
        plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
        words = a.draw(n, g)
        seen.append(words)
        assert len(got) == len(plan) == 3 and [len(b) for b in plan] == [16, 16, 8]
        o = 0
        for (x, y, idx), b in zip(got, plan):
            w = words[o:o + len(b)]
            o += len(b)
            assert torch.equal(idx.cpu(), b) and idx.dtype == torch.int64 and torch.equal(y.cpu(), torch.from_numpy(labels)[b])
            assert torch.equal(x, tr(torch.from_numpy(host_augmented(imgs[b.numpy()], w)).cuda()))
    assert not torch.equal(seen[0], seen[1])                         # the second epoch draws new words
    # without augmentation the plans are RandomSampler's alone: the generator is not advanced by any word
    g = torch.Generator().manual_seed(12)
    src = torch.from_numpy(imgs).cuda()
    for _ in range(2):
        plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
        for (x, y, idx), b in zip(list(plain), plan):
            assert torch.equal(idx.cpu(), b) and torch.equal(y.cpu(), torch.from_numpy(labels)[b]) and torch.equal(x, tr(src, idx))
    # the two-tuple form
    pair = next(iter(qat_vit_amd.GpuImageLoader(imgs, labels, bs, augment=a, generator=torch.Generator().manual_seed(3), transform=tr)))
    assert len(pair) == 2 and pair[0].shape == (16, 3, 224, 224)


def test_refusals():
    tr, imgs, src, words, w = _case(32, 224, 4)
    with pytest.raises(ValueError, match="aug must be"):
        tr(src, aug=w.long())
    with pytest.raises(ValueError, match="aug must be"):
        tr(src, aug=w[:5])
    with pytest.raises(ValueError, match="aug must be"):
        tr(src, aug=words)                                           # on the host
    with pytest.raises(ValueError, match="aug must be"):
        tr(src, aug=torch.zeros(68, dtype=torch.int32, device="cuda")[::2])
    with pytest.raises(ValueError, match="padding_mode must be"):
        tr(src, aug=w, padding_mode="edge")
    with pytest.raises(ValueError, match="fill must be"):
        tr(src, aug=w, fill=256)
    with pytest.raises(ValueError, match="exceed S - 1"):
        tr(src, aug=w, padding_mode="reflect", padding=32)
    tr(src, aug=w, padding_mode="reflect", padding=31)
    tr8 = _case(8, 224, 7)[0]
    with pytest.raises(ValueError, match="exceeds S - 1"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64), 2, transform=tr8, augment=qat_vit_amd.RandomCropFlip(8))
    qat_vit_amd.GpuImageLoader(np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64), 2, transform=tr8, augment=qat_vit_amd.RandomCropFlip(7))
    with pytest.raises(TypeError, match="RandomCropFlip"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64), 2, transform=tr8, augment="crop")
