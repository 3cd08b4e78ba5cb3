"""The colour augmentations inside the batch launch (qatvit_image_batch_color / qatvit_image_batch_rrc_color through GpuResizeNormalize(color=...)
and GpuImageLoader(color=...)) on an MI355X.  Every comparison is torch.equal, without a tolerance, against the composition of the existing host
references: value_table[color_ref(host resize or rrc_ref.host_rrc)], then erase_ref, then mix_ref; tests/color_ref.py is held equal to Pillow
by tests/test_color_abi.py.  The luma sums of the statistics launch are compared exactly too."""
import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from tests import augment_ref, color_ref, erase_ref, mix_ref, rrc_ref
from tests.color_ref import BRIGHTNESS as BR, CONTRAST as CO, SATURATION as SA, pack
from tests.kernel_check import guarded

pytestmark = pytest.mark.gpu

SIZES = [(32, 224), (8, 36), (37, 224)]                              # the DT = 224 forms; DT = 0 with a last band of 4 rows; odd source rows
ARM = {(32, 224): None, (8, 36): ("constant", 131), (37, 224): ("reflect", 0)}      # no words, words in both padding modes
B = 8
IDENT = [0, 0, 0, 0]
_cache, _resized = {}, {}


def _case(s, d):
    """Per size, built once and never changed: transform, images (host and device), words (host)."""
    if (s, d) not in _cache:
        rng = np.random.default_rng(100 + s)
        imgs = rng.integers(0, 256, (B, s, s, 3), dtype=np.uint8)
        imgs[1] = np.clip(rng.normal(128, 40, (s, s, 3)), 0, 255).astype(np.uint8)       # a low-contrast one
        words = qat_vit_amd.RandomCropFlip(padding=3).draw(B, torch.Generator().manual_seed(s))
        _cache[(s, d)] = (qat_vit_amd.GpuResizeNormalize(s, out_size=d), imgs, torch.from_numpy(imgs).cuda(), words)
    return _cache[(s, d)]


def _windows(s):
    """One rrc record per position: the whole image, flips, a one-pixel-wide window, windows in the corners."""
    recs = [(0, 0, s, s, False), (1, 2, s - 3, s - 2, True), (s - 5, 0, 5, s, False), (0, s - 1, s, 1, True), (3, 3, 2, 3, False),
            (s // 2, s // 3, s // 2, s // 2, True), (0, 0, 1, 1, False), (s - 7, s - 6, 7, 6, True)]
    return torch.tensor([rrc_ref.pack(*r) for r in recs], dtype=torch.int32)


def _u8(s, d, front):
    """uint8 [B, d, d, 3] behind the resize, on the host: front = None, ("aug", mode, fill) or "rrc".  Formed once per case."""
    key = (s, d, front)
    if key not in _resized:
        _, imgs, _, words = _case(s, d)
        if front == "rrc":
            _resized[key] = rrc_ref.host_rrc(imgs, _windows(s).numpy(), d)
        else:
            a = imgs if front is None else augment_ref.host_augmented(imgs, words, front[1], front[2])
            _resized[key] = rrc_ref.host_rrc(a, [rrc_ref.pack(0, 0, s, s, False)] * B, d)
    return _resized[key]


def _front_kw(s, d, front):
    words = _case(s, d)[3]
    if front == "rrc":
        return {"rrc": _windows(s).cuda()}
    return {} if front is None else {"aug": words.cuda(), "padding_mode": front[1], "fill": front[2]}


def _front(s, d):
    return None if ARM[(s, d)] is None else ("aug",) + ARM[(s, d)]


def _want(s, d, front, color, erase=None, mix=None, contrast=True):
    """(fp32 [B, 3, d, d] tensor, int64 [B] sums): the composition of the host references."""
    tr = _case(s, d)[0]
    c, sums = color_ref.apply_batch(_u8(s, d, front), color, contrast)
    x = color_ref.normalized(c, tr.table.cpu().numpy())
    if erase is not None:
        x = erase_ref.erased(x, erase)
    if mix is not None:
        x = mix_ref.mixed_images(x, mix)
    return torch.from_numpy(x), sums


def _t(recs):
    return torch.tensor(recs, dtype=torch.int32).cuda()


def _run(s, d, front, color, erase=None, mix=None, contrast=True, poison=True):
    """(output on the host, the workspace as int64 on the host) of the wrapper's call; the workspace holds ffffffff before it."""
    tr, _, src, _ = _case(s, d)
    if poison:
        tr.color_sums(B).fill_(-1)
    out = tr(src, color=_t(color), erase=None if erase is None else _t(erase), mix=None if mix is None else _t(mix), contrast=contrast,
             **_front_kw(s, d, front))
    return out.cpu(), tr.color_sums(B).cpu().to(torch.int64) & 0xffffffff


def _fixture_records():
    """The fixture's records at D = 36: each op alone at the factors 0, 0.5, 1, 1.7, 2, grayscale, solarize, all six orders, contrast around
    brightness, grayscale + solarize + three ops."""
    return color_ref.load()["records_36"].tolist()


@pytest.mark.parametrize("s,d", SIZES)
def test_chain_equals_the_composition_and_the_sums_are_exact(s, d):
    recs, front = _fixture_records(), _front(s, d)
    assert len(recs) >= 28
    recs = recs + [IDENT] * (-len(recs) % B)
    for o in range(0, len(recs), B):
        chunk = recs[o:o + B]
        got, sums = _run(s, d, front, chunk)
        want, s_ref = _want(s, d, front, chunk)
        assert got.shape == (B, 3, d, d) and got.dtype == torch.float32 and torch.equal(got, want), o
        assert sums.tolist() == s_ref.tolist(), o                    # 0 where the record has no contrast op, over the poison
        assert any(s_ref.tolist()) or not any(CO in color_ref.unpack(r)[0] for r in chunk)
    plain = _run(s, d, front, [IDENT] * B)[0]
    assert not torch.equal(got, plain)


@pytest.mark.parametrize("s,d", SIZES)
def test_the_statistic_is_taken_at_the_contrast_ops_position(s, d):
    front = _front(s, d)
    first, last = pack((CO, BR), 1.7, 1.6), pack((BR, CO), 1.7, 1.6)
    # positions 0 .. 3 hold image 0 .. 3 through contrast-then-brightness, 4 .. 7 the same images through brightness-then-contrast
    tr, imgs, src, _ = _case(s, d)
    index = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3]).cuda()
    recs = [first] * 4 + [last] * 4
    tr.color_sums(B).fill_(-1)
    got = tr(src, index, color=_t(recs), **({} if front is None else {"aug": _case(s, d)[3][:4].repeat(2).cuda(), "padding_mode": front[1],
                                                                      "fill": front[2]})).cpu()
    sums = (tr.color_sums(B).cpu().to(torch.int64) & 0xffffffff).tolist()
    u8 = _u8(s, d, front)[[0, 1, 2, 3, 0, 1, 2, 3]]
    c, s_ref = color_ref.apply_batch(u8, recs)
    assert torch.equal(got, torch.from_numpy(color_ref.normalized(c, tr.table.cpu().numpy()))) and sums == s_ref.tolist()
    for k in range(4):
        assert not torch.equal(got[k], got[k + 4]) and sums[k] != sums[k + 4] and sums[k] == int(color_ref.luma(u8[k]).sum())


@pytest.mark.parametrize("s,d", [(32, 224), (8, 36)])
def test_constant_images_through_contrast(s, d):
    tr = _case(s, d)[0]
    src = torch.zeros(B, s, s, 3, dtype=torch.uint8)
    src[4:] = 255
    recs = [pack((CO,), contrast=0.0), pack((CO,), contrast=2.0), pack((CO, SA), contrast=2.0, saturation=2.0), IDENT] * 2
    tr.color_sums(B).fill_(-1)
    got = tr(src.cuda(), color=_t(recs)).cpu()
    u8 = np.repeat(np.array([0] * 4 + [255] * 4, np.uint8)[:, None, None, None], d * d * 3, 1).reshape(B, d, d, 3)
    c, s_ref = color_ref.apply_batch(u8, recs)
    assert np.array_equal(c, u8)                                     # a constant image is its own mean
    assert torch.equal(got, torch.from_numpy(color_ref.normalized(c, tr.table.cpu().numpy())))
    assert (tr.color_sums(B).cpu().to(torch.int64) & 0xffffffff).tolist() == s_ref.tolist() == [0] * 4 + [255 * d * d] * 3 + [0]


def _erase_records(d):
    none = [0] * 8
    return [erase_ref.pack(3, 29, 5, d - 3, (0.5, -0.5, 2.0)), none, erase_ref.pack(14, 18, 6, 10, (1.0, 1.0, 1.0)), none,
            erase_ref.pack(0, d, 0, 7, (-1.0, -2.0, -3.0)), erase_ref.pack(d - 3, d, 1, d - 2, (3.0, 3.0, 3.0)), none,
            erase_ref.pack(10, 20, 10, 20, (0.25, 0.25, 0.25))]


def _mix_records(d):
    """0 <-> 1 mixup and cutmix; 2 -> 5 mixup; 3 the identity; 4 takes all of 7 (a whole-image box); 5 mixup with itself; 6 a small box of 2;
    7 a partner outside the batch: itself."""
    return [mix_ref.mixup(1, 0.3), mix_ref.cutmix(0, (3, 29, 5, d - 3), d), mix_ref.mixup(5, 0.75), mix_ref.record(3),
            mix_ref.cutmix(7, (0, d, 0, d), d), mix_ref.mixup(5, 0.6), mix_ref.cutmix(2, (14, 18, 6, 10), d), mix_ref.mixup(100, 0.5)]


def _color_records():
    """Contrast at 0, 1, 2, 5, 7 (7 is the partner that 4 takes whole; 5 is the partner of 2 and of itself), none at 3, 4, 6."""
    return [pack((CO, BR, SA), 1.3, 1.7, 0.4), pack((SA, CO), contrast=0.5, saturation=1.8, gray=False, solarize=100), pack((CO,), contrast=2.0),
            IDENT, pack((BR,), 0.6, gray=True), pack((BR, CO), 1.7, 1.6), pack((SA,), saturation=2.0, solarize=64), pack((CO, SA), 0, 1.4, 0.0)]


@pytest.mark.parametrize("s,d", SIZES)
def test_identity_records_no_records_and_no_workspace(s, d):
    tr, _, src, words = _case(s, d)
    ident, er, mx = _t([IDENT] * B), _t(_erase_records(d)), _t(_mix_records(d))
    fronts = [_front_kw(s, d, f) for f in (None, ("aug", "reflect", 0), "rrc")]
    for kw in fronts:
        for extra in ({}, {"erase": er}, {"mix": mx}, {"erase": er, "mix": mx}):
            sibling = tr(src, **kw, **extra)
            buf = torch.full_like(sibling, float("nan"))
            assert tr(src, out=buf, color=ident, **kw, **extra) is buf
            assert torch.equal(buf.view(torch.int32), sibling.view(torch.int32))                 # identity records: bitwise the sibling's
            assert torch.equal(tr(src, color=ident, contrast=False, **kw, **extra).view(torch.int32), sibling.view(torch.int32))
            assert torch.equal(tr(src, color=None, **kw, **extra).view(torch.int32), sibling.view(torch.int32))
    # the C entries with color == NULL launch the erase entries' kernels; sums is not touched
    L, w, rrc = data.native.lib(), words.cuda(), _windows(s).cuda()
    sums = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    for m in (mx, None):
        opt = None if m is None else m.data_ptr()
        want = tr(src, aug=w, padding_mode="reflect", mix=m, erase=er)
        out = torch.full_like(want, float("nan"))
        data.native.check(L.qatvit_image_batch_color(src.data_ptr(), None, B, B, s, d, tr.coeffs.data_ptr(), tr.table.data_ptr(), w.data_ptr(), 1, 200,
                                                     opt, er.data_ptr(), None, sums.data_ptr(), out.data_ptr(), data.native.stream_ptr()), "color")
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        want = tr(src, rrc=rrc, mix=m, erase=er)
        out = torch.full_like(want, float("nan"))
        data.native.check(L.qatvit_image_batch_rrc_color(src.data_ptr(), None, B, B, s, d, tr.window_tables().data_ptr(), tr.table.data_ptr(),
                                                         rrc.data_ptr(), opt, er.data_ptr(), None, sums.data_ptr(), out.data_ptr(),
                                                         data.native.stream_ptr()), "rrc_color")
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert bool((sums == -1).all())
    # sums == NULL with contrast records: the result of the records without their contrast op, and the workspace stays as it was
    recs, front = _color_records(), _front(s, d)
    tr.color_sums(B).fill_(-1)
    got = tr(src, color=_t(recs), contrast=False, **_front_kw(s, d, front)).cpu()
    assert bool((tr.color_sums(B) == -1).all())
    stripped = [color_ref.cleaned(r, contrast=False) for r in recs]
    assert stripped != recs and not any(CO in color_ref.unpack(r)[0] for r in stripped)
    assert torch.equal(got, _want(s, d, front, recs, contrast=False)[0]) and torch.equal(got, _run(s, d, front, stripped)[0])
    assert not torch.equal(got, _run(s, d, front, recs)[0])


@pytest.mark.parametrize("s,d", [(32, 224), (8, 36)])
def test_record_b_goes_with_batch_position_b(s, d):
    front, recs = _front(s, d), _color_records()
    perm = [3, 0, 7, 1, 6, 2, 5, 4]
    tr, _, src, words = _case(s, d)
    index = torch.tensor(perm).cuda()
    kw = {} if front is None else {"aug": words[perm].contiguous().cuda(), "padding_mode": front[1], "fill": front[2]}
    base, base_sums = _run(s, d, front, recs)
    tr.color_sums(B).fill_(-1)
    got = tr(src, index, color=_t([recs[k] for k in perm]), **kw).cpu()    # images, words and records permuted together: the outputs permute
    assert torch.equal(got, base[perm]) and (tr.color_sums(B).cpu().to(torch.int64) & 0xffffffff).tolist() == base_sums[perm].tolist()
    other = tr(src, index, color=_t(recs), **kw).cpu()                     # the records left in place: position b takes record b
    u8 = _u8(s, d, front)[perm]
    c, _ = color_ref.apply_batch(u8, recs)
    assert torch.equal(other, torch.from_numpy(color_ref.normalized(c, tr.table.cpu().numpy()))) and not torch.equal(other, got)


@pytest.mark.parametrize("s,d", SIZES)
def test_a_malformed_record_gives_the_cleaned_records_result(s, d):
    f, front = color_ref.f32_bits, _front(s, d)
    good = pack((CO, BR, SA), 1.5, 0.5, 2.0, gray=True, solarize=77)
    bad = [good,
           [-1] * 4,                                                 # all bits set: saturation thrice with a NaN factor; grayscale, solarize 255
           [good[0] | 0xC0 | 0xFC00 | -(1 << 24)] + good[1:],        # every stray bit of word 0
           pack((BR, BR, CO), 1.5, 0.5),                             # a repeated op code
           pack((CO, CO, CO), contrast=1.7),
           pack((BR, CO, SA), 1.5, float("nan"), 2.0),               # NaN, -inf, negative factors: the op alone is the identity
           pack((SA, BR, CO), float("-inf"), 1.7, -0.5),
           [200 << 16, f(3.0), f(-1.0), f(float("inf"))]]            # a threshold without the solarize bit, factors without ops: the identity
    fixed = [color_ref.cleaned(r) for r in bad]
    assert fixed[0] == good and fixed[2] == good and fixed[7] == IDENT and fixed != bad
    got, sums = _run(s, d, front, bad)
    again, sums2 = _run(s, d, front, fixed)
    want, s_ref = _want(s, d, front, fixed)
    assert torch.equal(got, again) and torch.equal(got, want) and sums.tolist() == sums2.tolist() == s_ref.tolist()
    assert s_ref[5] == 0 and s_ref[3] > 0 and torch.equal(got[7], _run(s, d, front, [IDENT] * B)[0][7])


@pytest.mark.parametrize("front", ["aug", "rrc"])
@pytest.mark.parametrize("s,d", SIZES)
def test_mix_takes_the_coloured_and_erased_partner(s, d, front):
    front = "rrc" if front == "rrc" else ("aug", "reflect", 0)
    col, er, mx = _color_records(), _erase_records(d), _mix_records(d)
    got, sums = _run(s, d, front, col, erase=er, mix=mx)
    want, s_ref = _want(s, d, front, col, erase=er, mix=mx)
    assert torch.equal(got, want) and sums.tolist() == s_ref.tolist() and s_ref[7] > 0 and s_ref[4] == 0
    alone = _want(s, d, front, col, erase=er)[0]
    assert torch.equal(got[4], alone[7]) and torch.equal(got[3], alone[3])         # all of the partner, by the partner's records and sums[7]
    assert not torch.equal(got[0], alone[0]) and not torch.equal(got[6], alone[6])
    # without erase records, and without mix records
    got2, _ = _run(s, d, front, col, mix=mx)
    assert torch.equal(got2, _want(s, d, front, col, mix=mx)[0]) and not torch.equal(got2, got)
    assert torch.equal(_run(s, d, front, col, erase=er)[0], alone)
    # with the partner's record exchanged, only the positions that take something from that partner change
    col2 = list(col)
    col2[7] = pack((CO,), contrast=0.3)
    got3, _ = _run(s, d, front, col2, erase=er, mix=mx)
    changed = [b for b in range(B) if not torch.equal(got3[b], got[b])]
    assert changed == [4, 7] and torch.equal(got3, _want(s, d, front, col2, erase=er, mix=mx)[0])


@pytest.mark.parametrize("s,d", SIZES)
def test_guard_bands_around_out_and_sums_stay_intact(s, d):
    tr, _, src, words = _case(s, d)
    L, col, er, mx = data.native.lib(), _t(_color_records()), _t(_erase_records(d)), _t(_mix_records(d))
    w, rrc = words.cuda(), _windows(s).cuda()
    for use_rrc in (False, True):
        for m in (None, mx):
            out, check_out = guarded(B * 3 * d, d, torch.float32, "cuda")
            sums, check_sums = guarded(1, B, torch.int32, "cuda", pad=8)
            opt = None if m is None else m.data_ptr()
            if use_rrc:
                rc = L.qatvit_image_batch_rrc_color(src.data_ptr(), None, B, B, s, d, tr.window_tables().data_ptr(), tr.table.data_ptr(), rrc.data_ptr(),
                                                    opt, er.data_ptr(), col.data_ptr(), sums.data_ptr(), out.data_ptr(), data.native.stream_ptr())
            else:
                rc = L.qatvit_image_batch_color(src.data_ptr(), None, B, B, s, d, tr.coeffs.data_ptr(), tr.table.data_ptr(), w.data_ptr(), 1, 0, opt,
                                                er.data_ptr(), col.data_ptr(), sums.data_ptr(), out.data_ptr(), data.native.stream_ptr())
            data.native.check(rc, "color")
            torch.cuda.synchronize()
            check_out(f"out {s} {d} rrc={use_rrc}")
            check_sums(f"sums {s} {d} rrc={use_rrc}")
            want, s_ref = _want(s, d, "rrc" if use_rrc else ("aug", "reflect", 0), _color_records(), erase=_erase_records(d),
                                mix=None if m is None else _mix_records(d))
            assert torch.equal(out.view(B, 3, d, d).cpu(), want)     # every element stored: none is the sentinel
            assert (sums.cpu().to(torch.int64) & 0xffffffff).flatten().tolist() == s_ref.tolist()


@pytest.mark.parametrize("crop", [False, True], ids=["augment", "crop"])
def test_loader_draws_the_records_last_and_does_not_synchronise(crop):
    n, bs = 20, 8
    rng = np.random.default_rng(78)
    imgs, labels = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, n)
    tr = _case(32, 224)[0]
    a, c, m = qat_vit_amd.RandomCropFlip(4), qat_vit_amd.RandomResizedCrop(), qat_vit_amd.MixupCutmix(mode="elem")
    e = qat_vit_amd.RandomErasing(p=0.6)
    j = qat_vit_amd.ColorJitter(0.4, 0.4, 0.4, grayscale=0.2, solarize=0.2)
    front = {"crop": c} if crop else {"augment": a}
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, mix=m, erase=e, color=j, generator=torch.Generator().manual_seed(12),
                                        return_index=True, transform=tr, **front)
    tr.window_tables()                                               # (built on first use: here, not under the mode below)
    for size in (8, 4):
        tr.color_sums(size)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            loader.labels.sum().item()                               # the mode is honoured: a synchronising call raises
        epochs = [list(loader) for _ in range(2)]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    g = torch.Generator().manual_seed(12)                            # the expectation: plan, words / windows, mix, erase, colour records
    src, seen = torch.from_numpy(imgs).cuda(), []
    for got in epochs:
        plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
        w = c.draw(n, 32, g) if crop else a.draw(n, g)
        recs = m.draw([len(b) for b in plan], 224, g)
        boxes = e.draw(n, 224, g)
        cols = j.draw(n, g)
        seen.append(cols)
        assert len(got) == len(plan) == 3 and [len(b) for b in plan] == [8, 8, 4]
        o = 0
        for (x, y, idx, r), b in zip(got, plan):
            sl = slice(o, o + len(b))
            o += len(b)
            assert torch.equal(idx.cpu(), b) and torch.equal(y.cpu(), torch.from_numpy(labels)[b]) and torch.equal(r.cpu(), recs[sl])
            kw = {"rrc": w[sl].cuda()} if crop else {"aug": w[sl].cuda(), "padding_mode": a.padding_mode, "fill": a.fill}
            direct = tr(src, idx, mix=recs[sl].cuda(), erase=boxes[sl].cuda(), color=cols[sl].cuda(), **kw)
            assert torch.equal(x.view(torch.int32), direct.view(torch.int32))                    # a direct call with the drawn records
            assert not torch.equal(x, tr(src, idx, mix=recs[sl].cuda(), erase=boxes[sl].cuda(), **kw))
    assert not torch.equal(seen[0], seen[1])                         # the second epoch draws new records
    # with color set, the plan, the words / windows, the mix and the erase records are those of the same seed without it
    old = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, mix=m, erase=e, generator=torch.Generator().manual_seed(12), return_index=True,
                                     transform=tr, **front)
    g = torch.Generator().manual_seed(12)
    qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
    w = c.draw(n, 32, g) if crop else a.draw(n, g)
    m.draw([8, 8, 4], 224, g)
    boxes, o = e.draw(n, 224, g), 0
    for (x, y, idx, r), (x2, y2, idx2, r2) in zip(list(old), epochs[0]):
        assert torch.equal(idx, idx2) and torch.equal(y, y2) and torch.equal(r, r2) and x.shape == x2.shape
        kw = {"rrc": w[o:o + len(idx)].cuda()} if crop else {"aug": w[o:o + len(idx)].cuda(), "padding_mode": a.padding_mode, "fill": a.fill}
        assert torch.equal(x, tr(src, idx, mix=r, erase=boxes[o:o + len(idx)].cuda(), **kw))      # the same erase records, too
        o += len(idx)
    # the tuple forms are the loader's without color; alone, color draws nothing but its records behind a sequential plan, and without
    # contrast no statistics launch runs: the workspace stays as it was
    for ret, mix, length in ((False, m, 3), (True, None, 3), (False, None, 2)):
        first = next(iter(qat_vit_amd.GpuImageLoader(imgs, labels, bs, mix=mix, color=j, generator=torch.Generator().manual_seed(3), transform=tr,
                                                     return_index=ret)))
        assert len(first) == length and first[0].shape == (8, 3, 224, 224) and first[1].shape == (8,)
        if mix is None:
            cols = j.draw(n, torch.Generator().manual_seed(3))
            assert torch.equal(first[0], tr(src[:8].contiguous(), color=cols[:8].cuda()))
    tr.color_sums(8).fill_(-1)
    j2 = qat_vit_amd.ColorJitter(0.4, 0, 0.4)
    first = next(iter(qat_vit_amd.GpuImageLoader(imgs, labels, bs, color=j2, generator=torch.Generator().manual_seed(3), transform=tr)))
    assert bool((tr.color_sums(8) == -1).all())
    assert torch.equal(first[0], tr(src[:8].contiguous(), color=j2.draw(n, torch.Generator().manual_seed(3))[:8].cuda()))


def test_refusals():
    tr, _, src, _ = _case(32, 224)
    r = _t(_color_records())
    for bad in (r.long(), r[:5], r.cpu(), r[:, :3], torch.zeros(B, 8, dtype=torch.int32, device="cuda")[:, ::2], r.flatten()):
        for kw in ({}, {"mix": _t(_mix_records(224))}, {"rrc": _windows(32).cuda()}):
            with pytest.raises(ValueError, match="color must be"):
                tr(src, color=bad, **kw)
    with pytest.raises(ValueError, match="erase must be"):
        tr(src, color=r, erase=torch.zeros(B, 6, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError, match="ColorJitter"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 32, 32, 3), np.uint8), np.zeros(4, np.int64), 2, transform=tr, color="jitter")
