"""The bytes-in blur form (qatvit_image_bytes_blur through GpuBytesBlurNormalize, GpuWideResizeNormalize(blur=True) and GpuImageLoader) on an
MI355X.  Every comparison is exact: against the one-launch entry at S = D as int32 views where that entry is served (D <= 144 with mix records),
against Pillow's own bytes of tests/golden/blur_kat.npz, and against the host composition value_table[jitter(blur_ref(grayscale / solarize(bytes)))]
-> erase_ref -> mix_ref where it is not (D = 224, D = 384).  Batches hold 3 .. 6 distinct images (2 at D = 384), so a halo row taken from the neighbouring sample
or from outside the batch shows.  The band is 16 rows without mix records and 8 with them: D = 8 is one band with both clamps in one buffer,
D = 20 a 16-row band and a 4-row band, D = 224 the constant-D kernels, D = 384 the 8-row band without mix records."""
import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from tests import blur_ref, color_ref, erase_ref, mix_ref, wide_ref
from tests.kernel_check import Guarded
from tests.test_gpu_blur import NOBLUR, _blur_records, _color_records, _erase_records, _mix_records
from tests.wide_ref import host_window, pack

pytestmark = pytest.mark.gpu

BATCH = {8: 5, 20: 3, 36: 4, 144: 4, 224: 4}
_cache, _ref = {}, {}


def _case(d):
    """Per size, built once and never changed: the new transform, the one-launch transform at S = D, distinct images (host and device)."""
    if d not in _cache:
        imgs = wide_ref.images(BATCH[d], d, d, 300 + d)
        _cache[d] = (qat_vit_amd.GpuBytesBlurNormalize(d), qat_vit_amd.GpuResizeNormalize(d, out_size=d), imgs, torch.from_numpy(imgs).cuda())
    return _cache[d]


def _t(recs):
    return None if recs is None else torch.as_tensor(np.asarray(recs), dtype=torch.int32).cuda()


def _host(u8, table, color, blur, erase=None, mix=None, contrast=True):
    """(fp32 tensor, int64 sums) of the host composition on uint8 [B, D, D, 3]."""
    c, sums = blur_ref.apply_batch(u8, color, blur, contrast)
    x = color_ref.normalized(c, table)
    if erase is not None:
        x = erase_ref.erased(x, np.asarray(erase).tolist())
    if mix is not None:
        x = mix_ref.mixed_images(x, np.asarray(mix))
    return torch.from_numpy(x), sums


def _sums(tr, B):
    return (tr.color_sums(B).cpu().to(torch.int64) & 0xffffffff).tolist()


def _both(d, color, blur, erase=None, mix=None, contrast=True):
    """The new entry and the one-launch entry at S = D on the same bytes and records, each with its workspace poisoned: (new, old, sums, sums)."""
    new, old, _, src = _case(d)
    B = BATCH[d]
    new.color_sums(B).fill_(-1), old.color_sums(B).fill_(-1)
    kw = dict(color=_t(color), blur=_t(blur), erase=_t(erase), mix=_t(mix), contrast=contrast)
    return new(src, **kw), old(src, None, **kw), _sums(new, B), _sums(old, B)


@pytest.mark.parametrize("d", [8, 20, 36, 144])
def test_bit_for_bit_the_one_launch_entry_where_both_are_served(d):
    B = BATCH[d]
    blur, col, er, mx = _blur_records(B), _color_records(B), _erase_records(d, B), _mix_records(d, B)
    seen = []
    for mix in (None, mx):
        for color, contrast in ((None, True), (col, True), (col, False)):
            for erase in (None, er):
                got, want, s_new, s_old = _both(d, color, blur, erase, mix, contrast)
                what = (d, mix is not None, color is not None, contrast, erase is not None)
                assert got.shape == (B, 3, d, d) and got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32)), what
                assert s_new == s_old, what
                if color is not None and contrast:
                    assert s_new[0] > 0 and s_new[2] == 0, what     # over the poison: a contrast op at 0, none at 2
                else:
                    assert s_new == [0xffffffff] * B, what           # no statistics launch: the workspace stays
                seen.append(got)
    assert not any(torch.equal(seen[0], x) for x in seen[1:])
    assert not torch.equal(seen[0], _both(d, None, [NOBLUR] * B)[0])


@pytest.mark.parametrize("d", [8, 36, 144])
def test_mix_blurs_each_side_by_its_own_record_as_the_one_launch_entry_does(d):
    B = BATCH[d]
    col, er = _color_records(B), _erase_records(d, B)
    on, on2 = blur_ref.pack(2.0), blur_ref.pack(0.5)
    cases = {"sample": [on, NOBLUR, on2, NOBLUR, on], "partner": [NOBLUR, on, NOBLUR, on2, NOBLUR], "both": [on, on2, on2, on, on2]}
    for kind, mx in (("mixup and a box", _mix_records(d, B)), ("cutmix", [mix_ref.cutmix(B - 1 - b, (1, d - 2, 2, d - 1), d) for b in range(B)]),
                     ("mixup", [mix_ref.mixup(B - 1 - b, 0.4) for b in range(B)])):
        outs = {}
        for name, blur in cases.items():
            got, want, s_new, s_old = _both(d, col, blur[:B], er, mx)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and s_new == s_old, (kind, name)
            outs[name] = got
        assert not torch.equal(outs["sample"], outs["partner"]) and not torch.equal(outs["both"], outs["sample"]), kind


def test_pillows_own_bytes():
    """The bytes are what Pillow blurs, so the outputs are the value table of Pillow's bytes in the fixture: at 36 every fixture radius with both
    neighbours of the radius step at r = 1.4142135, the constant images and the impulses; at 224 the two stored radii."""
    f = blur_ref.load()
    below, above = (float(v) for v in f["step"])
    radii = [float(r) for r in f["radii_36"]]
    assert below in radii and above in radii and blur_ref.weights(below)[0] == 0 and blur_ref.weights(above)[0] == 1
    tr = _case(36)[0]
    table = tr.table.cpu().numpy()
    src, recs, want = f["images_36"][f["image_of_36"]], [blur_ref.pack(r) for r in radii], color_ref.normalized(f["out_36"], table)
    assert [r[1:3] for r in recs] == f["weights_36"][:, 1:].tolist()
    sp = f["special_images"]
    src = np.concatenate([src, np.repeat(sp, len(f["special_radii"]), 0)])
    recs += [blur_ref.pack(r) for r in f["special_radii"]] * len(sp)
    want = np.concatenate([want, color_ref.normalized(f["special_out"].reshape(-1, 36, 36, 3), table)])
    assert len(src) == len(recs) == len(want) == 52
    for o in range(0, 52, 4):                                        # four samples per call
        got = tr(torch.from_numpy(src[o:o + 4]).cuda(), blur=_t(recs[o:o + 4]))
        assert torch.equal(got.cpu(), torch.from_numpy(want[o:o + 4])), o
    big = _case(224)[0]
    src = np.concatenate([f["images_224"][f["image_of_224"]], _case(224)[2][:1]])                  # the two stored outputs and a third, other image
    recs = [blur_ref.pack(r) for r in f["radii_224"]] + [NOBLUR]
    got = big(torch.from_numpy(src).cuda(), blur=_t(recs)).cpu()
    assert torch.equal(got[:2], torch.from_numpy(color_ref.normalized(f["out_224"], table)))
    assert torch.equal(got[2], torch.from_numpy(color_ref.normalized(src[2:], table))[0])


def _three_augment_records(seed=5):
    """Four samples of a ThreeAugment draw: one grayscale, one solarize, one blurred at box radius 0 and one at box radius 1."""
    color, blur = qat_vit_amd.ThreeAugment().draw(64, torch.Generator().manual_seed(seed))
    gray, sol = (color[:, 0] >> 8 & 1).bool(), (color[:, 0] >> 9 & 1).bool()
    on, radius = (blur[:, 0] & 1).bool(), blur[:, 0] >> 8 & 255
    pick = [int(m.nonzero()[0]) for m in (on & (radius == 1), gray, on & (radius == 0), sol)]
    color, blur = color[pick], blur[pick]
    # asserted, not supposed: both box radii, and grayscale / solarize / blur / "no blur" all occur
    assert (blur[:, 0] & 1).tolist() == [1, 0, 1, 0] and (blur[:, 0] >> 8 & 255).tolist() == [1, 0, 0, 0]
    assert (color[:, 0] >> 8 & 3).tolist() == [0, 1, 0, 2] and bool((color[:, 0] & 0x3f).all())      # and jitter ops on every one
    return color, blur


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
def test_the_host_composition_at_224_where_the_one_launch_entry_is_refused(mixed):
    new, old, imgs, src = _case(224)
    B = BATCH[224]
    color, blur = _three_augment_records()
    er, mx = _erase_records(224, B), _mix_records(224, B) if mixed else None
    with pytest.raises(RuntimeError, match="qatvit_image_batch_blur: source 224 -> output 224 needs (89536|98272) bytes of LDS"):
        old(src, blur=_t(blur), mix=_t(mx))
    key = ("composition", mixed)
    if key not in _ref:
        _ref[key] = _host(imgs, new.table.cpu().numpy(), color.numpy(), blur.numpy(), er, mx)
    want, s_ref = _ref[key]
    new.color_sums(B).fill_(-1)
    got = new(src, color=color.cuda(), blur=blur.cuda(), erase=_t(er), mix=_t(mx))
    assert torch.equal(got.cpu(), want) and _sums(new, B) == s_ref.tolist()
    assert not torch.equal(got, new(src, color=color.cuda(), blur=_t([NOBLUR] * B), erase=_t(er), mix=_t(mx)))


def _impulse_images(d):
    """Six uint8 [d, d, 3] images: 255 on black in the four corners; on either side of the seams of the 16-row bands (15 | 16, 31 | 32) and of
    the 8-row bands (7 | 8, 15 | 16); in the first and the last column; and two constant images."""
    a = np.zeros((6, d, d, 3), np.uint8)
    for y, x in ((0, 0), (0, d - 1), (d - 1, 0), (d - 1, d - 1)):
        a[0, y, x] = 255
    for y, x in ((15, 5), (16, 20), (31, 9), (32, 30)):
        a[1, y, x] = 255
    for y, x in ((7, 3), (8, 17), (15, 29), (16, 11)):
        a[2, y, x] = 255
    for y, x in ((10, 0), (20, d - 1), (7, d - 1), (8, 0), (16, 0), (31, d - 1)):
        a[3, y, x] = 255
    a[4], a[5] = 255, 77
    return a


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("d", [36, 224])
def test_seams_and_edges_against_the_host_blur(d, mixed):
    tr = _case(d)[0]
    table = tr.table.cpu().numpy()
    imgs = _impulse_images(d)
    blur = [blur_ref.pack(2.0)] * 6                                  # box radius 1: the widest halo
    assert blur_ref.weights(2.0)[0] == 1
    mx = None
    if mixed:
        mx = [mix_ref.mixup(1, 0.3), mix_ref.cutmix(0, (2, d - 1, 1, d - 3), d), mix_ref.record(2), mix_ref.mixup(5, 0.75),
              mix_ref.cutmix(3, (6, 18, 0, d), d), mix_ref.mixup(100, 0.5)]
    key = ("impulses", d)
    if key not in _ref:
        _ref[key] = blur_ref.apply_batch(imgs, None, blur)[0]
    blurred = _ref[key]
    assert np.array_equal(blurred[4:], imgs[4:]) and not np.array_equal(blurred[:4], imgs[:4])       # constant images stay constant
    assert all(blurred[k].max() < 255 and blurred[k].sum() > 0 for k in range(4))
    want = color_ref.normalized(blurred, table)
    if mixed:
        want = mix_ref.mixed_images(want, np.asarray(mx))
    got = tr(torch.from_numpy(imgs).cuda(), blur=_t(blur), mix=_t(mx))
    assert torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("d", [36, 224])
def test_no_blur_is_bitwise_the_colour_entry(d):
    new, old, _, src = _case(d)
    B = BATCH[d]
    none, col, er, mx = _t([NOBLUR] * B), _t(_color_records(B)), _t(_erase_records(d, B)), _t(_mix_records(d, B))
    for extra in ({}, {"color": col}, {"color": col, "contrast": False}, {"erase": er}, {"mix": mx}, {"color": col, "erase": er},
                  {"color": col, "mix": mx}, {"color": col, "erase": er, "mix": mx}):
        new.color_sums(B).fill_(-1), old.color_sums(B).fill_(-1)
        sibling = old(src, None, **extra)                            # no blur=: the colour, erase, mix or plain entry
        buf = torch.full_like(sibling, float("nan"))
        assert new(src, out=buf, blur=none, **extra) is buf
        assert torch.equal(buf.view(torch.int32), sibling.view(torch.int32)), sorted(extra)
        if "color" in extra:
            assert _sums(new, B) == _sums(old, B), sorted(extra)


@pytest.mark.parametrize("d", [20, 36])
def test_a_malformed_record_gives_the_cleaned_records_result(d):
    new, _, imgs, src = _case(d)
    B, good = BATCH[d], blur_ref.pack(2.0)
    groups = [[[good[0] | 0xFE | -(1 << 16)] + good[1:3] + [-1],     # stray bits of word 0 and word 3: the good record
               [1 | 2 << 8] + good[1:],                              # radius 2
               [good[0], 0, good[2], 0],                             # ww = 0
               [good[0], good[1], good[2] + 1, 0]],                  # weights summing above 2^24
              [[1, (1 << 24) + 1, 0, 0], [good[0], good[1], -1, 0], [1, 1, 0x7fffffff, 0], [good[0] & ~1] + good[1:]],   # .. negative fw .. bit 0 clear
              [[-1] * 4, [1 | 255 << 8, 1, 0, 0], [1, -(1 << 31), 0, 0], [1, 1 << 24, 0, 0]]]     # the last: valid, the identity
    col, table = _color_records(B), new.table.cpu().numpy()
    assert [blur_ref.cleaned(r) is None for r in groups[0]] == [False, True, True, True]
    for bad in groups:
        bad = bad[:B]
        fixed = [list(blur_ref.cleaned(r) or ()) for r in bad]
        fixed = [[1 | c[0] << 8, c[1], c[2], 0] if c else NOBLUR for c in fixed]
        outs = []
        for recs in (bad, fixed):
            new.color_sums(B).fill_(-1)
            outs.append((new(src, color=_t(col), blur=_t(recs)), _sums(new, B)))
        want, s_ref = _host(imgs, table, col, fixed)
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][0].cpu(), want)
        assert outs[0][1] == outs[1][1] == s_ref.tolist()
    assert torch.equal(outs[0][0], new(src, color=_t(col), blur=_t([NOBLUR] * B)))      # the last group: nothing is blurred


@pytest.mark.parametrize("d", [8, 20, 36, 224])
def test_guard_bands_around_out_and_sums_stay_intact_and_every_element_is_written(d):
    new, _, _, src = _case(d)
    B, L = BATCH[d], data.native.lib()
    col, er, bl = _t(_color_records(B)), _t(_erase_records(d, B)), _t(_blur_records(B, 2))
    for m in (None, _t(_mix_records(d, B))):
        out = Guarded(B * 3 * d, d, torch.float32, "cuda")           # the view holds the sentinel: an element that is not stored stays a NaN
        sums = Guarded(1, B, torch.int32, "cuda", pad=64)
        rc = L.qatvit_image_bytes_blur(src.data_ptr(), B, d, new.table.data_ptr(), None if m is None else m.data_ptr(), er.data_ptr(), col.data_ptr(),
                                       sums.t.data_ptr(), bl.data_ptr(), out.t.data_ptr(), data.native.stream_ptr())
        data.native.check(rc, "qatvit_image_bytes_blur")
        torch.cuda.synchronize()
        out.check(f"out {d} mix={m is not None}")
        sums.check(f"sums {d} mix={m is not None}")
        want = new(src, color=col, erase=er, blur=bl, mix=m)
        assert not bool(torch.isnan(out.t).any()) and torch.equal(out.t.view(B, 3, d, d).view(torch.int32), want.view(torch.int32))
        assert torch.equal(sums.t.flatten(), new.color_sums(B))


def _mix6(d):
    return [mix_ref.mixup(1, 0.3), mix_ref.cutmix(0, (2, d - 1, 1, d - 3), d), mix_ref.record(2), mix_ref.mixup(5, 0.75),
            mix_ref.cutmix(3, (0, d, 0, d), d), mix_ref.mixup(100, 0.5)]


@pytest.mark.parametrize("S", [32, 37])
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
def test_the_two_paths_agree_where_both_apply(S, mixed):
    d, B = 224, 6
    one, two = qat_vit_amd.GpuResizeNormalize(S, out_size=d), qat_vit_amd.GpuWideResizeNormalize((S, S), out_size=d, blur=True)
    imgs = torch.from_numpy(wide_ref.images(10, S, S, S)).cuda()
    g = torch.Generator().manual_seed(S)
    index = torch.cat([torch.randperm(10, generator=g)[:4], torch.randint(0, 10, (2,), generator=g)]).cuda()
    r = torch.cat([torch.tensor(wide_ref.corner_records(S, S, d)[:3], dtype=torch.int32), qat_vit_amd.RandomResizedCrop().draw(3, S, g)]).cuda()
    m = _t(_mix6(d)) if mixed else None
    e = qat_vit_amd.RandomErasing(p=0.7, mode="pixel").draw(B, d, g).cuda()
    c, bl = (t.cuda() for t in qat_vit_amd.ThreeAugment().draw(B, g))
    bl2 = _t(_blur_records(B))
    for kw in ({"blur": bl2}, {"blur": bl2, "erase": e}, {"blur": bl, "color": c}, {"blur": bl2, "erase": e, "color": c},
               {"blur": bl2, "color": c, "contrast": False}):
        one.color_sums(B).fill_(-1), two.color_sums(B).fill_(-1)
        a, b = one(imgs, index, rrc=r, mix=m, **kw), two(imgs, index, rrc=r, mix=m, **kw)
        assert b.shape == (B, 3, d, d) and b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32)), sorted(kw)
        assert torch.equal(one.color_sums(B), two.color_sums(B)), sorted(kw)
    # without blur records the object is what it is without the switch
    plain = qat_vit_amd.GpuWideResizeNormalize((S, S), out_size=d)
    assert torch.equal(two(imgs, index, rrc=r, mix=m, color=c, erase=e).view(torch.int32), plain(imgs, index, rrc=r, mix=m, color=c, erase=e).view(torch.int32))
    with pytest.raises(NotImplementedError, match="cap of 65536 bytes"):
        plain(imgs, index, rrc=r, blur=bl2)
    with pytest.raises(ValueError, match="aug does not apply"):
        two(imgs, index, aug=torch.zeros(B, dtype=torch.int32).cuda(), blur=bl2)


@pytest.mark.parametrize("H,W,d,B", [(64, 48, 32, 6), (256, 256, 224, 3)])
def test_a_rectangular_source_equals_the_host_window_and_the_host_composition(H, W, d, B):
    tr = qat_vit_amd.GpuWideResizeNormalize((H, W), out_size=d, blur=True)
    imgs = wide_ref.images(B, H, W, 7 * H + W)
    g = torch.Generator().manual_seed(H)
    r = qat_vit_amd.RandomResizedCrop().draw(B, (H, W), g)
    color, blur = qat_vit_amd.ThreeAugment().draw(B, g)
    if B == 3:
        color, blur = (t[[0, 2, 3]] for t in _three_augment_records())    # blurred at box radius 1, at box radius 0, solarized
    assert 0 < int((blur[:, 0] & 1).sum()) < B
    er = qat_vit_amd.RandomErasing(p=0.7, value=(0.5, -1.0, 2.0)).draw(B, d, g)
    mx = _mix6(d)[:B - 1] + [mix_ref.mixup(100, 0.5)]
    u8 = host_window(imgs, r, d)
    table = tr.inner_blur.table.cpu().numpy()
    src = torch.from_numpy(imgs).cuda()
    for mix in (None, mx):
        want, s_ref = _host(u8, table, color.numpy(), blur.numpy(), er.numpy(), mix)
        tr.color_sums(B).fill_(-1)
        got = tr(src, rrc=r.cuda(), color=color.cuda(), blur=blur.cuda(), erase=er.cuda(), mix=_t(mix))
        assert torch.equal(tr.staged(B).cpu(), torch.from_numpy(u8))
        assert torch.equal(got.cpu(), want) and _sums(tr, B) == s_ref.tolist(), mix is not None


def test_loader_with_three_augment_over_a_rectangular_source_does_not_synchronise():
    H, W, D, n, bs = 64, 48, 32, 20, 8
    rng = np.random.default_rng(81)
    imgs, labels = wide_ref.images(n, H, W, 11), rng.integers(0, 10, n)
    tr = qat_vit_amd.GpuWideResizeNormalize((H, W), out_size=D, blur=True)
    c, m = qat_vit_amd.RandomResizedCrop(), qat_vit_amd.MixupCutmix(mode="elem")
    e, t = qat_vit_amd.RandomErasing(p=0.6), qat_vit_amd.ThreeAugment()
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, crop=c, mix=m, erase=e, three_augment=t, transform=tr, return_index=True,
                                        generator=torch.Generator().manual_seed(12))
    for size in (8, 4):                                              # (made on first use: here, not under the mode below)
        tr.color_sums(size), tr.staged(size)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            loader.labels.sum().item()                               # the mode is honoured: a synchronising call raises
        got = [tuple(v.clone() for v in batch) for batch in loader]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    table = tr.inner_blur.table.cpu().numpy()
    g = torch.Generator().manual_seed(12)                            # the expectation: plan, windows of (H, W), mix, erase, then colour and blur records
    plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
    w, recs, boxes = c.draw(n, (H, W), g), m.draw([len(b) for b in plan], D, g), e.draw(n, D, g)
    cols, blurs = t.draw(n, g)
    assert 0 < int((blurs[:, 0] & 1).sum()) < n and len(got) == len(plan) == 3 and [len(b) for b in plan] == [8, 8, 4]
    o = 0
    for (x, y, idx, r), b in zip(got, plan):
        sl = slice(o, o + len(b))
        o += len(b)
        assert torch.equal(idx.cpu(), b) and torch.equal(y.cpu(), torch.from_numpy(labels)[b]) and torch.equal(r.cpu(), recs[sl])
        want, _ = _host(host_window(imgs[b.numpy()], w[sl], D), table, cols[sl].numpy(), blurs[sl].numpy(), boxes[sl].numpy(), recs[sl].numpy())
        assert torch.equal(x.cpu(), want)


def test_384_is_served_without_mix_records_and_refused_with_them():
    d, B = 384, 2
    tr = qat_vit_amd.GpuBytesBlurNormalize(d)
    imgs = wide_ref.images(B, d, d, 384)
    src = torch.from_numpy(imgs).cuda()
    col, blur, er = _color_records(B), [blur_ref.pack(2.0), blur_ref.pack(0.5)], _erase_records(d, B)
    want, s_ref = _host(imgs, tr.table.cpu().numpy(), col, blur, er)
    tr.color_sums(B).fill_(-1)
    got = tr(src, color=_t(col), blur=_t(blur), erase=_t(er))
    assert torch.equal(got.cpu(), want) and _sums(tr, B) == s_ref.tolist()
    mx = _t([mix_ref.mixup(1, 0.3), mix_ref.mixup(0, 0.6)])
    with pytest.raises(RuntimeError, match=r"qatvit_image_bytes_blur failed \(1\): qatvit_image_bytes_blur: output 384 needs 72192 bytes of LDS"):
        tr(src, blur=_t(blur), mix=mx)
    wide = qat_vit_amd.GpuWideResizeNormalize((64, 48), out_size=d, blur=True)      # through the wide transform the library's error arrives unchanged
    small = torch.from_numpy(wide_ref.images(B, 64, 48, 5)).cuda()
    with pytest.raises(RuntimeError, match="qatvit_image_bytes_blur: output 384 needs 72192 bytes of LDS"):
        wide(small, blur=_t(blur), mix=mx)
    assert wide(small, blur=_t(blur)).shape == (B, 3, d, d)
