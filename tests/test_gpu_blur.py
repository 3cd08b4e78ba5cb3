"""Gaussian blur inside the batch launch (qatvit_image_batch_blur / qatvit_image_batch_rrc_blur through GpuResizeNormalize(blur=...) and
GpuImageLoader(blur=... / three_augment=...)) on an MI355X.  Every comparison is torch.equal, without a tolerance, against
value_table[jitter(blur_ref(grayscale / solarize(host resize)))], then erase_ref, then mix_ref; tests/blur_ref.py is held equal to Pillow by
tests/test_blur_abi.py, and at S = D = 36, where the resize returns its input, the outputs are compared with Pillow's own bytes of
tests/golden/blur_kat.npz.  The luma sums of the statistics launch are compared exactly too.  The kernel's band is 16 rows, and 8 with mix
records: D = 8 is one band smaller than band + halo, D = 20 and D = 36 end in a band of 4 rows, D = 224 takes the constant-D kernels."""
import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from tests import augment_ref, blur_ref, color_ref, erase_ref, mix_ref, rrc_ref
from tests.color_ref import BRIGHTNESS as BR, CONTRAST as CO, SATURATION as SA, pack
from tests.kernel_check import guarded

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (12, 20), (8, 36), (32, 224)]
BATCH = {(8, 8): 5, (12, 20): 3, (8, 36): 4, (32, 224): 4}
FRONTS = [("aug", "reflect", 0), "rrc"]
NOBLUR = [0, 0, 0, 0]
_cache, _resized, _ref = {}, {}, {}


def _case(s, d):
    """Per size, built once and never changed: transform, images (host and device), words (host)."""
    if (s, d) not in _cache:
        rng, B = np.random.default_rng(200 + s + d), BATCH[(s, d)]
        imgs = rng.integers(0, 256, (B, s, s, 3), dtype=np.uint8)
        imgs[1] = np.clip(rng.normal(128, 40, (s, s, 3)), 0, 255).astype(np.uint8)
        words = qat_vit_amd.RandomCropFlip(padding=3).draw(B, torch.Generator().manual_seed(s))
        _cache[(s, d)] = (qat_vit_amd.GpuResizeNormalize(s, out_size=d), imgs, torch.from_numpy(imgs).cuda(), words)
    return _cache[(s, d)]


def _windows(s, B):
    recs = [(0, 0, s, s, False), (1, 2, s - 3, s - 2, True), (s - 5, 0, 5, s, False), (0, s - 1, s, 1, True), (3, 3, 2, 3, False)]
    return torch.tensor([rrc_ref.pack(*r) for r in recs[:B]], dtype=torch.int32)


def _u8(s, d, front):
    """uint8 [B, d, d, 3] behind the resize, on the host: front = None, ("aug", mode, fill) or "rrc".  Formed once per case."""
    key = (s, d, front)
    if key not in _resized:
        _, imgs, _, words = _case(s, d)
        B = len(imgs)
        if front == "rrc":
            _resized[key] = rrc_ref.host_rrc(imgs, _windows(s, B).numpy(), d)
        else:
            a = imgs if front is None else augment_ref.host_augmented(imgs, words, front[1], front[2])
            _resized[key] = rrc_ref.host_rrc(a, [rrc_ref.pack(0, 0, s, s, False)] * B, d)
    return _resized[key]


def _front_kw(s, d, front):
    B = BATCH[(s, d)]
    if front == "rrc":
        return {"rrc": _windows(s, B).cuda()}
    return {} if front is None else {"aug": _case(s, d)[3].cuda(), "padding_mode": front[1], "fill": front[2]}


def _t(recs):
    return None if recs is None else torch.tensor(recs, dtype=torch.int32).cuda()


def _want(s, d, front, color, blur, erase=None, mix=None, contrast=True):
    """(fp32 [B, 3, d, d] tensor, int64 [B] sums): the composition of the host references; the coloured and blurred bytes are formed once per key."""
    key = (s, d, front, repr(color), repr(blur), contrast)
    if key not in _ref:
        _ref[key] = blur_ref.apply_batch(_u8(s, d, front), color, blur, contrast)
    c, sums = _ref[key]
    x = color_ref.normalized(c, _case(s, d)[0].table.cpu().numpy())
    if erase is not None:
        x = erase_ref.erased(x, erase)
    if mix is not None:
        x = mix_ref.mixed_images(x, mix)
    return torch.from_numpy(x), sums


def _run(s, d, front, color, blur, erase=None, mix=None, contrast=True):
    """(output on the host, the workspace as int64 on the host) of the wrapper's call; the workspace holds ffffffff before it."""
    tr, _, src, _ = _case(s, d)
    B = BATCH[(s, d)]
    tr.color_sums(B).fill_(-1)
    out = tr(src, color=_t(color), blur=_t(blur), erase=_t(erase), mix=_t(mix), contrast=contrast, **_front_kw(s, d, front))
    return out.cpu(), tr.color_sums(B).cpu().to(torch.int64) & 0xffffffff


def _step():
    return [float(v) for v in blur_ref.load()["step"]]


def _blur_records(B, shift=0):
    """Position b: box radius 1 (r = 2.0), none, box radius 0 (r = 0.5), the radius just above the step, just below it - from `shift` on."""
    below, above = _step()
    recs = [blur_ref.pack(2.0), NOBLUR, blur_ref.pack(0.5), blur_ref.pack(above), blur_ref.pack(below), blur_ref.pack(0.1), blur_ref.pack(1.0)]
    return [recs[(b + shift) % len(recs)] for b in range(B)]


def _color_records(B):
    """Contrast behind the blur at 0, 1 (a sample that is not blurred), 3; grayscale / solarize in front of it at 1, 2, 4."""
    recs = [pack((CO, BR, SA), 1.3, 1.7, 0.4), pack((SA, CO), contrast=0.5, saturation=1.8, gray=True, solarize=100), pack((BR,), 0.6, solarize=64),
            pack((BR, CO), 1.7, 1.6), pack(gray=True)]
    return recs[:B]


def _erase_records(d, B):
    none = [0] * 8
    recs = [erase_ref.pack(1, d - 2, 2, d - 1, (0.5, -0.5, 2.0)), none, erase_ref.pack(d // 2, d // 2 + 3, 1, 5, (1.0, 1.0, 1.0)),
            erase_ref.pack(0, d, 0, 3, (-1.0, -2.0, -3.0)), erase_ref.pack(d - 3, d, 1, d - 2, (3.0, 3.0, 3.0))]
    return recs[:B]


def _mix_records(d, B):
    """0 mixup with 1; 1 takes a box of 0; 2 the identity (B = 3) or mixup with the last; the last but one a whole-image box of the last (B = 5);
    the last: a partner outside the batch, itself."""
    recs = [mix_ref.mixup(1, 0.3), mix_ref.cutmix(0, (2, d - 1, 1, d - 3), d)]
    if B == 3:
        return recs + [mix_ref.record(2)]
    recs.append(mix_ref.mixup(B - 1, 0.75))
    if B == 5:
        recs.append(mix_ref.cutmix(4, (0, d, 0, d), d))
    return recs + [mix_ref.mixup(100, 0.5)]


@pytest.mark.parametrize("front", FRONTS, ids=["aug", "rrc"])
@pytest.mark.parametrize("s,d", SIZES)
def test_every_form_equals_the_composition_and_the_sums_are_exact(s, d, front):
    B = BATCH[(s, d)]
    blur, col, er, mx = _blur_records(B), _color_records(B), _erase_records(d, B), _mix_records(d, B)
    seen = []
    for color in (col, None):
        for erase in (er, None):
            for mix in (mx, None):
                got, sums = _run(s, d, front, color, blur, erase, mix)
                want, s_ref = _want(s, d, front, color, blur, erase, mix)
                assert got.shape == (B, 3, d, d) and got.dtype == torch.float32 and torch.equal(got, want), (color is None, erase is None, mix is None)
                if color is not None:
                    assert sums.tolist() == s_ref.tolist() and s_ref[0] > 0 and s_ref[1] > 0 and s_ref[2] == 0     # over the poison
                else:
                    assert bool((sums == 0xffffffff).all())          # no colour records: no statistics launch, the workspace stays
                seen.append(got)
    assert not any(torch.equal(seen[0], x) for x in seen[1:])
    # the sum of a blurred sample is that of the BLURRED image in front of its contrast op: it differs from the sum without the blur
    unblurred, s_ref = color_ref.apply_batch(_u8(s, d, front), col)[1], _want(s, d, front, col, blur)[1]
    assert s_ref[0] != unblurred[0] and s_ref[1] == unblurred[1]      # 0 is blurred; 1 is not
    # without aug words (aug == NULL: the zero word)
    if front != "rrc":
        assert torch.equal(_run(s, d, None, col, blur, er, mx)[0], _want(s, d, None, col, blur, er, mx)[0])


def test_pillows_own_bytes_at_36():
    """S = D = 36: the resize returns its input, so the outputs are the value table of Pillow's bytes in the fixture - every fixture radius, both
    sides of the radius step, the constant images, the impulses in the corners and either side of the band seams at rows 8 and 16."""
    f = blur_ref.load()
    tr = qat_vit_amd.GpuResizeNormalize(36, out_size=36)
    table = tr.table.cpu().numpy()
    src = torch.from_numpy(np.concatenate([f["images_36"], f["special_images"]])).cuda()
    n_img, radii = len(f["images_36"]), f["radii_36"]
    index = torch.from_numpy(f["image_of_36"]).cuda()
    recs = [blur_ref.pack(r) for r in radii]
    assert [r[1:3] for r in recs] == f["weights_36"][:, 1:].tolist() and {r[0] >> 8 for r in recs} == {0, 1}
    got = tr(src, index, blur=_t(recs)).cpu()
    assert torch.equal(got, torch.from_numpy(color_ref.normalized(f["out_36"], table)))
    assert not torch.equal(got, tr(src, index).cpu())
    sp_r = f["special_radii"]
    index = torch.arange(n_img, n_img + len(f["special_images"])).repeat_interleave(len(sp_r)).cuda()
    recs = [blur_ref.pack(r) for r in sp_r] * len(f["special_images"])
    want = color_ref.normalized(f["special_out"].reshape(-1, 36, 36, 3), table)
    for kw in ({}, {"rrc": torch.tensor([rrc_ref.pack(0, 0, 36, 36, False)] * len(recs), dtype=torch.int32).cuda()}):
        got = tr(src, index, blur=_t(recs), **kw).cpu()
        assert torch.equal(got, torch.from_numpy(want))
    k = len(sp_r)
    assert torch.equal(got[:2 * k], tr(src, index).cpu()[:2 * k])    # the constant images 0 and 255 stay what they are


@pytest.mark.parametrize("s,d", [(8, 8), (32, 224)])
def test_constant_images_through_blur_and_contrast(s, d):
    tr, B = _case(s, d)[0], 4
    src = torch.zeros(B, s, s, 3, dtype=torch.uint8)
    src[2:] = 255
    col = [pack((CO,), contrast=2.0), pack((CO, SA), contrast=0.0, saturation=2.0)] * 2
    blur = [blur_ref.pack(2.0), blur_ref.pack(_step()[0])] * 2
    tr.color_sums(B).fill_(-1)
    got = tr(src.cuda(), color=_t(col), blur=_t(blur)).cpu()
    u8 = np.repeat(np.array([0] * 2 + [255] * 2, np.uint8)[:, None, None, None], d * d * 3, 1).reshape(B, d, d, 3)
    c, s_ref = blur_ref.apply_batch(u8, col, blur)
    assert np.array_equal(c, u8)                                     # a constant image is its own blur and its own mean
    assert torch.equal(got, torch.from_numpy(color_ref.normalized(c, tr.table.cpu().numpy())))
    assert (tr.color_sums(B).cpu().to(torch.int64) & 0xffffffff).tolist() == s_ref.tolist() == [0] * 2 + [255 * d * d] * 2


@pytest.mark.parametrize("front", FRONTS, ids=["aug", "rrc"])
@pytest.mark.parametrize("s,d", [(8, 36), (32, 224)])
def test_mix_blurs_each_side_by_its_own_record(s, d, front):
    B = BATCH[(s, d)]                                                # 4: 0 <-> 1 mixup and a box, 2 mixup with 3, 3 itself
    col, er, mx = _color_records(B), _erase_records(d, B), _mix_records(d, B)
    on, on2 = blur_ref.pack(2.0), blur_ref.pack(0.5)
    cases = {"sample": [on, NOBLUR, on2, NOBLUR], "partner": [NOBLUR, on, NOBLUR, on2], "both": [on, on2, on2, on], "none": [NOBLUR] * 4}
    outs = {}
    for name, blur in cases.items():
        got, sums = _run(s, d, front, col, blur, er, mx)
        want, s_ref = _want(s, d, front, col, blur, er, mx)
        assert torch.equal(got, want) and sums.tolist() == s_ref.tolist(), name
        outs[name] = got
    alone = _want(s, d, front, col, cases["partner"], er)[0]
    # position 1 takes a box of 0: outside the box its own blurred pixels, inside the pixels of 0, which is not blurred
    assert not torch.equal(outs["partner"][1], alone[1]) and not torch.equal(outs["partner"], outs["sample"])
    assert not torch.equal(outs["both"], outs["sample"]) and not torch.equal(outs["both"], outs["partner"])
    # with the partner's record exchanged, only the positions that take something from that partner change
    blur2 = list(cases["both"])
    blur2[3] = blur_ref.pack(1.0)
    got2 = _run(s, d, front, col, blur2, er, mx)[0]
    assert [b for b in range(B) if not torch.equal(got2[b], outs["both"][b])] == [2, 3]
    assert torch.equal(got2, _want(s, d, front, col, blur2, er, mx)[0])


@pytest.mark.parametrize("s,d", SIZES)
def test_no_blur_is_bitwise_the_colour_entry(s, d):
    tr, _, src, words = _case(s, d)
    B = BATCH[(s, d)]
    none, col, er, mx = _t([NOBLUR] * B), _t(_color_records(B)), _t(_erase_records(d, B)), _t(_mix_records(d, B))
    for front in (None,) + tuple(FRONTS):
        kw = _front_kw(s, d, front)
        for extra in ({"color": col}, {"color": col, "erase": er}, {"color": col, "mix": mx}, {"color": col, "erase": er, "mix": mx}, {"erase": er}, {"mix": mx}, {}):
            sibling = tr(src, **kw, **extra)
            buf = torch.full_like(sibling, float("nan"))
            assert tr(src, out=buf, blur=none, **kw, **extra) is buf
            assert torch.equal(buf.view(torch.int32), sibling.view(torch.int32))                 # "no blur" records: bitwise the sibling's
            assert torch.equal(tr(src, blur=None, **kw, **extra).view(torch.int32), sibling.view(torch.int32))
    # the C entries with blur == NULL are the colour entries
    L, w, rrc = data.native.lib(), words.cuda(), _windows(s, B).cuda()
    for m in (mx, None):
        opt = None if m is None else m.data_ptr()
        sums = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        want = tr(src, aug=w, padding_mode="reflect", mix=m, erase=er, color=col)
        want_sums = tr.color_sums(B).clone()
        out = torch.full_like(want, float("nan"))
        data.native.check(L.qatvit_image_batch_blur(src.data_ptr(), None, B, B, s, d, tr.coeffs.data_ptr(), tr.table.data_ptr(), w.data_ptr(), 1, 200,
                                                    opt, er.data_ptr(), col.data_ptr(), sums.data_ptr(), None, out.data_ptr(),
                                                    data.native.stream_ptr()), "blur")
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(sums, want_sums)
        want = tr(src, rrc=rrc, mix=m, erase=er, color=col)
        out = torch.full_like(want, float("nan"))
        data.native.check(L.qatvit_image_batch_rrc_blur(src.data_ptr(), None, B, B, s, d, tr.window_tables().data_ptr(), tr.table.data_ptr(),
                                                        rrc.data_ptr(), opt, er.data_ptr(), col.data_ptr(), sums.data_ptr(), None, out.data_ptr(),
                                                        data.native.stream_ptr()), "rrc_blur")
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(sums, tr.color_sums(B))


@pytest.mark.parametrize("s,d", [(12, 20), (32, 224)])
def test_a_malformed_record_gives_the_cleaned_records_result(s, d):
    B, good = BATCH[(s, d)], blur_ref.pack(2.0)
    groups = [[[good[0] | 0xFE | -(1 << 16)] + good[1:3] + [-1],     # stray bits of word 0 and word 3: the good record
               [1 | 2 << 8] + good[1:],                              # radius 2
               [good[0], 0, good[2], 0],                             # ww = 0
               [good[0], good[1], good[2] + 1, 0]],                  # oversized weights
              [[1, (1 << 24) + 1, 0, 0], [good[0], good[1], -1, 0], [1, 1, 0x7fffffff, 0], [good[0] & ~1] + good[1:]],
              [[-1] * 4, [1 | 255 << 8, 1, 0, 0], [1, -(1 << 31), 0, 0], [1, 1 << 24, 0, 0]]]     # the last: valid, the identity
    col = _color_records(B)
    for bad in groups:
        bad = bad[:B]
        fixed = [list(blur_ref.cleaned(r) or ()) for r in bad]
        fixed = [[1 | c[0] << 8, c[1], c[2], 0] if c else NOBLUR for c in fixed]
        for front in FRONTS:
            got, sums = _run(s, d, front, col, bad)
            again, sums2 = _run(s, d, front, col, fixed)
            want, s_ref = _want(s, d, front, col, fixed)
            assert torch.equal(got, again) and torch.equal(got, want) and sums.tolist() == sums2.tolist() == s_ref.tolist()
    assert [blur_ref.cleaned(r) is None for r in groups[0]] == [False, True, True, True]
    assert torch.equal(got, _run(s, d, front, col, [NOBLUR] * B)[0])  # the last group: nothing is blurred


@pytest.mark.parametrize("s,d", SIZES)
def test_guard_bands_around_out_and_sums_stay_intact(s, d):
    tr, _, src, words = _case(s, d)
    B = BATCH[(s, d)]
    L, col, er, mx, bl = data.native.lib(), _t(_color_records(B)), _t(_erase_records(d, B)), _t(_mix_records(d, B)), _t(_blur_records(B, 2))
    w, rrc = words.cuda(), _windows(s, B).cuda()
    for use_rrc in (False, True):
        for m in (None, mx):
            out, check_out = guarded(B * 3 * d, d, torch.float32, "cuda")
            sums, check_sums = guarded(1, B, torch.int32, "cuda", pad=64)         # 64 rows of B words: the view stays 256-byte aligned
            opt = None if m is None else m.data_ptr()
            if use_rrc:
                rc = L.qatvit_image_batch_rrc_blur(src.data_ptr(), None, B, B, s, d, tr.window_tables().data_ptr(), tr.table.data_ptr(), rrc.data_ptr(),
                                                   opt, er.data_ptr(), col.data_ptr(), sums.data_ptr(), bl.data_ptr(), out.data_ptr(),
                                                   data.native.stream_ptr())
            else:
                rc = L.qatvit_image_batch_blur(src.data_ptr(), None, B, B, s, d, tr.coeffs.data_ptr(), tr.table.data_ptr(), w.data_ptr(), 1, 0, opt,
                                               er.data_ptr(), col.data_ptr(), sums.data_ptr(), bl.data_ptr(), out.data_ptr(), data.native.stream_ptr())
            data.native.check(rc, "blur")
            torch.cuda.synchronize()
            check_out(f"out {s} {d} rrc={use_rrc}")
            check_sums(f"sums {s} {d} rrc={use_rrc}")
            want, s_ref = _want(s, d, "rrc" if use_rrc else ("aug", "reflect", 0), _color_records(B), _blur_records(B, 2), _erase_records(d, B),
                                None if m is None else _mix_records(d, B))
            assert torch.equal(out.view(B, 3, d, d).cpu(), want)     # every element stored: none is the sentinel
            assert (sums.cpu().to(torch.int64) & 0xffffffff).flatten().tolist() == s_ref.tolist()


@pytest.mark.parametrize("crop", [False, True], ids=["augment", "crop"])
def test_loader_with_three_augment_does_not_synchronise(crop):
    n, bs = 20, 8
    rng = np.random.default_rng(79)
    imgs, labels = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, n)
    tr = _case(32, 224)[0]
    a, c, m = qat_vit_amd.RandomCropFlip(4), qat_vit_amd.RandomResizedCrop(), qat_vit_amd.MixupCutmix(mode="elem")
    e, t = qat_vit_amd.RandomErasing(p=0.6), qat_vit_amd.ThreeAugment()
    front = {"crop": c} if crop else {"augment": a}
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, mix=m, erase=e, three_augment=t, generator=torch.Generator().manual_seed(12),
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
        got = list(loader)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    g = torch.Generator().manual_seed(12)                            # the expectation: plan, words / windows, mix, erase, then colour and blur records
    src = torch.from_numpy(imgs).cuda()
    plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
    w = c.draw(n, 32, g) if crop else a.draw(n, g)
    recs, boxes = m.draw([len(b) for b in plan], 224, g), e.draw(n, 224, g)
    cols, blurs = t.draw(n, g)
    assert 0 < int((blurs[:, 0] & 1).sum()) < n and len(got) == len(plan) == 3
    o = 0
    for (x, y, idx, r), b in zip(got, plan):
        sl = slice(o, o + len(b))
        o += len(b)
        assert torch.equal(idx.cpu(), b) and torch.equal(y.cpu(), torch.from_numpy(labels)[b]) and torch.equal(r.cpu(), recs[sl])
        kw = {"rrc": w[sl].cuda()} if crop else {"aug": w[sl].cuda(), "padding_mode": a.padding_mode, "fill": a.fill}
        direct = tr(src, idx, mix=recs[sl].cuda(), erase=boxes[sl].cuda(), color=cols[sl].cuda(), blur=blurs[sl].cuda(), **kw)
        assert torch.equal(x.view(torch.int32), direct.view(torch.int32))                        # a direct call with the drawn records
        if bool((blurs[sl, 0] & 1).any()):                           # a batch with a blurred sample differs from the call without blur records
            assert not torch.equal(x, tr(src, idx, mix=recs[sl].cuda(), erase=boxes[sl].cuda(), color=cols[sl].cuda(), **kw))
    # the first batch against the host references
    b = plan[0]
    u8 = rrc_ref.host_rrc(imgs[b.numpy()], w[:8].numpy(), 224) if crop else \
        rrc_ref.host_rrc(augment_ref.host_augmented(imgs[b.numpy()], w[:8], a.padding_mode, a.fill), [rrc_ref.pack(0, 0, 32, 32, False)] * 8, 224)
    cb, _ = blur_ref.apply_batch(u8, cols[:8].numpy(), blurs[:8].numpy())
    x = mix_ref.mixed_images(erase_ref.erased(color_ref.normalized(cb, tr.table.cpu().numpy()), boxes[:8].numpy()), recs[:8].numpy())
    assert torch.equal(got[0][0].cpu(), torch.from_numpy(x))


def test_refusals():
    tr, _, src, _ = _case(32, 224)
    B = BATCH[(32, 224)]
    r = _t(_blur_records(B))
    for bad in (r.long(), r[:3], r.cpu(), r[:, :3], torch.zeros(B, 8, dtype=torch.int32, device="cuda")[:, ::2], r.flatten()):
        for kw in ({}, {"mix": _t(_mix_records(224, B))}, {"rrc": _windows(32, B).cuda()}):
            with pytest.raises(ValueError, match="blur must be"):
                tr(src, blur=bad, **kw)
    big = qat_vit_amd.GpuResizeNormalize(32, out_size=384)           # above 64 KB of LDS: refused under the entry's name before any launch
    with pytest.raises(RuntimeError, match="qatvit_image_batch_blur: source 32 -> output 384 needs 85248 bytes of LDS"):
        big(src, blur=r)
