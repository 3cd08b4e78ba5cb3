"""RandomErasing inside the batch launch (qatvit_image_batch_erase / qatvit_image_batch_rrc_erase through GpuResizeNormalize(erase=...) and
GpuImageLoader(erase=...)) on an MI355X.  Constant fills EQUAL, bit for bit, tests/erase_ref.py applied to what the existing entries write; the
noise equals the fp64 evaluation of include/qatvit.h's formula within NOISE_BOUND; under mix records the batch is tests/mix_ref.py's composition
of the ERASED batch, the partner erased by its own record."""
import math

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from tests import erase_ref, mix_ref
from tests.erase_ref import pack
from tests.test_gpu_mix import _records as _mix_records
from tests.test_gpu_rrc import _mix_case as _windows

pytestmark = pytest.mark.gpu

# The largest deviation of the kernel's noise from the fp64 evaluation of the same formula, measured on an MI355X over every noise element this file
# compares (4.88e-7) and over the 1.2 million elements of eight whole-image records in tools/bench_input_pipeline.py --erase (6.08e-7, at z = 4.35;
# profiles/erase_bench.txt): the rounding of logf, sqrtf, cospif / sinpif and one product in fp32 at |z| up to 5.1.  Asserted at four times the
# larger, since those functions may differ by a few ulp between ROCm releases; a wrong counter or key is off by order 1.
NOISE_MEASURED = 6.083e-7
NOISE_BOUND = 4 * NOISE_MEASURED
assert NOISE_BOUND < 1e-5

SIZES = [(32, 224), (8, 36), (37, 224)]                              # the DT = 224 forms; DT = 0 with a last band of 4 rows; odd source rows
ARMS = [None, ("constant", 131), ("reflect", 0)]                     # no words, words in both padding modes
B = 16                                                               # the batch of the mix records of tests/test_gpu_mix.py
KEY_A, KEY_B = (0x243f6a88, 0x85a308d3), (7, 0xffffffff)
_cache, _fields = {}, {}


def _field(key, D):
    """erase_ref.noise(key, D) in fp64, formed once per key and size and never changed."""
    if (key, D) not in _fields:
        _fields[(key, D)] = erase_ref.noise(key, D)
    return _fields[(key, D)]


def _case(s, d):
    """Per size, built once and never changed: transform, images on the device, words (host)."""
    if (s, d) not in _cache:
        rng = np.random.default_rng(s)
        words = qat_vit_amd.RandomCropFlip(padding=4).draw(B, torch.Generator().manual_seed(s))
        _cache[(s, d)] = (qat_vit_amd.GpuResizeNormalize(s, out_size=d), torch.from_numpy(rng.integers(0, 256, (B, s, s, 3), dtype=np.uint8)).cuda(), words)
    return _cache[(s, d)]


def _kw(arm, words):
    return {} if arm is None else {"aug": words.cuda(), "padding_mode": arm[0], "fill": arm[1]}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(torch.as_tensor(b).cpu()))


def _boxes(D):
    """(y0, y1, x0, x1); the comments name what each is there for."""
    last = (D - 1) // 16 * 16                                        # the first row of the last band (D = 36: rows 32 .. 35)
    return [(0, D, 0, D),                                            # the whole image
            (D // 2 + 1, D // 2 + 2, D // 2 - 3, D // 2 - 2),        # 1 x 1
            (3, 29, 5, D - 3),                                       # edges off the float4 grid, across a band boundary
            (14, 18, 6, 10),                                         # two rows on either side of a band boundary
            (last + 1, D - 1, 1, D - 2),                             # wholly inside the last band, short at D = 36
            (D - 10, 65535, D - 7, 40000),                           # given beyond D: clamped
            (20, 10, 3, 30),                                         # y1 < y0: empty
            (0, 0, 0, 0)]                                            # the identity


def _const_records(D):
    fills = [(0.0, 0.0, 0.0), (1.5, -2.0, -0.0)]                     # timm's const; a negative value and -0.0 (compared by bits)
    recs = [pack(*box, fills[k & 1]) for k, box in enumerate(_boxes(D) + _boxes(D)[::-1])]
    assert len(recs) == B
    return torch.tensor(recs, dtype=torch.int32)


def _close_to_noise(got, want, mask, weight=1.0, slack=None):
    """Inside `mask` |got - want| <= weight * NOISE_BOUND (+ slack); outside it the values are equal (as torch.equal has it: the composition of
    tests/mix_ref.py gives fl(1 * -0.0) + fl(0 * x) = +0.0 where the kernel's identity bands store -0.0).  Prints the largest deviation."""
    got, want = got.cpu().numpy(), np.asarray(want)
    assert np.array_equal(got[~mask], want.astype(np.float32)[~mask])
    dev = np.abs(got.astype(np.float64) - want)[mask]
    tol = (np.broadcast_to(weight, got.shape)[mask] * NOISE_BOUND + (0.0 if slack is None else slack[mask]))
    print(f"noise: {mask.sum()} elements, largest deviation {dev.max():.3e} (bound {NOISE_BOUND:.2e}), largest deviation / tolerance {np.max(dev / tol):.3f}")
    assert np.all(dev <= tol), float(np.max(dev / tol))


@pytest.mark.parametrize("arm", ARMS, ids=["nowords", "constant", "reflect"])
@pytest.mark.parametrize("s,d", SIZES)
def test_constant_fill_equals_the_erased_batch(s, d, arm):
    tr, src, words = _case(s, d)
    kw, recs = _kw(arm, words), _const_records(d)
    X = tr(src, **kw)
    want = torch.from_numpy(erase_ref.erased(X.cpu().numpy(), recs))
    got = tr(src, erase=recs.cuda(), **kw)
    assert got.shape == (B, 3, d, d) and got.dtype == torch.float32 and got.is_contiguous()
    assert _same_bits(got, want)
    Xc = X.cpu()
    assert _same_bits(want[6], Xc[6]) and _same_bits(want[7], Xc[7]) and not torch.equal(want[1], Xc[1]) and not torch.equal(want[4], Xc[4])
    assert bool((want[0] == 0).all()) and _same_bits(want[15][1], torch.full((d, d), -2.0)) and _same_bits(want[15][2], torch.full((d, d), -0.0))


@pytest.mark.parametrize("s,d", SIZES)
def test_noise_is_the_stated_function_of_key_channel_row_and_column(s, d):
    tr, src, words = _case(s, d)
    boxes = _boxes(d)
    recs = [pack(0, d, 0, d, mode=1, key=KEY_A), pack(0, d, 0, d, mode=1, key=KEY_B)]
    recs += [pack(*box, (9.0, 9.0, 9.0), mode=1, key=KEY_A if k & 1 else KEY_B) for k, box in enumerate(boxes[1:])]       # the fill is unused
    recs += [pack(0, d, 0, d, mode=1, key=KEY_A)] + [[0] * 8] * (B - 10)
    recs = torch.tensor(recs, dtype=torch.int32)
    fields = {k: _field(k, d) for k in (KEY_A, KEY_B)}
    for kw in ({}, _kw(ARMS[2], words)):
        X = tr(src, **kw)
        got = tr(src, erase=recs.cuda(), **kw)
        # fp64 inside the boxes, X outside them
        want, mask = X.cpu().numpy().astype(np.float64), erase_ref.box_mask(recs, d)
        for b, rec in enumerate(recs.tolist()):
            if mask[b].any():
                want[b][mask[b]] = fields[erase_ref.unpack(rec)[6]][mask[b]]
        _close_to_noise(got, want, mask)
        assert _same_bits(got[0], got[9]) and not torch.equal(got[0], got[1])        # one key at two positions: equal bits; two keys differ
        assert _same_bits(got[3][:, 3:29, 5:d - 3], got[0][:, 3:29, 5:d - 3])          # a box shows the same field as the whole image
        z = got[0].double()
        n = z.numel()
        assert abs(float(z.mean())) < 5 / math.sqrt(n) and abs(float(z.std()) - 1) < 5 / math.sqrt(2 * n)


@pytest.mark.parametrize("s,d", SIZES)
def test_identity_records_and_no_records_are_the_existing_calls(s, d):
    tr, src, words = _case(s, d)
    ident = torch.zeros(B, 8, dtype=torch.int32, device="cuda")
    mix, rrc = _mix_records(d).cuda(), _windows(s, d).cuda()
    for kw in [_kw(arm, words) for arm in ARMS] + [{"mix": mix}, dict(_kw(ARMS[1], words), mix=mix), {"rrc": rrc}, {"rrc": rrc, "mix": mix}]:
        X = tr(src, **kw)
        assert torch.equal(tr(src, erase=None, **kw), X)
        buf = torch.full_like(X, float("nan"))
        assert tr(src, out=buf, erase=ident, **kw) is buf and _same_bits(buf, X)
    # the C entries with erase == NULL launch the existing entries' kernels
    L, w = data.native.lib(), words.cuda()
    for aug, m in ((w, mix), (None, mix), (w, None), (None, None)):
        want = tr(src, **({} if aug is None else {"aug": aug, "padding_mode": "reflect"}), **({} if m is None else {"mix": m}))
        out = torch.full_like(want, float("nan"))
        data.native.check(L.qatvit_image_batch_erase(src.data_ptr(), None, B, B, s, d, tr.coeffs.data_ptr(), tr.table.data_ptr(),
                                                     None if aug is None else aug.data_ptr(), 1, 200, None if m is None else m.data_ptr(), None,
                                                     out.data_ptr(), data.native.stream_ptr()), "erase")
        assert _same_bits(out, want)
    for m in (mix, None):
        want = tr(src, rrc=rrc, mix=m)
        out = torch.full_like(want, float("nan"))
        data.native.check(L.qatvit_image_batch_rrc_erase(src.data_ptr(), None, B, B, s, d, tr.window_tables().data_ptr(), tr.table.data_ptr(),
                                                         rrc.data_ptr(), None if m is None else m.data_ptr(), None, out.data_ptr(),
                                                         data.native.stream_ptr()), "rrc_erase")
        assert _same_bits(out, want)


@pytest.mark.parametrize("s,d", [(32, 224), (8, 36)])
def test_record_b_goes_with_batch_position_b(s, d):
    tr, src, words = _case(s, d)
    g = torch.Generator().manual_seed(s)
    index = torch.cat([torch.randperm(B, generator=g)[:10], torch.randint(0, B, (6,), generator=g)])      # permuted, then repeating
    assert len(set(index.tolist())) < B
    recs = _const_records(d).flip(0).contiguous()                    # reversed records
    kw = dict(aug=words.cuda(), padding_mode="constant", fill=7)
    X = tr(src, index.cuda(), **kw)
    want = erase_ref.erased(X.cpu().numpy(), recs)
    buf = torch.full((B, 3, d, d), float("nan"), device="cuda")
    assert tr(src, index.cuda(), out=buf, erase=recs.cuda(), **kw) is buf and _same_bits(buf, want)
    assert not torch.equal(buf, tr(src, index.cuda(), erase=recs.flip(0).contiguous().cuda(), **kw))


@pytest.mark.parametrize("s,d", SIZES)
def test_a_malformed_record_gives_the_clamped_records_result(s, d):
    tr, src, words = _case(s, d)
    good = pack(2, 9, 3, 13, (0.25, 0.5, -1.0))
    bad = [good,
           [-1] * 8,                                                 # all bits set: the whole image, noise, key ffffffff ffffffff
           pack(0, 0xffff, 0, 0xffff, (1.0, 2.0, 3.0), mode=6),      # bounds far beyond D; bits 1 and 2 of the mode alone: constant
           pack(5, 0xffff, d, 0xffff, mode=7),                       # x0 = D: empty after the clamp
           pack(d - 1, d + 1, d - 1, 0x8000, (4.0, 4.0, 4.0), mode=-2),   # one element in the corner; every mode bit but bit 0
           pack(0xffff, 0xffff, 0, d),                               # y0 = y1 = D after the clamp: empty
           [-(1 << 31), -(1 << 31), 0, 0, 0, -(1 << 31), 0, 0],      # bit 31 of the box words: y1 = x1 = 32768 -> D, y0 = x0 = 0; mode bit 0 clear
           good]
    fixed = [erase_ref.clamped(r, d) for r in bad]
    assert fixed[0] == good and fixed[1] == pack(d, d, d, d)[:2] + [-1, -1, -1, 1, -1, -1] and fixed[5][:2] == pack(d, d, 0, d)[:2]
    assert fixed[6][:2] == pack(0, d, 0, d)[:2] and fixed[6][5] == 0 and fixed[4][5] == 0 and fixed[3][5] == 1
    n = len(bad)
    sub = src[:n].contiguous()
    X = tr(sub)
    got = tr(sub, erase=torch.tensor(bad, dtype=torch.int32).cuda())
    assert _same_bits(got, tr(sub, erase=torch.tensor(fixed, dtype=torch.int32).cuda()))
    want = erase_ref.erased(X.cpu().numpy(), fixed, fields={(0xffffffff, 0xffffffff): np.zeros((3, d, d))})
    assert _same_bits(got[2:], want[2:]) and _same_bits(got[0], want[0])
    assert _same_bits(got[1], X[1])                                  # all bits set clamps to y0 = y1 = D: empty
    assert _same_bits(got[3], X[3]) and _same_bits(got[5], X[5]) and bool((got[6] == 0).all()) and float(got[4][0, d - 1, d - 1]) == 4.0
    alone = tr(sub, erase=torch.tensor([good] * n, dtype=torch.int32).cuda())
    assert _same_bits(got[0], alone[0]) and _same_bits(got[-1], alone[-1])                       # the neighbours are unaffected


def _erase_under_mix(D):
    """One erase record per position of tests/test_gpu_mix.py's 16 mix records (partners 0 -> 1 -> 2 -> 0, 3 -> 4, 4 -> 5 .. 9 -> 10, 10 -> 10,
    11 and 12 -> themselves, 13 -> 3 unmixed, 14 -> 15, 15 -> 0 with weight 0): the sample, the partner, both or neither erased."""
    none = [0] * 8
    recs = [pack(10, 60, 8, 30, (0.5, -0.5, 2.0)),                   # 0: the chain; its partner 1 is a noise partner, and 2's partner 0 is this box
            pack(5, 33, 18, D - 2, mode=1, key=KEY_A),               # 1: noise, as the sample and as the partner of 0
            none,                                                    # 2: only its partner is erased
            none,                                                    # 3: all partner (lam 0), and the partner is erased
            pack(0, 17, 0, 17, (1.0, 1.0, 1.0)),                     # 4: whole-image cutmix: nothing of its own box survives
            none,                                                    # 5: neither (its 1 x 1 box takes an element of 6 outside the box of 6)
            pack(10, 40, 2, 14, (-1.0, -2.0, -3.0)),                 # 6: cutmix box (3..29, 5..D-3) over both erase boxes: this one ...
            pack(0, 20, 30, D, mode=1, key=KEY_B),                   # 7: ... and the partner's noise
            none, none,                                              # 8, 9: neither
            pack(D - 20, D, 0, D, (0.75, 0.75, 0.75)),               # 10: mixup with itself: fl(lam E) + fl((1 - lam) E)
            pack(1, D - 1, 1, D - 1, mode=1, key=KEY_B),             # 11: noise, partner outside the batch = itself
            pack(25, 75, 25, 75, (3.0, 3.0, 3.0)),                   # 12: cutmix with itself over its own erase box
            pack(0, D, 0, 7, (-0.0, -0.0, -0.0)),                    # 13: the identity mix record: the output is E[13]
            pack(30, 110, 0, 9, mode=1, key=KEY_A),                  # 14: a blend and a box, noise, with ...
            pack(35, 60, 2, 5, (2.0, 0.0, -2.0))]                    # 15: ... a constant partner; 15 itself has w_self 0.5 and no partner
    assert len(recs) == B
    return torch.tensor(recs, dtype=torch.int32)


def _check_mixed(got, X, er, mix, d):
    """got == mix_ref.mixed_images(E) with E = erase_ref.erased(X, er), its noise the fp64 field rounded to fp32: bitwise where no noise
    element takes part; elsewhere within the bound carried through the blend.  A noise element of E is within NOISE_BOUND + 2^-22 of the
    kernel's (the rounding of a |z| < 8 to fp32), so an element taken from a cutmix box is too, and a blended one is within
    (|w_self| [own is noise] + |w_partner| [partner's is noise]) times that, plus the roundings of the two products and the sum in both
    evaluations, 4 * 2^-24 (|w_self E[b]| + |w_partner E[p]|) to first order."""
    E = erase_ref.erased(X.cpu().numpy(), er, fields={k: _field(k, d) for k in (KEY_A, KEY_B)})
    want = mix_ref.mixed_images(E, mix)
    noisy = erase_ref.box_mask(er, d) & np.array([erase_ref.unpack(r)[5] == 1 for r in er.tolist()])[:, None, None, None]
    mask, weight, slack = np.zeros_like(noisy), np.zeros(E.shape), np.zeros(E.shape)
    for b, rec in enumerate(mix.tolist()):
        p = mix_ref.partner_of(rec, b, B)
        _, ws, wp, (y0, y1, x0, x1), _ = mix_ref.fields(rec, B, d)
        ws, wp = abs(float(ws)), abs(float(wp))
        weight[b] = ws * noisy[b] + wp * noisy[p]
        mask[b] = weight[b] != 0
        slack[b] = 4 * 2.0 ** -24 * (ws * np.abs(E[b]) + wp * np.abs(E[p]))
        if y1 > y0 and x1 > x0:                                      # inside the box the partner's element is taken as it is
            box = (slice(None), slice(y0, y1), slice(x0, x1))
            weight[b][box], mask[b][box], slack[b][box] = noisy[p][box], noisy[p][box], 0.0
    slack += weight * 2.0 ** -22
    assert mask.any() and not mask.all()
    _close_to_noise(got, want.astype(np.float64), mask, weight, slack)
    return E, want


@pytest.mark.parametrize("arm", [None, ("reflect", 0)], ids=["nowords", "reflect"])
@pytest.mark.parametrize("s,d", SIZES)
def test_mix_blends_the_erased_sample_with_the_erased_partner(s, d, arm):
    tr, src, words = _case(s, d)
    kw, mix, er = _kw(arm, words), _mix_records(d), _erase_under_mix(d)
    X = tr(src, **kw)
    got = tr(src, mix=mix.cuda(), erase=er.cuda(), **kw)
    assert got.shape == (B, 3, d, d) and got.dtype == torch.float32 and got.is_contiguous()
    E, want = _check_mixed(got, X, er, mix, d)
    plain = tr(src, mix=mix.cuda(), **kw).cpu()
    assert _same_bits(got[3], E[4]) and _same_bits(got[4], E[5]) and _same_bits(got[13], E[13])      # all partner; the whole image; identity
    assert _same_bits(got[8], plain[8]) and _same_bits(got[9], plain[9]) and _same_bits(got[5], plain[5])      # neither side erased
    assert not torch.equal(got[2].cpu(), plain[2]) and not torch.equal(got[0].cpu(), plain[0])               # the partner's box shows in the blend
    # const only, every position erased, the sample and its partner: torch.equal
    const = _const_records(d)
    assert torch.equal(tr(src, mix=mix.cuda(), erase=const.cuda(), **kw).cpu(),
                       torch.from_numpy(mix_ref.mixed_images(erase_ref.erased(X.cpu().numpy(), const), mix)))


@pytest.mark.parametrize("s,d", SIZES)
def test_rrc_and_rrc_mix_erase_their_own_windows(s, d):
    tr, src, words = _case(s, d)
    r, mix, er, const = _windows(s, d).cuda(), _mix_records(d), _erase_under_mix(d), _const_records(d)
    X = tr(src, rrc=r)
    assert _same_bits(tr(src, rrc=r, erase=const.cuda()), erase_ref.erased(X.cpu().numpy(), const))
    fields = {k: _field(k, d) for k in (KEY_A, KEY_B)}
    noisy = erase_ref.box_mask(er, d) & np.array([erase_ref.unpack(q)[5] == 1 for q in er.tolist()])[:, None, None, None]
    _close_to_noise(tr(src, rrc=r, erase=er.cuda()), _erased64(X, er, fields, d), noisy)
    assert torch.equal(tr(src, rrc=r, mix=mix.cuda(), erase=const.cuda()).cpu(),
                       torch.from_numpy(mix_ref.mixed_images(erase_ref.erased(X.cpu().numpy(), const), mix)))
    _check_mixed(tr(src, rrc=r, mix=mix.cuda(), erase=er.cuda()), X, er, mix, d)


def _erased64(X, er, fields, d):
    """E in fp64: X (exact in fp64) outside the boxes, the constant fills, and the fp64 noise field itself inside the noise boxes."""
    want, mask = erase_ref.erased(X.cpu().numpy(), er, fields).astype(np.float64), erase_ref.box_mask(er, d)
    for b, rec in enumerate(er.tolist()):
        if erase_ref.unpack(rec)[5] and mask[b].any():
            want[b][mask[b]] = fields[erase_ref.unpack(rec)[6]][mask[b]]
    return want


@pytest.mark.parametrize("crop", [False, True], ids=["augment", "crop"])
def test_loader_draws_the_records_last_and_does_not_synchronise(crop):
    n, bs = 40, 16
    rng = np.random.default_rng(77)
    imgs, labels = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, n)
    tr = _case(32, 224)[0]
    a, c, m = qat_vit_amd.RandomCropFlip(4), qat_vit_amd.RandomResizedCrop(), qat_vit_amd.MixupCutmix(mode="elem")
    e = qat_vit_amd.RandomErasing(p=0.6, value="random")
    front = {"crop": c} if crop else {"augment": a}
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, mix=m, erase=e, generator=torch.Generator().manual_seed(12),
                                        return_index=True, transform=tr, **front)
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
    g = torch.Generator().manual_seed(12)                            # the expectation: plan, words / windows, mix records, erase records
    src, seen = torch.from_numpy(imgs).cuda(), []
    for got in epochs:
        plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
        w = c.draw(n, 32, g) if crop else a.draw(n, g)
        recs = m.draw([len(b) for b in plan], 224, g)
        boxes = e.draw(n, 224, g)
        seen.append(boxes)
        assert len(got) == len(plan) == 3 and [len(b) for b in plan] == [16, 16, 8] and boxes.any(1).sum() > 10
        o = 0
        for (x, y, idx, r), b in zip(got, plan):
            sl = slice(o, o + len(b))
            o += len(b)
            assert torch.equal(idx.cpu(), b) and idx.dtype == torch.int64 and torch.equal(y.cpu(), torch.from_numpy(labels)[b])
            assert r.dtype == torch.int32 and r.shape == (len(b), 6) and r.is_cuda and r.is_contiguous() and torch.equal(r.cpu(), recs[sl])
            kw = {"rrc": w[sl].cuda()} if crop else {"aug": w[sl].cuda(), "padding_mode": a.padding_mode, "fill": a.fill}
            assert _same_bits(x, tr(src, idx, mix=recs[sl].cuda(), erase=boxes[sl].cuda(), **kw))        # a direct call with the drawn records
            assert not torch.equal(x, tr(src, idx, mix=recs[sl].cuda(), **kw))
    assert not torch.equal(seen[0], seen[1])                         # the second epoch draws new records
    # with erase set, the plan, the words / windows and the mix records are those of the same seed without it
    old = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, mix=m, generator=torch.Generator().manual_seed(12), return_index=True,
                                     transform=tr, **front)
    for (x, y, idx, r), (x2, y2, idx2, r2) in zip(list(old), epochs[0]):
        assert torch.equal(idx, idx2) and torch.equal(y, y2) and torch.equal(r, r2) and x.shape == x2.shape
    # the tuple forms are the loader's without erase; alone, erase draws nothing but its records behind a sequential plan
    for ret, mix, length in ((False, m, 3), (True, None, 3), (False, None, 2)):
        first = next(iter(qat_vit_amd.GpuImageLoader(imgs, labels, bs, mix=mix, erase=e, generator=torch.Generator().manual_seed(3), transform=tr,
                                                     return_index=ret)))
        assert len(first) == length and first[0].shape == (16, 3, 224, 224) and first[1].shape == (16,)
        if mix is None:
            boxes = e.draw(n, 224, torch.Generator().manual_seed(3))
            assert _same_bits(first[0], tr(src[:16].contiguous(), erase=boxes[:16].cuda()))


def test_refusals():
    tr, src, words = _case(32, 224)
    r = _const_records(224).cuda()
    for bad in (r.long(), r[:5], r.cpu(), r[:, :6], torch.zeros(B, 16, dtype=torch.int32, device="cuda")[:, ::2], r.flatten()):
        for kw in ({}, {"mix": _mix_records(224).cuda()}, {"rrc": _windows(32, 224).cuda()}):
            with pytest.raises(ValueError, match="erase must be"):
                tr(src, erase=bad, **kw)
    with pytest.raises(ValueError, match="mix must be"):
        tr(src, erase=r, mix=torch.zeros(B, 5, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError, match="RandomErasing"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 32, 32, 3), np.uint8), np.zeros(4, np.int64), 2, transform=tr, erase="pixel")
