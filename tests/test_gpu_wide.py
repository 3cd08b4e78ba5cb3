"""The window stage and the two-stage wide transform (qatvit_image_window_u8 through GpuWindowResize, GpuWideResizeNormalize and
GpuImageLoader) on an MI355X: stage 1 EQUALS the bytes that tests/wide_ref.py forms on the host by crop, mirror and the two-pass resample with
stretched filters, and the stored Pillow bytes of tests/golden/wide_kat.npz; where both apply, the two-stage path EQUALS the one-launch path of
GpuResizeNormalize, with every kind of record; and the loader over a rectangular source equals the composition of the host references."""
import os

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from qat_vit_amd.vit import VisionTransformer
from tests import color_ref, erase_ref, mix_ref, wide_ref
from tests.kernel_check import Guarded
from tests.test_gpu_mix import _records as _mix_records
from tests.wide_ref import host_window, pack

pytestmark = pytest.mark.gpu

D = wide_ref.D_SMALL
_cache = {}


def _case(H, W):
    """Per source size at D = 32, built once and never changed: stage, images (host, device), corner + 16 drawn records (host, device), the
    expected bytes."""
    if (H, W) not in _cache:
        drawn = qat_vit_amd.RandomResizedCrop().draw(16, (H, W), torch.Generator().manual_seed(1000 * H + W))
        recs = torch.cat([torch.tensor(wide_ref.corner_records(H, W, D), dtype=torch.int32), drawn])
        imgs = wide_ref.images(len(recs), H, W, 100 * H + W)
        _cache[(H, W)] = (qat_vit_amd.GpuWindowResize((H, W), out_size=D), imgs, torch.from_numpy(imgs).cuda(), recs, recs.cuda(),
                          torch.from_numpy(host_window(imgs, recs, D)))
    return _cache[(H, W)]


def _guarded_u8(B, d):
    g = Guarded(B * d, d * 3, torch.uint8, "cuda", pad=256)          # [B, d, d, 3] as rows of one output row each, canary rows around it
    return g.t.view(B, d, d, 3), g.check


@pytest.mark.parametrize("H,W", wide_ref.SMALL)
def test_stage_one_equals_the_host_window_and_leaves_the_canaries(H, W):
    st, imgs, src, recs, r, want = _case(H, W)
    fields = [wide_ref.unpack(v) for v in recs[:-16].tolist()]
    for axis, side in ((0, H), (1, W)):                              # every listed side on either axis, the four corners, both flips
        assert {f[2 + axis] for f in fields} == set(wide_ref.side_values(side, D))
        assert any(f[axis] == 0 and f[2 + axis] < side for f in fields) and any(f[axis] == side - f[2 + axis] > 0 for f in fields)
    assert {f[4] for f in fields} == {False, True} and st.tables.shape == (max(H, W), 19 * D) and st.tables.is_cuda
    out, check = _guarded_u8(len(recs), D)
    assert st(src, rrc=r, out=out) is out
    torch.cuda.synchronize()
    check(f"stage 1 {H} x {W}")
    assert torch.equal(out.cpu(), want)                              # every byte stored: a skipped dword would hold the sentinel ff ff ff ff
    got = st(src, rrc=r)
    assert got.shape == (len(recs), D, D, 3) and got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got.cpu(), want)


def test_stage_one_equals_pillows_stored_bytes():
    z = wide_ref.load()
    for H, W in wide_ref.SMALL:
        image, records, pillow = (z[f"{k}_{H}_{W}_{D}"] for k in ("image", "records", "out"))
        src = torch.from_numpy(image[None]).cuda()
        index = torch.zeros(len(records), dtype=torch.int64, device="cuda")
        got = _case(H, W)[0](src, index, rrc=torch.from_numpy(records).cuda())
        assert torch.equal(got.cpu(), torch.from_numpy(pillow)), (H, W)


def test_256_to_224_equals_pillow_and_the_host_window():
    (H, W), d = wide_ref.BIG
    z = wide_ref.load()
    image, pillow = z[f"image_{H}_{W}_{d}"], z[f"out_{H}_{W}_{d}"]
    recs = [pack(0, 0, H, W, False), pack(3, 29, 250, 225, True), pack(H - 224, 0, 224, 256, False), pack(31, W - 111, 225, 111, True)]
    st = qat_vit_amd.GpuWindowResize((H, W), out_size=d, window=(3, 29, 250, 225))
    src = torch.from_numpy(image[None]).cuda()
    index = torch.zeros(len(recs), dtype=torch.int64, device="cuda")
    out, check = _guarded_u8(len(recs), d)
    st(src, index, rrc=torch.tensor(recs, dtype=torch.int32).cuda(), out=out)
    torch.cuda.synchronize()
    check("stage 1 256 -> 224")
    assert torch.equal(out[0].cpu(), torch.from_numpy(pillow[0]))
    assert torch.equal(out.cpu(), torch.from_numpy(host_window([image] * len(recs), recs, d)))
    default = host_window([image], [pack(3, 29, 250, 225, False)], d)                                     # rrc=None: the default window, not mirrored
    assert torch.equal(st(src).cpu(), torch.from_numpy(default)) and st.default_records(1) is st.default_records(1)


def test_a_side_whose_table_has_a_five_tap_row():
    """12 -> 44: the rounding of the doubles gives some outputs a fifth tap, of coefficient 0 (tests/test_wide_abi.py holds the restatement
    equal to Pillow there).  Windows of that side on either axis, and on both."""
    H, W, d = 48, 20, 44
    assert wide_ref.tables(12, d)[1].max() == 5
    st = qat_vit_amd.GpuWindowResize((H, W), out_size=d)
    imgs = wide_ref.images(6, H, W, 44)
    recs = [pack(3, 2, 12, 12, False), pack(0, 8, 40, 12, True), pack(36, 0, 12, 20, False), pack(36, 8, 12, 12, True), pack(0, 0, H, W, False),
            pack(1, 1, 12, 13, True)]
    out, check = _guarded_u8(len(recs), d)
    st(torch.from_numpy(imgs).cuda(), rrc=torch.tensor(recs, dtype=torch.int32).cuda(), out=out)
    torch.cuda.synchronize()
    check("stage 1 48 x 20 -> 44")
    assert torch.equal(out.cpu(), torch.from_numpy(host_window(imgs, recs, d)))


def _late_records(B, d, seed, mode="pixel"):
    """Erase and colour records on the device.  Pixel noise where two device paths are compared; constant fills where the host reference is
    (the noise's float half follows the device's math library to a few ulp)."""
    g = torch.Generator().manual_seed(seed)
    erase = qat_vit_amd.RandomErasing(p=0.7, value=(0.5, -1.0, 2.0) if mode == "const" else 0, mode=mode).draw(B, d, g)
    color = qat_vit_amd.ColorJitter(0.4, 0.4, 0.4, grayscale=0.2, solarize=0.2).draw(B, g)
    return erase.cuda(), color.cuda()


@pytest.mark.parametrize("S", [32, 37])
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
def test_the_two_paths_agree_where_both_apply(S, mixed):
    d, B = 224, 16
    one, two = qat_vit_amd.GpuResizeNormalize(S, out_size=d), qat_vit_amd.GpuWideResizeNormalize((S, S), out_size=d)
    imgs = torch.from_numpy(wide_ref.images(24, S, S, S)).cuda()
    g = torch.Generator().manual_seed(S)
    index = torch.cat([torch.randperm(24, generator=g)[:10], torch.randint(0, 24, (6,), generator=g)]).cuda()
    r = torch.cat([torch.tensor(wide_ref.corner_records(S, S, d)[:8], dtype=torch.int32), qat_vit_amd.RandomResizedCrop().draw(8, S, g)]).cuda()
    m = _mix_records(d).cuda() if mixed else None
    e, c = _late_records(B, d, S)
    for kw in ({}, {"erase": e}, {"color": c}, {"erase": e, "color": c}, {"color": c, "contrast": False}):
        a, b = one(imgs, index, rrc=r, mix=m, **kw), two(imgs, index, rrc=r, mix=m, **kw)
        assert b.shape == (B, 3, d, d) and b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32)), sorted(kw)
    whole = torch.tensor([pack(0, 0, S, S, False)] * B, dtype=torch.int32).cuda()
    assert torch.equal(two(imgs, index), one(imgs, index)) and torch.equal(two(imgs, index), two(imgs, index, rrc=whole))
    assert (two.src_size, two.out_size, two.mean, two.std, two.device) == ((S, S), d, one.mean, one.std, one.device)


def test_record_b_goes_with_batch_position_b_and_image_index_b():
    H, W = 64, 48
    st, imgs, src, recs, _, _ = _case(H, W)
    n = len(recs)
    g = torch.Generator().manual_seed(5)
    index = torch.cat([torch.randperm(n, generator=g)[:20], torch.randint(0, n, (20,), generator=g)])        # permuted, then repeating
    assert len(set(index.tolist())) < 40
    br = torch.cat([recs, recs[:3].flip(0)])[:40]
    want = torch.from_numpy(host_window(imgs[index.numpy()], br, D))
    got = st(src, index.cuda(), rrc=br.cuda())
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(got, st(src, index.cuda(), rrc=br.flip(0).contiguous().cuda()))
    buf = torch.full((40, D, D, 3), 0xa5, dtype=torch.uint8, device="cuda")                                 # a preallocated out= is filled completely
    assert st(src, index.cuda(), rrc=br.cuda(), out=buf) is buf and torch.equal(buf.cpu(), want)
    tr = qat_vit_amd.GpuWideResizeNormalize((H, W), out_size=D)
    table = tr.inner.table.cpu().numpy()
    x = torch.full((40, 3, D, D), float("nan"), device="cuda")
    assert tr(src, index.cuda(), rrc=br.cuda(), out=x) is x
    assert torch.equal(x.cpu(), torch.from_numpy(color_ref.normalized(want.numpy(), table)))
    assert tr.staged(40) is tr.staged(40) and torch.equal(tr.staged(40), got)                               # one buffer per batch size, static


@pytest.mark.parametrize("H,W", [(64, 48), (37, 128)])
def test_a_malformed_record_gives_the_clamped_records_result(H, W):
    st, imgs, src, recs, _, _ = _case(H, W)
    good = recs[-1].tolist()
    bad = [good, [0, 0], pack(1, 2, 0, 3, True), pack(0, 0, H + 5, 0x7fff, False), pack(3, 1, 0x7fff, 2, True), pack(0xffff, W, 3, 4, False),
           pack(H - 2, 0xffff, 3, W - 1, True), [-1, -1], [-(1 << 31), -(1 << 31)], good]
    fixed = [wide_ref.clamped(r, H, W) for r in bad]
    assert fixed[0] == good and fixed[1] == pack(0, 0, 1, 1, False) and fixed[7] == pack(0, 0, H, W, True) and fixed[5] == pack(H - 3, W - 4, 3, 4, False)
    sub = src[:len(bad)].contiguous()
    got = st(sub, rrc=torch.tensor(bad, dtype=torch.int32).cuda())
    assert torch.equal(got.cpu(), torch.from_numpy(host_window(imgs[:len(bad)], fixed, D)))
    assert torch.equal(got, st(sub, rrc=torch.tensor(fixed, dtype=torch.int32).cuda()))
    far = torch.tensor([-5, 1 << 40, 2, 10 ** 9], dtype=torch.int64).cuda()                                # an index outside 0 .. N-1 is clamped
    rec4 = torch.tensor([good] * 4, dtype=torch.int32).cuda()
    assert torch.equal(st(sub, far, rrc=rec4), st(sub, torch.tensor([0, len(bad) - 1, 2, len(bad) - 1]).cuda(), rrc=rec4))


def test_canaries_around_the_staged_bytes_and_the_final_batch():
    H, W, B = 64, 48, 16
    _, imgs, src, recs, _, _ = _case(H, W)
    tr = qat_vit_amd.GpuWideResizeNormalize((H, W), out_size=D)
    staged, check_staged = _guarded_u8(B, D)
    tr._staged[B] = staged                                           # the buffer the transform owns for this batch size, with canaries around it
    final = Guarded(B * 3 * D, D, torch.float32, "cuda", pad=256)
    r, m = recs[-16:].cuda(), _mix_records(D).cuda()
    e, c = _late_records(B, D, 3, mode="const")
    sub = src[:B].contiguous()
    out = tr(sub, rrc=r, mix=m, erase=e, color=c, out=final.t.view(B, 3, D, D))
    torch.cuda.synchronize()
    check_staged("staged bytes")
    final.check("final batch")
    u8 = host_window(imgs[:B], r.cpu(), D)
    assert torch.equal(staged.cpu(), torch.from_numpy(u8))
    x = color_ref.normalized(color_ref.apply_batch(u8, c.cpu().tolist())[0], tr.inner.table.cpu().numpy())
    x = mix_ref.mixed_images(erase_ref.erased(x, e.cpu().tolist()), m.cpu())
    assert torch.equal(out.cpu(), torch.from_numpy(x))


def test_loader_over_a_rectangular_source_equals_the_host_composition_and_does_not_synchronise():
    H, W, n, bs = 64, 48, 20, 8
    rng = np.random.default_rng(78)
    imgs, labels = wide_ref.images(n, H, W, 9), rng.integers(0, 10, n)
    tr = qat_vit_amd.GpuWideResizeNormalize((H, W), out_size=D)
    c, m = qat_vit_amd.RandomResizedCrop(), qat_vit_amd.MixupCutmix(mode="elem")
    e, j = qat_vit_amd.RandomErasing(p=0.6), qat_vit_amd.ColorJitter(0.4, 0.4, 0.4, grayscale=0.2, solarize=0.2)

    def loader(seed):
        return qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, crop=c, mix=m, erase=e, color=j, transform=tr, return_index=True,
                                          generator=torch.Generator().manual_seed(seed))

    first, second = loader(12), loader(12)                          # (the constructor copies the data set to the device: outside the mode)
    for size in (8, 4):                                              # (made on first use: here, not under the mode below)
        tr.color_sums(size), tr.staged(size)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            first.labels.sum().item()                                # the mode is honoured: a synchronising call raises
        epochs = [[tuple(t.clone() for t in batch) for batch in first] for _ in range(2)]
        again = [tuple(t.clone() for t in batch) for batch in second]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert all(torch.equal(a, b) for x, y in zip(epochs[0], again) for a, b in zip(x, y))      # one seed, the same epoch
    assert not torch.equal(epochs[0][0][0], epochs[1][0][0])
    table = tr.inner.table.cpu().numpy()
    g = torch.Generator().manual_seed(12)                            # the expectation: plan, windows of (H, W), mix, erase, colour records
    for got in epochs:
        plan = qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=g)
        w, recs, boxes, cols = c.draw(n, (H, W), g), m.draw([len(b) for b in plan], D, g), e.draw(n, D, g), j.draw(n, g)
        assert len(got) == len(plan) == 3 and [len(b) for b in plan] == [8, 8, 4]
        o = 0
        for (x, y, idx, r), b in zip(got, plan):
            sl = slice(o, o + len(b))
            o += len(b)
            assert torch.equal(idx.cpu(), b) and torch.equal(y.cpu(), torch.from_numpy(labels)[b]) and torch.equal(r.cpu(), recs[sl])
            u8 = host_window(imgs[b.numpy()], w[sl], D)
            want = color_ref.normalized(color_ref.apply_batch(u8, cols[sl].tolist())[0], table)
            want = mix_ref.mixed_images(erase_ref.erased(want, boxes[sl].tolist()), recs[sl])
            assert torch.equal(x.cpu(), torch.from_numpy(want))
    plain = next(iter(qat_vit_amd.GpuImageLoader(imgs, labels, bs, transform=tr)))               # no crop: the default window
    assert torch.equal(plain[0].cpu(), torch.from_numpy(color_ref.normalized(host_window(imgs[:8], [pack(0, 0, H, W, False)] * 8, D), table)))


def test_teacher_table_with_a_wide_transform(native_lib, tmp_path):
    H, W = 24, 40
    torch.manual_seed(31)
    teacher = VisionTransformer(embed_dim=128, depth=2, num_heads=2, num_classes=10, img_size=32).cuda().eval()
    for p in teacher.parameters():
        p.requires_grad = False
    imgs = torch.from_numpy(wide_ref.images(20, H, W, 4)).cuda()
    labels = torch.arange(20).cuda() % 10
    window = qat_vit_amd.center_crop_window(H, W)
    assert window == (0, 8, 24, 24)
    tr = qat_vit_amd.GpuWideResizeNormalize((H, W), out_size=32, window=window)
    table = qat_vit_amd.TeacherLogitTable.build(teacher, imgs, transform=tr, batch_size=8, labels=labels)
    assert table.logits.shape == (20, 10) and table.meta["transform"] == ((H, W), 32, tr.mean, tr.std, window)
    idx = torch.tensor([3, 19, 0, 7]).cuda()
    with torch.no_grad():
        assert torch.equal(table.rows(idx), teacher(tr(imgs, idx)))
    path = os.path.join(str(tmp_path), "wide.pt")
    table.save(path)
    loaded = qat_vit_amd.TeacherLogitTable.load(path, teacher=teacher, data_u8=imgs, transform=tr, labels=labels)
    assert torch.equal(loaded.logits, table.logits) and loaded.meta["transform"] == table.meta["transform"]
    with pytest.raises(ValueError, match="transform differs"):       # another default window: the teacher saw other pixels
        qat_vit_amd.TeacherLogitTable.load(path, transform=qat_vit_amd.GpuWideResizeNormalize((H, W), out_size=32))
    with pytest.raises(ValueError, match="transform differs"):
        qat_vit_amd.TeacherLogitTable.load(path, transform=qat_vit_amd.GpuResizeNormalize(24, out_size=32))
