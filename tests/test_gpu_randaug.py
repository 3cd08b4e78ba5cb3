"""The RandAugment stage (qatvit_image_bytes_randaug through GpuBytesRandAugment and GpuWideResizeNormalize(randaug=...)) on an MI355X.  Every
comparison is exact, against Pillow's own bytes in tests/golden/randaug_kat.npz (tools/gen_randaug_golden.py); nothing here imports Pillow.
Batches hold three distinct images (four at 224); operands of the direct calls sit in guarded allocations."""
import hashlib

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data
from tests import randaug_ref as ref
from tests.kernel_check import Guarded

pytestmark = pytest.mark.gpu

_fix = {}


def _f():
    if not _fix:
        _fix.update(np.load(ref.GOLDEN))
    return _fix


def _run(imgs, records):
    """The entry itself on uint8 [B, D, D, 3] and int32 [B, layers, 16]: all three images guarded, bytes unchanged, out fully written."""
    B, D = imgs.shape[0], imgs.shape[1]
    bufs = [Guarded(B * D, D * 3, torch.uint8, "cuda", pad=256) for _ in range(3)]
    src, scratch, out = bufs
    src.t.copy_(torch.from_numpy(imgs).view(B * D, D * 3))
    recs = torch.from_numpy(np.ascontiguousarray(records, dtype=np.int32)).cuda()
    rc = data.native.lib().qatvit_image_bytes_randaug(src.t.data_ptr(), B, D, recs.data_ptr(), recs.shape[1], scratch.t.data_ptr(), out.t.data_ptr(),
                                                      data.native.stream_ptr())
    data.native.check(rc, "qatvit_image_bytes_randaug")
    torch.cuda.synchronize()
    for g, name in zip(bufs, ("bytes", "scratch", "out")):
        g.check(name)
    assert np.array_equal(src.t.cpu().numpy().reshape(imgs.shape), imgs)
    return out.t.cpu().numpy().reshape(imgs.shape)


@pytest.mark.parametrize("D", ref.SIZES)
def test_every_op_equals_pillows_bytes(D):
    f = _f()
    imgs, records, want = ref.images(3, D, int(f[f"seed_{D}"])), f[f"records_{D}"], f[f"out_{D}"]
    assert sorted(set(records[:, 0])) == list(range(1, 16)) and {2, 3} <= set(records[records[:, 0] >= 11, 1])
    for k, rec in enumerate(records):
        got = _run(imgs, np.broadcast_to(rec, (3, 1, 16)))
        assert np.array_equal(got, want[k]), (D, k, rec[:4], np.argwhere(got != want[k])[:4])


@pytest.mark.parametrize("batch", range(4))
def test_chains_of_two_and_three_layers(batch):
    """Histogram op behind geometric op and the reverse, a no-op layer in the middle; two live layers start in scratch, three in out."""
    f = _f()
    records = f["chain_records"][batch]
    assert {2, 3} <= set((f["chain_records"][..., 0] != 0).sum(2).ravel())
    assert np.array_equal(_run(ref.images(3, 36, int(f["seed_36"])), records), f["chain_out"][batch])


def test_drawn_records_at_224():
    f = _f()
    got = _run(ref.images(4, 224, int(f["seed_224"])), f["records_224"])
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(f["sha_224"])


def test_identity_and_malformed_records():
    D = 36
    f = _f()
    imgs, good = ref.images(3, D, int(f["seed_36"])), f["records_36"]
    for layers in (1, 4):
        assert np.array_equal(_run(imgs, np.zeros((3, layers, 16), np.int32)), imgs)
    word = lambda rec, k, v: np.concatenate([rec[:k], np.asarray(v, np.int32).reshape(-1), rec[k + np.size(v):]])   # noqa: E731
    nan, inf = np.array([np.nan]).view(np.int32), np.array([-np.inf]).view(np.int32)
    rotate, poster, color = good[good[:, 0] == 15][0], good[good[:, 0] == 4][1], good[good[:, 0] == 7][0]
    bad = [word(rotate, 0, 16), word(rotate, 0, -1), word(rotate, 1, 1), word(rotate, 8, nan), word(rotate, 14, inf),        # the identity
           word(color, 2, np.array([np.inf], np.float32).view(np.int32)),
           word(poster, 1, 12), word(poster, 1, -5), word(good[good[:, 0] == 5][0], 1, 1000), word(rotate, 3, rotate[3] | 0x55 << 24)]
    fixed = [np.zeros(16, np.int32)] * 6 + [word(poster, 1, 8), word(poster, 1, 0), word(good[good[:, 0] == 5][0], 1, 256), rotate]
    assert [ref.cleaned(r) is None for r in bad] == [True] * 6 + [False] * 4
    for o in range(0, len(bad), 3):
        n = len(bad[o:o + 3])
        got, want = _run(imgs[:n], np.stack(bad[o:o + 3])[:, None]), _run(imgs[:n], np.stack(fixed[o:o + 3])[:, None])
        assert np.array_equal(got, want) and np.array_equal(got, ref.apply_batch(imgs[:n], np.stack(bad[o:o + 3])[:, None])), o
    # finite entries whose products overflow: every source point is a NaN or outside, the image is the fill
    huge = word(rotate, 4, np.array([1e308, -1e308, -1e300], np.float64).view(np.int32))
    assert np.array_equal(_run(imgs[:1], huge[None, None]), np.broadcast_to(np.uint8(data.RANDAUG_FILL), (1, D, D, 3)))


def test_through_the_wide_transform_with_mix_and_erase():
    H, W, D, B = 48, 40, 36, 3
    tr = qat_vit_amd.GpuWideResizeNormalize((H, W), out_size=D)
    g = torch.Generator().manual_seed(3)
    src = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    records = torch.from_numpy(_f()["chain_records"][2]).cuda()
    mix, erase = qat_vit_amd.MixupCutmix().draw([B], D, g).cuda(), qat_vit_amd.RandomErasing(p=1.0).draw(B, D, g).cuda()
    plain = tr(src, mix=mix, erase=erase).clone()
    assert getattr(tr, "_randaug", None) is None                     # the call without randaug made no buffer of the stage
    got = tr(src, mix=mix, erase=erase, randaug=records)
    staged = tr.staged(B).cpu().numpy()
    between = tr.randaug_stage().buffers(B)[1]
    assert np.array_equal(between.cpu().numpy(), ref.apply_batch(staged, records.cpu().numpy()))
    want = tr.inner(between, None, mix=mix, erase=erase)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not torch.equal(got, plain)
    with pytest.raises(NotImplementedError, match="GpuWideResizeNormalize"):
        qat_vit_amd.GpuResizeNormalize(D, D)(between, randaug=records)
