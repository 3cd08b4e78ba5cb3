"""CPU-side checks of the RandAugment stage (qatvit_image_bytes_randaug, qat_vit_amd.RandAugment): the symbol and every refusal of the entry,
under its name and before any HIP call; the draw's shapes, ranges and determinism (timm is not installed: the draw is a restatement and is
checked for its ranges only); the config string; and the NumPy restatement (tests/randaug_ref.py) against Pillow's bytes in the fixture.
Nothing here needs a GPU."""
import hashlib

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data, native
from tests import randaug_ref as ref

P = 1 << 20                                                          # non-null, aligned; never dereferenced on these paths
NAME = "qatvit_image_bytes_randaug"
IMAGE = 224 * 224 * 3


@pytest.mark.parametrize("text,kw", [
    ("null pointer argument", dict(bytes=None)), ("null pointer argument", dict(records=None)), ("null pointer argument", dict(scratch=None)),
    ("null pointer argument", dict(out=None)), ("output size 222 must be a multiple of 4 in 8 .. 384", dict(D=222)),
    ("output size 4 ", dict(D=4)), ("output size 388 ", dict(D=388)), ("batch 0 must be 1 .. 65535", dict(B=0)),
    ("batch 65536 must be 1 .. 65535", dict(B=65536)), ("0 layers are outside 1 .. 4", dict(layers=0)), ("5 layers are outside 1 .. 4", dict(layers=5)),
    ("misaligned pointer", dict(bytes=P + 1)), ("misaligned pointer", dict(records=P + 2)), ("misaligned pointer", dict(out=8 * P + 3)),
    ("three distinct buffers", dict(scratch=P)), ("three distinct buffers", dict(out=P)), ("three distinct buffers", dict(out=4 * P)),
    ("three distinct buffers", dict(scratch=P + IMAGE - 4)), ("three distinct buffers", dict(B=2, out=4 * P + IMAGE))])
def test_every_refusal_is_a_string_under_the_entrys_name(native_lib, text, kw):
    a = dict(bytes=P, B=1, D=224, records=64, layers=2, scratch=4 * P, out=8 * P)
    a.update(kw)
    rc = native_lib.qatvit_image_bytes_randaug(a["bytes"], a["B"], a["D"], a["records"], a["layers"], a["scratch"], a["out"], None)
    err = native_lib.qatvit_last_error().decode()
    assert rc != 0 and err.startswith(NAME + ": ") and text in err, (kw, err)
    assert native.SIGNATURES[NAME][0] is native.c_int and "RandAugment" in qat_vit_amd.__all__


@pytest.mark.parametrize("increasing", [True, False])
def test_draw_shapes_ranges_and_determinism(increasing):
    D, n = 224, 400
    aug = qat_vit_amd.RandAugment(magnitude=9, num_layers=3, mstd=0.5, prob=0.5, increasing=increasing)
    r = aug.draw(n, D, torch.Generator().manual_seed(1))
    assert r.shape == (n, 3, 16) and r.dtype == torch.int32 and torch.equal(r, aug.draw(n, D, torch.Generator().manual_seed(1)))
    assert not torch.equal(r, aug.draw(n, D, torch.Generator().manual_seed(2)))
    r = r.numpy().reshape(-1, 16)
    op, arg, f, m = r[:, 0], r[:, 1], r[:, 2].copy().view(np.float32), r[:, 4:].copy().view(np.float64)
    assert set(op) == set(range(16)) and 0.4 < (op == 0).mean() < 0.6 and not r[op == 0].any()
    assert (r[op > 0, 3] == 124 | 116 << 8 | 104 << 16).all() and set(arg[op >= 11]) == {2, 3}
    assert arg[op == 4].min() >= 0 and arg[op == 4].max() <= 4 and arg[op == 5].min() >= 0 and arg[op == 5].max() <= 256
    assert arg[op == 6].min() >= 0 and arg[op == 6].max() <= 128 and (arg[(op >= 1) & (op <= 3)] == 0).all()
    enh = f[(op >= 7) & (op <= 10)]
    assert enh.min() >= 0.1 and enh.max() <= 1.9 and ((enh < 1).any() and (enh > 1).any()) == increasing
    assert (np.abs(m[op == 11][:, 1]) <= 0.3).all() and (np.abs(m[op == 12][:, 3]) <= 0.3).all() and (m[op == 11][:, 1] < 0).any()
    assert (np.abs(m[op == 13][:, 2]) <= 0.45 * D).all() and (np.abs(m[op == 14][:, 5]) <= 0.45 * D).all()
    rot = m[op == 15]
    assert np.allclose(rot[:, 0] ** 2 + rot[:, 1] ** 2, 1, atol=1e-14) and (rot[:, 0] >= np.cos(np.radians(30)) - 1e-15).all()
    assert (m[(op > 0) & (op < 11)] == [1, 0, 0, 0, 1, 0]).all()
    for bad in (dict(magnitude=11), dict(num_layers=5), dict(prob=1.5), dict(interpolation=("nearest",)), dict(fill=(1, 2, 256))):
        with pytest.raises(ValueError):
            qat_vit_amd.RandAugment(**bad)


def test_from_config():
    a = qat_vit_amd.RandAugment.from_config("rand-m9-mstd0.5-inc1")
    assert (a.magnitude, a.num_layers, a.mstd, a.prob, a.increasing) == (9.0, 2, 0.5, 0.5, True)
    a = qat_vit_amd.RandAugment.from_config("rand-m7-n3-p0.25-mstd101", fill=(0, 0, 0))
    assert (a.magnitude, a.num_layers, a.mstd, a.prob, a.increasing, a.fill) == (7.0, 3, 101.0, 0.25, False, (0, 0, 0))
    for bad in ("augmix-m3", "rand-m9-mmax10", "rand-w0", "rand-t1", "rand-m", "rand-x3", "rand-n9"):
        with pytest.raises(ValueError):
            qat_vit_amd.RandAugment.from_config(bad)


def test_the_restatement_equals_the_fixture():
    f = np.load(ref.GOLDEN)
    for D in ref.SIZES:
        imgs = ref.images(3, D, int(f[f"seed_{D}"]))
        for rec, want in zip(f[f"records_{D}"], f[f"out_{D}"]):
            assert np.array_equal(ref.apply_batch(imgs, np.broadcast_to(rec, (3, 1, 16))), want), (D, rec[:4])
    imgs = ref.images(3, 36, int(f["seed_36"]))
    for records, want in zip(f["chain_records"], f["chain_out"]):
        assert np.array_equal(ref.apply_batch(imgs, records), want)
    got = ref.apply_batch(ref.images(4, 224, int(f["seed_224"])), f["records_224"])
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(f["sha_224"])
    assert np.array_equal(f["records_36"][-1], data.randaug_record("Rotate", 90.0, 36, "bilinear"))


def test_the_loader_draws_the_records_last_and_hands_them_over_per_batch(monkeypatch):
    from tests.test_bytes_blur_abi import _WideRecorder

    empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **k: empty(*a, **k))       # no accelerator here: the block is not pinned
    n, tr, aug, crop = 20, _WideRecorder(64, 48, 32), qat_vit_amd.RandAugment(num_layers=3), qat_vit_amd.RandomResizedCrop()
    imgs, labels = np.zeros((n, 64, 48, 3), np.uint8), np.zeros(n, np.int64)
    list(qat_vit_amd.GpuImageLoader(imgs, labels, 8, shuffle=True, generator=torch.Generator().manual_seed(1), transform=tr, crop=crop, rand_augment=aug))
    g = torch.Generator().manual_seed(1)
    qat_vit_amd.epoch_batches(n, 8, shuffle=True, generator=g), crop.draw(n, (64, 48), g)
    assert [tuple(c["randaug"].shape) for c in tr.calls] == [(8, 3, 16), (8, 3, 16), (4, 3, 16)]
    assert torch.equal(torch.cat([c["randaug"] for c in tr.calls]), aug.draw(n, 32, g))
    one = object.__new__(qat_vit_amd.GpuResizeNormalize)              # the constructor needs the GPU; the refusal does not
    one.device = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="GpuWideResizeNormalize"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 32, 32, 3), np.uint8), np.zeros(4, np.int64), 2, transform=one, rand_augment=aug)
