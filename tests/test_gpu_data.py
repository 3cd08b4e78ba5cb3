"""The input pipeline (qat_vit_amd.GpuResizeNormalize / GpuImageLoader, csrc/image.hip) on an MI355X: the batch EQUALS what Pillow's
Resize(BICUBIC) + ToTensor() + Normalize() give on the host, for every element of every fixture image; the loader yields a stock DataLoader's
batches; the native forwards cannot tell the two feeds apart; refusals."""
import copy

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, DistributedSampler, TensorDataset

import qat_vit_amd
from qat_vit_amd import data
from tests import resize_kat
from tests.util import prepare
from tools.gen_resize_golden import resize as np_resize

pytestmark = pytest.mark.gpu


def _normalized(resized_u8):
    """ToTensor() + Normalize(ImageNet) of uint8 [B, D, D, 3] images, with the transforms' own CPU expressions: fp32 [B, 3, D, D]."""
    x = torch.from_numpy(np.ascontiguousarray(resized_u8)).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    mean, std = torch.tensor(data.IMAGENET_MEAN).view(-1, 1, 1), torch.tensor(data.IMAGENET_STD).view(-1, 1, 1)
    return x.sub_(mean).div_(std)


def _host_resize(images_u8, D):
    """Resize(D, BICUBIC) of uint8 [B, S, S, 3] on the host: Pillow where it is installed, else the NumPy restatement that tests/test_data_abi.py
    holds equal to it."""
    try:
        from PIL import Image
    except ImportError:
        return np.stack([np_resize(a, D) for a in images_u8])
    return np.stack([np.asarray(Image.fromarray(a).resize((D, D), Image.BICUBIC)) for a in images_u8])


def test_batch_equals_the_value_table_of_the_expected_bytes_for_every_fixture_image():
    meta, cases = resize_kat.load()
    D = int(meta["dst"])
    table = data.value_table()
    g = torch.Generator().manual_seed(0)
    for s in meta["sizes"].tolist():
        mine = [(a, want) for cs, _, a, want in cases if cs == s]
        assert len(mine) == 4
        src = torch.from_numpy(np.stack([a for a, _ in mine])).cuda()
        exp = torch.from_numpy(np.stack([w for _, w in mine])).long()                      # [4, D, D, 3]
        want = torch.stack([table[c][exp[..., c]] for c in range(3)], dim=1)               # table[c][expected_u8], [4, 3, D, D]
        assert torch.equal(want, _normalized(np.stack([w for _, w in mine])))              # ... which is what the transforms give
        want = want.cuda()
        tr = qat_vit_amd.GpuResizeNormalize(s)
        out = tr(src)
        assert out.shape == (4, 3, D, D) and out.dtype == torch.float32 and out.is_contiguous()
        assert torch.equal(out, want), s
        for idx in ([2], [3, 1, 1, 0, 2, 3, 0], torch.randint(0, 4, (256,), generator=g).tolist()):   # batch 1, 7 (permuted, repeated), 256
            idx = torch.tensor(idx, dtype=torch.int64, device="cuda")
            assert torch.equal(tr(src, idx), want[idx]), (s, idx.numel())
        idx = torch.tensor([1, 0, 3], dtype=torch.int64, device="cuda")
        buf = torch.full((3, 3, D, D), float("nan"), device="cuda")
        assert tr(src, idx, out=buf) is buf and torch.equal(buf, want[idx])
        buf4 = torch.full((4, 3, D, D), float("nan"), device="cuda")
        assert tr(src, out=buf4) is buf4 and torch.equal(buf4, want)


@pytest.mark.parametrize("s,d", [(8, 224), (37, 224), (150, 224), (223, 224), (96, 384), (384, 384)])
def test_other_sizes_equal_the_host_transform(s, d):
    """Sizes off the fixture: rows that are not dword-aligned (odd S), the smallest S, and the kernel's form for an output size other than 224."""
    rng = np.random.default_rng(s)
    imgs = np.stack([rng.integers(0, 256, (s, s, 3), dtype=np.uint8), (rng.integers(0, 2, (s, s, 3)) * 255).astype(np.uint8),
                     np.clip(rng.normal(128, 60, (s, s, 3)), 0, 255).astype(np.uint8)])
    want = _normalized(_host_resize(imgs, d)).cuda()
    tr = qat_vit_amd.GpuResizeNormalize(s, out_size=d)
    assert torch.equal(tr(torch.from_numpy(imgs).cuda()), want)
    idx = torch.tensor([2, 0, 2, 1, 1], dtype=torch.int64, device="cuda")
    assert torch.equal(tr(torch.from_numpy(imgs).cuda(), idx), want[idx])


def _cifar_like(n, seed):
    rng = np.random.default_rng(seed)
    imgs = np.clip(rng.normal(120, 70, (n, 32, 32, 3)), 0, 255).astype(np.uint8)
    labels = rng.integers(0, 10, n)
    return imgs, labels, _normalized(_host_resize(imgs, 224))


def test_loader_yields_the_batches_of_a_stock_dataloader():
    n, bs = 53, 8
    imgs, labels, x_cpu = _cifar_like(n, 1)
    ds = TensorDataset(x_cpu, torch.from_numpy(labels))

    def same(loader, ref):
        got, want = list(loader), list(ref)
        assert len(got) == len(want) == len(loader) == len(ref)
        for (gx, gy), (wx, wy) in zip(got, want):
            assert gx.is_cuda and gy.is_cuda and gy.dtype == torch.int64
            assert torch.equal(gx.cpu(), wx) and torch.equal(gy.cpu(), wy)
        assert len({gx.data_ptr() for gx, _ in got}) == len(got)            # held batches are never overwritten: each is its own tensor
        return got

    for drop_last in (False, True):
        got = same(qat_vit_amd.GpuImageLoader(imgs, labels, bs, drop_last=drop_last), DataLoader(ds, batch_size=bs, drop_last=drop_last))
        assert got[-1][0].shape[0] == (bs if drop_last else n % bs)
        for rank in range(2):
            s1, s2 = (DistributedSampler(ds, num_replicas=2, rank=rank, shuffle=True, seed=3) for _ in range(2))
            loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, sampler=s1, drop_last=drop_last)
            for epoch in range(2):
                s1.set_epoch(epoch), s2.set_epoch(epoch)
                same(loader, DataLoader(ds, batch_size=bs, sampler=s2, drop_last=drop_last))
    # shuffle without a sampler: every image once, in the order RandomSampler draws from the generator
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, bs, shuffle=True, generator=torch.Generator().manual_seed(4))
    order = torch.cat(qat_vit_amd.epoch_batches(n, bs, shuffle=True, generator=torch.Generator().manual_seed(4)))
    got = list(loader)
    assert sorted(order.tolist()) == list(range(n)) and order.tolist() != list(range(n))
    assert torch.equal(torch.cat([x for x, _ in got]).cpu(), x_cpu[order]) and torch.equal(torch.cat([y for _, y in got]).cpu(), torch.from_numpy(labels)[order])


def _student(seed):
    torch.manual_seed(seed)
    return qat_vit_amd.create_model("vit_small_patch16_224_student", pretrained=False, num_classes=10, qat_wrapper=True, depth=2)


def test_native_forwards_cannot_tell_the_loader_from_the_host_built_batch():
    imgs, labels, x_cpu = _cifar_like(8, 2)
    (x, y), = list(qat_vit_amd.GpuImageLoader(imgs, labels, 8))
    assert torch.equal(x.cpu(), x_cpu) and torch.equal(y.cpu(), torch.from_numpy(labels))
    # QAT forward: two copies of one prepared model (the forward updates the observers)
    p1 = prepare(_student(0), "qnnpack").cuda().train()
    p2 = copy.deepcopy(p1)
    a, b = p1(x), p2(x_cpu.cuda())
    assert torch.isfinite(a).all() and torch.equal(a, b)
    f1, f2 = (qat_vit_amd.native_float(_student(1).cuda().train()) for _ in range(2))     # the same seed: the same weights (a deepcopy drops the opt-in)
    assert all(qat_vit_amd.float_engine.is_native_float(f) for f in (f1, f2))
    a, b = f1(x), f2(x_cpu.cuda())
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_refusals():
    tr = qat_vit_amd.GpuResizeNormalize(32)
    imgs = torch.zeros(2, 32, 32, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="move the uint8 images to the GPU"):
        tr(imgs)
    with pytest.raises(TypeError, match="uint8"):
        tr(imgs.cuda().float())
    with pytest.raises(ValueError, match=r"\[N, 32, 32, 3\]"):
        tr(torch.zeros(2, 3, 32, 32, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        tr(torch.zeros(2, 32, 32, 6, dtype=torch.uint8, device="cuda")[..., ::2])
    with pytest.raises(ValueError, match="index"):
        tr(imgs.cuda(), torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        tr(imgs.cuda(), out=torch.empty(2, 3, 224, 224, dtype=torch.float16, device="cuda"))
    with pytest.raises(RuntimeError, match="downscaling is not supported"):
        qat_vit_amd.GpuResizeNormalize(256, out_size=224)
    with pytest.raises(ValueError, match="HWC"):
        qat_vit_amd.GpuImageLoader(np.zeros((4, 3, 32, 32), np.uint8), np.zeros(4, np.int64), 2)
