"""CPU-side checks of the input pipeline's boundary: the host-only table entry points against the Pillow-made fixture and torch's own expression,
argument errors as strings without a HIP call, the CIFAR-10 reader, and the epoch plan against a stock DataLoader."""
import ctypes
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import data, native
from tests import resize_kat
from tools.gen_resize_golden import resize as np_resize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_SYMBOLS = {"qatvit_image_resize_coeffs", "qatvit_image_table", "qatvit_image_batch"}


def test_image_symbols_in_header_signatures_and_exports(native_lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    assert IMAGE_SYMBOLS <= set(re.findall(r"\b(qatvit_[a-z0-9_]+)\s*\(", hdr))
    assert IMAGE_SYMBOLS <= set(native.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert IMAGE_SYMBOLS <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4


def test_resize_coeffs_equal_the_fixture_for_every_size(native_lib):
    meta, _ = resize_kat.load()
    D = int(meta["dst"])
    for s in meta["sizes"].tolist():
        xmin, ntaps, coef = data.resize_tables(s, D)
        assert np.array_equal(xmin.numpy(), meta[f"xmin_{s}"]), s
        assert np.array_equal(ntaps.numpy(), meta[f"ntaps_{s}"]), s
        assert np.array_equal(coef.numpy(), meta[f"coef_{s}"]), s


def test_fixture_outputs_follow_from_the_library_tables(native_lib):
    """The stored Pillow outputs are what the two integer passes give with the library's tables: every image, every element."""
    meta, cases = resize_kat.load()
    D = int(meta["dst"])
    tables = {s: tuple(t.numpy() for t in data.resize_tables(s, D)) for s in meta["sizes"].tolist()}
    assert len(cases) == 16
    for s, kind, a, want in cases:
        assert np.array_equal(np_resize(a, D, tables[s]), want), (s, kind)


def test_library_tables_reproduce_pillow_on_fresh_images(native_lib):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for s in (8, 16, 32, 37, 48, 64, 112, 150, 200, 223, 224):
        tables = tuple(t.numpy() for t in data.resize_tables(s, 224))
        assert int(tables[1].max()) <= 4
        for a in (rng.integers(0, 256, (s, s, 3), dtype=np.uint8), (rng.integers(0, 2, (s, s, 3)) * 255).astype(np.uint8)):
            want = np.asarray(Image.fromarray(a).resize((224, 224), Image.BICUBIC))
            assert np.array_equal(np_resize(a, 224, tables), want), s
    # another output size the kernel takes
    a = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    tables = tuple(t.numpy() for t in data.resize_tables(96, 384))
    assert np.array_equal(np_resize(a, 384, tables), np.asarray(Image.fromarray(a).resize((384, 384), Image.BICUBIC)))


def test_value_table_equals_torch_to_tensor_and_normalize(native_lib):
    for mean, std in ((data.IMAGENET_MEAN, data.IMAGENET_STD), ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))):
        table = data.value_table(mean, std)
        m, s = torch.tensor(mean, dtype=torch.float32).view(3, 1), torch.tensor(std, dtype=torch.float32).view(3, 1)
        want = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).view(1, 256).repeat(3, 1).sub_(m).div_(s)
        assert torch.equal(table, want)
    # and the transforms' own shapes: a [3, H, W] image through ToTensor's and Normalize's expressions
    img = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).repeat(3, 1, 1)
    x = img.to(torch.float32).div(255)
    x.sub_(torch.tensor(data.IMAGENET_MEAN).view(-1, 1, 1)).div_(torch.tensor(data.IMAGENET_STD).view(-1, 1, 1))
    table = data.value_table()
    assert torch.equal(torch.stack([table[c][img[c].long()] for c in range(3)]), x)


def test_image_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    i32 = lambda n: (ctypes.c_int32 * n)()   # noqa: E731
    xmin, ntaps, coef = i32(512), i32(512), i32(2048)
    for src, dst, msg in ((256, 224, b"downscaling is not supported"), (4, 224, b"outside 8"), (32, 222, b"multiple of 4"), (32, 512, b"at most 384")):
        assert L.qatvit_image_resize_coeffs(src, dst, xmin, ntaps, coef) != 0
        assert msg in L.qatvit_last_error(), (src, dst, L.qatvit_last_error())
    assert L.qatvit_image_resize_coeffs(32, 224, None, ntaps, coef) != 0 and b"null pointer" in L.qatvit_last_error()
    assert L.qatvit_image_table(None, None, None) != 0 and b"null pointer" in L.qatvit_last_error()
    f3, table = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 768)()
    assert L.qatvit_image_table(f3, (ctypes.c_float * 3)(0.5, 0.0, 0.5), table) != 0 and b"std[1] is zero" in L.qatvit_last_error()
    # the launch entry validates before any HIP call: these return on a machine without a GPU
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths
    assert L.qatvit_image_batch(None, None, 1, 1, 32, 224, p, p, p, None) != 0 and b"null pointer" in L.qatvit_last_error()
    assert L.qatvit_image_batch(p, None, 1, 1, 256, 224, p, p, p, None) != 0 and b"downscaling is not supported" in L.qatvit_last_error()
    assert L.qatvit_image_batch(p, None, 0, 1, 32, 224, p, p, p, None) != 0 and b"batch 0" in L.qatvit_last_error()
    assert L.qatvit_image_batch(p, None, 8, 4, 32, 224, p, p, p, None) != 0 and b"needs an index" in L.qatvit_last_error()
    assert L.qatvit_image_batch(p, None, 1, 1, 32, 224, p, p, p + 4, None) != 0 and b"misaligned" in L.qatvit_last_error()
    with pytest.raises(RuntimeError, match="downscaling is not supported"):
        data.resize_tables(256, 224)
    with pytest.raises(RuntimeError, match="CUDA device"):
        qat_vit_amd.GpuResizeNormalize(32, device="cpu")


def _write_cifar(root, rng):
    base = os.path.join(root, "cifar-10-batches-py")
    os.makedirs(base)
    planes, labels = {}, {}
    for name in [f"data_batch_{i}" for i in range(1, 6)] + ["test_batch"]:
        planes[name] = rng.integers(0, 256, (6, 3072), dtype=np.uint8)      # rows of 1024 R, 1024 G, 1024 B bytes, as in the archive
        labels[name] = rng.integers(0, 10, 6).tolist()
        with open(os.path.join(base, name), "wb") as f:
            pickle.dump({"batch_label": name, "labels": labels[name], "data": planes[name], "filenames": [f"{name}_{i}.png" for i in range(6)]}, f)
    return planes, labels


def test_cifar10_arrays_reads_the_archive_layout_and_never_downloads(tmp_path):
    planes, labels = _write_cifar(str(tmp_path), np.random.default_rng(3))
    x, y = qat_vit_amd.cifar10_arrays(str(tmp_path), train=True)
    assert x.dtype == np.uint8 and x.shape == (30, 32, 32, 3) and x.flags["C_CONTIGUOUS"] and y.dtype == np.int64 and y.shape == (30,)
    for i, name in enumerate(f"data_batch_{k}" for k in range(1, 6)):
        for j in range(6):
            for c in range(3):
                assert np.array_equal(x[6 * i + j, :, :, c], planes[name][j, 1024 * c:1024 * (c + 1)].reshape(32, 32))
        assert y[6 * i:6 * i + 6].tolist() == labels[name]
    xt, yt = qat_vit_amd.cifar10_arrays(str(tmp_path), train=False)
    assert xt.shape == (6, 32, 32, 3) and yt.tolist() == labels["test_batch"]
    os.remove(os.path.join(str(tmp_path), "cifar-10-batches-py", "data_batch_3"))
    with pytest.raises(FileNotFoundError, match="data_batch_3"):
        qat_vit_amd.cifar10_arrays(str(tmp_path), train=True)
    with pytest.raises(FileNotFoundError):
        qat_vit_amd.cifar10_arrays(os.path.join(str(tmp_path), "nowhere"), train=False)


@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_batches_equal_a_stock_dataloader_with_a_distributed_sampler(drop_last):
    from torch.utils.data import DataLoader, DistributedSampler

    n, bs = 103, 8
    for rank in range(2):
        sampler = DistributedSampler(range(n), num_replicas=2, rank=rank, shuffle=True, seed=5)
        for epoch in range(2):
            sampler.set_epoch(epoch)
            want = [b.tolist() for b in DataLoader(range(n), batch_size=bs, sampler=sampler, drop_last=drop_last)]
            got = qat_vit_amd.epoch_batches(n, bs, sampler=sampler, drop_last=drop_last)
            assert all(b.dtype == torch.int64 and b.dim() == 1 for b in got)
            assert [b.tolist() for b in got] == want
            assert len(want) == (52 // bs if drop_last else -(-52 // bs))
    # the two ranks of one epoch split the data set; two epochs differ
    s0, s1 = (DistributedSampler(range(n), num_replicas=2, rank=r, shuffle=True, seed=5) for r in range(2))
    e0 = torch.cat(qat_vit_amd.epoch_batches(n, bs, sampler=s0)).tolist()
    assert set(e0) | set(torch.cat(qat_vit_amd.epoch_batches(n, bs, sampler=s1)).tolist()) == set(range(n))
    s0.set_epoch(1)
    assert torch.cat(qat_vit_amd.epoch_batches(n, bs, sampler=s0)).tolist() != e0


@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_batches_equal_a_stock_dataloader_without_a_sampler(drop_last):
    from torch.utils.data import DataLoader

    n, bs = 45, 7
    want = [b.tolist() for b in DataLoader(range(n), batch_size=bs, drop_last=drop_last)]
    assert [b.tolist() for b in qat_vit_amd.epoch_batches(n, bs, drop_last=drop_last)] == want
    # shuffle: RandomSampler's permutation, drawn from the generator (a DataLoader iterator first takes its workers' base seed from the same
    # generator, so the two are compared through the sampler, not through equal seeds)
    from torch.utils.data import BatchSampler, RandomSampler

    g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    want = list(BatchSampler(RandomSampler(range(n), generator=g1), bs, drop_last))
    got = [b.tolist() for b in qat_vit_amd.epoch_batches(n, bs, shuffle=True, drop_last=drop_last, generator=g2)]
    flat = sum(got, [])
    assert got == want and flat != sorted(flat) and len(set(flat)) == len(flat) == (n // bs * bs if drop_last else n)
    again = sum((b.tolist() for b in qat_vit_amd.epoch_batches(n, bs, shuffle=True, drop_last=drop_last, generator=g2)), [])
    assert again != flat                                   # the next epoch draws a new order from the same generator
    with pytest.raises(ValueError, match="mutually exclusive"):
        qat_vit_amd.epoch_batches(n, bs, shuffle=True, sampler=range(n))
