"""CPU-side checks of the teacher logit table: the new symbol in the library, the header and native.py, its argument errors without a HIP call,
the host logic of TeacherLogitTable (save / load and every field load compares) on CPU tensors, and the indices a rank's loader hands out."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import distill, native
from qat_vit_amd.vit import VisionTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "qatvit_kd_ce_loss_table"
TRANSFORM = (8, 32, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def test_table_symbol_in_exports_signatures_and_header(native_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert SYMBOL in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert SYMBOL in native.SIGNATURES and len(native.SIGNATURES[SYMBOL][1]) == 13
    assert native_lib.qatvit_abi_version() == 4
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    assert SYMBOL in set(re.findall(r"\b(qatvit_[a-z0-9_]+)\s*\(", hdr))
    assert "#define QATVIT_ABI_VERSION 4" in hdr.replace("  ", " ")


def test_table_loss_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null, aligned stand-in; never dereferenced on these paths (each call returns before any HIP call)
    ok = dict(student=p, table=p, rows=8, index=p, labels=p, batch=4, classes=10, T=4.0, alpha=0.5, eps=0.1, out3=p, dlogits=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.qatvit_kd_ce_loss_table(a["student"], a["table"], a["rows"], a["index"], a["labels"], a["batch"], a["classes"], a["T"], a["alpha"],
                                         a["eps"], a["out3"], a["dlogits"], None)

    for name in ("student", "table", "index", "labels", "out3", "dlogits"):
        assert call(**{name: None}) != 0 and b"qatvit_kd_ce_loss_table: null pointer" in L.qatvit_last_error(), name
    assert call(classes=1) != 0 and b"bad shape" in L.qatvit_last_error()
    assert call(batch=0) != 0 and b"bad shape" in L.qatvit_last_error()
    assert call(T=0.0) != 0 and b"kd_temp must be > 0" in L.qatvit_last_error()
    assert call(T=-1.0) != 0 and b"kd_temp must be > 0" in L.qatvit_last_error()
    assert call(rows=0) != 0 and b"table_rows 0" in L.qatvit_last_error()
    assert call(rows=-3) != 0 and b"table_rows -3" in L.qatvit_last_error()


def _tiny_teacher(seed=0, num_classes=10):
    torch.manual_seed(seed)
    return VisionTransformer(embed_dim=128, depth=1, num_heads=2, num_classes=num_classes, img_size=32, patch_size=16).eval()


def _cpu_table(tmp_path):
    g = torch.Generator().manual_seed(1)
    teacher = _tiny_teacher()
    data = torch.randint(0, 256, (12, 8, 8, 3), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (12,), generator=g)
    logits = torch.randn(12, 10, generator=g)
    table = qat_vit_amd.TeacherLogitTable(logits, distill.TeacherLogitTable.describe(teacher, data, TRANSFORM, labels), teacher)
    path = os.path.join(str(tmp_path), "table.pt")
    table.save(path)
    return table, path, teacher, data, labels


def test_save_load_round_trip_on_cpu_tensors(tmp_path):
    table, path, teacher, data, labels = _cpu_table(tmp_path)
    assert qat_vit_amd.TeacherLogitTable is distill.TeacherLogitTable and "TeacherLogitTable" in qat_vit_amd.__all__
    assert table.meta["teacher_form"] == 3          # embed_dim 128 is no multiple of 384: the engine's own fall-back, not the environment's default
    again = qat_vit_amd.TeacherLogitTable.load(path, teacher=teacher, data_u8=data, transform=TRANSFORM, labels=labels, device="cpu")
    assert torch.equal(again.logits, table.logits) and again.meta == table.meta and (again.N, again.C, len(again)) == (12, 10, 12)
    bare = qat_vit_amd.TeacherLogitTable.load(path, device="cpu")      # nothing given, nothing compared
    assert torch.equal(bare.logits, table.logits)
    # the record is plain data: a digest is a function of the bytes alone
    assert distill.data_digest(data, labels) == distill.data_digest(data.clone().numpy(), labels.tolist()) == table.meta["data_digest"]
    assert distill.param_digest(teacher) == distill.param_digest(_tiny_teacher()) == table.meta["param_digest"]


def test_load_names_the_field_that_differs(tmp_path):
    table, path, teacher, data, labels = _cpu_table(tmp_path)
    load = lambda **kw: qat_vit_amd.TeacherLogitTable.load(path, device="cpu", **kw)   # noqa: E731
    changed = data.clone()
    changed[3, 2, 1, 0] ^= 1
    with pytest.raises(ValueError, match="data_digest differs"):
        load(data_u8=changed, labels=labels)
    other_labels = labels.clone()
    other_labels[0] = (other_labels[0] + 1) % 10
    with pytest.raises(ValueError, match="data_digest differs"):
        load(data_u8=data, labels=other_labels)
    with pytest.raises(ValueError, match="N differs"):
        load(data_u8=data[:11], labels=labels[:11])
    with pytest.raises(ValueError, match="param_digest differs"):
        load(teacher=_tiny_teacher(seed=5))
    moved = _tiny_teacher()
    with torch.no_grad():
        moved.blocks[0].mlp.fc2.bias[7] += 1e-3
    with pytest.raises(ValueError, match="param_digest differs"):
        load(teacher=moved)
    with pytest.raises(ValueError, match="C differs"):
        load(teacher=_tiny_teacher(num_classes=11))
    for other in ((8, 64) + TRANSFORM[2:], (16,) + TRANSFORM[1:], TRANSFORM[:2] + ((0.5, 0.5, 0.5), TRANSFORM[3]), TRANSFORM[:3] + ((0.5, 0.5, 0.5),)):
        with pytest.raises(ValueError, match="transform differs"):
            load(transform=other)
    # the teacher form: a table recorded in another form than this teacher's engine would run
    meta = dict(table.meta, teacher_form=2)
    other_path = os.path.join(str(tmp_path), "form2.pt")
    qat_vit_amd.TeacherLogitTable(table.logits, meta).save(other_path)
    with pytest.raises(ValueError, match="teacher_form differs"):
        qat_vit_amd.TeacherLogitTable.load(other_path, teacher=teacher, device="cpu")
    # a record that does not describe its logits is refused at construction
    with pytest.raises(ValueError, match="table record says"):
        qat_vit_amd.TeacherLogitTable(table.logits[:5].contiguous(), table.meta)
    with pytest.raises(ValueError, match="lacks"):
        qat_vit_amd.TeacherLogitTable(table.logits, {"N": 12, "C": 10})


def test_teacher_form_follows_the_engines_fall_backs(monkeypatch):
    wide = VisionTransformer(embed_dim=384, depth=1, num_heads=6, num_classes=10, img_size=32, patch_size=16).eval()
    monkeypatch.delenv("QATVIT_TEACHER_PASSES", raising=False)
    assert distill.teacher_form(wide) == 2 and distill.teacher_form(_tiny_teacher()) == 3
    monkeypatch.setenv("QATVIT_TEACHER_PASSES", "1")
    assert distill.teacher_form(wide) == 1 and distill.teacher_form(_tiny_teacher()) == 3
    monkeypatch.setenv("QATVIT_TEACHER_PASSES", "3")
    assert distill.teacher_form(wide) == 3
    monkeypatch.delenv("QATVIT_TEACHER_PASSES")
    with torch.no_grad():
        wide.blocks[0].norm1.weight.fill_(1e4)     # a LayerNorm gain that could leave fp16's range: the engine keeps the bf16-pair form
    assert distill.teacher_form(wide) == 3


def test_cpu_inputs_raise_and_a_changed_teacher_is_noticed(tmp_path):
    table, path, teacher, data, labels = _cpu_table(tmp_path)
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.TeacherLogitTable.build(teacher, data)
    with pytest.raises(RuntimeError, match="CUDA device"):
        qat_vit_amd.GpuImageLoader(data, labels, 4, device="cpu", return_index=True)
    idx = torch.arange(4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        table.rows(idx)
    with pytest.raises(RuntimeError, match="MI355X only"):
        table.loss(torch.randn(4, 10), idx, labels[:4])
    with pytest.raises(RuntimeError, match="MI355X only"):
        qat_vit_amd.functional.kd_ce_loss_table(torch.randn(4, 10), table.logits, idx, labels[:4])
    table.check_fresh()
    with torch.no_grad():
        teacher.head.weight.add_(1)
    with pytest.raises(RuntimeError, match="replaced or modified"):
        table.check_fresh()
    fresh = qat_vit_amd.TeacherLogitTable(table.logits, table.meta, teacher)
    fresh.check_fresh()
    teacher.load_state_dict(_tiny_teacher(seed=2).state_dict())
    with pytest.raises(RuntimeError, match="replaced or modified"):
        fresh.check_fresh()


@pytest.mark.parametrize("drop_last", [False, True])
def test_a_ranks_indices_are_the_plans_own_tensors(drop_last):
    """Host side of return_index=True under a DistributedSampler: the loader slices the concatenation of epoch_batches' tensors, batch by batch, so
    what a rank receives is its own plan (and through it a stock DataLoader's batches, tests/test_data_abi.py)."""
    from torch.utils.data import DataLoader, DistributedSampler

    n, bs = 103, 8
    seen = []
    for rank in range(2):
        sampler = DistributedSampler(range(n), num_replicas=2, rank=rank, shuffle=True, seed=5)
        sampler.set_epoch(1)
        plan = qat_vit_amd.epoch_batches(n, bs, sampler=sampler, drop_last=drop_last)
        flat, o = torch.cat(plan), 0
        for b, want in zip(plan, DataLoader(range(n), batch_size=bs, sampler=sampler, drop_last=drop_last)):
            assert torch.equal(flat[o:o + b.shape[0]], b) and torch.equal(b, want) and b.dtype == torch.int64
            assert int(b.min()) >= 0 and int(b.max()) < n          # every index a rank receives is a row of the full table it holds
            o += b.shape[0]
        assert o == flat.shape[0]
        seen += flat.tolist()
    if not drop_last:
        assert set(seen) == set(range(n))
