"""The teacher logit table on an MI355X (qat_vit_amd.TeacherLogitTable, F.kd_ce_loss_table, GpuImageLoader(return_index=True)):
rows against the live native teacher, the fused loss against kd_ce_loss on gathered rows, out-of-range indices, the loader's indices, a whole
training step, staleness, and the absence of the teacher's kernels from a table step."""
import copy
import os

import numpy as np
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd.vit import VisionTransformer
from tests.util import prepare

pytestmark = pytest.mark.gpu


def _frozen(model):
    for p in model.parameters():
        p.requires_grad = False
    return model.cuda().eval()


def _images(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, size, size, 3), generator=g, dtype=torch.uint8).cuda(), torch.randint(0, 10, (n,), generator=g).cuda()


@pytest.mark.parametrize("depth,passes", [(2, None), (2, "3"), (12, None)])
def test_rows_equal_the_live_teacher(native_lib, monkeypatch, depth, passes):
    """A table built at batch 256 over 600 images (the last chunk is padded) against the live teacher on shuffled batches of 256, 80 and 1:
    bit for bit.  The deviation of the live teacher from itself (the same 256 images in two batch compositions) is printed next to it."""
    if passes is None:
        monkeypatch.delenv("QATVIT_TEACHER_PASSES", raising=False)
    else:
        monkeypatch.setenv("QATVIT_TEACHER_PASSES", passes)
    torch.manual_seed(20 + depth)
    teacher = _frozen(VisionTransformer(embed_dim=768, depth=depth, num_heads=12, num_classes=10))
    data, _ = _images(600, 32, 1)
    tr = qat_vit_amd.GpuResizeNormalize(32)
    teacher.train()
    table = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=256)
    assert teacher.training and all(m.training for m in teacher.modules())      # the flags are restored
    teacher.eval()
    assert table.logits.shape == (600, 10) and table.logits.dtype == torch.float32 and table.logits.is_cuda and table.logits.is_contiguous()
    assert table.meta["teacher_form"] == (2 if passes is None else 3) and table.meta["N"] == 600 and table.meta["C"] == 10
    assert table.meta["transform"] == (32, 224, tr.mean, tr.std)
    assert bool(torch.isfinite(table.logits).all()) and float(table.logits.std()) > 1e-3
    perm = torch.randperm(600, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        for n in (256, 80, 1):
            idx = perm[300:300 + n].contiguous()       # straddles the chunks, the padded one included
            live = teacher(tr(data, idx))
            dev = float((table.rows(idx) - live).abs().max())
            print(f"depth {depth} form {table.meta['teacher_form']} batch {n}: max |table - live| = {dev:.3e}")
            assert torch.equal(table.rows(idx), live), (n, dev)
        # the live teacher against itself: the same 256 images, in this order and reversed
        idx = perm[:256].contiguous()
        a, b = teacher(tr(data, idx)), teacher(tr(data, idx.flip(0).contiguous())).flip(0)
        print(f"depth {depth} form {table.meta['teacher_form']}: live teacher, two batch compositions: max |a - b| = {float((a - b).abs().max()):.3e}")
        assert torch.equal(a, b)
    # the last image's row is that image's, not a padding artefact, and the table is usable at the padded chunk's end
    with torch.no_grad():
        last = torch.tensor([599], device="cuda")
        assert torch.equal(table.rows(last), teacher(tr(data, last)))


def _loss_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "loss_kat.npz"))
    for i in range(int(z["n"])):
        T, a, eps = (float(v) for v in z[f"{i}/hp"])
        yield f"kat{i}", torch.from_numpy(z[f"{i}/s"]).float(), torch.from_numpy(z[f"{i}/t"]).float(), torch.from_numpy(z[f"{i}/y"]), (T, a, eps)
    for B, C, hp in ((256, 10, (4.0, 0.5, 0.1)), (1024, 10, (4.0, 0.5, 0.1)), (256, 100, (2.0, 0.7, 0.0)), (1024, 37, (1.0, 0.3, 0.2))):
        g = torch.Generator().manual_seed(B + C)
        yield f"rand{B}x{C}", 3 * torch.randn(B, C, generator=g), 5 * torch.randn(B, C, generator=g), torch.randint(0, C, (B,), generator=g), hp


def _scatter(t, rows, seed):
    """The teacher rows scattered into a larger table under a random permutation: (table, index) with table[index] == t."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(rows, generator=g)[:t.shape[0]]
    table = torch.randn(rows, t.shape[1], generator=g) * 7
    table[idx] = t
    return table.cuda(), idx.cuda()


def _both(s, t_rows, table, idx, y, hp):
    s1 = s.clone().cuda().requires_grad_(True)
    l1, p1 = F.kd_ce_loss(s1, t_rows, y, *hp)
    l1.backward()
    s2 = s.clone().cuda().requires_grad_(True)
    l2, p2 = F.kd_ce_loss_table(s2, table, idx, y, *hp)
    l2.backward()
    return (l1.detach(), p1, s1.grad), (l2.detach(), p2, s2.grad)


def test_table_loss_equals_the_unfused_path(native_lib, golden_dir):
    n = 0
    for name, s, t, y, hp in _loss_cases(golden_dir):
        table, idx = _scatter(t, 3 * t.shape[0] + 11, n)
        y = y.cuda()
        (l1, p1, g1), (l2, p2, g2) = _both(s, table[idx], table, idx, y, hp)
        assert torch.equal(table[idx], t.cuda())
        assert torch.equal(l1, l2) and torch.equal(p1, p2) and torch.equal(g1, g2), name
        assert bool(torch.isfinite(p2).all()) and bool(torch.isfinite(g2).all()), name
        n += 1
    assert n >= 6
    # repeated indices (a padded batch) and a table of one row
    s, y = torch.randn(8, 10), torch.randint(0, 10, (8,)).cuda()
    table = torch.randn(1, 10).cuda()
    idx = torch.zeros(8, dtype=torch.int64, device="cuda")
    (l1, p1, g1), (l2, p2, g2) = _both(s, table[idx], table, idx, y, (4.0, 0.5, 0.1))
    assert torch.equal(p1, p2) and torch.equal(g1, g2)


@pytest.mark.parametrize("B", [256, 1024])
def test_out_of_range_index_poisons_its_row_and_reads_nothing(native_lib, B):
    """One index == table_rows and one == -1 among valid ones.  The table is the front of a larger allocation whose tail (where the bad index
    would land) holds a canary of huge values: the run completes, the loss and exactly those two gradient rows are NaN, every other row is what
    the valid case gives, and the canary is as it was."""
    rows, C, hp = 2 * B + 5, 10, (4.0, 0.5, 0.1)
    g = torch.Generator().manual_seed(B)
    s, t, y = 3 * torch.randn(B, C, generator=g), 5 * torch.randn(B, C, generator=g), torch.randint(0, C, (B,), generator=g).cuda()
    table, idx = _scatter(t, rows, 9)
    buf = torch.full(((rows + 64) * C,), 3.0e38, device="cuda")
    buf[:rows * C] = table.flatten()
    front = buf[:rows * C].view(rows, C)
    canary = buf[rows * C:].clone()
    (_, p_ok, g_ok), (_, p_ok2, g_ok2) = _both(s, front[idx], front, idx, y, hp)
    assert torch.equal(p_ok, p_ok2) and torch.equal(g_ok, g_ok2)
    bad = idx.clone()
    hit = [5, B - 3]
    bad[hit[0]], bad[hit[1]] = rows, -1
    s2 = s.clone().cuda().requires_grad_(True)
    loss, parts = F.kd_ce_loss_table(s2, front, bad, y, *hp)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss)) and bool(torch.isnan(parts).all())
    nan_rows = torch.isnan(s2.grad).any(1)
    assert nan_rows.nonzero().flatten().tolist() == hit and bool(torch.isnan(s2.grad[hit]).all())
    keep = ~nan_rows
    assert torch.equal(s2.grad[keep], g_ok[keep])
    assert torch.equal(buf[rows * C:], canary) and torch.equal(front, table)
    # far outside as well
    bad[hit[0]], bad[hit[1]] = 2 ** 62, -(2 ** 62)
    s3 = s.clone().cuda().requires_grad_(True)
    loss, _ = F.kd_ce_loss_table(s3, front, bad, y, *hp)
    loss.backward()
    assert bool(torch.isnan(loss)) and torch.isnan(s3.grad).any(1).nonzero().flatten().tolist() == hit and torch.equal(s3.grad[keep], g_ok[keep])


@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_returns_the_plans_indices(native_lib, drop_last):
    data, labels = _images(203, 32, 4)
    tr = qat_vit_amd.GpuResizeNormalize(32)
    mk = lambda **kw: qat_vit_amd.GpuImageLoader(data, labels, 16, shuffle=True, drop_last=drop_last, transform=tr,   # noqa: E731
                                                 generator=torch.Generator().manual_seed(6), **kw)
    plan = qat_vit_amd.epoch_batches(203, 16, shuffle=True, drop_last=drop_last, generator=torch.Generator().manual_seed(6))
    with_index, plain = list(mk(return_index=True)), list(mk())
    assert len(with_index) == len(plain) == len(plan) == len(mk(return_index=True))
    for (x3, y3, i3), two, want in zip(with_index, plain, plan):
        assert isinstance(two, tuple) and len(two) == 2
        assert i3.dtype == torch.int64 and i3.is_cuda and torch.equal(i3.cpu(), want)
        assert torch.equal(x3, two[0]) and torch.equal(y3, two[1]) and torch.equal(y3, labels[i3])
    assert len(next(iter(qat_vit_amd.GpuImageLoader(data, labels, 16, transform=tr)))) == 2          # the default is unchanged


def _tiny_setup():
    torch.manual_seed(31)
    teacher = _frozen(VisionTransformer(embed_dim=128, depth=2, num_heads=2, num_classes=10, img_size=32))
    torch.manual_seed(32)
    stu = qat_vit_amd.create_student("vit", qat_wrapper=True, embed_dim=128, depth=2, num_heads=2, img_size=32)
    student = prepare(stu.cuda().train(), "qnnpack").cuda().train()
    data, labels = _images(40, 8, 5)
    return teacher, student, data, labels, qat_vit_amd.GpuResizeNormalize(8, out_size=32)


def _run_arm(student0, teacher, table, data, labels, tr, steps=3):
    """Three optimizer steps from a copy of student0; `table` None = the live arm.  Returns the dlogits handed to the student backward per step
    and the parameters afterwards.  In the table arm every step also evaluates the live loss on the same logits, so the comparison of the two
    gradients does not depend on the arms' parameters having stayed equal (bias / LayerNorm gradients use fp32 atomics)."""
    student = copy.deepcopy(student0)
    opt = torch.optim.AdamW(student.parameters(), lr=1e-3)
    loader = qat_vit_amd.GpuImageLoader(data, labels, 8, shuffle=True, drop_last=True, transform=tr, generator=torch.Generator().manual_seed(7),
                                        return_index=True)
    handed = []
    for k, (x, y, idx) in zip(range(steps), loader):
        opt.zero_grad(set_to_none=True)
        out = student(x)
        out.register_hook(lambda g: handed.append(g.detach().clone()))
        if table is None:
            with torch.no_grad():
                t = teacher(x)
            loss, _ = F.kd_ce_loss(out, t, y, 4.0, 0.5, 0.1)
        else:
            loss, parts = table.loss(out, idx, y, 4.0, 0.5, 0.1)
            with torch.no_grad():
                t = teacher(x)
            o2 = out.detach().clone().requires_grad_(True)
            live, live_parts = F.kd_ce_loss(o2, t, y, 4.0, 0.5, 0.1)
            live.backward()
            assert torch.equal(table.rows(idx), t), k
            assert torch.equal(parts, live_parts), k
        loss.backward()
        if table is not None:
            assert torch.equal(handed[-1], o2.grad), k
        opt.step()
    torch.cuda.synchronize()
    return handed, torch.cat([p.detach().flatten() for p in student.parameters()])


def test_a_table_step_is_the_same_step(native_lib):
    teacher, student, data, labels, tr = _tiny_setup()
    table = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16, labels=labels)      # 40 = 2 x 16 + 8: padded
    h_a1, p_a1 = _run_arm(student, teacher, None, data, labels, tr)
    h_a2, p_a2 = _run_arm(student, teacher, None, data, labels, tr)
    h_b, p_b = _run_arm(student, teacher, table, data, labels, tr)
    assert len(h_a1) == len(h_b) == 3
    assert torch.equal(h_a1[0], h_b[0]) and torch.equal(h_a1[0], h_a2[0])        # identical initial state: the first step's dlogits, across arms
    spread = float((p_a1 - p_a2).abs().max())
    d1, d2 = float((p_b - p_a1).abs().max()), float((p_b - p_a2).abs().max())
    print(f"parameters after three steps: live vs live max |d| = {spread:.3e}; table vs live = {d1:.3e}, {d2:.3e}; "
          f"dlogits of steps 2, 3 equal across arms: {[bool(torch.equal(a, b)) for a, b in zip(h_a1[1:], h_b[1:])]}")
    assert bool(torch.isfinite(p_b).all()) and float((p_b - torch.cat([p.detach().flatten() for p in student.parameters()])).abs().max()) > 0
    # the table arm is a third draw of the same step: from a live run (the nearer of the two) no further than twice what the live runs differ
    assert min(d1, d2) <= 2 * spread, (d1, d2, spread)


def test_a_changed_teacher_makes_the_table_stale(native_lib, tmp_path):
    teacher, _, data, labels, tr = _tiny_setup()
    table = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16, labels=labels)
    s, idx = torch.randn(8, 10).cuda().requires_grad_(True), torch.arange(8).cuda()
    table.loss(s, idx, labels[:8])[0].backward()
    with torch.no_grad():
        teacher.head.weight.add_(1)
    with pytest.raises(RuntimeError, match="replaced or modified"):
        table.loss(s, idx, labels[:8])
    with pytest.raises(RuntimeError, match="replaced or modified"):
        table.rows(idx)
    rebuilt = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16, labels=labels)
    assert not torch.equal(rebuilt.logits, table.logits)
    loss, _ = rebuilt.loss(s, idx, labels[:8])
    assert bool(torch.isfinite(loss))
    with torch.no_grad():
        assert torch.equal(rebuilt.rows(idx), teacher(tr(data, idx)))
    # save / load on the device, against the same inputs; then load_state_dict makes it stale
    path = os.path.join(str(tmp_path), "t.pt")
    rebuilt.save(path)
    loaded = qat_vit_amd.TeacherLogitTable.load(path, teacher=teacher, data_u8=data, transform=tr, labels=labels)
    assert loaded.logits.is_cuda and torch.equal(loaded.logits, rebuilt.logits)
    assert torch.equal(loaded.loss(s, idx, labels[:8])[1], rebuilt.loss(s, idx, labels[:8])[1])
    other = copy.deepcopy(teacher)
    with torch.no_grad():
        other.blocks[1].attn.proj.bias.add_(0.5)
    with pytest.raises(ValueError, match="param_digest differs"):
        qat_vit_amd.TeacherLogitTable.load(path, teacher=other)
    teacher.load_state_dict(other.state_dict())
    for t in (loaded, rebuilt):
        with pytest.raises(RuntimeError, match="replaced or modified"):
            t.loss(s, idx, labels[:8])
    # a teacher that trains is refused at build
    teacher.head.bias.requires_grad = True
    with pytest.raises(RuntimeError, match="require grad"):
        qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16)


def test_no_teacher_kernel_in_a_table_step(native_lib):
    from torch.profiler import ProfilerActivity, profile

    teacher, student, data, labels, tr = _tiny_setup()
    table = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=16)
    loader = qat_vit_amd.GpuImageLoader(data, labels, 8, transform=tr, return_index=True)
    x, y, idx = next(iter(loader))

    def step(use_table):
        for p in student.parameters():
            p.grad = None
        out = student(x)
        if use_table:
            loss, _ = table.loss(out, idx, y, 4.0, 0.5, 0.1)
        else:
            with torch.no_grad():
                t = teacher(x)
            loss, _ = F.kd_ce_loss(out, t, y, 4.0, 0.5, 0.1)
        loss.backward()
        torch.cuda.synchronize()

    kernels = {}
    for use_table in (False, True):
        step(use_table)       # (first step outside the profiler: workspace allocation)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(use_table)
        kernels[use_table] = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("k_teacher_head" in k for k in kernels[False]), kernels[False]
    assert any("k_kd_ce" in k and "table" not in k for k in kernels[False])
    assert not any("k_teacher_head" in k for k in kernels[True]), sorted(k for k in kernels[True] if "teacher" in k)
    assert any("k_kd_ce_table" in k for k in kernels[True]), kernels[True]
