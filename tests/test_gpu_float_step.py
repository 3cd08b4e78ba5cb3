"""The native float (pre-QAT) student step (qat_vit_amd.native_float, float_engine.py) on an MI355X: parity with the fp64 tree, the
trajectory next to stock fp32 torch, autocast + GradScaler, run-time batch sizes, prepare_qat after the opt-in, the forward guard, stock
DDP on top, and that no stock GEMM / attention kernel runs in an opted-in step."""
import copy
import os
import socket

import pytest
import torch
import torch.nn.functional as TF

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd.float_engine import engine_of

pytestmark = pytest.mark.gpu
D2 = dict(depth=2)   # ViT-S width (384, 6 heads), two blocks


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _student(seed, name="vit_small_patch16_224_student", **kw):
    torch.manual_seed(seed)
    m = qat_vit_amd.create_model(name, pretrained=False, num_classes=10, qat_wrapper=True, **kw)
    with torch.no_grad():   # non-trivial biases / LayerNorm affines / cls token so that every gradient path carries signal
        for n, p in m.named_parameters():
            if n.endswith("bias") or "norm" in n or "cls_token" in n:
                p.add_(0.05 * torch.randn_like(p))
    return m


def _grads(m):
    return [p.grad for p in m.parameters()]


def _opted(m):
    return qat_vit_amd.native_float(m.cuda().train())


@pytest.mark.parametrize("case", [("vit_small_patch16_224_student", 8), ("vit_small_patch16_224_student", 256), ("vit_base_patch16_224_teacher", 8)])
def test_parity_with_fp64_tree(case):
    name, batch = case
    base = _student(1, name)
    ref = copy.deepcopy(base).double().cuda()
    m = _opted(base)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(batch, 3, 224, 224, generator=g)
    r = torch.randn(batch, 10, generator=g)
    out = m(x.cuda())
    assert out.dtype == torch.float32 and out.shape == (batch, 10)
    (out * r.cuda()).sum().backward()
    out_ref = ref(x.double().cuda())
    (out_ref * r.double().cuda()).sum().backward()
    assert rel(out, out_ref) <= 1e-4, rel(out, out_ref)
    names = [n for n, _ in m.named_parameters()]
    assert len(names) == (152 if name.startswith("vit_small") or name.startswith("vit_base") else len(names))
    errs = {n: rel(a, b) for n, a, b in zip(names, _grads(m), _grads(ref))}
    worst = max(errs, key=errs.get)
    print(f"{name} b{batch}: logits {rel(out, out_ref):.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert errs[worst] <= 1e-4, (worst, errs[worst])


def test_trajectory_next_to_stock_fp32():
    base = _student(3, **D2)
    stock = copy.deepcopy(base).cuda().train()
    m = _opted(base)
    o1 = qat_vit_amd.ClipAdamW(m.parameters(), lr=1e-4)
    o2 = qat_vit_amd.ClipAdamW(stock.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(4)
    for step in range(10):
        x = torch.randn(16, 3, 224, 224, generator=g).cuda()
        y = torch.randint(0, 10, (16,), generator=g).cuda()
        losses = []
        for model, opt in ((m, o1), (stock, o2)):
            opt.zero_grad(set_to_none=True)
            loss, _ = F.kd_ce_loss(model(x), None, y, 4.0, 0.5, 0.1)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        assert abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[1]), (step, losses)


def test_autocast_and_grad_scaler():
    base = _student(5, **D2)
    m = _opted(base)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(8, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 10, (8,), generator=g).cuda()
    TF.cross_entropy(m(x), y).backward()
    plain = [p.grad.clone() for p in m.parameters()]
    opt = qat_vit_amd.ClipAdamW(m.parameters(), lr=1e-4)
    opt.zero_grad(set_to_none=True)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    with torch.autocast("cuda", dtype=torch.float16):
        out = m(x)
        loss = TF.cross_entropy(out, y)
    assert out.dtype == torch.float32
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    for p, ref in zip(m.parameters(), plain):
        assert torch.isfinite(p.grad).all()
        assert rel(p.grad, ref) <= 1e-6
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 65536.0   # no step skipped (a skip halves the scale)


def test_batch_sizes_in_one_engine():
    base = _student(7, **D2)
    fresh = copy.deepcopy(base)
    m = _opted(base)
    g = torch.Generator().manual_seed(8)
    xb = torch.randn(1024, 3, 224, 224, generator=g).cuda()
    x7 = torch.randn(7, 3, 224, 224, generator=g).cuda()
    m(xb).sum().backward()
    eng = engine_of(m)
    assert eng.capacity == 1024 and eng.workspace.numel() == eng.workspace_bytes(1024)
    for p in m.parameters():
        p.grad = None
    out = m(x7)
    out.sum().backward()
    assert engine_of(m) is eng and eng.workspace.numel() == eng.workspace_bytes(1024)
    f = _opted(fresh)
    out_f = f(x7)
    out_f.sum().backward()
    assert engine_of(f).capacity == 7
    assert torch.equal(out, out_f)
    for (n, p), q in zip(m.named_parameters(), f.parameters()):
        assert rel(p.grad, q.grad) <= 1e-6, n   # (bias / LayerNorm column sums are atomics: their order differs run to run)


def test_prepare_qat_after_opt_in():
    from torch.ao.quantization import get_default_qat_qconfig, prepare_qat

    base = _student(9, **D2).cuda().train()
    never = copy.deepcopy(base)
    m = qat_vit_amd.native_float(base)
    for w in (m, never):
        w.qconfig = get_default_qat_qconfig("qnnpack")
    p1 = prepare_qat(m, inplace=False).cuda().train()
    p2 = prepare_qat(never, inplace=False).cuda().train()
    assert not qat_vit_amd.float_engine.is_native_float(p1)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(4, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 10, (4,), generator=g).cuda()
    outs = []
    for p in (p1, p2):
        out = p(x)
        F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)[0].backward()
        outs.append(out.detach())
    from qat_vit_amd.engine import engine_of as qat_engine_of

    assert qat_engine_of(p1) is not None and qat_engine_of(p2) is not None
    assert torch.equal(outs[0], outs[1])
    for (n, a), b in zip(p1.named_parameters(), p2.parameters()):
        assert rel(a.grad, b.grad) <= 1e-6, n
    for n, b in p2.named_buffers():
        assert torch.equal(dict(p1.named_buffers())[n], b), n
    out = m(x)                       # the float original still runs its native step
    F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)[0].backward()
    assert engine_of(m) is not None and all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_second_forward_before_backward_raises():
    m = _opted(_student(11, **D2))
    x = torch.randn(2, 3, 224, 224).cuda()
    out1 = m(x)
    m(x)
    with pytest.raises(RuntimeError, match="another forward"):
        out1.sum().backward()


def test_stock_ddp_single_rank():
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP

    base = _student(12, **D2)
    plain = _opted(copy.deepcopy(base))
    m = _opted(base)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(4, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 10, (4,), generator=g).cuda()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        ddp = DDP(m, device_ids=[0])
        out = ddp(x)
        F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)[0].backward()
        out_p = plain(x)
        F.kd_ce_loss(out_p, None, y, 4.0, 0.5, 0.1)[0].backward()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), out_p.detach())
        for (n, a), b in zip(m.named_parameters(), plain.parameters()):
            assert rel(a.grad, b.grad) <= 1e-6, n
    finally:
        dist.destroy_process_group()


def test_opted_in_step_runs_only_native_kernels():
    from torch.profiler import ProfilerActivity, profile

    m = _opted(_student(14, **D2))
    x = torch.randn(4, 3, 224, 224).cuda()
    r = torch.randn(4, 10).cuda()
    m(x).backward(r)   # (first step outside the profiler: workspace allocation)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for p in m.parameters():
            p.grad = None
        m(x).backward(r)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    banned = ("aten::mm", "aten::addmm", "aten::bmm", "aten::matmul", "aten::linear", "aten::conv2d", "aten::convolution", "aten::softmax",
              "aten::_softmax", "aten::layer_norm", "aten::native_layer_norm", "aten::gelu", "scaled_dot_product")
    hit = sorted(n for n in names if any(n.startswith(b) or b in n for b in banned))
    assert not hit, hit
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("qv::" in k for k in kernels), kernels
    other = sorted(k for k in kernels if "qv::" not in k and not any(s in k.lower() for s in ("fill", "copy", "memset", "memcpy", "elementwise")))
    assert not other, other
