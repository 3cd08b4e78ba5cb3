"""The bf16 (autocast) form of the native float student step (native_float(wrapper, amp=torch.bfloat16)) on an MI355X: parity with the fp64
tree next to stock bf16 autocast, the bf16 attention backward against an fp64 restatement, the trajectory next to stock bf16 autocast,
switching between the three forms in one engine, that no stock GEMM / attention / norm kernel runs in a bf16 autocast step, single-rank DDP,
and that a NaN input reaches the gradients as in stock."""
import copy
import os
import socket

import pytest
import torch
import torch.nn.functional as TF

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native
from qat_vit_amd.float_engine import engine_of
from tests.kernel_check import assert_tiles_close, guarded

pytestmark = pytest.mark.gpu
D2 = dict(depth=2)   # ViT-S width (384, 6 heads), two blocks
BF = torch.bfloat16


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


def _opted(m, amp=BF):
    return qat_vit_amd.native_float(m.cuda().train(), amp=amp)


def _linear_weight(n):
    return n.endswith("weight") and "norm" not in n


@pytest.mark.parametrize("case", [("vit_small_patch16_224_student", 8), ("vit_small_patch16_224_student", 256), ("vit_base_patch16_224_teacher", 8)])
def test_parity_with_fp64_tree_next_to_stock_bf16_autocast(case):
    name, batch = case
    base = _student(1, name)
    ref = copy.deepcopy(base).double().cuda()
    stock = copy.deepcopy(base).cuda().train()
    m = _opted(base)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    r = torch.randn(batch, 10, generator=g).cuda()
    with torch.autocast("cuda", dtype=BF):
        out = m(x)
        out_s = stock(x)
    assert out.dtype == BF and out_s.dtype == BF and out.shape == (batch, 10)
    (out.float() * r).sum().backward()
    (out_s.float() * r).sum().backward()
    out_ref = ref(x.double())
    (out_ref * r.double()).sum().backward()
    names = ["logits"] + [n for n, _ in m.named_parameters()]
    assert len(names) == 153
    nat = [rel(out, out_ref)] + [rel(a, b) for a, b in zip(_grads(m), _grads(ref))]
    sto = [rel(out_s, out_ref)] + [rel(a, b) for a, b in zip(_grads(stock), _grads(ref))]
    print(f"\n{name} b{batch}: relative L2 against fp64 (native bf16 / stock bf16 autocast)")
    for n, a, b in zip(names, nat, sto):
        print(f"  {n:40s} {a:.2e} {b:.2e}")
    bad = [(n, a, b) for n, a, b in zip(names, nat, sto) if a > max(2 * b, 1e-4) or a > 5e-2]
    assert not bad, bad


@pytest.mark.parametrize("hd", [64, 32])
def test_attention_backward_kernel_against_fp64(hd):
    B, T, H = 16, 197, 6 if hd == 64 else 12   # B * H = 96 / 192
    D = H * hd
    g = torch.Generator().manual_seed(hd)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).cuda()
    dO = (torch.randn(B * T, D, generator=g) * 1e-2).cuda()
    q, k, v = qkv.to(BF).double().view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    do = dO.to(BF).double().view(B, T, H, hd).transpose(1, 2)
    s = hd ** -0.5
    S = s * q @ k.transpose(-1, -2)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O = P @ v
    dV = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - (do * O).sum(-1, keepdim=True))
    dQ, dK = s * dS @ k, s * dS.transpose(-1, -2) @ q
    O16 = O.transpose(1, 2).reshape(B * T, D).to(BF).contiguous()
    lse32 = lse.float().contiguous()
    lib = native.lib()
    dqkv, canary = guarded(B * T, 3 * D, BF, "cuda")
    native.check(lib.qatvit_float_student_bf16_attn_backward(qkv.data_ptr(), O16.data_ptr(), lse32.data_ptr(), dO.data_ptr(), B, T, H, D,
                                                             dqkv.data_ptr(), native.stream_ptr()), "qatvit_float_student_bf16_attn_backward")
    torch.cuda.synchronize()
    got = dqkv.double().view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    errs = [rel(got[i], want) for i, want in enumerate((dQ, dK, dV))]
    print(f"\nhead_dim {hd}: dQ {errs[0]:.2e} dK {errs[1]:.2e} dV {errs[2]:.2e}")
    assert torch.isfinite(dqkv).all()
    assert max(errs) <= 2.5e-2, errs
    canary("dqkv")
    want2d = torch.stack((dQ, dK, dV)).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * D)      # the qkv layout of the output
    for name, c0 in (("dQ", 0), ("dK", D), ("dV", 2 * D)):
        assert_tiles_close(dqkv[:, c0:c0 + D], want2d[:, c0:c0 + D], 2.5e-2, what=name)


def test_trajectory_next_to_stock_bf16_autocast():
    base = _student(3, **D2)
    stock = copy.deepcopy(base).cuda().train()
    m = _opted(base)
    runs = []
    for model in (m, stock):
        opt = qat_vit_amd.ClipAdamW(model.parameters(), lr=1e-4)
        g = torch.Generator().manual_seed(4)
        losses = []
        for _ in range(10):
            x = torch.randn(64, 3, 224, 224, generator=g).cuda()
            y = torch.randint(0, 10, (64,), generator=g).cuda()
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=BF):
                loss, _ = F.kd_ce_loss(model(x).float(), None, y, 4.0, 0.5, 0.1)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        runs.append(losses)
    ln, ls = runs
    print("\nnative", ln, "\nstock ", ls)
    for step, (a, b) in enumerate(zip(ln, ls)):
        assert abs(a - b) <= 2e-3 * abs(b), (step, a, b)


def _step(model, x, r, dtype=None):
    for p in model.parameters():
        p.grad = None
    if dtype is None:
        out = model(x)
    else:
        with torch.autocast("cuda", dtype=dtype):
            out = model(x)
    out.backward(r.to(out.dtype))
    return out.detach(), [p.grad.clone() for p in model.parameters()]


def test_form_switching_in_one_engine():
    base = _student(7, **D2)
    plain = _opted(copy.deepcopy(base), amp=False)
    fp16 = _opted(copy.deepcopy(base), amp=True)
    m = _opted(base, amp=(torch.float16, BF))
    eng = engine_of(m)
    names = [n for n, _ in m.named_parameters()]
    g = torch.Generator().manual_seed(8)
    x = torch.randn(8, 3, 224, 224, generator=g).cuda()
    r = torch.randn(8, 10, generator=g).cuda()
    assert eng.fp32.workspace is None and eng.fp16.workspace is None and eng.bf16.workspace is None
    # fp32 -> bf16 -> fp16 -> bf16, each with its backward; each workspace is allocated by its own form only
    o32, g32 = _step(m, x, r)
    assert eng.fp32.workspace is not None and eng.fp16.workspace is None and eng.bf16.workspace is None
    ob1, gb1 = _step(m, x, r, BF)
    assert eng.bf16.workspace is not None and eng.fp16.workspace is None
    o16, g16 = _step(m, x, r, torch.float16)
    assert eng.fp16.workspace is not None
    ob2, gb2 = _step(m, x, r, BF)
    assert (o32.dtype, ob1.dtype, o16.dtype, ob2.dtype) == (torch.float32, BF, torch.float16, BF)
    p32, pg32 = _step(plain, x, r)
    p16, pg16 = _step(fp16, x, r, torch.float16)
    assert torch.equal(o32, p32) and torch.equal(o16, p16) and torch.equal(ob1, ob2)
    for n, a32, b32, a16, b16, c1, c2 in zip(names, g32, pg32, g16, pg16, gb1, gb2):
        assert torch.isfinite(c1).all(), n
        if _linear_weight(n):
            assert torch.equal(a32, b32) and torch.equal(a16, b16) and torch.equal(c1, c2), n
        else:
            for a, b in ((a32, b32), (a16, b16), (c1, c2)):
                assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), n
    # a forward of one form, then a forward of another before the first one's backward
    with torch.autocast("cuda", dtype=BF):
        a = m(x)
    with torch.autocast("cuda", dtype=torch.float16):
        b = m(x)
    with pytest.raises(RuntimeError, match="another forward"):
        a.float().sum().backward()
    b.float().sum().backward()
    c = m(x)
    with torch.autocast("cuda", dtype=BF):
        d = m(x)
    with pytest.raises(RuntimeError, match="another forward"):
        c.sum().backward()
    d.float().sum().backward()
    # a bf16-only engine: no fp16 workspace, and fp16 autocast raises
    only = _opted(_student(9, **D2))
    _step(only, x, r, BF)
    e = engine_of(only)
    assert e.bf16.workspace is not None and e.fp16.workspace is None and e.fp32.workspace is None
    with pytest.raises(RuntimeError, match="autocast dtype"):
        with torch.autocast("cuda", dtype=torch.float16):
            only(x)


def test_bf16_autocast_step_runs_only_native_kernels():
    from torch.profiler import ProfilerActivity, profile

    m = _opted(_student(14, **D2))
    x = torch.randn(4, 3, 224, 224).cuda()
    r = torch.randn(4, 10).cuda().to(BF)
    with torch.autocast("cuda", dtype=BF):
        out = m(x)
    out.backward(r)   # (first step outside the profiler: workspace allocation)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for p in m.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=BF):
            out = m(x)
        out.backward(r)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    banned = ("aten::mm", "aten::addmm", "aten::bmm", "aten::matmul", "aten::linear", "aten::conv2d", "aten::convolution", "aten::softmax",
              "aten::_softmax", "aten::layer_norm", "aten::native_layer_norm", "aten::gelu", "scaled_dot_product")
    hit = sorted(n for n in names if any(n.startswith(b) or b in n for b in banned))
    assert not hit, hit
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("k_fa_attn_bwd_fused" in k and ("__bf16" in k or "DF16b" in k) for k in kernels), kernels   # (DF16b: __bf16 mangled)
    other = sorted(k for k in kernels if "qv::" not in k and "_ZN2qv" not in k and not any(s in k.lower() for s in ("fill", "copy", "memset", "memcpy", "elementwise")))
    assert not other, other


def test_stock_ddp_single_rank_bf16():
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
        grads, outs = [], []
        for model, params in ((ddp, m.parameters), (plain, plain.parameters)):
            with torch.autocast("cuda", dtype=BF):
                out = model(x)
                loss = F.kd_ce_loss(out.float(), None, y, 4.0, 0.5, 0.1)[0]
            loss.backward()
            torch.cuda.synchronize()
            outs.append(out.detach())
            grads.append([p.grad.clone() for p in params()])
        assert outs[0].dtype == BF and torch.equal(outs[0], outs[1])
        for (n, _), a, b in zip(m.named_parameters(), grads[0], grads[1]):
            if _linear_weight(n):
                assert torch.equal(a, b), n
            else:
                assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), n
    finally:
        dist.destroy_process_group()


def test_nan_input_reaches_the_gradients_as_in_stock():
    base = _student(21, **D2)
    stock = copy.deepcopy(base).cuda().train()
    m = _opted(base)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(16, 3, 224, 224, generator=g).cuda()
    x[3, 1, 100, 37] = float("nan")
    y = torch.randint(0, 10, (16,), generator=g).cuda()
    finite = []
    for model in (stock, m):
        for p in model.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=BF):
            loss = TF.cross_entropy(model(x), y)
        loss.backward()
        finite.append([bool(torch.isfinite(p.grad).all()) for p in model.parameters()])
    names = [n for n, _ in m.named_parameters()]
    assert not all(finite[0])
    missed = [n for n, s, nat in zip(names, *finite) if not s and nat]
    assert not missed, missed
    # GradScaler with bf16 autocast skips that step, as for stock
    for model in (stock, m):
        opt = qat_vit_amd.ClipAdamW(model.parameters(), lr=1e-4)
        before = [p.detach().clone() for p in model.parameters()]
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF):
            loss = TF.cross_entropy(model(x), y)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() == 512.0
        assert all(torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
