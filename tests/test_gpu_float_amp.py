"""The fp16 (autocast) form of the native float student step (native_float(wrapper, amp=True)) on an MI355X: parity with the fp64 tree
next to stock autocast, the fp16 attention backward against an fp64 restatement, GradScaler's skip behaviour, the trajectory next to
stock autocast + GradScaler, switching forms in one engine, and that no stock GEMM / attention / norm kernel runs in an autocast step."""
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


def _opted(m, amp=True):
    return qat_vit_amd.native_float(m.cuda().train(), amp=amp)


@pytest.mark.parametrize("case", [("vit_small_patch16_224_student", 8), ("vit_small_patch16_224_student", 256), ("vit_base_patch16_224_teacher", 8)])
def test_parity_with_fp64_tree_next_to_stock_autocast(case):
    name, batch = case
    base = _student(1, name)
    ref = copy.deepcopy(base).double().cuda()
    stock = copy.deepcopy(base).cuda().train()
    m = _opted(base)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    r = torch.randn(batch, 10, generator=g).cuda()
    with torch.autocast("cuda", dtype=torch.float16):
        out = m(x)
        out_s = stock(x)
    assert out.dtype == torch.float16 and out_s.dtype == torch.float16 and out.shape == (batch, 10)
    (out.float() * r).sum().backward()
    (out_s.float() * r).sum().backward()
    out_ref = ref(x.double())
    (out_ref * r.double()).sum().backward()
    names = ["logits"] + [n for n, _ in m.named_parameters()]
    assert len(names) == 153
    nat = [rel(out, out_ref)] + [rel(a, b) for a, b in zip(_grads(m), _grads(ref))]
    sto = [rel(out_s, out_ref)] + [rel(a, b) for a, b in zip(_grads(stock), _grads(ref))]
    print(f"\n{name} b{batch}: relative L2 against fp64 (native / stock autocast)")
    for n, a, b in zip(names, nat, sto):
        print(f"  {n:40s} {a:.2e} {b:.2e}")
    bad = [(n, a, b) for n, a, b in zip(names, nat, sto) if a > max(2 * b, 1e-4) or a > 1e-2]
    assert not bad, bad


@pytest.mark.parametrize("hd", [64, 32])
def test_attention_backward_kernel_against_fp64(hd):
    B, T, H = 16, 197, 6 if hd == 64 else 12
    D = H * hd
    g = torch.Generator().manual_seed(hd)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).cuda()
    dO = (torch.randn(B * T, D, generator=g) * 1e-2).cuda()
    q, k, v = qkv.half().double().view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    do = dO.half().double().view(B, T, H, hd).transpose(1, 2)
    s = hd ** -0.5
    S = s * q @ k.transpose(-1, -2)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O = P @ v
    dV = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - (do * O).sum(-1, keepdim=True))
    dQ, dK = s * dS @ k, s * dS.transpose(-1, -2) @ q
    O16 = O.transpose(1, 2).reshape(B * T, D).half().contiguous()
    lse32 = lse.float().contiguous()
    lib = native.lib()
    dqkv, canary = guarded(B * T, 3 * D, torch.float16, "cuda")
    native.check(lib.qatvit_float_student_amp_attn_backward(qkv.data_ptr(), O16.data_ptr(), lse32.data_ptr(), dO.data_ptr(), B, T, H, D, dqkv.data_ptr(),
                                                            native.stream_ptr()), "qatvit_float_student_amp_attn_backward")
    torch.cuda.synchronize()
    got = dqkv.double().view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    errs = [rel(got[i], want) for i, want in enumerate((dQ, dK, dV))]
    print(f"\nhead_dim {hd}: dQ {errs[0]:.2e} dK {errs[1]:.2e} dV {errs[2]:.2e}")
    assert torch.isfinite(dqkv).all()
    assert max(errs) <= 3e-3, errs
    canary("dqkv")
    want2d = torch.stack((dQ, dK, dV)).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * D)      # the qkv layout of the output
    for name, c0 in (("dQ", 0), ("dK", D), ("dV", 2 * D)):
        assert_tiles_close(dqkv[:, c0:c0 + D], want2d[:, c0:c0 + D], 3e-3, what=name)


def _scaled_grads_finite(model, x, y, scale):
    for p in model.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.float16):
        out = model(x)
        loss = TF.cross_entropy(out, y)
    out.retain_grad()
    (loss * scale).backward()
    dl_finite = bool(torch.isfinite(out.grad).all())
    return all(bool(torch.isfinite(p.grad).all()) for p in model.parameters()), dl_finite


def test_grad_scaler_skips_where_stock_does():
    base = _student(5, **D2)
    stock = copy.deepcopy(base).cuda().train()
    m = _opted(base)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(64, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 10, (64,), generator=g).cuda()
    for model in (stock, m):   # the reference's init_scale: no step skipped
        opt = qat_vit_amd.ClipAdamW(model.parameters(), lr=1e-4)
        scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            loss = TF.cross_entropy(model(x), y)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() == 65536.0
    # the smallest power-of-two scale at which stock overflows (batch 64: its fp16 dlogits are then still finite, a gradient inside the
    # network overflows first)
    k = next(k for k in range(16, 48) if not _scaled_grads_finite(stock, x, y, 2.0 ** k)[0])
    print(f"\nstock overflows from 2^{k}")
    assert _scaled_grads_finite(stock, x, y, 2.0 ** k)[1], k
    assert not _scaled_grads_finite(m, x, y, 2.0 ** (k + 2))[0]
    assert _scaled_grads_finite(m, x, y, 2.0 ** (k - 2))[0]
    # and GradScaler skips that step natively (a skip halves the scale)
    opt = qat_vit_amd.ClipAdamW(m.parameters(), lr=1e-4)
    before = [p.detach().clone() for p in m.parameters()]
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** (k + 2))
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = TF.cross_entropy(m(x), y)
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 2.0 ** (k + 1)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, m.parameters()))


def test_trajectory_next_to_stock_autocast():
    base = _student(3, **D2)
    stock = copy.deepcopy(base).cuda().train()
    m = _opted(base)
    runs = []
    for model in (m, stock):
        opt = qat_vit_amd.ClipAdamW(model.parameters(), lr=1e-4)
        scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
        g = torch.Generator().manual_seed(4)
        losses, scales = [], []
        for _ in range(10):
            x = torch.randn(16, 3, 224, 224, generator=g).cuda()
            y = torch.randint(0, 10, (16,), generator=g).cuda()
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16):
                loss, _ = F.kd_ce_loss(model(x).float(), None, y, 4.0, 0.5, 0.1)
            scaler.scale(loss).backward()
            scaler.unscale_(opt)
            scaler.step(opt)
            scaler.update()
            losses.append(loss.item())
            scales.append(scaler.get_scale())
        runs.append((losses, scales))
    (ln, sn), (ls, ss) = runs
    print("\nnative", ln, "\nstock ", ls)
    for step, (a, b) in enumerate(zip(ln, ls)):
        assert abs(a - b) <= 1e-2 * abs(b), (step, a, b)
    assert sn == ss


def test_form_switching_in_one_engine():
    base = _student(7, **D2)
    plain = _opted(copy.deepcopy(base), amp=False)
    m = _opted(base)
    g = torch.Generator().manual_seed(8)
    names = [n for n, _ in m.named_parameters()]
    for batch in (8, 5, 1024, 3):
        x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
        r = torch.randn(batch, 10, generator=g).cuda()
        for model in (m, plain):
            for p in model.parameters():
                p.grad = None
        out, out_p = m(x), plain(x)   # (the plain engine runs between m's forward and backward: separate engines)
        assert out.dtype == torch.float32 and torch.equal(out, out_p)
        out.backward(r)
        out_p.backward(r)
        for n, a, b in zip(names, _grads(m), _grads(plain)):
            if n.endswith("weight") and "norm" not in n:
                assert torch.equal(a, b), n
            else:
                assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), n
        for p in m.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.float16):
            o16 = m(x)
        assert o16.dtype == torch.float16 and torch.isfinite(o16).all()
        o16.backward(r.half())
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    eng = engine_of(m)
    assert eng.capacity16 == 1024 and eng.capacity == 1024
    # a forward of one form, then a forward of the other before the first one's backward
    x = torch.randn(4, 3, 224, 224).cuda()
    a = m(x)
    with torch.autocast("cuda", dtype=torch.float16):
        b = m(x)
    with pytest.raises(RuntimeError, match="another forward"):
        a.sum().backward()
    b.float().sum().backward()
    with pytest.raises(RuntimeError, match="autocast dtype"):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            m(x)
    # amp=False keeps today's behaviour inside autocast: fp32 logits
    with torch.autocast("cuda", dtype=torch.float16):
        assert plain(x).dtype == torch.float32


def test_autocast_step_runs_only_native_kernels():
    from torch.profiler import ProfilerActivity, profile

    m = _opted(_student(14, **D2))
    x = torch.randn(4, 3, 224, 224).cuda()
    r = torch.randn(4, 10).cuda().half()
    with torch.autocast("cuda", dtype=torch.float16):
        out = m(x)
    out.backward(r)   # (first step outside the profiler: workspace allocation)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for p in m.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.float16):
            out = m(x)
        out.backward(r)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    banned = ("aten::mm", "aten::addmm", "aten::bmm", "aten::matmul", "aten::linear", "aten::conv2d", "aten::convolution", "aten::softmax",
              "aten::_softmax", "aten::layer_norm", "aten::native_layer_norm", "aten::gelu", "scaled_dot_product")
    hit = sorted(n for n in names if any(n.startswith(b) or b in n for b in banned))
    assert not hit, hit
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("k_fa_attn_bwd_fused" in k for k in kernels), kernels
    other = sorted(k for k in kernels if "qv::" not in k and "_ZN2qv" not in k and not any(s in k.lower() for s in ("fill", "copy", "memset", "memcpy", "elementwise")))
    assert not other, other


def test_forced_linear_weight_gradient_overflow_is_skipped():
    # a larger final-norm gain scales the head's input: its weight gradient (a fp16 tensor in stock, an fp32 sum here) passes 65,504 while the
    # fp16 dlogits and everything upstream stay finite; the native form must turn it into inf (k_fa_inf_rule), so GradScaler skips the step
    base = _student(21, **D2)
    with torch.no_grad():
        base.model.norm.weight.mul_(8.0)
    stock = copy.deepcopy(base).cuda().train()
    m = _opted(base)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(64, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 10, (64,), generator=g).cuda()
    out = stock(x)   # fp32 magnitudes at scale 1 pick the scale
    out.retain_grad()
    TF.cross_entropy(out, y).backward()
    mw, ml = stock.model.head.weight.grad.abs().max().item(), out.grad.abs().max().item()
    k = 1
    while mw * 2.0 ** k <= 1.5 * 65504:
        k += 1
    assert ml * 2.0 ** k < 0.5 * 65504, (mw, ml, k)
    scale = 2.0 ** k
    for model in (stock, m):
        for p in model.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.float16):
            o = model(x)
            loss = TF.cross_entropy(o, y)
        o.retain_grad()
        (loss * scale).backward()
        assert torch.isfinite(o.grad).all()
        assert not torch.isfinite(model.model.head.weight.grad).all()
    opt = qat_vit_amd.ClipAdamW(m.parameters(), lr=1e-4)
    before = [p.detach().clone() for p in m.parameters()]
    scaler = torch.amp.GradScaler("cuda", init_scale=scale)
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = TF.cross_entropy(m(x), y)
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == scale / 2
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, m.parameters()))


def test_stock_ddp_single_rank_with_grad_scaler():
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
            opt = qat_vit_amd.ClipAdamW(params(), lr=1e-4)
            scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
            with torch.autocast("cuda", dtype=torch.float16):
                out = model(x)
                loss = F.kd_ce_loss(out.float(), None, y, 4.0, 0.5, 0.1)[0]
            scaler.scale(loss).backward()
            scaler.unscale_(opt)
            torch.cuda.synchronize()
            outs.append(out.detach())
            grads.append([p.grad.clone() for p in params()])
        assert outs[0].dtype == torch.float16 and torch.equal(outs[0], outs[1])
        for (n, _), a, b in zip(m.named_parameters(), grads[0], grads[1]):
            if n.endswith("weight") and "norm" not in n:
                assert torch.equal(a, b), n
            else:
                assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), n
    finally:
        dist.destroy_process_group()
