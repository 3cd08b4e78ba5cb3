"""The observe-only native step (fake_quant_enabled = 0 on every module, torch.ao.quantization.disable_fake_quant) on an MI355X: the float
network's logits and gradients, the observers' EMA step without a scale / zero-point write, the float step's arithmetic bit for bit, switching
modes inside one engine, the refusal of mixed flags, hipGraph guards, two data-parallel ranks, and no stock GEMM / attention kernel."""
import copy
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch.ao.quantization import disable_fake_quant, disable_observer, enable_fake_quant

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd.engine import OBSERVE, QAT, engine_of, fq_modules_and_names
from tests.util import prepare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(embed_dim=128, depth=2, num_heads=2, img_size=32)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _student(seed, **kw):
    torch.manual_seed(seed)
    m = qat_vit_amd.create_model("vit_small_patch16_224_student", pretrained=False, num_classes=10, qat_wrapper=True, **kw)
    with torch.no_grad():   # non-trivial biases / LayerNorm affines / cls token so that every gradient path carries signal
        for n, p in m.named_parameters():
            if n.endswith("bias") or "norm" in n or "cls_token" in n:
                p.add_(0.05 * torch.randn_like(p))
    return m


def _qat_steps(p, n, batch, img, seed):
    """n fake-quant-on training steps (no optimizer): the observers hold state afterwards."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        x = torch.randn(batch, 3, img, img, generator=g).cuda() * 2
        y = torch.randint(0, 10, (batch,), generator=g).cuda()
        for t in p.parameters():
            t.grad = None
        F.kd_ce_loss(p(x), None, y, 4.0, 0.5, 0.1)[0].backward()
    for t in p.parameters():
        t.grad = None
    torch.cuda.synchronize()


def _fq_state(p):
    fqs, names = fq_modules_and_names(p)
    return {n: (f.activation_post_process.min_val.detach().clone(), f.activation_post_process.max_val.detach().clone(), f.scale.detach().clone(),
                f.zero_point.detach().clone()) for n, f in zip(names, fqs)}


def _observed(ref, names):
    """Forward hooks on the fp64 float tree at every point the prepared tree observes: fq name -> (min, max) of that tensor (per output channel
    for a per-channel weight quantizer: filled in by the caller)."""
    seen, hooks = {}, []
    mods = dict(ref.named_modules())
    for n in names:
        if n.endswith(".activation_post_process"):
            owner = n[: -len(".activation_post_process")]

            def hook(mod, inp, out, n=n):
                seen[n] = out.detach()

            hooks.append(mods[owner].register_forward_hook(hook))
    return seen, hooks


def _expected_ema(before, cur_min, cur_max, c=0.01):
    mn, mx = before[0].double().cpu(), before[1].double().cpu()
    emn = torch.where(torch.isinf(mn), cur_min, mn + c * (cur_min - mn))
    emx = torch.where(torch.isinf(mx), cur_max, mx + c * (cur_max - mx))
    return emn, emx


@pytest.mark.parametrize("case", [(2, 8, "qnnpack"), (2, 256, "x86"), (12, 8, "x86"), (12, 256, "qnnpack")])
def test_parity_with_fp64_float_tree(case):
    depth, batch, backend = case
    base = _student(1, depth=depth)
    p = prepare(copy.deepcopy(base).cuda(), backend)
    _qat_steps(p, 2, 8, 224, 5)
    p.apply(disable_fake_quant)
    fqs, names = fq_modules_and_names(p)
    before = _fq_state(p)
    ref = copy.deepcopy(base).double().cuda().train()
    seen, hooks = _observed(ref, names)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(batch, 3, 224, 224, generator=g)
    r = torch.randn(batch, 10, generator=g)
    out = p(x.cuda())
    (out * r.cuda()).sum().backward()
    assert engine_of(p).fq_mode == OBSERVE
    out_ref = ref(x.double().cuda())
    (out_ref * r.double().cuda()).sum().backward()
    for h in hooks:
        h.remove()
    assert rel(out, out_ref) <= 1e-4, rel(out, out_ref)
    gn = [n for n, _ in p.named_parameters()]
    assert len(gn) == 8 + 12 * depth
    ref_g = dict(ref.named_parameters())
    errs = {n: rel(t.grad, ref_g[n].grad) for n, t in p.named_parameters()}
    worst = max(errs, key=errs.get)
    assert errs[worst] <= 1e-4, (worst, errs[worst])
    after = _fq_state(p)
    ref_mods = dict(ref.named_modules())
    worst_obs = 0.0
    for n, f in zip(names, fqs):
        if n.endswith(".weight_fake_quant"):
            w = ref_mods[n[: -len(".weight_fake_quant")]].weight.detach()
            if f.is_per_channel:
                t = w.reshape(w.shape[0], -1)
                cmn, cmx = t.min(1).values.cpu(), t.max(1).values.cpu()
            else:
                cmn, cmx = w.min().cpu(), w.max().cpu()
        else:
            t = seen[n] if n != "quant.activation_post_process" else x.double()
            cmn, cmx = t.min().cpu(), t.max().cpu()
        emn, emx = _expected_ema(before[n], cmn, cmx)
        tol = 1e-5 * max(emn.abs().max().item(), emx.abs().max().item())
        e = max((after[n][0].double().cpu().reshape(emn.shape) - emn).abs().max().item(), (after[n][1].double().cpu().reshape(emx.shape) - emx).abs().max().item())
        worst_obs = max(worst_obs, e / max(tol, 1e-30) * 1e-5)
        assert e <= tol, (n, e, tol)
        assert torch.equal(after[n][2], before[n][2]) and torch.equal(after[n][3], before[n][3]), n   # scale / zero_point untouched
    print(f"depth {depth} b{batch} {backend}: logits {rel(out, out_ref):.2e}, worst gradient {worst} {errs[worst]:.2e}, observers {worst_obs:.2e}")


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_same_arithmetic_as_the_float_step(backend):
    base = _student(3, depth=2)
    p = prepare(copy.deepcopy(base).cuda(), backend)
    _qat_steps(p, 1, 4, 224, 6)
    fl = qat_vit_amd.native_float(copy.deepcopy(base).cuda().train())
    g = torch.Generator().manual_seed(7)
    x = torch.randn(16, 3, 224, 224, generator=g).cuda()
    r = torch.randn(16, 10, generator=g).cuda()
    for observers in (True, False):
        p.apply(disable_fake_quant)
        if not observers:
            p.apply(disable_observer)
        before = [b.clone() for b in p.buffers()]
        for m in (p, fl):
            for t in m.parameters():
                t.grad = None
        out, out_f = p(x), fl(x)
        out.backward(r)
        out_f.backward(r)
        assert torch.equal(out, out_f)
        for (n, a), b in zip(p.named_parameters(), fl.parameters()):
            if a.dim() >= 2 and n.endswith("weight"):
                assert torch.equal(a.grad, b.grad), n
            else:
                assert rel(a.grad, b.grad) <= 1e-6, (n, rel(a.grad, b.grad))
        if not observers:
            assert all(torch.equal(a, b) for a, b in zip(before, p.buffers()))   # observers off too: not a bit of FQ state moves
        else:
            assert not all(torch.equal(a, b) for a, b in zip(before, p.buffers()))


def test_disable_after_construction_gives_the_float_logits():
    base = _student(4, depth=2)
    p = prepare(copy.deepcopy(base).cuda(), "qnnpack")
    _qat_steps(p, 1, 4, 224, 8)
    eng = engine_of(p)
    assert eng.fq_mode == QAT
    fl = qat_vit_amd.native_float(copy.deepcopy(base).cuda().train())
    x = torch.randn(4, 3, 224, 224).cuda()
    with torch.no_grad():
        q = p(x)
        p.apply(disable_fake_quant)
        o = p(x)
        f = fl(x)
    assert engine_of(p) is eng and eng.fq_mode == OBSERVE
    assert torch.equal(o, f) and not torch.equal(q, f)


def test_on_off_on_within_one_engine(monkeypatch):
    base = _student(5, depth=2)
    a = prepare(copy.deepcopy(base).cuda(), "qnnpack")
    monkeypatch.setenv("QATVIT_DY16", "0")
    b = prepare(copy.deepcopy(base).cuda(), "qnnpack")
    with torch.no_grad():
        b(torch.zeros(8, 3, 224, 224).cuda() + 0.5)
    monkeypatch.delenv("QATVIT_DY16")
    with torch.no_grad():
        a(torch.zeros(8, 3, 224, 224).cuda() + 0.5)
    ea, eb = engine_of(a), engine_of(b)
    assert not eb.dy16
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(8, 3, 224, 224, generator=g).cuda(), torch.randint(0, 10, (8,), generator=g).cuda()) for _ in range(6)]
    modes = [QAT, QAT, OBSERVE, OBSERVE, QAT, QAT]
    for i, ((x, y), mode) in enumerate(zip(batches, modes)):
        for m in (a, b):
            m.apply(enable_fake_quant if mode == QAT else disable_fake_quant)
            for t in m.parameters():
                t.grad = None
            out = m(x)
            if m is a and ea.dy16:
                # the QAT step right after observe-only steps calibrates (pair form); the one after it is one-plane again
                if i == 4:
                    assert ea._fwd_x16 is False
                if i == 5:
                    assert ea._fwd_x16 is True
            F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)[0].backward()
        assert ea.fq_mode == eb.fq_mode == mode
    ga, gb = [t.grad for t in a.parameters()], [t.grad for t in b.parameters()]
    worst = max(rel(u, v) for u, v in zip(ga, gb))
    assert worst <= 1e-3, worst


def test_mixed_flags_raise_before_any_launch():
    p = prepare(_student(6, depth=2).cuda(), "qnnpack")
    _qat_steps(p, 1, 4, 224, 10)
    eng = engine_of(p)
    arena = eng.fq_arena.clone()
    gen = eng.generation
    p.apply(disable_fake_quant)
    p.model.blocks[0].attn.qkv.apply(enable_fake_quant)
    with pytest.raises(RuntimeError, match="model.blocks.0.attn.qkv.activation_post_process"):
        p(torch.randn(4, 3, 224, 224).cuda())
    torch.cuda.synchronize()
    assert torch.equal(eng.fq_arena, arena) and eng.generation == gen
    p.apply(disable_fake_quant)
    p(torch.randn(4, 3, 224, 224).cuda())     # all off: runs
    assert eng.fq_mode == OBSERVE


def test_hipgraph_guards():
    from qat_vit_amd.graph import GraphedStudentStep

    torch.manual_seed(0)
    p = prepare(qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **TINY).cuda(), "qnnpack")
    x = torch.randn(4, 3, 32, 32).cuda()
    y = torch.randint(0, 10, (4,)).cuda()
    step = GraphedStudentStep(p, x, y, warmup=1)
    step(x, y)
    p.apply(disable_fake_quant)
    with pytest.raises(RuntimeError, match="fake-quant flags changed since capture"):
        step(x, y)
    step.close()
    with pytest.raises(RuntimeError, match="observe-only"):
        GraphedStudentStep(p, x, y, warmup=1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _make_tiny(seed):
    torch.manual_seed(seed)
    return prepare(qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **TINY).cuda(), "qnnpack")


def _dp_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dp = _make_tiny(11 + rank)                         # replicas start different: enable_data_parallel broadcasts rank 0's
        with torch.no_grad():
            dp(torch.randn(2, 3, 32, 32).cuda())
        eng = engine_of(dp)
        eng.enable_data_parallel(bucket_bytes=64 << 10)
        g = torch.Generator().manual_seed(100)
        xs = torch.randn(2 * world, 3, 32, 32, generator=g).cuda() * 3
        ys = torch.randint(0, 10, (2 * world,), generator=g).cuda()
        dp.apply(disable_fake_quant)
        for t in dp.parameters():
            t.grad = None
        loss, _ = F.kd_ce_loss(dp(xs[2 * rank:2 * rank + 2]), None, ys[2 * rank:2 * rank + 2], 4.0, 0.5, 0.1)
        loss.backward()
        torch.cuda.synchronize()
        assert eng.fq_mode == OBSERVE
        grads = torch.cat([t.grad.flatten() for t in dp.parameters()]).cpu()
        state = torch.cat([b.detach().double().flatten() for b in _fq_buffers(dp)]).cpu()
        q.put((rank, grads.numpy(), state.numpy(), None))   # (numpy: pickled by value - a tensor would be a handle into this process)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, None, None, traceback.format_exc()[-2000:]))


def _fq_buffers(p):
    return [b for n, b in p.named_buffers() if "fake_quant_enabled" not in n and "observer_enabled" not in n]


@pytest.mark.timeout(600)
def test_two_ranks_one_gpu_observe_only(native_lib):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=480) for _ in procs], key=lambda t: t[0])
    for pr in procs:
        pr.join(60)
    assert all(e is None for *_, e in res), [e for *_, e in res]
    (_, g0, s0, _), (_, g1, s1, _) = [(r, torch.from_numpy(g), torch.from_numpy(s), e) for r, g, s, e in res]
    assert torch.equal(g0, g1)                                # one averaged gradient on both ranks
    # single process: rank 0's model and state (the training forward starts from rank 0's broadcast state on every rank), each shard observed
    # from that state; the gradient is the mean of the two shards' gradients
    single = _make_tiny(11)
    with torch.no_grad():
        single(torch.randn(2, 3, 32, 32).cuda())
    single.apply(disable_fake_quant)
    start = [b.clone() for b in _fq_buffers(single)]
    g = torch.Generator().manual_seed(100)
    xs = torch.randn(4, 3, 32, 32, generator=g).cuda() * 3
    ys = torch.randint(0, 10, (4,), generator=g).cuda()
    grads, states = [], []
    for r in range(2):
        with torch.no_grad():
            for b, v in zip(_fq_buffers(single), start):
                b.copy_(v)
        for t in single.parameters():
            t.grad = None
        F.kd_ce_loss(single(xs[2 * r:2 * r + 2]), None, ys[2 * r:2 * r + 2], 4.0, 0.5, 0.1)[0].backward()
        grads.append(torch.cat([t.grad.flatten() for t in single.parameters()]).cpu())
        states.append(torch.cat([b.detach().double().flatten() for b in _fq_buffers(single)]).cpu())
    mean = (grads[0] + grads[1]) / 2
    assert rel(g0, mean) <= 1e-6, rel(g0, mean)
    assert torch.equal(s0, states[0]) and torch.equal(s1, states[1])
    assert not torch.equal(states[0], states[1])              # (the shards differ: the comparison above sees the broadcast)


def test_observe_only_step_runs_only_native_kernels():
    from torch.profiler import ProfilerActivity, profile

    p = prepare(_student(14, depth=2).cuda(), "x86")
    p.apply(disable_fake_quant)
    x = torch.randn(4, 3, 224, 224).cuda()
    r = torch.randn(4, 10).cuda()
    p(x).backward(r)   # (first step outside the profiler: the engine and the observe-only buffers)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for t in p.parameters():
            t.grad = None
        p(x).backward(r)
        torch.cuda.synchronize()
    assert engine_of(p).fq_mode == OBSERVE
    names = {e.name for e in prof.events()}
    banned = ("aten::mm", "aten::addmm", "aten::bmm", "aten::matmul", "aten::linear", "aten::conv2d", "aten::convolution", "aten::softmax",
              "aten::_softmax", "aten::layer_norm", "aten::native_layer_norm", "aten::gelu", "scaled_dot_product", "fused_moving_avg_obs_fake_quant")
    hit = sorted(n for n in names if any(n.startswith(b) or b in n for b in banned))
    assert not hit, hit
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("k_obs_fold" in k for k in kernels), kernels
    other = sorted(k for k in kernels if "qv::" not in k and not any(s in k.lower() for s in ("fill", "copy", "memset", "memcpy", "elementwise")))
    assert not other, other
