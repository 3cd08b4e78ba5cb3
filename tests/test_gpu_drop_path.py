"""Stochastic depth (drop-path) in the native float step (all three forms) and the native QAT step, on an MI355X.

Every check runs under ``qat_vit_amd.forced_drop_path``: the table holds a different multiplier for every (branch, sample) - from {0, 0.5, 1.25, 2.0}, a zero and
a non-zero in every row - so a wrong sample index shows in the per-image logits and in every gradient.  Shapes: the smallest at which the row -> sample map
(T not a power of two, several workgroups), the column-group count (embed_dim 128 / 384 / 768) and each gradient form (bf16 pair, one fp16 plane, one bf16 plane,
the class-token rows of the last block) can go wrong.  Measured values: profiles/drop_path_bench.txt."""
import copy
import functools

import pytest
import torch

import qat_vit_amd
from oracle import step_ref
from oracle.vit_ref import RefVisionTransformer, randomize_
from qat_vit_amd import DropPath, forced_drop_path
from qat_vit_amd import functional as F
from qat_vit_amd.engine import engine_of
from qat_vit_amd.graph import GraphedStudentStep
from tests.test_gpu_float_shapes import FORMS, SEEDS, _assert_ran_natively, _errors, _step, _student
from tests.util import cosine, prepare, rel_l2

pytestmark = pytest.mark.gpu
VALUES = (0.5, 1.25, 2.0)


def mixed_table(rows, B, shift=0):
    """fp32 [rows, B]: row r holds one 0 (at sample (r + shift) % B) and otherwise non-zero multipliers that differ along the row and from row to row."""
    t = torch.empty(rows, B)
    for r in range(rows):
        for b in range(B):
            t[r, b] = 0.0 if b == (r + shift) % B else VALUES[(r + b + shift) % 3]
    assert all((row == 0).any() and (row != 0).any() for row in t)
    return t


# ---------------------------------------------------------------------------------------------------------------- the float step
# case: (model keywords on top of vit_small_patch16_224_student, tokens, batch)
FLOAT_CASES = {
    "T5": (dict(img_size=32, depth=2, num_heads=12), 5, 3),                      # M = 15: several workgroups, T not a power of two
    "T65": (dict(img_size=128, depth=2, mlp_ratio=2), 65, 2),                    # M = 130
    "B768": (dict(embed_dim=768, num_heads=12, depth=1, img_size=32), 5, 3),     # ViT-B width: three column groups per row
}


def _float_inputs(case, seed):
    kw, _, B = FLOAT_CASES[case]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, kw["img_size"], kw["img_size"], generator=g).cuda(), torch.randn(B, 10, generator=g).cuda()


@functools.lru_cache(maxsize=None)
def _float_reference(case):
    """The case's weights (CPU), its table, and the fp64 tree's steps under that table: {seed: (logits, gradients)}.  Once per case, shared by the forms."""
    kw, T, B = FLOAT_CASES[case]
    base = _student(1, 10, drop_path_rate=0.2, **kw)
    assert base.model.patch_embed.num_patches + 1 == T
    table = mixed_table(2 * kw["depth"], B).cuda()
    ref = copy.deepcopy(base).double().cuda().train()
    steps = {}
    with forced_drop_path(ref, table):
        for seed in SEEDS:
            x, r = _float_inputs(case, seed)
            steps[seed] = _step(ref, x, r, double=True)[:2]
    return base, table, steps


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", list(FLOAT_CASES))
def test_float_step_parity_with_fp64_tree_under_the_same_table(case, form):
    """The bounds of tests/test_gpu_float_shapes.py, unchanged: fp32 form 1e-4 relative L2 on the logits, each image's logits and every parameter gradient; 16-bit
    forms within twice the stock-autocast tree's own error against fp64 under the same table (largest of its four input seeds), floored at 1e-4 and at four unit
    roundoffs for tensors under 256 elements, capped at 1e-2 (fp16) / 5e-2 (bf16).  The step runs only this library's kernels."""
    from torch.profiler import ProfilerActivity, profile

    kw, T, B = FLOAT_CASES[case]
    amp, dt, cap, unit = FORMS[form]
    base, table, ref_steps = _float_reference(case)
    m = qat_vit_amd.native_float(copy.deepcopy(base).cuda().train(), amp=amp)
    stock = copy.deepcopy(base).cuda().train() if dt is not None else None
    names = [n for n, _ in m.named_parameters()]
    seeds = SEEDS if dt is not None else SEEDS[:1]
    nat, sto = {}, {}
    for seed in seeds:
        x, r = _float_inputs(case, seed)
        with forced_drop_path(m, table):
            if seed == seeds[-1]:
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    out, grads, _ = _step(m, x, r, dt)
                    torch.cuda.synchronize()
            else:
                out, grads, _ = _step(m, x, r, dt)
        assert out.dtype == (dt or torch.float32) and torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads)
        nat[seed] = _errors(out, grads, *ref_steps[seed], names)
        if stock is not None:
            with forced_drop_path(stock, table):
                out_s, grads_s, _ = _step(stock, x, r, dt)
            sto[seed] = _errors(out_s, grads_s, *ref_steps[seed], names)
    _assert_ran_natively(prof, m, form, B, len(seeds))
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("k_resid_ln_split_dp" in k for k in kernels) and any("k_ln_bwd_fq_dp" in k for k in kernels), kernels
    bad, worst = [], {t: max(run[t][0] for run in nat.values()) for t in nat[seeds[0]]}
    for t, a in worst.items():
        floor = max(s[t][0] for s in sto.values()) if sto else 0.0
        bound = 1e-4 if dt is None else min(max(2 * floor, 1e-4, 4 * unit if nat[seeds[0]][t][1] < 256 else 0.0), cap)
        if not a <= bound:
            bad.append((t, a, floor, bound))
    wt = max(worst, key=worst.get)
    print(f"DROPPATH float {case} {form}: logits {worst['logits']:.2e} worst tensor {wt} {worst[wt]:.2e}"
          + (f" (stock {max(s[wt][0] for s in sto.values()):.2e})" if sto else ""))
    assert not bad, bad
    # a table that differs only in sample 1's multipliers leaves the other images' logits as they were: the multipliers reach their own sample
    t2 = table.clone()
    t2[:, 1] = 1.0 - t2[:, 1].clamp(max=1.0)
    x, r = _float_inputs(case, seeds[-1])
    with forced_drop_path(m, t2), torch.autocast("cuda", dtype=dt, enabled=dt is not None):
        out2 = m(x).detach()
    keep = [b for b in range(B) if b != 1]
    assert torch.equal(out2[keep], out[keep]) and not torch.equal(out2[1], out[1])


# ---------------------------------------------------------------------------------------------------------------- the QAT step
TINY = dict(embed_dim=128, depth=2, num_heads=2, img_size=32)          # the tiny model of tests/test_gpu_step.py: the pair form throughout
W384 = dict(embed_dim=384, depth=2, img_size=32)                       # the width at which the fused dgrad + LayerNorm-backward epilogue would be chosen
S96 = dict(embed_dim=384, depth=2, img_size=96)                        # 37 tokens: the one-plane backward with the class-token last block from the second step on
QAT_MODELS = {"tiny": TINY, "w384": W384, "s96": S96}
B_QAT, STEPS = 3, 3


def _qat_pair(kw, backend, rate=0.2, seed=3):
    """(prepared student with drop-path, prepared twin without any DropPath module), same weights, on the GPU."""
    torch.manual_seed(seed)
    a = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, drop_path_rate=rate, **kw)
    with torch.no_grad():
        for n, p in a.named_parameters():
            if n.endswith("bias") or "norm" in n or "cls_token" in n:
                p.add_(0.05 * torch.randn_like(p))
    b = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **kw)
    b.load_state_dict(a.state_dict())
    return prepare(a.cuda(), backend), prepare(b.cuda(), backend)


def _qat_batches(kw, n=STEPS, B=B_QAT, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, 3, kw["img_size"], kw["img_size"], generator=g).cuda() * (1 + 0.25 * i), torch.randint(0, 10, (B,), generator=g).cuda())
            for i in range(n)]


def _qat_step(p, x, y):
    for q in p.parameters():
        q.grad = None
    out = p(x)
    loss, _ = F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)
    loss.backward()
    return out.detach(), loss.detach()


def _kernel_counts(prof):
    counts = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            counts[e.name] = counts.get(e.name, 0) + 1
    return counts


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
@pytest.mark.parametrize("model", list(QAT_MODELS))
def test_qat_all_ones_table_is_the_step_without_one_bit_for_bit(native_lib, model, backend):
    from torch.profiler import ProfilerActivity, profile

    kw = QAT_MODELS[model]
    a, b = _qat_pair(kw, backend)
    ones = torch.ones(2 * kw["depth"], B_QAT)
    for k, (x, y) in enumerate(_qat_batches(kw)):
        with forced_drop_path(a, ones):
            if k == STEPS - 1:
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    out_a, loss_a = _qat_step(a, x, y)
                    torch.cuda.synchronize()
            else:
                out_a, loss_a = _qat_step(a, x, y)
        out_b, loss_b = _qat_step(b, x, y)
        assert torch.equal(out_a, out_b) and torch.equal(loss_a, loss_b), k
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p.grad, q.grad), (k, n)
        for (n, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
            assert torch.equal(u, v), (k, n)
        assert engine_of(a)._fwd_x16 == engine_of(b)._fwd_x16 == (model == "s96" and k > 0)
    assert engine_of(a).dy16_fallbacks == 0 and engine_of(b).dy16_fallbacks == 0
    # the drop-path instantiations ran, and every LayerNorm backward ran as its own kernel (2 * depth + 1 of them: none inside a dgrad epilogue)
    counts = _kernel_counts(prof)
    n_of = lambda s: sum(c for k, c in counts.items() if s in k)   # noqa: E731
    depth = kw["depth"]
    assert n_of("k_resid_fq_lnstats_dp") == 2 * depth, counts
    assert n_of("k_ln_bwd_fq_dp") == 2 * depth and n_of("k_ln_bwd_fq") == 2 * depth + 1, counts


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
@pytest.mark.parametrize("model", list(QAT_MODELS))
def test_qat_dead_branch_has_exactly_zero_gradients(native_lib, model, backend):
    """Row 2 i all zero: block i's norm1, attn.qkv and attn.proj get exactly zero gradients; row 2 i + 1: its norm2, mlp.fc1, mlp.fc2.  Every other gradient is
    finite and non-zero.  First and last block (the last one: the class-token form where the one-plane backward runs), at every one of three steps."""
    kw = QAT_MODELS[model]
    depth = kw["depth"]
    dead_names = {0: ("norm1.", "attn.qkv.", "attn.proj."), 1: ("norm2.", "mlp.fc1.", "mlp.fc2.")}
    for blk in (0, depth - 1):
        for mlp in (0, 1):
            a, _ = _qat_pair(kw, backend)
            table = mixed_table(2 * depth, B_QAT, shift=blk + mlp).clamp(min=0.5)   # no zero anywhere else
            table[2 * blk + mlp] = 0.0
            for k, (x, y) in enumerate(_qat_batches(kw)):
                with forced_drop_path(a, table):
                    _qat_step(a, x, y)
                for n, p in a.named_parameters():
                    dead = n.startswith(f"model.blocks.{blk}.") and any(s in n for s in dead_names[mlp])
                    if dead:
                        assert torch.count_nonzero(p.grad).item() == 0, (blk, mlp, k, n)
                    else:
                        assert torch.isfinite(p.grad).all() and torch.count_nonzero(p.grad).item() > 0, (blk, mlp, k, n)
            assert engine_of(a)._fwd_x16 == (model == "s96")


REF_ARCH = {"tiny": "vit_tiny_test", "w384": "vit_small_depth2_test"}


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
@pytest.mark.parametrize("model", list(REF_ARCH))
def test_qat_parity_with_the_prepared_stock_tree_on_the_cpu(native_lib, model, backend):
    """Stock torch.ao on the CPU (the oracle's tree with this package's DropPath set into its blocks) under the same mixed table, one step.  Bound: the one
    tests/test_gpu_step.py holds its tiny cases to at network level (_tiny_case) - logits 0.15 relative L2, loss 3 %, gradient cosine 0.99.  Fake-quant code flips
    between CPU and GPU arithmetic are a property of the inputs, so the same weights and images first have to meet the bound WITHOUT drop-path (an all-ones table
    on both sides, which the exactness test shows to be the step without one); the native multiply is rounded like the stock one, so drop-path adds no flips."""
    kw = QAT_MODELS[model]
    depth = kw["depth"]
    w = step_ref.RefQATWrapper(randomize_(RefVisionTransformer(REF_ARCH[model], num_classes=10, img_size=32), 11))
    for b in w.model.blocks:
        b.drop_path1, b.drop_path2 = DropPath(0.2), DropPath(0.2)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, drop_path_rate=0.2, **kw)
    stu.load_state_dict(w.state_dict())
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(B_QAT, 3, 32, 32, generator=g) * (1 + 0.25 * k), torch.randint(0, 10, (B_QAT,), generator=g)) for k in range(STEPS)]
    names = [n for n, _ in stu.named_parameters()]
    for what, table in (("no drop-path", torch.ones(2 * depth, B_QAT)), ("drop-path", mixed_table(2 * depth, B_QAT))):
        po = step_ref.enable_qat(copy.deepcopy(w), backend)
        for i, b in enumerate(po.model.blocks):
            assert type(b.drop_path1) is DropPath and type(b.drop_path2) is DropPath
            b.drop_path1._forced, b.drop_path2._forced = table[2 * i], table[2 * i + 1]
        p = prepare(copy.deepcopy(stu).cuda(), backend)
        for k, (x, y) in enumerate(batches):      # three consecutive steps: the observers of both sides move with them
            ro, rl, _, _ = step_ref.student_step(po, x, y, None)
            with forced_drop_path(p, table):
                out, loss = _qat_step(p, x.cuda(), y.cuda())
            ga = torch.cat([dict(p.named_parameters())[n].grad.cpu().double().flatten() for n in names]).numpy()
            gb = torch.cat([dict(po.named_parameters())[n].grad.double().flatten() for n in names]).numpy()
            e_out, e_loss, cos = rel_l2(out.cpu().numpy(), ro.detach().numpy()), abs(loss.item() - rl.item()) / abs(rl.item()), cosine(ga, gb)
            print(f"DROPPATH qat parity {model} {backend} {what} step {k}: logits {e_out:.2e} loss {e_loss:.2e} gradients {rel_l2(ga, gb):.2e} cosine {cos:.6f}")
            assert e_out < 0.15 and e_loss < 0.03 and cos > 0.99, (what, k, e_out, e_loss, cos)


def _grads(p):
    return [q.grad.detach().clone() for q in p.parameters()]


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_qat_one_plane_and_class_token_backward_against_the_pair_form_under_a_mixed_table(native_lib, backend):
    """37 tokens, batch 3, three steps under a table whose multipliers differ from sample to sample: from the second step on one engine runs the one-plane
    backward with the last block on the compact class-token rows [B, D] (rows per sample 1), its twin (``dy16 = False``) the bf16-pair form at full height
    throughout (rows per sample T) - a reference that does not pass through the compact rows' sample map or the one-plane store.  Bound on every parameter
    gradient: 1e-3 relative L2, the bar tests/test_gpu_graph.py and tests/test_gpu_dy16.py hold one-plane steps to against pair-form twins; logits bit for bit
    (the forward does not depend on the gradient form).  A multiplier read for the wrong sample is off by a factor of 0 / 2.5 / 4 in that sample's rows."""
    from qat_vit_amd import engine as E

    kw = S96
    a, _ = _qat_pair(kw, backend)
    c = copy.deepcopy(a)
    E.bind(c, B_QAT).dy16 = False
    table = mixed_table(2 * kw["depth"], B_QAT)
    for k, (x, y) in enumerate(_qat_batches(kw)):
        with forced_drop_path(a, table):
            out_a, _ = _qat_step(a, x, y)
        with forced_drop_path(c, table):
            out_c, _ = _qat_step(c, x, y)
        assert engine_of(a)._fwd_x16 == (k > 0) and not engine_of(c)._fwd_x16
        assert torch.equal(out_a, out_c), k
        worst = max((rel_l2(p.grad.cpu(), q.grad.cpu()), n) for (n, p), q in zip(a.named_parameters(), c.parameters()))
        print(f"DROPPATH qat one-plane vs pair {backend} step {k}: worst gradient {worst[1]} {worst[0]:.2e}")
        assert worst[0] < 1e-3, (k, worst)
    assert engine_of(a).dy16_fallbacks == 0


@pytest.mark.parametrize("model,one_plane", [("tiny", False), ("w384", False), ("s96", False), ("s96", True)])
def test_injected_backward_stages_take_the_multipliers(native_lib, model, one_plane):
    """qatvit_student_backward_stages with QATVIT_STAGE_INJECT under a mixed table: a block stage whose input gradient is "injected" rebuilds the masked gradient
    entering fc2 with k_mask_bwd_dp (times the MLP branch's multipliers) instead of taking the one the previous stage's LayerNorm backward left.  Injecting what
    the previous stage itself left in dxA must therefore give the gradients of the whole backward in one call.  Pair form: every block stage injected, 1e-6
    (the same arithmetic in another kernel).  One-plane form (third step of the 37-token model): head and last block in one call, block 0 injected - the O16
    form of the kernel; the calls rescale their planes from their own history, so 1e-3 (the one-plane bar)."""
    from qat_vit_amd import engine as E

    kw = QAT_MODELS[model]
    depth = kw["depth"]
    a, _ = _qat_pair(kw, "qnnpack")
    table = mixed_table(2 * depth, B_QAT)
    batches = _qat_batches(kw)
    with forced_drop_path(a, table):
        for x, y in batches[:2] if one_plane else ():
            _qat_step(a, x, y)
        x, y = batches[2]
        out = a(x)
        loss, _ = F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)
        (dlogits,) = torch.autograd.grad(loss, out)
    eng = engine_of(a)
    assert eng._fwd_x16 == one_plane
    mode = E.BWD_DY16 if one_plane else 0
    whole = [v.clone() for v in eng.backward_stages(dlogits, 0, depth + 1, mode=mode)]
    if one_plane:
        calls = [(dlogits, 0, 1, False)] + [(None, s, s, True) for s in range(2, depth + 2)]
    else:
        calls = [(dlogits, 0, 0, False)] + [(None, s, s, True) for s in range(1, depth + 2)]
    parts = [torch.zeros_like(v) for v in whole]
    for dl, s0, s1, inject in calls:
        for acc, v in zip(parts, eng.backward_stages(dl, s0, s1, inject=inject, mode=mode)):
            acc += v
    assert not one_plane or not eng.dy16_overflowed()
    names = [n for n, _ in a.named_parameters()]
    by_ptr = {p.data_ptr(): n for n, p in a.named_parameters()}
    worst = max((rel_l2(g.cpu(), w.cpu()), by_ptr[p.data_ptr()]) for g, w, p in zip(parts, whole, eng.params))
    print(f"DROPPATH injected stages {model} {'one-plane' if one_plane else 'pair'}: worst gradient {worst[1]} {worst[0]:.2e}")
    assert len(names) == len(whole) and all(torch.isfinite(w).all() and torch.count_nonzero(w) > 0 for w in whole)
    assert worst[0] < (1e-3 if one_plane else 1e-6), worst


@pytest.mark.parametrize("form", ["fp16", "bf16"])
def test_float_16_bit_forms_hold_one_rounded_mask_in_both_directions(form):
    """Stock autocast multiplies by the SAME 16-bit mask forward and backward.  1 / 0.9 and 1 / 0.7 (what a draw holds) are not representable: the step under
    such a table equals, bit for bit in the logits and in every gradient, the step under the table rounded to the type - a backward that multiplied by the fp32
    value would differ in every gradient of a branch by up to one unit roundoff."""
    amp, dt, _, _ = FORMS[form]
    kw, _, B = FLOAT_CASES["T5"]
    base = _student(1, 10, drop_path_rate=0.2, **kw)
    m = qat_vit_amd.native_float(copy.deepcopy(base).cuda().train(), amp=amp)
    table = mixed_table(2 * kw["depth"], B)
    table[table == 1.25] = 1 / 0.9
    table[table == 2.0] = 1 / 0.7
    rounded = table.to(dt).float()
    assert not torch.equal(rounded, table)
    x, r = _float_inputs("T5", SEEDS[0])
    with forced_drop_path(m, table):
        out1, g1, _ = _step(m, x, r, dt)
    with forced_drop_path(m, rounded):
        out2, g2, _ = _step(m, x, r, dt)
    assert torch.equal(out1, out2)
    for n, u, v in zip([n for n, _ in m.named_parameters()], g1, g2):
        assert torch.equal(u, v), n
    # ... and it is stock autocast's step under the un-rounded table (which rounds the mask itself), to the bound of the parity test above
    stock = copy.deepcopy(base).cuda().train()
    with forced_drop_path(stock, table):
        out_s, g_s, _ = _step(stock, x, r, dt)
    e = max(rel_l2(u.float().cpu(), v.float().cpu()) for u, v in zip(g1, g_s))
    print(f"DROPPATH float {form} non-representable multipliers: worst gradient against stock autocast {e:.2e}")


def test_graphed_step_replays_with_the_table_of_each_call(native_lib):
    """GraphedStudentStep on the tiny model: two replays under two forced tables equal the eager steps under those tables to the bound of
    tests/test_gpu_graph.py (logits and loss bit for bit, gradients 1e-6); two replays without forcing draw two different tables (the engine's buffer)."""
    kw = TINY
    a, _ = _qat_pair(kw, "qnnpack", rate=0.5)
    b = copy.deepcopy(a)
    B = 4
    (w0, y0), *batches = _qat_batches(kw, n=5, B=B)
    tables = [mixed_table(2 * kw["depth"], B, shift=s) for s in range(3)]
    with forced_drop_path(b, tables[0]):
        step = GraphedStudentStep(b, w0, y0, warmup=1)
    with forced_drop_path(a, tables[0]):
        _qat_step(a, w0, y0)
    for (x, y), table in zip(batches[:2], tables[1:]):
        with forced_drop_path(a, table):
            out_a, loss_a = _qat_step(a, x, y)
        with forced_drop_path(b, table):
            out_b, loss_b, _ = step(x, y)
        assert torch.equal(step.engine.drop.view(B).cpu(), table)
        assert torch.equal(out_a, out_b) and torch.equal(loss_a, loss_b)
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert rel_l2(q.grad.cpu(), p.grad.cpu()) < 1e-6, n
    torch.manual_seed(1234)
    drawn = []
    for x, y in batches[2:4]:
        step(x, y)
        drawn.append(step.engine.drop.view(B).clone())
    assert not torch.equal(drawn[0], drawn[1])
    for t in drawn:
        assert torch.equal(t[:2], torch.ones(2, B, device=t.device)) and bool(((t[2:] == 0) | (t[2:] == 2.0)).all())
    step.close()


def test_graph_fallback_after_an_evaluation_forward_still_reads_the_table(native_lib):
    """The captured kernels carry the table's address, the eager repeat of an overflowed one-plane backward reads the workspace's binding - which an
    eval-mode forward between two replays removes (validation after an epoch).  As test_one_plane_replay_falls_back_on_the_captured_step, at 37 tokens and
    under mixed tables: after an eval forward a replay whose planes overflow is repeated in the pair form WITH the step's multipliers and equals the
    pair-form twin's step under the same table (2e-6, that test's bar)."""
    import ctypes
    import warnings

    from qat_vit_amd import engine as E

    kw = S96
    a, _ = _qat_pair(kw, "qnnpack")
    c = copy.deepcopy(a)
    E.bind(c, B_QAT).dy16 = False
    (x0, y0), (x1, y1), (x2, y2) = _qat_batches(kw)
    tables = [mixed_table(2 * kw["depth"], B_QAT, shift=s) for s in range(3)]
    with forced_drop_path(a, tables[0]):
        step = GraphedStudentStep(a, x0, y0, warmup=2)      # a calibrating step, a one-plane step; the capture executes nothing
    assert step.step.x16 and step._drop_path
    with forced_drop_path(c, tables[0]):
        _qat_step(c, x0, y0); _qat_step(c, x0, y0)
    with forced_drop_path(a, tables[1]):
        step(x1, y1)
    with forced_drop_path(c, tables[1]):
        _qat_step(c, x1, y1)
    worst = lambda: max((rel_l2(p.grad.cpu(), q.grad.cpu()), n) for (n, p), q in zip(a.named_parameters(), c.parameters()))   # noqa: E731
    assert step.engine.dy16_fallbacks == 0 and worst()[0] < 1e-3, worst()
    for m in (a, c):                                           # validation: eval mode, no table - the workspace is unbound
        m.eval()
        with torch.no_grad():
            m(x1[:2])
        m.train()
    assert not step.engine.drop.bound
    cf = step.step.cfg                                         # wreck the scale history: the planes of the next replay overflow
    off = step.engine.lib.qatvit_student_tensor_offset(ctypes.byref(cf), b"dy16", 0)
    st = step.engine.workspace[off:off + 4 * (64 + 256 * 4 * cf.depth)].view(torch.float32)
    for t in range(4 * cf.depth):
        st[64 + 256 * t + 3] = 2.0 ** -60
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        with forced_drop_path(a, tables[2]):
            step(x2, y2)
    with forced_drop_path(c, tables[2]):
        _qat_step(c, x2, y2)
    assert step.engine.dy16_fallbacks == 1
    for (n, p), q in zip(a.named_parameters(), c.parameters()):
        assert torch.isfinite(p.grad).all() and rel_l2(p.grad.cpu(), q.grad.cpu()) < 2e-6, n
    step.close()


@pytest.mark.parametrize("float_step", [False, True])
def test_unforced_draw_and_eval(native_lib, float_step):
    """drop_path_rate 0.5, depth 2, train mode: the engine's table holds 0 and 1 / keep_i only, row by row, and block 0 (rate 0) all ones; in eval mode the
    forward equals the forward of the tree without drop-path bit for bit and no table is bound."""
    B = 64
    if float_step:
        a = qat_vit_amd.native_float(_student(1, 10, drop_path_rate=0.5, img_size=32, depth=2).cuda().train())
        b = _student(1, 10, img_size=32, depth=2)
        b.load_state_dict(a.state_dict())
        b = qat_vit_amd.native_float(b.cuda().train())
        from qat_vit_amd.float_engine import engine_of as eng_of
    else:
        a, b = _qat_pair(TINY, "qnnpack", rate=0.5)
        eng_of = engine_of
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(9)).cuda()
    a.eval(); b.eval()                                                                   # (first: a training step moves the QAT observers of the two apart)
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    assert not eng_of(a).drop.bound
    a.train(); b.train()
    torch.manual_seed(77)
    out_a = a(x)
    out_a.float().sum().backward()
    t = eng_of(a).drop.view(B)
    assert torch.equal(t[:2], torch.ones(2, B, device=t.device))                       # block 0: rate 0
    assert bool(((t[2:] == 0) | (t[2:] == 2.0)).all())                                   # block 1: keep 0.5
    assert 0 < int((t[2:] == 0).sum()) < 2 * B
    assert not torch.equal(out_a.detach(), b(x).detach())
    assert len(eng_of(a).drop.bound) == 1 and not eng_of(b).drop.bound
    a.eval()
    with torch.no_grad():
        a(x)
    assert not eng_of(a).drop.bound                                                      # an eval forward after a training step unbinds the table
