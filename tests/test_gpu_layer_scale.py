"""LayerScale (``init_values``) in the native float step (all three forms) and the native QAT step, on an MI355X.

Test gammas: per branch from a seeded generator, magnitudes in [0.5, 2], both signs, two columns per branch exactly 0 (one of them column D - 1); one extra float
case with every gamma at 1e-5, the real initial value.  A zero column shows a gamma gradient formed by dividing by gamma or by differencing the residual stream;
the mixed signs and magnitudes a wrong column index.  Shapes: those of tests/test_gpu_drop_path.py.  Measured values: profiles/layer_scale_bench.txt."""
import copy
import functools

import pytest
import torch

import qat_vit_amd
from oracle import step_ref
from oracle.vit_ref import RefVisionTransformer, randomize_
from qat_vit_amd import DropPath, LayerScale, forced_drop_path
from qat_vit_amd import functional as F
from qat_vit_amd.engine import engine_of
from qat_vit_amd.graph import GraphedStudentStep
from tests.test_gpu_drop_path import (B_QAT, FLOAT_CASES, QAT_MODELS, REF_ARCH, S96, STEPS, TINY, _float_inputs, _kernel_counts, _qat_batches, _qat_step,
                                      mixed_table)
from tests.test_gpu_float_shapes import FORMS, SEEDS, _assert_ran_natively, _errors, _step, _student
from tests.util import cosine, prepare, rel_l2

pytestmark = pytest.mark.gpu


def zero_columns(D, k):
    """The two columns of branch k whose gamma is exactly 0: D - 1 and one that moves with the branch."""
    return [(37 * k + 5) % (D - 1), D - 1]


def set_gammas(vit, kind="mixed", seed=21):
    """kind "mixed": see the module docstring; "init": 1e-5 everywhere; "ones"."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, ls in enumerate(m for b in vit.blocks for m in (b.ls1, b.ls2)):
            assert type(ls) is LayerScale
            D = ls.gamma.numel()
            if kind == "mixed":
                v = (0.5 + 1.5 * torch.rand(D, generator=g)) * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
                v[zero_columns(D, k)] = 0.0
            else:
                v = torch.full((D,), 1e-5 if kind == "init" else 1.0)
            ls.gamma.copy_(v.to(ls.gamma.device, ls.gamma.dtype))
    return vit


# ---------------------------------------------------------------------------------------------------------------- the float step
@functools.lru_cache(maxsize=None)
def _float_reference(case, kind, drop):
    """The case's weights with LayerScale (CPU), its table (None without drop-path), and the fp64 tree's steps: {seed: (logits, gradients)}.  Once per case."""
    kw, T, B = FLOAT_CASES[case]
    base = _student(1, 10, init_values=1.0, **(dict(drop_path_rate=0.2) if drop else {}), **kw)
    set_gammas(base.model, kind)
    assert base.model.patch_embed.num_patches + 1 == T
    table = mixed_table(2 * kw["depth"], B).cuda() if drop else None
    ref = copy.deepcopy(base).double().cuda().train()
    steps = {}
    for seed in SEEDS:
        x, r = _float_inputs(case, seed)
        if drop:
            with forced_drop_path(ref, table):
                steps[seed] = _step(ref, x, r, double=True)[:2]
        else:
            steps[seed] = _step(ref, x, r, double=True)[:2]
    return base, table, steps


def _maybe_forced(m, table):
    import contextlib

    return forced_drop_path(m, table) if table is not None else contextlib.nullcontext()


FLOAT_PARAMS = [(c, "mixed") for c in FLOAT_CASES] + [("T5", "init")]


@pytest.mark.parametrize("drop", [True, False], ids=["droppath", "plain"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case,kind", FLOAT_PARAMS)
def test_float_step_parity_with_fp64_tree(case, kind, form, drop):
    """The bounds of tests/test_gpu_float_shapes.py, unchanged: fp32 form 1e-4 relative L2 on the logits, each image's logits and every parameter gradient - the
    gammas among them; 16-bit forms within twice the stock-autocast tree's own error against fp64 (largest of its four input seeds), floored at 1e-4 and at four
    unit roundoffs for tensors under 256 elements, capped at 1e-2 (fp16) / 5e-2 (bf16).  Under a mixed drop-path table and without drop-path.

    Every gamma at 1e-5, fp16 form: stock autocast holds each gradient inside a branch in fp16, where dx * s * 1e-5 lies in or under the subnormal range (no loss
    scale in this test's loss) - its own error on patch_embed.proj.weight is 4.6e-2 / 7.3e-2, beyond the 1e-2 cap.  The native form carries the gradients inside a
    branch at a power-of-two scale of the order of 1 / max |gamma| (csrc/float_step.hip) and stays at the level of the mixed-gamma cases (8e-4)."""
    from torch.profiler import ProfilerActivity, profile

    kw, T, B = FLOAT_CASES[case]
    amp, dt, cap, unit = FORMS[form]
    base, table, ref_steps = _float_reference(case, kind, drop)
    m = qat_vit_amd.native_float(copy.deepcopy(base).cuda().train(), amp=amp)
    stock = copy.deepcopy(base).cuda().train() if dt is not None else None
    names = [n for n, _ in m.named_parameters()]
    seeds = SEEDS if dt is not None else SEEDS[:1]
    nat, sto, zero_nat = {}, {}, {}
    D = base.model.embed_dim
    zero_of = {f"model.blocks.{i}.{ls}.gamma": zero_columns(D, 2 * i + mlp) for i in range(kw["depth"]) for mlp, ls in enumerate(("ls1", "ls2"))}

    def zero_errors(grads, ref_grads):
        """Per gamma gradient, the error over its two gamma == 0 columns alone: (relative to those two reference elements, relative to the whole reference)."""
        g, rg = dict(zip(names, grads)), dict(zip(names, ref_grads))
        return {n: (((g[n][c].double() - rg[n][c].double()).norm() / rg[n][c].double().norm()).item(),
                    ((g[n][c].double() - rg[n][c].double()).norm() / rg[n].double().norm()).item()) for n, c in zero_of.items()}

    for seed in seeds:
        x, r = _float_inputs(case, seed)
        with _maybe_forced(m, table):
            if seed == seeds[-1]:
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    out, grads, _ = _step(m, x, r, dt)
                    torch.cuda.synchronize()
            else:
                out, grads, _ = _step(m, x, r, dt)
        assert out.dtype == (dt or torch.float32) and torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads)
        nat[seed] = _errors(out, grads, *ref_steps[seed], names)
        zero_nat[seed] = zero_errors(grads, ref_steps[seed][1])
        if stock is not None:
            with _maybe_forced(stock, table):
                out_s, grads_s, _ = _step(stock, x, r, dt)
            sto[seed] = _errors(out_s, grads_s, *ref_steps[seed], names)
    _assert_ran_natively(prof, m, form, B, len(seeds))
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("k_resid_ln_split_ls" in k for k in kernels) and any("k_ln_bwd_fq_ls" in k for k in kernels), kernels
    assert not any("k_resid_ln_split_dp" in k or "k_ln_bwd_fq_dp" in k for k in kernels), kernels
    bad, worst = [], {t: max(run[t][0] for run in nat.values()) for t in nat[seeds[0]]}

    def bound_of(t, numel):
        floor = max(s[t][0] for s in sto.values()) if sto else 0.0
        return (1e-4 if dt is None else min(max(2 * floor, 1e-4, 4 * unit if numel < 256 else 0.0), cap)), floor

    for t, a in worst.items():
        bound, floor = bound_of(t, nat[seeds[0]][t][1])
        if not a <= bound:
            bad.append((t, a, floor, bound))
    wt = max(worst, key=worst.get)
    wg = max((t for t in worst if t.endswith(".gamma")), key=worst.get)
    print(f"LAYERSCALE float {case} {kind} {form} {'drop-path' if drop else 'plain'}: logits {worst['logits']:.2e} worst tensor {wt} {worst[wt]:.2e} worst gamma {wg} "
          f"{worst[wg]:.2e}" + (f" (stock {max(s[wg][0] for s in sto.values()):.2e})" if sto else ""))
    assert not bad, bad
    if kind != "mixed":
        return
    # gamma == 0 columns (last seed's gradients): nothing reaches the branch's last layer through them, yet gamma's own gradient is there, and right.  A tensor
    # within relative L2 b of its reference has every element within b * |reference|: the two elements are held to exactly that with the tensor's own bound
    # (a column whose gradient were missing is off by about |reference| / sqrt(D) >= 3.6e-2 |reference|, above every cap).  The fp32 form, whose 1e-4 does not
    # depend on a stock measurement, also holds the two elements to 1e-4 of themselves.  (Two fp16 / bf16 elements relative to themselves - a sum of 10 to 130
    # signed products - are off by up to 9e-2 in stock autocast itself: no bound of the tensor rule applies to them.)
    g = dict(zip(names, grads))
    for i in range(kw["depth"]):
        for mlp, (ls, layer) in enumerate((("ls1", "attn.proj"), ("ls2", "mlp.fc2"))):
            cols = zero_columns(D, 2 * i + mlp)
            pre = f"model.blocks.{i}."
            assert torch.count_nonzero(g[pre + layer + ".weight"][cols]).item() == 0 and torch.count_nonzero(g[pre + layer + ".bias"][cols]).item() == 0, (i, ls)
            assert torch.count_nonzero(g[pre + ls + ".gamma"][cols]).item() == len(cols), (i, ls)
            own = max(z[pre + ls + ".gamma"][0] for z in zero_nat.values())
            err = max(z[pre + ls + ".gamma"][1] for z in zero_nat.values())
            assert err <= bound_of(pre + ls + ".gamma", D)[0] and (dt is not None or own <= 1e-4), (i, ls, err, own)


@pytest.mark.parametrize("form", ["fp16", "bf16"])
def test_float_16_bit_forms_do_not_round_the_multipliers_under_layer_scale(form):
    """16-bit branch times fp32 gamma is an fp32 tensor, so stock DropPath multiplies it by an fp32 mask: with 1 / 0.9 in the table (not representable in the
    type) the native logits equal stock autocast's within the parity bound, and the same table pre-rounded to the type gives other logits."""
    amp, dt, cap, unit = FORMS[form]
    kw, _, B = FLOAT_CASES["T5"]
    base, _, ref_steps = _float_reference("T5", "mixed", True)
    m = qat_vit_amd.native_float(copy.deepcopy(base).cuda().train(), amp=amp)
    stock = copy.deepcopy(base).cuda().train()
    ref = copy.deepcopy(base).double().cuda().train()
    table = mixed_table(2 * kw["depth"], B)
    table[table == 1.25] = 1 / 0.9
    table[table == 2.0] = 1 / 0.7
    table = table.cuda()
    rounded = table.to(dt).float()
    assert not torch.equal(rounded, table)
    x, r = _float_inputs("T5", SEEDS[0])
    with forced_drop_path(ref, table):
        out_r = _step(ref, x, r, double=True)[0]
    with forced_drop_path(m, table):
        out1 = _step(m, x, r, dt)[0]
    with forced_drop_path(m, rounded):
        out2 = _step(m, x, r, dt)[0]
    with forced_drop_path(stock, table):
        out_s = _step(stock, x, r, dt)[0]
    e_nat, e_sto = rel_l2(out1.float().cpu(), out_r.cpu()), rel_l2(out_s.float().cpu(), out_r.cpu())
    bound = min(max(2 * e_sto, 1e-4, 4 * unit), cap)
    print(f"LAYERSCALE float {form} 1/0.9 table: logits against fp64 native {e_nat:.2e} stock autocast {e_sto:.2e} bound {bound:.2e}")
    assert e_nat <= bound
    assert not torch.equal(out1, out2)


# ---------------------------------------------------------------------------------------------------------------- the QAT step
def _ls_pair(kw, backend, kind="ones", rate=0.0, seed=3, twin=True):
    """(prepared student with LayerScale [and drop-path], prepared twin without LayerScale), same weights, on the GPU."""
    torch.manual_seed(seed)
    extra = dict(drop_path_rate=rate) if rate else {}
    a = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, init_values=1.0, **extra, **kw)
    with torch.no_grad():
        for n, p in a.named_parameters():
            if n.endswith("bias") or "norm" in n or "cls_token" in n:
                p.add_(0.05 * torch.randn_like(p))
    set_gammas(a.model, kind)
    b = None
    if twin:
        b = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **extra, **kw)
        assert b.load_state_dict(a.state_dict(), strict=False).unexpected_keys == [k for k in a.state_dict() if k.endswith(".gamma")]
        b = prepare(b.cuda(), backend)
    return prepare(a.cuda(), backend), b


@pytest.mark.parametrize("drop", [True, False], ids=["ones-table", "no-table"])
@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
@pytest.mark.parametrize("model", list(QAT_MODELS))
def test_qat_all_ones_gamma_is_the_step_without_layer_scale_bit_for_bit(native_lib, model, backend, drop):
    from torch.profiler import ProfilerActivity, profile

    kw = QAT_MODELS[model]
    a, b = _ls_pair(kw, backend, rate=0.2 if drop else 0.0)
    ones = torch.ones(2 * kw["depth"], B_QAT) if drop else None
    gq = dict(b.named_parameters())
    for k, (x, y) in enumerate(_qat_batches(kw)):
        with _maybe_forced(a, ones):
            if k == STEPS - 1:
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    out_a, loss_a = _qat_step(a, x, y)
                    torch.cuda.synchronize()
            else:
                out_a, loss_a = _qat_step(a, x, y)
        with _maybe_forced(b, ones):
            out_b, loss_b = _qat_step(b, x, y)
        assert torch.equal(out_a, out_b) and torch.equal(loss_a, loss_b), k
        for n, p in a.named_parameters():
            if n.endswith(".gamma"):
                assert torch.isfinite(p.grad).all() and torch.count_nonzero(p.grad) > 0, (k, n)
            else:
                assert torch.equal(p.grad, gq[n].grad), (k, n)
        for (n, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
            assert torch.equal(u, v), (k, n)
        assert engine_of(a)._fwd_x16 == engine_of(b)._fwd_x16 == (model == "s96" and k > 0)
    assert engine_of(a).dy16_fallbacks == 0 and engine_of(b).dy16_fallbacks == 0
    counts = _kernel_counts(prof)
    n_of = lambda s: sum(c for k, c in counts.items() if s in k)   # noqa: E731
    depth = kw["depth"]
    assert n_of("k_resid_fq_lnstats_ls") == 2 * depth and n_of("k_resid_fq_lnstats_dp") == 0, counts
    assert n_of("k_ln_bwd_fq_ls") == 2 * depth and n_of("k_ln_bwd_fq_dp") == 0 and n_of("k_ln_bwd_fq") == 2 * depth + 1, counts


@pytest.mark.parametrize("model", ["tiny", "w384"])
def test_qat_gamma_gradient_against_an_independent_evaluation(native_lib, model):
    """Pair form, stage by stage, under a mixed table: before block i's stage the workspace holds dxA = d loss / d x_in[i + 1] and the block's pre-FQ fc2 output
    Y2[i]; sum over rows of dxA * s[2 i + 1] * fake_quantize(Y2[i]) in fp64, with the module's scale / zero_point through torch.fake_quantize_per_tensor_affine,
    is ls2[i].gamma's gradient.  1e-5 relative L2: the same fp32 products summed in another order over at most 195 rows leave about 1e-6."""
    kw = QAT_MODELS[model]
    depth, D = kw["depth"], kw["embed_dim"]
    a, _ = _ls_pair(kw, "qnnpack", kind="mixed", rate=0.2, twin=False)
    table = mixed_table(2 * depth, B_QAT).cuda()
    x, y = _qat_batches(kw)[0]
    with forced_drop_path(a, table):
        out = a(x)
        loss, _ = F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)
        (dlogits,) = torch.autograd.grad(loss, out)
    eng = engine_of(a)
    assert not eng._fwd_x16
    T = a.model.patch_embed.num_patches + 1
    M = B_QAT * T
    idx = {p.data_ptr(): k for k, p in enumerate(eng.params)}
    acc = [v.clone() for v in eng.backward_stages(dlogits, 0, 0)]
    want = {}
    for s in range(1, depth + 1):
        i = depth - s
        dxA = eng.tensor("dxA", 0, (M, D)).double()
        Y2 = eng.tensor("Y2", i, (M, D)).clone()
        fq = a.model.blocks[i].mlp.fc2.activation_post_process
        B_ = torch.fake_quantize_per_tensor_affine(Y2, fq.scale, fq.zero_point, fq.activation_post_process.quant_min, fq.activation_post_process.quant_max)
        srow = table[2 * i + 1].double().repeat_interleave(T).view(M, 1)
        want[i] = (dxA * srow * B_.double()).sum(0)
        for u, v in zip(acc, eng.backward_stages(None, s, s)):
            u += v
    for i in range(depth):
        got = acc[idx[a.model.blocks[i].ls2.gamma.data_ptr()]].double()
        e = ((got - want[i]).norm() / want[i].norm()).item()
        print(f"LAYERSCALE qat dgamma {model} block {i} ls2: relative L2 against the fp64 evaluation {e:.2e}")
        assert e < 1e-5, (i, e)
        assert torch.count_nonzero(got[zero_columns(D, 2 * i + 1)]).item() == 2


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
@pytest.mark.parametrize("model", list(REF_ARCH))
def test_qat_parity_with_the_prepared_stock_tree_on_the_cpu(native_lib, model, backend):
    """As tests/test_gpu_drop_path.py's test of this name: the oracle's tree with this package's LayerScale and DropPath set into its blocks, three steps; logits
    0.15 relative L2, loss 3 %, gradient cosine 0.99 over all parameters, gammas included; the same inputs first meet the bound with all-ones gammas and table."""
    kw = QAT_MODELS[model]
    depth, D = kw["depth"], kw["embed_dim"]
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(B_QAT, 3, 32, 32, generator=g) * (1 + 0.25 * k), torch.randint(0, 10, (B_QAT,), generator=g)) for k in range(STEPS)]
    for what, kind, table in (("ones", "ones", torch.ones(2 * depth, B_QAT)), ("layer scale + drop-path", "mixed", mixed_table(2 * depth, B_QAT))):
        w = step_ref.RefQATWrapper(randomize_(RefVisionTransformer(REF_ARCH[model], num_classes=10, img_size=32), 11))
        for b in w.model.blocks:
            b.ls1, b.ls2 = LayerScale(D, 1.0), LayerScale(D, 1.0)
            b.drop_path1, b.drop_path2 = DropPath(0.2), DropPath(0.2)
        set_gammas(w.model, kind)
        stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, drop_path_rate=0.2, init_values=1.0, **kw)
        stu.load_state_dict(w.state_dict())
        names = [n for n, _ in stu.named_parameters()]
        po = step_ref.enable_qat(copy.deepcopy(w), backend)
        for i, b in enumerate(po.model.blocks):
            assert type(b.ls1) is LayerScale and type(b.drop_path1) is DropPath and not hasattr(b.ls1, "activation_post_process")
            b.drop_path1._forced, b.drop_path2._forced = table[2 * i], table[2 * i + 1]
        p = prepare(copy.deepcopy(stu).cuda(), backend)
        for k, (x, y) in enumerate(batches):
            ro, rl, _, _ = step_ref.student_step(po, x, y, None)
            with forced_drop_path(p, table):
                out, loss = _qat_step(p, x.cuda(), y.cuda())
            pa, pb = dict(p.named_parameters()), dict(po.named_parameters())
            cat = lambda d, ns: torch.cat([d[n].grad.cpu().double().flatten() for n in ns]).numpy()   # noqa: E731
            gn = [n for n in names if n.endswith(".gamma")]
            ga, gb = cat(pa, names), cat(pb, names)
            e_out, e_loss, cos = rel_l2(out.cpu().numpy(), ro.detach().numpy()), abs(loss.item() - rl.item()) / abs(rl.item()), cosine(ga, gb)
            print(f"LAYERSCALE qat parity {model} {backend} {what} step {k}: logits {e_out:.2e} loss {e_loss:.2e} gradients {rel_l2(ga, gb):.2e} cosine {cos:.6f} "
                  f"gamma cosine {cosine(cat(pa, gn), cat(pb, gn)):.6f}")
            assert e_out < 0.15 and e_loss < 0.03 and cos > 0.99, (what, k, e_out, e_loss, cos)


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_qat_one_plane_and_class_token_backward_against_the_pair_form(native_lib, backend):
    """37 tokens, mixed gammas and table: from the second step on the one-plane backward with the last block on the class-token rows, against a pair-form twin at
    full height.  Logits bit for bit, every gradient - gammas included - within 1e-3, no fallback."""
    from qat_vit_amd import engine as E

    kw = S96
    a, _ = _ls_pair(kw, backend, kind="mixed", rate=0.2, twin=False)
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
        wg = max((rel_l2(p.grad.cpu(), q.grad.cpu()), n) for (n, p), q in zip(a.named_parameters(), c.parameters()) if n.endswith(".gamma"))
        print(f"LAYERSCALE qat one-plane vs pair {backend} step {k}: worst gradient {worst[1]} {worst[0]:.2e} worst gamma {wg[1]} {wg[0]:.2e}")
        assert worst[0] < 1e-3, (k, worst)
    assert engine_of(a).dy16_fallbacks == 0


@pytest.mark.parametrize("model,one_plane", [("tiny", False), ("w384", False), ("s96", False), ("s96", True)])
def test_injected_backward_stages_reproduce_the_whole_backward(native_lib, model, one_plane):
    """As the drop-path test of injected stages: an injected block stage rebuilds the gradient entering fc2 with k_mask_bwd_ls.  Pair form 1e-6, one-plane 1e-3."""
    from torch.profiler import ProfilerActivity, profile

    from qat_vit_amd import engine as E

    kw = QAT_MODELS[model]
    depth = kw["depth"]
    a, _ = _ls_pair(kw, "qnnpack", kind="mixed", rate=0.2, twin=False)
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
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for dl, s0, s1, inject in calls:
            for acc, v in zip(parts, eng.backward_stages(dl, s0, s1, inject=inject, mode=mode)):
                acc += v
        torch.cuda.synchronize()
    assert any("k_mask_bwd_ls" in k for k in _kernel_counts(prof))
    assert not one_plane or not eng.dy16_overflowed()
    by_ptr = {p.data_ptr(): n for n, p in a.named_parameters()}
    worst = max((rel_l2(g.cpu(), w.cpu()), by_ptr[p.data_ptr()]) for g, w, p in zip(parts, whole, eng.params))
    print(f"LAYERSCALE injected stages {model} {'one-plane' if one_plane else 'pair'}: worst gradient {worst[1]} {worst[0]:.2e}")
    assert len(by_ptr) == len(whole) and all(torch.isfinite(w).all() and torch.count_nonzero(w) > 0 for w in whole)
    assert worst[0] < (1e-3 if one_plane else 1e-6), worst


# ---------------------------------------------------------------------------------------------------------------- host paths
def test_graphed_step_replay_equals_eager_with_gammas_changed_in_place(native_lib):
    kw = TINY
    a, _ = _ls_pair(kw, "qnnpack", kind="mixed", twin=False)
    b = copy.deepcopy(a)
    (w0, y0), *batches = _qat_batches(kw, n=4, B=4)
    step = GraphedStudentStep(b, w0, y0, warmup=1)
    _qat_step(a, w0, y0)
    for k, (x, y) in enumerate(batches):
        with torch.no_grad():   # an optimizer's in-place update: the addresses stay, the captured kernels read the new values
            for m in (a, b):
                for blk in m.model.blocks:
                    blk.ls1.gamma.mul_(1.0 + 0.1 * (k + 1))
                    blk.ls2.gamma.add_(0.01 * (k + 1))
        out_a, loss_a = _qat_step(a, x, y)
        out_b, loss_b, _ = step(x, y)
        assert torch.equal(out_a, out_b) and torch.equal(loss_a, loss_b), k
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert rel_l2(q.grad.cpu(), p.grad.cpu()) < 1e-6, (k, n)
    step.close()


def test_clip_adamw_ema_moves_the_gammas_and_the_eval_forward_uses_the_averages(native_lib):
    kw = TINY
    a, _ = _ls_pair(kw, "qnnpack", kind="mixed", twin=False)
    gam = [p for n, p in a.named_parameters() if n.endswith(".gamma")]
    before = [p.detach().clone() for p in gam]
    opt = qat_vit_amd.ClipAdamW(a.parameters(), lr=1e-2, ema_decay=0.9)
    batches = _qat_batches(kw, n=10)
    for x, y in batches:
        _qat_step(a, x, y)
        opt.step()
    assert all(not torch.equal(p, q) for p, q in zip(gam, before))
    x = batches[0][0]
    a.eval()
    live = [p.detach().clone() for p in gam]
    with torch.no_grad():
        with opt.ema_weights():
            avg = [p.detach().clone() for p in gam]
            twin = copy.deepcopy(a)
            out_ema = a(x)
        out_twin = twin(x)
        out_live = a(x)
    assert all(not torch.equal(u, v) for u, v in zip(avg, live)) and all(torch.equal(p, v) for p, v in zip(gam, live))
    assert torch.equal(out_ema, out_twin) and not torch.equal(out_ema, out_live)


def test_int8_student_refuses_and_import_round_trips(native_lib):
    a, _ = _ls_pair(TINY, "qnnpack", kind="mixed", twin=False)
    x, y = _qat_batches(TINY)[0]
    _qat_step(a, x, y)
    e = qat_vit_amd.export_int8(a)
    with pytest.raises(NotImplementedError, match="LayerScale"):
        qat_vit_amd.Int8Student(e)
    q = qat_vit_amd.import_int8(e)
    for (n, u), (_, v) in zip(a.named_parameters(), q.named_parameters()):
        if n.endswith(".gamma"):
            assert torch.equal(u, v), n
    a.eval()
    from torch.ao.quantization import disable_observer

    a.apply(disable_observer)
    with torch.no_grad():
        assert torch.equal(a(x), q(x))


def test_fake_quant_switching_keeps_working_with_layer_scale_bound(native_lib):
    from torch.ao.quantization import disable_fake_quant, enable_fake_quant

    a, _ = _ls_pair(TINY, "qnnpack", kind="mixed", twin=False)
    gam = [(n, p) for n, p in a.named_parameters() if n.endswith(".gamma")]
    batches = _qat_batches(TINY, n=3)
    for k, (x, y) in enumerate(batches):
        a.apply(disable_fake_quant if k == 1 else enable_fake_quant)
        out, _ = _qat_step(a, x, y)
        assert engine_of(a).fq_mode == ("observe" if k == 1 else "qat") and torch.isfinite(out).all()
        for n, p in gam:
            assert torch.isfinite(p.grad).all() and torch.count_nonzero(p.grad) > 0, (k, n)
