"""ClipLamb (qatvit_optim_grad_norm + qatvit_optim_lamb_moments + qatvit_optim_lamb_apply) against tests/lamb_ref.py, the fp64 restatement of the
arithmetic of include/qatvit.h, fed the kernels' own clip coefficient.

One parameter set takes every path of the two kernels: numels 1, 3, 4, 5 (scalar tails, an empty vector body), 16383 / 16384 / 16385 (around one
chunk), 2 * 16384 + 7 (two full chunks and a tail: the tensor's partial sums cross workgroups), a 2-D tensor, a view one element into a larger buffer
(the 16-byte test is false: scalar path), an all-zero tensor under weight decay (||p|| = 0 -> trust 1), a tensor without a gradient, and three groups:
weight_decay 0.05, weight_decay 0 (trust exactly 1 without always_adapt), and a third lr / betas / eps.  Half of the tensors are large against their
update direction (trust > 1), so trust_clip has something to cap.

Bounds.  exp_avg / exp_avg_sq: rel L2 < 2e-6 against the fp64 chain, the bar of tests/test_gpu_optim.py for the same element-wise arithmetic.  The
parameters and the trust ratios depend on two fp32 norms over up to 32775 elements, which that bar does not cover; theirs is measured: the same
lines of lamb_ref evaluated with stock fp32 torch ops on this GPU have an error against the fp64 chain, and the kernels may have twice that error, but
no less than 2e-6 is asked.  Both figures are printed per case (-s shows them); tools/bench_optim_lamb.py writes them into profiles/optim_lamb_bench.txt."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import qat_vit_amd  # noqa: E402
from qat_vit_amd import native, vit_param_groups  # noqa: E402
from qat_vit_amd.optim import _CHUNK, MAX_GROUPS, ClipLamb  # noqa: E402
from tests.lamb_ref import lamb_ref  # noqa: E402
from tests.util import rel_l2  # noqa: E402

assert _CHUNK == 16384
SHAPES = [(1,), (4,), (16383,), (16385,), (2 * 16384 + 7,), (48, 100), (33,), (3,), (16384,), (10,), (5,), (4099,)]
ZERO, NO_GRAD, VIEW = 6, 9, 11
CUTS = [0, 7, 10, len(SHAPES)]
HYPER3 = [dict(lr=1e-3, weight_decay=0.05), dict(lr=2e-3, weight_decay=0.0), dict(lr=3e-3, weight_decay=0.02, betas=(0.8, 0.99), eps=1e-8)]
SAME3 = [dict(lr=1e-3, weight_decay=0.05)] * 3
GROUP_OF = [gi for gi in range(3) for _ in range(CUTS[gi], CUTS[gi + 1])]
SCALES = [3.0, 0.001, 1.0, 0.002, 50.0]   # the norm over ~1.1e5 gradient elements is ~330 * scale: max_norm 1 clips steps 0, 2, 4 and not 1, 3
LIVE = [i for i in range(len(SHAPES)) if i != NO_GRAD]
FLOOR = 2e-6
POISON = 1234.5


@functools.lru_cache(maxsize=None)
def _cpu_params():
    g = torch.Generator().manual_seed(3)
    return [torch.zeros(s) if i == ZERO else torch.randn(s, generator=g) * (3.0 if i % 2 else 0.05) for i, s in enumerate(SHAPES)]


@functools.lru_cache(maxsize=None)
def _cpu_grads():
    """The gradients of five steps, shared by every test here; left unchanged."""
    g = torch.Generator().manual_seed(7)
    return [[torch.randn(s, generator=g) * SCALES[it] for s in SHAPES] for it in range(5)]


@functools.lru_cache(maxsize=None)
def _gpu_grads():
    return [[x.cuda() for x in gs] for gs in _cpu_grads()]


def _fresh_params():
    ps = []
    for i, x in enumerate(_cpu_params()):
        if i == VIEW:
            big = torch.empty(x.numel() + 8, device="cuda")
            q = torch.nn.Parameter(big[1:1 + x.numel()])
            q.data.copy_(x)
            assert q.data_ptr() % 16 == 4 and q.is_contiguous()
        else:
            q = torch.nn.Parameter(x.clone().cuda())
        ps.append(q)
    return ps


def _split(ps, hyper):
    return [dict(params=ps[a:b], **h) for a, b, h in zip(CUTS[:-1], CUTS[1:], hyper)]


def _fresh(hyper=HYPER3, groups=True, **kw):
    ps = _fresh_params()
    return ps, ClipLamb(_split(ps, hyper) if groups else ps, **kw)


def _give(ps, it, skip=(NO_GRAD,)):
    for i, (q, gr) in enumerate(zip(ps, _gpu_grads()[it])):
        q.grad = None if i in skip else gr.clone()


def _snapshot(ps, opt):
    return ([q.detach().clone() for q in ps], [opt.state[q]["exp_avg"].clone() if q in opt.state else None for q in ps],
            [opt.state[q]["exp_avg_sq"].clone() if q in opt.state else None for q in ps], opt.trust_ratios().clone())


def _run_kernels(steps, max_norm, hyper=HYPER3, groups=True, skip=lambda it: (NO_GRAD,), **kw):
    """`steps` steps of a fresh ClipLamb: per step (p, m, v, trust) and the clip coefficient the update used, read from the norm launch's own output."""
    ps, opt = _fresh(hyper, groups, **kw)
    out, coefs = [], []
    for it in range(steps):
        _give(ps, it, skip(it))
        coef = 1.0
        if max_norm is not None:
            opt.clip_grad_norm_(max_norm)
            coef = opt._pending[1].item()
        opt.step()
        out.append(_snapshot(ps, opt))
        coefs.append(coef)
    return ps, opt, out, coefs


def _hyper_of(opt, i):
    g = opt.param_groups[GROUP_OF[i]] if len(opt.param_groups) > 1 else opt.param_groups[0]
    return dict(lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], grad_averaging=g["grad_averaging"],
                always_adapt=g["always_adapt"], trust_clip=g["trust_clip"])


def _run_ref(opt, steps, coefs, dtype):
    """The same steps through lamb_ref, chained in `dtype` (float64: the reference, on the CPU; float32: stock fp32 torch ops on the GPU)."""
    dev = "cpu" if dtype == torch.float64 else "cuda"
    state = {i: (_cpu_params()[i].to(dev), torch.zeros(SHAPES[i], device=dev), torch.zeros(SHAPES[i], device=dev)) for i in LIVE}
    out = []
    for it in range(steps):
        trusts = []
        for i in LIVE:
            p, m, v = state[i]
            p, m, v, trust = lamb_ref(p, _cpu_grads()[it][i].to(dev), m, v, step=it + 1, coef=coefs[it], dtype=dtype, **_hyper_of(opt, i))
            state[i] = (p, m, v)
            trusts.append(trust)
        out.append(({i: state[i][0].cpu() for i in LIVE}, {i: state[i][1].cpu() for i in LIVE}, {i: state[i][2].cpu() for i in LIVE}, np.array(trusts)))
    return out


def compare_with_reference(steps, max_norm, tag, **kw):
    """Asserts the bounds of the module docstring on every step and tensor; returns the measured pair per quantity: {"p": (kernel, stock fp32),
    "trust": (kernel, stock fp32)}, each the largest rel L2 error against the fp64 chain."""
    ps, opt, ours, coefs = _run_kernels(steps, max_norm, **kw)
    if max_norm is not None:
        assert [c < 1.0 for c in coefs] == [True, False, True, False, True][:steps], coefs   # clipping is active in some steps and not in others
    ref, stock = _run_ref(opt, steps, coefs, torch.float64), _run_ref(opt, steps, coefs, torch.float32)
    worst = {"p": (0.0, 0.0), "trust": (0.0, 0.0), "m": 0.0, "v": 0.0}
    for it in range(steps):
        p, m, v, trust = ours[it]
        assert trust.shape == (len(LIVE),)
        for k, i in enumerate(LIVE):
            em, ev = rel_l2(m[i].cpu(), ref[it][1][i]), rel_l2(v[i].cpu(), ref[it][2][i])
            worst["m"], worst["v"] = max(worst["m"], em), max(worst["v"], ev)
            assert em < FLOOR and ev < FLOOR, (tag, it, i, em, ev)
            ek, es = rel_l2(p[i].cpu(), ref[it][0][i]), rel_l2(stock[it][0][i], ref[it][0][i])
            if ek >= worst["p"][0]:
                worst["p"] = (ek, es)
            assert ek <= max(2 * es, FLOOR), (tag, it, i, "p", ek, es)
        ek, es = rel_l2(trust.cpu(), ref[it][3]), rel_l2(stock[it][3], ref[it][3])
        if ek >= worst["trust"][0]:
            worst["trust"] = (ek, es)
        assert ek <= max(2 * es, FLOOR), (tag, it, "trust", ek, es)
        assert ps[NO_GRAD] not in opt.state and torch.equal(p[NO_GRAD].cpu(), _cpu_params()[NO_GRAD])
    print(f"\n[{tag}] rel L2 against the fp64 chain, kernels / stock fp32 torch ops on this GPU: p {worst['p'][0]:.3e} / {worst['p'][1]:.3e}, "
          f"trust {worst['trust'][0]:.3e} / {worst['trust'][1]:.3e}; exp_avg {worst['m']:.3e}, exp_avg_sq {worst['v']:.3e} (bar {FLOOR:g})")
    return ps, opt, ours, ref, worst


# ---- 1: five steps against the reference
@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["no_clip", "max_norm_1"])
def test_five_steps_match_the_reference(native_lib, max_norm):
    ps, opt, ours, ref, _ = compare_with_reference(5, max_norm, f"three groups, max_norm={max_norm}")
    for it in range(5):
        trust = ours[it][3].cpu()
        for k, i in enumerate(LIVE):
            if GROUP_OF[i] == 1 or (i == ZERO and it == 0):
                assert trust[k].item() == 1.0, (it, i)          # weight_decay 0 without always_adapt; ||p|| = 0 (before the first step): exactly 1
            else:
                assert trust[k].item() != 1.0, (it, i)
    assert (ours[0][3] > 1).any() and (ours[0][3] < 1).any()
    assert all(int(opt.state[q]["step"]) == 5 for i, q in enumerate(ps) if i != NO_GRAD)
    assert set(opt.state[ps[0]]) == {"step", "exp_avg", "exp_avg_sq"}
    # the all-zero tensor under decay moved by the plain step (trust 1)
    assert ours[0][0][ZERO].abs().max().item() > 0


def test_always_adapt_and_trust_clip(native_lib):
    _, _, ours, ref, _ = compare_with_reference(2, 1.0, "always_adapt", always_adapt=True)
    for it in range(2):
        trust = ours[it][3].cpu()
        for k, i in enumerate(LIVE):
            if GROUP_OF[i] == 1:
                assert trust[k].item() != 1.0 and abs(trust[k].item() - ref[it][3][k]) <= 1e-5 * ref[it][3][k], (it, i)
    assert (ours[0][3] > 1).any()
    _, _, capped, ref_c, _ = compare_with_reference(2, 1.0, "always_adapt + trust_clip", always_adapt=True, trust_clip=True)
    for it in range(2):
        assert capped[it][3].max().item() == 1.0 and (capped[it][3] < 1).any()
        assert np.array_equal(ref_c[it][3] == 1.0, capped[it][3].cpu().numpy() == 1.0)
    # grad_averaging=False goes through the same reference
    compare_with_reference(2, None, "grad_averaging=False", grad_averaging=False)


# ---- 2: bits
def _equal_runs(a, b, tag):
    for it, (x, y) in enumerate(zip(a, b)):
        for name, xs, ys in (("p", x[0], y[0]), ("m", x[1], y[1]), ("v", x[2], y[2])):
            for i in LIVE:
                assert torch.equal(xs[i], ys[i]), (tag, it, name, i)
        assert torch.equal(x[3], y[3]), (tag, it, "trust")


def test_bits_run_to_run_and_across_group_layouts(native_lib):
    _, _, a, ca = _run_kernels(3, 1.0)
    _, _, b, cb = _run_kernels(3, 1.0)
    assert ca == cb
    _equal_runs(a, b, "run to run")
    _, one, c, _ = _run_kernels(3, 1.0, hyper=SAME3[:1], groups=False, **SAME3[0])
    _, three, d, _ = _run_kernels(3, 1.0, hyper=SAME3)
    assert len(one.param_groups) == 1 and len(three.param_groups) == 3
    _equal_runs(c, d, "one group against three")
    assert not torch.equal(a[2][0][8], c[2][0][8])             # (tensor 8 has other hyper-parameters in the first pair: the comparison can fail)


# ---- 3: the weight average
def test_ema_is_the_lerp_of_a_twin_without_it(native_lib):
    d = 0.9
    grads_at = lambda it: () if it == 0 else (NO_GRAD,)   # noqa: E731  the tensor "without a gradient" has one in step 0 only: it owns an average
    _, twin_opt, twin, _ = _run_kernels(4, 1.0, skip=grads_at)
    ps, opt = _fresh(ema_decay=d)
    assert all(e is q for es, g in zip(opt.ema_parameters(), opt.param_groups) for e, q in zip(es, g["params"]))
    for it in range(4):
        _give(ps, it, grads_at(it))
        before = [opt.state[q]["ema"].clone() if "ema" in opt.state.get(q, ()) else q.detach().clone() for q in ps]
        opt.step(max_norm=1.0)
        for i, q in enumerate(ps):
            st = opt.state[q]
            assert torch.equal(q.detach(), twin[it][0][i]), (it, i, "p")
            assert torch.equal(st["exp_avg"], twin[it][1][i]) and torch.equal(st["exp_avg_sq"], twin[it][2][i]), (it, i, "moments")
            want = torch.lerp(before[i], q.detach(), 1 - d)
            if i == NO_GRAD and it:   # left out of the step: averaged by qatvit_optim_ema, whose two-rounding form tests/test_gpu_optim_ema.py pins
                assert rel_l2(st["ema"].cpu(), want.cpu()) < 2e-7, (it, i, "idle ema")
            else:
                assert torch.equal(st["ema"], want), (it, i, "ema")
        if it:
            assert torch.equal(opt.trust_ratios(), twin[it][3]) and len(opt.trust_ratios()) == len(LIVE)
            assert torch.equal(ps[NO_GRAD].detach(), twin[0][0][NO_GRAD]) and not torch.equal(opt.state[ps[NO_GRAD]]["ema"], before[NO_GRAD])   # the idle average advances
    assert [int(opt.state[q]["step"]) for q in ps] == [1 if i == NO_GRAD else 4 for i in range(len(ps))]
    assert set(opt.state[ps[0]]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
    # in-place swap: bit for bit there and back, no step while swapped
    live = [q.detach().clone() for q in ps]
    avg = [opt.state[q]["ema"].clone() for q in ps]
    ptrs = [q.data_ptr() for q in ps]
    with opt.ema_weights():
        assert opt.ema_swapped and all(torch.equal(q.detach(), a) and torch.equal(opt.state[q]["ema"], l) for q, a, l in zip(ps, avg, live))
        for call in (lambda: opt.step(), lambda: opt.step(max_norm=1.0), lambda: opt.clip_grad_norm_(1.0), lambda: opt.state_dict()):
            with pytest.raises(RuntimeError, match="ClipLamb: the averaged weights are swapped in"):
                call()
    assert not opt.ema_swapped and [q.data_ptr() for q in ps] == ptrs
    assert all(torch.equal(q.detach(), l) and torch.equal(opt.state[q]["ema"], a) for q, a, l in zip(ps, avg, live))
    # decay 0: the average is the parameter
    ps0, opt0 = _fresh(ema_decay=0.0)
    for it in range(2):
        _give(ps0, it)
        opt0.step(max_norm=1.0)
        assert all(torch.equal(opt0.state[q]["ema"], q.detach()) for i, q in enumerate(ps0) if i != NO_GRAD), it


# ---- 4: vit_param_groups on a tiny student
def test_vit_param_groups_with_layer_decay(native_lib):
    torch.manual_seed(0)
    model = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=128, depth=2, num_heads=2, img_size=32).cuda()
    groups = vit_param_groups(model, 0.05, lr=1e-3, layer_decay=0.75)
    assert 4 <= len(groups) <= 8 and len({g["lr"] for g in groups}) == 4
    opt = ClipLamb(groups)
    g = torch.Generator(device="cuda").manual_seed(4)
    params = [p for grp in opt.param_groups for p in grp["params"]]
    frozen = params[5]
    for p in params:
        p.grad = None if p is frozen else torch.randn(p.shape, device="cuda", generator=g) * 0.01
    before = [p.detach().clone() for p in params]
    opt.clip_grad_norm_(1.0)
    coef = opt._pending[1].item()
    opt.step()
    trust = opt.trust_ratios().cpu()
    assert len(trust) == len(params) - 1 == sum(p.grad is not None for p in params)
    k, worst = 0, (0.0, 0.0)
    for grp in opt.param_groups:
        hyper = dict(lr=grp["lr"], betas=grp["betas"], eps=grp["eps"], weight_decay=grp["weight_decay"])
        for p in grp["params"]:
            b = before[[id(q) for q in params].index(id(p))]
            if p is frozen:
                assert torch.equal(p.detach(), b) and p not in opt.state
                continue
            z = torch.zeros_like(b)
            want, m, v, t64 = lamb_ref(b.cpu(), p.grad.cpu(), z.cpu(), z.cpu(), step=1, coef=coef, **hyper)
            stock = lamb_ref(b, p.grad, z, z, step=1, coef=coef, dtype=torch.float32, **hyper)
            ek, es = rel_l2(p.detach().cpu(), want), rel_l2(stock[0].cpu(), want)
            worst = max(worst, (ek, es))
            assert ek <= max(2 * es, FLOOR), (k, ek, es)
            assert abs(trust[k].item() - t64) <= max(2 * abs(stock[3] - t64), FLOOR * t64), (k, trust[k].item(), t64, stock[3])
            assert grp["weight_decay"] != 0.0 or trust[k].item() == 1.0, k
            assert rel_l2(opt.state[p]["exp_avg"].cpu(), m) < FLOOR and rel_l2(opt.state[p]["exp_avg_sq"].cpu(), v) < FLOOR, k
            k += 1
    print(f"\n[vit_param_groups, layer decay] p: kernels {worst[0]:.3e} / stock fp32 {worst[1]:.3e}")


# ---- 5: checkpoint, group limit, no host round trip
def test_checkpoint_resumes_bit_for_bit(native_lib):
    _, _, whole, _ = _run_kernels(4, 1.0, ema_decay=0.99)
    ps, opt = _fresh(ema_decay=0.99)
    for it in range(2):
        _give(ps, it)
        opt.step(max_norm=1.0)
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "ema"} and len(sd["state"]) == len(LIVE)
    assert {"grad_averaging", "always_adapt", "trust_clip"} <= set(sd["param_groups"][0]) and "ema_decay" not in sd["param_groups"][0]
    ps2 = _fresh_params()
    for q, r in zip(ps2, ps):
        q.data.copy_(r.detach())
    opt2 = ClipLamb(_split(ps2, [dict(lr=7.0)] * 3), ema_decay=0.99)          # the groups' values come from the checkpoint
    opt2.load_state_dict(sd)
    for it in range(2, 4):
        _give(ps2, it)
        opt2.step(max_norm=1.0)
        for i in LIVE:
            assert torch.equal(ps2[i].detach(), whole[it][0][i]), (it, i)
            assert torch.equal(opt2.state[ps2[i]]["exp_avg"], whole[it][1][i]) and torch.equal(opt2.state[ps2[i]]["exp_avg_sq"], whole[it][2][i]), (it, i)
        assert torch.equal(opt2.trust_ratios(), whole[it][3]), it


def test_more_live_groups_than_one_launch_takes(native_lib):
    ps = [torch.nn.Parameter(torch.ones(3, device="cuda")) for _ in range(MAX_GROUPS + 1)]
    opt = ClipLamb([dict(params=[p], lr=1e-3 * (i + 1)) for i, p in enumerate(ps)])
    for p in ps[:-1]:
        p.grad = torch.ones(3, device="cuda")
    opt.step(max_norm=1.0)                                                     # MAX_GROUPS live groups: one launch pair
    assert len(opt.trust_ratios()) == MAX_GROUPS and all(int(opt.state[p]["step"]) == 1 for p in ps[:-1])
    ps[-1].grad = torch.ones(3, device="cuda")
    for call in (lambda: opt.step(), lambda: opt.clip_grad_norm_(1.0)):
        with pytest.raises(RuntimeError, match=f"^ClipLamb: {MAX_GROUPS + 1} param groups with gradients; one launch updates at most {MAX_GROUPS} groups$"):
            call()


def test_step_reads_nothing_back(native_lib):
    ps, opt = _fresh(ema_decay=0.5)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (1.0 + 0.5 * e))
    for i, q in enumerate(ps):
        q.grad = None if i == NO_GRAD else torch.empty_like(q)                 # fixed gradient buffers: the tables are keyed on their addresses

    def give(it):
        for i in LIVE:
            ps[i].grad.copy_(_gpu_grads()[it][i])

    give(0)
    opt.step(max_norm=1.0)
    sched.step()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            ps[0].sum().item()                                                 # the mode is honoured
        for it in range(1, 3):
            give(it)
            opt.ema_decay = 0.5 + 0.1 * it
            opt.step(max_norm=1.0)
            sched.step()
            trust = opt.trust_ratios()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert trust.is_cuda and trust.shape == (len(LIVE),) and all(int(opt.state[ps[i]]["step"]) == 3 for i in LIVE)
    # the scheduled lr reached the kernels: the same three steps with the same lr sequence set by hand
    ps2, opt2 = _fresh(ema_decay=0.5)
    base = [g["lr"] for g in opt2.param_groups]
    for it in range(3):
        _give(ps2, it)
        for g, b in zip(opt2.param_groups, base):
            g["lr"] = b * (1.0 / (1.0 + 0.5 * it))
        if it:
            opt2.ema_decay = 0.5 + 0.1 * it
        opt2.step(max_norm=1.0)
    for i in LIVE:
        assert torch.equal(ps[i].detach(), ps2[i].detach()) and torch.equal(opt.state[ps[i]]["ema"], opt2.state[ps2[i]]["ema"]), i


# ---- 6: direct calls with guarded operands
def _guarded(values, offset=0):
    n = values.numel()
    big = torch.full((n + 128 + 4,), POISON, device="cuda")
    view = big[64 + offset:64 + offset + n]
    view.copy_(values)
    return big, view


def _intact(big, view, offset):
    n = view.numel()
    return bool((big[:64 + offset] == POISON).all()) and bool((big[64 + offset + n:] == POISON).all())


@pytest.mark.parametrize("offset, decay", [(0, 0.9), (1, 0.25)], ids=["aligned", "off_by_one"])   # (0.25: the other branch of the lerp)
def test_direct_calls_stay_inside_their_operands(native_lib, offset, decay):
    L, st = native_lib, native.stream_ptr()
    sizes = [1, 3, 4, 5, 16383, 16384, 16385, 2 * 16384 + 7]
    g = torch.Generator().manual_seed(21)
    init = {k: [torch.randn(n, generator=g) * s for n in sizes] for k, s in (("p", 0.05), ("g", 1.0), ("m", 0.01), ("e", 0.05))}
    init["v"] = [torch.rand(n, generator=g) * 1e-3 for n in sizes]
    gs = {k: [_guarded(x, offset if k in "pe" else 0) for x in init[k]] for k in "pgmve"}
    tabs = {k: torch.tensor([v.data_ptr() for _, v in gs[k]], dtype=torch.int64, device="cuda") for k in "pgmve"}
    ct, ci, first = [], [], []
    for ti, n in enumerate(sizes):
        c = (n + _CHUNK - 1) // _CHUNK
        first.append(len(ct))
        ct += [ti] * c
        ci += list(range(c))
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")   # noqa: E731
    numel, ct_t, ci_t, first_t, tg = torch.tensor(sizes, dtype=torch.int64, device="cuda"), i32(ct), i32(ci), i32(first), i32([i % 2 for i in range(len(sizes))])
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.05)
    rows = (native.LambGroup * 2)(*[(1e-2, 0.9, 0.999, 1e-6, 0.05, 3, 1, 0, 0, 0)] * 2)
    clip = torch.tensor([2.0, 0.5], device="cuda")
    pbig, partials = _guarded(torch.zeros(2 * len(ct)))
    tbig, trust = _guarded(torch.zeros(len(sizes)))
    native.check(L.qatvit_optim_lamb_moments(tabs["p"].data_ptr(), tabs["g"].data_ptr(), tabs["m"].data_ptr(), tabs["v"].data_ptr(), numel.data_ptr(),
                                             tg.data_ptr(), ct_t.data_ptr(), ci_t.data_ptr(), len(ct), _CHUNK, rows, 2, clip.data_ptr(), partials.data_ptr(), st),
                 "lamb_moments")
    for i, n in enumerate(sizes):
        assert torch.equal(gs["p"][i][1].cpu(), init["p"][i]) and torch.equal(gs["g"][i][1].cpu(), init["g"][i]), ("moments leaves p and g", n)
        assert torch.equal(gs["e"][i][1].cpu(), init["e"][i]), n
    want = [lamb_ref(init["p"][i], init["g"][i], init["m"][i], init["v"][i], step=3, coef=0.5, **hyper) for i in range(len(sizes))]
    sums = partials.view(-1, 2).cpu().double()
    for i, n in enumerate(sizes):
        c = (n + _CHUNK - 1) // _CHUNK
        r = (want[i][0] - init["p"][i].double()) / (-1e-2 * want[i][3])
        assert abs(sums[first[i]:first[i] + c, 0].sum().item() - (r * r).sum().item()) <= 1e-5 * (r * r).sum().item(), ("sum r^2", n)
        assert abs(sums[first[i]:first[i] + c, 1].sum().item() - (init["p"][i].double() ** 2).sum().item()) <= 1e-5 * (init["p"][i].double() ** 2).sum().item(), n
    native.check(L.qatvit_optim_lamb_apply(tabs["p"].data_ptr(), tabs["m"].data_ptr(), tabs["v"].data_ptr(), tabs["e"].data_ptr(), numel.data_ptr(), tg.data_ptr(),
                                           first_t.data_ptr(), ct_t.data_ptr(), ci_t.data_ptr(), len(ct), _CHUNK, rows, 2, decay, partials.data_ptr(),
                                           trust.data_ptr(), st), "lamb_apply")
    for k in "pgmve":
        for i, (big, view) in enumerate(gs[k]):
            assert _intact(big, view, offset if k in "pe" else 0), (k, sizes[i], "guard")
    assert _intact(pbig, partials, 0) and _intact(tbig, trust, 0)
    for i, n in enumerate(sizes):
        assert rel_l2(gs["p"][i][1].cpu(), want[i][0]) < FLOOR and rel_l2(gs["m"][i][1].cpu(), want[i][1]) < FLOOR, n
        assert rel_l2(gs["v"][i][1].cpu(), want[i][2]) < FLOOR and abs(trust[i].item() - want[i][3]) <= 1e-5 * want[i][3], n
        assert torch.equal(gs["e"][i][1], torch.lerp(init["e"][i].cuda(), gs["p"][i][1], 1 - decay)), n
