"""ClipAdamW's weight EMA (qatvit_optim_adamw_ema / _groups_ema / qatvit_optim_ema / qatvit_optim_swap).

The average is checked BIT FOR BIT against a NumPy fp32 restatement of the formula of include/qatvit.h (`_lerp32` below), fed the average before the
step and the parameter after it; the update itself against the entries without the average (parameters, both moments and the norm `torch.equal`).
The one tolerance is the project's own bound for the parameters, rel L2 2e-6 against an fp64 chain run beside stock fp64 AdamW: the average is a
convex combination of parameter iterates that already meet it, plus one fp32 rounding per step.  Shapes: tests/test_gpu_optim.py's (numel 1 and 7,
a 40000-element tensor over three chunks, exact chunk multiples)."""
import collections
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import qat_vit_amd  # noqa: E402
from qat_vit_amd import native  # noqa: E402
from qat_vit_amd.optim import _CHUNK, ClipAdamW, ema_warmup_decay  # noqa: E402
from tests.test_gpu_optim import SHAPES, _params  # noqa: E402
from tests.test_gpu_optim_groups import CUTS3, HYPER3, SCALES, _Counting, _split  # noqa: E402
from tests.util import rel_l2  # noqa: E402

DECAYS = [0.9999, 0.99, 0.5, 0.1, 0.0]          # w < 0.5 (two), w = 0.5 and w > 0.5 (the other branch), w = 1 (the exact copy)
HYPER1 = [dict(lr=1.5e-4 * 0.5, weight_decay=1e-3, betas=(0.9, 0.999), eps=1e-8)]
LAYOUTS = {"one": ([0, len(SHAPES)], HYPER1), "three": (CUTS3, HYPER3)}
POISON = 1234.5


def _lerp32(e, p, decay):
    """include/qatvit.h, restated: w = (float)(1.0 - decay); d = p - e; e' = w < 0.5f ? e + w * d : p - d * (1.0f - w), every operation in fp32."""
    e, p = e.detach().cpu().numpy(), p.detach().cpu().numpy()
    assert e.dtype == p.dtype == np.float32
    w = np.float32(1.0 - decay)
    d = p - e
    out = e + w * d if w < np.float32(0.5) else p - d * (np.float32(1.0) - w)
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def _assert_lerp(ema_after, ema_before, p_after, decay, tag):
    want = _lerp32(ema_before, p_after, decay)
    assert torch.equal(ema_after.detach().cpu(), want), (tag, (ema_after.detach().cpu() - want).abs().max().item())


@functools.lru_cache(maxsize=None)
def _cpu_grads():
    """The gradients of four steps (clipped, not clipped, ... at max_norm 1), shared by every test here; left unchanged."""
    g = torch.Generator().manual_seed(7)
    return [[torch.randn(s, generator=g) * SCALES[it] for s in SHAPES] for it in range(4)]


@functools.lru_cache(maxsize=None)
def _gpu_grads():
    return [[x.cuda() for x in gs] for gs in _cpu_grads()]


def _fresh(layout, **kw):
    cuts, hyper = LAYOUTS[layout]
    ps = [torch.nn.Parameter(p.detach().clone().cuda()) for p in _params(1, SHAPES)]
    return ps, ClipAdamW(_split(ps, cuts, hyper), **kw)


def _give(ps, it, skip=()):
    for i, (q, gr) in enumerate(zip(ps, _gpu_grads()[it])):
        q.grad = None if i in skip else gr.clone()


def _averages_before(opt, ps):
    """What the next step averages from: state[p]["ema"], or - it is created as a clone of p before the update - the parameter."""
    return [opt.state[q]["ema"].clone() if "ema" in opt.state.get(q, ()) else q.detach().clone() for q in ps]


def _flat_avg(opt):
    return [e for es in opt.ema_parameters() for e in es]


@functools.lru_cache(maxsize=None)
def _plain_run(layout):
    """Four steps of ClipAdamW WITHOUT the average (the entries that exist): per step (parameters, exp_avg, exp_avg_sq, norm), computed once."""
    ps, opt = _fresh(layout)
    out = []
    for it in range(4):
        _give(ps, it)
        norm = opt.clip_grad_norm_(1.0).clone()
        opt.step()
        out.append(([q.detach().clone() for q in ps], [opt.state[q]["exp_avg"].clone() for q in ps], [opt.state[q]["exp_avg_sq"].clone() for q in ps], norm))
    assert all("ema" not in opt.state[q] for q in ps)
    return out


@functools.lru_cache(maxsize=None)
def _fp64_iterates(layout):
    """Stock fp64 AdamW + clip_grad_norm_ on the CPU over the same four steps: the parameters before the first step and after each."""
    cuts, hyper = LAYOUTS[layout]
    ps = [torch.nn.Parameter(p.detach().double()) for p in _params(1, SHAPES)]
    opt = torch.optim.AdamW(_split(ps, cuts, hyper), foreach=False)
    its = [[p.detach().clone() for p in ps]]
    for it in range(4):
        for p, gr in zip(ps, _cpu_grads()[it]):
            p.grad = gr.double()
        torch.nn.utils.clip_grad_norm_(ps, 1.0, foreach=False)
        opt.step()
        its.append([p.detach().clone() for p in ps])
    return its


@pytest.fixture
def counting(native_lib, monkeypatch):
    proxy = _Counting(native_lib)
    monkeypatch.setattr(native, "lib", lambda: proxy)
    return proxy.calls


# ---- 1: identity of the update, the average bit for bit, the fp64 chain
@pytest.mark.parametrize("layout", ["one", "three"])
@pytest.mark.parametrize("decay", DECAYS)
def test_update_is_identical_and_average_is_the_formula(native_lib, layout, decay):
    plain = _plain_run(layout)
    ps, opt = _fresh(layout, ema_decay=decay)
    assert all(e is q for e, q in zip(_flat_avg(opt), ps)) and not opt.state          # no state yet: every parameter is its own average
    for it in range(4):
        _give(ps, it)
        before = _averages_before(opt, ps)
        norm = opt.clip_grad_norm_(1.0).clone()
        opt.step()
        want_p, want_m, want_v, want_norm = plain[it]
        assert torch.equal(norm, want_norm), it
        for i, q in enumerate(ps):
            st = opt.state[q]
            assert torch.equal(q.detach(), want_p[i]), (it, i, "param")
            assert torch.equal(st["exp_avg"], want_m[i]) and torch.equal(st["exp_avg_sq"], want_v[i]), (it, i, "moments")
            assert int(st["step"]) == it + 1
            _assert_lerp(st["ema"], before[i], q, decay, (it, i))
            if decay == 0.0:
                assert torch.equal(st["ema"], q.detach()), (it, i, "decay 0 is the exact copy")
    assert all(e is opt.state[q]["ema"] for e, q in zip(_flat_avg(opt), ps))
    # the fp64 chain beside stock fp64 AdamW
    its = _fp64_iterates(layout)
    for i, q in enumerate(ps):
        e64 = its[0][i].clone()
        for it in range(4):
            e64 = e64 + (1.0 - decay) * (its[it + 1][i] - e64)
        assert rel_l2(opt.state[q]["ema"].cpu(), e64) < 2e-6, (i, rel_l2(opt.state[q]["ema"].cpu(), e64))


# ---- 2: parameters without .grad
def test_parameters_without_grad_are_averaged_by_one_separate_launch(counting):
    decay, skip = 0.9, {3, 4, 5}          # all of group 1 (a whole group, so that it may rejoin with its own step count)
    ps, opt = _fresh("three", ema_decay=decay)
    for it in range(4):
        idle = skip if it in (1, 2) else set()
        _give(ps, it, skip=idle)
        before = _averages_before(opt, ps)
        held = [q.detach().clone() for q in ps]
        counting.clear()
        opt.step(max_norm=1.0)
        assert counting["qatvit_optim_ema"] == (1 if idle else 0), (it, counting)
        assert counting["qatvit_optim_adamw_groups_ema"] == 1 and counting["qatvit_optim_grad_norm"] == 1, (it, counting)
        assert counting["qatvit_optim_adamw_groups"] == counting["qatvit_optim_adamw"] == counting["qatvit_optim_adamw_ema"] == 0, (it, counting)
        for i, q in enumerate(ps):
            if i in idle:
                assert torch.equal(q.detach(), held[i]), (it, i)          # no update: the average moves towards the unchanged value
            else:
                assert not torch.equal(q.detach(), held[i]), (it, i)
            _assert_lerp(opt.state[q]["ema"], before[i], q, decay, (it, i))
    assert [int(opt.state[q]["step"]) for q in ps] == [4, 4, 4, 2, 2, 2, 4, 4, 4]
    # one group goes through the other entry
    ps, opt = _fresh("one", ema_decay=decay)
    _give(ps, 0)
    counting.clear()
    opt.step(max_norm=1.0)
    assert counting == collections.Counter(qatvit_optim_grad_norm=1, qatvit_optim_adamw_ema=1), counting
    # a parameter that never had a gradient has no state and is its own average; with every gradient gone, only the averages move
    _give(ps, 1, skip=set(range(len(SHAPES))))
    before = [opt.state[q]["ema"].clone() for q in ps]
    counting.clear()
    opt.step(max_norm=1.0)
    assert counting == collections.Counter(qatvit_optim_ema=1), counting
    for i, q in enumerate(ps):
        _assert_lerp(opt.state[q]["ema"], before[i], q, decay, ("all idle", i))
    extra = torch.nn.Parameter(torch.ones(5, device="cuda"))
    opt.add_param_group(dict(params=[extra]))
    assert opt.ema_parameters()[1][0] is extra and extra not in opt.state


# ---- 3: direct calls with guarded operands
def _guarded(values, offset=0):
    """`values` placed inside a larger poisoned buffer with 64 guard elements on each side (+ `offset` elements: 1 breaks the 16-byte alignment)."""
    n = values.numel()
    big = torch.full((n + 128 + 4,), POISON, device="cuda")
    view = big[64 + offset:64 + offset + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == 4 * offset
    return big, view


def _guards_intact(big, view, offset):
    n = view.numel()
    return bool((big[:64 + offset] == POISON).all()) and bool((big[64 + offset + n:] == POISON).all())


def _tables(tensors):
    ct, ci = [], []
    for ti, x in enumerate(tensors):
        n = (x.numel() + _CHUNK - 1) // _CHUNK
        ct += [ti] * n
        ci += list(range(n))
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")   # noqa: E731
    return torch.tensor([x.numel() for x in tensors], dtype=torch.int64, device="cuda"), i32(ct), i32(ci), len(ct)


def _ptr_tables(lists):
    """One device array of addresses per tensor list; the caller holds them until its launch has been issued."""
    return [torch.tensor([x.data_ptr() for x in xs], dtype=torch.int64, device="cuda") for xs in lists]


@pytest.mark.parametrize("ema_offset", [0, 1], ids=["aligned", "ema_off_by_one"])
def test_direct_calls_with_guarded_operands(native_lib, ema_offset):
    L, st = native_lib, native.stream_ptr()
    sizes = [1, 3, 4, 5, 16384, 16385]
    g = torch.Generator().manual_seed(21)
    init = {k: [torch.randn(n, generator=g) * s for n in sizes] for k, s in (("p", 0.05), ("g", 1.0), ("m", 0.01), ("e", 0.05))}
    init["v"] = [torch.rand(n, generator=g) * 1e-3 for n in sizes]
    lr, b1, b2, eps, wd, step, decay = 1e-3, 0.9, 0.999, 1e-8, 0.05, 3, 0.99
    clip = torch.tensor([2.0, 0.5], device="cuda")                        # {norm, coefficient}: every gradient enters halved
    # the reference: qatvit_optim_adamw on clones
    ref = {k: [x.cuda() for x in init[k]] for k in "pgmv"}
    numel, ct, ci, n = _tables(ref["p"])
    tabs = _ptr_tables([ref[k] for k in "pgmv"])
    native.check(L.qatvit_optim_adamw(*[t.data_ptr() for t in tabs], numel.data_ptr(), ct.data_ptr(), ci.data_ptr(), n, _CHUNK, lr, b1, b2, eps, wd, step,
                                      clip.data_ptr(), st), "adamw")

    def guarded_set():
        return {k: [_guarded(x, ema_offset if k == "e" else 0) for x in init[k]] for k in "pgmve"}

    def check_update(gs, tag):
        for k in "pgmve":
            for i, (big, view) in enumerate(gs[k]):
                assert _guards_intact(big, view, ema_offset if k == "e" else 0), (tag, k, sizes[i], "guard")
        for i in range(len(sizes)):
            for k in "pmv":
                assert torch.equal(gs[k][i][1], ref[k][i]), (tag, k, sizes[i])
            assert torch.equal(gs["g"][i][1].cpu(), init["g"][i]), (tag, "g", sizes[i])
            _assert_lerp(gs["e"][i][1], init["e"][i], gs["p"][i][1], decay, (tag, sizes[i]))

    views = lambda gs, keys: [[v for _, v in gs[k]] for k in keys]   # noqa: E731
    gs = guarded_set()
    tabs = _ptr_tables(views(gs, "pgmve"))
    native.check(L.qatvit_optim_adamw_ema(*[t.data_ptr() for t in tabs], numel.data_ptr(), ct.data_ptr(), ci.data_ptr(), n, _CHUNK,
                                          lr, b1, b2, eps, wd, step, decay, clip.data_ptr(), st), "adamw_ema")
    check_update(gs, "adamw_ema")

    gs = guarded_set()                                                    # two groups with the same hyper-parameters, tensors dealt alternately
    tg = torch.tensor([i % 2 for i in range(len(sizes))], dtype=torch.int32, device="cuda")
    rows = (native.AdamWGroup * 2)((lr, b1, b2, eps, wd, step), (lr, b1, b2, eps, wd, step))
    tabs = _ptr_tables(views(gs, "pgmve"))
    native.check(L.qatvit_optim_adamw_groups_ema(*[t.data_ptr() for t in tabs], numel.data_ptr(), tg.data_ptr(), ct.data_ptr(),
                                                 ci.data_ptr(), n, _CHUNK, rows, 2, decay, clip.data_ptr(), st), "adamw_groups_ema")
    check_update(gs, "adamw_groups_ema")

    # the average alone: p is read only
    gs = guarded_set()
    tabs = _ptr_tables(views(gs, "pe"))
    native.check(L.qatvit_optim_ema(tabs[0].data_ptr(), tabs[1].data_ptr(), numel.data_ptr(), ct.data_ptr(), ci.data_ptr(), n, _CHUNK, decay, st), "ema")
    for i in range(len(sizes)):
        assert _guards_intact(*gs["p"][i], 0) and _guards_intact(*gs["e"][i], ema_offset), ("ema", sizes[i], "guard")
        assert torch.equal(gs["p"][i][1].cpu(), init["p"][i]), ("ema", sizes[i])
        _assert_lerp(gs["e"][i][1], init["e"][i], init["p"][i], decay, ("ema", sizes[i]))

    # the exchange: once = swapped, twice = restored, both bit for bit
    gs = guarded_set()
    bits = lambda x: x.detach().cpu().view(torch.int32)   # noqa: E731
    tabs = _ptr_tables(views(gs, "pe"))
    for rounds in (1, 2):
        native.check(L.qatvit_optim_swap(tabs[0].data_ptr(), tabs[1].data_ptr(), numel.data_ptr(), ct.data_ptr(), ci.data_ptr(), n, _CHUNK, st), "swap")
        a, b = ("e", "p") if rounds == 1 else ("p", "e")
        for i in range(len(sizes)):
            assert _guards_intact(*gs["p"][i], 0) and _guards_intact(*gs["e"][i], ema_offset), ("swap", rounds, sizes[i], "guard")
            assert torch.equal(bits(gs["p"][i][1]), bits(init[a][i])) and torch.equal(bits(gs["e"][i][1]), bits(init[b][i])), ("swap", rounds, sizes[i])


# ---- 4: swap through the class
def test_swap_through_the_class(native_lib, counting):
    ps, opt = _fresh("three", ema_decay=0.9)
    for it in range(2):
        _give(ps, it)
        opt.step(max_norm=1.0)
    live = [q.detach().clone() for q in ps]
    avg = [opt.state[q]["ema"].clone() for q in ps]
    moments = [opt.state[q]["exp_avg"].clone() for q in ps]
    ptrs = [(q.data_ptr(), opt.state[q]["ema"].data_ptr()) for q in ps]
    assert not any(torch.equal(a, b) for a, b in zip(live, avg))

    def holds(params, emas):
        return all(torch.equal(q.detach(), a) and torch.equal(opt.state[q]["ema"], b) for q, a, b in zip(ps, params, emas))

    counting.clear()
    opt.swap_ema()
    assert counting == collections.Counter(qatvit_optim_swap=1) and opt.ema_swapped
    assert holds(avg, live) and [(q.data_ptr(), opt.state[q]["ema"].data_ptr()) for q in ps] == ptrs
    assert all(e is q for e, q in zip(_flat_avg(opt), ps))                 # the parameters hold the averages now
    _give(ps, 2)
    counting.clear()
    for call in (lambda: opt.step(), lambda: opt.step(max_norm=1.0), lambda: opt.clip_grad_norm_(1.0), lambda: opt.state_dict()):
        with pytest.raises(RuntimeError, match="swapped in"):
            call()
    with pytest.raises(RuntimeError, match="swapped in"):
        with opt.ema_weights():
            pass
    assert not counting and holds(avg, live) and opt.ema_swapped
    assert all(torch.equal(opt.state[q]["exp_avg"], m) and int(opt.state[q]["step"]) == 2 for q, m in zip(ps, moments))
    opt.swap_ema()
    assert holds(live, avg) and not opt.ema_swapped

    with opt.ema_weights() as inside:
        assert inside is opt and opt.ema_swapped and holds(avg, live)
    assert not opt.ema_swapped and holds(live, avg)
    with pytest.raises(KeyError, match="inside the block"):
        with opt.ema_weights():
            assert holds(avg, live)
            raise KeyError("inside the block")
    assert not opt.ema_swapped and holds(live, avg)
    assert [(q.data_ptr(), opt.state[q]["ema"].data_ptr()) for q in ps] == ptrs
    opt.step(max_norm=1.0)                                                 # and training goes on
    assert all(int(opt.state[q]["step"]) == 3 for q in ps)


# ---- 5: no host round trip
def test_scheduled_lr_and_decay_cost_no_host_round_trip(native_lib):
    ps, opt = _fresh("three", ema_decay=ema_warmup_decay(0.999, 0))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (1.0 + 0.5 * e))
    for q in ps:
        q.grad = torch.empty_like(q)                                       # fixed gradient buffers: the tables are keyed on their addresses

    def give(it):
        for q, d in zip(ps, _gpu_grads()[it]):
            q.grad.copy_(d)                                                # device to device

    give(0)
    opt.step(max_norm=1.0)                                                 # builds the tables and the averages
    sched.step()
    torch.cuda.synchronize()
    decays, snaps = [], []
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            ps[0].sum().item()                                             # the mode is honoured
        for it in range(1, 4):
            give(it)
            opt.ema_decay = ema_warmup_decay(0.999, it)
            decays.append(opt.ema_decay)
            before = [opt.state[q]["ema"].clone() for q in ps]
            opt.step(max_norm=1.0)
            sched.step()
            snaps.append((before, [q.detach().clone() for q in ps], [opt.state[q]["ema"].clone() for q in ps]))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert decays == [2 / 11, 3 / 12, 4 / 13]
    for k, (before, after_p, after_e) in enumerate(snaps):
        for i in range(len(ps)):
            _assert_lerp(after_e[i], before[i], after_p[i], decays[k], (k, i))
    assert all(int(opt.state[q]["step"]) == 4 for q in ps)


# ---- 6: checkpoints
def test_checkpoints_carry_the_average(native_lib):
    decay = 0.99
    ps_a, opt_a = _fresh("three", ema_decay=decay)                         # the uninterrupted run
    for it in range(4):
        _give(ps_a, it)
        opt_a.step(max_norm=1.0)
    ps_b, opt_b = _fresh("three", ema_decay=decay)
    for it in range(2):
        _give(ps_b, it)
        opt_b.step(max_norm=1.0)
    sd = copy.deepcopy(opt_b.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "ema"} and len(sd["state"]) == len(SHAPES)
    assert "ema_decay" not in sd["param_groups"][0]
    cuts, hyper = LAYOUTS["three"]
    ps_c = [torch.nn.Parameter(q.detach().clone()) for q in ps_b]
    opt_c = ClipAdamW(_split(ps_c, cuts, hyper), ema_decay=decay)
    opt_c.load_state_dict(copy.deepcopy(sd))
    assert all(opt_c.state[q]["ema"].is_cuda and opt_c.state[q]["ema"].data_ptr() != opt_b.state[r]["ema"].data_ptr() for q, r in zip(ps_c, ps_b))
    for it in range(2, 4):
        _give(ps_c, it)
        opt_c.step(max_norm=1.0)
    for i, (q, r) in enumerate(zip(ps_c, ps_a)):
        assert torch.equal(q.detach(), r.detach()), i
        for name in ("exp_avg", "exp_avg_sq", "ema"):
            assert torch.equal(opt_c.state[q][name], opt_a.state[r][name]), (i, name)

    # the same checkpoint in stock AdamW on the CPU: the extra key is ignored, and it steps
    ps_d = [torch.nn.Parameter(q.detach().cpu().clone()) for q in ps_b]
    opt_d = torch.optim.AdamW(_split(ps_d, cuts, hyper), foreach=False)
    opt_d.load_state_dict(copy.deepcopy(sd))
    for q, gr in zip(ps_d, _cpu_grads()[2]):
        q.grad = gr.clone()
    torch.nn.utils.clip_grad_norm_(ps_d, 1.0, foreach=False)
    opt_d.step()
    _give(ps_b, 2)
    opt_b.step(max_norm=1.0)
    for i, (q, r) in enumerate(zip(ps_d, ps_b)):
        assert int(opt_d.state[q]["step"]) == 3 and rel_l2(r.detach().cpu(), q.detach()) < 5e-5, i   # test_gpu_optim's bound against fp32 stock with a clip

    # a checkpoint without averages: they start from the parameters at the next step
    bare = copy.deepcopy(sd)
    for st in bare["state"].values():
        del st["ema"]
    ps_e = [torch.nn.Parameter(q.detach().clone()) for q in ps_c]
    opt_e = ClipAdamW(_split(ps_e, cuts, hyper), ema_decay=decay)
    opt_e.load_state_dict(bare)
    assert all(e is q for e, q in zip(_flat_avg(opt_e), ps_e))
    start = [q.detach().clone() for q in ps_e]
    _give(ps_e, 2)
    opt_e.step(max_norm=1.0)
    for i, q in enumerate(ps_e):
        assert int(opt_e.state[q]["step"]) == 3
        _assert_lerp(opt_e.state[q]["ema"], start[i], q, decay, ("bare", i))


# ---- 7: end to end on the tiny student
def _tiny():
    torch.manual_seed(0)
    return qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=128, depth=2, num_heads=2, img_size=32)


def test_tiny_float_student_evaluates_its_average_in_place(native_lib):
    from qat_vit_amd import functional as F

    model = _tiny().cuda().train()
    x, y = torch.randn(4, 3, 32, 32).cuda(), torch.randint(0, 10, (4,)).cuda()
    opt = ClipAdamW(model.parameters(), lr=1e-3, weight_decay=1e-3, ema_decay=0.9)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        F.kd_ce_loss(model(x), None, y, 4.0, 0.5, 0.1)[0].backward()
        opt.step(max_norm=1.0)
    model.eval()
    ptrs = [p.data_ptr() for p in model.parameters()]
    sd = opt.ema_state_dict(model)
    assert list(sd) == list(model.state_dict())
    twin = copy.deepcopy(model)
    twin.load_state_dict(sd)
    with torch.no_grad():
        live = model(x).clone()
        with opt.ema_weights():
            averaged = model(x).clone()
            inside = opt.ema_state_dict(model)                             # the same checkpoint from inside the block
        assert torch.equal(model(x), live)
        assert torch.equal(averaged, twin(x)) and not torch.equal(averaged, live)
    assert [p.data_ptr() for p in model.parameters()] == ptrs
    for k in sd:
        assert torch.equal(inside[k], sd[k]), k
    for n, p in model.named_parameters():
        assert torch.equal(sd[n], opt.state[p]["ema"]) and sd[n].data_ptr() != opt.state[p]["ema"].data_ptr(), n
    # through DistributedDataParallel's .module: the keys are the bare model's
    wrapped = torch.nn.parallel.DistributedDataParallel.__new__(torch.nn.parallel.DistributedDataParallel)
    torch.nn.Module.__init__(wrapped)
    wrapped.module = model
    assert list(opt.ema_state_dict(wrapped)) == list(sd)


def test_prepared_student_checkpoint_keeps_keys_and_live_buffers(native_lib):
    from qat_vit_amd import functional as F
    from tests.util import prepare

    model = prepare(_tiny().cuda(), "qnnpack")
    x, y = torch.randn(4, 3, 32, 32).cuda(), torch.randint(0, 10, (4,)).cuda()
    opt = ClipAdamW(model.parameters(), lr=1e-3, weight_decay=1e-3, ema_decay=0.9)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        F.kd_ce_loss(model(x), None, y, 4.0, 0.5, 0.1)[0].backward()
        opt.step(max_norm=1.0)
    live, sd = model.state_dict(), opt.ema_state_dict(model)
    assert list(sd) == list(live)
    names = {n for n, _ in model.named_parameters()}
    params = dict(model.named_parameters())
    assert names and names < set(sd)
    for k in sd:
        if k in names:
            assert torch.equal(sd[k], opt.state[params[k]]["ema"]), k
        else:
            assert torch.equal(sd[k], live[k]), k                          # buffers (observer ranges, scales, zero points) are the live ones
    assert not any(torch.equal(sd[k], live[k]) for k in names if params[k].ndim == 2)   # the weight matrices' averages are not the live weights
