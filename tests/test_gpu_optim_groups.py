"""ClipAdamW with several param groups (one global norm, one qatvit_optim_adamw_groups launch) against stock torch on the CPU:
``torch.optim.AdamW(groups, foreach=False)`` + ``torch.nn.utils.clip_grad_norm_(all_params, max_norm, foreach=False)`` in fp32 and in fp64, on the
same gradients.  Shapes and tolerances are those of tests/test_gpu_optim.py: rel L2 < 2e-6 against the fp64 run, < 5e-5 against the fp32 run when a
clip is applied (2e-6 without), the norm within 1e-6 relative of the fp64 norm."""
import collections
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import qat_vit_amd  # noqa: E402
from qat_vit_amd import native, vit_param_groups  # noqa: E402
from qat_vit_amd.optim import MAX_GROUPS, ClipAdamW  # noqa: E402
from tests.test_gpu_optim import SHAPES, _params  # noqa: E402
from tests.util import rel_l2  # noqa: E402

SCALES = [3.0, 0.02, 1.0, 50.0]          # clipped, not clipped, ...
HYPER3 = [dict(lr=1.5e-4, weight_decay=1e-3, betas=(0.9, 0.999), eps=1e-8),
          dict(lr=3e-3, weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6),
          dict(lr=5e-5, weight_decay=0.1, betas=(0.95, 0.9), eps=1e-10)]
CUTS3 = [0, 3, 6, len(SHAPES)]


def _split(ps, cuts, hyper):
    return [dict(params=ps[a:b], **h) for a, b, h in zip(cuts[:-1], cuts[1:], hyper)]


class _Trio:
    """The same parameters three times: stock fp32 and stock fp64 on the CPU, ours on the GPU."""

    def __init__(self, seed, shapes, cuts, hyper):
        self.ref = _params(seed, shapes)
        self.ref64 = [torch.nn.Parameter(p.detach().double()) for p in self.ref]
        self.ours = [torch.nn.Parameter(p.detach().clone().cuda()) for p in self.ref]
        self.o_ref = torch.optim.AdamW(_split(self.ref, cuts, hyper), foreach=False)
        self.o_ref64 = torch.optim.AdamW(_split(self.ref64, cuts, hyper), foreach=False)
        self.o_ours = ClipAdamW(_split(self.ours, cuts, hyper))

    def add_group(self, shapes, seed, **hyper):
        new = _params(seed, shapes)
        new64 = [torch.nn.Parameter(p.detach().double()) for p in new]
        mine = [torch.nn.Parameter(p.detach().clone().cuda()) for p in new]
        for o, ps, own in ((self.o_ref, new, self.ref), (self.o_ref64, new64, self.ref64), (self.o_ours, mine, self.ours)):
            o.add_param_group(dict(params=ps, **hyper))
            own += ps

    def set_grads(self, g, scale, skip=()):
        for i, (p, p64, q) in enumerate(zip(self.ref, self.ref64, self.ours)):
            if i in skip:
                p.grad = p64.grad = q.grad = None
                continue
            p.grad = torch.randn(p.shape, generator=g) * scale
            p64.grad = p.grad.double()
            q.grad = p.grad.clone().cuda()

    def step(self, max_norm):
        """One step of all three; the norm ours returned is checked against the fp64 norm."""
        live = lambda ps: [p for p in ps if p.grad is not None]   # noqa: E731
        kept = [None if q.grad is None else q.grad.clone() for q in self.ours]
        if max_norm is None:
            self.o_ref.step(), self.o_ref64.step(), self.o_ours.step()
        else:
            torch.nn.utils.clip_grad_norm_(live(self.ref), max_norm, foreach=False)
            tot64 = torch.nn.utils.clip_grad_norm_(live(self.ref64), max_norm, foreach=False)
            self.o_ref.step(), self.o_ref64.step()
            tot = self.o_ours.clip_grad_norm_(max_norm)
            self.o_ours.step()
            assert abs(tot.item() - tot64.item()) <= 1e-6 * tot64.item(), (tot.item(), tot64.item())
        for q, k in zip(self.ours, kept):      # ours leaves .grad unscaled (the coefficient is applied inside the update)
            assert (q.grad is None) == (k is None) and (k is None or torch.equal(q.grad, k))

    def check(self, clipped, tag=None):
        for i, (p, p64, q) in enumerate(zip(self.ref, self.ref64, self.ours)):
            assert rel_l2(q.detach().cpu(), p64.detach()) < 2e-6, (tag, i, "param")
            assert rel_l2(q.detach().cpu(), p.detach()) < (5e-5 if clipped else 2e-6), (tag, i, "param")
            assert bool(self.o_ours.state[q]) == bool(self.o_ref.state[p]), (tag, i)
            if not self.o_ref.state[p]:
                continue
            for name in ("exp_avg", "exp_avg_sq"):
                a = self.o_ours.state[q][name].cpu()
                assert rel_l2(a, self.o_ref64.state[p64][name]) < 2e-6, (tag, i, name)
                assert rel_l2(a, self.o_ref.state[p][name]) < (5e-5 if clipped else 2e-6), (tag, i, name)
            assert int(self.o_ours.state[q]["step"]) == int(self.o_ref.state[p]["step"]), (tag, i)


class _Counting:
    """Counts the calls that go through the library object."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)

        return counted


@pytest.fixture
def counting(native_lib, monkeypatch):
    proxy = _Counting(native_lib)
    monkeypatch.setattr(native, "lib", lambda: proxy)
    return proxy.calls


# ---- 1
@pytest.mark.parametrize("max_norm", [1.0, 1e6, None])
def test_three_groups_with_differing_hyper_parameters(native_lib, max_norm):
    t = _Trio(1, SHAPES, CUTS3, HYPER3)
    g = torch.Generator().manual_seed(7)
    for it in range(4):
        t.set_grads(g, SCALES[it])
        t.step(max_norm)
        t.check(max_norm is not None, it)
        assert all(int(t.o_ours.state[q]["step"]) == it + 1 for q in t.ours)


# ---- 2
def test_identical_groups_update_to_the_bits_of_one_group(native_lib):
    """The same parameters as one group (qatvit_optim_adamw, the existing path) and cut into two and into five groups with the same hyper-parameters
    (qatvit_optim_adamw_groups): parameters, both moments and the norm are EQUAL after each of four clipped steps."""
    base = _params(4, SHAPES)
    h = dict(lr=1.5e-4, weight_decay=1e-3, betas=(0.9, 0.999), eps=1e-8)
    runs = []
    for cuts in ([0, len(SHAPES)], [0, 4, len(SHAPES)], [0, 2, 4, 5, 7, len(SHAPES)]):
        ps = [torch.nn.Parameter(p.detach().clone().cuda()) for p in base]
        runs.append((ps, ClipAdamW(_split(ps, cuts, [h] * (len(cuts) - 1)))))
    g = torch.Generator().manual_seed(9)
    for it in range(4):
        grads = [(torch.randn(p.shape, generator=g) * SCALES[it]).cuda() for p in base]
        norms = []
        for ps, opt in runs:
            for q, gr in zip(ps, grads):
                q.grad = gr.clone()
            norms.append(opt.clip_grad_norm_(1.0).clone())
            opt.step()
        one_ps, one = runs[0]
        for (ps, opt), nrm in zip(runs[1:], norms[1:]):
            assert torch.equal(nrm, norms[0]), it
            for i, (q, q1) in enumerate(zip(ps, one_ps)):
                assert torch.equal(q.detach(), q1.detach()), (it, len(opt.param_groups), i)
                for name in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(opt.state[q][name], one.state[q1][name]), (it, len(opt.param_groups), i, name)


# ---- 3
def test_28_groups_take_two_library_calls(counting):
    small = [s for s in SHAPES if s not in ((384, 384), (1536, 384))]
    shapes = [small[i % len(small)] for i in range(28)]
    ps = [torch.nn.Parameter(p.detach().cuda()) for p in _params(5, shapes)]
    opt = ClipAdamW([dict(params=[p], lr=1e-3 * 0.9 ** i, weight_decay=0.05 * (i % 2)) for i, p in enumerate(ps)])
    assert len(opt.param_groups) == 28
    for k in range(2):
        for p in ps:
            p.grad = torch.ones_like(p)
        counting.clear()
        opt.step(max_norm=1.0)
        assert counting["qatvit_optim_grad_norm"] == 1 and counting["qatvit_optim_adamw_groups"] == 1 and counting["qatvit_optim_adamw"] == 0, (k, counting)


# ---- 4
def test_a_scheduled_lr_costs_no_host_round_trip(native_lib):
    """After the first step the tables exist; three more steps under LambdaLR (every group's lr changes before each) run with synchronising calls
    turned into errors - a host-to-device copy from pageable memory is one - and still match stock torch under the same schedule."""
    t = _Trio(6, SHAPES, CUTS3, HYPER3)
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, lambda e: 1.0 / (1.0 + 0.5 * e)) for o in (t.o_ref, t.o_ref64, t.o_ours)]
    g = torch.Generator().manual_seed(8)
    cpu_grads = [[torch.randn(p.shape, generator=g) * SCALES[it] for p in t.ref] for it in range(4)]
    gpu_grads = [[x.cuda() for x in gs] for gs in cpu_grads]

    # the native side's gradients live in fixed buffers, as the engine's flat gradient buffer does: the tables are keyed on their addresses
    for q in t.ours:
        q.grad = torch.empty_like(q)

    def give_refs(it):
        for p, p64, c in zip(t.ref, t.ref64, cpu_grads[it]):
            p.grad, p64.grad = c.clone(), c.double()

    def give_ours(it):
        for q, d in zip(t.ours, gpu_grads[it]):
            q.grad.copy_(d)                              # device to device: no synchronisation

    give_refs(0)
    give_ours(0)
    t.step(1.0)                                          # builds the tables
    for s in scheds:
        s.step()
    torch.cuda.synchronize()
    lrs, norms = [], []
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            t.ours[0].sum().item()                       # the mode is honoured: a synchronising call raises
        for it in range(1, 4):
            give_ours(it)
            lrs.append([grp["lr"] for grp in t.o_ours.param_groups])
            norms.append(t.o_ours.clip_grad_norm_(1.0).clone())
            t.o_ours.step()
            scheds[2].step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert lrs[0] != lrs[1] != lrs[2] and all(a != b for a, b in zip(lrs[0], lrs[2]))
    for it in range(1, 4):
        give_refs(it)
        assert [grp["lr"] for grp in t.o_ref.param_groups] == lrs[it - 1]
        torch.nn.utils.clip_grad_norm_(t.ref, 1.0, foreach=False)
        tot64 = torch.nn.utils.clip_grad_norm_(t.ref64, 1.0, foreach=False)
        t.o_ref.step(), t.o_ref64.step()
        scheds[0].step(), scheds[1].step()
        assert abs(norms[it - 1].item() - tot64.item()) <= 1e-6 * tot64.item()
    t.check(True)
    assert all(int(t.o_ours.state[q]["step"]) == 4 for q in t.ours)


# ---- 5
def test_a_group_added_later_starts_at_step_one(native_lib):
    t = _Trio(10, SHAPES[:6], [0, 3, 6], HYPER3[:2])
    g = torch.Generator().manual_seed(11)
    for it in range(2):
        t.set_grads(g, SCALES[it])
        t.step(1.0)
    t.add_group(SHAPES[6:], 12, **HYPER3[2])
    t.set_grads(g, SCALES[2])
    t.step(1.0)
    t.check(True, "after add_param_group")
    assert [int(t.o_ours.state[q]["step"]) for q in t.ours] == [3] * 6 + [1] * 3
    t.set_grads(g, SCALES[3])
    t.step(1.0)
    t.check(True, "second step after add_param_group")


def test_parameters_and_groups_without_a_gradient_are_skipped(native_lib, counting):
    t = _Trio(13, SHAPES, CUTS3, HYPER3)
    g = torch.Generator().manual_seed(14)
    before = [q.detach().clone() for q in t.ours]
    skip = {1, 3, 4, 5}                                   # one parameter of group 0, all of group 1
    t.set_grads(g, 3.0, skip=skip)
    t.step(1.0)
    t.check(True, "skipped")
    for i in skip:
        assert torch.equal(t.ours[i].detach(), before[i]) and not t.o_ours.state[t.ours[i]]
    t.set_grads(g, 1.0)                                   # they join later: step 1 for group 1, and group 0 no longer shares one step count
    with pytest.raises(RuntimeError, match="share their step count"):
        t.o_ours.step()
    # every gradient None: a zero norm, and nothing is launched
    t.set_grads(g, 1.0, skip=set(range(len(SHAPES))))
    counting.clear()
    now = [q.detach().clone() for q in t.ours]
    tot = t.o_ours.clip_grad_norm_(1.0)
    t.o_ours.step()
    t.o_ours.step(max_norm=1.0)
    assert float(tot) == 0.0 and not counting
    assert all(torch.equal(q.detach(), b) for q, b in zip(t.ours, now))


# ---- 6
def test_state_dict_moves_both_ways_between_torch_and_native(native_lib):
    base = _params(15, SHAPES[:6])
    g = torch.Generator().manual_seed(16)

    def pair(first):
        """`first` takes a clipped step, the other kind of optimizer loads its state on copies of the parameters, both take one more step."""
        a = [torch.nn.Parameter(p.detach().clone().cuda()) for p in base]
        o_a = (ClipAdamW if first == "native" else lambda gs: torch.optim.AdamW(gs, foreach=False))(_split(a, [0, 2, 4, 6], HYPER3))
        for q in a:
            q.grad = (torch.randn(q.shape, generator=g) * 3.0).cuda()
        if first == "native":
            o_a.step(max_norm=1.0)
        else:
            torch.nn.utils.clip_grad_norm_(a, 1.0, foreach=False)
            o_a.step()
        sd = o_a.state_dict()
        assert len(sd["param_groups"]) == 3 and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
        b = [torch.nn.Parameter(q.detach().clone()) for q in a]
        o_b = (ClipAdamW if first == "stock" else lambda gs: torch.optim.AdamW(gs, foreach=False))(_split(b, [0, 2, 4, 6], HYPER3))
        o_b.load_state_dict(copy.deepcopy(sd))
        for q, r in zip(a, b):
            q.grad = torch.randn(q.shape, generator=g).cuda()
            r.grad = q.grad.clone()
        o_a.step()
        o_b.step()
        for i, (q, r) in enumerate(zip(a, b)):
            assert rel_l2(q.detach().cpu(), r.detach().cpu()) < 2e-6, (first, i)
            assert int(o_a.state[q]["step"]) == int(o_b.state[r]["step"]) == 2

    pair("native")
    pair("stock")


# ---- 7
def test_64_groups_work_and_65_raise_before_anything_is_touched(native_lib, counting):
    shapes = [(i + 1,) if i % 4 else (i + 1, 5) for i in range(MAX_GROUPS)]
    hyper = [dict(lr=1e-3 * (1 + i % 5), weight_decay=0.01 * (i % 3), betas=(0.9 - 0.01 * (i % 4), 0.999), eps=1e-8) for i in range(MAX_GROUPS)]
    t = _Trio(17, shapes, list(range(MAX_GROUPS + 1)), hyper)
    g = torch.Generator().manual_seed(18)
    for it in range(2):
        t.set_grads(g, SCALES[it])
        counting.clear()
        t.step(1.0)
        assert counting["qatvit_optim_adamw_groups"] == 1 and counting["qatvit_optim_adamw"] == 0
        t.check(True, it)
    extra = torch.nn.Parameter(torch.ones(3, device="cuda"))
    t.o_ours.add_param_group(dict(params=[extra]))
    for q in t.ours + [extra]:
        q.grad = torch.ones_like(q)
    params = [q.detach().clone() for q in t.ours + [extra]]
    state = {q: {k: v.clone() for k, v in t.o_ours.state[q].items()} for q in t.ours}
    counting.clear()
    for call in (lambda: t.o_ours.step(), lambda: t.o_ours.step(max_norm=1.0), lambda: t.o_ours.clip_grad_norm_(1.0)):
        with pytest.raises(RuntimeError, match=f"at most {MAX_GROUPS} groups"):
            call()
    assert not counting and not t.o_ours.state[extra]
    assert all(torch.equal(q.detach(), b) for q, b in zip(t.ours + [extra], params))
    for q in t.ours:
        assert set(t.o_ours.state[q]) == set(state[q]) and all(torch.equal(t.o_ours.state[q][k], v) for k, v in state[q].items())
    extra.grad = None                                     # 64 groups with gradients again: the step goes through
    t.o_ours.step(max_norm=1.0)
    assert all(int(t.o_ours.state[q]["step"]) == 3 for q in t.ours)


# ---- 8
def test_full_student_step_with_layer_decay_groups(native_lib):
    """End to end on the tiny student: native fwd+bwd, then the 8 groups of vit_param_groups through the native clip + AdamW == stock
    clip_grad_norm_ + AdamW built from the same groups on copies of the parameters and gradients."""
    from qat_vit_amd import functional as F
    from tests.util import prepare

    torch.manual_seed(0)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=128, depth=2, num_heads=2, img_size=32)
    model = prepare(stu.cuda(), "qnnpack")
    x, y = torch.randn(4, 3, 32, 32).cuda(), torch.randint(0, 10, (4,)).cuda()
    groups = vit_param_groups(model, 0.05, lr=1e-3, layer_decay=0.75)
    assert len(groups) == 8
    opt = ClipAdamW(groups)
    twin_of = {p: torch.nn.Parameter(p.detach().clone()) for p in model.parameters()}
    twin = list(twin_of.values())
    o_twin = torch.optim.AdamW([dict(params=[twin_of[p] for p in grp["params"]], lr=grp["lr"], weight_decay=grp["weight_decay"]) for grp in groups],
                               foreach=False)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss, _ = F.kd_ce_loss(model(x), None, y, 4.0, 0.5, 0.1)
        loss.backward()
        for p, t in twin_of.items():
            t.data.copy_(p.data)
            t.grad = p.grad.detach().clone()
        torch.nn.utils.clip_grad_norm_(twin, 1.0, foreach=False)
        o_twin.step()
        opt.step(max_norm=1.0)
        for (n, p), t in zip(model.named_parameters(), twin):
            assert rel_l2(p.detach().cpu(), t.detach().cpu()) < 2e-6, n
