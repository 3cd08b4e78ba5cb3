"""CPU-side checks of the LAMB entries (qatvit_optim_lamb_moments / qatvit_optim_lamb_apply): the two symbols in the library, the header and
native.py, every argument error as a string without a HIP call, what ClipLamb decides on the host - and the reference of the GPU tests itself:
tests/lamb_ref.py against stock ``torch.optim.Adam`` in fp64 where both are the same expression, and its trust rules on hand-made tensors."""
import math
import os
import re
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.optim import MAX_GROUPS, ClipAdamW, ClipLamb
from tests.lamb_ref import lamb_ref
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"qatvit_optim_lamb_moments": 15, "qatvit_optim_lamb_apply": 17}
P = 4096   # a non-null stand-in; never dereferenced on these paths (each call returns before any HIP call)
GOOD = (1e-3, 0.9, 0.999, 1e-6, 0.01, 1, 1, 0, 0, 0)
BAD_CHUNKING = (dict(n_chunks=0), dict(n_chunks=-3), dict(chunk=0), dict(chunk=-4), dict(chunk=16382))
BAD_ROWS = ((dict(step=0), b"step=0"), (dict(lr=-1e-3), b"lr=-0.001"), (dict(b1=1.0), b"betas=(1, 0.999)"), (dict(b2=1.0), b"betas=(0.9, 1)"),
            (dict(b1=-0.1), b"betas=(-0.1"), (dict(b2=-0.5), b"betas=(0.9, -0.5)"), (dict(eps=-1e-8), b"eps=-1e-08"), (dict(wd=-0.01), b"weight_decay=-0.01"),
            (dict(lr=math.nan), b"lr=nan"))


def _row(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, step=1):
    return (lr, b1, b2, eps, wd, step, 1, 0, 0, 0)


def _moments(L, rows=(GOOD, GOOD), n_groups=None, n_chunks=3, chunk=16384, **null):
    groups = (native.LambGroup * max(len(rows), 1))(*rows)
    a = dict(params=P, grads=P, m=P, v=P, numel=P, tg=P, ct=P, ci=P, groups=groups, partials=P)
    a.update(null)
    return L.qatvit_optim_lamb_moments(a["params"], a["grads"], a["m"], a["v"], a["numel"], a["tg"], a["ct"], a["ci"], n_chunks, chunk, a["groups"],
                                       len(rows) if n_groups is None else n_groups, None, a["partials"], None)


def _apply(L, rows=(GOOD, GOOD), n_groups=None, n_chunks=3, chunk=16384, decay=0.99, ema=P, **null):
    groups = (native.LambGroup * max(len(rows), 1))(*rows)
    a = dict(params=P, m=P, v=P, numel=P, tg=P, first=P, ct=P, ci=P, groups=groups, partials=P)
    a.update(null)
    return L.qatvit_optim_lamb_apply(a["params"], a["m"], a["v"], ema, a["numel"], a["tg"], a["first"], a["ct"], a["ci"], n_chunks, chunk, a["groups"],
                                     len(rows) if n_groups is None else n_groups, decay, a["partials"], None, None)


ENTRIES = {"qatvit_optim_lamb_moments": (_moments, ("params", "grads", "m", "v", "numel", "tg", "ct", "ci", "groups", "partials")),
           "qatvit_optim_lamb_apply": (_apply, ("params", "m", "v", "numel", "tg", "first", "ct", "ci", "groups", "partials"))}


def test_symbols_in_exports_signatures_and_header(native_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    text = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(qatvit_[a-z0-9_]+)\s*\(([^)]*)\)", hdr)}
    for name, arity in ARITY.items():
        assert name in exported, name
        assert name in native.SIGNATURES and len(native.SIGNATURES[name][1]) == arity, name
        assert name in declared and len(declared[name].split(",")) == arity, name
        args = [a.split()[-1].lstrip("*") for a in declared[name].split(",")]
        assert args[args.index("n_groups") - 1] == "groups" and args[-1] == "stream", (name, args)
    args = [a.split()[-1].lstrip("*") for a in declared["qatvit_optim_lamb_apply"].split(",")]
    assert native.SIGNATURES["qatvit_optim_lamb_apply"][1][args.index("ema_decay")] is native.c_double
    assert {"ema_ptrs", "tensor_first_chunk", "trust_out", "partials2"} <= set(args) and "grad_ptrs" not in args
    assert not any(n.startswith("qatvit_optim_lamb") for n in exported - set(ARITY))      # no separate one-group entries
    assert native_lib.qatvit_abi_version() == 4                                           # added symbols: the version stays
    # struct qatvit_lamb_group as the header lays it out, and QATVIT_OPTIM_MAX_GROUPS as Python knows it
    assert [n for n, _ in native.LambGroup._fields_] == re.search(r"typedef struct qatvit_lamb_group \{(.*?)\}", hdr, re.S).group(1).replace(
        "double", "").replace("int64_t", "").replace("int32_t", "").replace(";", ",").replace(" ", "").replace("\n", "").strip(",").split(",")
    import ctypes
    assert ctypes.sizeof(native.LambGroup) == 64 and int(re.search(r"#define QATVIT_OPTIM_MAX_GROUPS (\d+)", text).group(1)) == MAX_GROUPS == ClipLamb.MAX_GROUPS
    # the arithmetic is stated in the header comment
    for line in ("m   <- b1 * m + (1 - b1) * g", "v   <- b2 * v + (1 - b2) * g * g", "r    = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd * p",
                 "trust = ||p||_2 / ||r||_2  if (wd != 0 or always_adapt) and ||p|| > 0 and ||r|| > 0, else 1", "p   <- p - lr * trust * r"):
        assert line in text, line


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_argument_errors(native_lib, name):
    L = native_lib
    call, tables = ENTRIES[name]
    tag = name.encode()
    for ptr in tables:
        assert call(L, **{ptr: None}) != 0 and tag + b": null pointer" in L.qatvit_last_error(), ptr
    for kw in BAD_CHUNKING:
        assert call(L, **kw) != 0 and tag + b": bad chunking" in L.qatvit_last_error(), kw
    assert call(L, n_groups=0) != 0 and tag + b": n_groups 0 outside [1, 64]" in L.qatvit_last_error()
    assert call(L, rows=(GOOD,) * 65) != 0 and tag + b": n_groups 65 outside [1, 64]" in L.qatvit_last_error()
    assert call(L, n_groups=-1) != 0 and b"n_groups -1" in L.qatvit_last_error()
    for kw, what in BAD_ROWS:
        assert call(L, rows=(GOOD, _row(**kw))) != 0, kw
        msg = L.qatvit_last_error()
        assert tag + b": bad hyper-parameters in group 1" in msg and what in msg, msg
        assert call(L, rows=(_row(**kw), GOOD)) != 0 and b"in group 0" in L.qatvit_last_error(), kw


def test_apply_checks_the_decay_only_with_averages(native_lib):
    L = native_lib
    for decay, what in ((-0.1, b"ema_decay -0.1 outside [0, 1)"), (1.0, b"ema_decay 1 outside [0, 1)"), (math.nan, b"outside [0, 1)")):
        assert _apply(L, decay=decay) != 0, decay
        msg = L.qatvit_last_error()
        assert b"qatvit_optim_lamb_apply: ema_decay" in msg and what in msg, msg
    # every earlier rule still comes first with a bad decay
    assert _apply(L, decay=2.0, params=None) != 0 and b"null pointer" in L.qatvit_last_error()
    assert _apply(L, decay=2.0, rows=(_row(step=0),)) != 0 and b"bad hyper-parameters in group 0" in L.qatvit_last_error()


def test_optional_arguments_are_nullable(native_lib):
    """trust_out, clip_out2 and ema_ptrs may be null (and ema_decay is then not looked at): with all three null the error names something else.
    (No call here or above has valid arguments throughout: it would launch.)"""
    L = native_lib
    assert _apply(L, ema=None, decay=math.nan, n_chunks=0) != 0 and b"bad chunking" in L.qatvit_last_error()
    assert _moments(L, n_chunks=0) != 0 and b"bad chunking" in L.qatvit_last_error()


def test_constructor_validation():
    p = [torch.nn.Parameter(torch.zeros(8))]
    opt = ClipLamb(p)
    assert opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_averaging=True, always_adapt=False, trust_clip=False)
    assert opt.ema_decay is None and opt.ema_swapped is False and opt.trust_ratios() is None
    assert "ema_decay" not in opt.param_groups[0] and ClipLamb.MAX_GROUPS == ClipAdamW.MAX_GROUPS
    for bad in (dict(lr=-1e-3), dict(eps=-1e-6), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError, match="invalid LAMB hyper-parameters"):
            ClipLamb(p, **bad)
    for bad in (1.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match=r"ClipLamb: ema_decay .* outside \[0, 1\)"):
            ClipLamb(p, ema_decay=bad)
        with pytest.raises(ValueError, match="ClipLamb: ema_decay"):
            opt.ema_decay = bad
    opt.ema_decay = 0.5
    assert opt.ema_decay == 0.5
    groups = ClipLamb([dict(params=p, weight_decay=0.0, always_adapt=True)], lr=2e-3, trust_clip=True).param_groups
    assert groups[0]["always_adapt"] is True and groups[0]["trust_clip"] is True and groups[0]["lr"] == 2e-3 and groups[0]["grad_averaging"] is True
    assert "ClipLamb" in qat_vit_amd.__all__ and qat_vit_amd.ClipLamb is ClipLamb


def test_cpu_parameters_are_refused_before_any_state():
    a, b = torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(3))
    a.grad, b.grad = torch.ones(8), torch.ones(3)
    for kw in (dict(), dict(ema_decay=0.99)):
        opt = ClipLamb([dict(params=[a]), dict(params=[b], lr=1e-2, weight_decay=0.0)], **kw)
        for call in (lambda: opt.clip_grad_norm_(1.0), lambda: opt.step(), lambda: opt.step(max_norm=1.0)):
            with pytest.raises(RuntimeError, match="ClipLamb runs on MI355X only"):
                call()
        assert not opt.state and torch.equal(a.detach(), torch.zeros(8)) and opt.trust_ratios() is None


def test_clipadamw_keeps_its_texts_and_groups():
    """The shared base must not show in ClipAdamW: its messages carry its own name, its groups are torch.optim.AdamW's."""
    a = torch.nn.Parameter(torch.zeros(8))
    a.grad = torch.ones(8)
    opt = ClipAdamW([a])
    assert set(opt.param_groups[0]) - {"params"} == {"lr", "betas", "eps", "weight_decay"} and not hasattr(opt, "trust_ratios")
    with pytest.raises(RuntimeError, match="^ClipAdamW runs on MI355X only: parameters must be contiguous fp32 CUDA tensors$"):
        opt.step()
    with pytest.raises(ValueError, match=r"^ClipAdamW: ema_decay 1.0 outside \[0, 1\)$"):
        ClipAdamW([a], ema_decay=1.0)
    with pytest.raises(ValueError, match="^invalid AdamW hyper-parameters$"):
        ClipAdamW([a], lr=-1.0)


# ---- the reference itself
def test_reference_is_stock_adam_where_trust_is_one():
    """weight_decay = 0 without always_adapt and without a clip: trust == 1, and the step is Adam's (bias-corrected moments, eps added to the
    corrected denominator).  Stock fp64 Adam writes the same expression with a lerp and an addcdiv: equal to a few roundings of double."""
    g = torch.Generator().manual_seed(5)
    shapes, lr, betas, eps = [(1,), (7,), (33, 5), (1000,)], 3e-3, (0.9, 0.999), 1e-6
    ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).double()) for s in shapes]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps, weight_decay=0, foreach=False)
    mine = [(p.detach().float(), torch.zeros(s), torch.zeros(s)) for p, s in zip(ps, shapes)]
    for step in range(1, 6):
        grads = [torch.randn(s, generator=g) * (0.01 if step % 2 else 3.0) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.double()
        opt.step()
        nxt = []
        for (p, m, v), gr in zip(mine, grads):
            p, m, v, trust = lamb_ref(p, gr, m, v, step=step, lr=lr, betas=betas, eps=eps, weight_decay=0.0)
            assert trust == 1.0 and p.dtype == m.dtype == v.dtype == torch.float64
            nxt.append((p, m, v))
        mine = nxt
        for i, (q, (p, m, v)) in enumerate(zip(ps, mine)):
            st = opt.state[q]
            assert rel_l2(p, q.detach()) <= 1e-15 and rel_l2(m, st["exp_avg"]) <= 1e-15 and rel_l2(v, st["exp_avg_sq"]) <= 1e-15, (step, i)


def test_reference_trust_rules():
    z = torch.zeros(4)
    kw = dict(step=1, lr=0.1, betas=(0.9, 0.999), eps=0.0)
    p, g = torch.tensor([3.0, 0.0, 0.0, 4.0]), torch.tensor([1.0, -1.0, 1.0, -1.0])
    # step 1, eps 0: m-hat / sqrt(v-hat) = sign(g), so ||r|| = 2 without decay and ||p|| = 5
    new, m, v, trust = lamb_ref(p, g, z, z, weight_decay=0.0, always_adapt=True, **kw)
    assert trust == pytest.approx(2.5, rel=1e-12) and torch.allclose(new, p.double() - 0.25 * g.double(), rtol=1e-12, atol=0)
    assert torch.allclose(m, 0.1 * g.double(), rtol=1e-12, atol=0) and torch.allclose(v, 0.001 * torch.ones(4, dtype=torch.float64), rtol=1e-9, atol=0)
    # no decay and no always_adapt: 1, whatever the norms
    assert lamb_ref(p, g, z, z, weight_decay=0.0, **kw)[3] == 1.0
    # trust_clip caps at 1 and leaves a smaller ratio alone
    assert lamb_ref(p, g, z, z, weight_decay=0.0, always_adapt=True, trust_clip=True, **kw)[3] == 1.0
    small = lamb_ref(p * 0.1, g, z, z, weight_decay=0.0, always_adapt=True, trust_clip=True, **kw)[3]
    assert small == pytest.approx(0.25, rel=1e-6) and small == lamb_ref(p * 0.1, g, z, z, weight_decay=0.0, always_adapt=True, **kw)[3]
    # ||p|| == 0 with decay: 1, and the update is the plain one
    new, _, _, trust = lamb_ref(z, g, z, z, weight_decay=0.05, **kw)
    assert trust == 1.0 and torch.allclose(new, -0.1 * g.double(), rtol=1e-12, atol=0)
    # ||r|| == 0 (no gradient signal, no moments; the decay term vanishes with p = 0 only, so take wd * p = 0 through always_adapt): 1
    new, _, _, trust = lamb_ref(p, z, z, z, weight_decay=0.0, always_adapt=True, step=1, lr=0.1, betas=(0.9, 0.999), eps=1e-6)
    assert trust == 1.0 and torch.equal(new, p.double())
    # the ratio uses the weight BEFORE the update and the decay term inside r
    new, _, _, trust = lamb_ref(p, g, z, z, weight_decay=0.5, **kw)
    r = g.double() + 0.5 * p.double()
    assert trust == pytest.approx(5.0 / r.norm().item(), rel=1e-12) and torch.allclose(new, p.double() - 0.1 * trust * r, rtol=1e-12, atol=0)
    # grad_averaging=False: m <- b1 * m + g; the clip coefficient scales g first
    _, m, v, _ = lamb_ref(p, g, torch.ones(4), z, weight_decay=0.0, grad_averaging=False, coef=0.5, **kw)
    assert torch.allclose(m, 0.9 + 0.5 * g.double(), rtol=1e-12, atol=0) and torch.allclose(v, torch.full((4,), 0.001 * 0.25, dtype=torch.float64), rtol=1e-9, atol=0)
