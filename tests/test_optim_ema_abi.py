"""CPU-side checks of the weight-EMA entries of the optimizer: the four symbols in the library, the header and native.py, every argument error as a
string without a HIP call, and what ClipAdamW / ema_warmup_decay decide on the host."""
import math
import os
import re
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.optim import ClipAdamW, ema_warmup_decay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"qatvit_optim_adamw_ema": 19, "qatvit_optim_adamw_groups_ema": 16, "qatvit_optim_ema": 9, "qatvit_optim_swap": 8}
P = 4096   # a non-null stand-in; never dereferenced on these paths (each call returns before any HIP call)
GOOD = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1)
BAD_DECAYS = ((-0.1, b"ema_decay -0.1 outside [0, 1)"), (1.0, b"ema_decay 1 outside [0, 1)"), (math.nan, b"outside [0, 1)"))
BAD_CHUNKING = (dict(n_chunks=0), dict(n_chunks=-3), dict(chunk=0), dict(chunk=16382))


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
    # ema_ptrs follows exp_avg_sq_ptrs, ema_decay follows step (one group) / n_groups (the groups' steps are in their rows)
    for name, after_decay in (("qatvit_optim_adamw_ema", "step"), ("qatvit_optim_adamw_groups_ema", "n_groups")):
        args = [a.split()[-1].lstrip("*") for a in declared[name].split(",")]
        assert args[args.index("exp_avg_sq_ptrs") + 1] == "ema_ptrs" and args[args.index(after_decay) + 1] == "ema_decay", (name, args)
        assert native.SIGNATURES[name][1][args.index("ema_decay")] is native.c_double
    assert native_lib.qatvit_abi_version() == 4        # added symbols: the version the other ABI tests pin stays
    assert "e' = (w < 0.5f) ? e + w * d : p' - d * (1.0f - w)" in text   # the arithmetic is stated in the header comment


def _decay_and_chunking(L, name, call):
    for decay, what in BAD_DECAYS:
        assert call(decay=decay) != 0, (name, decay)
        msg = L.qatvit_last_error()
        assert name.encode() + b": ema_decay" in msg and what in msg, msg
    for kw in BAD_CHUNKING:
        assert call(**kw) != 0 and name.encode() + b": bad chunking" in L.qatvit_last_error(), (name, kw)


def test_adamw_ema_argument_errors(native_lib):
    L, name = native_lib, "qatvit_optim_adamw_ema"

    def call(hyper=GOOD, decay=0.999, n_chunks=3, chunk=16384, **null):
        a = dict(params=P, grads=P, m=P, v=P, ema=P, numel=P, ct=P, ci=P)
        a.update(null)
        lr, b1, b2, eps, wd, step = hyper
        return L.qatvit_optim_adamw_ema(a["params"], a["grads"], a["m"], a["v"], a["ema"], a["numel"], a["ct"], a["ci"], n_chunks, chunk, lr, b1, b2, eps,
                                        wd, step, decay, None, None)

    for ptr in ("params", "grads", "m", "v", "ema", "numel", "ct", "ci"):
        assert call(**{ptr: None}) != 0 and b"qatvit_optim_adamw_ema: null pointer" in L.qatvit_last_error(), ptr
    _decay_and_chunking(L, name, call)
    # the hyper-parameter errors of qatvit_optim_adamw
    for bad, what in (((1e-3, 0.9, 0.999, 1e-8, 0.01, 0), b"step=0"), ((-1e-3, 0.9, 0.999, 1e-8, 0.01, 1), b"lr=-0.001"),
                      ((1e-3, 1.0, 0.999, 1e-8, 0.01, 1), b"betas=(1, 0.999)"), ((1e-3, 0.9, 1.0, 1e-8, 0.01, 1), b"betas=(0.9, 1)"),
                      ((1e-3, -0.1, 0.999, 1e-8, 0.01, 1), b"betas=(-0.1"), ((1e-3, 0.9, 0.999, -1e-8, 0.01, 1), b"eps=-1e-08")):
        assert call(hyper=bad) != 0, what
        msg = L.qatvit_last_error()
        assert b"qatvit_optim_adamw_ema: bad hyper-parameters" in msg and what in msg, msg


def test_adamw_groups_ema_argument_errors(native_lib):
    L, name = native_lib, "qatvit_optim_adamw_groups_ema"

    def call(rows=(GOOD, GOOD), n_groups=None, decay=0.999, n_chunks=3, chunk=16384, **null):
        groups = (native.AdamWGroup * max(len(rows), 1))(*rows)
        a = dict(params=P, grads=P, m=P, v=P, ema=P, numel=P, tg=P, ct=P, ci=P, groups=groups)
        a.update(null)
        return L.qatvit_optim_adamw_groups_ema(a["params"], a["grads"], a["m"], a["v"], a["ema"], a["numel"], a["tg"], a["ct"], a["ci"], n_chunks, chunk,
                                               a["groups"], len(rows) if n_groups is None else n_groups, decay, None, None)

    for ptr in ("params", "grads", "m", "v", "ema", "numel", "tg", "ct", "ci", "groups"):
        assert call(**{ptr: None}) != 0 and b"qatvit_optim_adamw_groups_ema: null pointer" in L.qatvit_last_error(), ptr
    _decay_and_chunking(L, name, call)
    # the errors of qatvit_optim_adamw_groups
    assert call(n_groups=0) != 0 and b"qatvit_optim_adamw_groups_ema: n_groups 0 outside [1, 64]" in L.qatvit_last_error()
    assert call(rows=(GOOD,) * 65) != 0 and b"n_groups 65 outside [1, 64]" in L.qatvit_last_error()
    assert call(n_groups=-1) != 0 and b"n_groups -1" in L.qatvit_last_error()
    for bad, what in (((1e-3, 0.9, 0.999, 1e-8, 0.01, 0), b"step=0"), ((-1e-3, 0.9, 0.999, 1e-8, 0.01, 1), b"lr=-0.001"),
                      ((1e-3, 1.0, 0.999, 1e-8, 0.01, 1), b"betas=(1, 0.999)"), ((1e-3, 0.9, 1.0, 1e-8, 0.01, 1), b"betas=(0.9, 1)"),
                      ((1e-3, -0.1, 0.999, 1e-8, 0.01, 1), b"betas=(-0.1"), ((1e-3, 0.9, 0.999, -1e-8, 0.01, 1), b"eps=-1e-08"),
                      ((1e-3, 0.9, 0.999, 1e-8, -0.01, 1), b"weight_decay=-0.01")):
        assert call(rows=(GOOD, bad)) != 0, what
        msg = L.qatvit_last_error()
        assert b"qatvit_optim_adamw_groups_ema: bad hyper-parameters in group 1" in msg and what in msg, msg
        assert call(rows=(bad, GOOD)) != 0 and b"in group 0" in L.qatvit_last_error()


def test_ema_and_swap_argument_errors(native_lib):
    L = native_lib

    def ema(decay=0.999, n_chunks=3, chunk=16384, **null):
        a = dict(params=P, ema=P, numel=P, ct=P, ci=P)
        a.update(null)
        return L.qatvit_optim_ema(a["params"], a["ema"], a["numel"], a["ct"], a["ci"], n_chunks, chunk, decay, None)

    def swap(n_chunks=3, chunk=16384, **null):
        a = dict(a=P, b=P, numel=P, ct=P, ci=P)
        a.update(null)
        return L.qatvit_optim_swap(a["a"], a["b"], a["numel"], a["ct"], a["ci"], n_chunks, chunk, None)

    for ptr in ("params", "ema", "numel", "ct", "ci"):
        assert ema(**{ptr: None}) != 0 and b"qatvit_optim_ema: null pointer" in L.qatvit_last_error(), ptr
    _decay_and_chunking(L, "qatvit_optim_ema", ema)
    for ptr in ("a", "b", "numel", "ct", "ci"):
        assert swap(**{ptr: None}) != 0 and b"qatvit_optim_swap: null pointer" in L.qatvit_last_error(), ptr
    for kw in BAD_CHUNKING:
        assert swap(**kw) != 0 and b"qatvit_optim_swap: bad chunking" in L.qatvit_last_error(), kw


def test_constructor_and_property_validate_the_decay():
    p = [torch.nn.Parameter(torch.zeros(8))]
    assert ClipAdamW(p).ema_decay is None                       # the default: no average
    opt = ClipAdamW(p, ema_decay=0.9998)
    assert opt.ema_decay == 0.9998 and opt.ema_swapped is False
    assert "ema_decay" not in opt.param_groups[0]               # the groups of state_dict() stay torch.optim.AdamW's
    for bad in (1.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="ema_decay"):
            ClipAdamW(p, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            opt.ema_decay = bad
        assert opt.ema_decay == 0.9998
    opt.ema_decay = 0.0
    assert opt.ema_decay == 0.0
    opt.ema_decay = None
    assert opt.ema_decay is None


def test_cpu_parameters_are_refused_with_ema_before_any_state():
    a, b = torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(3))
    a.grad, b.grad = torch.ones(8), torch.ones(3)
    for groups in ([a, b], [dict(params=[a]), dict(params=[b], lr=1e-2, weight_decay=0.0)]):
        opt = ClipAdamW(groups, ema_decay=0.99)
        for call in (lambda: opt.clip_grad_norm_(1.0), lambda: opt.step(), lambda: opt.step(max_norm=1.0)):
            with pytest.raises(RuntimeError, match="MI355X only"):
                call()
        assert not opt.state and torch.equal(a.detach(), torch.zeros(8))
        # without state every parameter is its own average
        assert all(e is p for es, g in zip(opt.ema_parameters(), opt.param_groups) for e, p in zip(es, g["params"]))


def test_ema_warmup_decay():
    assert ema_warmup_decay(0.9999, 0) == 0.1
    assert ema_warmup_decay(0.9999, 1) == 2 / 11
    assert ema_warmup_decay(0.9999, 10 ** 6) == 0.9999
    assert ema_warmup_decay(0.05, 0) == 0.05


def test_names_are_exported():
    assert "ema_warmup_decay" in qat_vit_amd.__all__ and qat_vit_amd.ema_warmup_decay is ema_warmup_decay
    assert "ClipAdamW" in qat_vit_amd.__all__
