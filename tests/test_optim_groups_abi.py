"""CPU-side checks of the grouped AdamW entry: the new symbol in the library, the header and native.py, every argument error as a string without a
HIP call, and the refusal of CPU parameters by a two-group ClipAdamW."""
import ctypes
import os
import re
import struct
import subprocess

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.optim import MAX_GROUPS, ClipAdamW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "qatvit_optim_adamw_groups"


def test_symbol_in_exports_signatures_and_header(native_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert SYMBOL in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert SYMBOL in native.SIGNATURES and len(native.SIGNATURES[SYMBOL][1]) == 14
    assert native_lib.qatvit_abi_version() == 4        # an added symbol: the version the other ABI tests pin stays
    text = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert SYMBOL in set(re.findall(r"\b(qatvit_[a-z0-9_]+)\s*\(", hdr))
    assert f"#define QATVIT_OPTIM_MAX_GROUPS {MAX_GROUPS}" in hdr and MAX_GROUPS == 64
    # the ctypes record is the header's: five doubles, then the int64 step
    m = re.search(r"typedef struct qatvit_adamw_group \{(.*?)\} qatvit_adamw_group;", hdr, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "double lr, beta1, beta2, eps, weight_decay; int64_t step;"
    assert [n for n, _ in native.AdamWGroup._fields_] == ["lr", "beta1", "beta2", "eps", "weight_decay", "step"]
    assert ctypes.sizeof(native.AdamWGroup) == 48 == struct.calcsize("=5dq")      # ClipAdamW packs its rows with this format


def test_argument_errors_are_strings_without_a_gpu(native_lib):
    L = native_lib
    p = 4096   # a non-null stand-in; never dereferenced on these paths (each call returns before any HIP call)
    good = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1)

    def call(rows=(good, good), n_groups=None, n_chunks=3, chunk=16384, **null):
        groups = (native.AdamWGroup * max(len(rows), 1))(*rows)
        a = dict(params=p, grads=p, m=p, v=p, numel=p, tg=p, ct=p, ci=p, groups=groups)
        a.update(null)
        return L.qatvit_optim_adamw_groups(a["params"], a["grads"], a["m"], a["v"], a["numel"], a["tg"], a["ct"], a["ci"], n_chunks, chunk, a["groups"],
                                           len(rows) if n_groups is None else n_groups, None, None)

    for name in ("params", "grads", "m", "v", "numel", "tg", "ct", "ci", "groups"):
        assert call(**{name: None}) != 0 and b"qatvit_optim_adamw_groups: null pointer" in L.qatvit_last_error(), name
    assert call(n_groups=0) != 0 and b"n_groups 0 outside [1, 64]" in L.qatvit_last_error()
    assert call(rows=(good,) * 65) != 0 and b"n_groups 65 outside [1, 64]" in L.qatvit_last_error()
    assert call(n_groups=-1) != 0 and b"n_groups -1" in L.qatvit_last_error()
    for bad, what in (((1e-3, 0.9, 0.999, 1e-8, 0.01, 0), b"step=0"), ((-1e-3, 0.9, 0.999, 1e-8, 0.01, 1), b"lr=-0.001"),
                      ((1e-3, 1.0, 0.999, 1e-8, 0.01, 1), b"betas=(1, 0.999)"), ((1e-3, 0.9, 1.0, 1e-8, 0.01, 1), b"betas=(0.9, 1)"),
                      ((1e-3, -0.1, 0.999, 1e-8, 0.01, 1), b"betas=(-0.1"), ((1e-3, 0.9, 0.999, -1e-8, 0.01, 1), b"eps=-1e-08"),
                      ((1e-3, 0.9, 0.999, 1e-8, -0.01, 1), b"weight_decay=-0.01")):
        assert call(rows=(good, bad)) != 0, what
        msg = L.qatvit_last_error()
        assert b"bad hyper-parameters in group 1" in msg and what in msg, msg
        assert call(rows=(bad, good)) != 0 and b"in group 0" in L.qatvit_last_error()
    for kw in (dict(n_chunks=0), dict(n_chunks=-3), dict(chunk=0), dict(chunk=16382)):
        assert call(**kw) != 0 and b"qatvit_optim_adamw_groups: bad chunking" in L.qatvit_last_error(), kw


def test_cpu_parameters_in_two_groups_are_refused():
    a, b = torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(3))
    a.grad, b.grad = torch.ones(8), torch.ones(3)
    opt = ClipAdamW([dict(params=[a]), dict(params=[b], lr=1e-2, weight_decay=0.0)])
    with pytest.raises(RuntimeError, match="MI355X only"):
        opt.clip_grad_norm_(1.0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        opt.step()
    with pytest.raises(RuntimeError, match="MI355X only"):
        opt.step(max_norm=1.0)
    assert not opt.state and torch.equal(a.detach(), torch.zeros(8))       # refused before anything was touched


def test_names_are_exported():
    assert "vit_param_groups" in qat_vit_amd.__all__ and callable(qat_vit_amd.vit_param_groups)
