"""The host-side fake-quant mode decision of the native step (engine.decide_fq_mode) on a CPU-prepared student: QAT with fake-quant on
everywhere, observe-only with it off everywhere, a mix refused by name; the flags are read only when torch.ao.quantization moved their version."""
import pytest
import torch
from torch.ao.quantization import disable_fake_quant, enable_fake_quant

import qat_vit_amd
from qat_vit_amd.engine import OBSERVE, QAT, FqModeState, decide_fq_mode, fq_flags_and_names, fq_modules_and_names

from util import prepare

TINY = dict(embed_dim=128, depth=2, num_heads=2, img_size=32)
BACKENDS = ["qnnpack", "x86"]


def _prepared(backend):
    torch.manual_seed(0)
    return prepare(qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **TINY), backend)


@pytest.mark.parametrize("backend", BACKENDS)
def test_all_on_all_off_and_mixed(backend):
    p = _prepared(backend)
    fqs, names = fq_modules_and_names(p)
    assert len(fqs) == (4 + 6 * 2) + (2 + 4 * 2) and len(set(names)) == len(names)
    fqs, _ = fq_flags_and_names(p)
    assert names[0] == "quant.activation_post_process" and names[-1] == "model.head.weight_fake_quant"
    st = FqModeState()
    assert decide_fq_mode(st, fqs, names) == QAT
    p.apply(disable_fake_quant)
    assert decide_fq_mode(st, fqs, names) == OBSERVE
    p.model.blocks[1].mlp.fc1.apply(enable_fake_quant)
    with pytest.raises(RuntimeError, match="only|everywhere") as e:
        decide_fq_mode(st, fqs, names)
    msg = str(e.value)
    assert "model.blocks.1.mlp.fc1.activation_post_process" in msg and "model.blocks.1.mlp.fc1.weight_fake_quant" in msg   # the enabled ones
    assert "quant.activation_post_process" in msg                                                                         # a disabled one
    assert "enabled on 2 modules" in msg and f"disabled on {len(fqs) - 2}" in msg
    assert st.mode == OBSERVE                 # a refused decision leaves the state as it was ...
    with pytest.raises(RuntimeError):         # ... and keeps refusing while the mix stands
        decide_fq_mode(st, fqs, names)
    p.apply(enable_fake_quant)
    assert decide_fq_mode(st, fqs, names) == QAT


@pytest.mark.parametrize("backend", BACKENDS)
def test_unchanged_versions_read_no_flag(backend):
    p = _prepared(backend)
    fqs, names = fq_flags_and_names(p)
    st = FqModeState()
    assert decide_fq_mode(st, fqs, names) == QAT and st.reads == 1
    for _ in range(3):
        assert decide_fq_mode(st, fqs, names) == QAT
    assert st.reads == 1
    # a write that does not go through the tensor's version counter is invisible to the decision: proof that no flag was read
    for t in fqs:
        t.data[0] = 0
    assert decide_fq_mode(st, fqs, names) == QAT and st.reads == 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_disable_after_a_decision_is_seen_on_the_next(backend):
    p = _prepared(backend)
    fqs, names = fq_flags_and_names(p)
    st = FqModeState()
    assert decide_fq_mode(st, fqs, names) == QAT
    v0 = fqs[0]._version
    p.apply(disable_fake_quant)
    assert fqs[0]._version > v0
    assert decide_fq_mode(st, fqs, names) == OBSERVE and st.reads == 2
    assert decide_fq_mode(st, fqs, names) == OBSERVE and st.reads == 2
    p.apply(enable_fake_quant)
    assert decide_fq_mode(st, fqs, names) == QAT and st.reads == 3


def test_observe_symbols_and_buffer_size_without_a_gpu(native_lib):
    import ctypes
    import os
    import re
    import subprocess

    from qat_vit_amd import native

    syms = {"qatvit_float_student_observe_bytes", "qatvit_float_student_observe_init", "qatvit_float_student_forward_observe"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "qatvit.h")).read(), flags=re.S)
    assert syms <= set(re.findall(r"\b(qatvit_[a-z0-9_]+)\s*\(", hdr)) and syms <= set(native.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert syms <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert native_lib.qatvit_abi_version() == 4

    def cfg(**kw):
        c = dict(batch=8, img_size=224, patch_size=16, in_chans=3, embed_dim=384, depth=12, num_heads=6, mlp_hidden=1536, num_classes=10,
                 act_qmin=0, act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, ln_eps=1e-6)
        c.update(kw)
        return native.Cfg(**c)

    ob = native_lib.qatvit_float_student_observe_bytes
    n8, n256 = ob(ctypes.byref(cfg())), ob(ctypes.byref(cfg(batch=256)))
    assert 0 < n8 == n256                                   # batch independent
    assert ob(ctypes.byref(cfg(w_per_channel=1))) > n8 > ob(ctypes.byref(cfg(depth=2)))
    assert ob(ctypes.byref(cfg(num_heads=4))) == -1 and b"float student: unsupported config" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_forward_observe(None, None, None, None, None, None, None) != 0
    assert b"null argument" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_float_student_observe_init(None, None, None, None, None) != 0
