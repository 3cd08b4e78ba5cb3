"""Stochastic depth (drop-path) on the host: the module tree (qat_vit_amd.DropPath, ``drop_path_rate``, ``forced_drop_path``), what ``prepare_qat`` makes of
it, and the two C entries that hand a scale table to a workspace (include/qatvit.h) - without a GPU.  The native steps: tests/test_gpu_drop_path.py."""
import copy
import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.vit import DropPath, drop_path_branches, drop_path_plan
from tests.util import fq_modules, prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(embed_dim=128, depth=3, num_heads=2, img_size=32)
SYMBOLS = ("qatvit_student_set_drop_path", "qatvit_float_student_set_drop_path")


def _student(rate, **kw):
    torch.manual_seed(0)
    return qat_vit_amd.create_student("vit", qat_wrapper=True, drop_path_rate=rate, **{**TINY, **kw})


def test_create_student_takes_drop_path_rate_and_follows_linspace():
    m = qat_vit_amd.create_student("vit", drop_path_rate=0.1)                      # the call the reference makes through timm
    want = torch.linspace(0, 0.1, 12)
    for i, b in enumerate(m.blocks):
        assert isinstance(b.drop_path1, DropPath) and isinstance(b.drop_path2, DropPath)
        assert b.drop_path1.drop_prob == b.drop_path2.drop_prob == pytest.approx(want[i].item(), abs=1e-7)
        assert isinstance(b.ls1, nn.Identity) and isinstance(b.ls2, nn.Identity)
    assert m.blocks[0].drop_path1.drop_prob == 0.0 and m.blocks[-1].drop_path1.drop_prob == pytest.approx(0.1)
    for make in (qat_vit_amd.create_model, ):                                      # ... and through create_model / the wrapper
        w = make("vit_small_patch16_224_student", pretrained=False, qat_wrapper=True, drop_path_rate=0.2, depth=2)
        assert [b.drop_path1.drop_prob for b in w.model.blocks] == pytest.approx([0.0, 0.2])
    with pytest.raises(ValueError, match="drop_path_rate"):
        qat_vit_amd.create_student("vit", drop_path_rate=1.0, depth=2)


def test_rate_zero_is_the_tree_as_it_was():
    a, b = _student(0.0), _student(0.3)
    for blk in a.model.blocks:
        assert type(blk.drop_path1) is nn.Identity and type(blk.drop_path2) is nn.Identity
    assert drop_path_plan(a.model) is None
    assert list(a.state_dict()) == list(b.state_dict())                            # DropPath has no parameter and no buffer
    assert list(copy.deepcopy(b).state_dict()) == list(b.state_dict())
    keep, mult = drop_path_plan(b.model)
    assert keep == pytest.approx([1.0, 1.0, 0.85, 0.85, 0.7, 0.7]) and mult == pytest.approx([1 / k for k in keep])


def test_eval_is_the_identity_and_train_is_x_times_the_mask_it_drew():
    d = DropPath(0.4)
    x = torch.randn(64, 5, 8)
    assert d.eval()(x) is x
    assert DropPath(0.0).train()(x) is x
    d.train()
    torch.manual_seed(7)
    y = d(x)
    torch.manual_seed(7)
    m = x.new_empty(64, 1, 1).bernoulli_(0.6).div_(0.6)                             # timm's draw
    assert torch.equal(y, x * m)
    assert 0 < int((m == 0).sum()) < 64
    torch.manual_seed(7)
    assert torch.equal(DropPath(0.4, scale_by_keep=False).train()(x), x * (m != 0))


def test_forced_drop_path_makes_the_stock_forward_the_written_composition():
    w = _student(0.3).train()
    B, depth = 3, TINY["depth"]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, 32, 32, generator=g)
    table = torch.tensor([0.0, 0.5, 1.25, 2.0])[torch.randint(0, 4, (2 * depth, B), generator=g)]
    with qat_vit_amd.forced_drop_path(w, table):
        out1, out2 = w(x), w(x)
    assert torch.equal(out1, out2)                                                  # nothing is drawn
    m = w.model
    h = m.patch_embed(x)
    h = torch.cat([m.cls_token.expand(B, -1, -1), h], dim=1) + m.pos_embed
    for i, blk in enumerate(m.blocks):
        h = h + blk.attn(blk.norm1(h)) * table[2 * i].view(B, 1, 1)
        h = h + blk.mlp(blk.norm2(h)) * table[2 * i + 1].view(B, 1, 1)
    want = m.head(m.norm(h)[:, 0])
    assert torch.equal(out1, want)
    assert all(b._forced is None for b in drop_path_branches(m))                    # the context is over: the modules draw again
    assert not torch.equal(w(x), w(x))
    assert torch.equal(w.eval()(x), w(x))                                           # eval: no mask at all
    with qat_vit_amd.forced_drop_path(w, table):                                    # ... also inside the context
        assert torch.equal(w(x), _plain(m, x))
    w.train()
    with pytest.raises(ValueError, match=r"\[6, B\]"):
        with qat_vit_amd.forced_drop_path(w, table[:4]):
            pass
    with pytest.raises(RuntimeError, match="3 samples"):
        with qat_vit_amd.forced_drop_path(w, table):
            w(x[:2])
    with pytest.raises(ValueError, match="drop_path_rate > 0"):
        with qat_vit_amd.forced_drop_path(_student(0.0), table):
            pass


def _plain(m, x):
    h = m.patch_embed(x)
    h = torch.cat([m.cls_token.expand(x.shape[0], -1, -1), h], dim=1) + m.pos_embed
    for blk in m.blocks:
        h = h + blk.attn(blk.norm1(h))
        h = h + blk.mlp(blk.norm2(h))
    return m.head(m.norm(h)[:, 0])


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_prepare_qat_leaves_drop_path_alone(backend):
    w = qat_vit_amd.create_student("vit", qat_wrapper=True, drop_path_rate=0.1)
    p = prepare(w, backend)
    assert len(fq_modules(p)) == 126                                                # ViT-S: 76 activation + 50 weight fake-quant modules, as without it
    assert len(fq_modules(prepare(qat_vit_amd.create_student("vit", qat_wrapper=True), backend))) == 126
    for i, b in enumerate(p.model.blocks):
        for d in (b.drop_path1, b.drop_path2):
            assert type(d) is DropPath and not hasattr(d, "activation_post_process") and not list(d.children())
            assert d.drop_prob == w.model.blocks[i].drop_path1.drop_prob
    # a prepared tree on the CPU: the stock modules with the forced table (what the GPU parity test compares the native step with)
    t = qat_vit_amd.create_student("vit", qat_wrapper=True, drop_path_rate=0.1, **TINY)
    pt = prepare(t, backend)
    table = torch.full((2 * TINY["depth"], 2), 0.5)
    with qat_vit_amd.forced_drop_path(pt, table):
        out = pt.dequant(pt.model(pt.quant(torch.randn(2, 3, 32, 32))))
    assert out.shape == (2, 10) and torch.isfinite(out).all()


def test_engine_table_follows_a_drop_path_schedule():
    """The engines' table state (native.DropPathTable, host logic here on the CPU) reads the modules' rates before every step: a schedule that changes
    ``drop_prob`` between epochs reaches the native draw as it reaches the stock forward; eval mode and a rate-0 tree have no table."""
    w = _student(0.3).train()
    t = native.DropPathTable(w.model, torch.device("cpu"))
    assert t.active() and t.keep.flatten().tolist() == pytest.approx([1.0, 1.0, 0.85, 0.85, 0.7, 0.7])
    for b in w.model.blocks:
        b.drop_path1.drop_prob = b.drop_path2.drop_prob = 0.5
    assert t.active() and t.keep.flatten().tolist() == pytest.approx([0.5] * 6) and t.mult.flatten().tolist() == pytest.approx([2.0] * 6)
    for b in w.model.blocks:
        b.drop_path1.drop_prob = b.drop_path2.drop_prob = 0.0
    assert not t.active()
    with qat_vit_amd.forced_drop_path(w, torch.ones(6, 2)):
        assert t.active()
        assert not native.DropPathTable(w.eval().model, torch.device("cpu")).active()
    assert not native.DropPathTable(_student(0.0).train().model, torch.device("cpu")).active()


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert decl, f"{name} is not declared in include/qatvit.h"
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_symbols_in_header_signatures_and_exports(native_lib):
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in SYMBOLS:
        assert _params(name) == ["const qatvit_cfg* cfg", "void* workspace", "const float* scale_table"]
        res, args = native.SIGNATURES[name]
        assert res is native.c_int and args == [native.c_void_p] * 3
        assert name in exported
        assert getattr(native_lib, name)(None, None, None) != 0                     # an argument error is a string, without a HIP call
        assert b"null argument" in native_lib.qatvit_last_error() and name.encode() in native_lib.qatvit_last_error()
    assert native_lib.qatvit_abi_version() == 4                                     # added symbols: the version stays
    assert {"DropPath", "forced_drop_path"} <= set(qat_vit_amd.__all__)
    text = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    assert "no dropout / drop-path" not in text and "not skipped" in text and "epilogue" in text   # the limit is lifted, the two new ones are stated


def test_binding_is_host_state_and_needs_no_gpu(native_lib):
    """Binding and unbinding launch nothing: both entries succeed on a machine without a GPU, for any address."""
    c = native.Cfg(batch=2, img_size=32, patch_size=16, in_chans=3, embed_dim=128, depth=2, num_heads=2, mlp_hidden=512, num_classes=10, act_qmin=0,
                   act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, ln_eps=1e-6)
    import ctypes

    for name in SYMBOLS:
        fn = getattr(native_lib, name)
        assert fn(ctypes.byref(c), 4096, 8192) == 0
        assert fn(ctypes.byref(c), 4096, None) == 0
        assert fn(ctypes.byref(c), 4096, None) == 0                                 # unbinding twice is fine
