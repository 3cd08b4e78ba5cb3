"""LayerScale (``init_values``) on the host: the module tree (qat_vit_amd.LayerScale), what ``prepare_qat`` makes of it, parameter groups, the flat gradient
layout, the int8 export and the C entries that bind the gammas to a workspace (include/qatvit.h) - without a GPU.  The native steps: tests/test_gpu_layer_scale.py."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn

import qat_vit_amd
from qat_vit_amd import LayerScale, native
from qat_vit_amd.engine import FlatGradLayout
from qat_vit_amd.vit import _native_teacher_ok, layer_scale_params
from tests.util import fq_modules, prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(embed_dim=128, depth=3, num_heads=2, img_size=32)


def _student(init_values, **kw):
    torch.manual_seed(0)
    return qat_vit_amd.create_student("vit", qat_wrapper=True, init_values=init_values, **{**TINY, **kw})


def test_init_values_none_is_the_tree_as_it_was_and_a_value_adds_only_the_gammas():
    plain = qat_vit_amd.create_student("vit", qat_wrapper=True, **TINY)
    for falsy in (None, 0, 0.0):
        a = _student(falsy)
        assert list(a.state_dict()) == list(plain.state_dict())
        assert [type(m) for m in a.modules()] == [type(m) for m in plain.modules()]
        assert all(type(b.ls1) is nn.Identity and type(b.ls2) is nn.Identity for b in a.model.blocks) and layer_scale_params(a.model) == []
    b = _student(1e-5)
    extra = [k for k in b.state_dict() if k not in plain.state_dict()]
    assert extra == [f"model.blocks.{i}.{n}.gamma" for i in range(TINY["depth"]) for n in ("ls1", "ls2")]
    assert [k for k in b.state_dict() if k in plain.state_dict()] == list(plain.state_dict())
    for k in extra:
        assert torch.equal(b.state_dict()[k], 1e-5 * torch.ones(TINY["embed_dim"])) and b.state_dict()[k].dtype == torch.float32
    assert [id(p) for p in layer_scale_params(b.model)] == [id(m.gamma) for blk in b.model.blocks for m in (blk.ls1, blk.ls2)]
    assert "LayerScale" in qat_vit_amd.__all__ and type(b.model.blocks[0].ls1) is LayerScale and not b.model.blocks[0].ls1.inplace
    c = copy.deepcopy(b)                                                          # deep copy, and a strict load between two such trees
    with torch.no_grad():
        for p in layer_scale_params(c.model):
            p.uniform_(-2, 2)
    assert b.load_state_dict(c.state_dict(), strict=True).missing_keys == []
    assert all(torch.equal(p, q) for p, q in zip(layer_scale_params(b.model), layer_scale_params(c.model)))
    with pytest.raises(RuntimeError, match="gamma"):
        plain.load_state_dict(c.state_dict(), strict=True)
    w = qat_vit_amd.create_model("vit_small_patch16_224_student", pretrained=False, qat_wrapper=True, init_values=0.1, depth=2)   # through create_model
    assert torch.equal(w.model.blocks[1].ls2.gamma, 0.1 * torch.ones(384))
    x = torch.randn(2, 3, 4)
    assert torch.equal(LayerScale(4, 0.5)(x), x * 0.5)
    y = x.clone()
    assert LayerScale(4, 0.5, inplace=True)(y) is y and torch.equal(y, x * 0.5)
    assert _native_teacher_ok(plain.model) and not _native_teacher_ok(b.model)   # a LayerScale teacher: the stock module forward


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_prepare_qat_leaves_layer_scale_alone(backend):
    w = qat_vit_amd.create_student("vit", qat_wrapper=True, init_values=1e-5, drop_path_rate=0.1)
    p = prepare(w, backend)
    assert len(fq_modules(p)) == 126                                              # ViT-S: as without LayerScale
    for b in p.model.blocks:
        for m in (b.ls1, b.ls2):
            assert type(m) is LayerScale and not hasattr(m, "activation_post_process") and not list(m.children())
    assert len(layer_scale_params(p.model)) == 24


def test_forward_is_the_written_composition_in_fp64():
    w = _student(1e-5, drop_path_rate=0.3).double().train()
    B, depth = 3, TINY["depth"]
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in layer_scale_params(w.model):
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64))
    x = torch.randn(B, 3, 32, 32, generator=g, dtype=torch.float64)
    table = torch.tensor([0.0, 0.5, 1.25, 2.0])[torch.randint(0, 4, (2 * depth, B), generator=g)]
    with qat_vit_amd.forced_drop_path(w, table):
        out = w(x)
    m = w.model
    h = m.patch_embed(x)
    h = torch.cat([m.cls_token.expand(B, -1, -1), h], dim=1) + m.pos_embed
    for i, blk in enumerate(m.blocks):
        h = h + (blk.attn(blk.norm1(h)) * blk.ls1.gamma) * table[2 * i].double().view(B, 1, 1)
        h = h + (blk.mlp(blk.norm2(h)) * blk.ls2.gamma) * table[2 * i + 1].double().view(B, 1, 1)
    assert torch.equal(out, m.head(m.norm(h)[:, 0]))
    # bf16 tensor times fp32 parameter inside autocast: the product is fp32 (what the native 16-bit forms follow)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert (torch.ones(2, 4, dtype=torch.bfloat16) * LayerScale(4).gamma).dtype == torch.float32


def test_vit_param_groups_put_every_gamma_in_the_no_decay_group_of_its_block():
    w = _student(1e-5)
    groups = qat_vit_amd.vit_param_groups(w, weight_decay=0.05, lr=1e-3, layer_decay=0.5)
    depth = TINY["depth"]
    where = {id(p): g for g in groups for p in g["params"]}
    for i, blk in enumerate(w.model.blocks):
        for m in (blk.ls1, blk.ls2):
            g = where[id(m.gamma)]
            assert g["weight_decay"] == 0.0 and g["lr"] == pytest.approx(1e-3 * 0.5 ** (depth + 1 - (i + 1)))
            assert any(p is blk.norm1.bias for p in g["params"])                  # the no-decay group of its own block


def test_flat_grad_layout_with_gammas():
    depth, D = 3, 128
    w = _student(1e-5)
    base = [p.numel() for p in native.vit_params(w.model)]
    old, new = FlatGradLayout(base, depth), FlatGradLayout(base + [D] * (2 * depth), depth)
    ref = {}                                                                      # today's layout, restated: stage order, 64-element alignment
    n = 0
    for pi in [len(base) - 4 + k for k in range(4)] + [4 + 12 * i + k for i in reversed(range(depth)) for k in range(12)] + [0, 1, 2, 3]:
        ref[pi] = n
        n += (base[pi] + 63) // 64 * 64
    assert old.offset == ref and old.numel == n
    nb = len(base)
    spans = sorted((new.offset[pi], new.offset[pi] + new.numels[pi]) for pi in range(nb + 2 * depth))
    assert all(a % 64 == 0 for a, _ in spans) and all(e0 <= a1 for (_, e0), (a1, _) in zip(spans, spans[1:])) and spans[-1][1] <= new.numel
    for i in range(depth):
        s = depth - i                                                             # block i's backward stage
        lo, hi = new.stage_end[s - 1], new.stage_end[s]
        for pi in (nb + 2 * i, nb + 2 * i + 1, 4 + 12 * i, 4 + 12 * i + 11):
            assert lo <= new.offset[pi] and new.offset[pi] + new.numels[pi] <= hi, (i, pi)
    assert new.stage_end[0] == old.stage_end[0] and new.numel == old.numel + 2 * depth * D
    with pytest.raises(ValueError, match="LayerScale"):
        FlatGradLayout(base + [D], depth)


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_export_import_round_trips_the_gammas(backend):
    p = prepare(_student(1e-5), backend)
    with torch.no_grad():
        for q in layer_scale_params(p.model):
            q.copy_(torch.randn(q.shape) * 1e-3)
        p.dequant(p.model(p.quant(torch.randn(2, 3, 32, 32))))                    # one observer pass of the stock modules: every quantizer has a range
    e = qat_vit_amd.export_int8(p)
    assert all(e["float"][f"model.blocks.{i}.{n}.gamma"].dtype == torch.float32 for i in range(TINY["depth"]) for n in ("ls1", "ls2"))
    q = qat_vit_amd.import_int8(e, device="cpu")
    got = layer_scale_params(q.model)
    assert len(got) == 2 * TINY["depth"] and all(torch.equal(u, v) for u, v in zip(got, layer_scale_params(p.model)))
    plain = qat_vit_amd.import_int8(qat_vit_amd.export_int8(prepare(_student(None), backend)), device="cpu")
    assert layer_scale_params(plain.model) == []


def _decl(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qatvit.h")).read(), flags=re.S)
    decl = re.search(r"\b(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert decl, f"{name} is not declared in include/qatvit.h"
    return decl.group(1), [" ".join(p.split()) for p in decl.group(2).split(",")]


def test_symbols_in_header_signatures_and_exports(native_lib):
    exported = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    common = ["const qatvit_cfg* cfg", "void* workspace", "const float* const* gammas", "float* const* grads"]
    want = {"qatvit_student_set_layer_scale": ("int", common, native.c_int, 4),
            "qatvit_float_student_set_layer_scale": ("int", common + ["void* saved"], native.c_int, 5),
            "qatvit_float_student_layer_scale_bytes": ("int64_t", ["const qatvit_cfg* cfg"], native.c_int64, 1)}
    for name, (ret, params, res, n) in want.items():
        assert _decl(name) == (ret, params)
        assert native.SIGNATURES[name] == (res, [native.c_void_p] * n) and name in exported
    for name in list(want)[:2]:
        assert getattr(native_lib, name)(*[None] * want[name][3]) != 0            # an argument error is a string, without a HIP call
        assert b"null argument" in native_lib.qatvit_last_error() and name.encode() in native_lib.qatvit_last_error()
    assert native_lib.qatvit_abi_version() == 4
    text = open(os.path.join(ROOT, "include", "qatvit.h")).read()
    assert "no LayerScale" not in text and "WITHOUT the STE mask" in text


def test_binding_is_host_state_and_needs_no_gpu(native_lib):
    c = native.Cfg(batch=2, img_size=32, patch_size=16, in_chans=3, embed_dim=128, depth=2, num_heads=2, mlp_hidden=512, num_classes=10, act_qmin=0,
                   act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01, ln_eps=1e-6)
    assert native_lib.qatvit_float_student_layer_scale_bytes(ctypes.byref(c)) == 2 * 2 * 2 * 5 * 128 * 4 + 256   # the branch outputs, and 256 bytes of per-branch scales
    ptrs = (ctypes.c_void_p * 4)(4096, 8192, 12288, 16384)
    hole = (ctypes.c_void_p * 4)(4096, None, 12288, 16384)
    q, f = native_lib.qatvit_student_set_layer_scale, native_lib.qatvit_float_student_set_layer_scale
    assert q(ctypes.byref(c), 4096, ptrs, ptrs) == 0 and q(ctypes.byref(c), 4096, ptrs, None) == 0
    assert q(ctypes.byref(c), 4096, hole, None) != 0 and b"branch 1" in native_lib.qatvit_last_error()
    assert q(ctypes.byref(c), 4096, None, None) == 0 and q(ctypes.byref(c), 4096, None, None) == 0      # unbinding twice is fine
    assert f(ctypes.byref(c), 4096, ptrs, ptrs, 65536) == 0 and f(ctypes.byref(c), 4096, ptrs, None, None) == 0
    assert f(ctypes.byref(c), 4096, ptrs, ptrs, None) != 0 and b"saved" in native_lib.qatvit_last_error()
    assert f(ctypes.byref(c), 4096, None, None, None) == 0


def test_float_check_shape_takes_identity_or_layer_scale_on_both_branches():
    from qat_vit_amd.float_engine import check_shape

    check_shape(_student(1e-5).model)
    check_shape(_student(None).model)
    w = _student(1e-5)
    w.model.blocks[1].ls2 = nn.Identity()
    with pytest.raises(RuntimeError, match="ls1 / ls2"):
        check_shape(w.model)
    w = _student(1e-5)
    w.model.blocks[0].ls1.inplace = w.model.blocks[0].ls2.inplace = True
    with pytest.raises(RuntimeError, match="ls1 / ls2"):
        check_shape(w.model)
