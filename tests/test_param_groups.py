"""vit_param_groups against a plain restatement of its rule (no weight decay for 1-d parameters, biases and the named embeddings; layer-wise
learning-rate decay by layer id), on the tiny student as a float tree and after prepare_qat.  No GPU."""
import pytest
import torch

import qat_vit_amd
from qat_vit_amd import vit_param_groups
from tests.util import prepare

DEPTH = 2
NO_DECAY = ("cls_token", "pos_embed")


def _student(kind):
    torch.manual_seed(0)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=128, depth=DEPTH, num_heads=2, img_size=32)
    return prepare(stu, "qnnpack") if kind == "prepared" else stu


def _rule(name, p, wd, lr, d):
    """(layer id, weight_decay, lr) of a parameter called `name` inside the VisionTransformer."""
    wd = 0.0 if (p.ndim <= 1 or name.endswith(".bias") or name.split(".")[-1] in NO_DECAY) else wd
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed."):
        lid = 0
    elif name.startswith("blocks."):
        lid = int(name.split(".")[1]) + 1
    else:
        assert name.startswith(("norm.", "head.")), name
        lid = DEPTH + 1
    return lid, wd, lr * d ** (DEPTH + 1 - lid)


@pytest.fixture(scope="module", params=["float", "prepared"])
def student(request):
    return _student(request.param)


def test_layer_decay_groups_follow_the_rule(student):
    wd, lr, d = 0.05, 1e-3, 0.75
    groups = vit_param_groups(student, wd, lr=lr, layer_decay=d)
    named = [(n, p) for n, p in student.named_parameters()]
    assert named and all(n.startswith("model.") for n, _ in named)
    where = {}
    for gi, g in enumerate(groups):
        assert set(g) == {"params", "weight_decay", "lr"} and g["params"]            # no empty group
        for p in g["params"]:
            assert id(p) not in where                                                 # exactly once
            where[id(p)] = gi
    assert set(where) == {id(p) for _, p in named}
    keys = []
    for n, p in named:
        lid, w, l = _rule(n[len("model."):], p, wd, lr, d)
        g = groups[where[id(p)]]
        assert g["weight_decay"] == w and g["lr"] == l, n
        keys.append((lid, w == 0.0))
    # ascending layer id, decay before no-decay; named_parameters() order inside a group
    order = sorted(set(keys))
    assert [(_rule(n[len("model."):], p, wd, lr, d)[0], g["weight_decay"] == 0.0) for g in groups
            for n, p in named if p is g["params"][0]] == order
    for g in groups:
        pos = [i for p in g["params"] for i, (_, q) in enumerate(named) if q is p]
        assert pos == sorted(pos)
    # layer 0: patch_embed.proj.weight | its bias, cls_token, pos_embed; each block and the norm/head layer: weights | biases and norms
    empty = sum((lid, nd) not in order for lid in range(DEPTH + 2) for nd in (False, True))
    assert len(groups) == 2 * (DEPTH + 2) - empty and empty == 0
    assert groups[-1]["lr"] == lr and groups[0]["lr"] == lr * d ** (DEPTH + 1)
    decayed = {n for n, p in named if groups[where[id(p)]]["weight_decay"] == wd}
    assert "model.blocks.0.attn.qkv.weight" in decayed and "model.head.weight" in decayed and "model.patch_embed.proj.weight" in decayed
    assert not any(n.endswith(("bias", "cls_token", "pos_embed")) or ".norm" in n for n in decayed)


def test_two_groups_without_layer_decay(student):
    groups = vit_param_groups(student, 0.05)
    assert [g["weight_decay"] for g in groups] == [0.05, 0.0] and all(set(g) == {"params", "weight_decay"} for g in groups)
    named = list(student.named_parameters())
    for want, g in zip((0.05, 0.0), groups):
        assert [id(p) for p in g["params"]] == [id(p) for n, p in named if _rule(n[len("model."):], p, 0.05, 1.0, 1.0)[1] == want]
    with_lr = vit_param_groups(student, 0.05, lr=3e-4)
    assert [g["lr"] for g in with_lr] == [3e-4, 3e-4]
    # the embeddings decay once they are not named
    plain = vit_param_groups(student, 0.05, no_decay_names=())
    assert any(p is student.model.pos_embed for p in plain[0]["params"]) and any(p is student.model.cls_token for p in plain[0]["params"])


def test_frozen_parameters_are_left_out_and_empty_groups_not_emitted():
    stu = _student("float")
    vit = stu.model
    frozen = [vit.pos_embed, vit.blocks[1].mlp.fc1.weight, vit.head.weight, vit.head.bias, vit.norm.weight, vit.norm.bias]
    for p in vit.patch_embed.parameters():
        frozen.append(p)
    frozen.append(vit.cls_token)
    for p in frozen:
        p.requires_grad_(False)
    groups = vit_param_groups(stu, 0.05, lr=1e-3, layer_decay=0.75)
    got = [id(p) for g in groups for p in g["params"]]
    assert len(got) == len(set(got)) and set(got) == {id(p) for p in stu.parameters() if p.requires_grad}
    assert not set(got) & {id(p) for p in frozen}
    # layer 0 and layer depth + 1 are entirely frozen: both of their groups are gone
    assert len(groups) == 2 * (DEPTH + 2) - 4 and all(g["params"] for g in groups)
    assert [g["lr"] for g in groups] == [1e-3 * 0.75 ** 2] * 2 + [1e-3 * 0.75] * 2


def test_layer_decay_needs_lr_and_a_vit():
    stu = _student("float")
    with pytest.raises(ValueError, match="lr"):
        vit_param_groups(stu, 0.05, layer_decay=0.75)
    with pytest.raises(TypeError, match="VisionTransformer"):
        vit_param_groups(torch.nn.Linear(3, 3), 0.05)


def test_the_bare_tree_and_a_ddp_style_wrapper_give_the_same_groups():
    stu = _student("float")

    class Wrapped(torch.nn.Module):      # DistributedDataParallel's naming: the model under `.module`
        def __init__(self, m):
            super().__init__()
            self.module = m

    ref = vit_param_groups(stu, 0.05, lr=1e-3, layer_decay=0.75)
    for other in (stu.model, Wrapped(stu), Wrapped(stu.model)):
        got = vit_param_groups(other, 0.05, lr=1e-3, layer_decay=0.75)
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert [id(p) for p in a["params"]] == [id(p) for p in b["params"]] and a["lr"] == b["lr"] and a["weight_decay"] == b["weight_decay"]
    opt = torch.optim.AdamW(ref, lr=1e-3)       # the dicts are what stock torch takes
    assert len(opt.param_groups) == len(ref)
