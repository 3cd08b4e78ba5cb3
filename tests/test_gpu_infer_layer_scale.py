"""The integer forward of an export that holds LayerScale gammas (``Int8Student(export, layer_scale=True)`` -> ``qatvit_infer_forward_ls``): its logits are
BIT-IDENTICAL to the fake-quant forward of the exporting model with its observers switched off - the native QAT forward, whose residual kernel computes
``x + fq(y) * gamma`` with the product rounded on its own, which is what the proj / fc2 GEMM epilogues of the integer forward compute.

Every model is trained for two steps (so no scale is a default), gets its biases and norms perturbed and its gammas set by the "mixed" rule of
tests/test_gpu_layer_scale.py (both signs, magnitudes 0.5 .. 2, two exact zeros per branch - never the 1e-5 of a fresh LayerScale, under which a wrong
gamma would vanish in the logits' last bits), observes once more and is frozen.  Shapes: the widths ``Int8Student`` admits at token counts the QAT engine
is tested at - 15, 222 (one row group past a 208-row tile) and 394 rows, head_dim 64 and 32, per-tensor and per-channel weights."""
import copy
import functools
import io

import pytest
import torch
from torch.ao.quantization import disable_observer
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

import qat_vit_amd  # noqa: E402
from qat_vit_amd import functional as F  # noqa: E402
from qat_vit_amd.export import Int8Student, export_int8, import_int8  # noqa: E402
from tests.test_gpu_layer_scale import set_gammas, zero_columns  # noqa: E402
from tests.util import prepare  # noqa: E402

# name: (architecture, batch, backend)
MODELS = {
    "w384-15rows-qnnpack": (dict(embed_dim=384, depth=2, img_size=32), 3, "qnnpack"),
    "w384-15rows-x86": (dict(embed_dim=384, depth=2, img_size=32), 3, "x86"),
    "w384-222rows": (dict(embed_dim=384, depth=2, img_size=96), 6, "qnnpack"),
    "w384-head32": (dict(embed_dim=384, depth=1, num_heads=12, img_size=32), 3, "qnnpack"),
    "w768-x86": (dict(embed_dim=768, depth=1, num_heads=12, img_size=32), 2, "x86"),
    "w384-394rows": (dict(embed_dim=384, depth=1, img_size=224), 2, "qnnpack"),
}


def _freeze(model, x):
    with torch.no_grad():
        model(x)                                 # the weights (and the gammas) moved: observe once more, then freeze
    model.apply(disable_observer)
    return model.eval()


def _build(kw, B, backend, layer_scale=True, kind="mixed", rate=0.0, ema=None, steps=2):
    """(frozen eval model, images, optimizer).  As tests/test_gpu_infer.py::_trained, with LayerScale (and drop-path) in the tree."""
    torch.manual_seed(3)
    extra = dict(init_values=1.0) if layer_scale else {}
    if rate:
        extra["drop_path_rate"] = rate
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **extra, **kw)
    with torch.no_grad():                        # timm's init leaves biases at zero: make every term of the epilogues count
        for n, p in stu.named_parameters():
            if p.dim() == 1 and not n.endswith(".gamma"):
                p.add_(0.05 * torch.randn_like(p))
    model = prepare(stu.cuda(), backend)
    g = torch.Generator().manual_seed(1)
    s = kw["img_size"]
    x, y = torch.randn(B, 3, s, s, generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()
    opt = qat_vit_amd.ClipAdamW(model.parameters(), lr=1e-3, weight_decay=1e-3, **({} if ema is None else dict(ema_decay=ema)))
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        F.kd_ce_loss(model(x), None, y, 4.0, 0.5, 0.1)[0].backward()
        opt.step(max_norm=1.0)
    if layer_scale:
        set_gammas(model.model, kind)
    return _freeze(model, x), x, opt


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, images, reference logits, export) of a LayerScale model: built once, never written to."""
    kw, B, backend = MODELS[name]
    model, x, _ = _build(kw, B, backend)
    with torch.no_grad():
        ref = model(x).clone()
    return model, x, ref, export_int8(model)


def _without_gammas(export):
    e = dict(export)
    e["float"] = {n: t for n, t in export["float"].items() if not n.endswith(".gamma")}
    return e


@pytest.mark.parametrize("name", list(MODELS))
def test_int8_inference_with_layer_scale_equals_the_fake_quant_forward(native_lib, name):
    model, x, ref, export = _case(name)
    depth = MODELS[name][0]["depth"]
    assert sum(n.endswith(".gamma") for n in export["float"]) == 2 * depth
    buf = io.BytesIO()
    torch.save(export, buf)
    buf.seek(0)
    infer = Int8Student(torch.load(buf, weights_only=False), layer_scale=True)
    assert len(infer.ls_gamma) == 2 * depth
    out = infer(x)
    assert torch.equal(out, ref), (out - ref).abs().max().item()
    with torch.no_grad():
        ref2 = model(x[:2]).clone()
    assert torch.equal(infer(x[:2]), ref2)       # a smaller batch in the same workspace
    assert torch.equal(infer(x), ref)            # and again: nothing in the workspace is consumed
    assert infer.capacity == x.shape[0]
    # the gammas matter: the integer forward of the same export without them is another function
    assert not torch.equal(Int8Student(_without_gammas(export))(x), ref)
    # and the fake-quant forward rebuilt from the export agrees as well
    with torch.no_grad():
        assert torch.equal(import_int8(export)(x), ref)


@pytest.mark.parametrize("name", list(MODELS))
def test_control_the_same_models_without_layer_scale(native_lib, name):
    """Existing code at these small shapes: a tree without LayerScale through ``Int8Student(e)``, and through the keyword, which changes nothing for it."""
    kw, B, backend = MODELS[name]
    model, x, _ = _build(kw, B, backend, layer_scale=False)
    with torch.no_grad():
        ref = model(x).clone()
    e = export_int8(model)
    assert not any(n.endswith(".gamma") for n in e["float"])
    assert torch.equal(Int8Student(e)(x), ref)
    on = Int8Student(e, layer_scale=True)
    assert on.ls_gamma == [] and torch.equal(on(x), ref)


@pytest.mark.parametrize("name", ["w384-15rows-qnnpack", "w384-222rows", "w768-x86"])
def test_all_ones_gammas_are_the_forward_without_gammas_bit_for_bit(native_lib, name):
    kw, B, backend = MODELS[name]
    model, x, _ = _build(kw, B, backend, kind="ones")
    e = export_int8(model)
    assert all(bool((t == 1).all()) for n, t in e["float"].items() if n.endswith(".gamma"))
    with torch.no_grad():
        ref = model(x).clone()
    out = Int8Student(e, layer_scale=True)(x)
    assert torch.equal(out, Int8Student(_without_gammas(e))(x))
    assert torch.equal(out, ref)


def test_one_gamma_of_one_branch_changes_the_logits(native_lib):
    _, x, ref, export = _case("w384-15rows-qnnpack")
    for name, col in (("model.blocks.0.ls1.gamma", 7), ("model.blocks.1.ls2.gamma", 200)):
        k = 2 * int(name.split(".")[2]) + (name.split(".")[3] == "ls2")
        assert col not in zero_columns(384, k)
        e = dict(export)
        e["float"] = dict(export["float"])
        e["float"][name] = export["float"][name].clone()
        e["float"][name][col] *= -1.0
        assert not torch.equal(Int8Student(e, layer_scale=True)(x), ref), name
    assert torch.equal(Int8Student(export, layer_scale=True)(x), ref)   # the shared export was not written to


def test_export_inside_ema_weights_carries_the_averaged_gammas(native_lib):
    kw, B, backend = MODELS["w384-15rows-qnnpack"]
    model, x, opt = _build(kw, B, backend, ema=0.5, steps=3)
    names = [n for n, _ in model.named_parameters() if n.endswith(".gamma")]
    gam = dict(model.named_parameters())
    with torch.no_grad():
        live = model(x).clone()
        with opt.ema_weights():
            e = export_int8(model)
            inside = model(x).clone()
            avg = {n: gam[n].detach().cpu().clone() for n in names}
        e_live = export_int8(model)
    assert all(torch.equal(e["float"][n], avg[n]) for n in names)
    assert any(not torch.equal(e["float"][n], e_live["float"][n]) for n in names)
    assert not torch.equal(inside, live)
    assert torch.equal(Int8Student(e, layer_scale=True)(x), inside)
    assert torch.equal(Int8Student(e_live, layer_scale=True)(x), live)


def test_drop_path_and_layer_scale_model_equals_its_eval_forward(native_lib):
    kw, B, backend = MODELS["w384-15rows-qnnpack"]
    model, x, _ = _build(kw, B, backend, rate=0.1)
    assert any(type(m) is qat_vit_amd.DropPath for m in model.modules())
    with torch.no_grad():
        ref = model(x).clone()
    e = export_int8(model)
    assert torch.equal(Int8Student(e, layer_scale=True)(x), ref)
    with torch.no_grad():
        assert torch.equal(import_int8(e)(x), ref)


def test_evaluate_agrees_on_every_sample(native_lib):
    model, _, _, export = _case("w384-15rows-qnnpack")
    g = torch.Generator().manual_seed(14)
    loader = DataLoader(TensorDataset(torch.randn(20, 3, 32, 32, generator=g), torch.randint(0, 10, (20,), generator=g)), batch_size=8)
    infer = Int8Student(export, layer_scale=True)
    m = copy.deepcopy(model)
    r = qat_vit_amd.evaluate(infer, loader, other=m)
    assert r.total == 20 and r.agree == r.total and r.other_rows_seen == 20 and r.other_correct == r.correct and r.agreement == 100.0
    assert r.correct == qat_vit_amd.evaluate(m, loader).correct
