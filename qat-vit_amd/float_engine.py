"""Host side of the native float (pre-QAT) student step (``qatvit_float_student_*``, include/qatvit.h).

The reference trains the FLOAT student for the first ``qat_start_epoch`` epochs (qat_trainer.py:295-361 before ``prepare_qat``):
in fp32 in train_final.sh, under ``torch.amp.autocast`` + ``GradScaler`` in the Optuna objective.  ``native_float(wrapper)`` opts an
unprepared ``QATWrapper(vit_*_patch16_224)`` into the native step: its ``forward`` on a CUDA tensor then runs
``qatvit_float_student_forward`` and autograd's backward ``qatvit_float_student_backward``, fp32-accurate (bf16 (hi, lo) pairs, three
MFMA passes per product) whatever autocast says.  ``native_float(wrapper, amp=True)`` adds the fp16 form
(``qatvit_float_student_amp_*``): a forward inside ``torch.autocast("cuda", dtype=torch.float16)`` then follows stock autocast - fp16 GEMM
operands, fp32 residual / LayerNorm / softmax, fp16 logits - and outside autocast runs the fp32-accurate form above; the choice is made per
forward.  ``amp=torch.bfloat16`` adds the bf16 form (``qatvit_float_student_bf16_*``) the same way for
``torch.autocast("cuda", dtype=torch.bfloat16)`` (bf16 planes and MFMA, bf16 logits), and ``amp=(torch.float16, torch.bfloat16)`` follows both
autocast dtypes.  Without the opt-in nothing changes: the float tree is ordinary ``nn.Module`` code.

Engines live in a ``WeakKeyDictionary`` keyed by the wrapper, never on the module, so ``copy.deepcopy`` / ``prepare_qat(inplace=False)``
copy no ctypes state; a copy is not opted in.  A prepared wrapper always takes the QAT engine (engine.py) first.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import List, Optional

import torch
import torch.nn as nn

from . import native

_OPTED = weakref.WeakKeyDictionary()   # wrapper -> FloatStudentEngine (or None until its first CUDA forward)


def check_shape(model: nn.Module, amp=False) -> None:
    """Raise unless the native float step covers this tree (the QAT engine's limits; amp: also the fp16 / bf16 forms')."""
    from .vit import DropPath, LayerScale, VisionTransformer

    if not isinstance(model, VisionTransformer):
        raise RuntimeError(f"native float step: expected the ViT student tree, got {type(model).__name__}")
    D, heads, depth = model.embed_dim, model.num_heads, len(model.blocks)
    hd = D // heads
    why = []
    if D % 128 or D > 768:
        why.append(f"embed_dim {D} (a multiple of 128, <= 768)")
    if D % heads or hd not in (32, 64):
        why.append(f"head_dim {hd} (32 or 64)")
    if model.patch_embed.num_patches + 1 > 224:
        why.append(f"{model.patch_embed.num_patches + 1} tokens (<= 224)")
    if depth < 1 or depth > 12:
        why.append(f"depth {depth} (1..12)")
    pe = model.patch_embed.proj
    if model.patch_embed.img_size % model.patch_embed.patch_size:   # (stock would crop the image to whole patches; the native step reads whole images)
        why.append(f"img_size {model.patch_embed.img_size} (a multiple of the patch size {model.patch_embed.patch_size})")
    if pe.kernel_size[0] % 4 or (pe.in_channels * pe.kernel_size[0] * pe.kernel_size[1]) % 128:
        why.append("patch embedding (patch size a multiple of 4, in_chans * patch^2 a multiple of 128)")
    if type(model.head) is not nn.Linear or type(pe) is not nn.Conv2d:
        why.append("head / patch embedding are not plain Linear / Conv2d")
    for b in model.blocks:
        if b.mlp.fc1.weight.shape[0] % 128:
            why.append(f"mlp hidden {b.mlp.fc1.weight.shape[0]} (a multiple of 128)")
            break
    for m in model.modules():
        if isinstance(m, nn.Dropout) and m.p != 0.0:
            why.append("dropout != 0")
            break
    for b in model.blocks:
        # LayerScale: this package's module (its gamma travels to the residual kernels, which also form its gradient), or none - both branches alike
        kinds = {type(getattr(b, n)) for n in ("ls1", "ls2")}
        if not (kinds == {nn.Identity} or (kinds == {LayerScale} and not (b.ls1.inplace or b.ls2.inplace))):
            why.append("ls1 / ls2 are neither both Identity nor both qat_vit_amd.LayerScale (inplace=False)")
            break
    for b in model.blocks:   # stochastic depth: this package's DropPath (its multipliers travel to the residual kernels), or none
        if not all(isinstance(getattr(b, n), (nn.Identity, DropPath)) for n in ("drop_path1", "drop_path2")):
            why.append("drop_path1 / drop_path2 are neither Identity nor qat_vit_amd.DropPath")
            break
    hidden = model.blocks[0].mlp.fc1.weight.shape[0] if depth else 0
    if amp and (D % 384 or hidden % 384):
        why.append(f"amp=True: embed_dim {D} and mlp hidden {hidden} (multiples of 384 for the fp16 / bf16 forms)")
    if why:
        raise RuntimeError("native float step: unsupported model: " + "; ".join(why))


# the forms: (prefix of the C symbols, dtype of the logits and dlogits)
FP32 = ("qatvit_float_student", torch.float32)        # fp32-accurate: bf16 (hi, lo) pairs, three MFMA passes
FP16 = ("qatvit_float_student_amp", torch.float16)    # stock fp16 autocast
BF16 = ("qatvit_float_student_bf16", torch.bfloat16)  # stock bf16 autocast


def autocast_dtypes(amp) -> tuple:
    """native_float's ``amp`` as the autocast dtypes the engine follows: False -> (), True -> (fp16,), a dtype or several."""
    if amp is None or amp is False:
        return ()
    if amp is True:
        return (torch.float16,)
    dts = (amp,) if isinstance(amp, torch.dtype) else tuple(amp)
    for dt in dts:
        if dt not in (torch.float16, torch.bfloat16):
            raise ValueError(f"native_float: amp={amp!r}: the native forms follow autocast dtypes torch.float16 and torch.bfloat16")
    return dts


class Form:
    """One form of the float step: its C symbols and logits dtype, and its workspace with the batch that is sized for."""

    def __init__(self, prefix: str, dtype: torch.dtype):
        self.prefix, self.dtype = prefix, dtype
        self.workspace: Optional[torch.Tensor] = None
        self.capacity = 0

    def call(self, name: str, *args) -> None:
        """<prefix>_<name>(*args, workspace, stream), checked."""
        fn = f"{self.prefix}_{name}"
        native.check(getattr(native.lib(), fn)(*args, self.workspace.data_ptr(), native.stream_ptr()), fn)

    def workspace_bytes(self, c: native.Cfg) -> int:
        L = native.lib()
        n = getattr(L, self.prefix + "_workspace_bytes")(ctypes.byref(c))
        if n <= 0:
            raise RuntimeError(f"{self.prefix}_workspace_bytes: " + L.qatvit_last_error().decode())
        return n

    def reserve(self, c: native.Cfg, device: torch.device) -> None:
        if c.batch <= self.capacity:
            return
        nbytes = self.workspace_bytes(c)
        self.workspace = None
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.capacity = c.batch
        self.call("init", ctypes.byref(c))


class FloatStudentEngine:
    def __init__(self, wrapper: nn.Module, amp=False):
        model = wrapper.model
        self.amp = autocast_dtypes(amp)   # the autocast dtypes this engine follows (empty: the fp32-accurate form always)
        check_shape(model, bool(self.amp))
        self.lib = native.lib()
        self.params = native.vit_params(model)
        dev = self.params[0].device
        # LayerScale: the 2 * depth gammas behind the parameters of the C ABI, bound to a form's workspace with qatvit_float_student_set_layer_scale
        self.n_abi = len(self.params)
        self.ls = native.LayerScaleBinding(model, dev)
        self.params = self.params + self.ls.gammas
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev or not p.is_cuda:
                raise RuntimeError("native float step: the parameters must be contiguous fp32 tensors on one CUDA device")
        self.device = dev
        self._cfg_kw = dict(native.vit_shape(model), act_qmin=0, act_qmax=255, w_qmin=-128, w_qmax=127, w_per_channel=0, averaging_const=0.01)
        self._ptrs_key = tuple(p.data_ptr() for p in self.params)
        self._ptr_params = (ctypes.c_void_p * len(self.params))(*self._ptrs_key)
        self.fp32, self.fp16, self.bf16 = Form(*FP32), Form(*FP16), Form(*BF16)   # each workspace allocated by the first forward of its form
        self.generation = 0         # bumped by every forward of any form: the workspaces hold the activations of exactly one forward
        self.grad_numel = sum(p.numel() for p in self.params)
        self._grad_offsets = [sum(p.numel() for p in self.params[:i]) for i in range(len(self.params))]   # dense, in parameter order
        self.drop = native.DropPathTable(model, dev)   # stochastic depth: the per-sample multipliers of a training-mode step, one buffer for all three forms

    def cfg_for(self, batch: int) -> native.Cfg:
        return native.Cfg(batch=batch, **self._cfg_kw)

    # the fp32 form's workspace, and each form's capacity, by the names callers read
    workspace = property(lambda self: self.fp32.workspace)
    capacity = property(lambda self: self.fp32.capacity)
    capacity16 = property(lambda self: self.fp16.capacity)

    def workspace_bytes(self, batch: int) -> int:
        return self.fp32.workspace_bytes(self.cfg_for(batch))

    def stale(self) -> bool:
        return tuple(p.data_ptr() for p in self.params) != self._ptrs_key

    def autocast_form(self, dt: torch.dtype) -> Form:
        """The form that follows autocast dtype dt, or RuntimeError when this engine does not follow it."""
        if dt not in self.amp:
            names = " / ".join(f"torch.autocast('cuda', dtype={d})" for d in self.amp)
            raise RuntimeError(f"native float step (amp=True): autocast dtype {dt} is not supported; this engine follows {names} only "
                               "(native_float(..., amp=...) selects the autocast dtypes)")
        return self.fp16 if dt == torch.float16 else self.bf16

    def forward(self, images: torch.Tensor, form: Optional[Form] = None) -> torch.Tensor:
        k = self._cfg_kw
        if images.dim() != 4 or images.shape[0] < 1 or tuple(images.shape[1:]) != (k["in_chans"], k["img_size"], k["img_size"]):
            raise RuntimeError(f"expected images of shape (B, {k['in_chans']}, {k['img_size']}, {k['img_size']}), got {tuple(images.shape)}")
        if not images.is_cuda or images.device != self.device:
            raise RuntimeError(f"native float step: images on {images.device}, parameters on {self.device}")
        images = images.to(torch.float32).contiguous()
        form = form or self.fp32
        c = self.cfg_for(images.shape[0])
        form.reserve(c, self.device)
        # drop-path: filled here, read by this forward and by its backward (the binding stays until the next forward of this form)
        # (with LayerScale the branch is an fp32 tensor when DropPath meets it - 16-bit branch times fp32 gamma - so the multipliers stay fp32 in every form)
        self.drop.bind("qatvit_float_student_set_drop_path", c, form.workspace,
                       self.drop.step(c.batch, form.capacity, round_to=None if form is self.fp32 or self.ls else form.dtype))
        self.ls.bind_float(c, form.workspace)
        logits = torch.empty(c.batch, c.num_classes, dtype=form.dtype, device=self.device)
        self.generation += 1
        form.call("forward", ctypes.byref(c), self._ptr_params, images.data_ptr(), logits.data_ptr())
        return logits

    def backward(self, dlogits: torch.Tensor, batch: int, form: Optional[Form] = None) -> List[torch.Tensor]:
        form = form or self.fp32
        c = self.cfg_for(batch)
        dlogits = dlogits.to(form.dtype).contiguous()
        _, views, gptr = native.flat_grad_buffers(self.params, self._grad_offsets, self.grad_numel)
        self.ls.bind_float(c, form.workspace, views[self.n_abi:])
        form.call("backward", ctypes.byref(c), self._ptr_params, dlogits.data_ptr(), gptr)
        return views


def _step_forward(ctx, images, engine, form: Form):
    ctx.engine = engine
    out = engine.forward(images, form)
    ctx.generation = engine.generation
    ctx.batch = images.shape[0]
    ctx.form = form
    return out


def _step_backward(ctx, dlogits):
    eng = ctx.engine
    native.check_generation(eng, ctx.generation)
    grads = eng.backward(dlogits, ctx.batch, ctx.form)
    native.assign_grads(eng.params, grads)
    return (None, None, None) + (None,) * len(grads)


class _FloatStudentStep(torch.autograd.Function):
    # cast_inputs=float32: inside torch.autocast("cuda") the step keeps its own (fp32-accurate) arithmetic and returns fp32 logits
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, images, engine, form, *params):
        return _step_forward(ctx, images, engine, form)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dlogits):
        return _step_backward(ctx, dlogits)


class _FloatStudentAmpStep(torch.autograd.Function):
    # the fp16 / bf16 form (native_float(..., amp=...) inside fp16 / bf16 autocast): fp16 / bf16 logits as stock autocast's head Linear returns;
    # ctx.form records the form for the backward
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, images, engine, form, *params):
        return _step_forward(ctx, images, engine, form)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dlogits):
        return _step_backward(ctx, dlogits)


def native_float(wrapper: nn.Module, amp=False) -> nn.Module:
    """Opt an unprepared ``QATWrapper(vit_*_patch16_224)`` into the native float step; returns the wrapper.

    The parameters must already be on the GPU; the shape is checked here.  Afterwards ``wrapper(x)`` on a CUDA tensor runs the native
    forward (and its backward), a CPU tensor raises; ``prepare_qat`` of the wrapper is unaffected (a prepared wrapper takes the QAT engine).
    amp=True: a forward inside ``torch.autocast("cuda", dtype=torch.float16)`` runs the fp16 form (fp16 logits, stock autocast's numerics and
    overflow behaviour, for GradScaler); outside autocast the fp32-accurate form; bf16 autocast raises.  amp=torch.bfloat16: the same for
    ``torch.autocast("cuda", dtype=torch.bfloat16)`` with the bf16 form (bf16 logits; no GradScaler needed); fp16 autocast raises.
    amp=(torch.float16, torch.bfloat16): both, chosen per forward.  Any amp needs embed_dim and mlp_hidden multiples of 384."""
    from .model_registry import QATWrapper

    if not isinstance(wrapper, QATWrapper):
        raise TypeError(f"native_float expects a QATWrapper, got {type(wrapper).__name__}")
    if hasattr(wrapper.quant, "activation_post_process"):
        raise RuntimeError("native_float: the wrapper is already prepared for QAT (it runs the native QAT step)")
    if any(not p.is_cuda for p in wrapper.parameters()):
        raise RuntimeError("native_float: move the model to the GPU first (model.cuda()); the native float step runs on MI355X only")
    _OPTED[wrapper] = FloatStudentEngine(wrapper, amp=amp)
    return wrapper


def is_native_float(wrapper) -> bool:
    return wrapper in _OPTED


def engine_of(wrapper) -> Optional[FloatStudentEngine]:
    return _OPTED.get(wrapper)


def float_forward(wrapper, images: torch.Tensor) -> torch.Tensor:
    eng = _OPTED.get(wrapper)
    if eng is None or eng.stale():   # parameters re-allocated (e.g. .to()): the float step keeps no state, rebuild
        eng = _OPTED[wrapper] = FloatStudentEngine(wrapper, amp=eng.amp if eng is not None else False)
    if eng.amp and torch.is_autocast_enabled("cuda"):   # decided per forward
        return _FloatStudentAmpStep.apply(images, eng, eng.autocast_form(torch.get_autocast_dtype("cuda")), *eng.params)
    return _FloatStudentStep.apply(images, eng, eng.fp32, *eng.params)
