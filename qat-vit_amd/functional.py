"""torch.autograd glue over the per-op C ABI (include/qatvit.h).

torch is plumbing here: it owns device memory and streams; every arithmetic
step of these ops runs in libqatvit.so.  All functions require CUDA (HIP)
tensors and raise otherwise.
"""
from __future__ import annotations

import torch

from . import native


def _need_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: qat-vit_amd ops run on MI355X only (got a {t.device} tensor); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected float32, got {t.dtype}")


_WS = {}


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
        _WS[key] = ws
    return ws


def fq_module_args(fq):
    """Pull the in-place state of a FusedMovingAvgObsFakeQuantize module
    (torch/ao/quantization/fake_quantize.py:371-438) out as C-ABI arguments."""
    obs = fq.activation_post_process
    return obs, float(obs.averaging_constant), int(obs.quant_min), int(obs.quant_max), bool(fq.is_per_channel), bool(fq.is_symmetric_quant)


class _FakeQuantFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fq):
        _need_cuda(x, "fake_quant")
        x = x.contiguous()
        obs, c, qmin, qmax, per_channel, symmetric = fq_module_args(fq)
        n = x.numel()
        if per_channel:
            if fq.ch_axis != 0:
                raise RuntimeError("per-channel fake-quant is only defined for ch_axis 0 (as in ATen's fused op)")
            channels, inner = x.shape[0], n // max(1, x.shape[0])
            if obs.min_val.numel() == 0:  # first call: the fused op sizes its state here
                obs.min_val.resize_(channels).fill_(float("inf"))
                obs.max_val.resize_(channels).fill_(float("-inf"))
                fq.scale.resize_(channels).fill_(1.0)
                fq.zero_point.resize_(channels).fill_(0)
        else:
            channels, inner = 1, n
        y = torch.empty_like(x)
        mask = torch.empty(((n + 31) // 32) * 4, dtype=torch.uint8, device=x.device)
        L = native.lib()
        ws = _workspace(x.device, L.qatvit_fq_workspace_bytes(channels))
        native.check(
            L.qatvit_fq_forward(
                x.data_ptr(), y.data_ptr(), mask.data_ptr(), obs.min_val.data_ptr(), obs.max_val.data_ptr(),
                fq.scale.data_ptr(), fq.zero_point.data_ptr(), fq.observer_enabled.data_ptr(), fq.fake_quant_enabled.data_ptr(),
                c, qmin, qmax, channels, inner, int(per_channel), int(symmetric), ws.data_ptr(), native.stream_ptr(),
            ),
            "qatvit_fq_forward",
        )
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        native.check(native.lib().qatvit_fq_backward(dy.data_ptr(), mask.data_ptr(), dx.data_ptr(), dy.numel(), native.stream_ptr()), "qatvit_fq_backward")
        return dx, None


def fake_quant(x: torch.Tensor, fq_module) -> torch.Tensor:
    """Native replacement for ``fq_module(x)``; updates the module's buffers in place."""
    return _FakeQuantFn.apply(x, fq_module)


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        _need_cuda(x, "layer_norm")
        x = x.contiguous()
        D = x.shape[-1]
        rows = x.numel() // D
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        native.check(
            native.lib().qatvit_ln_forward(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                           rows, D, float(eps), native.stream_ptr()),
            "qatvit_ln_forward",
        )
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        D = x.shape[-1]
        dx = torch.empty_like(x)
        dg = torch.zeros_like(gamma)
        db = torch.zeros_like(gamma)
        native.check(
            native.lib().qatvit_ln_backward(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                            dg.data_ptr(), db.data_ptr(), x.numel() // D, D, native.stream_ptr()),
            "qatvit_ln_backward",
        )
        return dx, dg, db, None


def layer_norm(x, gamma, beta, eps=1e-6):
    return _LayerNormFn.apply(x, gamma, beta, eps)


class _KDCELossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, labels, kd_temp, kd_alpha, label_smoothing):
        _need_cuda(student, "kd_ce_loss")
        student = student.contiguous()
        B, C = student.shape
        out3 = torch.empty(3, dtype=torch.float32, device=student.device)
        dlogits = torch.empty_like(student)
        tptr = 0
        if teacher is not None:
            teacher = teacher.contiguous().float()
            tptr = teacher.data_ptr()
        labels = labels.contiguous()
        if labels.dtype != torch.int64:
            raise RuntimeError("kd_ce_loss: labels must be int64")
        native.check(
            native.lib().qatvit_kd_ce_loss(student.data_ptr(), tptr, labels.data_ptr(), B, C, float(kd_temp), float(kd_alpha),
                                           float(label_smoothing), out3.data_ptr(), dlogits.data_ptr(), native.stream_ptr()),
            "qatvit_kd_ce_loss",
        )
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(out3)
        return out3[0], out3

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dloss, None, None, None, None, None


def kd_ce_loss(student, teacher, labels, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1):
    """Returns (loss, [loss, ce, kd*T^2]).  ``teacher=None`` -> CE only
    (the reference's step at /root/reference/src/training/qat_trainer.py:343-349)."""
    return _KDCELossFn.apply(student, teacher, labels, kd_temp, kd_alpha, label_smoothing)


class _KDCELossTableFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, table, index, labels, kd_temp, kd_alpha, label_smoothing):
        _need_cuda(student, "kd_ce_loss_table")
        _need_cuda(table, "kd_ce_loss_table")
        student = student.contiguous()
        B, C = student.shape
        if table.dim() != 2 or table.shape[1] != C or table.shape[0] < 1 or not table.is_contiguous() or table.device != student.device:
            raise RuntimeError(f"kd_ce_loss_table: the table must be a contiguous [rows, {C}] tensor on {student.device}, got {tuple(table.shape)} on {table.device}")
        index, labels = index.contiguous(), labels.contiguous()
        if index.dtype != torch.int64 or labels.dtype != torch.int64:
            raise RuntimeError("kd_ce_loss_table: index and labels must be int64")
        if index.shape != (B,) or labels.shape != (B,) or index.device != student.device or labels.device != student.device:
            raise RuntimeError(f"kd_ce_loss_table: index and labels must be [{B}] tensors on {student.device}")
        out3 = torch.empty(3, dtype=torch.float32, device=student.device)
        dlogits = torch.empty_like(student)
        native.check(
            native.lib().qatvit_kd_ce_loss_table(student.data_ptr(), table.data_ptr(), table.shape[0], index.data_ptr(), labels.data_ptr(), B, C,
                                                 float(kd_temp), float(kd_alpha), float(label_smoothing), out3.data_ptr(), dlogits.data_ptr(),
                                                 native.stream_ptr()),
            "qatvit_kd_ce_loss_table",
        )
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(out3)
        return out3[0], out3

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dloss, None, None, None, None, None, None


def kd_ce_loss_table(student, table, index, labels, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1):
    """``kd_ce_loss(student, table[index], labels, ...)`` in one launch, without the gathered tensor: returns (loss, [loss, ce, kd*T^2]).
    ``table`` is fp32 ``[rows, C]`` (per-sample teacher logits, distill.TeacherLogitTable), ``index`` int64 ``[B]``.  An index outside the table
    makes the loss and that row of the gradient NaN; it is not an error on the host (nothing here synchronises)."""
    return _KDCELossTableFn.apply(student, table, index, labels, kd_temp, kd_alpha, label_smoothing)


class _KDCELossMixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing):
        who = "kd_ce_loss_mix" if table is None else "kd_ce_loss_table_mix"
        _need_cuda(student, who)
        student = student.contiguous()
        B, C = student.shape
        dev = student.device
        tptr = bptr = iptr = None
        rows = 0
        if teacher is not None:
            teacher = teacher.contiguous().float()
            if teacher.shape != (B, C) or teacher.device != dev:
                raise RuntimeError(f"{who}: the teacher must be a [{B}, {C}] tensor on {dev}, got {tuple(teacher.shape)} on {teacher.device}")
            tptr = teacher.data_ptr()
        if table is not None:
            _need_cuda(table, who)
            if table.dim() != 2 or table.shape[1] != C or table.shape[0] < 1 or not table.is_contiguous() or table.device != dev:
                raise RuntimeError(f"{who}: the table must be a contiguous [rows, {C}] tensor on {dev}, got {tuple(table.shape)} on {table.device}")
            index = index.contiguous()
            if index.dtype != torch.int64 or index.shape != (B,) or index.device != dev:
                raise RuntimeError(f"{who}: index must be an int64 [{B}] tensor on {dev}")
            bptr, iptr, rows = table.data_ptr(), index.data_ptr(), table.shape[0]
        labels = labels.contiguous()
        if labels.dtype != torch.int64 or labels.shape != (B,) or labels.device != dev:
            raise RuntimeError(f"{who}: labels must be an int64 [{B}] tensor on {dev}")
        mptr = None
        if mix is not None:
            if mix.dtype != torch.int32 or tuple(mix.shape) != (B, 6) or not mix.is_contiguous() or mix.device != dev:
                raise RuntimeError(f"{who}: mix must be a contiguous int32 [{B}, 6] tensor on {dev}")
            mptr = mix.data_ptr()
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(student)
        native.check(
            native.lib().qatvit_kd_ce_loss_mix(student.data_ptr(), tptr, bptr, rows, iptr, labels.data_ptr(), mptr, B, C, float(kd_temp),
                                               float(kd_alpha), float(label_smoothing), out3.data_ptr(), dlogits.data_ptr(), native.stream_ptr()),
            "qatvit_kd_ce_loss_mix",
        )
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(out3)
        return out3[0], out3

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * dloss,) + (None,) * 8


def kd_ce_loss_mix(student, teacher, labels, mix, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1):
    """``kd_ce_loss`` on a mixed batch: returns (loss, [loss, ce, kd*T^2]).  ``mix`` is the int32 ``[B, 6]`` record tensor the images were mixed
    with (data.MixupCutmix): row b's hard target is ``lam`` on ``labels[b]`` and ``1 - lam`` on the partner's label.  ``teacher`` (``[B, C]`` or
    None) is the teacher's output on the mixed images, so the KD part is ``kd_ce_loss``'s.  ``mix=None`` is ``kd_ce_loss``."""
    return _KDCELossMixFn.apply(student, teacher, None, None, labels, mix, kd_temp, kd_alpha, label_smoothing)


def kd_ce_loss_table_mix(student, table, index, labels, mix, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1):
    """``kd_ce_loss_table`` on a mixed batch: the hard target as in ``kd_ce_loss_mix``, the KD target
    ``lam * softmax(table[index[b]] / T) + (1 - lam) * softmax(table[index[p]] / T)`` - the usual mixed soft label, not the teacher's output on
    the mixed image.  An index outside the table, of the row or (where ``lam != 1``) of its partner, makes the loss and that row of the gradient
    NaN.  ``mix=None`` is ``kd_ce_loss_table``."""
    return _KDCELossMixFn.apply(student, None, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing)


class _KDBCELossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing, target_threshold, sum_classes):
        who = "kd_bce_loss"
        _need_cuda(student, who)
        if student.dim() != 2:
            raise RuntimeError(f"{who}: the student logits must be [B, C], got {tuple(student.shape)}")
        student = student.contiguous()
        B, C = student.shape
        dev = student.device
        if teacher is not None and table is not None:
            raise RuntimeError(f"{who}: a teacher tensor and a teacher table are mutually exclusive")
        tptr = bptr = iptr = None
        rows = 0
        if teacher is not None:
            teacher = teacher.contiguous().float()
            if teacher.shape != (B, C) or teacher.device != dev:
                raise RuntimeError(f"{who}: the teacher must be a [{B}, {C}] tensor on {dev}, got {tuple(teacher.shape)} on {teacher.device}")
            tptr = teacher.data_ptr()
        if table is not None:
            _need_cuda(table, who)
            if table.dim() != 2 or table.shape[1] != C or table.shape[0] < 1 or not table.is_contiguous() or table.device != dev:
                raise RuntimeError(f"{who}: the table must be a contiguous [rows, {C}] tensor on {dev}, got {tuple(table.shape)} on {table.device}")
            if index is None:
                raise RuntimeError(f"{who}: a teacher table needs an index")
            index = index.contiguous()
            if index.dtype != torch.int64 or index.shape != (B,) or index.device != dev:
                raise RuntimeError(f"{who}: index must be an int64 [{B}] tensor on {dev}")
            bptr, iptr, rows = table.data_ptr(), index.data_ptr(), table.shape[0]
        labels = labels.contiguous()
        if labels.dtype != torch.int64 or labels.shape != (B,) or labels.device != dev:
            raise RuntimeError(f"{who}: labels must be an int64 [{B}] tensor on {dev}")
        mptr = None
        if mix is not None:
            if mix.dtype != torch.int32 or tuple(mix.shape) != (B, 6) or not mix.is_contiguous() or mix.device != dev:
                raise RuntimeError(f"{who}: mix must be a contiguous int32 [{B}, 6] tensor on {dev}")
            mptr = mix.data_ptr()
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        partials = torch.empty(2 * B, dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(student)
        native.check(
            native.lib().qatvit_kd_bce_loss(student.data_ptr(), tptr, bptr, rows, iptr, labels.data_ptr(), mptr, B, C, float(kd_temp), float(kd_alpha),
                                            float(label_smoothing), -1.0 if target_threshold is None else float(target_threshold),
                                            int(bool(sum_classes)), partials.data_ptr(), out3.data_ptr(), dlogits.data_ptr(), native.stream_ptr()),
            "qatvit_kd_bce_loss",
        )
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(out3)
        return out3[0], out3

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * dloss,) + (None,) * 10


def kd_bce_loss(student, labels, teacher=None, table=None, index=None, mix=None, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1,
                target_threshold=None, sum_classes=False):
    """KD + binary cross-entropy with logits on smoothed, mixed targets (timm's ``BinaryCrossEntropy`` behind its ``Mixup``; the DeiT-III
    criterion): returns (loss, [loss, bce, kd*T^2]).  The hard target of row b is ``kd_ce_loss_mix``'s - ``lam`` on ``labels[b]``, ``1 - lam`` on
    the partner's label, smoothed to ``(1 - eps) * t + eps / C`` - used per class; ``target_threshold`` (None or negative: off) then turns it into
    ``t > threshold``.  The hard part is the mean over all ``B * C`` elements (``BCEWithLogitsLoss()``), or with ``sum_classes`` the sum over the
    classes and the mean over the batch.  ``teacher`` (``[B, C]``: its output on the mixed images) or ``table`` + ``index`` (the mixed soft label of
    ``kd_ce_loss_table_mix``) add the KD part with weight ``kd_alpha``, the hard part then has ``1 - kd_alpha``; with neither, the loss is the hard
    part.  An index outside the table makes the loss and that row of the gradient NaN; nothing here synchronises."""
    if target_threshold is not None and not isinstance(target_threshold, (int, float)):
        raise RuntimeError("kd_bce_loss: target_threshold must be None or a Python number (a tensor would have to be read on the host)")
    return _KDBCELossFn.apply(student, teacher, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing, target_threshold, sum_classes)
