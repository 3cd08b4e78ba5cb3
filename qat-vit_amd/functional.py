"""torch.autograd glue over the per-op C ABI (include/qatvit.h).

torch is plumbing here: it owns device memory and streams; every arithmetic
step of these ops runs in libqatvit.so.  All functions require CUDA (HIP)
tensors and raise otherwise.
"""
from __future__ import annotations

import torch

from . import native


# the dtype codes of include/qatvit.h (QATVIT_EVAL_F16 / _BF16) for the entries that take 16-bit logits
_DTYPE16 = {torch.float16: 1, torch.bfloat16: 2}


def _need_cuda(t: torch.Tensor, what: str, half: bool = False) -> None:
    """``half``: the tensor is a fp16 / bf16 student of a class-parallel loss instead of a float32 one."""
    if not t.is_cuda:
        raise RuntimeError(f"{what}: qat-vit_amd ops run on MI355X only (got a {t.device} tensor); there is no CPU fallback")
    if half:
        if t.dtype not in _DTYPE16:
            raise RuntimeError(f"{what}: expected float16 or bfloat16, got {t.dtype}")
    elif t.dtype != torch.float32:
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


def _no_grad_scale(who, grad_scale):
    """The default (one thread per row) forms are float32 only: a ``grad_scale`` there is a mistake, not something to ignore."""
    if grad_scale is not None:
        raise RuntimeError(f"{who}: grad_scale belongs to a float16 / bfloat16 student, which this form (class_parallel=False) does not take")


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


def kd_ce_loss(student, teacher, labels, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1, class_parallel=False, grad_scale=None):
    """Returns (loss, [loss, ce, kd*T^2]).  ``teacher=None`` -> CE only
    (the reference's step at /root/reference/src/training/qat_trainer.py:343-349).  ``class_parallel=True``: the same loss by
    ``qatvit_kd_ce_loss_rows`` (see ``kd_ce_loss_mix``, also for a fp16 / bf16 student and ``grad_scale``)."""
    if class_parallel:
        out = _loss16("kd_ce_loss", student, grad_scale, teacher=teacher, labels=labels, kd_temp=kd_temp, kd_alpha=kd_alpha, label_smoothing=label_smoothing)
        if out is not None:
            return out
        return _KDCELossRowsFn.apply(student, teacher, None, None, labels, None, kd_temp, kd_alpha, label_smoothing, "kd_ce_loss")
    _no_grad_scale("kd_ce_loss", grad_scale)
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


def kd_ce_loss_table(student, table, index, labels, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1, class_parallel=False, grad_scale=None):
    """``kd_ce_loss(student, table[index], labels, ...)`` in one launch, without the gathered tensor: returns (loss, [loss, ce, kd*T^2]).
    ``table`` is fp32 ``[rows, C]`` (per-sample teacher logits, distill.TeacherLogitTable), ``index`` int64 ``[B]``.  An index outside the table
    makes the loss and that row of the gradient NaN; it is not an error on the host (nothing here synchronises).  ``class_parallel=True``: the same
    loss by ``qatvit_kd_ce_loss_rows`` (see ``kd_ce_loss_mix``)."""
    if class_parallel:
        out = _loss16("kd_ce_loss_table", student, grad_scale, table=table, index=index, labels=labels, kd_temp=kd_temp, kd_alpha=kd_alpha,
                      label_smoothing=label_smoothing)
        if out is not None:
            return out
        return _KDCELossRowsFn.apply(student, None, table, index, labels, None, kd_temp, kd_alpha, label_smoothing, "kd_ce_loss_table")
    _no_grad_scale("kd_ce_loss_table", grad_scale)
    return _KDCELossTableFn.apply(student, table, index, labels, kd_temp, kd_alpha, label_smoothing)


def _kd_ce_operands(who, student, teacher, table, index, labels, mix, half=False):
    """The argument checks the mixed CE forms share: (contiguous student, (teacher, table, index, labels, mix) addresses or None, table rows, the
    converted tensors, which the caller holds until its launch is enqueued).  ``half``: a fp16 / bf16 student (_KDLoss16Fn)."""
    _need_cuda(student, who, half)
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
    return student, (tptr, bptr, iptr, labels.data_ptr(), mptr), rows, (teacher, index, labels)


class _KDCELossMixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing):
        who = "kd_ce_loss_mix" if table is None else "kd_ce_loss_table_mix"
        student, (tptr, bptr, iptr, lptr, mptr), rows, keep = _kd_ce_operands(who, student, teacher, table, index, labels, mix)
        (B, C), dev = student.shape, student.device
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(student)
        native.check(
            native.lib().qatvit_kd_ce_loss_mix(student.data_ptr(), tptr, bptr, rows, iptr, lptr, mptr, B, C, float(kd_temp),
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


class _KDCELossRowsFn(torch.autograd.Function):
    """Every form of the KD + CE loss through qatvit_kd_ce_loss_rows: _KDCELossMixFn's checks, plus the partials workspace."""

    @staticmethod
    def forward(ctx, student, teacher, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing, who):
        student, (tptr, bptr, iptr, lptr, mptr), rows, keep = _kd_ce_operands(who, student, teacher, table, index, labels, mix)
        (B, C), dev = student.shape, student.device
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        partials = torch.empty(2 * B, dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(student)
        native.check(
            native.lib().qatvit_kd_ce_loss_rows(student.data_ptr(), tptr, bptr, rows, iptr, lptr, mptr, B, C, float(kd_temp),
                                                float(kd_alpha), float(label_smoothing), partials.data_ptr(), out3.data_ptr(), dlogits.data_ptr(),
                                                native.stream_ptr()),
            "qatvit_kd_ce_loss_rows",
        )
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(out3)
        return out3[0], out3

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * dloss,) + (None,) * 9


def kd_ce_loss_mix(student, teacher, labels, mix, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1, class_parallel=False, grad_scale=None):
    """``kd_ce_loss`` on a mixed batch: returns (loss, [loss, ce, kd*T^2]).  ``mix`` is the int32 ``[B, 6]`` record tensor the images were mixed
    with (data.MixupCutmix): row b's hard target is ``lam`` on ``labels[b]`` and ``1 - lam`` on the partner's label.  ``teacher`` (``[B, C]`` or
    None) is the teacher's output on the mixed images, so the KD part is ``kd_ce_loss``'s.  ``mix=None`` is ``kd_ce_loss``.

    ``class_parallel=True`` runs the same loss by ``qatvit_kd_ce_loss_rows``: a row's classes spread over one wave (``C <= 1024``) or one workgroup
    (up to ``C = 32768``; the default form stops at 4096) instead of one thread per row - the form for 100 classes and more.  Two launches instead of
    one, so at ``C = 10`` the default is the faster one.  Same arithmetic per element; the sums are added in another order, so the results agree to
    rounding, not bit for bit.

    The class-parallel forms also take a ``torch.float16`` / ``torch.bfloat16`` student, as a head under autocast returns it
    (``qatvit_kd_ce_loss_rows16`` and its siblings): the logits are up-cast exactly, the arithmetic is the fp32 entry's, and the gradient comes back
    in the student's dtype, rounded once.  ``grad_scale`` (a 0-dim float32 tensor on the device, e.g. ``scaler.scale(torch.ones((), device=dev))``)
    multiplies the gradient before that rounding - without it a fp16 gradient of ``(p - t) / B`` size is subnormal - and backward returns
    ``dlogits * (dloss / grad_scale)``: under ``scaler.scale(loss).backward()`` the factor is exactly 1.  The returned loss and ``out3`` stay float32
    and unscaled.  The default (``class_parallel=False``) forms stay float32 only."""
    if class_parallel:
        out = _loss16("kd_ce_loss_mix", student, grad_scale, teacher=teacher, labels=labels, mix=mix, kd_temp=kd_temp, kd_alpha=kd_alpha,
                      label_smoothing=label_smoothing)
        if out is not None:
            return out
        return _KDCELossRowsFn.apply(student, teacher, None, None, labels, mix, kd_temp, kd_alpha, label_smoothing, "kd_ce_loss_mix")
    _no_grad_scale("kd_ce_loss_mix", grad_scale)
    return _KDCELossMixFn.apply(student, teacher, None, None, labels, mix, kd_temp, kd_alpha, label_smoothing)


def kd_ce_loss_table_mix(student, table, index, labels, mix, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1, class_parallel=False, grad_scale=None):
    """``kd_ce_loss_table`` on a mixed batch: the hard target as in ``kd_ce_loss_mix``, the KD target
    ``lam * softmax(table[index[b]] / T) + (1 - lam) * softmax(table[index[p]] / T)`` - the usual mixed soft label, not the teacher's output on
    the mixed image.  An index outside the table, of the row or (where ``lam != 1``) of its partner, makes the loss and that row of the gradient
    NaN.  ``mix=None`` is ``kd_ce_loss_table``.  ``class_parallel=True``: the same loss by ``qatvit_kd_ce_loss_rows`` (see ``kd_ce_loss_mix``)."""
    if class_parallel:
        out = _loss16("kd_ce_loss_table_mix", student, grad_scale, table=table, index=index, labels=labels, mix=mix, kd_temp=kd_temp, kd_alpha=kd_alpha,
                      label_smoothing=label_smoothing)
        if out is not None:
            return out
        return _KDCELossRowsFn.apply(student, None, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing, "kd_ce_loss_table_mix")
    _no_grad_scale("kd_ce_loss_table_mix", grad_scale)
    return _KDCELossMixFn.apply(student, None, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing)


def teacher_topk(logits, k, kd_temp=4.0):
    """Teacher logits fp32 ``[B, C]`` -> the compressed rows ``(idx int16 [B, k], val fp32 [B, k], tail fp32 [B])`` of ``qatvit_teacher_topk_rows``:
    the k largest logits of a row in descending order (equal values lower class first) and the one logit ``tail`` that every other class is given, which
    keeps the tail's softmax mass at temperature ``kd_temp``.  ``1 <= k <= min(64, C - 1)``, ``2 <= C <= 32768``."""
    _need_cuda(logits, "teacher_topk")
    if logits.dim() != 2:
        raise RuntimeError(f"teacher_topk: the logits must be [B, C], got {tuple(logits.shape)}")
    logits = logits.contiguous()
    B, C = logits.shape
    idx = torch.empty(B, int(k), dtype=torch.int16, device=logits.device)
    val = torch.empty(B, int(k), dtype=torch.float32, device=logits.device)
    tail = torch.empty(B, dtype=torch.float32, device=logits.device)
    native.check(native.lib().qatvit_teacher_topk_rows(logits.data_ptr(), B, C, int(k), float(kd_temp), idx.data_ptr(), val.data_ptr(), tail.data_ptr(),
                                                       native.stream_ptr()), "qatvit_teacher_topk_rows")
    return idx, val, tail


class _KDCELossTopKFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, idx, val, tail, index, labels, mix, kd_temp, kd_alpha, label_smoothing):
        who = "kd_ce_loss_topk"
        student, (_, _, _, lptr, mptr), _, keep = _kd_ce_operands(who, student, None, None, None, labels, mix)
        (B, C), dev = student.shape, student.device
        rows, k = (idx.shape[0], idx.shape[1]) if idx.dim() == 2 else (0, 0)
        for name, t, dtype, shape in (("idx", idx, torch.int16, (rows, k)), ("val", val, torch.float32, (rows, k)), ("tail", tail, torch.float32, (rows,))):
            if t.dtype != dtype or tuple(t.shape) != shape or rows < 1 or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f"{who}: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        index = index.contiguous()
        if index.dtype != torch.int64 or index.shape != (B,) or index.device != dev:
            raise RuntimeError(f"{who}: index must be an int64 [{B}] tensor on {dev}")
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        partials = torch.empty(2 * B, dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(student)
        native.check(
            native.lib().qatvit_kd_ce_loss_topk(student.data_ptr(), idx.data_ptr(), val.data_ptr(), tail.data_ptr(), rows, k, index.data_ptr(), lptr, mptr,
                                                B, C, float(kd_temp), float(kd_alpha), float(label_smoothing), partials.data_ptr(), out3.data_ptr(),
                                                dlogits.data_ptr(), native.stream_ptr()),
            "qatvit_kd_ce_loss_topk",
        )
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(out3)
        return out3[0], out3

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * dloss,) + (None,) * 9


def kd_ce_loss_topk(student, idx, val, tail, index, labels, mix=None, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1, grad_scale=None):
    """``kd_ce_loss_table_mix(student, rows, index, labels, mix, ..., class_parallel=True)`` with ``rows`` the decompression of the compressed table
    ``(idx, val, tail)`` (``teacher_topk``; distill.TeacherTopKTable) - bit for bit, without the dense rows ever existing in global memory: the kernel
    decompresses the rows of a sample and, where ``lam != 1``, of its partner in LDS.  Returns (loss, [loss, ce, kd*T^2]); an index outside the
    table makes the loss and that row of the gradient NaN.  A fp16 / bf16 student and ``grad_scale``: as ``kd_ce_loss_mix`` states (there the result
    agrees with the fp32 form on the up-cast logits to rounding)."""
    out = _loss16("kd_ce_loss_topk", student, grad_scale, topk=(idx, val, tail), index=index, labels=labels, mix=mix, kd_temp=kd_temp, kd_alpha=kd_alpha,
                  label_smoothing=label_smoothing)
    if out is not None:
        return out
    return _KDCELossTopKFn.apply(student, idx, val, tail, index, labels, mix, kd_temp, kd_alpha, label_smoothing)


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
                target_threshold=None, sum_classes=False, grad_scale=None):
    """KD + binary cross-entropy with logits on smoothed, mixed targets (timm's ``BinaryCrossEntropy`` behind its ``Mixup``; the DeiT-III
    criterion): returns (loss, [loss, bce, kd*T^2]).  The hard target of row b is ``kd_ce_loss_mix``'s - ``lam`` on ``labels[b]``, ``1 - lam`` on
    the partner's label, smoothed to ``(1 - eps) * t + eps / C`` - used per class; ``target_threshold`` (None or negative: off) then turns it into
    ``t > threshold``.  The hard part is the mean over all ``B * C`` elements (``BCEWithLogitsLoss()``), or with ``sum_classes`` the sum over the
    classes and the mean over the batch.  ``teacher`` (``[B, C]``: its output on the mixed images) or ``table`` + ``index`` (the mixed soft label of
    ``kd_ce_loss_table_mix``) add the KD part with weight ``kd_alpha``, the hard part then has ``1 - kd_alpha``; with neither, the loss is the hard
    part.  An index outside the table makes the loss and that row of the gradient NaN; nothing here synchronises.  ``C <= 4096`` with a teacher of
    either dense kind; the hard part alone runs to ``C = 32768``, and a teacher above 4096 classes is a compressed table (``kd_bce_loss_topk``).
    The hard part alone above 4096 classes also takes a fp16 / bf16 student and ``grad_scale`` (see ``kd_ce_loss_mix``); every other form here is
    float32 only."""
    if target_threshold is not None and not isinstance(target_threshold, (int, float)):
        raise RuntimeError("kd_bce_loss: target_threshold must be None or a Python number (a tensor would have to be read on the host)")
    if teacher is None and table is None and student.dim() == 2 and student.shape[1] > 4096:
        # above the one-wave-per-row entry's 4096 classes the hard part runs class-parallel over a workgroup (qatvit_kd_bce_loss_topk without a table)
        out = _loss16("kd_bce_loss", student, grad_scale, labels=labels, mix=mix, kd_temp=kd_temp, kd_alpha=kd_alpha, label_smoothing=label_smoothing,
                      bce=(target_threshold, sum_classes))
        if out is not None:
            return out
        return _KDBCELossTopKFn.apply(student, None, None, None, None, labels, mix, kd_temp, kd_alpha, label_smoothing, target_threshold, sum_classes,
                                      "kd_bce_loss")
    if grad_scale is not None:
        raise RuntimeError("kd_bce_loss: grad_scale belongs to a float16 / bfloat16 student, which this form (a teacher, or up to 4096 classes) does not take")
    return _KDBCELossFn.apply(student, teacher, table, index, labels, mix, kd_temp, kd_alpha, label_smoothing, target_threshold, sum_classes)


class _KDBCELossTopKFn(torch.autograd.Function):
    """qatvit_kd_bce_loss_topk: _KDCELossTopKFn's checks of the compressed table (all of idx, val, tail, index, or none of them), the BCE arguments."""

    @staticmethod
    def forward(ctx, student, idx, val, tail, index, labels, mix, kd_temp, kd_alpha, label_smoothing, target_threshold, sum_classes, who):
        student, (_, _, _, lptr, mptr), _, keep = _kd_ce_operands(who, student, None, None, None, labels, mix)
        (B, C), dev = student.shape, student.device
        rows = k = 0
        ptrs = (None, None, None, None)
        if idx is not None:
            if val is None or tail is None or index is None:
                raise RuntimeError(f"{who}: a compressed table is idx, val and tail together, and needs an index")
            rows, k = (idx.shape[0], idx.shape[1]) if idx.dim() == 2 else (0, 0)
            for name, t, dtype, shape in (("idx", idx, torch.int16, (rows, k)), ("val", val, torch.float32, (rows, k)), ("tail", tail, torch.float32, (rows,))):
                if t.dtype != dtype or tuple(t.shape) != shape or rows < 1 or not t.is_contiguous() or t.device != dev:
                    raise RuntimeError(f"{who}: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            index = index.contiguous()
            if index.dtype != torch.int64 or index.shape != (B,) or index.device != dev:
                raise RuntimeError(f"{who}: index must be an int64 [{B}] tensor on {dev}")
            ptrs = (idx.data_ptr(), val.data_ptr(), tail.data_ptr(), index.data_ptr())
        elif val is not None or tail is not None:
            raise RuntimeError(f"{who}: val and tail without idx")
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        partials = torch.empty(2 * B, dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(student)
        native.check(
            native.lib().qatvit_kd_bce_loss_topk(student.data_ptr(), ptrs[0], ptrs[1], ptrs[2], rows, k, ptrs[3], lptr, mptr, B, C, float(kd_temp),
                                                 float(kd_alpha), float(label_smoothing), -1.0 if target_threshold is None else float(target_threshold),
                                                 int(bool(sum_classes)), partials.data_ptr(), out3.data_ptr(), dlogits.data_ptr(), native.stream_ptr()),
            "qatvit_kd_bce_loss_topk",
        )
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(out3)
        return out3[0], out3

    @staticmethod
    def backward(ctx, dloss, _):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * dloss,) + (None,) * 12


def kd_bce_loss_topk(student, labels, idx=None, val=None, tail=None, index=None, mix=None, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1,
                     target_threshold=None, sum_classes=False, grad_scale=None):
    """``kd_bce_loss`` to 32768 classes with the teacher read from the compressed table ``(idx, val, tail)`` (``teacher_topk``;
    distill.TeacherTopKTable): returns (loss, [loss, bce, kd*T^2]).  The KD target is ``kd_bce_loss``'s on the decompressed rows, but evaluated from
    the rows' at most ``k`` (under a mix record ``2 k``) explicit classes and one constant for all the others - no dense teacher row exists, and the
    teacher's exp / log run once per entry; the result agrees with the dense evaluation to rounding.  Without a table (``idx=None``) it is the hard part
    alone: plain BCE at any class count to 32768.  An index outside the table makes the loss and that row of the gradient NaN; nothing synchronises.
    A fp16 / bf16 student and ``grad_scale``: as ``kd_ce_loss_mix`` states."""
    if target_threshold is not None and not isinstance(target_threshold, (int, float)):
        raise RuntimeError("kd_bce_loss_topk: target_threshold must be None or a Python number (a tensor would have to be read on the host)")
    if idx is None and (val is not None or tail is not None):
        raise RuntimeError("kd_bce_loss_topk: val and tail without idx")
    out = _loss16("kd_bce_loss_topk", student, grad_scale, topk=None if idx is None else (idx, val, tail), index=index, labels=labels, mix=mix,
                  kd_temp=kd_temp, kd_alpha=kd_alpha, label_smoothing=label_smoothing, bce=(target_threshold, sum_classes))
    if out is not None:
        return out
    return _KDBCELossTopKFn.apply(student, idx, val, tail, index, labels, mix, kd_temp, kd_alpha, label_smoothing, target_threshold, sum_classes,
                                  "kd_bce_loss_topk")


class _KDLoss16Fn(torch.autograd.Function):
    """The class-parallel losses on a fp16 / bf16 student (qatvit_kd_ce_loss_rows16, qatvit_kd_ce_loss_topk16, qatvit_kd_bce_loss_topk16): the checks
    of the fp32 Functions, one entry chosen from what is given - ``bce = (target_threshold, sum_classes)``: the BCE entry (``topk`` optional);
    ``topk = (idx, val, tail)``: the compressed-table CE entry; else the rows entry with ``teacher`` / ``table`` / neither.  ``dlogits`` has the
    student's dtype and holds ``grad_scale`` times the gradient; backward undoes the factor on ``dloss``, so nothing here reads the scale on the host."""

    @staticmethod
    def forward(ctx, student, who, teacher, table, topk, index, labels, mix, kd_temp, kd_alpha, label_smoothing, bce, grad_scale):
        student, (tptr, bptr, iptr, lptr, mptr), rows, keep = _kd_ce_operands(who, student, teacher, table, index, labels, mix, half=True)
        (B, C), dev = student.shape, student.device
        if grad_scale is not None and (grad_scale.dtype != torch.float32 or grad_scale.numel() != 1 or grad_scale.device != dev):
            raise RuntimeError(f"{who}: grad_scale must be a float32 scalar tensor on {dev}")
        k = 0
        ptrs = (None, None, None)
        if topk is not None:
            idx, val, tail = topk
            if idx is None or val is None or tail is None or index is None:
                raise RuntimeError(f"{who}: a compressed table is idx, val and tail together, and needs an index")
            rows, k = (idx.shape[0], idx.shape[1]) if idx.dim() == 2 else (0, 0)
            for name, t, dtype, shape in (("idx", idx, torch.int16, (rows, k)), ("val", val, torch.float32, (rows, k)), ("tail", tail, torch.float32, (rows,))):
                if t.dtype != dtype or tuple(t.shape) != shape or rows < 1 or not t.is_contiguous() or t.device != dev:
                    raise RuntimeError(f"{who}: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            index = index.contiguous()
            if index.dtype != torch.int64 or index.shape != (B,) or index.device != dev:
                raise RuntimeError(f"{who}: index must be an int64 [{B}] tensor on {dev}")
            ptrs, iptr = (idx.data_ptr(), val.data_ptr(), tail.data_ptr()), index.data_ptr()
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        partials = torch.empty(2 * B, dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(student)
        L, code = native.lib(), _DTYPE16[student.dtype]
        gptr = None if grad_scale is None else grad_scale.data_ptr()
        common = (lptr, mptr, B, C, float(kd_temp), float(kd_alpha), float(label_smoothing))
        tails = (gptr, partials.data_ptr(), out3.data_ptr(), dlogits.data_ptr(), native.stream_ptr())
        if bce is not None:
            thr, sum_classes = bce
            native.check(L.qatvit_kd_bce_loss_topk16(student.data_ptr(), code, *ptrs, rows, k, iptr, *common, -1.0 if thr is None else float(thr),
                                                     int(bool(sum_classes)), *tails), "qatvit_kd_bce_loss_topk16")
        elif topk is not None:
            native.check(L.qatvit_kd_ce_loss_topk16(student.data_ptr(), code, *ptrs, rows, k, iptr, *common, *tails), "qatvit_kd_ce_loss_topk16")
        else:
            native.check(L.qatvit_kd_ce_loss_rows16(student.data_ptr(), code, tptr, bptr, rows, iptr, *common, *tails), "qatvit_kd_ce_loss_rows16")
        ctx.save_for_backward(dlogits, *(() if grad_scale is None else (grad_scale,)))
        ctx.mark_non_differentiable(out3)
        return out3[0], out3

    @staticmethod
    def backward(ctx, dloss, _):
        dlogits, *scale = ctx.saved_tensors
        return (dlogits * (dloss / scale[0] if scale else dloss),) + (None,) * 12


def _loss16(who, student, grad_scale, teacher=None, table=None, topk=None, index=None, labels=None, mix=None, kd_temp=4.0, kd_alpha=0.5,
            label_smoothing=0.1, bce=None):
    """None for a float32 student (which takes no ``grad_scale``), else the loss of _KDLoss16Fn."""
    if student.dtype not in _DTYPE16:
        if grad_scale is not None:
            raise RuntimeError(f"{who}: grad_scale belongs to a float16 / bfloat16 student; a float32 gradient needs no scale")
        return None
    return _KDLoss16Fn.apply(student, who, teacher, table, topk, index, labels, mix, kd_temp, kd_alpha, label_smoothing, bce, grad_scale)
