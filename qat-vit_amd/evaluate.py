"""Validation on MI355X (libqatvit.so: qatvit_eval_accumulate).

Stands where the reference has ``evaluate_fp32`` (qat_trainer.py:49-61), ``_eval_acc_limited`` of the Optuna objective and ``evaluate_model``
(evaluator.py): ``argmax``, ``==`` and ``.sum().item()`` per batch, one host round trip each.  Here one launch per batch adds the batch's counts
(accuracy, cross-entropy, confusion matrix, agreement with a second model) to a small block on the device, and ``result()`` copies that block to
the host once.  There is no CPU path: CPU tensors raise."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from . import native
from .distill import TeacherLogitTable

STATE_WORDS = 10   # QATVIT_EVAL_STATE_WORDS: nine int64 counters, then the double loss sum
COUNTERS = ("total", "correct", "bad_labels", "nonfinite_rows", "other_rows_seen", "agree", "other_correct", "bad_index", "loss_rows")
DTYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


class EvalResult:
    """What an evaluation counted.  ``accuracy`` is the reference's ``100.0 * correct / max(1, total)`` (0.0 for an empty evaluation);
    ``loss`` is the mean cross-entropy (no smoothing) over the ``loss_rows`` rows that have a valid label and a finite loss - ``loss_sum`` is their
    sum - or NaN if there is none; ``nonfinite_rows`` / ``bad_labels`` / ``bad_index`` count what was left out and why.  ``agree``, ``agreement``
    (per cent of the ``other_rows_seen`` rows compared) and ``other_correct`` describe the second opinion and are None when none was ever given.
    ``confusion`` is a CPU int64 ``[C, C]`` tensor (rows: label, columns: prediction) or None, ``per_class_accuracy`` its diagonal over its row
    sums in per cent (NaN for a class without samples)."""

    def __init__(self, state: torch.Tensor, confusion: Optional[torch.Tensor] = None, had_other: bool = False):
        if state.dtype != torch.int64 or state.shape != (STATE_WORDS,) or state.is_cuda:
            raise ValueError(f"state must be a CPU int64 [{STATE_WORDS}] tensor")
        for name, v in zip(COUNTERS, state[:len(COUNTERS)].tolist()):
            setattr(self, name, int(v))
        self.loss_sum = float(state[len(COUNTERS):].view(torch.float64)[0])
        self.accuracy = 100.0 * self.correct / max(1, self.total)
        self.loss = self.loss_sum / self.loss_rows if self.loss_rows else math.nan
        if had_other:
            self.agreement = 100.0 * self.agree / max(1, self.other_rows_seen)
        else:
            self.agree = self.agreement = self.other_correct = None
        self.confusion = confusion
        self.per_class_accuracy = None
        if confusion is not None:
            self.per_class_accuracy = 100.0 * confusion.diagonal().double() / confusion.sum(1).double()   # 0 / 0 -> NaN

    def __repr__(self):
        other = "" if self.agree is None else f", agree={self.agree}, other_correct={self.other_correct}"
        return (f"EvalResult(total={self.total}, correct={self.correct}, accuracy={self.accuracy:.4f}, loss={self.loss:.6f}, nonfinite_rows={self.nonfinite_rows}, "
                f"bad_labels={self.bad_labels}, bad_index={self.bad_index}{other})")


def _need_cuda(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what}: qat-vit_amd ops run on MI355X only (got {where}); there is no CPU fallback")


class EvalAccumulator:
    """The state block of one evaluation and, with ``confusion=True``, its ``[C, C]`` matrix, both in one device buffer (allocated by the first
    ``update``).  ``update`` is one launch and no host synchronisation; ``result`` is one device-to-host copy."""

    def __init__(self, num_classes: int, device="cuda", confusion: bool = True):
        self.num_classes = int(num_classes)
        if self.num_classes < 2:
            raise ValueError(f"num_classes {num_classes} (at least 2)")
        self.device = torch.device(device)
        self.with_confusion = bool(confusion)
        self._buf: Optional[torch.Tensor] = None
        self._had_other = False

    def _words(self) -> int:
        return STATE_WORDS + (self.num_classes ** 2 if self.with_confusion else 0)

    def reset(self) -> None:
        """Clears every count (a fill on the current stream, no synchronisation)."""
        if self._buf is not None:
            self._buf.zero_()
        self._had_other = False

    def update(self, logits: torch.Tensor, labels: torch.Tensor, other=None, other_index: Optional[torch.Tensor] = None) -> None:
        """Adds one batch.  `logits` fp32 / fp16 / bf16 ``[B, C]`` with ``stride(1) == 1`` (a column slice of a wider buffer is read in place),
        `labels` int64 ``[B]``.  `other`: fp32 logits of a second model for the same samples, ``[B, C]``, or - with `other_index` int64 ``[B]`` -
        a per-sample table ``[rows, C]`` or a ``TeacherLogitTable``, read at row ``other_index[b]``."""
        C = self.num_classes
        _need_cuda(logits, "EvalAccumulator.update")
        _need_cuda(labels, "EvalAccumulator.update")
        if self.device.type != "cuda":
            raise RuntimeError(f"EvalAccumulator.update: qat-vit_amd ops run on MI355X only (the accumulator is on {self.device}); there is no CPU fallback")
        if logits.dtype not in DTYPE_CODES:
            raise TypeError(f"logits must be float32, float16 or bfloat16, got {logits.dtype}")
        if logits.dim() != 2 or logits.shape[1] != C:
            raise ValueError(f"logits must be [B, {C}], got {tuple(logits.shape)}")
        B = logits.shape[0]
        if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < C):
            raise ValueError(f"logits must have stride(1) == 1 and a row stride of at least {C}, got strides {logits.stride()}")
        dev = logits.device
        if labels.dtype != torch.int64 or labels.shape != (B,) or labels.device != dev:
            raise ValueError(f"labels must be an int64 [{B}] tensor on {dev}, got {labels.dtype} {tuple(labels.shape)} on {labels.device}")
        optr = iptr = None
        old, rows = C, 0
        if isinstance(other, TeacherLogitTable):
            if other_index is None:
                raise ValueError("a TeacherLogitTable is read at one row per sample: pass other_index (GpuImageLoader(..., return_index=True) yields it)")
            other._need_device("rows")
            other.check_fresh()
            other = other.logits
        if other is not None:
            _need_cuda(other, "EvalAccumulator.update")
            want = f"[rows, {C}]" if other_index is not None else f"[{B}, {C}]"
            if other.dtype != torch.float32 or other.dim() != 2 or other.shape[1] != C or other.device != dev or (other_index is None and other.shape[0] != B):
                raise ValueError(f"other must be a float32 {want} tensor on {dev}, got {other.dtype} {tuple(other.shape)} on {other.device}")
            if other.shape[0] < 1 or other.stride(1) != 1 or (other.shape[0] > 1 and other.stride(0) < C):
                raise ValueError(f"other must have at least one row, stride(1) == 1 and a row stride of at least {C}, got strides {other.stride()}")
            old = max(other.stride(0), C)
            if other_index is not None:
                if other_index.dtype != torch.int64 or other_index.shape != (B,) or other_index.device != dev:
                    raise ValueError(f"other_index must be an int64 [{B}] tensor on {dev}")
                other_index = other_index.contiguous()
                iptr, rows = other_index.data_ptr(), other.shape[0]
            optr = other.data_ptr()
        elif other_index is not None:
            raise ValueError("other_index given without other")
        home = self._buf.device if self._buf is not None else self.device
        if home != dev and not (self._buf is None and home.index is None):
            raise ValueError(f"this accumulator counts on {home}, the batch is on {dev}")
        if self._buf is None:
            self._buf = torch.zeros(self._words(), dtype=torch.int64, device=dev)
        if B == 0:
            return
        labels = labels.contiguous()
        self._had_other |= optr is not None
        cptr = self._buf[STATE_WORDS:].data_ptr() if self.with_confusion else None
        with torch.cuda.device(dev):
            native.check(native.lib().qatvit_eval_accumulate(logits.data_ptr(), DTYPE_CODES[logits.dtype], max(logits.stride(0), C), labels.data_ptr(), B, C,
                                                             optr, old, iptr, rows, self._buf.data_ptr(), cptr, native.stream_ptr()),
                         "qatvit_eval_accumulate")

    def result(self) -> EvalResult:
        """The counts so far: one device-to-host copy (the only synchronisation of an evaluation)."""
        C = self.num_classes
        host = self._buf.cpu() if self._buf is not None else torch.zeros(self._words(), dtype=torch.int64)
        conf = host[STATE_WORDS:].view(C, C) if self.with_confusion else None
        return EvalResult(host[:STATE_WORDS], conf, self._had_other)


def _device_of(model, device):
    if device is not None:
        return torch.device(device)
    if isinstance(model, nn.Module):
        p = next(model.parameters(), None)
        if p is not None:
            return p.device
    return torch.device(getattr(model, "device", "cuda"))


@torch.no_grad()
def evaluate(model, loader, max_batches: Optional[int] = None, other=None, device=None, confusion: bool = True) -> EvalResult:
    """The body of the reference's ``evaluate_fp32`` / ``_eval_acc_limited``: ``evaluate(model, loader).accuracy`` is their return value, with one
    host synchronisation per evaluation instead of one per batch.

    `model` is any callable from images to ``[B, C]`` logits (fp32, fp16 or bf16): the prepared QAT wrapper, a ``native_float`` wrapper (also
    inside ``torch.autocast``), the native teacher, an ``Int8Student``, a stock module on the GPU, a DDP wrapper of one.  An ``nn.Module`` is put
    into ``eval()`` for the pass and every module's ``training`` flag is restored afterwards; the pass runs under ``torch.no_grad()``, issues no
    collective (evaluation on rank 0 only keeps working) and leaves no ``.grad`` behind.  `loader` yields ``(images, labels)`` or
    ``(images, labels, index)``; CPU batches of a stock ``DataLoader`` are moved with ``non_blocking=True``.  `other` is a second callable run on
    the same batch, or a ``TeacherLogitTable`` (then the loader must yield the indices: ``GpuImageLoader(..., return_index=True)``); the result
    then says on how many samples the two agree.  `max_batches` stops after that many batches.  `device` defaults to the model's.

    Evaluating a prepared QAT model whose observers are enabled MOVES them, as it does in the reference: ATen's fused fake-quant op does not
    look at ``training``, and the native engine mirrors that.  Apply ``disable_observer`` first where that is not wanted."""
    dev = _device_of(model, device)
    if dev.type != "cuda":
        raise RuntimeError(f"evaluate: qat-vit_amd ops run on MI355X only (the model is on {dev}); there is no CPU fallback")
    is_table = isinstance(other, TeacherLogitTable)
    modules = [m for m in (model, None if is_table else other) if isinstance(m, nn.Module)]
    flags = [(s, s.training) for m in modules for s in m.modules()]
    for m in modules:
        m.eval()
    acc = None
    try:
        for k, batch in enumerate(loader):
            if max_batches is not None and k >= max_batches:
                break
            if len(batch) not in (2, 3):
                raise ValueError(f"the loader must yield (images, labels) or (images, labels, index), got {len(batch)} items")
            images, labels = batch[0].to(dev, non_blocking=True), batch[1].to(dev, non_blocking=True)
            index = batch[2].to(dev, non_blocking=True) if len(batch) == 3 else None
            if is_table and index is None:
                raise ValueError("evaluate(other=TeacherLogitTable) needs a loader that yields (images, labels, index): "
                                 "GpuImageLoader(..., return_index=True)")
            logits = model(images)
            if acc is None:
                acc = EvalAccumulator(logits.shape[-1], device=logits.device, confusion=confusion)
            if is_table:
                acc.update(logits, labels, other, index)
            elif other is not None:
                acc.update(logits, labels, other(images).float())
            else:
                acc.update(logits, labels)
    finally:
        for s, t in flags:
            s.training = t
    if acc is None:   # an empty loader: the reference returns 0.0
        return EvalResult(torch.zeros(STATE_WORDS, dtype=torch.int64), None, other is not None)
    return acc.result()
