"""Validation on MI355X (libqatvit.so: qatvit_eval_accumulate, qatvit_eval_accumulate_rank; DESIGN.md sections 7j and 7zc).

Stands where the reference has ``evaluate_fp32`` (qat_trainer.py:49-61), ``_eval_acc_limited`` of the Optuna objective and ``evaluate_model``
(evaluator.py): ``argmax``, ``==`` and ``.sum().item()`` per batch, one host round trip each.  Here one launch per batch adds the batch's counts
(accuracy, cross-entropy, confusion matrix, agreement with a second model) to a small block on the device, and ``result()`` copies that block to
the host once.  With ``topk=``, ``label_smoothing=`` or ``per_class=`` a second, class-parallel launch (csrc/eval_rank.hip) adds the histogram of the
label's rank - every top-k at once -, the label-smoothed loss and per-class counts to a second block of the same buffer.  There is no CPU path: CPU
tensors raise."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from . import native
from .distill import TeacherLogitTable

STATE_WORDS = 10   # QATVIT_EVAL_STATE_WORDS: nine int64 counters, then the double loss sum
COUNTERS = ("total", "correct", "bad_labels", "nonfinite_rows", "other_rows_seen", "agree", "other_correct", "bad_index", "loss_rows")
RANK_BINS = 32          # QATVIT_EVAL_RANK_BINS: ranks 0 .. 30 and "31 or more"
RANK_STATE_WORDS = 74   # QATVIT_EVAL_RANK_STATE_WORDS: seven int64 counters, a zero, the double loss sum, a zero, two histograms of RANK_BINS
RANK_COUNTERS = ("total", "bad_labels", "nonfinite_rows", "loss_rows", "other_rows_seen", "agree", "bad_index")
DTYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


class EvalResult:
    """What an evaluation counted.  ``accuracy`` is the reference's ``100.0 * correct / max(1, total)`` (0.0 for an empty evaluation);
    ``loss`` is the mean cross-entropy (no smoothing) over the ``loss_rows`` rows that have a valid label and a finite loss - ``loss_sum`` is their
    sum - or NaN if there is none; ``nonfinite_rows`` / ``bad_labels`` / ``bad_index`` count what was left out and why.  ``agree``, ``agreement``
    (per cent of the ``other_rows_seen`` rows compared) and ``other_correct`` describe the second opinion and are None when none was ever given.
    ``confusion`` is a CPU int64 ``[C, C]`` tensor (rows: label, columns: prediction) or None, ``per_class_accuracy`` its diagonal over its row
    sums in per cent (NaN for a class without samples).

    With a rank block (``EvalAccumulator(topk=..., label_smoothing=..., per_class=...)``), else None: ``rank_hist`` is a CPU int64 ``[32]`` tensor,
    bin r the valid-label rows whose label has rank r (the number of columns that beat it in torch.argmax's order: larger, or equal at a lower
    index), bin 31 every rank from 31 up; ``topk_accuracy`` maps each requested k to ``100 * rank_hist[:k].sum() / max(1, valid labels)`` - a tied
    label is inside the top k by the argmax order, not by ``torch.topk``'s undocumented one; ``smoothed_loss`` is the mean label-smoothed
    cross-entropy over the rank block's finite rows (``smoothed_loss_sum`` their sum, last bits order-dependent; NaN if there is none);
    ``per_class_recall`` (with ``per_class=True``) is a double ``[C]`` tensor in per cent, NaN for a class without samples, and ``class_counts`` the
    int64 ``[2, C]`` counts (samples, top-1 hits) behind it; ``other_rank_hist`` / ``other_topk_accuracy`` say the same of the second opinion."""

    def __init__(self, state: torch.Tensor, confusion: Optional[torch.Tensor] = None, had_other: bool = False, rank: Optional[torch.Tensor] = None,
                 class_counts: Optional[torch.Tensor] = None, topk=()):
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
        self.rank_hist = self.topk_accuracy = self.smoothed_loss = self.smoothed_loss_sum = self.other_rank_hist = self.other_topk_accuracy = None
        self.class_counts, self.per_class_recall = class_counts, None
        if rank is not None:
            if rank.dtype != torch.int64 or rank.shape != (RANK_STATE_WORDS,) or rank.is_cuda:
                raise ValueError(f"rank must be a CPU int64 [{RANK_STATE_WORDS}] tensor")
            self.rank_hist = rank[10:10 + RANK_BINS]
            self.topk_accuracy = _topk_percent(self.rank_hist, topk)
            self.smoothed_loss_sum = float(rank[8:9].view(torch.float64)[0])
            self.smoothed_loss = self.smoothed_loss_sum / int(rank[3]) if int(rank[3]) else math.nan
            if had_other:
                self.other_rank_hist = rank[10 + RANK_BINS:]
                self.other_topk_accuracy = _topk_percent(self.other_rank_hist, topk)
        if class_counts is not None:
            self.per_class_recall = 100.0 * class_counts[1].double() / class_counts[0].double()   # 0 / 0 -> NaN

    def __repr__(self):
        other = "" if self.agree is None else f", agree={self.agree}, other_correct={self.other_correct}"
        return (f"EvalResult(total={self.total}, correct={self.correct}, accuracy={self.accuracy:.4f}, loss={self.loss:.6f}, nonfinite_rows={self.nonfinite_rows}, "
                f"bad_labels={self.bad_labels}, bad_index={self.bad_index}{other})")


def _topk_percent(hist: torch.Tensor, topk) -> dict:
    valid = max(1, int(hist.sum()))
    return {k: 100.0 * int(hist[:k].sum()) / valid for k in topk}


def _check_topk(topk) -> tuple:
    """`topk` as a tuple of ints in 1 .. 31 (None: empty); anything else raises ValueError."""
    if topk is None:
        return ()
    if not isinstance(topk, (tuple, list)) or not topk:
        raise ValueError(f"topk must be None or a non-empty tuple of ints in 1 .. {RANK_BINS - 1}, got {topk!r}")
    for k in topk:
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= RANK_BINS - 1:
            raise ValueError(f"topk entries must be ints in 1 .. {RANK_BINS - 1} (ranks from {RANK_BINS - 1} up share one bin), got {k!r}")
    return tuple(topk)


def _need_cuda(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what}: qat-vit_amd ops run on MI355X only (got {where}); there is no CPU fallback")


class EvalAccumulator:
    """The state block of one evaluation and, with ``confusion=True``, its ``[C, C]`` matrix, both in one device buffer (allocated by the first
    ``update``).  ``update`` is one launch and no host synchronisation; ``result`` is one device-to-host copy.

    `topk` (a tuple of ints in 1 .. 31), `label_smoothing` (in [0, 1)) and `per_class`: any of them makes ``update`` launch the class-parallel rank
    entry (``qatvit_eval_accumulate_rank``, at most 32768 classes) into a second state block - and, with `per_class`, ``[2, C]`` counts - of the same
    buffer, so ``result`` is still one copy.  ``confusion=True``, the default, still launches the older entry as well, with its ``[C, C]`` matrix
    (8 MB at 1000 classes, 8.6 GB at 32768): pass ``confusion=False`` at many classes.  Then the rank entry is the only launch, the older
    counters of the result are filled from its block (``correct = rank_hist[0]``, ``other_correct = other_rank_hist[0]``) and ``loss`` is the
    smoothed loss where `label_smoothing` is 0 and NaN otherwise (``smoothed_loss`` always has it).  With all three at their defaults nothing
    changes: the same launch, buffer and result as before.  Under data parallelism each rank counts its own shard; adding the state blocks is the
    caller's reduction."""

    def __init__(self, num_classes: int, device="cuda", confusion: bool = True, topk=None, label_smoothing: float = 0.0, per_class: bool = False):
        self.num_classes = int(num_classes)
        if self.num_classes < 2:
            raise ValueError(f"num_classes {num_classes} (at least 2)")
        self.device = torch.device(device)
        self.with_confusion = bool(confusion)
        self.topk = _check_topk(topk)
        self.label_smoothing = float(label_smoothing)
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"label_smoothing {label_smoothing} is outside [0, 1)")
        self.per_class = bool(per_class)
        self.with_rank = bool(self.topk) or self.label_smoothing != 0.0 or self.per_class
        if self.with_rank and self.num_classes > 32768:
            raise ValueError(f"topk / label_smoothing / per_class serve at most 32768 classes, got {self.num_classes}")
        self._buf: Optional[torch.Tensor] = None
        self._had_other = False

    def _words(self) -> int:
        return STATE_WORDS + (self.num_classes ** 2 if self.with_confusion else 0)

    def _rank_words(self) -> int:
        """Words behind ``_words()``: the rank block and the per-class counts."""
        return (RANK_STATE_WORDS + (2 * self.num_classes if self.per_class else 0)) if self.with_rank else 0

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
            self._buf = torch.zeros(self._words() + self._rank_words(), dtype=torch.int64, device=dev)
        if B == 0:
            return
        labels = labels.contiguous()
        self._had_other |= optr is not None
        cptr = self._buf[STATE_WORDS:].data_ptr() if self.with_confusion else None
        with torch.cuda.device(dev):
            if self.with_confusion or not self.with_rank:
                native.check(native.lib().qatvit_eval_accumulate(logits.data_ptr(), DTYPE_CODES[logits.dtype], max(logits.stride(0), C), labels.data_ptr(), B, C,
                                                                 optr, old, iptr, rows, self._buf.data_ptr(), cptr, native.stream_ptr()),
                             "qatvit_eval_accumulate")
            if self.with_rank:
                rank = self._buf.data_ptr() + 8 * self._words()   # the second block, then the [2, C] counts
                native.check(native.lib().qatvit_eval_accumulate_rank(logits.data_ptr(), DTYPE_CODES[logits.dtype], max(logits.stride(0), C), labels.data_ptr(),
                                                                      B, C, self.label_smoothing, optr, old, iptr, rows, rank,
                                                                      rank + 8 * RANK_STATE_WORDS if self.per_class else None, native.stream_ptr()),
                             "qatvit_eval_accumulate_rank")

    def result(self) -> EvalResult:
        """The counts so far: one device-to-host copy (the only synchronisation of an evaluation)."""
        C = self.num_classes
        host = self._buf.cpu() if self._buf is not None else torch.zeros(self._words() + self._rank_words(), dtype=torch.int64)
        conf = host[STATE_WORDS:self._words()].view(C, C) if self.with_confusion else None
        if not self.with_rank:
            return EvalResult(host[:STATE_WORDS], conf, self._had_other)
        rank = host[self._words():self._words() + RANK_STATE_WORDS]
        counts = host[self._words() + RANK_STATE_WORDS:].view(2, C) if self.per_class else None
        state = host[:STATE_WORDS]
        if not self.with_confusion:   # the older entry did not run: its counters from the rank block
            named = dict(zip(RANK_COUNTERS, rank.tolist()), correct=int(rank[10]), other_correct=int(rank[10 + RANK_BINS]))
            if self.label_smoothing != 0.0:
                named["loss_rows"] = 0
            state = torch.tensor([named[n] for n in COUNTERS] + [int(rank[8]) if self.label_smoothing == 0.0 else 0], dtype=torch.int64)
        return EvalResult(state, conf, self._had_other, rank, counts, self.topk)


def _device_of(model, device):
    if device is not None:
        return torch.device(device)
    if isinstance(model, nn.Module):
        p = next(model.parameters(), None)
        if p is not None:
            return p.device
    return torch.device(getattr(model, "device", "cuda"))


@torch.no_grad()
def evaluate(model, loader, max_batches: Optional[int] = None, other=None, device=None, confusion: bool = True, topk=None, label_smoothing: float = 0.0,
             per_class: bool = False) -> EvalResult:
    """The body of the reference's ``evaluate_fp32`` / ``_eval_acc_limited``: ``evaluate(model, loader).accuracy`` is their return value, with one
    host synchronisation per evaluation instead of one per batch.

    `model` is any callable from images to ``[B, C]`` logits (fp32, fp16 or bf16): the prepared QAT wrapper, a ``native_float`` wrapper (also
    inside ``torch.autocast``), the native teacher, an ``Int8Student``, a stock module on the GPU, a DDP wrapper of one.  An ``nn.Module`` is put
    into ``eval()`` for the pass and every module's ``training`` flag is restored afterwards; the pass runs under ``torch.no_grad()``, issues no
    collective (evaluation on rank 0 only keeps working) and leaves no ``.grad`` behind.  `loader` yields ``(images, labels)`` or
    ``(images, labels, index)``; CPU batches of a stock ``DataLoader`` are moved with ``non_blocking=True``.  `other` is a second callable run on
    the same batch, or a ``TeacherLogitTable`` (then the loader must yield the indices: ``GpuImageLoader(..., return_index=True)``); the result
    then says on how many samples the two agree.  `max_batches` stops after that many batches.  `device` defaults to the model's.  `confusion`, `topk`,
    `label_smoothing` and `per_class` are ``EvalAccumulator``'s: ``evaluate(model, loader, confusion=False, topk=(1, 5), label_smoothing=0.1)`` is the
    recipes' ``accuracy(output, target, topk=(1, 5))`` and smoothed validation loss.

    Evaluating a prepared QAT model whose observers are enabled MOVES them, as it does in the reference: ATen's fused fake-quant op does not
    look at ``training``, and the native engine mirrors that.  Apply ``disable_observer`` first where that is not wanted."""
    dev = _device_of(model, device)
    keywords = dict(confusion=confusion, topk=topk, label_smoothing=label_smoothing, per_class=per_class)
    EvalAccumulator(2, **keywords)   # a bad keyword raises here, before the model is touched
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
                acc = EvalAccumulator(logits.shape[-1], device=logits.device, **keywords)
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
        rank = torch.zeros(RANK_STATE_WORDS, dtype=torch.int64) if EvalAccumulator(2, **keywords).with_rank else None
        return EvalResult(torch.zeros(STATE_WORDS, dtype=torch.int64), None, other is not None, rank, None, _check_topk(topk))
    return acc.result()
