"""Criterion modules over the native loss entries (functional.py)."""
from __future__ import annotations

import torch

from . import functional as F


class BinaryCrossEntropy(torch.nn.Module):
    """timm's ``BinaryCrossEntropy(smoothing, target_threshold, sum_classes=...)`` on integer labels and the mix records of a mixing loader
    instead of a dense ``[B, C]`` target: ``crit(logits, labels, mix=None)`` returns the loss, one native launch pair for the forward and the
    gradient (``F.kd_bce_loss`` without a teacher).  ``labels`` int64 ``[B]``, ``mix`` the int32 ``[B, 6]`` records the images were mixed with
    (``MixupCutmix``) or None.  No ``weight`` / ``pos_weight``; fp32 logits on the GPU only."""

    def __init__(self, smoothing=0.1, target_threshold=None, sum_classes=False):
        super().__init__()
        smoothing = float(smoothing)
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"smoothing must be in [0, 1), got {smoothing}")
        if target_threshold is not None:
            target_threshold = float(target_threshold)
            if not 0.0 <= target_threshold < 1.0:   # (NaN fails both)
                raise ValueError(f"target_threshold must be None or in [0, 1), got {target_threshold}")
        self.smoothing, self.target_threshold, self.sum_classes = smoothing, target_threshold, bool(sum_classes)

    def forward(self, logits, labels, mix=None):
        return F.kd_bce_loss(logits, labels, mix=mix, label_smoothing=self.smoothing, target_threshold=self.target_threshold,
                             sum_classes=self.sum_classes)[0]

    def extra_repr(self):
        return f"smoothing={self.smoothing}, target_threshold={self.target_threshold}, sum_classes={self.sum_classes}"
