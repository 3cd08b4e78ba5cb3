"""Restatements of qatvit_kd_bce_loss (include/qatvit.h) in torch.  `loss` is the fp64 reference on the host: the targets built from the labels and
the mix records as the header states them, F.binary_cross_entropy_with_logits, and the KD term of tests/mix_ref.py.  `timm_target` builds the same
target the way timm's Mixup and BinaryCrossEntropy do (tests/test_bce_abi.py holds the two against each other).  `composition` is the objective as a
user would write it from torch ops on whatever device and dtype the logits have - the yardstick of tests/test_gpu_bce_loss.py for the fp32 rounding
at large C, never the reference."""
import numpy as np
import torch

from tests import mix_ref


def _records(records, B):
    recs = [mix_ref.record(b) for b in range(B)] if records is None else torch.as_tensor(records).cpu().tolist()
    part = torch.tensor([mix_ref.partner_of(r, b, B) for b, r in enumerate(recs)])
    lam32 = np.array([mix_ref.bits_f32(r[5]) for r in recs], dtype=np.float32)
    return part, lam32


def targets(labels, C, records=None, label_smoothing=0.1, target_threshold=None):
    """fp64 [B, C]: (1 - eps) * (lam * onehot(y) + (1 - lam) * onehot(y_p)) + eps / C, then `> target_threshold` where one is given (None or
    negative: off).  1 - lam is formed in fp32, as the kernel forms it."""
    labels = torch.as_tensor(labels).cpu().long()
    B = labels.shape[0]
    part, lam32 = _records(records, B)
    lam = torch.from_numpy(lam32.astype(np.float64))[:, None]
    oml = torch.from_numpy((np.float32(1) - lam32).astype(np.float64))[:, None]
    onehot = lambda y: torch.nn.functional.one_hot(y, C).double()   # noqa: E731
    t = (1.0 - label_smoothing) * (lam * onehot(labels) + oml * onehot(labels[part])) + label_smoothing / C
    if target_threshold is not None and target_threshold >= 0:
        t = (t > target_threshold).double()
    return t


def loss(student, labels, records=None, teacher=None, table=None, index=None, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1,
         target_threshold=None, sum_classes=False):
    """fp64: (loss, bce, kd * T^2).  `student` may require grad (then it is used as it is, a float64 tensor)."""
    s = student if student.dtype == torch.float64 else student.detach().double().cpu()
    B, C = s.shape
    t = targets(labels, C, records, label_smoothing, target_threshold)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(s, t, reduction="sum") / (B if sum_classes else B * C)
    if teacher is None and table is None:
        return bce, bce, torch.zeros((), dtype=torch.float64)
    kd = mix_ref.loss(s, labels, records, teacher=teacher, table=table, index=index, kd_temp=kd_temp, kd_alpha=kd_alpha,
                      label_smoothing=label_smoothing)[2]
    return kd_alpha * kd + (1.0 - kd_alpha) * bce, bce, kd


def timm_target(labels, C, lam=1.0, partner=None, smoothing=0.1, target_threshold=None):
    """timm.data.mixup.mixup_target followed by BinaryCrossEntropy's threshold, in fp64: one-hot with on = 1 - eps + eps / C and off = eps / C,
    y1 * lam + y2 * (1 - lam) with y2 the partner rows (timm: the flipped batch), then target.gt(threshold)."""
    labels = torch.as_tensor(labels).long()
    off = smoothing / C
    on = 1.0 - smoothing + off
    y1 = torch.full((labels.shape[0], C), off, dtype=torch.float64).scatter_(1, labels.view(-1, 1), on)
    y2 = y1.flip(0) if partner is None else y1[torch.as_tensor(partner).long()]
    lam = torch.as_tensor(lam, dtype=torch.float64).reshape(-1, 1)
    t = y1 * lam + y2 * (1.0 - lam)
    if target_threshold is not None:
        t = t.gt(target_threshold).double()
    return t


def composition(student, labels, mix=None, teacher=None, table=None, index=None, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1,
                target_threshold=None, sum_classes=False):
    """(loss, bce, kd * T^2) from stock torch ops in the dtype and on the device of `student`, nothing read on the host: smoothed one-hot, the mix by
    index_select, F.binary_cross_entropy_with_logits, the KD term.  `student` may require grad."""
    B, C = student.shape
    dt, dev = student.dtype, student.device
    ar = torch.arange(B, device=dev)
    if mix is None:
        part, lam = ar, torch.ones(B, dtype=dt, device=dev)
    else:
        p = mix[:, 0].long()
        part = torch.where((p >= 0) & (p < B), p, ar)
        lam = mix[:, 5].contiguous().view(torch.float32)
    oml = (1 - lam).to(dt)[:, None]                                # 1 - lam in fp32, as the records' weights are formed
    lam = lam.to(dt)[:, None]
    off = label_smoothing / C
    onehot = torch.full((B, C), off, dtype=dt, device=dev).scatter_(1, labels.view(-1, 1), 1.0 - label_smoothing + off)
    t = lam * onehot + oml * onehot.index_select(0, part)
    if target_threshold is not None:
        t = (t > target_threshold).to(dt)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(student, t, reduction="sum") / (B if sum_classes else B * C)
    if teacher is None and table is None:
        return bce, bce, torch.zeros((), dtype=dt, device=dev)
    T = float(kd_temp)
    if teacher is not None:
        q = torch.softmax(teacher.to(dt) / T, 1)
    else:
        q = torch.softmax(table.to(dt).index_select(0, index) / T, 1)
        q2 = torch.softmax(table.to(dt).index_select(0, index.index_select(0, part)) / T, 1)
        q = torch.where(lam != 1, lam * q + oml * q2, q)
    kd = (torch.xlogy(q, q) - q * torch.log_softmax(student / T, 1)).sum(1).mean() * T * T
    return kd_alpha * kd + (1.0 - kd_alpha) * bce, bce, kd
