"""Host restatement of the mix record (include/qatvit.h): qatvit_image_batch_mix on fp32 batches by separate numpy multiplies and an add, then
the box overwrite; qatvit_kd_ce_loss_mix in fp64 torch.  tests/test_mix_abi.py checks the drawing rule against the fields read here;
tests/test_gpu_mix.py and tests/test_gpu_loss_mix.py build their expectations with it."""
import numpy as np
import torch


def f32_bits(v):
    return int(np.float32(v).view(np.int32))


def bits_f32(w):
    return np.int32(w).view(np.float32)


def record(partner, w_self=1.0, w_partner=0.0, box=(0, 0, 0, 0), lam=1.0):
    """The six int32 words of one batch position; box = (y0, y1, x0, x1), each 0 .. 65535."""
    y0, y1, x0, x1 = box
    assert all(0 <= v <= 0xffff for v in box)
    pack = lambda lo, hi: int(np.uint32(lo | hi << 16).view(np.int32))   # noqa: E731
    return [int(partner), f32_bits(w_self), f32_bits(w_partner), pack(y0, y1), pack(x0, x1), f32_bits(lam)]


def mixup(partner, lam):
    """The record the host forms for mixup: w_self = fp32(lam), w_partner = fp32(1) - w_self."""
    lam = np.float32(lam)
    return record(partner, lam, np.float32(1) - lam, lam=lam)


def cutmix(partner, box, D):
    y0, y1, x0, x1 = (min(max(v, 0), D) for v in box)
    area = max(y1 - y0, 0) * max(x1 - x0, 0)
    return record(partner, 1.0, 0.0, box, np.float32(1.0 - area / float(D * D)))


def fields(rec, B, D=None):
    """(partner, w_self, w_partner, (y0, y1, x0, x1), lam) of one record as the kernels read it: the partner of position b resolved by the caller
    (`partner` is returned raw), the box clamped to [0, D] when D is given."""
    p, ws, wp, wy, wx, lam = (int(v) for v in rec)
    box = [wy & 0xffff, wy >> 16 & 0xffff, wx & 0xffff, wx >> 16 & 0xffff]
    if D is not None:
        box = [min(v, D) for v in box]
    return p, bits_f32(ws), bits_f32(wp), tuple(box), bits_f32(lam)


def partner_of(rec, b, B):
    p = int(rec[0])
    return p if 0 <= p < B else b


def mixed_images(X, records):
    """X fp32 [B, 3, D, D] (what the existing entries give per position), records int [B, 6] -> the mixed batch."""
    X = np.asarray(X, dtype=np.float32)
    B, D = X.shape[0], X.shape[-1]
    out = np.empty_like(X)
    for b, rec in enumerate(np.asarray(records).tolist()):
        p = partner_of(rec, b, B)
        _, ws, wp, (y0, y1, x0, x1), _ = fields(rec, B, D)
        a = (X[b] * np.float32(ws)).astype(np.float32)
        c = (X[p] * np.float32(wp)).astype(np.float32)
        out[b] = a + c
        if y1 > y0 and x1 > x0:
            out[b, :, y0:y1, x0:x1] = X[p, :, y0:y1, x0:x1]
    return out


def loss(student, labels, records=None, teacher=None, table=None, index=None, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1):
    """fp64: (loss, ce, kd * T^2).  `student` may require grad (then it is used as it is, a float64 tensor); everything else is converted.
    records None = no mixing.  1 - lam is formed in fp32, as the kernel forms it."""
    s = student if student.dtype == torch.float64 else student.detach().double().cpu()
    B, C = s.shape
    labels = torch.as_tensor(labels).cpu().long()
    recs = [record(b) for b in range(B)] if records is None else torch.as_tensor(records).cpu().tolist()
    part = torch.tensor([partner_of(r, b, B) for b, r in enumerate(recs)])
    lam32 = np.array([bits_f32(r[5]) for r in recs], dtype=np.float32)
    lam = torch.from_numpy(lam32.astype(np.float64))[:, None]
    oml = torch.from_numpy((np.float32(1) - lam32).astype(np.float64))[:, None]
    onehot = lambda y: torch.nn.functional.one_hot(y, C).double()   # noqa: E731
    t = lam * onehot(labels) + oml * onehot(labels[part])
    ysm = (1.0 - label_smoothing) * t + label_smoothing / C
    ce = -(ysm * torch.log_softmax(s, 1)).sum(1).mean()
    if teacher is None and table is None:
        return ce, ce, torch.zeros((), dtype=torch.float64)
    T = float(kd_temp)
    if teacher is not None:
        q = torch.softmax(teacher.detach().double().cpu() / T, 1)
    else:
        tab, idx = table.detach().double().cpu(), torch.as_tensor(index).cpu().long()
        q = torch.softmax(tab[idx] / T, 1)
        mixing = torch.from_numpy(lam32 != 1)[:, None]
        q = torch.where(mixing, lam * q + oml * torch.softmax(tab[idx[part]] / T, 1), q)
    logq = torch.where(q > 0, torch.log(q.clamp_min(1e-300)), torch.zeros_like(q))
    kd = (q * (logq - torch.log_softmax(s / T, 1))).sum(1).mean() * T * T
    return kd_alpha * kd + (1.0 - kd_alpha) * ce, ce, kd
