"""Distillation from a per-sample table of teacher logits (libqatvit.so: qatvit_kd_ce_loss_table).

The reference loop feeds its frozen teacher un-augmented images (Resize + ToTensor + Normalize, nothing random), so the teacher's logits for
image i are the same in every epoch and in every search trial.  ``TeacherLogitTable.build`` runs the native teacher forward once over the data set
and keeps fp32 ``[N, num_classes]`` on the device; a training step then reads row ``index[b]`` inside the loss kernel instead of running the
teacher.  ``GpuImageLoader(..., return_index=True)`` supplies ``index``.

A table is only valid for the teacher weights, the teacher's arithmetic form, the data and the transform it was built from.  It is WRONG under
random augmentation of the teacher's input and for a teacher that trains; neither can be seen from here in general, so what can be detected is
refused: teacher parameters that require grad at build, teacher parameters replaced or modified since (``rows`` / ``loss`` raise), and any
mismatch between a saved table and what ``load`` is given.  The caller chooses the table; nothing selects it automatically.  Under data
parallelism every rank builds or loads the whole table for itself (CIFAR-10: 2 MB); no collective is involved.
"""
from __future__ import annotations

import hashlib
import weakref

import torch

from . import functional as F
from . import native
from .data import GpuResizeNormalize
from .vit import layer_scale_params

FORMAT = 1
FIELDS = ("N", "C", "teacher_form", "transform", "data_digest", "param_digest")


def transform_tuple(transform) -> tuple:
    """``(src_size, out_size, mean, std)`` of a ``GpuResizeNormalize`` (or of such a tuple itself), in plain Python numbers; of a
    ``GpuWideResizeNormalize``, ``((H, W), out_size, mean, std, (top, left, h, w))`` with its default window."""
    if isinstance(transform, (tuple, list)):
        src, out, mean, std = transform[:4]
        window = transform[4] if len(transform) > 4 else None
    else:
        src, out, mean, std = transform.src_size, transform.out_size, transform.mean, transform.std
        window = getattr(transform, "window", None)
    plain = (int(out), tuple(float(v) for v in mean), tuple(float(v) for v in std))
    if isinstance(src, (tuple, list)):
        # a GpuWideResizeNormalize: (H, W) in the place of the side, and behind the rest the default window, which decides what the teacher saw
        H, W = (int(v) for v in src)
        return ((H, W),) + plain + (tuple(int(v) for v in (window if window is not None else (0, 0, H, W))),)
    return (int(src),) + plain


def data_digest(data_u8, labels=None) -> str:
    """SHA-256 of the uint8 images (shape and bytes) and, when given, of the int64 labels; computed on the host."""
    data_u8 = torch.as_tensor(data_u8)
    if data_u8.dtype != torch.uint8:
        raise TypeError(f"images must be uint8, got {data_u8.dtype}")
    h = hashlib.sha256(repr(tuple(data_u8.shape)).encode())
    h.update(data_u8.detach().cpu().contiguous().numpy().tobytes())
    if labels is not None:
        h.update(b"labels")
        h.update(torch.as_tensor(labels).detach().to("cpu", torch.int64).contiguous().numpy().tobytes())
    return h.hexdigest()


def param_digest(teacher) -> str:
    """SHA-256 of the teacher's parameters in the order of the C ABI (native.vit_params); computed on the host."""
    h = hashlib.sha256()
    for p in native.vit_params(teacher) + layer_scale_params(teacher):   # (LayerScale gammas, where the teacher has them, behind the ABI's parameters)
        h.update(repr((tuple(p.shape), str(p.dtype))).encode())
        h.update(p.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def teacher_form(teacher) -> int:
    """The arithmetic form (teacher.py: 1, 2 or 3) a native engine built now for this teacher runs in, after the engine's own fall-backs."""
    from .teacher import TeacherEngine

    return TeacherEngine.resolve_passes(teacher, warn=False)


def _versions(teacher) -> tuple:
    return tuple((p.data_ptr(), p._version) for p in native.vit_params(teacher) + layer_scale_params(teacher))


class TeacherLogitTable:
    """fp32 ``[N, C]`` teacher logits of a data set, one row per sample, with the record of what they were computed from (see the module text
    for when a table is valid: fixed teacher, no random augmentation of the teacher's input)."""

    def __init__(self, logits: torch.Tensor, meta: dict, teacher=None):
        if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
            raise ValueError("logits must be a contiguous fp32 [N, C] tensor")
        missing = [k for k in FIELDS if k not in meta]
        if missing:
            raise ValueError(f"table record lacks {missing}")
        if (int(meta["N"]), int(meta["C"])) != tuple(logits.shape):
            raise ValueError(f"table record says [{meta['N']}, {meta['C']}], the logits are {tuple(logits.shape)}")
        self.logits = logits
        self.meta = dict(meta)
        self._teacher = weakref.ref(teacher) if teacher is not None else None
        self._teacher_versions = _versions(teacher) if teacher is not None else None

    N = property(lambda self: self.logits.shape[0])
    C = property(lambda self: self.logits.shape[1])
    device = property(lambda self: self.logits.device)

    def __len__(self):
        return self.logits.shape[0]

    @staticmethod
    def describe(teacher, data_u8, transform, labels=None, form=None) -> dict:
        """The record of a table over these inputs (digests are computed here, on the host: once per build / load, never per step)."""
        data_u8 = torch.as_tensor(data_u8)
        return {"format": FORMAT, "N": int(data_u8.shape[0]), "C": int(teacher.head.weight.shape[0]),
                "teacher_form": int(teacher_form(teacher) if form is None else form), "transform": transform_tuple(transform),
                "data_digest": data_digest(data_u8, labels), "param_digest": param_digest(teacher)}

    @classmethod
    def build(cls, teacher, data_u8, transform=None, batch_size=256, labels=None):
        """One pass of the native teacher forward over `data_u8` (uint8 ``[N, S, S, 3]`` on the device) in index order.  Every chunk has exactly
        `batch_size` images (the last one is filled up by repeating the last index), so one engine serves the whole pass; the forward writes its
        logits straight into the table rows of the chunk.  `labels`, when given, enter the data digest.  The teacher's ``training`` flags are
        restored afterwards."""
        from .teacher import _ENGINES, teacher_forward
        from .vit import _native_teacher_ok

        data_u8 = torch.as_tensor(data_u8)
        if not data_u8.is_cuda:
            raise RuntimeError("TeacherLogitTable.build runs on MI355X only: move the uint8 images to the GPU (there is no CPU fallback)")
        params = native.vit_params(teacher)
        if layer_scale_params(teacher):
            raise RuntimeError("TeacherLogitTable.build: the native teacher forward does not cover a LayerScale teacher (its stock module forward does)")
        if any(not p.is_cuda for p in params):
            raise RuntimeError("TeacherLogitTable.build runs on MI355X only: move the teacher to the GPU (there is no CPU fallback)")
        if any(p.requires_grad for p in teacher.parameters()):
            raise RuntimeError("TeacherLogitTable.build: the teacher has parameters that require grad; a table is only valid for a frozen teacher "
                               "(set requires_grad = False on its parameters, as the reference loop does)")
        if not _native_teacher_ok(teacher):
            raise RuntimeError("TeacherLogitTable.build: this teacher has no native forward (vit._native_teacher_ok); there is no fallback")
        batch_size = int(batch_size)
        if batch_size < 1 or data_u8.shape[0] < 1:
            raise ValueError("batch_size and the number of images must be at least 1")
        if transform is None:
            transform = GpuResizeNormalize(data_u8.shape[1], device=data_u8.device)
        dev = transform.device
        N, C = data_u8.shape[0], teacher.head.weight.shape[0]
        chunks = (N + batch_size - 1) // batch_size
        full = torch.empty(chunks * batch_size, C, dtype=torch.float32, device=dev)
        order = torch.arange(chunks * batch_size, dtype=torch.int64, device=dev).clamp_(max=N - 1)
        images = torch.empty(batch_size, 3, transform.out_size, transform.out_size, dtype=torch.float32, device=dev)
        flags = [(m, m.training) for m in teacher.modules()]
        teacher.eval()
        try:
            with torch.no_grad(), torch.cuda.device(dev):
                for k in range(chunks):
                    rows = slice(k * batch_size, (k + 1) * batch_size)
                    teacher_forward(teacher, transform(data_u8, order[rows], out=images), out=full[rows])
        finally:
            for m, t in flags:
                m.training = t
        form = _ENGINES[teacher].passes   # the form that ran
        return cls(full[:N], cls.describe(teacher, data_u8, transform, labels, form), teacher)

    def check_fresh(self) -> None:
        """Raises when a parameter of the teacher this table was built from (or loaded against) has been replaced or modified in place since."""
        t = self._teacher() if self._teacher is not None else None
        if t is not None and _versions(t) != self._teacher_versions:
            raise RuntimeError("TeacherLogitTable: a teacher parameter was replaced or modified after the table was built; the rows no longer are this "
                               "teacher's logits - build the table again")

    def _need_device(self, what):
        if not self.logits.is_cuda:
            raise RuntimeError(f"TeacherLogitTable.{what}: qat-vit_amd ops run on MI355X only (the table is on {self.logits.device}); there is no CPU fallback")

    def rows(self, index: torch.Tensor) -> torch.Tensor:
        """``[len(index), C]`` teacher logits of the samples `index` (int64, on the table's device), for a caller with a loss of its own."""
        self._need_device("rows")
        self.check_fresh()
        return self.logits.index_select(0, index)

    def loss(self, student_logits, index, labels, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1, mix=None):
        """``F.kd_ce_loss(student_logits, teacher(images of index), labels, ...)`` without the teacher forward: (loss, [loss, ce, kd*T^2]).
        ``mix`` (the int32 ``[B, 6]`` records a mixing loader yields) mixes the labels and the teacher's rows of each sample and its partner
        (``F.kd_ce_loss_table_mix``)."""
        self._need_device("loss")
        self.check_fresh()
        if mix is not None:
            return F.kd_ce_loss_table_mix(student_logits, self.logits, index, labels, mix, kd_temp, kd_alpha, label_smoothing)
        return F.kd_ce_loss_table(student_logits, self.logits, index, labels, kd_temp, kd_alpha, label_smoothing)

    def bce_loss(self, student_logits, index, labels, kd_temp=4.0, kd_alpha=0.5, label_smoothing=0.1, mix=None, target_threshold=None,
                 sum_classes=False):
        """``loss`` with the binary cross-entropy of ``F.kd_bce_loss`` as the hard part: (loss, [loss, bce, kd*T^2]).  The KD part and what ``mix``
        does to the labels and the teacher's rows are ``loss``'s."""
        self._need_device("bce_loss")
        self.check_fresh()
        return F.kd_bce_loss(student_logits, labels, table=self.logits, index=index, mix=mix, kd_temp=kd_temp, kd_alpha=kd_alpha,
                             label_smoothing=label_smoothing, target_threshold=target_threshold, sum_classes=sum_classes)

    def save(self, path) -> None:
        torch.save({"logits": self.logits.detach().cpu(), "meta": self.meta}, path)

    @classmethod
    def load(cls, path, teacher=None, data_u8=None, transform=None, labels=None, device="cuda"):
        """The table saved at `path`, on `device`.  Whatever is given of the teacher, the data (with `labels` if the table was built with them)
        and the transform is compared with the table's record; a difference raises a ValueError that names the field.  With a teacher given,
        later changes of its parameters are watched as after ``build``."""
        blob = torch.load(path, map_location="cpu", weights_only=True)
        logits, meta = blob["logits"], blob["meta"]
        if meta.get("format") != FORMAT:
            raise ValueError(f"{path}: table format {meta.get('format')!r}, this version reads {FORMAT}")

        def same(field, have):
            if meta[field] != have:
                raise ValueError(f"{path}: {field} differs: the table was built with {meta[field]!r}, got {have!r}")

        if data_u8 is not None:
            data_u8 = torch.as_tensor(data_u8)
            same("N", int(data_u8.shape[0]))
            same("data_digest", data_digest(data_u8, labels))
        if transform is not None:
            same("transform", transform_tuple(transform))
        if teacher is not None:
            same("C", int(teacher.head.weight.shape[0]))
            same("teacher_form", teacher_form(teacher))
            same("param_digest", param_digest(teacher))
        return cls(logits.to(device).contiguous(), meta, teacher)
