"""qat-vit_amd: MI355X-native QAT-ViT student training path (drop-in below the
reference's ``src.models`` API).  Import as ``qat_vit_amd``."""
from .model_registry import (  # noqa: F401
    PLATFORM,
    QATWrapper,
    create_model,
    create_student,
    create_teacher,
    list_available_models,
    register_model,
)

from .vit import DropPath, LayerScale, forced_drop_path  # noqa: F401,E402
from .float_engine import native_float  # noqa: F401,E402
from .export import Int8Student, export_int8, import_int8  # noqa: F401,E402
from .optim import ClipAdamW, ClipLamb, ema_warmup_decay, vit_param_groups  # noqa: F401,E402
from .data import ColorJitter, GaussianBlur, ThreeAugment, GpuImageLoader, GpuResizeNormalize, MixupCutmix, RandomCropFlip, RandomErasing, RandomResizedCrop, cifar10_arrays, epoch_batches  # noqa: F401,E402
from .data import GpuBytesBlurNormalize, GpuWideResizeNormalize, GpuWindowResize, center_crop_window  # noqa: F401,E402
from .distill import TeacherLogitTable  # noqa: F401,E402
from .evaluate import EvalAccumulator, EvalResult, evaluate  # noqa: F401,E402
from .loss import BinaryCrossEntropy  # noqa: F401,E402

__all__ = ["BinaryCrossEntropy", "DropPath", "LayerScale", "forced_drop_path", "EvalAccumulator", "EvalResult", "evaluate", "TeacherLogitTable", "native_float", "ClipAdamW", "ClipLamb", "ema_warmup_decay", "vit_param_groups", "ColorJitter", "GaussianBlur", "ThreeAugment", "GpuImageLoader", "GpuResizeNormalize", "GpuBytesBlurNormalize", "GpuWideResizeNormalize", "GpuWindowResize", "center_crop_window", "MixupCutmix", "RandomCropFlip", "RandomErasing", "RandomResizedCrop", "cifar10_arrays", "epoch_batches", "Int8Student", "export_int8", "import_int8", "PLATFORM", "QATWrapper", "create_model", "create_student", "create_teacher", "list_available_models", "register_model"]
