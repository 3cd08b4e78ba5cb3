"""Worker of tests/test_gpu_head_mfma.py: one forward + backward (no optimiser step) of a tiny student at 200 classes (embed_dim 128, depth 2, 32-pixel
images, batch 3, fixed seeds) under whatever QATVIT_* knobs the environment holds; argv[2] is the qconfig.  Writes logits, loss, every parameter gradient,
the observer buffers and the engine's head form to the .pt file argv[1]."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qat_vit_amd  # noqa: E402
from qat_vit_amd import functional as F  # noqa: E402
from qat_vit_amd.engine import engine_of  # noqa: E402
from tests.util import fq_modules, prepare  # noqa: E402


def main():
    torch.manual_seed(5)
    stu = qat_vit_amd.create_student("vit", num_classes=200, qat_wrapper=True, embed_dim=128, depth=2, num_heads=2, img_size=32)
    p = prepare(stu.cuda(), sys.argv[2])
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 200, (3,), generator=g).cuda()
    out = p(x)
    loss, _ = F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)
    loss.backward()
    torch.cuda.synchronize()
    torch.save({"logits": out.detach().cpu(), "loss": loss.detach().cpu(), "grads": {n: q.grad.detach().cpu() for n, q in p.named_parameters()},
                "fq": {n: [t.detach().cpu() for t in (m.scale, m.zero_point, m.activation_post_process.min_val, m.activation_post_process.max_val)]
                       for n, m in fq_modules(p).items()},
                "head_mfma": int(engine_of(p).head_mfma)}, sys.argv[1])


if __name__ == "__main__":
    main()
