"""Worker of tests/test_gpu_float_head_mfma.py: one forward + backward of a tiny native float student at 200 classes under whatever QATVIT_* knobs the
environment holds.  argv: the .pt file to write, the form (fp32: embed_dim 128, depth 2; fp16 / bf16: embed_dim 384, depth 1, under autocast; 32-pixel images,
batch 3), the seed.  Writes logits, loss, every parameter gradient, the engine's head form and, for fp32, whether the observe-only forward of the prepared
copy (disable_fake_quant) gave the float forward's logits bit for bit."""
import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qat_vit_amd  # noqa: E402
from qat_vit_amd import functional as F  # noqa: E402
from qat_vit_amd.float_engine import engine_of  # noqa: E402
from tests.util import prepare  # noqa: E402


def main():
    out, kind, seed = sys.argv[1], sys.argv[2], int(sys.argv[3])
    torch.manual_seed(seed)
    kw = dict(embed_dim=128, depth=2, num_heads=2) if kind == "fp32" else dict(embed_dim=384, depth=1, num_heads=6)
    stu = qat_vit_amd.create_student("vit", num_classes=200, qat_wrapper=True, img_size=32, **kw).cuda().train()
    m = qat_vit_amd.native_float(copy.deepcopy(stu), amp={"fp32": False, "fp16": True, "bf16": torch.bfloat16}[kind])
    g = torch.Generator().manual_seed(seed + 100)
    x, y = torch.randn(3, 3, 32, 32, generator=g).cuda(), torch.randint(0, 200, (3,), generator=g).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16 if kind == "bf16" else torch.float16, enabled=kind != "fp32"):
        logits = m(x)
    loss = F.kd_ce_loss(logits.float(), None, y, 4.0, 0.5, 0.1)[0]
    (loss * (1024.0 if kind == "fp16" else 1.0)).backward()   # (fp16: a fixed loss scale, as GradScaler applies one)
    res = {"logits": logits.detach().cpu(), "loss": loss.detach().cpu(), "grads": {n: q.grad.detach().cpu() for n, q in m.named_parameters()},
           "head_mfma": engine_of(m).head_mfma}
    if kind == "fp32":
        from torch.ao.quantization import disable_fake_quant

        p = prepare(copy.deepcopy(stu), "qnnpack")
        p.apply(disable_fake_quant)
        with torch.no_grad():
            res["observe_equal"] = torch.equal(p(x), m(x))
    torch.cuda.synchronize()
    torch.save(res, out)


if __name__ == "__main__":
    main()
