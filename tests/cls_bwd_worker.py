"""Worker of tests/test_gpu_cls_bwd.py: tests/knob_worker.py's two training steps (ViT-S width, depth 2, fixed seeds) at the batch size given as argv[3],
under whatever QATVIT_* knobs the environment holds; same record in the .pt file argv[1].  With argv[4] == "staged" the second (one-plane) backward is then
repeated through the stage-level entry point - in ONE call, and as stage 0 followed by stages 1 .. last in a call of their own - and both sets of
gradients are stored as res["single"] / res["staged"]."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qat_vit_amd  # noqa: E402
from qat_vit_amd import engine as E  # noqa: E402
from qat_vit_amd import functional as F  # noqa: E402
from tests.util import fq_modules, prepare  # noqa: E402


def main():
    batch = int(sys.argv[3])
    staged = len(sys.argv) > 4 and sys.argv[4] == "staged"
    torch.manual_seed(3)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=384, depth=2, num_heads=6, img_size=224)
    p = prepare(stu.cuda(), sys.argv[2])
    g = torch.Generator().manual_seed(4)
    x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 10, (batch,), generator=g).cuda()
    res, dl = {}, []
    for step in (1, 2):
        for q in p.parameters():
            q.grad = None
        out = p(x)
        out.register_hook(lambda gr: dl.append(gr.detach().clone()))
        loss, _ = F.kd_ce_loss(out, None, y, 4.0, 0.5, 0.1)
        loss.backward()
        torch.cuda.synchronize()
        res[step] = {"logits": out.detach().cpu(), "loss": loss.detach().cpu(), "grads": {n: q.grad.detach().cpu() for n, q in p.named_parameters()},
                     "fq": {n: (m.scale.detach().cpu(), m.zero_point.detach().cpu(), m.activation_post_process.min_val.detach().cpu(),
                                m.activation_post_process.max_val.detach().cpu()) for n, m in fq_modules(p).items()}}
    eng = E.engine_of(p)
    res["one_plane"] = bool(eng._fwd_x16)
    if staged:
        names = [n for n, _ in p.named_parameters()]
        pidx = {id(q): k for k, q in enumerate(eng.params)}
        order = [pidx[id(q)] for _, q in p.named_parameters()]
        last = eng.layout.last_stage

        def grads_of(views):
            torch.cuda.synchronize()
            return {n: views[k].detach().cpu().clone() for n, k in zip(names, order)}

        # every one-plane call that starts at stage 0 takes its scales from the maxima of the call before it: one call to settle them on this step's own
        eng.backward_stages(dl[-1], 0, last, mode=E.BWD_DY16)
        res["single"] = grads_of(eng.backward_stages(dl[-1], 0, last, mode=E.BWD_DY16))
        v0 = grads_of(eng.backward_stages(dl[-1], 0, 0, mode=E.BWD_DY16))
        v1 = grads_of(eng.backward_stages(None, 1, last, mode=E.BWD_DY16))
        res["staged"] = {n: v0[n] + v1[n] for n in names}     # (each call returns zeros for the stages it did not run)
        res["overflowed"] = bool(eng.dy16_overflowed())
    torch.save(res, sys.argv[1])


if __name__ == "__main__":
    main()
