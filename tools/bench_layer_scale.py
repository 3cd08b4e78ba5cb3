#!/usr/bin/env python3
"""Step time of the native steps without LayerScale, with it, and with it plus stochastic depth, on one MI355X: profiles/layer_scale_bench.txt.

    python tools/bench_layer_scale.py [--batch 256] [--steps 20] [--warmup 5] [--rounds 3] [--only NAME ...]

Arms (ViT-S, qnnpack, the benchmark's C2 shape by default): the QAT step and the three float forms, each with init_values=None (the step as it was: nothing
bound, the launches of a tree without LayerScale), with init_values=1e-5, and with init_values=1e-5 and drop_path_rate=0.1.
Each arm: warm-up steps, then `rounds` windows of `steps` steps between device events; the arms alternate round by round, so drift hits all alike.  Prints ms
per step (min / median / max over the rounds) and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import qat_vit_amd  # noqa: E402
from qat_vit_amd import functional as F  # noqa: E402

VARIANTS = {"init_values=None": {}, "init_values=1e-5": dict(init_values=1e-5), "init_values=1e-5 drop_path_rate=0.1": dict(init_values=1e-5, drop_path_rate=0.1)}


def make_arm(kind, model_kw, batch):
    """A callable that runs one training step (forward, loss, backward) of the arm."""
    torch.manual_seed(0)
    w = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, **model_kw).cuda().train()
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    y = torch.randint(0, 10, (batch,), device="cuda")
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(kind.split("-")[-1])
    if kind == "qat":
        from torch.ao.quantization import get_default_qat_qconfig, prepare_qat

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            w.qconfig = get_default_qat_qconfig("qnnpack")
            m = prepare_qat(w, inplace=False).cuda().train()
    else:
        m = qat_vit_amd.native_float(w, amp=dt if dt is not None else False)

    def step():
        for p in m.parameters():
            p.grad = None
        if kind == "qat":
            F.kd_ce_loss(m(x), None, y, 4.0, 0.5, 0.1)[0].backward()
            return
        with torch.autocast("cuda", dtype=dt, enabled=dt is not None):
            out = m(x)
        torch.nn.functional.cross_entropy(out.float(), y).backward()

    return step


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", nargs="*", default=None, help="arm kinds to run: qat native-fp32 native-fp16 native-bf16")
    a = ap.parse_args()
    kinds = a.only or ["qat", "native-fp32", "native-fp16", "native-bf16"]
    arms = {}
    for kind in kinds:
        for name, kw in VARIANTS.items():
            arms[f"{kind} {name}"] = make_arm(kind, kw, a.batch)
    for step in arms.values():
        for _ in range(a.warmup):
            step()
    torch.cuda.synchronize()
    ms = {n: [] for n in arms}
    for _ in range(a.rounds):
        for name, step in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    for name, v in ms.items():
        print(f"{name:52s} ms/step min {min(v):8.3f}  median {statistics.median(v):8.3f}  max {max(v):8.3f}")
    print(json.dumps({"batch": a.batch, "steps": a.steps, "rounds": a.rounds, "ms_per_step": ms}))


if __name__ == "__main__":
    main()
