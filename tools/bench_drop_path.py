#!/usr/bin/env python3
"""Step time of the native steps with and without stochastic depth (drop-path), on one MI355X: profiles/drop_path_bench.txt.

    python tools/bench_drop_path.py [--batch 256] [--steps 20] [--warmup 5] [--rounds 3] [--only NAME ...]

Arms (ViT-S, qnnpack, the benchmark's C2 shape by default): the QAT step without a table (drop_path_rate 0) and with drop_path_rate 0.1; the three float
forms without and with it; the stock-torch float step with DropPath for reference.  QATVIT_LNB_FUSE=0 in the environment (a knob read once per process) turns
the fused dgrad + LayerNorm-backward epilogue off: `--only qat` under it separates the cost of the form change from the cost of the multipliers.
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


def make_arm(kind, rate, batch):
    """A callable that runs one training step (forward, loss, backward) of the arm."""
    torch.manual_seed(0)
    w = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, drop_path_rate=rate).cuda().train()
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    y = torch.randint(0, 10, (batch,), device="cuda")
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(kind.split("-")[-1])
    if kind == "qat":
        from torch.ao.quantization import get_default_qat_qconfig, prepare_qat

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            w.qconfig = get_default_qat_qconfig("qnnpack")
            m = prepare_qat(w, inplace=False).cuda().train()
    elif kind.startswith("native"):
        m = qat_vit_amd.native_float(w, amp=dt if dt is not None else False)
    else:
        m = w   # stock torch

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
    ap.add_argument("--only", nargs="*", default=None, help="arm kinds to run: qat native-fp32 native-fp16 native-bf16 stock-fp32")
    a = ap.parse_args()
    kinds = a.only or ["qat", "native-fp32", "native-fp16", "native-bf16", "stock-fp32"]
    arms = {}
    for kind in kinds:
        for rate in (0.0, 0.1):
            arms[f"{kind} drop_path_rate={rate}"] = make_arm(kind, rate, a.batch)
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
    lnb = os.environ.get("QATVIT_LNB_FUSE", "1")
    for name, v in ms.items():
        print(f"{name:36s} QATVIT_LNB_FUSE={lnb}  ms/step min {min(v):8.3f}  median {statistics.median(v):8.3f}  max {max(v):8.3f}")
    print(json.dumps({"batch": a.batch, "steps": a.steps, "rounds": a.rounds, "lnb_fuse": lnb, "ms_per_step": ms}))


if __name__ == "__main__":
    main()
