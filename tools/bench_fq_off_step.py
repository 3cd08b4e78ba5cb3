#!/usr/bin/env python3
"""Time per step of the observe-only native step (a prepared student after torch.ao.quantization.disable_fake_quant), ViT-S/16, batch 256,
one GPU, next to the QAT step of the same tree and the native float step (qat_vit_amd.native_float) of an unprepared copy.  A step = forward,
CE loss, backward, ClipAdamW step, timed with HIP events after the warm-up.  Also reports the observe-only buffers the engine allocates beside
its QAT workspace.  Prints one line per run and a JSON summary.
usage: python3 tools/bench_fq_off_step.py [--steps K] [--warmup W] [--observe-only]"""
import argparse
import copy
import json
import os
import sys
import warnings

import torch
import torch.nn.functional as TF
from torch.ao.quantization import disable_fake_quant, disable_observer

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.filterwarnings("ignore")
import qat_vit_amd  # noqa: E402
from qat_vit_amd.engine import engine_of  # noqa: E402


def run(model, batch, steps, warmup):
    opt = qat_vit_amd.ClipAdamW(model.parameters(), lr=1e-4)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(batch, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(0, 10, (batch,), device="cuda", generator=g)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            ev[0].record()
        opt.zero_grad(set_to_none=True)
        TF.cross_entropy(model(x), y).backward()
        opt.step()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def prepared(base):
    from torch.ao.quantization import get_default_qat_qconfig, prepare_qat

    m = copy.deepcopy(base)
    m.qconfig = get_default_qat_qconfig("qnnpack")
    return prepare_qat(m, inplace=False).cuda().train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--observe-only", action="store_true", help="only the observe-only step (for a kernel trace)")
    a = ap.parse_args()
    B = 256
    torch.manual_seed(0)
    base = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda().train()
    res = {"gpu": torch.cuda.get_device_name(0), "model": "vit_small_patch16_224", "batch": B, "steps": a.steps, "warmup": a.warmup}
    if not a.observe_only:
        q = prepared(base)
        res["qat_ms"] = run(q, B, a.steps, a.warmup)
        print(f"QAT step (fake-quant on):               {res['qat_ms']:8.2f} ms/step", flush=True)
        del q
        torch.cuda.empty_cache()
    p = prepared(base)
    with torch.no_grad():
        p(torch.zeros(B, 3, 224, 224, device="cuda"))   # the engine and its QAT workspace, as in a run that switches after QAT steps
    p.apply(disable_fake_quant)
    res["observe_ms"] = run(p, B, a.steps, a.warmup)
    print(f"observe-only step (fake-quant off):     {res['observe_ms']:8.2f} ms/step", flush=True)
    eng = engine_of(p)
    res["qat_workspace_mb"] = eng.workspace.numel() / 2**20
    res["observe_float_workspace_mb"] = eng.float_form.workspace.numel() / 2**20
    res["observe_stats_kb"] = eng.observe_buf.numel() / 2**10
    print(f"  beside the QAT workspace ({res['qat_workspace_mb']:.0f} MiB): float workspace {res['observe_float_workspace_mb']:.0f} MiB, "
          f"observer statistics {res['observe_stats_kb']:.0f} KiB", flush=True)
    if not a.observe_only:
        p.apply(disable_observer)
        res["observe_observers_off_ms"] = run(p, B, a.steps, a.warmup)
        print(f"observe-only step, observers off:       {res['observe_observers_off_ms']:8.2f} ms/step", flush=True)
        del p, eng
        torch.cuda.empty_cache()
        f = qat_vit_amd.native_float(copy.deepcopy(base))
        res["native_float_ms"] = run(f, B, a.steps, a.warmup)
        print(f"native float step (unprepared copy):    {res['native_float_ms']:8.2f} ms/step", flush=True)
        res["observe_over_float"] = res["observe_ms"] / res["native_float_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
