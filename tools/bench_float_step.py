#!/usr/bin/env python3
"""Time per step of the float (pre-QAT) student step, ViT-S/16 on one GPU: the native step (qat_vit_amd.native_float) against stock fp32
torch and stock autocast + GradScaler on the same tree, batch 256 (train_final.sh's fp32 float epochs), and the native step at batch 1024
(the Optuna objective's default).  A step = forward, CE loss, backward, ClipAdamW step.  Prints one line per run and a JSON summary.
usage: python3 tools/bench_float_step.py [--steps K] [--warmup W] [--native-only]"""
import argparse
import copy
import json
import os
import sys
import warnings

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.filterwarnings("ignore")
import qat_vit_amd  # noqa: E402


def run(model, batch, steps, warmup, amp=False):
    opt = qat_vit_amd.ClipAdamW(model.parameters(), lr=1e-4)
    scaler = torch.amp.GradScaler("cuda") if amp else None
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(batch, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(0, 10, (batch,), device="cuda", generator=g)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            ev[0].record()
        opt.zero_grad(set_to_none=True)
        if amp:
            with torch.autocast("cuda", dtype=torch.float16):
                loss = TF.cross_entropy(model(x), y)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            TF.cross_entropy(model(x), y).backward()
            opt.step()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--native-only", action="store_true", help="only the native step at batch 256 (for a kernel trace)")
    a = ap.parse_args()
    torch.manual_seed(0)
    base = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda().train()
    res = {"gpu": torch.cuda.get_device_name(0), "model": "vit_small_patch16_224", "steps": a.steps, "warmup": a.warmup}
    native = qat_vit_amd.native_float(copy.deepcopy(base))
    res["native_fp32_b256_ms"] = run(native, 256, a.steps, a.warmup)
    print(f"native float step, batch 256:          {res['native_fp32_b256_ms']:8.2f} ms/step", flush=True)
    if not a.native_only:
        res["stock_fp32_b256_ms"] = run(copy.deepcopy(base), 256, a.steps, a.warmup)
        print(f"stock fp32 torch, batch 256:           {res['stock_fp32_b256_ms']:8.2f} ms/step", flush=True)
        res["stock_autocast_b256_ms"] = run(copy.deepcopy(base), 256, a.steps, a.warmup, amp=True)
        print(f"stock autocast + GradScaler, batch 256: {res['stock_autocast_b256_ms']:8.2f} ms/step", flush=True)
        del native
        torch.cuda.empty_cache()
        native = qat_vit_amd.native_float(copy.deepcopy(base))
        res["native_fp32_b1024_ms"] = run(native, 1024, a.steps, a.warmup)
        print(f"native float step, batch 1024:         {res['native_fp32_b1024_ms']:8.2f} ms/step", flush=True)
        res["speedup_vs_stock_fp32_b256"] = res["stock_fp32_b256_ms"] / res["native_fp32_b256_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
