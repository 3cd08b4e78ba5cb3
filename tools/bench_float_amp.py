#!/usr/bin/env python3
"""Time per step of the float (pre-QAT) student step under autocast, ViT-S/16 on one GPU, in one process: the native fp16 form
(native_float(..., amp=True) inside fp16 autocast), the native fp32-accurate form, stock autocast + GradScaler on the same tree, the native
bf16 form (native_float(..., amp=torch.bfloat16) inside bf16 autocast) and stock bf16 autocast (no GradScaler), at batch 256 and 1024 (the
Optuna objective's batch).  A step = forward, KD/CE loss, backward, ClipAdamW step (GradScaler for the fp16 autocast runs).
Gates: the native fp16 / bf16 step at batch 256 takes at most half of stock fp16 / bf16 autocast's time; the bf16 form at most 1.05 x the
fp16 form's.  Prints one line per run and a JSON summary.
usage: python3 tools/bench_float_amp.py [--steps K] [--warmup W] [--native-only [--bf16]]"""
import argparse
import copy
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.filterwarnings("ignore")
import qat_vit_amd  # noqa: E402
from qat_vit_amd import functional as F  # noqa: E402


def run(model, batch, steps, warmup, amp, dtype=torch.float16):
    opt = qat_vit_amd.ClipAdamW(model.parameters(), lr=1e-4)
    scaler = torch.amp.GradScaler("cuda") if amp and dtype == torch.float16 else None
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(batch, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(0, 10, (batch,), device="cuda", generator=g)
    t = torch.randn(batch, 10, device="cuda", generator=g)   # teacher logits (the KD term)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            ev[0].record()
        opt.zero_grad(set_to_none=True)
        if scaler:
            with torch.autocast("cuda", dtype=dtype):
                loss, _ = F.kd_ce_loss(model(x).float(), t, y, 4.0, 0.5, 0.1)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        elif amp:   # bf16: no GradScaler
            with torch.autocast("cuda", dtype=dtype):
                loss, _ = F.kd_ce_loss(model(x).float(), t, y, 4.0, 0.5, 0.1)
            loss.backward()
            opt.step()
        else:
            loss, _ = F.kd_ce_loss(model(x), t, y, 4.0, 0.5, 0.1)
            loss.backward()
            opt.step()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--native-only", action="store_true", help="only the native fp16 step at batch 256 (for a kernel trace)")
    ap.add_argument("--bf16", action="store_true", help="with --native-only: the native bf16 step instead")
    a = ap.parse_args()
    torch.manual_seed(0)
    base = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda().train()
    res = {"gpu": torch.cuda.get_device_name(0), "model": "vit_small_patch16_224", "steps": a.steps, "warmup": a.warmup}
    batches = (256,) if a.native_only else (256, 1024)
    for b in batches:
        if a.native_only and a.bf16:
            m = qat_vit_amd.native_float(copy.deepcopy(base), amp=torch.bfloat16)
            res[f"native_bf16_b{b}_ms"] = run(m, b, a.steps, a.warmup, amp=True, dtype=torch.bfloat16)
            print(f"native bf16 form (bf16 autocast),          batch {b:4d}: {res[f'native_bf16_b{b}_ms']:8.2f} ms/step", flush=True)
            break
        m = qat_vit_amd.native_float(copy.deepcopy(base), amp=True)
        res[f"native_fp16_b{b}_ms"] = run(m, b, a.steps, a.warmup, amp=True)
        print(f"native fp16 form (autocast + GradScaler), batch {b:4d}: {res[f'native_fp16_b{b}_ms']:8.2f} ms/step", flush=True)
        if a.native_only:
            break
        res[f"native_fp32_b{b}_ms"] = run(m, b, a.steps, a.warmup, amp=False)
        print(f"native fp32 form,                          batch {b:4d}: {res[f'native_fp32_b{b}_ms']:8.2f} ms/step", flush=True)
        del m
        torch.cuda.empty_cache()
        res[f"stock_autocast_b{b}_ms"] = run(copy.deepcopy(base), b, a.steps, a.warmup, amp=True)
        print(f"stock autocast + GradScaler,               batch {b:4d}: {res[f'stock_autocast_b{b}_ms']:8.2f} ms/step", flush=True)
        torch.cuda.empty_cache()
        m = qat_vit_amd.native_float(copy.deepcopy(base), amp=torch.bfloat16)
        res[f"native_bf16_b{b}_ms"] = run(m, b, a.steps, a.warmup, amp=True, dtype=torch.bfloat16)
        print(f"native bf16 form (bf16 autocast),          batch {b:4d}: {res[f'native_bf16_b{b}_ms']:8.2f} ms/step", flush=True)
        del m
        torch.cuda.empty_cache()
        res[f"stock_bf16_autocast_b{b}_ms"] = run(copy.deepcopy(base), b, a.steps, a.warmup, amp=True, dtype=torch.bfloat16)
        print(f"stock bf16 autocast,                       batch {b:4d}: {res[f'stock_bf16_autocast_b{b}_ms']:8.2f} ms/step", flush=True)
        torch.cuda.empty_cache()
    if not a.native_only:
        res["fp16_over_stock_autocast_b256"] = res["native_fp16_b256_ms"] / res["stock_autocast_b256_ms"]
        res["gate_fp16_le_half_stock_b256"] = res["fp16_over_stock_autocast_b256"] <= 0.5
        res["bf16_over_stock_bf16_autocast_b256"] = res["native_bf16_b256_ms"] / res["stock_bf16_autocast_b256_ms"]
        res["bf16_over_fp16_b256"] = res["native_bf16_b256_ms"] / res["native_fp16_b256_ms"]
        res["gate_bf16_le_half_stock_b256"] = res["bf16_over_stock_bf16_autocast_b256"] <= 0.5
        res["gate_bf16_le_1.05_fp16_b256"] = res["bf16_over_fp16_b256"] <= 1.05
    print(json.dumps(res))


if __name__ == "__main__":
    main()
