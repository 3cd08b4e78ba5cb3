#!/usr/bin/env python3
"""Measures on-device validation (qat_vit_amd.evaluate) on one MI355X and writes profiles/evaluate_bench.txt.

The reference's validation pass: 10,000 test images, 40 batches of 256 (here synthetic uint8 32x32 images resident on the device, drawn by
GpuImageLoader), a prepared QAT ViT-S/16 student (qnnpack), in three arms:
  (a) the reference loop (qat_trainer.py:49-61) restated below: argmax, ==, .sum().item() per batch      - one host round trip per batch;
  (b) qat_vit_amd.evaluate(model, loader)                                                               - one per evaluation;
  (c) qat_vit_amd.evaluate(Int8Student(export), loader, other=the prepared model with observers off)    - the int8 claim over the whole set.
One warm-up pass of each arm, then five timed passes per arm, interleaved a, b, c, a, b, c, ... in this process; a pass is a host clock from a
device synchronisation to the return of the arm (each arm ends in a device-to-host copy of its result).  Also: the counting kernel's own time
(HIP events around 200 launches, five repetitions).

The one condition: median (b) - median (a) <= the spread (max - min) of (a)'s five passes, i.e. (b) is not slower than (a) beyond the run-to-run
spread.  The exit status says whether it held; the ratio is reported whatever it is.

Run it as one step under its own time limit, and chain steps with &&, so that a failing step starts nothing after it:
  timeout -k 10 600 python3 tools/bench_evaluate.py && echo done

usage: python3 tools/bench_evaluate.py [--images N] [--repeats R] [--out FILE]"""
import argparse
import copy
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
BATCH = 256
CLOCK_NOTE = ("clocks: as the machine had them (not pinned, not changed, not read); every figure follows its own warm-up, and the interleaved "
              "passes show the drift inside this run")


@torch.no_grad()
def evaluate_fp32(model, dataloader, device):
    """qat_trainer.py:49-61, restated."""
    model.eval()
    correct = 0
    total = 0
    for images, labels in dataloader:
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        outputs = model(images)
        preds = outputs.argmax(dim=1)
        correct += (preds == labels).sum().item()
        total += labels.size(0)
    return 100.0 * correct / max(1, total)


def fmt(v):
    return ", ".join(f"{t:.1f}" for t in v)


def kernel_time(lines, C):
    from qat_vit_amd import EvalAccumulator

    g = torch.Generator(device="cuda").manual_seed(3)
    logits = torch.randn(BATCH, C, device="cuda", generator=g)
    other = torch.randn(BATCH, C, device="cuda", generator=g)
    y = torch.randint(0, C, (BATCH,), device="cuda", generator=g)
    acc = EvalAccumulator(C)
    for name, fn in (("update(logits, labels)", lambda: acc.update(logits, y)), ("update(logits, labels, other)", lambda: acc.update(logits, y, other))):
        for _ in range(20):
            fn()
        reps = []
        for _ in range(5):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(200):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            reps.append(ev[0].elapsed_time(ev[1]) / 200)
        lines.append(f"  {name:32s} {statistics.median(reps) * 1e3:7.1f} us per call (five repetitions of 200 calls, launch and host glue included: "
                     f"{', '.join(f'{r * 1e3:.1f}' for r in reps)} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluate.py needs an MI355X: there is no CPU form of the forwards or of the counting kernel to time")
    import qat_vit_amd
    from torch.ao.quantization import disable_observer, get_default_qat_qconfig, prepare_qat

    dev = torch.device("cuda", 0)
    lines = [f"on-device validation on {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    g = torch.Generator(device="cuda").manual_seed(0)
    data = torch.randint(0, 256, (args.images, 32, 32, 3), device="cuda", generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (args.images,), device="cuda", generator=g)
    tr = qat_vit_amd.GpuResizeNormalize(32)
    loader = qat_vit_amd.GpuImageLoader(data, labels, BATCH, transform=tr)
    torch.manual_seed(0)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda().train()
    stu.qconfig = get_default_qat_qconfig("qnnpack")
    model = prepare_qat(stu, inplace=False).cuda().train()
    with torch.no_grad():
        model(next(iter(loader))[0])                      # the observers have seen data
    frozen = copy.deepcopy(model)
    frozen.apply(disable_observer)
    infer = qat_vit_amd.Int8Student(qat_vit_amd.export_int8(frozen))

    lines.append(f"the counting kernel, batch {BATCH}, 10 classes, fp32 logits:")
    kernel_time(lines, 10)

    arms = {"a": lambda: evaluate_fp32(model, loader, dev), "b": lambda: qat_vit_amd.evaluate(model, loader),
            "c": lambda: qat_vit_amd.evaluate(infer, loader, other=frozen)}

    def timed(arm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = arms[arm]()
        return (time.perf_counter() - t0) * 1e3, out

    out = {arm: timed(arm)[1] for arm in "abc"}            # the warm-up pass of each arm
    w = {arm: [] for arm in "abc"}
    for _ in range(args.repeats):
        for arm in "abc":
            ms, out[arm] = timed(arm)
            w[arm].append(ms)
    med = {arm: statistics.median(w[arm]) for arm in "abc"}
    spread = max(w["a"]) - min(w["a"])
    ok = med["b"] - med["a"] <= spread
    rb, rc = out["b"], out["c"]
    lines.append(f"validation pass: {args.images:,} images, {len(loader)} batches of {BATCH}, prepared QAT ViT-S/16 (qnnpack), {args.repeats} interleaved passes "
                 "per arm after one warm-up pass each, ms per pass:")
    lines.append(f"  (a) reference loop, .item() per batch:           median {med['a']:.1f}  ({fmt(w['a'])}); spread {spread:.1f}")
    lines.append(f"  (b) evaluate(model, loader):                     median {med['b']:.1f}  ({fmt(w['b'])})")
    lines.append(f"  (c) evaluate(Int8Student, loader, other=frozen): median {med['c']:.1f}  ({fmt(w['c'])})")
    lines.append(f"  (b) - (a) = {med['b'] - med['a']:+.1f} ms against the spread of (a) {spread:.1f} ms -> {'holds' if ok else 'DOES NOT HOLD'}; "
                 f"(b) / (a) = {med['b'] / med['a']:.3f}; images/s: (a) {args.images / med['a'] * 1e3:,.0f}, (b) {args.images / med['b'] * 1e3:,.0f}, "
                 f"(c) {args.images / med['c'] * 1e3:,.0f} (two forwards per batch)")
    lines.append(f"  last pass: (a) accuracy {out['a']!r}; (b) accuracy {rb.accuracy!r}, {rb.correct} of {rb.total}, mean loss {rb.loss:.6f}, "
                 f"{rb.nonfinite_rows} non-finite rows; (c) {rc.agree} of {rc.total} agree, int8 correct {rc.correct}, fake-quant correct {rc.other_correct}")
    lines.append("  ((a) and (b) run on the same model with its observers enabled, one pass after the other, so their accuracies belong to two "
                 "successive observer states)")
    lines.append(CLOCK_NOTE)
    lines.append("command: timeout -k 10 600 python3 tools/bench_evaluate.py")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
