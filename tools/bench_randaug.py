#!/usr/bin/env python3
"""Measures the RandAugment stage (qatvit_image_bytes_randaug, GpuBytesRandAugment, GpuWideResizeNormalize(randaug=...))
on an MI355X -> profiles/randaug_bench.txt.

Per batch of 256 at D = 224, the stage arms on the same staged bytes (stage 1 of 256 x 256 sources under default RandomResizedCrop records,
formed once):
  (a)  the stage alone, records drawn by RandAugment.from_config("rand-m9-mstd0.5-inc1") with seed 1
  (b)  the stage alone, all-identity records (one copy per sample)
  (c)  the stage alone, every sample on one bicubic rotate by 27 degrees
  (d)  the full two-stage batch on the 256 x 256 sources with erase records, without the stage
  (e)  (d) with the stage on (a)'s records
  (f)  Pillow on the host, one process: the same ops on the first `--host-images` samples of (a), per image
HIP events around `--launches` launches after `--warmup` warm-up launches per arm, `--reps` repetitions interleaved in this one process.  The
stage's three images of a batch are 3 x 38.5 MB; the fp32 output of (d) and (e) rotates over four buffers (616 MB), beyond the 256 MiB Infinity
Cache.  Clocks as the machine has them.  The tool reports times; it measures no counter, so it says nothing about what bounds the kernel.

usage: python3 tools/bench_randaug.py [--launches K] [--warmup W] [--reps R] [--host-images N] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B, D = 256, 224


def timed(run, args):
    import torch

    for i in range(args.warmup):
        run(i)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(args.launches):
        run(i)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / args.launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "randaug_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import qat_vit_amd
    from qat_vit_amd.data import RANDAUG_OPS, randaug_record

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 256, (1024, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
    index = torch.randint(0, 1024, (B,), generator=g).to(dev)
    rrc = qat_vit_amd.RandomResizedCrop().draw(B, (256, 256), g).to(dev)
    boxes = qat_vit_amd.RandomErasing().draw(B, D, torch.Generator().manual_seed(1)).to(dev)
    drawn = qat_vit_amd.RandAugment.from_config("rand-m9-mstd0.5-inc1").draw(B, D, torch.Generator().manual_seed(1))
    none = torch.zeros(B, 2, 16, dtype=torch.int32, device=dev)
    rotate = torch.from_numpy(np.stack([randaug_record("Rotate", 27.0, D, "bicubic"), randaug_record(None)])).repeat(B, 1, 1).to(dev)
    staged = qat_vit_amd.GpuWindowResize((256, 256), out_size=D)(src, index, rrc)
    stage = qat_vit_amd.GpuBytesRandAugment(D)
    wide = qat_vit_amd.GpuWideResizeNormalize((256, 256), out_size=D)
    outs = [torch.empty(B, 3, D, D, device=dev) for _ in range(4)]
    records = drawn.to(dev)
    arms = {
        "a": ("the stage alone, drawn rand-m9-mstd0.5-inc1 records", lambda i: stage(staged, records)),
        "b": ("the stage alone, all-identity records", lambda i: stage(staged, none)),
        "c": ("the stage alone, every sample on a bicubic rotate", lambda i: stage(staged, rotate)),
        "d": ("two stages on 256 x 256 sources, erase records, without the stage", lambda i: wide(src, index, rrc=rrc, out=outs[i % 4], erase=boxes)),
        "e": ("(d) with the stage on (a)'s records", lambda i: wide(src, index, rrc=rrc, out=outs[i % 4], erase=boxes, randaug=records)),
    }
    assert torch.equal(arms["b"][1](0), staged) and not torch.equal(arms["a"][1](0), staged)
    reps = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, (_, run) in arms.items():
            reps[k].append(timed(run, args))
    med = {k: statistics.median(v) for k, v in reps.items()}
    ops = drawn[..., 0].flatten()
    counts = ", ".join(f"{RANDAUG_OPS[c - 1]} {int((ops == c).sum())}" for c in range(1, 16))
    lines = [f"RandAugment stage, batch {B}, D = {D}, us per batch: HIP events around {args.launches} launches after {args.warmup} warm-up launches per "
             f"arm, {args.reps} repetitions interleaved in this one process; {torch.cuda.get_device_name(0)}; clocks as the machine had them (not "
             "pinned, not changed, not read).  One workgroup of 1024 lanes per sample: a batch of 256 is one workgroup on each of 256 CUs",
             f"  records drawn with seed 1: {int((ops > 0).sum())} live layers of {ops.numel()}, {int((drawn[..., 0] > 0).any(1).sum())} of {B} samples "
             f"touched; {counts}"]
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<72} median {med[k]:8.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {max(reps[k]) - min(reps[k]):.1f}")
    lines.append(f"  reported: (e) - (d) = {med['e'] - med['d']:+.1f} us; (a) / (b) = {med['a'] / med['b']:.2f}; (c) / (b) = {med['c'] / med['b']:.2f}; (b) moves "
                 f"{2 * B * 3 * D * D / 1e6:.1f} MB: {2 * B * 3 * D * D / med['b'] / 1e3:.0f} GB/s")
    try:
        from tools.gen_randaug_golden import pillow_records

        n = min(args.host_images, B)
        imgs, recs = staged[:n].cpu().numpy(), drawn[:n].numpy()
        want = pillow_records(imgs, recs)                            # (warm)
        t0 = time.perf_counter()
        for _ in range(3):
            pillow_records(imgs, recs)
        per_image = (time.perf_counter() - t0) / 3 / n * 1e6
        same = np.array_equal(stage(staged, records)[:n].cpu().numpy(), want)
        lines.append(f"  (f) Pillow on the host, one process, the first {n} samples of (a): {per_image:.1f} us per image = {per_image * B:.0f} us per batch of "
                     f"{B} on one core; the stage's bytes equal Pillow's on these samples: {'yes' if same else 'NO'}")
    except ImportError as e:
        lines.append(f"  (f) Pillow on the host: not measured ({e})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
