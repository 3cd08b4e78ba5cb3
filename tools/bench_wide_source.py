#!/usr/bin/env python3
"""Measures the wide-source input path (GpuWindowResize / GpuWideResizeNormalize) on an MI355X -> profiles/wide_source_bench.txt.

Per batch of 256 at D = 224, records of the default RandomResizedCrop (seed 1), a random index into a resident uint8 data set:
  (a) the one-launch rrc path, GpuResizeNormalize(224, 224)(rrc=...), on a 224 x 224 source: the baseline, what the tree had before
  (b) the two-stage path on the same source, index and records
  (c) the two-stage path on a 256 x 256 source        (d) on a 512 x 512 source
  (e) (f) (g) stage 1 alone on the 224 / 256 / 512 sources, with its algorithmic bytes (the window's bytes read + 150,528 written per sample)
      over its time against the 8 TB/s of the project's rooflines
  (h) for orientation only, torch ops on the 256 x 256 source: gather, crop-free F.interpolate(mode="bicubic", antialias=True) of the whole
      image + normalise.  It is not byte-equal to Pillow and crops nothing.
HIP events around `--launches` launches after `--warmup` warm-up launches per arm, `--reps` repetitions interleaved a .. h in this one process; the
fp32 output rotates over four buffers (616 MB) and stage 1's uint8 output over eight (308 MB), both beyond the 256 MiB Infinity Cache, so that the
stores go to HBM.  Clocks as the machine has them.  The tool reports times and algorithmic bytes over time; it measures no counter, so it
says nothing about what bounds a kernel.

usage: python3 tools/bench_wide_source.py [--launches K] [--warmup W] [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qat_vit_amd  # noqa: E402

B, D = 256, 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_source_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    sets, recs, index, window_bytes = {}, {}, {}, {}
    for S, n in ((224, 1024), (256, 1024), (512, 512)):
        sets[S] = torch.randint(0, 256, (n, S, S, 3), dtype=torch.uint8, generator=g).to(dev)
        r = qat_vit_amd.RandomResizedCrop().draw(B, S, g)
        recs[S], index[S] = r.to(dev), torch.randint(0, n, (B,), generator=g).to(dev)
        hw = r.to(torch.int64)[:, 1]
        window_bytes[S] = float(((hw & 0x7fff) * (hw >> 15 & 0x7fff) * 3).double().mean())
    one = qat_vit_amd.GpuResizeNormalize(224, out_size=D)
    one.window_tables()
    wide = {S: qat_vit_amd.GpuWideResizeNormalize((S, S), out_size=D) for S in sets}
    outs = [torch.empty(B, 3, D, D, device=dev) for _ in range(4)]
    u8 = [torch.empty(B, D, D, 3, dtype=torch.uint8, device=dev) for _ in range(8)]
    mean = torch.tensor(qat_vit_amd.data.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1) * 255.0
    std = torch.tensor(qat_vit_amd.data.IMAGENET_STD, device=dev).view(1, 3, 1, 1) * 255.0

    def torch_ops(i):
        x = sets[256].index_select(0, index[256]).permute(0, 3, 1, 2).float()
        x = torch.nn.functional.interpolate(x, size=(D, D), mode="bicubic", antialias=True, align_corners=False)
        torch.div(x.clamp_(0, 255).sub_(mean), std, out=outs[i % 4])

    arms = {
        "a": ("one launch, rrc, 224 x 224 source (baseline)", lambda i: one(sets[224], index[224], rrc=recs[224], out=outs[i % 4])),
        "b": ("two stages, 224 x 224 source", lambda i: wide[224](sets[224], index[224], rrc=recs[224], out=outs[i % 4])),
        "c": ("two stages, 256 x 256 source", lambda i: wide[256](sets[256], index[256], rrc=recs[256], out=outs[i % 4])),
        "d": ("two stages, 512 x 512 source", lambda i: wide[512](sets[512], index[512], rrc=recs[512], out=outs[i % 4])),
        "e": ("stage 1 alone, 224 x 224 source", lambda i: wide[224].stage(sets[224], index[224], recs[224], out=u8[i % 8])),
        "f": ("stage 1 alone, 256 x 256 source", lambda i: wide[256].stage(sets[256], index[256], recs[256], out=u8[i % 8])),
        "g": ("stage 1 alone, 512 x 512 source", lambda i: wide[512].stage(sets[512], index[512], recs[512], out=u8[i % 8])),
        "h": ("torch ops, whole 256 x 256 image, antialiased bicubic", torch_ops),
    }
    assert torch.equal(one(sets[224], index[224], rrc=recs[224]), wide[224](sets[224], index[224], rrc=recs[224]))   # (a) and (b) compute the same batch
    reps = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, (_, fn) in arms.items():
            for i in range(args.warmup):
                fn(i)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for i in range(args.launches):
                fn(i)
            ev[1].record()
            torch.cuda.synchronize()
            reps[k].append(ev[0].elapsed_time(ev[1]) * 1e3 / args.launches)
    med = {k: statistics.median(v) for k, v in reps.items()}
    lines = [f"wide-source input path, batch {B}, D = {D}, us per batch: HIP events around {args.launches} launches after {args.warmup} warm-up launches per "
             f"arm, {args.reps} repetitions interleaved a .. h in this one process, fp32 output rotating over 616 MB, stage 1's uint8 output over 308 MB; {torch.cuda.get_device_name(0)}; clocks as "
             "the machine had them (not pinned, not changed, not read)"]
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<58} median {med[k]:8.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {max(reps[k]) - min(reps[k]):.1f}")
    lines.append(f"  the second launch on the same source: (b) - (a) = {med['b'] - med['a']:.1f} us per batch, (b) / (a) = {med['b'] / med['a']:.3f}; "
                 f"(c) / (a) = {med['c'] / med['a']:.3f}, (d) / (a) = {med['d'] / med['a']:.3f}")
    for k, S in (("e", 224), ("f", 256), ("g", 512)):
        nbytes = B * (window_bytes[S] + D * D * 3)
        tbs = nbytes / (med[k] * 1e-6) / 1e12
        lines.append(f"  ({k}) stage 1, {S} x {S}: mean window {window_bytes[S] / 1e3:.1f} KB read + {D * D * 3 / 1e3:.1f} KB written per sample = "
                     f"{nbytes / 1e6:.1f} MB per batch in {med[k]:.1f} us = {tbs:.3f} TB/s, {100 * tbs / 8.0:.1f} % of 8 TB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
