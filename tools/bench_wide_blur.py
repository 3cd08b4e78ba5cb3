#!/usr/bin/env python3
"""Measures the bytes-in blur form (qatvit_image_bytes_blur, GpuBytesBlurNormalize, GpuWideResizeNormalize(blur=True)) on an
MI355X -> profiles/wide_blur_bench.txt.

Per batch of 256 at D = 224.  The second-stage arms run on the same staged bytes (stage 1 of 256 x 256 sources under default RandomResizedCrop
records, formed once) and, where they apply, the same erase, colour and blur records, all drawn with seed 1:
  (a)  the existing colour second stage, GpuResizeNormalize(224, 224)(bytes, color=...), on 3-Augment-style colour records without blur (two
       independent coins): the path the tree had before, and the yardstick that nothing existing moved
  (b)  the new entry, the same records, every blur record "no blur"
  (c)  the new entry, ThreeAugment records (a third blurred)
  (d1) (d2) the new entry, (a)'s colour records, every sample blurred at radius 0.1 / 2.0
  (e)  for scale: the one-launch blur entry at 32 -> 224 (GpuResizeNormalize(32, 224), random index into 50,000 resident images, no crop
       words) on (c)'s colour and blur records
  (f)  (a) + three 3 x 3 box convolutions (each covers both axes, replicated edge) as torch ops on the float batch, as
       tools/bench_input_pipeline.py --blur builds them (time only: not Pillow's values)
  (g)  the full two-stage batch on the 256 x 256 sources with ThreeAugment records, GpuWideResizeNormalize(blur=True)
  (h)  the full two-stage batch with (a)'s colour records and no blur records
HIP events around `--launches` launches after `--warmup` warm-up launches per arm, `--reps` repetitions interleaved in this one process; the fp32
output rotates over four buffers (616 MB), beyond the 256 MiB Infinity Cache, so that the stores go to HBM.  Clocks as the machine has them.
With `--parent DIR` (another checkout of this repository with its library built, e.g. the parent commit) arm (a) is first measured in fresh
processes of its own, alternating DIR and this tree (in the order P B B P ..), `--alternations` times each: the spread of the parent against which (a) here is read.
The tool reports times; it measures no counter, so it says nothing about what bounds a kernel.

usage: python3 tools/bench_wide_blur.py [--launches K] [--warmup W] [--reps R] [--parent DIR] [--alternations A] [--out FILE]"""
import argparse
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, D = 256, 224
LDS_PER_CU = 160 * 1024


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="another checkout (built) in which arm (a) is measured too, alternating")
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--root", default=HERE, help="the checkout whose package is imported (used by --parent's child processes)")
    ap.add_argument("--arm-a-only", action="store_true", help="measure arm (a) alone and print one line (uses nothing the parent lacks)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "wide_blur_bench.txt"))
    return ap.parse_args()


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
    args = parse()
    alternated = []
    if args.parent and not args.arm_a_only:
        # before this process touches the GPU: fresh child processes, one at a time
        for k in range(args.alternations):
            pair = (("parent", os.path.abspath(args.parent)), ("branch", HERE))
            for name, root in (pair if k % 2 == 0 else pair[::-1]):   # P B B P P B B P: a drift over the call falls on both alike
                cmd = [sys.executable, os.path.abspath(__file__), "--arm-a-only", "--root", root, "--launches", str(args.launches), "--warmup",
                       str(args.warmup), "--reps", str(args.reps)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.exit(f"arm (a) in {root} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
                line = next(l for l in r.stdout.splitlines() if l.startswith("ARM_A "))
                alternated.append((name, k, [float(v) for v in line.split()[1:]]))
                print(name, k, line, flush=True)
    sys.path.insert(0, args.root)
    import torch

    import qat_vit_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    src256 = torch.randint(0, 256, (1024, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
    index256 = torch.randint(0, 1024, (B,), generator=g).to(dev)
    rrc = qat_vit_amd.RandomResizedCrop().draw(B, (256, 256), g).to(dev)
    boxes = qat_vit_amd.RandomErasing().draw(B, D, torch.Generator().manual_seed(1)).to(dev)
    aug3 = qat_vit_amd.ColorJitter(0.3, 0.3, 0.3, grayscale=1 / 3, solarize=1 / 3).draw(B, torch.Generator().manual_seed(1)).to(dev)
    staged = qat_vit_amd.GpuWindowResize((256, 256), out_size=D)(src256, index256, rrc)
    second = qat_vit_amd.GpuResizeNormalize(D, out_size=D)
    outs = [torch.empty(B, 3, D, D, device=dev) for _ in range(4)]
    arm_a = lambda i: second(staged, None, out=outs[i % 4], erase=boxes, color=aug3)   # noqa: E731
    if args.arm_a_only:
        reps = [timed(arm_a, args) for _ in range(args.reps)]
        print("ARM_A " + " ".join(f"{r:.2f}" for r in reps))
        return

    col3, blur3 = qat_vit_amd.ThreeAugment().draw(B, torch.Generator().manual_seed(1))
    n_blur = int((blur3[:, 0] & 1).sum())
    col3, blur3 = col3.to(dev), blur3.to(dev)
    weights = qat_vit_amd.data.blur_weights
    rec = lambda r: [1 | weights(r)[0] << 8, weights(r)[1], weights(r)[2], 0]   # noqa: E731
    none = torch.zeros(B, 4, dtype=torch.int32, device=dev)
    all01, all20 = (torch.tensor([rec(r)] * B, dtype=torch.int32).to(dev) for r in (0.1, 2.0))
    new = qat_vit_amd.GpuBytesBlurNormalize(D)
    src32 = torch.randint(0, 256, (50000, 32, 32, 3), dtype=torch.uint8, generator=g).to(dev)
    index32 = torch.randint(0, 50000, (B,), generator=g).to(dev)
    one = qat_vit_amd.GpuResizeNormalize(32, out_size=D)
    wide = qat_vit_amd.GpuWideResizeNormalize((256, 256), out_size=D, blur=True)
    mean = torch.tensor(qat_vit_amd.data.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(qat_vit_amd.data.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    box3 = torch.full((3, 1, 3, 3), 1.0 / 9.0, device=dev)

    def composed(i):
        x = arm_a(i)
        x = (x * std + mean) * 255.0
        for _ in range(3):
            x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), box3, groups=3)
        return (x / 255.0 - mean) / std

    arms = {
        "a": ("colour second stage (existing), 3-Augment-style records without blur", arm_a),
        "b": ("bytes-in blur entry, the same records, every blur record \"no blur\"",
              lambda i: new(staged, out=outs[i % 4], erase=boxes, color=aug3, blur=none)),
        "c": ("bytes-in blur entry, ThreeAugment records", lambda i: new(staged, out=outs[i % 4], erase=boxes, color=col3, blur=blur3)),
        "d1": ("bytes-in blur entry, (a)'s colour records, every sample blurred at radius 0.1",
               lambda i: new(staged, out=outs[i % 4], erase=boxes, color=aug3, blur=all01)),
        "d2": ("bytes-in blur entry, (a)'s colour records, every sample blurred at radius 2.0",
               lambda i: new(staged, out=outs[i % 4], erase=boxes, color=aug3, blur=all20)),
        "e": ("one-launch blur entry at 32 -> 224, (c)'s records (for scale)",
              lambda i: one(src32, index32, out=outs[i % 4], erase=boxes, color=col3, blur=blur3)),
        "f": ("(a) + three 3 x 3 box convolutions as torch ops (time only)", composed),
        "g": ("two stages on 256 x 256 sources, ThreeAugment records",
              lambda i: wide(src256, index256, rrc=rrc, out=outs[i % 4], erase=boxes, color=col3, blur=blur3)),
        "h": ("two stages on 256 x 256 sources, (a)'s colour records, no blur records",
              lambda i: wide(src256, index256, rrc=rrc, out=outs[i % 4], erase=boxes, color=aug3)),
    }
    # what is timed is what the tests hold: "no blur" records give the colour entry's batch, and the two-stage batch is the second stage on stage 1's bytes
    assert torch.equal(arms["b"][1](0), arms["a"][1](1)) and not torch.equal(arms["d2"][1](2), arms["a"][1](3))
    assert torch.equal(arms["g"][1](0), arms["c"][1](1)) and torch.equal(arms["h"][1](2), arms["a"][1](3))
    reps = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, (_, run) in arms.items():
            reps[k].append(timed(run, args))
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    lds = lambda band, sides: 3072 + (sides + 1) * (band + 12) * 3 * D   # noqa: E731
    mr = (16 * D + D - 1) // D + 5
    colour_lds = D * 5 * 4 + 768 * 4 + ((mr * D * 3 + 15) & ~15) + mr * 3 * D
    lines = [f"bytes-in blur form, batch {B}, D = {D}, us per batch: HIP events around {args.launches} launches after {args.warmup} warm-up launches per "
             f"arm, {args.reps} repetitions interleaved in this one process, fp32 output rotating over 616 MB; the second-stage arms on the same staged "
             f"bytes (stage 1 of 256 x 256 sources, formed once), erase records of the default RandomErasing, records drawn once with seed 1; "
             f"{torch.cuda.get_device_name(0)}; clocks as the machine had them (not pinned, not changed, not read).  (a) .. (e) are three stream "
             "operations per batch (the zeroing of sums, the statistics launch, the batch launch), (g) and (h) four (stage 1 in front)",
             f"  records drawn: (c), (e), (g) {n_blur} of {B} blurred, the others grayscale or solarized; every sample holds three jitter ops"]
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<84} median {med[k]:8.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {spread[k]:.1f}")
    for k, base in (("b", "a"), ("c", "a"), ("d1", "a"), ("d2", "a"), ("c", "e"), ("d2", "f"), ("g", "h")):
        lines.append(f"  reported: ({k}) / ({base}) = {med[k] / med[base]:.3f}; ({k}) - ({base}) = {med[k] - med[base]:+.1f} us")
    lines.append(f"  the LDS request of a launch in which no record blurs, section 7v's finding here: (b) - (a) = {med['b'] - med['a']:+.1f} us against a "
                 f"run-to-run spread of (a) of {spread['a']:.1f} us.  LDS per workgroup: the new entry {lds(16, 1)} B without mix records ({lds(8, 2)} B with), "
                 f"the colour second stage {colour_lds} B: by LDS alone {LDS_PER_CU // lds(16, 1)} against {LDS_PER_CU // colour_lds} workgroups of a "
                 f"{LDS_PER_CU // 1024} KB CU (occupancy was not measured)")
    if alternated:
        for name in ("parent", "branch"):
            runs = [r for n, _, r in alternated if n == name]
            meds = [statistics.median(r) for r in runs]
            flat = [v for r in runs for v in r]
            lines.append(f"  (a) in fresh processes, alternating parent / branch, {name}: medians {', '.join(f'{m:.1f}' for m in meds)} "
                         f"(all repetitions {min(flat):.1f} .. {max(flat):.1f})")
        p = [v for n, _, r in alternated if n == "parent" for v in r]
        bm = [statistics.median(r) for n, _, r in alternated if n == "branch"]
        inside = all(min(p) <= m <= max(p) for m in bm)
        lines.append(f"  (a) at the branch inside the parent's own spread {min(p):.1f} .. {max(p):.1f}: {'yes' if inside else 'NO'}; mean of the medians, branch - "
                     f"parent = {statistics.mean(bm) - statistics.mean(statistics.median(r) for n, _, r in alternated if n == 'parent'):+.2f} us (reported, not a gate; the "
                     "machine code of the kernels of (a) is identical, profiles/wide_blur_isa_identity.txt)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
