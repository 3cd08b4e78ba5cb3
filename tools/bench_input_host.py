#!/usr/bin/env python3
"""Measures the host cost of GpuImageLoader's epoch on one MI355X, for this checkout and, with --other DIR, for another checkout of the project
(e.g. the parent commit's, built) in the same process, the two alternated, and writes profiles/input_host_one_body_bench.txt.

Data: 50,000 synthetic uint8 32 x 32 images resident on the device, batch 256, drop_last, D = 224 (condition (b) of
tools/bench_input_pipeline.py): 195 batches per epoch.  Three option sets - none; augment + mix + erase + color + blur; crop + mix + erase +
three_augment - each with the real transform (``for batch in loader: pass``, then one ``torch.cuda.synchronize()``) and with a null transform
that returns one preallocated tensor: the kernels hide the Python cost per batch, the null transform shows it.  An epoch holds the plan, the
record draws, the one copy and the per-batch slicing.  Per arm one warm-up epoch per tree, then five timed epochs per tree, alternated other,
this, other, this, ...; the median and the min .. max range of each, in ms per epoch.

The condition, per arm: this checkout's median is at most the other's median plus the other's own min-to-max spread.  The exit status says
whether it held for every arm (0 without --other: nothing is compared).

usage: python3 tools/bench_input_host.py [--other DIR] [--out FILE]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
N, BATCH, EPOCHS = 50000, 256, 5


def load(root, name):
    """The package of the checkout at `root` under the module name `name` (what qat_vit_amd.py does for its own)."""
    d = os.path.join(root, "qat-vit_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Null:
    """Takes what a transform takes and returns one preallocated tensor."""

    def __init__(self, device, out_size):
        self.device, self.out_size, self.x = device, out_size, torch.zeros(1, device=device)

    def __call__(self, data, index, **kw):
        return self.x


def option_sets(q):
    return {"none": {},
            "augment + mix + erase + color + blur": dict(augment=q.RandomCropFlip(4), mix=q.MixupCutmix(), erase=q.RandomErasing(),
                                                         color=q.ColorJitter(0.4, 0.4, 0.4), blur=q.GaussianBlur(p=0.5)),
            "crop + mix + erase + three_augment": dict(crop=q.RandomResizedCrop(), mix=q.MixupCutmix(), erase=q.RandomErasing(),
                                                       three_augment=q.ThreeAugment())}


def epoch_ms(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for batch in loader:
        pass
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None, help="the root of another checkout of the project, built, to measure next to this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_host_one_body_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_host.py needs an MI355X: the loader's data set lives on the device")
    trees = ([("other", load(os.path.abspath(args.other), "qat_vit_amd_other"))] if args.other else []) + [("this", load(ROOT, "qat_vit_amd"))]
    g = torch.Generator(device="cuda").manual_seed(0)
    data = torch.randint(0, 256, (N, 32, 32, 3), device="cuda", generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (N,), device="cuda", generator=g)
    lines = [f"host cost of GpuImageLoader's epoch on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"{N} uint8 32 x 32 images on the device, batch {BATCH}, shuffle, drop_last, D = 224: {N // BATCH} batches per epoch; ms per epoch (plan, record "
             f"draws, one copy, {N // BATCH} x slice + transform + label gather, one synchronize); one warm-up epoch per tree and arm, then {EPOCHS} timed "
             f"epochs per tree, alternated " + ", ".join(t for t, _ in trees) + ", ...",
             "real: GpuResizeNormalize(32); null: a transform that returns one preallocated tensor (the Python cost per batch, which the kernels hide)"]
    ok = True
    for which in ("real", "null"):
        for name in option_sets(trees[0][1]):
            loaders = {}
            for tree, q in trees:
                tr = q.GpuResizeNormalize(32) if which == "real" else Null(torch.device("cuda", torch.cuda.current_device()), 224)
                loaders[tree] = q.GpuImageLoader(data, labels, BATCH, shuffle=True, drop_last=True, transform=tr, generator=torch.Generator().manual_seed(2),
                                                 **option_sets(q)[name])
                epoch_ms(loaders[tree])
            ms = {tree: [] for tree in loaders}
            for _ in range(EPOCHS):
                for tree, loader in loaders.items():
                    ms[tree].append(epoch_ms(loader))
            lines.append(f"{which}, {name}:")
            for tree, v in ms.items():
                lines.append(f"  {tree + ':':<7} median {statistics.median(v):8.2f}  range {min(v):.2f} .. {max(v):.2f}  ({', '.join(f'{t:.2f}' for t in v)});"
                             f"  {statistics.median(v) / (N // BATCH) * 1e3:.1f} us per batch")
            if "other" in ms:
                med, allowed = statistics.median(ms["this"]), statistics.median(ms["other"]) + max(ms["other"]) - min(ms["other"])
                ok = ok and med <= allowed
                lines.append(f"  this / other = {med / statistics.median(ms['other']):.3f}; allowed: other's median + its spread = {allowed:.2f} ms -> "
                             f"{'holds' if med <= allowed else 'DOES NOT HOLD'}")
    lines.append("clocks: as the machine had them (not pinned, not changed, not read); the alternation of the two trees shows the drift inside this run")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
