#!/usr/bin/env python3
"""Measures the input pipeline (qat_vit_amd.GpuResizeNormalize / GpuImageLoader) on one MI355X and writes profiles/input_pipeline_bench.txt:

1. the host path of the reference loop on this box (Pillow Resize(224, BICUBIC) + ToTensor + Normalize per 32x32 image): images/s on one core and
   on 16 processes.  Runs first, before the GPU is opened, so the worker processes never hold it.
2. the kernel: time per batch of 256 from S = 32 out of a 50,000-image resident set with a random index, HIP events around 200 launches after 20
   warm-up launches, five repetitions, the output rotating over four buffers (616 MB, beyond the 256 MiB Infinity Cache) so that the stores go to HBM;
   its write rate next to the 8 TB/s peak and the 6.3 TB/s streaming stores reach on this part.
3. the one condition: the QAT step of the C2 shape (ViT-S/16, batch 256, qnnpack, no teacher; forward + loss + backward as bench.py times it), the
   same number of steps (a) on one resident fp32 batch and (b) drawing every batch from GpuImageLoader over the 50,000 uint8 images with
   shuffle=True, interleaved a, b, a, b, ... five times in this process, each window a host clock between two device synchronisations.
   (b) may exceed (a) by the kernel's time per batch plus the spread (max - min) of (a), and no more; the exit status says whether it held.

With --augment it measures only the augmenting form of the kernel and writes profiles/augment_bench.txt: three arms with
the method of 2., interleaved a, b, c, a, b, c, ... over the five repetitions - (a) qatvit_image_batch, (b) qatvit_image_batch_aug with the words of
RandomCropFlip(4) and constant padding, (c) the same with reflect padding.  (b) and (c) may exceed (a) by (a)'s own spread over its repetitions
plus 1 % of (a) - the extra bytes moved are at most the source bytes once more and 4 B per sample, against 154 MB written - and no more; the exit
status says whether it held.

usage: python3 tools/bench_input_pipeline.py [--steps K] [--warmup W] [--out FILE] [--augment]"""
import argparse
import multiprocessing
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BATCH_BYTES = 256 * 3 * 224 * 224 * 4


def host_images_per_second(n):
    """One process, one thread: n images through the reference transform's own expressions."""
    from PIL import Image

    torch.set_num_threads(1)
    im = Image.fromarray(np.random.default_rng(os.getpid()).integers(0, 256, (32, 32, 3), dtype=np.uint8))
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    t0 = time.perf_counter()
    for _ in range(n):
        r = im.resize((224, 224), Image.BICUBIC)
        x = torch.from_numpy(np.asarray(r).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        x.sub_(mean).div_(std)
    return n / (time.perf_counter() - t0)


def host_path(lines):
    try:
        import PIL
    except ImportError:
        lines.append("host path: Pillow is not installed on this box; an earlier session measured 805 images/s per core (Pillow 12.2, one thread)")
        return
    host_images_per_second(50)
    one = host_images_per_second(400)
    with multiprocessing.get_context("fork").Pool(16) as pool:
        t0 = time.perf_counter()
        pool.map(host_images_per_second, [400] * 16)
        many = 16 * 400 / (time.perf_counter() - t0)
    lines.append(f"host path (Pillow {PIL.__version__} resize + to-tensor + normalise, 32x32 -> 224x224): one core {one:.0f} images/s; "
                 f"16 processes {many:.0f} images/s")


CLOCK_NOTE = ("clocks: as the machine had them (not pinned, not changed, not read); every figure follows its own warm-up, the kernel's five "
              "repetitions and the interleaved step windows show the drift inside this run")


def kernel_time(lines, data, tr):
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randint(0, data.shape[0], (256,), device="cuda", generator=g)
    outs = [torch.empty(256, 3, 224, 224, device="cuda") for _ in range(4)]
    for i in range(20):
        tr(data, idx, out=outs[i % 4])
    reps = []
    for _ in range(5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(200):
            tr(data, idx, out=outs[i % 4])
        ev[1].record()
        torch.cuda.synchronize()
        reps.append(ev[0].elapsed_time(ev[1]) / 200)
    ms = statistics.median(reps)
    rate = BATCH_BYTES / (ms * 1e-3) / 1e12
    lines.append(f"kernel (batch 256, S = 32 -> 224, random index into 50,000 resident images): {ms * 1e3:.1f} us per batch "
                 f"(five repetitions of 200 launches: {', '.join(f'{r * 1e3:.1f}' for r in reps)} us)")
    lines.append(f"  writes {BATCH_BYTES / 1e6:.1f} MB -> {rate:.2f} TB/s = {rate / 8.0:.0%} of the 8 TB/s peak, {rate / 6.3:.0%} of the 6.3 TB/s "
                 f"streaming stores reach; {256 / (ms * 1e-3):,.0f} images/s")
    return ms


def augment_arms(lines, data, tr):
    import qat_vit_amd

    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randint(0, data.shape[0], (256,), device="cuda", generator=g)
    words = qat_vit_amd.RandomCropFlip(4).draw(256, torch.Generator().manual_seed(1)).cuda()
    outs = [torch.empty(256, 3, 224, 224, device="cuda") for _ in range(4)]
    arms = {"a": ("qatvit_image_batch", {}),
            "b": ("qatvit_image_batch_aug, constant padding, p = 4", {"aug": words, "padding_mode": "constant", "padding": 4}),
            "c": ("qatvit_image_batch_aug, reflect padding, p = 4", {"aug": words, "padding_mode": "reflect", "padding": 4})}
    for _, kw in arms.values():
        for i in range(20):
            tr(data, idx, out=outs[i % 4], **kw)
    reps = {k: [] for k in arms}
    for _ in range(5):
        for k, (_, kw) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(200):
                tr(data, idx, out=outs[i % 4], **kw)
            ev[1].record()
            torch.cuda.synchronize()
            reps[k].append(ev[0].elapsed_time(ev[1]) / 200 * 1e3)
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    allowed = med["a"] + spread["a"] + 0.01 * med["a"]
    lines.append("kernel with augmentation (batch 256, S = 32 -> 224, random index into 50,000 resident images, one word per sample), us per batch; "
                 "HIP events around 200 launches after 20 warm-up launches per arm, five repetitions interleaved a, b, c, output rotating over 616 MB:")
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<52} median {med[k]:.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {spread[k]:.1f}")
    ok = True
    for k in ("b", "c"):
        held = med[k] <= allowed
        ok = ok and held
        lines.append(f"  ({k}) / (a) = {med[k] / med['a']:.3f}; ({k}) - (a) = {med[k] - med['a']:+.1f} us; allowed: (a) {med['a']:.1f} + spread of (a) "
                     f"{spread['a']:.1f} + 1 % of (a) {0.01 * med['a']:.1f} = {allowed:.1f} us -> {'holds' if held else 'DOES NOT HOLD'}")
    return ok


def step_condition(lines, data, labels, tr, kernel_ms, steps, warmup):
    import qat_vit_amd
    from qat_vit_amd import functional as F
    from qat_vit_amd.engine import engine_of
    from torch.ao.quantization import get_default_qat_qconfig, prepare_qat

    torch.manual_seed(0)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda().train()
    stu.qconfig = get_default_qat_qconfig("qnnpack")
    model = prepare_qat(stu, inplace=False).cuda().train()
    loader = qat_vit_amd.GpuImageLoader(data, labels, 256, shuffle=True, drop_last=True, transform=tr, generator=torch.Generator().manual_seed(2))
    x0, y0 = next(iter(loader))
    with torch.no_grad():
        model(x0)
    params = engine_of(model).params
    feed = {"it": iter(loader)}

    def resident():
        return x0, y0

    def drawn():
        try:
            return next(feed["it"])
        except StopIteration:          # a new epoch, inside the timed window as in a training loop
            feed["it"] = iter(loader)
            return next(feed["it"])

    def window(batch, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            for p in params:
                p.grad = None
            x, y = batch()
            loss, _ = F.kd_ce_loss(model(x), None, y, 4.0, 0.5, 0.1)
            loss.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    window(resident, warmup), window(drawn, warmup)
    a, b = [], []
    for _ in range(5):
        a.append(window(resident, steps))
        b.append(window(drawn, steps))
    am, bm, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
    allowed = kernel_ms + spread
    ok = bm - am <= allowed
    fmt = lambda v: ", ".join(f"{t:.3f}" for t in v)   # noqa: E731
    lines.append(f"QAT step, C2 shape (ViT-S/16, batch 256, qnnpack, no teacher), {steps} steps per window, five interleaved windows each, ms per step:")
    lines.append(f"  (a) one resident fp32 batch:            median {am:.3f}  ({fmt(a)}); spread {spread:.3f}")
    lines.append(f"  (b) every batch from GpuImageLoader:    median {bm:.3f}  ({fmt(b)})")
    lines.append(f"  (b) - (a) = {bm - am:+.3f} ms; allowed: kernel {kernel_ms:.3f} + spread of (a) {spread:.3f} = {allowed:.3f} ms -> {'holds' if ok else 'DOES NOT HOLD'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="profiles/input_pipeline_bench.txt, or profiles/augment_bench.txt with --augment")
    ap.add_argument("--augment", action="store_true", help="only the three arms of the augmenting kernel")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "augment_bench.txt" if args.augment else "input_pipeline_bench.txt")
    lines = []
    if not args.augment:
        host_path(lines)                  # before the first CUDA call: the pool's processes are forked from a process without a GPU context
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_pipeline.py needs an MI355X: there is no CPU form of the pipeline to time")
    import qat_vit_amd

    g = torch.Generator(device="cuda").manual_seed(0)
    data = torch.randint(0, 256, (50000, 32, 32, 3), device="cuda", generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (50000,), device="cuda", generator=g)
    tr = qat_vit_amd.GpuResizeNormalize(32)
    lines.insert(0, f"input pipeline on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if args.augment:
        ok = augment_arms(lines, data, tr)
    else:
        kernel_ms = kernel_time(lines, data, tr)
        ok = step_condition(lines, data, labels, tr, kernel_ms, args.steps, args.warmup)
    lines.append(CLOCK_NOTE)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
