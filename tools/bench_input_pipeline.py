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

With --mix it measures only the mixing form of the kernel and writes profiles/mix_bench.txt: five arms with the method of
2., interleaved over the five repetitions - (a) qatvit_image_batch_aug alone, (b) what a user composes for mixup without the entry: (a) +
index_select of the partners + two mul + add, (c) qatvit_image_batch_mix with mixup records, every partner another position, (d) the same with
cutmix records whose box is about half the area, (e) the same with identity records.  The condition: (c) and (d) no slower than (b)'s median; the
exit status says whether it held.  (e) against (a) is reported.  --note FILE appends that file's text (the machine-code comparison, the register
report) to the output.

With --rrc it measures only the resized-crop forms of the kernel and writes profiles/rrc_bench.txt: six arms with the
method of 2., interleaved over the five repetitions in the one process, the records of the default RandomResizedCrop - (a) qatvit_image_batch,
(b) qatvit_image_batch_rrc, (c) / (e) qatvit_image_batch_mix with the words of RandomCropFlip(4) and the mixup / cutmix records of --mix,
(d) / (f) qatvit_image_batch_rrc with the same mix records.  The expectation under test: (b) within 10 % of (a), (d) of (c), (f) of (e); the exit
status says whether it held.  --note FILE appends that file's text as with --mix.

With --erase it measures only the erasing forms of the kernel and writes profiles/erase_bench.txt: twelve arms with the
method of 2., interleaved over the five repetitions in the one process, the records of the default RandomErasing - (a) qatvit_image_batch_aug,
(b) / (b') what a user composes today: (a) + a slice assignment / a normal_() on a view per erased sample, (c) / (d) qatvit_image_batch_erase with
those records, const / pixel noise, (c<), (d<) / (d>) the records of (c), (d) with the erased samples at the first / last
batch positions, (e) every sample erased over a third of its area with noise, (f) identity records, (g) / (h) rrc + mixup
without / with the pixel-noise records.  The condition: (c) faster than (b) and (d) than (b'), beyond both arms' spreads; the exit status says
whether it held.  (c), (d), (f) against (a), (h) against (g) and (e) are reported, and so is the largest deviation of the kernel's noise from the
fp64 evaluation of its formula.  --note FILE appends that file's text as with --mix.

With --blur it measures only the blur forms against the colour entry on records without blur and writes
profiles/blur_bench.txt: the colour entry, the blur entry with "no blur" records, ThreeAugment records, every sample blurred at radius 0.1 and at
2.0, and box convolutions as torch ops for scale.
With --color it measures only the colour forms of the kernel and writes profiles/color_bench.txt: eight arms with the method
of 2., interleaved over the five repetitions in the one process - (a) the erase entry of the parent with the default erase records, (b) the colour
entry with the records of ColorJitter(0.4, 0.4, 0.4) and the same erase records, (b-) the same records without the workspace (no statistics
launch), (c) jitter(0.4, 0, 0.4), (d) / (d-) identity colour records with / without the workspace, (e) the 3-Augment records, (f) the same chain
as torch ops on the float batch (time only).  Every comparison is against (a), the parent's entry; nothing is required, the figures are
reported.  --note FILE appends that file's text as with --mix.

usage: python3 tools/bench_input_pipeline.py [--steps K] [--warmup W] [--out FILE] [--augment | --mix | --rrc | --erase | --color | --blur [--note FILE]]"""
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


def mix_arms(lines, data, tr):
    import qat_vit_amd

    B, D = 256, 224
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randint(0, data.shape[0], (B,), device="cuda", generator=g)
    words = qat_vit_amd.RandomCropFlip(4).draw(B, torch.Generator().manual_seed(1)).cuda()
    kw = {"aug": words, "padding_mode": "constant", "padding": 4}
    bits = lambda v: int(np.float32(v).view(np.int32))   # noqa: E731
    lam = np.random.default_rng(1).beta(0.8, 0.8, B).astype(np.float32)
    partner = [B - 1 - b for b in range(B)]              # the flip: every partner is another position
    mixup = torch.tensor([[p, bits(l), bits(np.float32(1) - l), 0, 0, bits(l)] for p, l in zip(partner, lam)], dtype=torch.int32).cuda()
    y0, y1, x0, x1 = 33, 191, 33, 192                    # 158 x 159 of 224 x 224: 0.5007 of the area, edges off the band and float4 grids
    area = (y1 - y0) * (x1 - x0) / float(D * D)
    cutmix = torch.tensor([[p, bits(1), 0, y0 | y1 << 16, x0 | x1 << 16, bits(1 - area)] for p in partner], dtype=torch.int32).cuda()
    ident = torch.tensor([[p, bits(1), 0, 0, 0, bits(1)] for p in partner], dtype=torch.int32).cuda()
    part = torch.tensor(partner, device="cuda")
    ws, wp = torch.from_numpy(lam).cuda().view(B, 1, 1, 1), torch.from_numpy(np.float32(1) - lam).cuda().view(B, 1, 1, 1)
    outs = [torch.empty(B, 3, D, D, device="cuda") for _ in range(4)]

    def composed(i):
        x = tr(data, idx, out=outs[i % 4], **kw)
        return torch.add(x.mul(ws), x.index_select(0, part).mul(wp))

    arms = {"a": ("qatvit_image_batch_aug alone", lambda i: tr(data, idx, out=outs[i % 4], **kw)),
            "b": ("(a) + index_select + two mul + add (mixup today)", composed),
            "c": ("qatvit_image_batch_mix, mixup records", lambda i: tr(data, idx, out=outs[i % 4], mix=mixup, **kw)),
            "d": (f"qatvit_image_batch_mix, cutmix, box {area:.3f} of the area", lambda i: tr(data, idx, out=outs[i % 4], mix=cutmix, **kw)),
            "e": ("qatvit_image_batch_mix, identity records", lambda i: tr(data, idx, out=outs[i % 4], mix=ident, **kw))}
    assert torch.equal(arms["c"][1](0), composed(1)) and torch.equal(arms["e"][1](2), arms["a"][1](3))
    for _, run in arms.values():
        for i in range(20):
            run(i)
    reps = {k: [] for k in arms}
    for _ in range(5):
        for k, (_, run) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(200):
                run(i)
            ev[1].record()
            torch.cuda.synchronize()
            reps[k].append(ev[0].elapsed_time(ev[1]) / 200 * 1e3)
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    lines.append("kernel with mixup / cutmix (batch 256, S = 32 -> 224, random index into 50,000 resident images, words of RandomCropFlip(4), constant "
                 "padding), us per batch; HIP events around 200 launches after 20 warm-up launches per arm, five repetitions interleaved a .. e, output "
                 "rotating over 616 MB:")
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<58} median {med[k]:.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {spread[k]:.1f}")
    ok = True
    for k in ("c", "d"):
        held = med[k] <= med["b"]
        ok = ok and held
        lines.append(f"  ({k}) / (b) = {med[k] / med['b']:.3f}; ({k}) / (a) = {med[k] / med['a']:.3f}; the condition ({k}) <= (b)'s median {med['b']:.1f} us -> "
                     f"{'holds' if held else 'DOES NOT HOLD'}")
    allowed = med["a"] + spread["a"] + 0.01 * med["a"]
    lines.append(f"  reported, not required: (e) / (a) = {med['e'] / med['a']:.3f}; (e) - (a) = {med['e'] - med['a']:+.1f} us; (a) + spread of (a) "
                 f"{spread['a']:.1f} + 1 % of (a) = {allowed:.1f} us -> {'within' if med['e'] <= allowed else 'NOT within'}")
    lines.append(f"  LDS per workgroup: aug kernel {lds_bytes(32, D)[0]} B, mix kernel {lds_bytes(32, D)[1]} B")
    return ok


def rrc_arms(lines, data, tr):
    import qat_vit_amd

    B, D = 256, 224
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randint(0, data.shape[0], (B,), device="cuda", generator=g)
    host_windows = qat_vit_amd.RandomResizedCrop().draw(B, 32, torch.Generator().manual_seed(1))
    windows = host_windows.cuda()
    words = qat_vit_amd.RandomCropFlip(4).draw(B, torch.Generator().manual_seed(1)).cuda()
    kw = {"aug": words, "padding_mode": "constant", "padding": 4}
    bits = lambda v: int(np.float32(v).view(np.int32))   # noqa: E731
    lam = np.random.default_rng(1).beta(0.8, 0.8, B).astype(np.float32)
    partner = [B - 1 - b for b in range(B)]              # the flip: every partner is another position
    mixup = torch.tensor([[p, bits(l), bits(np.float32(1) - l), 0, 0, bits(l)] for p, l in zip(partner, lam)], dtype=torch.int32).cuda()
    y0, y1, x0, x1 = 33, 191, 33, 192                    # the box of --mix: 0.5007 of the area, edges off the band and float4 grids
    area = (y1 - y0) * (x1 - x0) / float(D * D)
    cutmix = torch.tensor([[p, bits(1), 0, y0 | y1 << 16, x0 | x1 << 16, bits(1 - area)] for p in partner], dtype=torch.int32).cuda()
    whole = torch.tensor([[0, 32 | 32 << 15]] * B, dtype=torch.int32).cuda()
    part = torch.tensor(partner, device="cuda")
    ws, wp = torch.from_numpy(lam).cuda().view(B, 1, 1, 1), torch.from_numpy(np.float32(1) - lam).cuda().view(B, 1, 1, 1)
    outs = [torch.empty(B, 3, D, D, device="cuda") for _ in range(4)]
    arms = {"a": ("qatvit_image_batch", lambda i: tr(data, idx, out=outs[i % 4])),
            "b": ("qatvit_image_batch_rrc", lambda i: tr(data, idx, out=outs[i % 4], rrc=windows)),
            "c": ("qatvit_image_batch_mix, words of RandomCropFlip(4), mixup", lambda i: tr(data, idx, out=outs[i % 4], mix=mixup, **kw)),
            "d": ("qatvit_image_batch_rrc, mixup records", lambda i: tr(data, idx, out=outs[i % 4], rrc=windows, mix=mixup)),
            "e": (f"qatvit_image_batch_mix, words, cutmix, box {area:.3f}", lambda i: tr(data, idx, out=outs[i % 4], mix=cutmix, **kw)),
            "f": (f"qatvit_image_batch_rrc, cutmix, box {area:.3f}", lambda i: tr(data, idx, out=outs[i % 4], rrc=windows, mix=cutmix))}
    # what is timed is what the tests hold: the whole-image record is the plain call, and the mixed call is the composition of the rrc batch
    assert torch.equal(tr(data, idx, rrc=whole), arms["a"][1](0))
    x = arms["b"][1](1)
    assert torch.equal(arms["d"][1](2), torch.add(x.mul(ws), x.index_select(0, part).mul(wp)))
    for _, run in arms.values():
        for i in range(20):
            run(i)
    reps = {k: [] for k in arms}
    for _ in range(5):
        for k, (_, run) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(200):
                run(i)
            ev[1].record()
            torch.cuda.synchronize()
            reps[k].append(ev[0].elapsed_time(ev[1]) / 200 * 1e3)
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    h, w = (host_windows[:, 1] & 0x7fff).double(), (host_windows[:, 1] >> 15 & 0x7fff).double()
    lines.append("kernel with the resized crop (batch 256, S = 32 -> 224, random index into 50,000 resident images, one record of the default "
                 "RandomResizedCrop per sample), us per batch; HIP events around 200 launches after 20 warm-up launches per arm, five repetitions "
                 "interleaved a .. f in this one process, output rotating over 616 MB:")
    lines.append(f"  windows drawn: h {int(h.min())} .. {int(h.max())} (mean {float(h.mean()):.1f}), w {int(w.min())} .. {int(w.max())} (mean {float(w.mean()):.1f})")
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<62} median {med[k]:.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {spread[k]:.1f}")
    ok = True
    for k, base in (("b", "a"), ("d", "c"), ("f", "e")):
        held = med[k] <= 1.10 * med[base]
        ok = ok and held
        lines.append(f"  ({k}) / ({base}) = {med[k] / med[base]:.3f}; ({k}) - ({base}) = {med[k] - med[base]:+.1f} us; the expectation ({k}) <= 1.10 x ({base}) = "
                     f"{1.10 * med[base]:.1f} us -> {'holds' if held else 'DOES NOT HOLD'}")
    lines.append(f"  every arm writes {BATCH_BYTES / 1e6:.1f} MB; (b) -> {BATCH_BYTES / (med['b'] * 1e-6) / 1e12:.2f} TB/s, (a) -> "
                 f"{BATCH_BYTES / (med['a'] * 1e-6) / 1e12:.2f} TB/s")
    lines.append(f"  LDS per workgroup: plain kernel {lds_bytes(32, D)[0]} B, rrc kernel {lds_bytes(32, D)[0] + 320} B, mix kernel {lds_bytes(32, D)[1]} B, "
                 f"rrc-mix kernel {lds_bytes(32, D)[1] + 640} B")
    return ok


def erase_arms(lines, data, tr):
    import qat_vit_amd
    from tests import erase_ref

    B, D = 256, 224
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randint(0, data.shape[0], (B,), device="cuda", generator=g)
    words = qat_vit_amd.RandomCropFlip(4).draw(B, torch.Generator().manual_seed(1)).cuda()
    kw = {"aug": words, "padding_mode": "constant", "padding": 4}
    host_const = qat_vit_amd.RandomErasing().draw(B, D, torch.Generator().manual_seed(1))
    host_pixel = qat_vit_amd.RandomErasing(value="random").draw(B, D, torch.Generator().manual_seed(1))
    const, pixel, ident = host_const.cuda(), host_pixel.cuda(), torch.zeros(B, 8, dtype=torch.int32, device="cuda")
    assert torch.equal(host_const[:, :2], host_pixel[:, :2])
    # the same pixel-noise records with the erased samples at the first / the last batch positions: the workgroups of a launch start in the order
    # of the positions, so these two arms show what the place of the touched workgroups inside the launch costs
    hit = host_pixel.any(1)
    first, last = torch.cat([host_pixel[hit], host_pixel[~hit]]).cuda(), torch.cat([host_pixel[~hit], host_pixel[hit]]).cuda()
    const_first = torch.cat([host_const[hit], host_const[~hit]]).cuda()
    # the worst case: every sample erased, a box of one third of the area (129 x 129 of 224 x 224, edges off the band and float4 grids), noise
    y0, y1, x0, x1 = 47, 176, 46, 175
    rng = np.random.default_rng(1)
    third = torch.tensor([erase_ref.pack(y0, y1, x0, x1, mode=1, key=(int(k[0]), int(k[1]))) for k in rng.integers(0, 1 << 32, (B, 2))],
                         dtype=torch.int32).cuda()
    boxes = [(b,) + erase_ref.unpack(r)[:4] for b, r in enumerate(host_const.tolist()) if any(r)]
    fills = [torch.tensor(erase_ref.unpack(r)[4], device="cuda").view(3, 1, 1) for r in host_const.tolist() if any(r)]
    host_windows = qat_vit_amd.RandomResizedCrop().draw(B, 32, torch.Generator().manual_seed(1)).cuda()
    bits = lambda v: int(np.float32(v).view(np.int32))   # noqa: E731
    lam = np.random.default_rng(1).beta(0.8, 0.8, B).astype(np.float32)
    mixup = torch.tensor([[B - 1 - b, bits(l), bits(np.float32(1) - l), 0, 0, bits(l)] for b, l in enumerate(lam)], dtype=torch.int32).cuda()
    outs = [torch.empty(B, 3, D, D, device="cuda") for _ in range(4)]

    def loop_fill(i):
        x = tr(data, idx, out=outs[i % 4], **kw)
        for (b, r0, r1, c0, c1), f in zip(boxes, fills):
            x[b, :, r0:r1, c0:c1] = f
        return x

    def loop_normal(i):
        x = tr(data, idx, out=outs[i % 4], **kw)
        for b, r0, r1, c0, c1 in boxes:
            x[b, :, r0:r1, c0:c1].normal_()
        return x

    arms = {"a": ("qatvit_image_batch_aug, words of RandomCropFlip(4)", lambda i: tr(data, idx, out=outs[i % 4], **kw)),
            "b": (f"(a) + a slice assignment per erased sample ({len(boxes)} of 256)", loop_fill),
            "b'": (f"(a) + normal_() on a view per erased sample ({len(boxes)} of 256)", loop_normal),
            "c": ("qatvit_image_batch_erase, default records, const", lambda i: tr(data, idx, out=outs[i % 4], erase=const, **kw)),
            "d": ("qatvit_image_batch_erase, the same boxes, pixel noise", lambda i: tr(data, idx, out=outs[i % 4], erase=pixel, **kw)),
            "c<": ("(c) with the erased samples at the first positions", lambda i: tr(data, idx, out=outs[i % 4], erase=const_first, **kw)),
            "d<": ("(d) with the erased samples at the first positions", lambda i: tr(data, idx, out=outs[i % 4], erase=first, **kw)),
            "d>": ("(d) with the erased samples at the last positions", lambda i: tr(data, idx, out=outs[i % 4], erase=last, **kw)),
            "e": ("qatvit_image_batch_erase, every sample, 1/3 of the area, noise", lambda i: tr(data, idx, out=outs[i % 4], erase=third, **kw)),
            "f": ("qatvit_image_batch_erase, identity records", lambda i: tr(data, idx, out=outs[i % 4], erase=ident, **kw)),
            "g": ("qatvit_image_batch_rrc, mixup records", lambda i: tr(data, idx, out=outs[i % 4], rrc=host_windows, mix=mixup)),
            "h": ("qatvit_image_batch_rrc_erase, mixup, default pixel noise", lambda i: tr(data, idx, out=outs[i % 4], rrc=host_windows, mix=mixup,
                                                                                          erase=pixel))}
    # what is timed is what the tests hold: the entry equals the loop for constant fills, and identity records give the aug call
    assert torch.equal(arms["c"][1](0), loop_fill(1)) and torch.equal(arms["f"][1](2), arms["a"][1](3))
    # the noise against the fp64 evaluation of the header's formula: eight whole-image records with keys of their own
    keys = [(int(k[0]), int(k[1])) for k in rng.integers(0, 1 << 32, (8, 2))]
    whole = torch.tensor([erase_ref.pack(0, D, 0, D, mode=1, key=k) for k in keys], dtype=torch.int32).cuda()
    z = tr(data, idx[:8].contiguous(), erase=whole).cpu().numpy().astype(np.float64)
    ref = np.stack([erase_ref.noise(k, D) for k in keys])
    dev = np.abs(z - ref)
    at = np.unravel_index(dev.argmax(), dev.shape)
    for _, run in arms.values():
        for i in range(20):
            run(i)
    reps = {k: [] for k in arms}
    for _ in range(5):
        for k, (_, run) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(200):
                run(i)
            ev[1].record()
            torch.cuda.synchronize()
            reps[k].append(ev[0].elapsed_time(ev[1]) / 200 * 1e3)
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    area = torch.tensor([(r1 - r0) * (c1 - c0) for _, r0, r1, c0, c1 in boxes]).double() / (D * D)
    lines.append("kernel with RandomErasing (batch 256, S = 32 -> 224, random index into 50,000 resident images, words of RandomCropFlip(4), constant "
                 "padding; records of the default RandomErasing, p = 0.25, seed 1), us per batch; HIP events around 200 launches after 20 warm-up "
                 "launches per arm, five repetitions interleaved a .. h in this one process, output rotating over 616 MB:")
    lines.append(f"  records drawn: {len(boxes)} of 256 erased, box area {float(area.min()):.3f} .. {float(area.max()):.3f} of the image (mean "
                 f"{float(area.mean()):.3f}); {float(area.sum()) / B:.4f} of all elements erased; (e): {(y1 - y0) * (x1 - x0) / (D * D):.3f} of every sample")
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<66} median {med[k]:.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {spread[k]:.1f}")
    ok = True
    for k, base in (("c", "b"), ("d", "b'")):
        held = med[k] + spread[k] + spread[base] < med[base]
        ok = ok and held
        lines.append(f"  ({k}) / ({base}) = {med[k] / med[base]:.3f}; the condition ({k}) + both spreads = {med[k] + spread[k] + spread[base]:.1f} us < ({base}) = "
                     f"{med[base]:.1f} us -> {'holds' if held else 'DOES NOT HOLD'}")
    for k, base in (("c", "a"), ("d", "a"), ("f", "a"), ("h", "g")):
        lines.append(f"  reported, not required: ({k}) / ({base}) = {med[k] / med[base]:.3f}; ({k}) - ({base}) = {med[k] - med[base]:+.1f} us; expected within "
                     f"10 %: {1.10 * med[base]:.1f} us -> {'within' if med[k] <= 1.10 * med[base] else 'NOT within'}")
    lines.append(f"  reported: (e) / (a) = {med['e'] / med['a']:.3f}; (e) - (a) = {med['e'] - med['a']:+.1f} us")
    lines.append(f"  reported: the place of the touched workgroups in the launch: (c<) - (a) = {med['c<'] - med['a']:+.1f} us, (c) - (a) = "
                 f"{med['c'] - med['a']:+.1f} us; (d<) - (a) = {med['d<'] - med['a']:+.1f} us, (d) - (a) = "
                 f"{med['d'] - med['a']:+.1f} us, (d>) - (a) = {med['d>'] - med['a']:+.1f} us")
    lines.append(f"  noise against the fp64 evaluation of the same formula (tests/erase_ref.py), {dev.size} elements of eight whole-image records: largest "
                 f"deviation {dev.max():.3e} (at z = {ref[at]:+.4f}), mean {dev.mean():.3e}; largest |z| {np.abs(ref).max():.3f}")
    lines.append(f"  LDS per workgroup: the erase forms request what their siblings request: aug {lds_bytes(32, D)[0]} B, rrc-mix {lds_bytes(32, D)[1] + 640} B")
    return ok


def color_arms(lines, data, tr):
    import qat_vit_amd
    from tests import color_ref

    B, D = 256, 224
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randint(0, data.shape[0], (B,), device="cuda", generator=g)
    words = qat_vit_amd.RandomCropFlip(4).draw(B, torch.Generator().manual_seed(1)).cuda()
    kw = {"aug": words, "padding_mode": "constant", "padding": 4}
    boxes = qat_vit_amd.RandomErasing().draw(B, D, torch.Generator().manual_seed(1)).cuda()
    host_full = qat_vit_amd.ColorJitter(0.4, 0.4, 0.4).draw(B, torch.Generator().manual_seed(1))
    host_two = qat_vit_amd.ColorJitter(0.4, 0, 0.4).draw(B, torch.Generator().manual_seed(1))
    host_aug3 = qat_vit_amd.ColorJitter(0.3, 0.3, 0.3, grayscale=1 / 3, solarize=1 / 3).draw(B, torch.Generator().manual_seed(1))
    full, two, aug3, ident = host_full.cuda(), host_two.cuda(), host_aug3.cuda(), torch.zeros(B, 4, dtype=torch.int32, device="cuda")
    outs = [torch.empty(B, 3, D, D, device="cuda") for _ in range(4)]
    # the same chain as torch ops on a float batch in [0, 255] (brightness, contrast, saturation in that order; for time only: no rounding to
    # bytes between the ops, so its values are not Pillow's)
    fac = host_full[:, 1:].contiguous().view(torch.float32).cuda()
    fb, fc, fs = (fac[:, k].view(B, 1, 1, 1) for k in range(3))
    lw = torch.tensor([0.299, 0.587, 0.114], device="cuda").view(1, 3, 1, 1)
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)

    def composed(i):
        x = tr(data, idx, out=outs[i % 4], **kw)
        x = (x * std + mean) * 255.0                                 # back to the byte range
        x = (x * fb).clamp_(0, 255)
        m = (x * lw).sum(1, keepdim=True).mean((2, 3), keepdim=True)
        x = (m + fc * (x - m)).clamp_(0, 255)
        l = (x * lw).sum(1, keepdim=True)
        x = (l + fs * (x - l)).clamp_(0, 255)
        return (x / 255.0 - mean) / std

    arms = {"a": ("qatvit_image_batch_erase, default erase records (the parent's entry)", lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, **kw)),
            "b": ("qatvit_image_batch_color, jitter(0.4, 0.4, 0.4), the same erase records", lambda i: tr(data, idx, out=outs[i % 4], erase=boxes,
                                                                                                       color=full, **kw)),
            "b-": ("(b)'s records without a workspace: contrast the identity, no statistics launch", lambda i: tr(data, idx, out=outs[i % 4], erase=boxes,
                                                                                                            color=full, contrast=False, **kw)),
            "c": ("qatvit_image_batch_color, jitter(0.4, 0, 0.4): contrast left out", lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=two,
                                                                                                contrast=False, **kw)),
            "d": ("qatvit_image_batch_color, identity records, with the workspace", lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=ident,
                                                                                              **kw)),
            "d-": ("qatvit_image_batch_color, identity records, no workspace", lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=ident,
                                                                                        contrast=False, **kw)),
            "e": ("3-Augment: gray 1/3, solarize 1/3, jitter(0.3, 0.3, 0.3)", lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=aug3, **kw)),
            "f": ("qatvit_image_batch_aug + the chain as torch ops on the float batch (time only)", composed)}
    # what is timed is what the tests hold: identity records give the erase entry's batch, and the sums are those of the host restatement
    assert torch.equal(arms["d"][1](0), arms["a"][1](1)) and torch.equal(arms["d-"][1](2), arms["a"][1](3))
    arms["b"][1](0)
    sums = (tr.color_sums(B).cpu().to(torch.int64) & 0xffffffff)
    assert int((sums > 0).sum()) == B
    for _, run in arms.values():
        for i in range(20):
            run(i)
    reps = {k: [] for k in arms}
    for _ in range(5):
        for k, (_, run) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(200):
                run(i)
            ev[1].record()
            torch.cuda.synchronize()
            reps[k].append(ev[0].elapsed_time(ev[1]) / 200 * 1e3)
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    n_gray = sum(color_ref.unpack(r)[1] for r in host_aug3.tolist())
    n_sol = sum(color_ref.unpack(r)[2] for r in host_aug3.tolist())
    lines.append("kernel with the colour augmentations (batch 256, S = 32 -> 224, random index into 50,000 resident images, words of RandomCropFlip(4), "
                 "constant padding, erase records of the default RandomErasing, colour records of ColorJitter drawn once with seed 1), us per batch; "
                 "HIP events around 200 launches after 20 warm-up launches per arm, five repetitions interleaved a .. f in this one process, output "
                 "rotating over 616 MB.  (b), (d), (e) are three stream operations per batch: the zeroing of sums, the statistics launch, the batch launch:")
    lines.append(f"  records drawn: (b) every sample holds three ops in a random order; (e) {n_gray} of 256 grayscale, {n_sol} of 256 solarized")
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<84} median {med[k]:.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {spread[k]:.1f}")
    for k, base in (("b", "a"), ("b-", "a"), ("c", "a"), ("d", "a"), ("d-", "a"), ("e", "a"), ("b", "f")):
        lines.append(f"  reported: ({k}) / ({base}) = {med[k] / med[base]:.3f}; ({k}) - ({base}) = {med[k] - med[base]:+.1f} us")
    lines.append(f"  the statistics launch and the zeroing, by difference: (b) - (b-) = {med['b'] - med['b-']:+.1f} us (this also holds the contrast op's own "
                 f"arithmetic in the batch launch); with records that ask for nothing (every workgroup returns at once): (d) - (d-) = "
                 f"{med['d'] - med['d-']:+.1f} us")
    lines.append(f"  LDS per workgroup: the colour forms request what their siblings request: aug {lds_bytes(32, D)[0]} B; the statistics launch the same")
    return True


def blur_arms(lines, data, tr):
    import qat_vit_amd
    from tests import blur_ref

    B, D = 256, 224
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randint(0, data.shape[0], (B,), device="cuda", generator=g)
    words = qat_vit_amd.RandomCropFlip(4).draw(B, torch.Generator().manual_seed(1)).cuda()
    kw = {"aug": words, "padding_mode": "constant", "padding": 4}
    boxes = qat_vit_amd.RandomErasing().draw(B, D, torch.Generator().manual_seed(1)).cuda()
    # (a): the colour bench's 3-Augment-style records (two independent coins, no blur); (c): ThreeAugment's one-of-three choice
    aug3 = qat_vit_amd.ColorJitter(0.3, 0.3, 0.3, grayscale=1 / 3, solarize=1 / 3).draw(B, torch.Generator().manual_seed(1)).cuda()
    col3, blur3 = qat_vit_amd.ThreeAugment().draw(B, torch.Generator().manual_seed(1))
    n_blur = int((blur3[:, 0] & 1).sum())
    col3, blur3 = col3.cuda(), blur3.cuda()
    none = torch.zeros(B, 4, dtype=torch.int32, device="cuda")
    all01 = torch.tensor([blur_ref.pack(0.1)] * B, dtype=torch.int32).cuda()      # box radius 0: 3 halo rows on each side
    all20 = torch.tensor([blur_ref.pack(2.0)] * B, dtype=torch.int32).cuda()      # box radius 1: 6 halo rows on each side
    outs = [torch.empty(B, 3, D, D, device="cuda") for _ in range(4)]
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    box3 = torch.full((3, 1, 3, 3), 1.0 / 9.0, device="cuda")

    def composed(i):
        # three 3 x 3 box passes as one depthwise convolution each on the float batch, replicated edge (time only: not Pillow's values)
        x = tr(data, idx, out=outs[i % 4], erase=boxes, color=aug3, **kw)
        x = (x * std + mean) * 255.0
        for _ in range(3):
            x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), box3, groups=3)
        return (x / 255.0 - mean) / std

    arms = {"a": ("qatvit_image_batch_color, 3-Augment-style records without blur (the parent's entry)",
                  lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=aug3, **kw)),
            "b": ("qatvit_image_batch_blur, the same colour records, every blur record \"no blur\"",
                  lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=aug3, blur=none, **kw)),
            "c": ("qatvit_image_batch_blur, ThreeAugment records", lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=col3, blur=blur3, **kw)),
            "d1": ("qatvit_image_batch_blur, (a)'s colour records, every sample blurred at radius 0.1",
                   lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=aug3, blur=all01, **kw)),
            "d2": ("qatvit_image_batch_blur, (a)'s colour records, every sample blurred at radius 2.0",
                   lambda i: tr(data, idx, out=outs[i % 4], erase=boxes, color=aug3, blur=all20, **kw)),
            "e": ("(a) + three 3 x 3 box convolutions as torch ops on the float batch (time only)", composed)}
    # what is timed is what the tests hold: "no blur" records give the colour entry's batch
    assert torch.equal(arms["b"][1](0), arms["a"][1](1)) and not torch.equal(arms["d2"][1](2), arms["a"][1](3))
    for _, run in arms.values():
        for i in range(20):
            run(i)
    reps = {k: [] for k in arms}
    for _ in range(5):
        for k, (_, run) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(200):
                run(i)
            ev[1].record()
            torch.cuda.synchronize()
            reps[k].append(ev[0].elapsed_time(ev[1]) / 200 * 1e3)
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    lines.append("kernel with Gaussian blur (batch 256, S = 32 -> 224, random index into 50,000 resident images, words of RandomCropFlip(4), constant "
                 "padding, erase records of the default RandomErasing, records drawn once with seed 1), us per batch; HIP events around 200 launches "
                 "after 20 warm-up launches per arm, five repetitions interleaved a .. e in this one process, output rotating over 616 MB.  Every arm "
                 "is three stream operations per batch: the zeroing of sums, the statistics launch, the batch launch:")
    lines.append(f"  records drawn: (c) {n_blur} of 256 blurred, the others grayscale or solarized; every sample holds three jitter ops")
    for k, (name, _) in arms.items():
        lines.append(f"  ({k}) {name + ':':<92} median {med[k]:.1f}  ({', '.join(f'{r:.1f}' for r in reps[k])}); spread {spread[k]:.1f}")
    for k, base in (("b", "a"), ("c", "a"), ("d1", "a"), ("d2", "a"), ("d2", "e")):
        lines.append(f"  reported: ({k}) / ({base}) = {med[k] / med[base]:.3f}; ({k}) - ({base}) = {med[k] - med[base]:+.1f} us")
    lines.append(f"  expectation (b) within the run-to-run spread of (a), {spread['a']:.1f} us: (b) - (a) = {med['b'] - med['a']:+.1f} us -> "
                 f"{'confirmed' if abs(med['b'] - med['a']) <= spread['a'] else 'REFUTED'} (reported, not a gate)")
    mr = (28 * 32 + D - 1) // D + 5
    one = D * 5 * 4 + 768 * 4 + ((mr * 32 * 3 + 15) & ~15) + mr * 3 * D
    lines.append(f"  LDS per workgroup: the blur forms request {((one + 15) & ~15) + 2 * 28 * 3 * D} B without mix records (aug), bands of 16 rows (8 with mix records); "
                 f"the colour forms {lds_bytes(32, D)[0]} B, bands of 16 rows")
    return True


def lds_bytes(S, D):
    """(aug kernel, mix kernel) dynamic LDS of one workgroup, as csrc/image.hip sizes them: tables, source rows, one or two plane sets."""
    mr = (16 * S + D - 1) // D + 5
    one = D * 5 * 4 + 768 * 4 + ((mr * S * 3 + 15) & ~15) + mr * 3 * D
    return one, one + mr * 3 * D


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
    ap.add_argument("--mix", action="store_true", help="only the five arms of the mixing kernel")
    ap.add_argument("--rrc", action="store_true", help="only the six arms of the resized-crop kernels")
    ap.add_argument("--erase", action="store_true", help="only the arms of the erasing kernels")
    ap.add_argument("--color", action="store_true", help="only the arms of the colour kernels")
    ap.add_argument("--blur", action="store_true", help="only the arms of the blur kernels")
    ap.add_argument("--note", default=None, help="with --mix, --rrc, --erase or --color: a text file appended to the output")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "blur_bench.txt" if args.blur else "color_bench.txt" if args.color else "erase_bench.txt" if args.erase else "rrc_bench.txt" if args.rrc else "mix_bench.txt" if args.mix else
                                "augment_bench.txt" if args.augment else "input_pipeline_bench.txt")
    lines = []
    if not args.augment and not args.mix and not args.rrc and not args.erase and not args.color and not args.blur:
        host_path(lines)                  # before the first CUDA call: the pool's processes are forked from a process without a GPU context
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_pipeline.py needs an MI355X: there is no CPU form of the pipeline to time")
    import qat_vit_amd

    g = torch.Generator(device="cuda").manual_seed(0)
    data = torch.randint(0, 256, (50000, 32, 32, 3), device="cuda", generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (50000,), device="cuda", generator=g)
    tr = qat_vit_amd.GpuResizeNormalize(32)
    lines.insert(0, f"input pipeline on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if args.blur:
        ok = blur_arms(lines, data, tr)
    elif args.color:
        ok = color_arms(lines, data, tr)
    elif args.erase:
        ok = erase_arms(lines, data, tr)
    elif args.rrc:
        ok = rrc_arms(lines, data, tr)
    elif args.mix:
        ok = mix_arms(lines, data, tr)
    elif args.augment:
        ok = augment_arms(lines, data, tr)
    else:
        kernel_ms = kernel_time(lines, data, tr)
        ok = step_condition(lines, data, labels, tr, kernel_ms, args.steps, args.warmup)
    lines.append(CLOCK_NOTE)
    if (args.mix or args.rrc or args.erase or args.color or args.blur) and args.note:
        lines.append("")
        lines.append(open(args.note).read().rstrip("\n"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
