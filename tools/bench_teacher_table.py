#!/usr/bin/env python3
"""Measures distillation from a teacher logit table (qat_vit_amd.TeacherLogitTable) on one MI355X and writes profiles/teacher_table_bench.txt.

The student step of the C2 shape (QAT ViT-S/16, batch 256, qnnpack; forward + loss + backward as bench.py times it), every batch drawn from
GpuImageLoader(shuffle=True, return_index=True) over 50,000 synthetic uint8 32x32 images, in three arms:
  (a) the live frozen ViT-B teacher (native forward) + kd_ce_loss       - the step of the reference loop;
  (b) the table + kd_ce_loss_table                                       - this feature;
  (c) no teacher (kd_ce_loss with teacher=None)                          - the floor: a step that has no teacher to pay for.
Windows of --steps steps, interleaved a, b, c, a, b, c, ... five times in this process after a warm-up window of each arm, each window a host
clock between two device synchronisations.  Also: the time to build the table (the teacher pass and the host digests separately), the two loss
kernels' own times (HIP events around 200 launches, five repetitions), the deviation of table rows from the live teacher and of the live teacher
from itself, and with --float-fp16 the same three arms for the fp16 float step (native_float(amp=True) under autocast + GradScaler + ClipAdamW).

The one condition: (b) - (c) <= the window spread (max - min) of (c) + what the table loss kernel takes beyond the CE-only launch of (c); i.e. a
table step costs what a step without a teacher costs.  The exit status says whether it held.  Reported next to it: (a) / (b), the build time and
the epochs of 195 steps after which the build has paid for itself.

usage: python3 tools/bench_teacher_table.py [--steps K] [--warmup W] [--float-fp16] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
N_IMAGES, BATCH, KD = 50000, 256, (4.0, 0.5, 0.1)
CLOCK_NOTE = ("clocks: as the machine had them (not pinned, not changed, not read); every figure follows its own warm-up, and the interleaved "
              "windows show the drift inside this run")


def fmt(v):
    return ", ".join(f"{t:.3f}" for t in v)


def loss_kernel_times(lines, table):
    import qat_vit_amd.functional as F

    g = torch.Generator(device="cuda").manual_seed(3)
    s = torch.randn(BATCH, table.C, device="cuda", generator=g)
    y = torch.randint(0, table.C, (BATCH,), device="cuda", generator=g)
    idx = torch.randint(0, table.N, (BATCH,), device="cuda", generator=g)
    t = table.rows(idx)
    forms = {"kd_ce_loss, teacher tensor": lambda: F.kd_ce_loss(s, t, y, *KD), "kd_ce_loss, teacher=None": lambda: F.kd_ce_loss(s, None, y, *KD),
             "kd_ce_loss_table": lambda: F.kd_ce_loss_table(s, table.logits, idx, y, *KD)}
    out = {}
    for name, fn in forms.items():
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
        out[name] = statistics.median(reps)
        lines.append(f"  {name:28s} {out[name] * 1e3:7.1f} us per call (five repetitions of 200 calls, launch and host glue included: "
                     f"{', '.join(f'{r * 1e3:.1f}' for r in reps)} us)")
    return out


def three_arms(lines, title, loader, teacher, table, forward_backward, params, steps, warmup, extra_ms):
    """forward_backward(x, loss_fn) runs one step's forward, loss_fn(logits) and backward."""
    from qat_vit_amd import functional as F

    feed = {"it": iter(loader)}

    def draw():
        try:
            return next(feed["it"])
        except StopIteration:          # a new epoch, inside the timed window as in a training loop
            feed["it"] = iter(loader)
            return next(feed["it"])

    def live(x, y, idx):
        with torch.no_grad():
            t = teacher(x)
        return lambda out: F.kd_ce_loss(out, t, y, *KD)

    arms = {"a": live, "b": lambda x, y, idx: (lambda out: table.loss(out, idx, y, *KD)), "c": lambda x, y, idx: (lambda out: F.kd_ce_loss(out, None, y, *KD))}

    def window(arm, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            for p in params:
                p.grad = None
            x, y, idx = draw()
            forward_backward(x, arms[arm](x, y, idx))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for arm in "abc":
        window(arm, warmup)
    w = {arm: [] for arm in "abc"}
    for _ in range(5):
        for arm in "abc":
            w[arm].append(window(arm, steps))
    med = {arm: statistics.median(w[arm]) for arm in "abc"}
    spread = max(w["c"]) - min(w["c"])
    allowed = spread + extra_ms
    ok = med["b"] - med["c"] <= allowed
    lines.append(f"{title}, {steps} steps per window, five interleaved windows per arm, ms per step:")
    lines.append(f"  (a) live ViT-B teacher + kd_ce_loss:   median {med['a']:.3f}  ({fmt(w['a'])})")
    lines.append(f"  (b) table + kd_ce_loss_table:          median {med['b']:.3f}  ({fmt(w['b'])})")
    lines.append(f"  (c) no teacher:                        median {med['c']:.3f}  ({fmt(w['c'])}); spread {spread:.3f}")
    lines.append(f"  (b) - (c) = {med['b'] - med['c']:+.3f} ms; allowed: spread of (c) {spread:.3f} + table loss kernel beyond the CE-only launch "
                 f"{extra_ms:.3f} = {allowed:.3f} ms -> {'holds' if ok else 'DOES NOT HOLD'}")
    lines.append(f"  (a) / (b) = {med['a'] / med['b']:.2f}x; images/s: (a) {BATCH / med['a'] * 1e3:,.0f}, (b) {BATCH / med['b'] * 1e3:,.0f}, (c) {BATCH / med['c'] * 1e3:,.0f}")
    return ok, med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--float-fp16", action="store_true", help="also the three arms for the fp16 float (pre-QAT) step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teacher_table_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_teacher_table.py needs an MI355X: there is no CPU form of the teacher or of the loss to time")
    import qat_vit_amd
    from qat_vit_amd import distill
    from qat_vit_amd.engine import engine_of
    from torch.ao.quantization import get_default_qat_qconfig, prepare_qat

    lines = [f"teacher logit table on {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    g = torch.Generator(device="cuda").manual_seed(0)
    data = torch.randint(0, 256, (N_IMAGES, 32, 32, 3), device="cuda", generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (N_IMAGES,), device="cuda", generator=g)
    tr = qat_vit_amd.GpuResizeNormalize(32)
    torch.manual_seed(1)
    teacher = qat_vit_amd.create_teacher("vit", num_classes=10).cuda().eval()
    for p in teacher.parameters():
        p.requires_grad = False

    # ---- the build: once cold (engine construction included), once more for the figure; the host digests on their own
    with torch.no_grad():
        teacher(tr(data, torch.arange(BATCH, device="cuda")))       # the engine of batch 256 exists, as in a loop that has run the teacher once
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = qat_vit_amd.TeacherLogitTable.build(teacher, data, transform=tr, batch_size=BATCH, labels=labels)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    distill.data_digest(data, labels), distill.param_digest(teacher)
    digest_s = time.perf_counter() - t0
    chunks = -(-N_IMAGES // BATCH)
    lines.append(f"build: {N_IMAGES:,} images, {chunks} teacher forwards at batch {BATCH} in form {table.meta['teacher_form']}, table {table.N} x {table.C} fp32 = "
                 f"{table.logits.numel() * 4 / 1e6:.1f} MB: {build_s:.2f} s in all, of which the host digests (150 MB of images, the teacher's "
                 f"parameters) {digest_s:.2f} s; teacher pass {(build_s - digest_s) / chunks * 1e3:.1f} ms per chunk")

    # ---- rows against the live teacher, and the live teacher against itself (two batch compositions of the same 256 images)
    with torch.no_grad():
        idx = torch.randperm(N_IMAGES, device="cuda", generator=g)[:BATCH].contiguous()
        a = teacher(tr(data, idx))
        b = teacher(tr(data, idx.flip(0).contiguous())).flip(0)
        dev_rows, dev_self = float((table.rows(idx) - a).abs().max()), float((a - b).abs().max())
        a80 = teacher(tr(data, idx[:80].contiguous()))
        dev80 = float((table.rows(idx[:80].contiguous()) - a80).abs().max())
    lines.append(f"rows: max |table - live teacher| over a shuffled batch of 256: {dev_rows:.3e}; of 80: {dev80:.3e}; live teacher against itself "
                 f"(the same 256 images in two orders): {dev_self:.3e}")

    lines.append("loss kernels, batch 256, 10 classes:")
    kt = loss_kernel_times(lines, table)
    extra_ms = max(0.0, kt["kd_ce_loss_table"] - kt["kd_ce_loss, teacher=None"])

    # ---- the QAT step
    torch.manual_seed(0)
    stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda().train()
    stu.qconfig = get_default_qat_qconfig("qnnpack")
    model = prepare_qat(stu, inplace=False).cuda().train()
    loader = qat_vit_amd.GpuImageLoader(data, labels, BATCH, shuffle=True, drop_last=True, transform=tr, generator=torch.Generator().manual_seed(2),
                                        return_index=True)
    with torch.no_grad():
        model(next(iter(loader))[0])

    def qat_step(x, loss_fn):
        loss_fn(model(x))[0].backward()

    ok, med = three_arms(lines, "QAT step, C2 shape (ViT-S/16, batch 256, qnnpack)", loader, teacher, table, qat_step, engine_of(model).params,
                         args.steps, args.warmup, extra_ms)
    per_epoch = len(loader)
    saved_s = (med["a"] - med["b"]) * per_epoch / 1e3
    lines.append(f"  break-even: the build's {build_s:.2f} s against {saved_s:.2f} s saved per epoch of {per_epoch} steps = "
                 f"{build_s / saved_s:.2f} epochs" if saved_s > 0 else "  break-even: never (the table arm is not faster)")

    if args.float_fp16:
        torch.manual_seed(0)
        fm = qat_vit_amd.native_float(qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda().train(), amp=True)
        opt = qat_vit_amd.ClipAdamW(fm.parameters(), lr=1e-4)
        scaler = torch.amp.GradScaler("cuda")

        def float_step(x, loss_fn):
            with torch.autocast("cuda", dtype=torch.float16):
                loss = loss_fn(fm(x).float())[0]
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()

        ok2, _ = three_arms(lines, "fp16 float step (native_float(amp=True), autocast + GradScaler + ClipAdamW), ViT-S/16, batch 256", loader, teacher,
                            table, float_step, list(fm.parameters()), args.steps, args.warmup, extra_ms)
        ok = ok and ok2
    lines.append(CLOCK_NOTE)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
