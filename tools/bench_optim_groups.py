#!/usr/bin/env python3
"""Measures the grouped optimizer step (ClipAdamW with param groups) on one MI355X and writes profiles/optim_groups_bench.txt.

The parameters of the ViT-S/16 student (152 tensors) with synthetic gradients in fixed buffers; `step(max_norm=1.0)` in three arms, each on its own
copy of the parameters:
  (a) ClipAdamW over ONE group                                         - qatvit_optim_grad_norm + qatvit_optim_adamw, the path that existed;
  (b) ClipAdamW over the 28 groups of vit_param_groups(layer_decay)    - qatvit_optim_grad_norm + qatvit_optim_adamw_groups;
  (c) stock clip_grad_norm_ + torch.optim.AdamW(foreach=True) over the same 28 groups - for context only, it gates nothing.
One warm-up window of each arm, then `--repeats` timed windows per arm, interleaved a, b, c, a, b, c, ... in this process; a window is `--steps`
steps under a host clock from a device synchronisation to a device synchronisation, reported as microseconds per step.  Also: the update launch
alone (qatvit_optim_adamw against qatvit_optim_adamw_groups on the tables of (a) and (b)), HIP events around 100 back-to-back calls, five
repetitions, with the HBM rate that follows from 28 bytes per parameter.

The one condition: median (b) - median (a) <= the spread (max - min) of (a)'s windows, i.e. grouping costs nothing beyond (a)'s own run-to-run
spread.  The exit status says whether it held; the figures are reported whatever they are.

Run it as one step under its own time limit, and chain steps with &&, so that a failing step starts nothing after it:
  timeout -k 10 300 python3 tools/bench_optim_groups.py && echo done

usage: python3 tools/bench_optim_groups.py [--steps N] [--repeats R] [--out FILE]"""
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
CLOCK_NOTE = ("clocks: as the machine had them (not pinned, not changed, not read); every figure follows its own warm-up, and the interleaved "
              "windows show the drift inside this run")


def fmt(v):
    return ", ".join(f"{t:.1f}" for t in v)


def update_alone(lines, one, many, numel):
    """Device time of the update launch of each entry, on the tables the two optimizers built."""
    from qat_vit_amd import native
    from qat_vit_amd.optim import _CHUNK

    L, st = native.lib(), native.stream_ptr()
    t1, t28 = one._live_tables(), many._live_tables()
    head = lambda t: (t["params"].data_ptr(), t["grads"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["numel"].data_ptr())   # noqa: E731
    rows = [(float(g["lr"]), 0.9, 0.999, 1e-8, float(g["weight_decay"]), 10) for g in t28["live"]]
    groups = (native.AdamWGroup * len(rows))(*rows)
    calls = (("qatvit_optim_adamw, 1 group", lambda: L.qatvit_optim_adamw(*head(t1), t1["ct"].data_ptr(), t1["ci"].data_ptr(), t1["n"], _CHUNK, 1e-3, 0.9, 0.999,
                                                                           1e-8, 0.05, 10, t1["out2"].data_ptr(), st)),
             (f"qatvit_optim_adamw_groups, {len(rows)} groups", lambda: L.qatvit_optim_adamw_groups(*head(t28), t28["tg"].data_ptr(), t28["ct"].data_ptr(), t28["ci"].data_ptr(),
                                                                                                     t28["n"], _CHUNK, groups, len(rows), t28["out2"].data_ptr(), st)))
    reps = {name: [] for name, _ in calls}
    for name, fn in calls:
        for _ in range(20):
            native.check(fn(), name)
    for _ in range(5):
        for name, fn in calls:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(100):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            reps[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / 100)
    for name, _ in calls:
        med = statistics.median(reps[name])
        lines.append(f"  {name:40s} {med:7.1f} us per launch ({fmt(reps[name])}); 28 B x {numel:,} parameters = {28 * numel / med / 1e6:.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_groups_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_groups.py needs an MI355X: there is no CPU form of the optimizer kernels to time")
    import qat_vit_amd
    from qat_vit_amd import ClipAdamW, vit_param_groups

    torch.manual_seed(0)
    first = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda()
    models = {"a": first, "b": copy.deepcopy(first), "c": copy.deepcopy(first)}
    g = torch.Generator(device="cuda").manual_seed(1)
    for m in models.values():
        for p in m.parameters():
            p.grad = torch.randn(p.shape, device="cuda", generator=g) * 0.01
    numel = sum(p.numel() for p in models["a"].parameters())
    layout = dict(weight_decay=0.05, lr=1e-3, layer_decay=0.75)
    opt_a = ClipAdamW(models["a"].parameters(), lr=1e-3, weight_decay=0.05)
    opt_b = ClipAdamW(vit_param_groups(models["b"], **layout))
    opt_c = torch.optim.AdamW(vit_param_groups(models["c"], **layout), foreach=True)
    params_c = list(models["c"].parameters())

    def stock():
        torch.nn.utils.clip_grad_norm_(params_c, 1.0)
        opt_c.step()

    arms = {"a": lambda: opt_a.step(max_norm=1.0), "b": lambda: opt_b.step(max_norm=1.0), "c": stock}

    def window(arm):
        fn = arms[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.steps

    lines = [f"optimizer step with param groups on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"ViT-S/16 student: {len(params_c)} tensors, {numel:,} parameters; (b) and (c): {len(opt_b.param_groups)} groups "
             f"(vit_param_groups, weight_decay 0.05, lr 1e-3, layer_decay 0.75)"]
    for arm in "abc":
        window(arm)                                        # the warm-up window of each arm
    w = {arm: [] for arm in "abc"}
    for _ in range(args.repeats):
        for arm in "abc":
            w[arm].append(window(arm))
    med = {arm: statistics.median(w[arm]) for arm in "abc"}
    spread = {arm: max(w[arm]) - min(w[arm]) for arm in "abc"}
    ok = med["b"] - med["a"] <= spread["a"]
    lines.append(f"step(max_norm=1.0): {args.repeats} interleaved windows of {args.steps} steps per arm after one warm-up window each, us per step (host clock, "
                 "synchronised at both ends):")
    lines.append(f"  (a) ClipAdamW, 1 group (qatvit_optim_adamw):            median {med['a']:.1f}  ({fmt(w['a'])}); spread {spread['a']:.1f}")
    lines.append(f"  (b) ClipAdamW, {len(opt_b.param_groups)} groups (qatvit_optim_adamw_groups):   median {med['b']:.1f}  ({fmt(w['b'])}); spread {spread['b']:.1f}")
    lines.append(f"  (c) stock clip_grad_norm_ + AdamW(foreach=True), {len(opt_c.param_groups)} groups: median {med['c']:.1f}  ({fmt(w['c'])}); spread {spread['c']:.1f}")
    lines.append(f"  (b) - (a) = {med['b'] - med['a']:+.1f} us against the spread of (a) {spread['a']:.1f} us -> {'holds' if ok else 'DOES NOT HOLD'}; "
                 f"(b) / (a) = {med['b'] / med['a']:.3f}; (c) / (b) = {med['c'] / med['b']:.2f} (context only)")
    lines.append("the update launch alone (device time, HIP events around 100 back-to-back calls, five interleaved repetitions):")
    update_alone(lines, opt_a, opt_b, numel)
    lines.append(CLOCK_NOTE)
    lines.append("command: timeout -k 10 300 python3 tools/bench_optim_groups.py")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
