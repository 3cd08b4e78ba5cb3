#!/usr/bin/env python3
"""Measures the optimizer step with a weight EMA (ClipAdamW(ema_decay=...)) on one MI355X and writes profiles/optim_ema_bench.txt.

The parameters of the ViT-S/16 student (152 tensors, one param group) with synthetic gradients in fixed buffers; `step(max_norm=1.0)` in four arms,
each on its own copy of the parameters:
  (a) ClipAdamW without an average                        - qatvit_optim_grad_norm + qatvit_optim_adamw, the path that existed;
  (b) ClipAdamW(ema_decay=0.9998)                         - qatvit_optim_grad_norm + qatvit_optim_adamw_ema: the average inside the update launch;
  (c) (a), then torch._foreach_lerp_(emas, params, 1 - d) - the external form (a `ModelEma` beside the optimizer);
  (d) opt.swap_ema() twice                                - swapping the averages in and back out (qatvit_optim_swap), no step.
One warm-up window of each arm, then `--repeats` timed windows per arm, interleaved a, b, c, d, a, ... in this process; a window is `--steps` steps
under a host clock from a device synchronisation to a device synchronisation, reported as microseconds per step (per swap pair for (d)).  Also: the
update launch alone (qatvit_optim_adamw against qatvit_optim_adamw_ema on the tables of (a) and (b)), HIP events around 100 back-to-back calls, five
interleaved repetitions, with the HBM rate that follows from 28 and 36 bytes per parameter.

Two conditions, both against this same run:
  1. median (c) - median (b) > the larger of the spreads (max - min) of (b)'s and (c)'s windows;
  2. the rate of (b)'s launch (36 B per parameter) >= the rate of (a)'s (28 B) minus the larger of the two spreads of the event repetitions.
The exit status says whether both held; the figures are reported whatever they are.

Run it as one step under its own time limit, and chain steps with &&, so that a failing step starts nothing after it:
  timeout -k 10 300 python3 tools/bench_optim_ema.py && echo done

usage: python3 tools/bench_optim_ema.py [--steps N] [--repeats R] [--out FILE]"""
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
DECAY = 0.9998
CLOCK_NOTE = ("clocks: as the machine had them (not pinned, not changed, not read); every figure follows its own warm-up, and the interleaved "
              "windows show the drift inside this run")


def fmt(v, digits=1):
    return ", ".join(f"{t:.{digits}f}" for t in v)


def update_alone(lines, plain, with_ema, numel):
    """Device time of the update launch of each entry, on the tables the two optimizers built; returns whether condition 2 held."""
    from qat_vit_amd import native
    from qat_vit_amd.optim import _CHUNK

    L, st = native.lib(), native.stream_ptr()
    ta, tb = plain._live_tables(), with_ema._live_tables()
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.05, 10)
    calls = (("qatvit_optim_adamw", 28, lambda: L.qatvit_optim_adamw(ta["params"].data_ptr(), ta["grads"].data_ptr(), ta["m"].data_ptr(), ta["v"].data_ptr(),
                                                                      ta["numel"].data_ptr(), ta["ct"].data_ptr(), ta["ci"].data_ptr(), ta["n"], _CHUNK, *hyper,
                                                                      ta["out2"].data_ptr(), st)),
             ("qatvit_optim_adamw_ema", 36, lambda: L.qatvit_optim_adamw_ema(tb["params"].data_ptr(), tb["grads"].data_ptr(), tb["m"].data_ptr(), tb["v"].data_ptr(),
                                                                              tb["ema"].data_ptr(), tb["numel"].data_ptr(), tb["ct"].data_ptr(), tb["ci"].data_ptr(),
                                                                              tb["n"], _CHUNK, *hyper, DECAY, tb["out2"].data_ptr(), st)))
    reps = {name: [] for name, _, _ in calls}
    for name, _, fn in calls:
        for _ in range(20):
            native.check(fn(), name)
    for _ in range(5):
        for name, _, fn in calls:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(100):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            reps[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / 100)
    rate, spread = {}, {}
    for name, nbytes, _ in calls:
        rates = [nbytes * numel / us / 1e6 for us in reps[name]]          # TB/s
        rate[name], spread[name] = statistics.median(rates), max(rates) - min(rates)
        lines.append(f"  {name:24s} {statistics.median(reps[name]):7.1f} us per launch ({fmt(reps[name])}); {nbytes} B x {numel:,} parameters = "
                     f"{rate[name]:.2f} TB/s ({fmt(rates, 2)}; spread {spread[name]:.2f})")
    a, b = "qatvit_optim_adamw", "qatvit_optim_adamw_ema"
    ok = rate[b] >= rate[a] - max(spread[a], spread[b])
    lines.append(f"  condition 2: {rate[b]:.2f} TB/s with the average against {rate[a]:.2f} TB/s without, larger spread {max(spread[a], spread[b]):.2f} "
                 f"-> {'holds' if ok else 'DOES NOT HOLD'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_ema_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_ema.py needs an MI355X: there is no CPU form of the optimizer kernels to time")
    import qat_vit_amd
    from qat_vit_amd import ClipAdamW

    torch.manual_seed(0)
    first = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda()
    models = {arm: first if arm == "a" else copy.deepcopy(first) for arm in "abcd"}
    g = torch.Generator(device="cuda").manual_seed(1)
    for m in models.values():
        for p in m.parameters():
            p.grad = torch.randn(p.shape, device="cuda", generator=g) * 0.01
    numel = sum(p.numel() for p in first.parameters())
    hyper = dict(lr=1e-3, weight_decay=0.05)
    opt = {"a": ClipAdamW(models["a"].parameters(), **hyper), "b": ClipAdamW(models["b"].parameters(), ema_decay=DECAY, **hyper),
           "c": ClipAdamW(models["c"].parameters(), **hyper), "d": ClipAdamW(models["d"].parameters(), ema_decay=DECAY, **hyper)}
    params_c = list(models["c"].parameters())
    emas_c = [p.detach().clone() for p in params_c]
    opt["d"].step(max_norm=1.0)                                # creates the averages that (d) swaps

    def external():
        opt["c"].step(max_norm=1.0)
        torch._foreach_lerp_(emas_c, params_c, 1.0 - DECAY)

    def swap_pair():
        opt["d"].swap_ema()
        opt["d"].swap_ema()

    arms = {"a": lambda: opt["a"].step(max_norm=1.0), "b": lambda: opt["b"].step(max_norm=1.0), "c": external, "d": swap_pair}

    def window(arm):
        fn = arms[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.steps

    lines = [f"optimizer step with a weight EMA on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"ViT-S/16 student: {len(params_c)} tensors, {numel:,} parameters, one param group; ema_decay {DECAY}"]
    for arm in "abcd":
        window(arm)                                            # the warm-up window of each arm
    w = {arm: [] for arm in "abcd"}
    for _ in range(args.repeats):
        for arm in "abcd":
            w[arm].append(window(arm))
    med = {arm: statistics.median(w[arm]) for arm in "abcd"}
    spread = {arm: max(w[arm]) - min(w[arm]) for arm in "abcd"}
    ok1 = med["c"] - med["b"] > max(spread["b"], spread["c"])
    lines.append(f"step(max_norm=1.0): {args.repeats} interleaved windows of {args.steps} steps per arm after one warm-up window each, us per step (host clock, "
                 "synchronised at both ends):")
    names = {"a": "(a) ClipAdamW without an average (qatvit_optim_adamw):     ", "b": "(b) ClipAdamW(ema_decay) (qatvit_optim_adamw_ema):         ",
             "c": "(c) (a) + torch._foreach_lerp_ over 152 tensors:           ", "d": "(d) swap_ema() twice (2 x qatvit_optim_swap), per pair:    "}
    for arm in "abcd":
        lines.append(f"  {names[arm]} median {med[arm]:.1f}  (min {min(w[arm]):.1f}, max {max(w[arm]):.1f}: {fmt(w[arm])}); spread {spread[arm]:.1f}")
    lines.append(f"  condition 1: (c) - (b) = {med['c'] - med['b']:+.1f} us against the larger spread of (b), (c) {max(spread['b'], spread['c']):.1f} us -> "
                 f"{'holds' if ok1 else 'DOES NOT HOLD'}; (b) - (a) = {med['b'] - med['a']:+.1f} us; (b) / (a) = {med['b'] / med['a']:.3f}")
    lines.append(f"  (d): one swap moves 16 B x {numel:,} parameters; {med['d'] / 2:.1f} us per swap_ema() including its host part")
    lines.append("the update launch alone (device time, HIP events around 100 back-to-back calls, five interleaved repetitions):")
    ok2 = update_alone(lines, opt["a"], opt["b"], numel)
    lines.append(CLOCK_NOTE)
    lines.append("command: timeout -k 10 300 python3 tools/bench_optim_ema.py")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    raise SystemExit(0 if ok1 and ok2 else 1)


if __name__ == "__main__":
    main()
