#!/usr/bin/env python3
"""Measures the LAMB optimizer step (ClipLamb) on one MI355X and writes profiles/optim_lamb_bench.txt.

The parameters of the ViT-S/16 QAT student (152 tensors) with synthetic gradients in fixed buffers; `step(max_norm=1.0)` in five arms, each on its own
copy of the parameters:
  (a) ClipLamb, one param group                            - qatvit_optim_grad_norm + qatvit_optim_lamb_moments + qatvit_optim_lamb_apply;
  (b) ClipLamb over vit_param_groups(layer_decay=0.75)     - the same three launches for all 28 groups;
  (c) ClipLamb(ema_decay=0.9998), one group                - the average written by the apply launch;
  (d) ClipAdamW, one group                                 - qatvit_optim_grad_norm + qatvit_optim_adamw: the code that existed, the yardstick;
  (e) the same LAMB step composed from torch._foreach ops  - what a run with LAMB fell back to.
Per arm: one warm-up window, then `--repeats` windows interleaved a, b, c, d, e, a, ...; a window is `--steps` steps between two HIP events on the
stream, reported as microseconds per step (the host keeps up or it does not: either way this is the time a training loop sees).  Also the update
launches alone - qatvit_optim_adamw, qatvit_optim_lamb_moments, qatvit_optim_lamb_apply on the tables of (d) and (a) - HIP events around 100
back-to-back calls, five interleaved repetitions, with the HBM rate that follows from 28, 24 and 16 bytes per parameter, and the ratio
(moments + apply) / adamw next to the 40 / 28 = 1.43 the byte counts give.  No time is fixed in advance: the figures are reported as measured.

Last, the tolerance pair of tests/test_gpu_optim_lamb.py: the rel L2 error of the kernels and of stock fp32 torch ops against the fp64 reference,
for the parameters and the trust ratios, as that test measures them (its own function is called).

Run it as one step under its own time limit, and chain steps with &&, so that a failing step starts nothing after it:
  timeout -k 10 300 python3 tools/bench_optim_lamb.py && echo done

usage: python3 tools/bench_optim_lamb.py [--steps N] [--repeats R] [--out FILE]"""
import argparse
import copy
import math
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
DECAY = 0.9998
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.05)
CLOCK_NOTE = ("clocks: as the machine had them (not pinned, not changed, not read); every figure follows its own warm-up, and the interleaved "
              "windows show the drift inside this run")


def fmt(v, digits=1):
    return ", ".join(f"{t:.{digits}f}" for t in v)


class ForeachLamb:
    """The arithmetic of include/qatvit.h for one param group with weight decay, composed from stock multi-tensor ops (no host read-back either)."""

    def __init__(self, params):
        self.params = [p.detach() for p in params]
        self.grads = [p.grad for p in params]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.t = 0

    @torch.no_grad()
    def step(self, max_norm):
        lr, (b1, b2), eps, wd = HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"]
        self.t += 1
        total = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(self.grads)))
        coef = (max_norm / (total + 1e-6)).clamp(max=1.0)
        g = torch._foreach_mul(self.grads, coef)
        torch._foreach_mul_(self.m, b1)
        torch._foreach_add_(self.m, g, alpha=1 - b1)
        torch._foreach_mul_(self.v, b2)
        torch._foreach_addcmul_(self.v, g, g, value=1 - b2)
        denom = torch._foreach_sqrt(self.v)
        torch._foreach_div_(denom, math.sqrt(1 - b2 ** self.t))
        torch._foreach_add_(denom, eps)
        r = torch._foreach_div(self.m, 1 - b1 ** self.t)
        torch._foreach_div_(r, denom)
        torch._foreach_add_(r, self.params, alpha=wd)
        pn, rn = torch.stack(torch._foreach_norm(self.params)), torch.stack(torch._foreach_norm(r))
        scale = torch.where((pn > 0) & (rn > 0), pn / rn, torch.ones_like(pn)) * -lr
        torch._foreach_mul_(r, list(scale.unbind(0)))
        torch._foreach_add_(self.params, r)


def launches_alone(lines, adamw, lamb, numel):
    """Device time of each update launch on the tables the two optimizers built; returns the three medians (us)."""
    import struct

    from qat_vit_amd import native
    from qat_vit_amd.optim import _CHUNK

    L, st = native.lib(), native.stream_ptr()
    ta, tl = adamw._live_tables(), lamb._live_tables()
    rows = struct.pack("=5dq4i", HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], 10, 1, 0, 0, 0)
    calls = (("qatvit_optim_adamw", 28, lambda: L.qatvit_optim_adamw(ta["params"].data_ptr(), ta["grads"].data_ptr(), ta["m"].data_ptr(), ta["v"].data_ptr(),
                                                                      ta["numel"].data_ptr(), ta["ct"].data_ptr(), ta["ci"].data_ptr(), ta["n"], _CHUNK, 1e-3, 0.9, 0.999,
                                                                      1e-8, 0.05, 10, ta["out2"].data_ptr(), st)),
             ("qatvit_optim_lamb_moments", 24, lambda: L.qatvit_optim_lamb_moments(tl["params"].data_ptr(), tl["grads"].data_ptr(), tl["m"].data_ptr(), tl["v"].data_ptr(),
                                                                                    tl["numel"].data_ptr(), tl["tg"].data_ptr(), tl["ct"].data_ptr(), tl["ci"].data_ptr(),
                                                                                    tl["n"], _CHUNK, rows, 1, tl["out2"].data_ptr(), tl["partials2"].data_ptr(), st)),
             ("qatvit_optim_lamb_apply", 16, lambda: L.qatvit_optim_lamb_apply(tl["params"].data_ptr(), tl["m"].data_ptr(), tl["v"].data_ptr(), None, tl["numel"].data_ptr(),
                                                                                tl["tg"].data_ptr(), tl["first_chunk"].data_ptr(), tl["ct"].data_ptr(), tl["ci"].data_ptr(),
                                                                                tl["n"], _CHUNK, rows, 1, 0.0, tl["partials2"].data_ptr(), tl["trust"].data_ptr(), st)))
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
    med = {}
    for name, nbytes, _ in calls:
        med[name] = statistics.median(reps[name])
        rates = [nbytes * numel / us / 1e6 for us in reps[name]]          # TB/s
        lines.append(f"  {name:27s} {med[name]:7.1f} us per launch ({fmt(reps[name])}); {nbytes} B x {numel:,} parameters = "
                     f"{statistics.median(rates):.2f} TB/s ({fmt(rates, 2)})")
    return med["qatvit_optim_adamw"], med["qatvit_optim_lamb_moments"], med["qatvit_optim_lamb_apply"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_lamb_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_lamb.py needs an MI355X: there is no CPU form of the optimizer kernels to time")
    import qat_vit_amd
    from qat_vit_amd import ClipAdamW, ClipLamb, vit_param_groups

    torch.manual_seed(0)
    first = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True).cuda()
    models = {arm: first if arm == "a" else copy.deepcopy(first) for arm in "abcde"}
    g = torch.Generator(device="cuda").manual_seed(1)
    for m in models.values():
        for p in m.parameters():
            p.grad = torch.randn(p.shape, device="cuda", generator=g) * 0.01
    n_tensors = len(list(first.parameters()))
    numel = sum(p.numel() for p in first.parameters())
    groups_b = vit_param_groups(models["b"], HYPER["weight_decay"], lr=HYPER["lr"], layer_decay=0.75)
    opt = {"a": ClipLamb(models["a"].parameters(), **HYPER), "b": ClipLamb(groups_b, betas=HYPER["betas"], eps=HYPER["eps"]),
           "c": ClipLamb(models["c"].parameters(), ema_decay=DECAY, **HYPER),
           "d": ClipAdamW(models["d"].parameters(), lr=1e-3, weight_decay=0.05)}
    fe = ForeachLamb(list(models["e"].parameters()))
    arms = {arm: (lambda o=opt[arm]: o.step(max_norm=1.0)) for arm in "abcd"}
    arms["e"] = lambda: fe.step(1.0)

    def window(arm):
        fn = arms[arm]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(args.steps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / args.steps

    lines = [f"LAMB optimizer step on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"ViT-S/16 QAT student: {n_tensors} tensors, {numel:,} parameters; {len(groups_b)} param groups in (b); ema_decay {DECAY} in (c)"]
    for arm in "abcde":
        window(arm)                                            # the warm-up window of each arm
    w = {arm: [] for arm in "abcde"}
    for _ in range(args.repeats):
        for arm in "abcde":
            w[arm].append(window(arm))
    med = {arm: statistics.median(w[arm]) for arm in "abcde"}
    lines.append(f"step(max_norm=1.0): {args.repeats} interleaved windows of {args.steps} steps per arm after one warm-up window each, us per step (HIP events "
                 "around the window):")
    names = {"a": "(a) ClipLamb, one group:                               ", "b": f"(b) ClipLamb, vit_param_groups layer decay ({len(groups_b)} groups): ",
             "c": "(c) ClipLamb(ema_decay), one group:                    ", "d": "(d) ClipAdamW, one group (the yardstick):              ",
             "e": "(e) LAMB from torch._foreach ops:                      "}
    for arm in "abcde":
        lines.append(f"  {names[arm]} median {med[arm]:.1f}  (min {min(w[arm]):.1f}, max {max(w[arm]):.1f}: {fmt(w[arm])})")
    lines.append(f"  (a) / (d) = {med['a'] / med['d']:.3f}; (b) - (a) = {med['b'] - med['a']:+.1f} us; (c) - (a) = {med['c'] - med['a']:+.1f} us; "
                 f"(e) / (a) = {med['e'] / med['a']:.2f}")
    lines.append("the update launches alone (device time, HIP events around 100 back-to-back calls, five interleaved repetitions):")
    t_adamw, t_mom, t_app = launches_alone(lines, opt["d"], opt["a"], numel)
    lines.append(f"  bytes by construction: moments 16 B read + 8 B written, apply 12 B + 4 B: 40 B per parameter against AdamW's 28 B, ratio 1.43; "
                 f"measured (moments + apply) / adamw = ({t_mom:.1f} + {t_app:.1f}) / {t_adamw:.1f} = {(t_mom + t_app) / t_adamw:.2f}")
    lines.append(CLOCK_NOTE)
    lines.append("command: timeout -k 10 300 python3 tools/bench_optim_lamb.py")
    # the tolerance pair of the GPU test, measured by the test's own function
    from tests.test_gpu_optim_lamb import FLOOR, compare_with_reference

    lines.append(f"tolerance pair of tests/test_gpu_optim_lamb.py (largest rel L2 error against the fp64 reference over 5 steps and 11 tensors; the kernels are "
                 f"allowed max(2 x stock, {FLOOR:g})):")
    for max_norm in (None, 1.0):
        worst = compare_with_reference(5, max_norm, f"bench, max_norm={max_norm}")[4]
        lines.append(f"  max_norm={max_norm}: parameters kernels {worst['p'][0]:.3e} / stock fp32 torch ops {worst['p'][1]:.3e}; trust ratios kernels "
                     f"{worst['trust'][0]:.3e} / stock {worst['trust'][1]:.3e}; exp_avg {worst['m']:.3e}, exp_avg_sq {worst['v']:.3e} (bar {FLOOR:g})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
