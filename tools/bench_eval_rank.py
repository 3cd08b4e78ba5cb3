#!/usr/bin/env python3
"""Times validation at many classes (qatvit_eval_accumulate_rank, EvalAccumulator(topk=...)) on one MI355X and writes profiles/eval_rank_bench.txt.

Shapes (B, C) = (256, 10), (1024, 1000), (256, 21841), (64, 32768), fp32 logits.  Per shape, in one process, the arms interleaved:
  entry    qatvit_eval_accumulate_rank alone on a preallocated state block (label_smoothing 0.1, no per-class counts): one launch;
  update   EvalAccumulator(C, confusion=False, topk=(1, 5), label_smoothing=0.1).update: the same launch behind the wrapper's checks;
  parent   EvalAccumulator(C, confusion=False).update: the older entry (qatvit_eval_accumulate), which gives top-1 and the unsmoothed loss only;
  torch    the same figures from stock torch ops, accumulated on the device: topk(5), cross_entropy(label_smoothing=0.1, reduction="sum"), bincount.
Every figure: the median of five repetitions of --calls calls between two HIP events after a warm-up of every arm (tools/bench_bce_loss.py's
time_arms); launch and host glue are included, as a validation loop pays them.  Spread = largest minus smallest of the five repetitions.
Algorithmic bytes: one read of the logits, B * C * 4; the entry's share of 8 TB/s is bytes / time / 8e12.

The one condition: at (1024, 1000), update takes no longer than torch by more than either arm's own spread.  The exit status says whether it held.

Also recorded: the largest relative error of the entry's loss sum against F.cross_entropy in fp64, over the class counts, formats and smoothings of
tests/test_gpu_eval_rank.py (its bound is 1e-5).

usage: python3 tools/bench_eval_rank.py [--calls N] [--out FILE]"""
import argparse
import os
import sys
import warnings

import torch
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
warnings.filterwarnings("ignore")
from bench_bce_loss import CLOCK_NOTE, time_arms  # noqa: E402

SHAPES = [(256, 10), (1024, 1000), (256, 21841), (64, 32768)]
GATED = (1024, 1000)
EPS, TOPK = 0.1, (1, 5)
HBM_BYTES_PER_S = 8e12
ERROR_CLASSES = [2, 5, 64, 65, 256, 257, 1000, 1024, 1025, 4096, 4097, 8193, 32768]


def inputs(B, C, dtype=torch.float32):
    g = torch.Generator().manual_seed(B + C)
    x, y = 3 * torch.randn(B, C, generator=g), torch.randint(0, C, (B,), generator=g)
    odd = torch.arange(1, B, 2)   # every other label lifted towards the top of its row (low ranks); the plain rows keep the loss sum of order B
    x[odd, y[odd]] += torch.linspace(0, 14, len(odd))
    return x.to(dtype).cuda(), y.cuda()


def arms(x, y):
    """name -> a callable that adds the batch's counts once, without a host synchronisation of its own choosing."""
    import qat_vit_amd
    from qat_vit_amd import native
    from qat_vit_amd.evaluate import RANK_STATE_WORDS

    B, C = x.shape
    L = native.lib()
    state = torch.zeros(RANK_STATE_WORDS, dtype=torch.int64, device="cuda")
    new = qat_vit_amd.EvalAccumulator(C, confusion=False, topk=TOPK, label_smoothing=EPS)
    old = qat_vit_amd.EvalAccumulator(C, confusion=False)
    hits, loss, counts = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((), dtype=torch.float64, device="cuda"), torch.zeros(C, dtype=torch.int64, device="cuda")

    def entry():
        native.check(L.qatvit_eval_accumulate_rank(x.data_ptr(), 0, C, y.data_ptr(), B, C, EPS, None, 0, None, 0, state.data_ptr(), None, native.stream_ptr()),
                     "qatvit_eval_accumulate_rank")

    def composition():
        hit = x.topk(max(TOPK), 1).indices == y[:, None]
        hits[0] += hit[:, :1].sum()
        hits[1] += hit.sum()
        loss.add_(TF.cross_entropy(x, y, label_smoothing=EPS, reduction="sum"))
        counts.add_(torch.bincount(y, minlength=C))

    return {"entry": entry, "update": lambda: new.update(x, y), "parent": lambda: old.update(x, y), "torch": composition}


def errors(lines):
    import qat_vit_amd

    lines.append("largest relative error of the loss sum against F.cross_entropy in fp64 (B = 33; label_smoothing 0 and 0.1; the tests' bound is 1e-5):")
    worst = 0.0
    for C in ERROR_CLASSES:
        row = []
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            x, y = inputs(33, C, dtype)
            for eps in (0.0, EPS):
                acc = qat_vit_amd.EvalAccumulator(C, confusion=False, topk=(1,), label_smoothing=eps)
                acc.update(x, y)
                want = float(TF.cross_entropy(x.double(), y, label_smoothing=eps, reduction="sum"))
                row.append(abs(acc.result().smoothed_loss_sum - want) / abs(want))
        worst = max(worst, max(row))
        lines.append(f"  C={C:5d}  " + " ".join(f"{e:.1e}" for e in row) + "   (fp32, fp16, bf16; each eps 0, 0.1)")
    lines.append(f"  measured maximum {worst:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rank_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_rank.py needs an MI355X: there is no CPU form of the kernel to time")
    import qat_vit_amd  # noqa: F401

    lines = [f"validation at many classes on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per batch, median of five repetitions of {args.calls} calls (spread = max - min of the five), launch and host glue included; fp32 logits, "
             f"label_smoothing {EPS}, topk {TOPK}:",
             "  entry = qatvit_eval_accumulate_rank alone, update = EvalAccumulator(confusion=False, topk, label_smoothing).update, parent = "
             "EvalAccumulator(confusion=False).update (top-1 and the unsmoothed loss only), torch = topk + cross_entropy(label_smoothing) + bincount"]
    ok = True
    for B, C in SHAPES:
        r = time_arms(arms(*inputs(B, C)), args.calls)
        med = {k: v[0] for k, v in r.items()}
        spread = {k: max(v[1]) - min(v[1]) for k, v in r.items()}
        share = B * C * 4 / (med["entry"] * 1e-6) / HBM_BYTES_PER_S
        line = ("  B={:5d} C={:5d}  ".format(B, C) + "  ".join(f"{k} {med[k]:8.1f} (+-{spread[k]:.1f})" for k in r)
                + f"  |  entry: {B * C * 4 / 1e6:.2f} MB read, {100 * share:.2f} % of 8 TB/s  |  torch / update {med['torch'] / med['update']:.2f}x  "
                  f"parent / update {med['parent'] / med['update']:.2f}x")
        if (B, C) == GATED:
            held = med["torch"] - med["update"] > max(spread["update"], spread["torch"])
            ok = ok and held
            line += "  -> " + ("holds" if held else "DOES NOT HOLD")
        lines.append(line)
        lines.append("      repetitions: " + "; ".join(f"{k} {', '.join(f'{v:.1f}' for v in r[k][1])}" for k in r))
    lines.append(f"condition (update faster than torch at {GATED} by more than either arm's spread): {'holds' if ok else 'DOES NOT HOLD'}")
    errors(lines)
    lines.append(CLOCK_NOTE)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
