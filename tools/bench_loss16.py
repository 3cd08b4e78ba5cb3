#!/usr/bin/env python3
"""Times the class-parallel losses on bf16 logits (qatvit_kd_ce_loss_rows16, qatvit_kd_ce_loss_topk16, qatvit_kd_bce_loss_topk16) on one MI355X against
the route a bf16 step had before them, and writes profiles/loss16_bench.txt.

Per (B, C, k) of (1024, 1000, 32), (256, 21841, 16), (64, 32768, 32), with a teacher table of 4 * B rows (dense for the rows entry, compressed to k for the
other two), plain and with mix records, in one process, the arms interleaved:
  new    the 16-bit entry alone on preallocated buffers: bf16 logits in, bf16 dlogits out (two launches);
  old    student.float(), the fp32 entry of the same name on preallocated buffers, dlogits.to(torch.bfloat16): the same result type from the same
         input, five launches.
Every figure: the median of five repetitions of N calls between two HIP events after a warm-up of every arm (bench_bce_loss.py's time_arms and
inputs); N is chosen per line so that a window of the faster arm lasts about --window seconds (a 50-call probe of it after warm-up; 16 us calls need
tens of thousands), or is --calls where given; launch and host glue are included.  Nothing is gated.  Before timing, the two arms' out3 and dlogits
are compared (printed).

usage: python3 tools/bench_loss16.py [--window SECONDS] [--calls N] [--out FILE]"""
import argparse
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
warnings.filterwarnings("ignore")
from bench_bce_loss import CLOCK_NOTE, inputs, time_arms  # noqa: E402

SHAPES = [(1024, 1000, 32), (256, 21841, 16), (64, 32768, 32)]
T, ALPHA, EPS = 4.0, 0.5, 0.1


def arms(s16, y, mix, table, index, k):
    """entry -> form -> {"new": fn, "old": fn}, and the buffers the two arms write."""
    import qat_vit_amd
    from qat_vit_amd import native

    B, C = s16.shape
    L = native.lib()
    tab = qat_vit_amd.TeacherTopKTable.from_dense(table, k, T)
    ptr = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    out = {a: (torch.empty(3, device="cuda"), torch.empty(2 * B, device="cuda")) for a in ("new", "old")}
    d16, d32 = torch.empty_like(s16), torch.empty(B, C, device="cuda")
    st = native.stream_ptr()
    topk = (ptr(tab.idx), ptr(tab.val), ptr(tab.tail), tab.N, k, ptr(index), ptr(y))
    dense = (None, ptr(table), table.shape[0], ptr(index), ptr(y))
    hyper = (B, C, T, ALPHA, EPS)

    def call(entry, m, new):
        o3, partials = out["new" if new else "old"]
        s = s16 if new else s16.float()
        head = (ptr(s), 2) if new else (ptr(s),)
        tail = ((None,) if new else ()) + (ptr(partials), ptr(o3), ptr(d16 if new else d32), st)
        name = entry + ("16" if new else "")
        if entry == "qatvit_kd_ce_loss_rows":
            args = head + dense + (ptr(m),) + hyper + tail
        elif entry == "qatvit_kd_ce_loss_topk":
            args = head + topk + (ptr(m),) + hyper + tail
        else:
            args = head + topk + (ptr(m),) + hyper + (-1.0, 0) + tail
        native.check(getattr(L, name)(*args), name)
        return d16 if new else d32.to(torch.bfloat16)

    fns = {}
    for entry in ("qatvit_kd_ce_loss_rows", "qatvit_kd_ce_loss_topk", "qatvit_kd_bce_loss_topk"):
        for form, m in (("plain", None), ("mix", mix)):
            fns[(entry, form)] = {"new": lambda e=entry, m=m: call(e, m, True), "old": lambda e=entry, m=m: call(e, m, False)}
    return fns, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss16_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss16.py needs an MI355X: there is no CPU form of these kernels to run")
    lines = [f"class-parallel losses on bf16 logits on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per call (loss and bf16 dlogits), median of five repetitions of N calls (N per line: windows of about {args.window} s of the new arm"
             f"{'' if not args.calls else ', here --calls ' + str(args.calls)}), launch and host glue included; T {T}, alpha {ALPHA}, eps {EPS}; table of 4 * B rows:",
             "  new = the ...16 entry on bf16 logits (two launches); old = student.float() + the fp32 entry + dlogits.to(bfloat16) (five launches)"]
    for B, C, k in SHAPES:
        s, y, mix, table, index = inputs(B, C, B + C + k)
        fns, out = arms(s.to(torch.bfloat16), y, mix, table, index, k)
        for (entry, form), pair in fns.items():
            dn, do = pair["new"]().float(), pair["old"]().float()
            e3 = float(((out["new"][0] - out["old"][0]).abs() / out["old"][0].abs().clamp_min(1e-30)).max())
            eg = float(((dn - do).abs().amax(1) / do.abs().amax(1)).max())
            calls = args.calls
            if not calls:
                for _ in range(20):
                    pair["new"]()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                for _ in range(50):
                    pair["new"]()
                ev[1].record()
                torch.cuda.synchronize()
                calls = max(200, int(args.window * 1e3 / (ev[0].elapsed_time(ev[1]) / 50)))
            r = time_arms(pair, calls)
            new, old = r["new"][0], r["old"][0]
            lines.append(f"  B={B:5d} C={C:5d} k={k:2d} {entry + '16':27s} {form:5s}  N {calls:6d}  new {new:8.1f}  old {old:8.1f}  old / new {old / new:5.2f}x"
                         f"{'  (the new entry is NOT faster here)' if new >= old else ''}  |  new against old: out3 {e3:.1e}, dlogits per row {eg:.1e}")
            lines.append("      repetitions: " + "; ".join(f"{n} {', '.join(f'{v:.1f}' for v in r[n][1])}" for n in r))
    lines.append(CLOCK_NOTE)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
