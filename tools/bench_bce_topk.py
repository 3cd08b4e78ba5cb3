#!/usr/bin/env python3
"""Times qatvit_kd_bce_loss_topk (BCE + KD from the compressed teacher table, sparse form) on one MI355X and writes profiles/bce_topk_bench.txt; with
--errors it measures instead what the EXISTING entries miss the fp64 reference by and writes profiles/bce_topk_errors.txt.

Timing.  Per (B, C, k) of (1024, 1000, 32), (256, 21841, 16), (256, 21841, 64), (64, 32768, 32), with a table of 4 * B rows, plain and with mix records, in
one process, the arms interleaved:
  new    qatvit_kd_bce_loss_topk alone on preallocated buffers (two launches);
  dense  (C = 1000 only; the entry stops at 4096 classes) qatvit_kd_bce_loss alone with the DECOMPRESSED table of the same rows;
  torch  the same objective from stock torch ops in fp32 on the decompressed table (tools/bench_bce_loss.py's composition) with autograd for dlogits.
Every figure: the median of five repetitions of --calls calls between two HIP events after a warm-up of every arm (bench_bce_loss.py's time_arms and
inputs); launch and host glue are included.  Nothing is gated.  Before timing, each shape's new result is compared with the torch arm's (printed).

--errors.  On the cases of tests/test_gpu_bce_topk.py, against that file's fp64 reference, the two quantities its bars are made of - the largest
relative error of out3 and the largest per-row max |dlogits - ref| / max |ref| - for
  C <= 4096: F.kd_bce_loss with the dense decompressed table (or without a teacher), every configuration of the test;
  C >  4096: where no BCE entry existed, F.kd_ce_loss_topk's KD number and gradient with the hard part removed from both sides (kd_alpha = 1).
The entry under test is printed next to them and takes no part in the recorded worst.

usage: python3 tools/bench_bce_topk.py [--calls N] [--errors] [--out FILE]"""
import argparse
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
warnings.filterwarnings("ignore")
from bench_bce_loss import CLOCK_NOTE, composition, inputs, time_arms  # noqa: E402

SHAPES = [(1024, 1000, 32), (256, 21841, 16), (256, 21841, 64), (64, 32768, 32)]
T, ALPHA, EPS = 4.0, 0.5, 0.1


def arms(s, y, mix, table, index, k):
    import qat_vit_amd
    from qat_vit_amd import native

    B, C = s.shape
    L = native.lib()
    tab = qat_vit_amd.TeacherTopKTable.from_dense(table, k, T)
    dense = tab.rows(torch.arange(tab.N, device="cuda"))
    bufs = {n: (torch.empty(3, device="cuda"), torch.empty(2 * B, device="cuda"), torch.empty_like(s)) for n in ("new", "dense")}
    ptr = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    sg = s.clone().requires_grad_(True)

    def new(m):
        out3, partials, dl = bufs["new"]
        native.check(L.qatvit_kd_bce_loss_topk(ptr(s), ptr(tab.idx), ptr(tab.val), ptr(tab.tail), tab.N, k, ptr(index), ptr(y), ptr(m), B, C, T, ALPHA, EPS,
                                               -1.0, 0, ptr(partials), ptr(out3), ptr(dl), native.stream_ptr()), "qatvit_kd_bce_loss_topk")

    def dense_bce(m):
        out3, partials, dl = bufs["dense"]
        native.check(L.qatvit_kd_bce_loss(ptr(s), None, ptr(dense), tab.N, ptr(index), ptr(y), ptr(m), B, C, T, ALPHA, EPS, -1.0, 0, ptr(partials),
                                          ptr(out3), ptr(dl), native.stream_ptr()), "qatvit_kd_bce_loss")

    def torch_arm(m):
        out = composition(sg, y, m, dense, index)
        return torch.stack(out).detach(), torch.autograd.grad(out[0], sg)[0]

    agree = []
    for m in (None, mix):
        new(m)
        want3, wantg = torch_arm(m)
        out3, _, dl = bufs["new"]
        agree.append((float(((out3 - want3).abs() / want3.abs()).max()), float(((dl - wantg).abs().amax(1) / wantg.abs().amax(1)).max())))
    fns = {"new plain": lambda: new(None), "torch plain": lambda: torch_arm(None), "new mix": lambda: new(mix), "torch mix": lambda: torch_arm(mix)}
    if C <= 4096:
        fns.update({"dense plain": lambda: dense_bce(None), "dense mix": lambda: dense_bce(mix)})
    return fns, agree


def bench(args):
    lines = [f"BCE + KD from the compressed teacher table on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per call (loss and dlogits), median of five repetitions of {args.calls} calls, launch and host glue included; T {T}, alpha {ALPHA}, eps {EPS}; "
             "table of 4 * B rows:",
             "  new = qatvit_kd_bce_loss_topk, dense = qatvit_kd_bce_loss on the decompressed table (C <= 4096 only), both alone on preallocated buffers, two "
             "launches; torch = the objective from stock fp32 torch ops on the decompressed table + autograd"]
    for B, C, k in SHAPES:
        s, y, mix, table, index = inputs(B, C, B + C + k)
        fns, agree = arms(s, y, mix, table, index, k)
        r = time_arms(fns, args.calls)
        med = {n: v[0] for n, v in r.items()}
        for form, (e3, eg) in zip(("plain", "mix"), agree):
            d = f"dense {med[f'dense {form}']:8.1f}  dense / new {med[f'dense {form}'] / med[f'new {form}']:5.2f}x  " if C <= 4096 else ""
            lines.append(f"  B={B:5d} C={C:5d} k={k:2d} {form:5s}  new {med[f'new {form}']:8.1f}  {d}torch {med[f'torch {form}']:8.1f}  torch / new "
                         f"{med[f'torch {form}'] / med[f'new {form}']:6.2f}x  |  new against torch fp32: out3 {e3:.1e}, dlogits per row {eg:.1e}")
        lines.append("      repetitions: " + "; ".join(f"{n} {', '.join(f'{v:.1f}' for v in r[n][1])}" for n in r))
        slower = [n for n in ("plain", "mix") if C <= 4096 and med[f"new {n}"] >= med[f"dense {n}"]]
        if slower:
            lines.append(f"      the new entry is NOT faster than the dense one here: {', '.join(slower)}")
    lines.append(CLOCK_NOTE)
    return lines


def errors():
    import qat_vit_amd.functional as F
    from tests import mix_ref
    from tests import test_gpu_bce_topk as t

    lines = ["what the entries that existed before qatvit_kd_bce_loss_topk miss the fp64 reference of tests/test_gpu_bce_topk.py by, on that file's cases",
             "out3: the largest |v - ref| / |ref| of the numbers compared; dlogits: the largest over the rows of max |dlogits - ref| / max |ref|",
             "(new = the entry under test on the same case, for comparison; it takes no part in the recorded worst)"]
    worst = {False: [0.0, 0.0], True: [0.0, 0.0]}
    for B, C, k in t.SHAPES:
        c = t.case(B, C, k)
        s, tab, dense, index, y, recs = c
        for table, mix, thr, sc in t.CONFIGS:
            new = t.errors(*t.run(c, table, mix, thr, sc), t.want(c, table, mix, thr, sc))
            m = recs.cuda() if mix else None
            sg = s.clone().cuda().requires_grad_(True)
            if C <= 4096:
                what = "F.kd_bce_loss, dense decompressed table" if table else "F.kd_bce_loss, no teacher"
                kw = {"table": dense.cuda(), "index": index.cuda()} if table else {}
                loss, parts = F.kd_bce_loss(sg, y.cuda(), mix=m, kd_temp=T, kd_alpha=ALPHA, label_smoothing=EPS, target_threshold=thr, sum_classes=sc, **kw)
                loss.backward()
                old = t.errors(parts.detach().cpu(), sg.grad.cpu(), t.want(c, table, mix, thr, sc))
            elif table:
                what = "F.kd_ce_loss_topk, KD number and gradient (kd_alpha = 1)"
                loss, parts = F.kd_ce_loss_topk(sg, *(v.cuda() for v in tab), index.cuda(), y.cuda(), m, T, 1.0, EPS)
                loss.backward()
                s64 = s.double().requires_grad_(True)
                ref = mix_ref.loss(s64, y, recs if mix else None, table=dense, index=index, kd_temp=T, kd_alpha=1.0, label_smoothing=EPS)
                ref[2].backward()
                old = t.errors(parts[2:].detach().cpu(), sg.grad.cpu(), ([float(ref[2])], s64.grad))
            else:
                continue                                             # no teacher above 4096 classes: nothing existed to measure
            worst[C > 4096] = [max(a, b) for a, b in zip(worst[C > 4096], old)]
            lines.append(f"  B={B} C={C:5d} k={k:2d} table={table!s:5} mix={mix!s:5} thr={thr!s:4} sum_classes={sc!s:5}  {what}: out3 {old[0]:.3e} dlogits {old[1]:.3e}"
                         f"   |   new: out3 {new[0]:.3e} dlogits {new[1]:.3e}")
    for big, name in ((False, "C <= 4096"), (True, "C >  4096")):
        lines.append(f"worst, {name}: out3 {worst[big][0]:.3e} dlogits {worst[big][1]:.3e}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bce_topk.py needs an MI355X: there is no CPU form of these kernels to run")
    import qat_vit_amd  # noqa: F401

    out = args.out or os.path.join(ROOT, "profiles", "bce_topk_errors.txt" if args.errors else "bce_topk_bench.txt")
    text = "\n".join(errors() if args.errors else bench(args)) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
