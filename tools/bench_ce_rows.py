#!/usr/bin/env python3
"""Times the class-parallel KD + CE loss (qatvit_kd_ce_loss_rows, class_parallel=True) against the serial CE entry on one MI355X and writes
profiles/ce_rows_bench.txt.

Shapes (B, C) = (256, 10), (256, 100), (256, 1000), (1024, 1000), (256, 4096), (256, 21841); forms: plain (labels only), mix (labels + mix records),
mix + table (labels, records and a teacher logit table of 4 * B rows).  Per shape and form, in one process, the arms interleaved:
  rows    qatvit_kd_ce_loss_rows alone on preallocated buffers (two launches), and through F.kd_ce_loss_mix / _table_mix(class_parallel=True);
  serial  qatvit_kd_ce_loss_mix alone (one workgroup, one thread per row), and through its wrapper; refused above 4096 classes, where only rows is timed;
  bce     qatvit_kd_bce_loss alone on the same shape and form (another objective with the same sweeps; up to 4096 classes);
  torch   the same CE objective composed from stock torch ops in fp32, and torch.autograd.grad for dlogits.
Every figure: the median of five repetitions of --calls calls between two HIP events after a warm-up of every arm (tools/bench_bce_loss.py's
time_arms and inputs); launch and host glue are included, as a training step pays them.

The one condition: rows alone < serial alone at every shape with C >= 100 where the serial entry runs, in every form.  The exit status says whether it
held.  C = 10 is reported, not gated.

Also recorded: the fp32 error of the entry and of the torch composition against the composition evaluated in fp64 at C = 1000, 4096, 21841.

usage: python3 tools/bench_ce_rows.py [--calls N] [--out FILE]"""
import argparse
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
warnings.filterwarnings("ignore")
from bench_bce_loss import CLOCK_NOTE, FORMS, inputs, time_arms  # noqa: E402

SHAPES = [(256, 10), (256, 100), (256, 1000), (1024, 1000), (256, 4096), (256, 21841)]
T, ALPHA, EPS = 4.0, 0.5, 0.1
SERIAL_MAX_C = 4096


def composition(student, labels, mix=None, table=None, index=None, teacher=None):
    """(loss, ce, kd * T^2) from stock torch ops in the dtype of `student`; nothing is read on the host.  tests/test_gpu_ce_rows.py takes its bars
    above 257 classes from this function."""
    B, C = student.shape
    dt, dev = student.dtype, student.device
    ar = torch.arange(B, device=dev)
    part, lam = ar, torch.ones(B, dtype=dt, device=dev)
    if mix is not None:
        p = mix[:, 0].long()
        part, lam = torch.where((p >= 0) & (p < B), p, ar), mix[:, 5].contiguous().view(torch.float32)
    oml, lam = (1 - lam).to(dt)[:, None], lam.to(dt)[:, None]
    onehot = torch.full((B, C), EPS / C, dtype=dt, device=dev).scatter_(1, labels.view(-1, 1), 1.0 - EPS + EPS / C)
    ce = -((lam * onehot + oml * onehot.index_select(0, part)) * torch.log_softmax(student, 1)).sum(1).mean()
    if table is None and teacher is None:
        return ce, ce, torch.zeros((), dtype=dt, device=dev)
    if teacher is not None:
        q = torch.softmax(teacher.to(dt) / T, 1)
    else:
        q = torch.softmax(table.to(dt).index_select(0, index) / T, 1)
        q2 = torch.softmax(table.to(dt).index_select(0, index.index_select(0, part)) / T, 1)
        q = torch.where(lam != 1, lam * q + oml * q2, q)
    kd = (torch.xlogy(q, q) - q * torch.log_softmax(student / T, 1)).sum(1).mean() * T * T
    return ALPHA * kd + (1.0 - ALPHA) * ce, ce, kd


def pick(form, mix, table, index):
    return (None if form == "plain" else mix), *((table, index) if form == "mix + table" else (None, None))


def loss_fn(tab):
    import qat_vit_amd.functional as F

    if tab is None:
        return lambda s, idx, y, m, **kw: F.kd_ce_loss_mix(s, None, y, m, T, ALPHA, EPS, **kw)
    return lambda s, idx, y, m, **kw: F.kd_ce_loss_table_mix(s, tab, idx, y, m, T, ALPHA, EPS, **kw)


def arms(form, s, y, mix, table, index):
    """name -> a callable that computes the loss and dlogits once."""
    from qat_vit_amd import native

    B, C = s.shape
    m, tab, idx = pick(form, mix, table, index)
    L = native.lib()
    out3, partials, dl = torch.empty(3, device="cuda"), torch.empty(2 * B, device="cuda"), torch.empty_like(s)
    ptr = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    rows = 0 if tab is None else tab.shape[0]
    sg = s.clone().requires_grad_(True)
    wrapped = loss_fn(tab)

    def rows_alone():
        native.check(L.qatvit_kd_ce_loss_rows(ptr(s), None, ptr(tab), rows, ptr(idx), ptr(y), ptr(m), B, C, T, ALPHA, EPS, ptr(partials), ptr(out3), ptr(dl),
                                              native.stream_ptr()), "qatvit_kd_ce_loss_rows")

    def serial_alone():
        native.check(L.qatvit_kd_ce_loss_mix(ptr(s), None, ptr(tab), rows, ptr(idx), ptr(y), ptr(m), B, C, T, ALPHA, EPS, ptr(out3), ptr(dl),
                                             native.stream_ptr()), "qatvit_kd_ce_loss_mix")

    def bce_alone():
        native.check(L.qatvit_kd_bce_loss(ptr(s), None, ptr(tab), rows, ptr(idx), ptr(y), ptr(m), B, C, T, ALPHA, EPS, -1.0, 0, ptr(partials), ptr(out3),
                                          ptr(dl), native.stream_ptr()), "qatvit_kd_bce_loss")

    fns = {"rows alone": rows_alone, "rows": lambda: wrapped(s, idx, y, m, class_parallel=True),
           "torch": lambda: torch.autograd.grad(composition(sg, y, m, tab, idx)[0], sg)}
    if C <= SERIAL_MAX_C:
        fns.update({"serial alone": serial_alone, "serial": lambda: wrapped(s, idx, y, m), "bce alone": bce_alone})
    return fns


def errors(lines):
    def err(got, grad, want, want_grad):
        rel = [abs(float(a) - float(b)) / max(1.0, abs(float(b))) for a, b in zip(got, want)]
        return rel + [float((grad.double() - want_grad).norm() / want_grad.norm())]

    lines.append("fp32 error against the torch composition evaluated in fp64 (loss, ce, kd: |v - ref| / max(1, |ref|); gradient: relative L2):")
    for B, C in [(9, 1000), (9, 4096), (9, 21841)]:
        s, y, mix, table, index = inputs(B, C, 7 * B + C)
        for form in FORMS:
            m, tab, idx = pick(form, mix, table, index)
            s64 = s.double().requires_grad_(True)
            want = composition(s64, y, m, tab, idx)
            want_grad = torch.autograd.grad(want[0], s64)[0]
            s32 = s.clone().requires_grad_(True)
            got = composition(s32, y, m, tab, idx)
            e_torch = err(got, torch.autograd.grad(got[0], s32)[0], want, want_grad)
            sn = s.clone().requires_grad_(True)
            loss, parts = loss_fn(tab)(sn, idx, y, m, class_parallel=True)
            e_new = err(parts, torch.autograd.grad(loss, sn)[0], want, want_grad)
            f = lambda e: " ".join(f"{v:.1e}" for v in e)   # noqa: E731
            lines.append(f"  B={B:5d} C={C:5d} {form:12s} entry: {f(e_new)}   torch fp32: {f(e_torch)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_rows_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ce_rows.py needs an MI355X: there is no CPU form of the loss to time")
    import qat_vit_amd  # noqa: F401

    lines = [f"class-parallel KD + CE loss on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per call (loss and dlogits), median of five repetitions of {args.calls} calls, launch and host glue included; T {T}, alpha {ALPHA}, eps {EPS}:",
             "  rows = qatvit_kd_ce_loss_rows (two launches), serial = qatvit_kd_ce_loss_mix (one workgroup, one thread per row; refused above 4096 classes), "
             "bce = qatvit_kd_bce_loss (another objective), torch = the CE objective from stock torch ops + autograd; 'alone' = the C entry on preallocated "
             "buffers, without the wrapper"]
    ok = True
    for B, C in SHAPES:
        s, y, mix, table, index = inputs(B, C, B + C)
        for form in FORMS:
            r = time_arms(arms(form, s, y, mix, table, index), args.calls)
            med = {k: v[0] for k, v in r.items()}
            line = f"  B={B:5d} C={C:5d} {form:12s} rows alone {med['rows alone']:8.1f}  rows {med['rows']:8.1f}  torch {med['torch']:8.1f}"
            if "serial alone" in med:
                held = med["rows alone"] < med["serial alone"]
                gated = C >= 100
                ok = ok and (held or not gated)
                line += (f"  |  serial alone {med['serial alone']:8.1f}  serial {med['serial']:8.1f}  bce alone {med['bce alone']:8.1f}  |  serial alone / rows alone "
                         f"{med['serial alone'] / med['rows alone']:7.2f}x  rows alone / bce alone {med['rows alone'] / med['bce alone']:5.2f}x  -> "
                         + (("holds" if held else "DOES NOT HOLD") if gated else "not gated"))
            else:
                line += "  |  serial and bce: refused (C > 4096)"
            lines.append(line)
            lines.append("      repetitions: " + "; ".join(f"{k} {', '.join(f'{v:.1f}' for v in r[k][1])}" for k in r))
    lines.append(f"condition (rows alone < serial alone at every shape with C >= 100 and in every form): {'holds' if ok else 'DOES NOT HOLD'}")
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
