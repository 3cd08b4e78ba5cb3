#!/usr/bin/env python3
"""Times the binary cross-entropy objective (qatvit_kd_bce_loss, F.kd_bce_loss) on one MI355X and writes profiles/bce_loss_bench.txt.

Shapes (B, C) = (256, 10), (256, 100), (256, 1000), (1024, 1000); forms: plain (labels only), mix (labels + mix records), mix + table (labels, mix
records and a teacher logit table of 4 * B rows).  Per shape and form, in one process:
  new    F.kd_bce_loss: loss and dlogits in one call (two launches), the wrapper's allocations included; and the C entry alone on preallocated buffers;
  torch  the same objective composed from stock torch ops in fp32 - smoothed one-hot by scatter_, the mix by index_select,
         F.binary_cross_entropy_with_logits, the KD term - and torch.autograd.grad for dlogits: what a user writes today;
  ce     the existing softmax-CE entry of the same form (F.kd_ce_loss_mix / F.kd_ce_loss_table_mix, one single-workgroup launch with one thread per
         row), through its wrapper and alone.  ANOTHER objective: it is here to show what the per-row serial form costs as C grows.
Every figure: the median of five repetitions of --calls calls between two HIP events after a warm-up of every arm, the arms interleaved
(new, torch, ce, new, ...), so the drift of the clocks inside the run falls on all of them; launch and host glue are included, as a training
step pays them.

The one condition: new < torch at every shape and form.  The exit status says whether it held.

Also recorded: the fp32 error of the entry and of the torch composition against the composition evaluated in fp64, at the large class counts of
tests/test_gpu_bce_loss.py.

usage: python3 tools/bench_bce_loss.py [--calls N] [--out FILE]"""
import argparse
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
SHAPES = [(256, 10), (256, 100), (256, 1000), (1024, 1000)]
FORMS = ["plain", "mix", "mix + table"]
T, ALPHA, EPS = 4.0, 0.5, 0.1
CLOCK_NOTE = ("clocks: as the machine had them (not pinned, not changed, not read); every figure follows its own warm-up, and the interleaved "
              "repetitions show the drift inside this run")


def composition(student, labels, mix=None, table=None, index=None, target_threshold=None, sum_classes=False):
    """(loss, bce, kd * T^2) from stock torch ops in the dtype of `student`; nothing is read on the host."""
    B, C = student.shape
    dt, dev = student.dtype, student.device
    ar = torch.arange(B, device=dev)
    if mix is None:
        part, lam = ar, torch.ones(B, dtype=dt, device=dev)
    else:
        p = mix[:, 0].long()
        part = torch.where((p >= 0) & (p < B), p, ar)
        lam = mix[:, 5].contiguous().view(torch.float32)
    oml = (1 - lam).to(dt)[:, None]
    lam = lam.to(dt)[:, None]
    off = EPS / C
    onehot = torch.full((B, C), off, dtype=dt, device=dev).scatter_(1, labels.view(-1, 1), 1.0 - EPS + off)
    t = lam * onehot + oml * onehot.index_select(0, part)
    if target_threshold is not None:
        t = (t > target_threshold).to(dt)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(student, t, reduction="sum") / (B if sum_classes else B * C)
    if table is None:
        return bce, bce, torch.zeros((), dtype=dt, device=dev)
    q = torch.softmax(table.to(dt).index_select(0, index) / T, 1)
    q2 = torch.softmax(table.to(dt).index_select(0, index.index_select(0, part)) / T, 1)
    q = torch.where(lam != 1, lam * q + oml * q2, q)
    kd = (torch.xlogy(q, q) - q * torch.log_softmax(student / T, 1)).sum(1).mean() * T * T
    return ALPHA * kd + (1.0 - ALPHA) * bce, bce, kd


def inputs(B, C, seed):
    """student, labels, mix records (mixup with the flipped batch, one lam per row, every eighth row unmixed), table, index - all on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = 3 * torch.randn(B, C, device="cuda", generator=g)
    y = torch.randint(0, C, (B,), device="cuda", generator=g)
    lam = torch.rand(B, device="cuda", generator=g)
    lam[::8] = 1.0
    mix = torch.zeros(B, 6, dtype=torch.int32, device="cuda")
    mix[:, 0] = torch.arange(B - 1, -1, -1, device="cuda", dtype=torch.int32)
    mix[:, 1], mix[:, 2], mix[:, 5] = lam.view(torch.int32), (1 - lam).view(torch.int32), lam.view(torch.int32)
    table = 5 * torch.randn(4 * B, C, device="cuda", generator=g)
    index = torch.randint(0, 4 * B, (B,), device="cuda", generator=g)
    return s, y, mix, table, index


def arms(form, s, y, mix, table, index):
    """name -> a callable that computes the loss and dlogits once."""
    import qat_vit_amd.functional as F
    from qat_vit_amd import native

    B, C = s.shape
    m = None if form == "plain" else mix
    tab, idx = (table, index) if form == "mix + table" else (None, None)
    L = native.lib()
    out3, partials, dl = torch.empty(3, device="cuda"), torch.empty(2 * B, device="cuda"), torch.empty_like(s)
    ptr = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    rows = 0 if tab is None else tab.shape[0]
    sg = s.clone().requires_grad_(True)

    def torch_arm():
        return torch.autograd.grad(composition(sg, y, m, tab, idx)[0], sg)

    def new_alone():
        native.check(L.qatvit_kd_bce_loss(ptr(s), None, ptr(tab), rows, ptr(idx), ptr(y), ptr(m), B, C, T, ALPHA, EPS, -1.0, 0, ptr(partials), ptr(out3),
                                          ptr(dl), native.stream_ptr()), "qatvit_kd_bce_loss")

    def ce_alone():
        native.check(L.qatvit_kd_ce_loss_mix(ptr(s), None, ptr(tab), rows, ptr(idx), ptr(y), ptr(m), B, C, T, ALPHA, EPS, ptr(out3), ptr(dl),
                                             native.stream_ptr()), "qatvit_kd_ce_loss_mix")

    ce = (lambda: F.kd_ce_loss_table_mix(s, tab, idx, y, m, T, ALPHA, EPS)) if tab is not None else (lambda: F.kd_ce_loss_mix(s, None, y, m, T, ALPHA, EPS))
    return {"new": lambda: F.kd_bce_loss(s, y, table=tab, index=idx, mix=m, kd_temp=T, kd_alpha=ALPHA, label_smoothing=EPS), "torch": torch_arm, "ce": ce,
            "new alone": new_alone, "ce alone": ce_alone}


def time_arms(fns, calls):
    """name -> (median, the five repetitions), microseconds per call."""
    for fn in fns.values():
        for _ in range(20):
            fn()
    reps = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(calls):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            reps[k].append(ev[0].elapsed_time(ev[1]) / calls * 1e3)
    return {k: (statistics.median(v), v) for k, v in reps.items()}


def errors(lines):
    import qat_vit_amd.functional as F

    def err(got, grad, want, want_grad):
        rel = [abs(float(a) - float(b)) / max(1.0, abs(float(b))) for a, b in zip(got, want)]
        return rel + [float((grad.double() - want_grad).norm() / want_grad.norm())]

    lines.append("fp32 error against the torch composition evaluated in fp64 (loss, bce, kd: |v - ref| / max(1, |ref|); gradient: relative L2), eps 0.1, "
                 "mean over B * C:")
    for B, C in [(9, 1000), (9, 4096), (1024, 1000)]:
        s, y, mix, table, index = inputs(B, C, 7 * B + C)
        for form in FORMS:
            m = None if form == "plain" else mix
            tab, idx = (table, index) if form == "mix + table" else (None, None)
            s64 = s.double().requires_grad_(True)
            want = composition(s64, y, m, tab, idx)
            want_grad = torch.autograd.grad(want[0], s64)[0]
            s32 = s.clone().requires_grad_(True)
            got = composition(s32, y, m, tab, idx)
            e_torch = err(got, torch.autograd.grad(got[0], s32)[0], want, want_grad)
            sn = s.clone().requires_grad_(True)
            loss, parts = F.kd_bce_loss(sn, y, table=tab, index=idx, mix=m, kd_temp=T, kd_alpha=ALPHA, label_smoothing=EPS)
            e_new = err(parts, torch.autograd.grad(loss, sn)[0], want, want_grad)
            f = lambda e: " ".join(f"{v:.1e}" for v in e)   # noqa: E731
            lines.append(f"  B={B:5d} C={C:5d} {form:12s} entry: {f(e_new)}   torch fp32: {f(e_torch)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bce_loss_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bce_loss.py needs an MI355X: there is no CPU form of the loss to time")
    import qat_vit_amd  # noqa: F401

    lines = [f"binary cross-entropy objective on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per call (loss and dlogits), median of five repetitions of {args.calls} calls, launch and host glue included; T {T}, alpha {ALPHA}, eps {EPS}:",
             "  new = F.kd_bce_loss (two launches), torch = the objective from stock torch ops + autograd, ce = the softmax-CE entry of the same form "
             "(another objective; one workgroup, one thread per row); 'alone' = the C entry on preallocated buffers, no wrapper"]
    ok = True
    for B, C in SHAPES:
        s, y, mix, table, index = inputs(B, C, B + C)
        for form in FORMS:
            r = time_arms(arms(form, s, y, mix, table, index), args.calls)
            held = r["new"][0] < r["torch"][0]
            ok = ok and held
            lines.append(f"  B={B:5d} C={C:5d} {form:12s} new {r['new'][0]:8.1f}  torch {r['torch'][0]:8.1f}  ce {r['ce'][0]:8.1f}  |  new alone {r['new alone'][0]:8.1f}  "
                         f"ce alone {r['ce alone'][0]:8.1f}  |  torch / new {r['torch'][0] / r['new'][0]:5.2f}x  ce alone / new alone "
                         f"{r['ce alone'][0] / r['new alone'][0]:6.2f}x  -> {'holds' if held else 'DOES NOT HOLD'}")
            lines.append("      repetitions: " + "; ".join(f"{k} {', '.join(f'{v:.1f}' for v in r[k][1])}" for k in r))
    lines.append(f"condition (new < torch at every shape and form): {'holds' if ok else 'DOES NOT HOLD'}")
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
