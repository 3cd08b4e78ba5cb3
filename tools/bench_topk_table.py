#!/usr/bin/env python3
"""Times the compressed teacher table (qatvit_teacher_topk_rows, qatvit_kd_ce_loss_topk) on one MI355X and writes profiles/topk_table_bench.txt.

Per (B, C, k) of (1024, 1000, 32), (256, 21841, 16), (256, 21841, 64), (64, 32768, 32), with a table of 4 * B rows, in one process, the arms interleaved:
  compress   qatvit_teacher_topk_rows on a [B, C] chunk of logits (one launch) - what TeacherTopKTable.build pays per teacher chunk;
  sparse     qatvit_kd_ce_loss_topk alone on preallocated buffers (two launches), plain and with mix records;
  dense      qatvit_kd_ce_loss_rows alone with the DECOMPRESSED table of the same rows (the entry the sparse one equals bit for bit).
Every figure: the median of five repetitions of --calls calls between two HIP events after a warm-up of every arm (tools/bench_bce_loss.py's time_arms
and inputs); launch and host glue are included.  Nothing is gated: the gain of the compressed table is capacity, and the bytes are arithmetic.  Before
timing, each shape's sparse result is compared with the dense one (equal bits, or the run stops).

usage: python3 tools/bench_topk_table.py [--calls N] [--out FILE]"""
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

SHAPES = [(1024, 1000, 32), (256, 21841, 16), (256, 21841, 64), (64, 32768, 32)]
T, ALPHA, EPS = 4.0, 0.5, 0.1
DATASETS = [("ImageNet-1k", 1281167, 1000), ("ImageNet-21k", 14197122, 21841)]


def arms(s, y, mix, table, index, k):
    import qat_vit_amd
    from qat_vit_amd import native

    B, C = s.shape
    L = native.lib()
    tab = qat_vit_amd.TeacherTopKTable.from_dense(table, k, T)
    dense = tab.rows(torch.arange(tab.N, device="cuda"))
    chunk = table[:B].contiguous()
    cidx, cval, ctail = torch.empty(B, k, dtype=torch.int16, device="cuda"), torch.empty(B, k, device="cuda"), torch.empty(B, device="cuda")
    bufs = {n: (torch.empty(3, device="cuda"), torch.empty(2 * B, device="cuda"), torch.empty_like(s)) for n in ("sparse", "dense")}
    ptr = lambda v: None if v is None else v.data_ptr()   # noqa: E731

    def compress():
        native.check(L.qatvit_teacher_topk_rows(ptr(chunk), B, C, k, T, ptr(cidx), ptr(cval), ptr(ctail), native.stream_ptr()), "qatvit_teacher_topk_rows")

    def sparse(m):
        out3, partials, dl = bufs["sparse"]
        native.check(L.qatvit_kd_ce_loss_topk(ptr(s), ptr(tab.idx), ptr(tab.val), ptr(tab.tail), tab.N, k, ptr(index), ptr(y), ptr(m), B, C, T, ALPHA, EPS,
                                              ptr(partials), ptr(out3), ptr(dl), native.stream_ptr()), "qatvit_kd_ce_loss_topk")

    def dense_rows(m):
        out3, partials, dl = bufs["dense"]
        native.check(L.qatvit_kd_ce_loss_rows(ptr(s), None, ptr(dense), tab.N, ptr(index), ptr(y), ptr(m), B, C, T, ALPHA, EPS, ptr(partials), ptr(out3),
                                              ptr(dl), native.stream_ptr()), "qatvit_kd_ce_loss_rows")

    for m in (None, mix):
        sparse(m), dense_rows(m)
        torch.cuda.synchronize()
        if not (torch.equal(bufs["sparse"][0], bufs["dense"][0]) and torch.equal(bufs["sparse"][2], bufs["dense"][2])):
            raise SystemExit(f"B={B} C={C} k={k}: the sparse loss differs from the dense entry on the decompressed rows")
    fns = {"compress": compress, "sparse plain": lambda: sparse(None), "dense plain": lambda: dense_rows(None), "sparse mix": lambda: sparse(mix),
           "dense mix": lambda: dense_rows(mix)}
    return fns, tab.nbytes, dense.numel() * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_table_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_table.py needs an MI355X: there is no CPU form of these kernels to time")
    import qat_vit_amd  # noqa: F401

    lines = [f"compressed teacher table on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"us per call, median of five repetitions of {args.calls} calls, launch and host glue included; T {T}, alpha {ALPHA}, eps {EPS}; table of 4 * B rows:",
             "  compress = qatvit_teacher_topk_rows on [B, C] logits (one launch); sparse = qatvit_kd_ce_loss_topk, dense = qatvit_kd_ce_loss_rows on the "
             "decompressed table of the same rows (equal bits, checked before timing); both loss entries alone on preallocated buffers, two launches"]
    for B, C, k in SHAPES:
        s, y, mix, table, index = inputs(B, C, B + C + k)
        fns, sparse_bytes, dense_bytes = arms(s, y, mix, table, index, k)
        r = time_arms(fns, args.calls)
        med = {n: v[0] for n, v in r.items()}
        lines.append(f"  B={B:5d} C={C:5d} k={k:2d}  compress {med['compress']:8.1f}  |  plain: sparse {med['sparse plain']:8.1f}  dense {med['dense plain']:8.1f}  "
                     f"dense / sparse {med['dense plain'] / med['sparse plain']:5.2f}x  |  mix: sparse {med['sparse mix']:8.1f}  dense {med['dense mix']:8.1f}  "
                     f"dense / sparse {med['dense mix'] / med['sparse mix']:5.2f}x  |  table of {4 * B} rows: {sparse_bytes} B compressed, {dense_bytes} B dense")
        lines.append("      repetitions: " + "; ".join(f"{n} {', '.join(f'{v:.1f}' for v in r[n][1])}" for n in r))
        slower = [n for n in ("plain", "mix") if med[f"sparse {n}"] >= med[f"dense {n}"]]
        if slower:
            lines.append(f"      the sparse loss is NOT faster than the dense one here: {', '.join(slower)}")
    lines.append("table bytes (arithmetic: N * (6 k + 4) compressed, N * 4 C dense):")
    for name, N, C in DATASETS:
        lines.append(f"  {name} (N = {N}, C = {C}): dense {N * 4 * C / 1e9:.2f} GB; " + ", ".join(f"k = {k}: {N * (6 * k + 4) / 1e9:.3f} GB" for k in (16, 32, 64)))
    lines.append(CLOCK_NOTE)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
