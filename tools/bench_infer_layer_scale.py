#!/usr/bin/env python3
"""Forward time of the integer inference with LayerScale against the same forward without the gammas and against the fake-quant forward, on one MI355X:
profiles/infer_layer_scale_bench.txt.

    python tools/bench_infer_layer_scale.py [--batch 256] [--window 1.0] [--warmup 5] [--rounds 5] [--out profiles/infer_layer_scale_bench.txt]

One ViT-S with init_values (qnnpack), trained for a step at a small batch so that no scale is a default, gammas of mixed sign and magnitude 0.5 .. 2, frozen
and exported once.  Arms, all on the same images at 224 x 224:
  int8 + LayerScale   Int8Student(export, layer_scale=True): qatvit_infer_forward_ls, proj / fc2 with the kEpiResidFqLs epilogue
  int8 plain          Int8Student on the same export with the gamma entries removed: qatvit_infer_forward, the kEpiResidFq epilogue
  fake-quant          import_int8(export): the native QAT forward of the LayerScale model with frozen observers (what stood in for the first arm before)
Each arm is warmed, its window is sized to `--window` seconds of device time from a calibration run, and the arms alternate round by round, so drift hits all
alike; a window lies between two device events and ends in their synchronisation.  Prints ms per forward (min / median / max over the rounds, and the spread
(max - min) / median), the extra work of the first arm over the second as the algorithm counts it, and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import qat_vit_amd  # noqa: E402
from qat_vit_amd import functional as F  # noqa: E402
from qat_vit_amd.export import Int8Student, export_int8, import_int8  # noqa: E402


def build_export():
    from torch.ao.quantization import disable_observer, get_default_qat_qconfig, prepare_qat

    torch.manual_seed(0)
    w = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, init_values=1.0).cuda().train()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w.qconfig = get_default_qat_qconfig("qnnpack")
        m = prepare_qat(w, inplace=False).cuda().train()
    x = torch.randn(4, 3, 224, 224, device="cuda")
    y = torch.randint(0, 10, (4,), device="cuda")
    opt = qat_vit_amd.ClipAdamW(m.parameters(), lr=1e-3)
    F.kd_ce_loss(m(x), None, y, 4.0, 0.5, 0.1)[0].backward()
    opt.step(max_norm=1.0)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith(".gamma"):
                v = (0.5 + 1.5 * torch.rand(p.numel(), generator=g)) * torch.where(torch.rand(p.numel(), generator=g) < 0.5, -1.0, 1.0)
                p.copy_(v.to(p.device))
        m(x)
    m.apply(disable_observer)
    return export_int8(m.eval())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of device time per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "infer_layer_scale_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_infer_layer_scale: needs an MI355X (there is nothing to measure without one)")
    e = build_export()
    depth, dim = e["arch"]["depth"], e["arch"]["embed_dim"]
    plain_e = dict(e)
    plain_e["float"] = {n: t for n, t in e["float"].items() if not n.endswith(".gamma")}
    ls, plain, fq = Int8Student(e, layer_scale=True), Int8Student(plain_e), import_int8(e)
    x = torch.randn(a.batch, 3, 224, 224, device="cuda")
    arms = {"int8 + LayerScale": lambda: ls(x), "int8 plain": lambda: plain(x), "fake-quant (import_int8)": lambda: fq(x)}
    lines = []

    def say(s=""):
        print(s)
        lines.append(s)

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    with torch.no_grad():
        same = torch.equal(ls(x), fq(x))
        iters = {}
        for name, fn in arms.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            iters[name] = max(10, int(a.window * 1e3 / window(fn, 10)))
        ms = {n: [] for n in arms}
        for _ in range(a.rounds):
            for name, fn in arms.items():
                ms[name].append(window(fn, iters[name]))
    tokens = a.batch * ((e["arch"]["img_size"] // e["arch"]["patch_size"]) ** 2 + 1)
    say(f"ViT-S (depth {depth}, width {dim}), batch {a.batch}, 224 x 224, qnnpack; {a.rounds} alternating rounds, windows of about {a.window:g} s of device time")
    say(f"device: {torch.cuda.get_device_name(0)}; logits of the LayerScale integer forward equal the fake-quant forward's bit for bit: {same}")
    for name, v in ms.items():
        med = statistics.median(v)
        say(f"{name:28s} {iters[name]:4d} forwards / window   ms/forward min {min(v):7.3f}  median {med:7.3f}  max {max(v):7.3f}   spread {(max(v) - min(v)) / med * 100:5.2f} %"
            f"   {a.batch / med * 1e3:8.0f} img/s")
    m_ls, m_pl, m_fq = (statistics.median(ms[n]) for n in arms)
    say(f"LayerScale over plain: {m_ls - m_pl:+.3f} ms ({(m_ls / m_pl - 1) * 100:+.2f} %); fake-quant over the LayerScale integer forward: {m_fq / m_ls:.2f} x")
    say(f"extra work of the LayerScale form as the algorithm counts it: 2 * depth * D * 4 = {2 * depth * dim * 4} bytes of gamma per forward (re-read per 208-row tile "
        f"from the caches: {2 * depth * -(-tokens // 208)} tiles x {dim * 4} B), one multiply per residual element = 2 * depth * tokens * D = "
        f"{2 * depth * tokens * dim / 1e6:.1f} M multiplies, beside the {2 * depth * tokens * dim * 8 / 1e6:.0f} MB of residual stream (4 B read + 4 B written per element) "
        f"that the {2 * depth} residual epilogues of a forward move anyway")
    say(json.dumps({"batch": a.batch, "rounds": a.rounds, "forwards_per_window": iters, "ms_per_forward": ms, "bit_identical_to_fake_quant": same}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
