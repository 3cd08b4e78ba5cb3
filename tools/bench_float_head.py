"""The float steps' classifier head per call, form 0 (scalar kernels) against form 1 (MFMA, float_head_mfma.hip) through qatvit_float_head_forward /
qatvit_float_head_backward in fp32, fp16 and bf16, and the ViT-S batch-256 float step of each form at 1000 classes with QATVIT_FLOAT_HEAD_MFMA on and off.  The two
forms alternate in one process (the step: one child process per arm, the knob is read once per process); every figure is the median of the rounds with their
spread.  For form 1 each call's algorithmic bytes against 8 TB/s and FLOPs against the matching MFMA peak (fp32 157 TFLOP/s, 16 bits 2.5 PFLOP/s: BASELINE.md)
give its bound and its share of it.  Writes profiles/float_head_mfma_bench.txt.

    python tools/bench_float_head.py               # everything (BENCH_FLOAT_HEAD_OUT=path: write there instead)
    python tools/bench_float_head.py step fp16     # (child) one arm of the whole step: prints ms per step"""
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qat_vit_amd  # noqa: E402
from qat_vit_amd import native  # noqa: E402

DEV = "cuda"
SHAPES = [(256, 384, 128), (256, 384, 1000), (256, 384, 21841), (256, 384, 32768), (1024, 384, 1000)]
KINDS = [("fp32", torch.float32, 157e12), ("fp16", torch.float16, 2.5e15), ("bf16", torch.bfloat16, 2.5e15)]   # name, element type, MFMA peak FLOP/s
HBM = 8e12
ROUNDS = 5


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n   # us per call


def head_calls(L, B, D, C, code, dt, form):
    g = torch.Generator().manual_seed(C)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    x = r(B, D)
    o = dict(x=x, mean=x.mean(1), rstd=(x.var(1, unbiased=False) + 1e-6).rsqrt(), gamma=1 + 0.1 * r(D), beta=0.1 * r(D), W=0.05 * r(C, D), bias=r(C),
             dl=(1e-2 * r(B, C)).to(dt), hn=torch.empty(B, D, device=DEV), lg=torch.empty(B, C, dtype=dt, device=DEV), dW=torch.empty(C, D, device=DEV),
             db=torch.empty(C, device=DEV), dh=torch.empty(B, D, device=DEV))
    n = L.qatvit_float_head_scratch_bytes(B, D, C)
    o["scratch"] = torch.empty(max(n, 4), dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda k: o[k].data_ptr()

    def fwd():
        assert L.qatvit_float_head_forward(p("x"), p("mean"), p("rstd"), p("gamma"), p("beta"), p("W"), p("bias"), p("hn"), p("lg"), None, B, D, 1, C, code, form,
                                           s) == 0, L.qatvit_last_error()

    def bwd():
        assert L.qatvit_float_head_backward(p("dl"), p("hn"), p("W"), p("dW"), p("db"), p("dh"), p("scratch"), n, B, D, C, code, form, s) == 0, L.qatvit_last_error()
    return fwd, bwd, o


def bounds(B, D, C, es, peak):
    """(least microseconds, which bound) of the forward and of the backward (dgrad + wgrad) from their algorithmic bytes and FLOPs."""
    fb, ff = C * D * 4 + B * D * 4 + B * C * es, 2 * B * C * D
    bb, bf = 2 * (B * C * es + C * D * 4 + B * D * 4), 4 * B * C * D
    return [(max(by / HBM, fl / peak) * 1e6, "HBM" if by / HBM > fl / peak else "MFMA") for by, fl in ((fb, ff), (bb, bf))]


def step_arm(kind):
    from qat_vit_amd import functional as F

    torch.manual_seed(0)
    amp = {"fp32": False, "fp16": True, "bf16": torch.bfloat16}[kind]
    m = qat_vit_amd.native_float(qat_vit_amd.create_student("vit", num_classes=1000, qat_wrapper=True).cuda().train(), amp=amp)
    x, y = torch.randn(256, 3, 224, 224, device=DEV), torch.randint(0, 1000, (256,), device=DEV)

    def one():
        for q in m.parameters():
            q.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16 if kind == "bf16" else torch.float16, enabled=kind != "fp32"):
            out = m(x)
        F.kd_ce_loss(out.float(), None, y, 4.0, 0.5, 0.1)[0].backward()
    for _ in range(3):
        one()
    torch.cuda.synchronize()
    print("STEP_MS", statistics.median(timed(one, 4) / 1e3 for _ in range(3)), "HEAD_MFMA", qat_vit_amd.float_engine.engine_of(m).head_mfma)


def spread(v):
    return f"{statistics.median(v):9.1f} us ({min(v):.1f} .. {max(v):.1f})"


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "step":
        return step_arm(sys.argv[2])
    L = native.lib()
    out = [f"tools/bench_float_head.py on {torch.cuda.get_device_name(0)}: us per call, median of {ROUNDS} alternating rounds (min .. max); every figure measured on the GPU.",
           "backward = dgrad + its reduce + wgrad (one call).  bound: the least time of form 1's algorithmic bytes at 8 TB/s or FLOPs at the MFMA peak; share = bound / median.", ""]
    wins = {}
    for code, (kind, dt, peak) in enumerate(KINDS):
        for B, D, C in SHAPES:
            calls = {f: head_calls(L, B, D, C, code, dt, f) for f in (0, 1)}
            res = {(f, k): [] for f in (0, 1) for k in (0, 1)}
            for f in (0, 1):
                calls[f][0](); calls[f][1]()
            torch.cuda.synchronize()
            for _ in range(ROUNDS):
                for f in (0, 1):
                    for k in (0, 1):
                        res[(f, k)].append(timed(calls[f][k], 20 if (f == 1 or C <= 1000) else 2))
            for k, name in ((0, "forward "), (1, "backward")):
                least, which = bounds(B, D, C, dt.itemsize, peak)[k]
                m0, m1 = statistics.median(res[(0, k)]), statistics.median(res[(1, k)])
                wins[(kind, B, C, name.strip())] = m1 < m0
                out.append(f"{kind} B {B:5d} D {D} C {C:6d} {name}: form 0 {spread(res[(0, k)])} | form 1 {spread(res[(1, k)])} | x{m0 / m1:6.1f} | bound {which} {least:7.1f} us,"
                           f" share {least / m1:.3f}")
        out.append("")
    lost = [k for k, w in wins.items() if not w]
    out.append("form 1 is the faster one at every measured shape, dtype and direction: the threshold stays at 128 classes" if not lost else f"form 1 loses at: {lost}")
    out += ["", "ViT-S float step, batch 256, 1000 classes; ms per forward + backward, one child process per arm (engine head_mfma in brackets):"]
    for kind, _, _ in KINDS:
        arms = {}
        for arm in ("on", "off"):
            env = {k: v for k, v in os.environ.items() if not k.startswith("QATVIT_")}
            if arm == "off":
                env["QATVIT_FLOAT_HEAD_MFMA"] = "0"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "step", kind], env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
            if r.returncode != 0:
                raise SystemExit(f"step arm {kind} {arm} failed ({r.returncode}): {r.stderr[-800:]}")   # (nothing is started after a failure)
            w = r.stdout.split("STEP_MS")[1].split()
            arms[arm] = f"{float(w[0]):.3f} [{w[2]}]"
        out.append(f"    {kind}: QATVIT_FLOAT_HEAD_MFMA unset: {arms['on']}   QATVIT_FLOAT_HEAD_MFMA=0: {arms['off']}")
    text = "\n".join(out) + "\n"
    print(text)
    dst = os.environ.get("BENCH_FLOAT_HEAD_OUT", os.path.join(ROOT, "profiles", "float_head_mfma_bench.txt"))
    open(dst, "w").write(text)


if __name__ == "__main__":
    main()
