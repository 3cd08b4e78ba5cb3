"""The classifier head per call, form 0 (one block per image) against form 1 (MFMA, head_mfma.hip) through qatvit_head_forward / qatvit_head_backward, and
the ViT-S batch-256 student step at 1000 classes with QATVIT_HEAD_MFMA on and off.  Arms alternate in one process (the step: in alternating child
processes, the knob is read once per process); every figure is the median of the rounds with their spread.  Writes profiles/head_mfma_bench.txt.

    python tools/bench_head.py            # everything (BENCH_HEAD_OUT=path: write there instead)
    python tools/bench_head.py step       # (child) one arm of the whole step: prints ms per step"""
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
SHAPES = [(256, 384, 10), (256, 384, 128), (256, 384, 1000), (256, 384, 21841), (256, 384, 32768), (1024, 384, 1000)]
ROUNDS = 5


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n   # us per call


def operands(B, D, C):
    g = torch.Generator().manual_seed(C)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    x = r(B, D)
    o = dict(x=x, mean=x.mean(1), rstd=(x.var(1, unbiased=False) + 1e-6).rsqrt(), gamma=1 + 0.1 * r(D), beta=0.1 * r(D),
             qp_norm=torch.tensor([0.02, 50.0, 128.0, 1.0], device=DEV), qp_logits=torch.tensor([0.05, 20.0, 128.0, 1.0], device=DEV),
             wq=torch.randint(-127, 128, (C, D), generator=g).float().bfloat16().to(DEV), w_scale=(0.002 + 0.004 * torch.rand(C, generator=g)).to(DEV),
             w_zp=torch.zeros(C, dtype=torch.int32, device=DEV), bias=r(C), W=0.3 * r(C, D), dl=1e-3 * r(B, C),
             hq=torch.empty(B, D, device=DEV), hq16=torch.empty(B, D, dtype=torch.bfloat16, device=DEV), lp=torch.empty(B, C, device=DEV),
             dW=torch.empty(C, D, device=DEV), db=torch.empty(C, device=DEV), dh=torch.empty(B, D, device=DEV))
    st = torch.zeros(32 * 32, dtype=torch.int32)
    st[0::32], st[1::32] = 0xFF800000 - (1 << 32), 0x007FFFFF
    o["stats"] = st.to(DEV)
    return o


def head_calls(L, o, B, D, C, form):
    s = torch.cuda.current_stream().cuda_stream
    n = L.qatvit_head_scratch_bytes(B, D, C)
    scratch = torch.empty(max(n, 4), dtype=torch.uint8, device=DEV)
    p = lambda k: o[k].data_ptr()

    def fwd():
        assert L.qatvit_head_forward(p("x"), p("mean"), p("rstd"), p("gamma"), p("beta"), p("qp_norm"), 0, 255, p("wq"), p("w_scale"), 1, p("bias"), p("hq"), p("hq16"),
                                     p("lp"), p("stats"), B, D, 1, C, form, s) == 0, L.qatvit_last_error()

    def bwd():
        assert L.qatvit_head_backward(p("dl"), p("lp"), p("qp_logits"), 0, 255, p("hq"), p("hq16"), p("qp_norm"), p("wq"), p("W"), p("w_scale"), p("w_zp"), 1, -128, 127,
                                      p("dW"), p("db"), p("dh"), scratch.data_ptr(), n, B, D, C, form, s) == 0, L.qatvit_last_error()
    return fwd, bwd, scratch


def step_arm():
    from qat_vit_amd import functional as F
    from tests.util import prepare

    torch.manual_seed(0)
    m = prepare(qat_vit_amd.create_student("vit", num_classes=1000, qat_wrapper=True).cuda(), "qnnpack")
    x, y = torch.randn(256, 3, 224, 224, device=DEV), torch.randint(0, 1000, (256,), device=DEV)

    def one():
        for q in m.parameters():
            q.grad = None
        F.kd_ce_loss(m(x), None, y, 4.0, 0.5, 0.1)[0].backward()
    for _ in range(4):
        one()
    torch.cuda.synchronize()
    print("STEP_MS", statistics.median(timed(one, 5) / 1e3 for _ in range(3)))


def spread(v):
    return f"{statistics.median(v):9.1f} us ({min(v):.1f} .. {max(v):.1f})"


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "step":
        return step_arm()
    L = native.lib()
    out = [f"tools/bench_head.py on {torch.cuda.get_device_name(0)}: us per call, median of {ROUNDS} alternating rounds (min .. max); per-channel weight scales", ""]
    for B, D, C in SHAPES:
        o = operands(B, D, C)
        forms = [0, 1] if C >= 128 else [0]
        calls = {f: head_calls(L, o, B, D, C, f) for f in forms}
        res = {(f, k): [] for f in forms for k in (0, 1)}
        for f in forms:
            calls[f][0](); calls[f][1]()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for f in forms:
                n = 20 if (f == 1 or C <= 1000) else 3
                for k in (0, 1):
                    res[(f, k)].append(timed(calls[f][k], n))
        for k, name in ((0, "forward "), (1, "backward")):
            out.append(f"B {B:5d} D {D} C {C:6d} {name}: " + " | ".join(f"form {f} {spread(res[(f, k)])}" for f in forms))
        if C == 21841:   # algorithmic bytes of the three kernels against 8 TB/s
            fb = C * D * 2 + B * C * 4 + B * D * 2
            bb = 4 * B * C * 4 + C * D * 2 + B * D * 2 + 2 * C * D * 4
            out.append(f"    algorithmic bytes at C = 21841: forward {fb / 1e6:.1f} MB = {fb / 8e6:.1f} us at 8 TB/s; dgrad + wgrad {bb / 1e6:.1f} MB = {bb / 8e6:.1f} us at 8 TB/s")
    arms = {"on": [], "off": []}
    for _ in range(2):
        for arm in ("on", "off"):
            env = {k: v for k, v in os.environ.items() if not k.startswith("QATVIT_")}
            if arm == "off":
                env["QATVIT_HEAD_MFMA"] = "0"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "step"], env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
            if r.returncode != 0:
                raise SystemExit(f"step arm {arm} failed ({r.returncode}): {r.stderr[-800:]}")
            arms[arm].append(float(r.stdout.split("STEP_MS")[1].split()[0]))
    out += ["", "ViT-S student step, batch 256, 1000 classes, qnnpack; ms per forward + backward, two alternating child processes per arm:",
            f"    QATVIT_HEAD_MFMA unset: {arms['on']}   QATVIT_HEAD_MFMA=0: {arms['off']}"]
    text = "\n".join(out) + "\n"
    print(text)
    dst = os.environ.get("BENCH_HEAD_OUT", os.path.join(ROOT, "profiles", "head_mfma_bench.txt"))
    open(dst, "w").write(text)


if __name__ == "__main__":
    main()
