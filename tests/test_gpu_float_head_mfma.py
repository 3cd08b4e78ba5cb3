"""The float steps' classifier head on MFMA (float_head_mfma.hip; qatvit_float_head_forward / _backward form 1) against the scalar kernels (form 0) and fp64, in
fp32, fp16 and bf16, on guarded operands at the smallest shapes at which the kernels can go wrong: the 128-class threshold's edge with a one-row batch and a
ragged class tile, a ragged row tile, a second 64-row block over several class tiles, an odd class count with misaligned [B, C] rows, more than one class range
per row tile in the dgrad, and the LDS budget at D = 768; then the whole step of each form against QATVIT_FLOAT_HEAD_MFMA=0.
The measured figures (lines starting with FLOAT_HEAD_MFMA, shown with -s) are what profiles/float_head_mfma_errors.txt holds."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
from tests.kernel_check import guarded_copy, rel_l2_t, tile_errors  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SHAPES = [(1, 128, 129), (3, 128, 136), (65, 384, 1000), (5, 384, 1001), (4, 128, 4099), (2, 768, 130)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]   # the C ABI's dtype codes 0, 1, 2
T = 3                                                     # tokens per image: the head reads rows b * T


def _operands(B, D, C, dt, exact, seed):
    """Everything on the device, the large tensors inside guarded padding.  exact: small integers times powers of two - at most 5 significant bits (bf16 keeps
    8), every product and partial sum a multiple of one power of two below 2^24 of it at every shape of SHAPES (asserted), logits below 768 * 56 / 64 + 2."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    if exact:
        assert max(D * 7 * 8, C * 4 * 8, B * 4 * 7) < 2 ** 24
        x, W, bias, dl = ri(-7, 7, B * T, D), ri(-8, 8, C, D) * 2.0 ** -6, ri(-16, 16, C) * 0.125, ri(-4, 4, B, C) * 2.0 ** -4
        mean, rstd, gamma, beta = torch.zeros(B * T), torch.ones(B * T), torch.ones(D), torch.zeros(D)     # hn = x exactly
    else:
        x, W, bias, dl = torch.randn(B * T, D, generator=g) * 1.7 + 0.3, torch.randn(C, D, generator=g) * 0.05, torch.randn(C, generator=g) * 0.5, torch.randn(B, C, generator=g) * 1e-2
        mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-6).rsqrt()
        gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    o = {"shape": (B, D, C), "dt": dt, "code": DTYPES.index(dt), "checks": []}
    for k, v in (("x", x), ("W", W), ("dl", dl.to(dt))):
        o[k], c = guarded_copy(v.to(DEV))
        o["checks"].append(c)
    o.update({k: v.to(DEV) for k, v in (("mean", mean), ("rstd", rstd), ("gamma", gamma), ("beta", beta), ("bias", bias))})
    return o


def _out(shape, dtype=torch.float32):
    return guarded_copy(torch.full(shape, float("nan"), dtype=dtype, device=DEV))


def _forward(L, form, o, stats=False):
    B, D, C = o["shape"]
    (hn, c1), (lg, c2) = _out((B, D)), _out((B, C), o["dt"])
    st = torch.zeros(32 * 32, dtype=torch.int32)
    st[0::32], st[1::32] = 0xFF800000 - (1 << 32), 0x007FFFFF
    st = st.to(DEV)
    rc = L.qatvit_float_head_forward(o["x"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(), o["gamma"].data_ptr(), o["beta"].data_ptr(), o["W"].data_ptr(),
                                     o["bias"].data_ptr(), hn.data_ptr(), lg.data_ptr(), st.data_ptr() if stats else None, B, D, T, C, o["code"], form,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.qatvit_last_error()
    torch.cuda.synchronize()
    for c in [c1, c2] + o["checks"]:
        c(f"forward form {form}")
    u = st.cpu().to(torch.int64) & 0xFFFFFFFF     # the fold over the slots (which slot a value lands in depends on the grid)
    return hn, lg, (int(u[0::32].min()), int(u[1::32].max()))


def _backward(L, form, o, hn):
    B, D, C = o["shape"]
    (dW, c1), (db, c2), (dh, c3) = _out((C, D)), _out((1, C)), _out((B, D))
    n = L.qatvit_float_head_scratch_bytes(B, D, C)
    scratch, c4 = _out((n // (4 * D), D))
    rc = L.qatvit_float_head_backward(o["dl"].data_ptr(), hn.data_ptr(), o["W"].data_ptr(), dW.data_ptr(), db.data_ptr(), dh.data_ptr(), scratch.data_ptr(), n, B, D,
                                      C, o["code"], form, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.qatvit_last_error()
    torch.cuda.synchronize()
    for c in [c1, c2, c3, c4] + o["checks"]:
        c(f"backward form {form}")
    return dW, db, dh


def _ref(o, hn):
    """The contract in fp64, unrounded, on operands rounded as the contract rounds them: logits, dW, dbias, dhn."""
    r = lambda t: t.to(o["dt"]).double()
    dl = o["dl"].double()
    return hn.double() @ r(o["W"]).t() + r(o["bias"]), dl.t() @ hn.double(), dl.sum(0, keepdim=True), dl @ r(o["W"])


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B,D,C", SHAPES)
def test_exact_operands_equal_fp64_and_the_scalar_form(native_lib, B, D, C, dt):
    o = _operands(B, D, C, dt, True, 7 * B + C)
    stats = dt == torch.float32
    hn0, lg0, st0 = _forward(native_lib, 0, o, stats)
    hn1, lg1, st1 = _forward(native_lib, 1, o, stats)
    lg, dW, db, dh = _ref(o, hn0)
    assert torch.equal(hn1, o["x"][::T]) and torch.equal(hn0, hn1) and lg.abs().max() < 65504
    assert torch.equal(lg1, lg.to(dt)) and torch.equal(lg1, lg0) and st1 == st0       # rounded once to the type
    for form in (1, 0):
        for name, got, want in zip(("dW", "dbias", "dhn"), _backward(native_lib, form, o, hn1), (dW.float(), db.float(), dh.to(dt).float())):
            assert torch.equal(got, want), (form, name, (got.double() - want.double()).abs().max().item())


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B,D,C", SHAPES)
def test_random_floats_repeat_and_stay_within_4x_the_scalar_error(native_lib, B, D, C, dt):
    """Form 1 twice: the same bits.  Against the unrounded fp64 contract its worst 16 x 16 tile (kernel_check.tile_errors) is at most 4 x form 0's on the same
    operands: both round the same operands and the same results and differ in the grouping of the fp32 sums alone (the QAT head's margin, measured 0.2 - 1.1 x)."""
    o = _operands(B, D, C, dt, False, 13 * B + C)
    L = native_lib
    hn0, lg0, _ = _forward(L, 0, o)
    hn1, lg1, _ = _forward(L, 1, o)
    assert torch.equal(hn0, hn1) and torch.equal(hn1, hn1.to(dt).float()) and torch.equal(_forward(L, 1, o)[1], lg1)
    one, again, tiny = (lg1,) + _backward(L, 1, o, hn1), (lg1,) + _backward(L, 1, o, hn1), (lg0,) + _backward(L, 0, o, hn1)
    for name, a, b, t, want in zip(("logits", "dW", "dbias", "dhn"), one, again, tiny, _ref(o, hn1)):
        assert torch.equal(a, b), f"{name}: two calls of form 1 differ"
        e1, e0 = tile_errors(a.float(), want)[1], tile_errors(t.float(), want)[1]
        print(f"FLOAT_HEAD_MFMA {str(dt)[6:]} B {B} D {D} C {C} {name}: worst tile against fp64: form 1 {e1:.3e}, form 0 {e0:.3e}, ratio {e1 / e0 if e0 else 0:.2f}")
        assert torch.equal(a, t) or e1 <= 4 * e0, (name, e1, e0)


# The worst per-parameter relative L2 between the default step and QATVIT_FLOAT_HEAD_MFMA=0 over seeds 0, 1, 2, measured once on an MI355X
# (profiles/float_head_mfma_errors.txt: fp32 6.0e-6 / 6.5e-6 / 6.5e-6; fp16 3.0e-4 / 4.9e-8 / 1.3e-5 - a sum that lands on the other side of an fp16 rounding
# boundary moves one logit by an ulp, or none does; bf16 2.7e-8 / 2.0e-8 / 1.8e-8 with equal logits).  The two steps differ in the head's summation order
# alone, and the bound is 4 x the measured value.
STEP_MEASURED = {"fp32": 6.531e-06, "fp16": 3.038e-04, "bf16": 2.688e-08}


def _worker(tmp_path, tag, knob, kind):
    out = tmp_path / f"{tag}.pt"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QATVIT_")}
    if knob is not None:
        env["QATVIT_FLOAT_HEAD_MFMA"] = knob
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "float_head_worker.py"), str(out), kind, "0"], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, (knob, r.returncode, r.stderr[-1500:])   # (nothing is started after a failure)
    return torch.load(out, weights_only=False)


@pytest.mark.parametrize("kind", ["fp32", "fp16", "bf16"])
def test_whole_step_matches_knob_off(native_lib, tmp_path, kind):
    new = _worker(tmp_path, "mfma", None, kind)
    old = _worker(tmp_path, "scalar", "0", kind)
    assert (new["head_mfma"], old["head_mfma"]) == (1, 0)
    assert new.get("observe_equal", True), "the observe-only forward's logits differ from the float forward's"
    pairs = [("logits", new["logits"], old["logits"]), ("loss", new["loss"], old["loss"])] + [(n, new["grads"][n], g) for n, g in old["grads"].items()]
    worst, name = max((rel_l2_t(a.float(), b.float()), n) for n, a, b in pairs)
    print(f"FLOAT_HEAD_MFMA whole step {kind}: worst relative L2 against QATVIT_FLOAT_HEAD_MFMA=0: {worst:.3e} ({name})")
    assert worst <= 4 * STEP_MEASURED[kind], (worst, name)
