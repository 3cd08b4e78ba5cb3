"""The classifier head on MFMA (head_mfma.hip; qatvit_head_forward / qatvit_head_backward form 1) against the one-block-per-image kernels (form 0) and fp64,
on guarded operands, at the smallest shapes at which the kernels can go wrong: the 128-class threshold's edge, a one-row batch, a ragged row tile, an odd class
count with misaligned [B, C] rows, more than one class range per row tile in the dgrad and more than one class tile; then the whole step and Int8Student.
The measured errors of the float cases (lines starting with HEAD_MFMA, shown with -s) are what profiles/head_mfma_errors.txt holds."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
from tests.kernel_check import guarded_copy, rel_l2_t  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SHAPES = [(1, 128, 129), (3, 128, 136), (65, 384, 1000), (5, 384, 1001), (4, 128, 4099)]
T = 3                     # tokens per image: the head reads rows b * T
QMIN, QMAX, WQMIN, WQMAX = 0, 255, -128, 127


def _g(x):
    """x on the device inside guarded padding: (view, check)."""
    return guarded_copy(x.to(DEV))


def _qp(scale, zp):
    return torch.tensor([scale, 1.0 / scale, zp, 1.0], dtype=torch.float32)


def _stats():
    s = torch.zeros(32 * 32, dtype=torch.int32)
    s[0::32], s[1::32] = 0xFF800000 - (1 << 32), 0x007FFFFF
    return s


def _fold(stats):
    """The {min, max} pairs folded over the slots, as the order-preserving words (which slot a value lands in depends on the grid, the fold does not)."""
    u = stats.cpu().to(torch.int64) & 0xFFFFFFFF
    return int(u[0::32].min()), int(u[1::32].max())


def _forward(L, form, o):
    B, D, C = o["shape"]
    hq, c1 = _g(torch.full((B, D), float("nan")))
    hq16, c2 = _g(torch.full((B, D), float("nan"), dtype=torch.bfloat16))
    lp, c3 = _g(torch.full((B, C), float("nan")))
    st = _stats().to(DEV)
    rc = L.qatvit_head_forward(o["x"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(), o["gamma"].data_ptr(), o["beta"].data_ptr(), o["qp_norm"].data_ptr(),
                               QMIN, QMAX, o["wq"].data_ptr(), o["w_scale"].data_ptr(), o["pc"], o["bias"].data_ptr(), hq.data_ptr(), hq16.data_ptr(),
                               lp.data_ptr(), st.data_ptr(), B, D, T, C, form, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.qatvit_last_error()
    torch.cuda.synchronize()
    for c in (c1, c2, c3) + o["checks"]:
        c(f"forward form {form}")
    return hq, hq16, lp, _fold(st)


def _backward(L, form, o):
    B, D, C = o["shape"]
    dW, c1 = _g(torch.full((C, D), float("nan")))
    db, c2 = _g(torch.full((1, C), float("nan")))
    dh, c3 = _g(torch.full((B, D), float("nan")))
    n = L.qatvit_head_scratch_bytes(B, D, C)
    scratch, c4 = _g(torch.full((n // (4 * D), D), float("nan")))
    rc = L.qatvit_head_backward(o["dl"].data_ptr(), o["lp"].data_ptr(), o["qp_logits"].data_ptr(), QMIN, QMAX, o["hq"].data_ptr(), o["hq16"].data_ptr(),
                                o["qp_norm"].data_ptr(), o["wq"].data_ptr(), o["W"].data_ptr(), o["w_scale"].data_ptr(), o["w_zp"].data_ptr(), o["pc"], WQMIN, WQMAX,
                                dW.data_ptr(), db.data_ptr(), dh.data_ptr(), scratch.data_ptr(), n, B, D, C, form, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.qatvit_last_error()
    torch.cuda.synchronize()
    for c in (c1, c2, c3, c4) + o["checks"]:
        c(f"backward form {form}")
    return dW, db[0], dh


def _bwd_ref(o, s_l, zp_l):
    """fp64: the STE masks, dW, dbias, dh."""
    lp, dl, W, sw = o["lp"].double(), o["dl"].double(), o["W"].double(), o["w_scale"].double()
    t = torch.round(lp.float() * (1.0 / s_l)).double() + zp_l          # (the kernel's fp32 product, then exact integers)
    d = dl * ((t >= QMIN) & (t <= QMAX))
    tw = torch.round((o["W"] * (1.0 / o["w_scale"]).unsqueeze(1)).float()).double() + o["w_zp"].double().unsqueeze(1)
    dW = (d.t() @ o["hq"].double()) * o["qp_norm"][0].double() * ((tw >= WQMIN) & (tw <= WQMAX))
    return dW, d.sum(0), (d * sw) @ o["wq"].double()


def _bwd_operands(B, D, C, pc, exact, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    o = {"shape": (B, D, C), "pc": pc}
    if exact:   # every product and every sum exact in fp32 whatever the order: K * max|a| * max|b| < 2^24 at every shape of SHAPES
        s_l, zp_l = 2.0 ** -3, 128.0
        dl, wq, lp = ri(-4, 4, B, C) * 2.0 ** -12, ri(-16, 16, C, D), ri(-200, 200, B, C) * 0.125     # |lp| > 16: outside the quantiser's range
        w_scale = 2.0 ** -(5 + torch.arange(C if pc else 1) % 4).float()
        W = torch.where(torch.rand(C, D, generator=g) < 0.1, ri(-300, 300, C, D), wq) * w_scale.unsqueeze(1)   # a tenth of them may clip
        w_zp, s_n = torch.zeros(C if pc else 1, dtype=torch.int32), 2.0 ** -5
    else:
        s_l, zp_l = 0.0371, 131.0
        dl, wq, lp = torch.randn(B, C, generator=g) * 1e-3, ri(-127, 127, C, D), torch.randn(B, C, generator=g) * 3.0
        w_scale = 0.002 + 0.004 * torch.rand(C if pc else 1, generator=g)
        W = torch.randn(C, D, generator=g) * 70.0 * w_scale.unsqueeze(1)
        w_zp, s_n = torch.randint(-3, 4, (C if pc else 1,), generator=g).int(), 0.0213
    hq = ri(-128, 127, B, D)
    o["qp_logits"], o["qp_norm"] = _qp(s_l, zp_l).to(DEV), _qp(s_n, 128.0).to(DEV)
    checks = []
    for k, v in (("dl", dl), ("lp", lp), ("wq", wq.bfloat16()), ("W", W), ("hq", hq), ("hq16", hq.bfloat16())):
        o[k], c = _g(v)
        checks.append(c)
    o["w_scale"], o["w_zp"], o["checks"] = w_scale.to(DEV), w_zp.to(DEV), tuple(checks)
    return o, s_l, zp_l


@pytest.mark.parametrize("pc", [0, 1])
@pytest.mark.parametrize("B,D,C", SHAPES)
def test_forward_equals_tiny_form_and_fp64(native_lib, B, D, C, pc):
    g = torch.Generator().manual_seed(B * 7 + C)
    x = torch.randn(B * T, D, generator=g) * 1.7 + 0.3
    o = {"shape": (B, D, C), "pc": pc, "mean": x.mean(1).to(DEV), "rstd": (x.var(1, unbiased=False) + 1e-6).rsqrt().to(DEV),
         "gamma": (1 + 0.2 * torch.randn(D, generator=g)).to(DEV), "beta": (0.1 * torch.randn(D, generator=g)).to(DEV), "qp_norm": _qp(0.012, 128.0).to(DEV),
         "w_scale": (0.002 + 0.004 * torch.rand(C if pc else 1, generator=g)).to(DEV), "bias": torch.randn(C, generator=g).to(DEV)}
    (o["x"], cx), (o["wq"], cw) = _g(x), _g(torch.randint(-127, 128, (C, D), generator=g).float().bfloat16())
    o["checks"] = (cx, cw)
    hq0, _, lp0, st0 = _forward(native_lib, 0, o)
    hq1, hq16, lp1, st1 = _forward(native_lib, 1, o)
    assert torch.equal(hq1, hq0) and torch.equal(hq16.float(), hq0) and hq0.abs().max() <= 255 and (hq0.abs() >= 127).any()    # (some elements clip)
    acc = (hq0.double() @ o["wq"].double().t()).float()               # exact: integers below 2^24
    ref = acc * (o["qp_norm"][0] * o["w_scale"]) + o["bias"]           # fp32, one rounding per operation as the kernels'
    assert acc.abs().max() < 2 ** 24
    assert torch.equal(lp1, lp0) and torch.equal(lp1, ref)
    assert st1 == st0 and st0 == tuple(int(v.view(torch.int32)) & 0xFFFFFFFF ^ (0x80000000 if v >= 0 else 0xFFFFFFFF) for v in (ref.min().cpu(), ref.max().cpu()))


@pytest.mark.parametrize("pc", [0, 1])
@pytest.mark.parametrize("B,D,C", SHAPES)
def test_backward_exact_inputs(native_lib, B, D, C, pc):
    o, s_l, zp_l = _bwd_operands(B, D, C, pc, True, 11 * B + C)
    ref = _bwd_ref(o, s_l, zp_l)
    masked = (o["lp"].abs() > 16).float().mean().item()
    assert 0.05 < masked < 0.95 and (ref[0] == 0).any()
    for form in (1, 0):
        for name, got, want in zip(("dW", "dbias", "dh"), _backward(native_lib, form, o), ref):
            assert torch.equal(got, want.float()), (form, name, (got.double() - want).abs().max().item())


@pytest.mark.parametrize("pc", [0, 1])
@pytest.mark.parametrize("B,D,C", SHAPES)
def test_backward_random_floats(native_lib, B, D, C, pc):
    """Form 1 twice: the same bits.  Against fp64 its relative L2 error is at most 4 x form 0's on the same inputs: the three-plane split adds at most
    3 * 2^-27 per term, below fp32's unit; what remains is another grouping of the same fp32 sums (a dropped lo plane is 2^-18, a dropped mid plane 2^-9)."""
    o, s_l, zp_l = _bwd_operands(B, D, C, pc, False, 13 * B + C)
    ref = _bwd_ref(o, s_l, zp_l)
    one, again, tiny = _backward(native_lib, 1, o), _backward(native_lib, 1, o), _backward(native_lib, 0, o)
    for name, a, b, t, want in zip(("dW", "dbias", "dh"), one, again, tiny, ref):
        assert torch.equal(a, b), f"{name}: two calls of form 1 differ"
        e1, e0 = rel_l2_t(a, want), rel_l2_t(t, want)
        print(f"HEAD_MFMA B {B} D {D} C {C} per_channel {pc} {name}: rel L2 against fp64: form 1 {e1:.3e}, form 0 {e0:.3e}")
        assert torch.equal(a, t) or e1 <= 4 * e0, (name, e1, e0)


# The worst per-parameter relative L2 of the default step's gradients against QATVIT_HEAD_MFMA=0, measured once on an MI355X (profiles/head_mfma_errors.txt).
# The forward and every STE mask are bit-identical, so only the head's fp32 rounding propagates, linearly: the bound is 4 x the measured value.
STEP_MEASURED = {"qnnpack": 6.664e-06, "x86": 7.177e-06}


def _worker(tmp_path, tag, knob, backend):
    out = tmp_path / f"{tag}.pt"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QATVIT_")}
    if knob is not None:
        env["QATVIT_HEAD_MFMA"] = knob
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "head_worker.py"), str(out), backend], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (knob, r.returncode, r.stderr[-1500:])   # (nothing is started after a failure)
    return torch.load(out, weights_only=False)


@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_whole_step_matches_knob_off(native_lib, tmp_path, backend):
    new = _worker(tmp_path, "mfma", None, backend)
    old = _worker(tmp_path, "tiny", "0", backend)
    assert (new["head_mfma"], old["head_mfma"]) == (1, 0)
    assert torch.equal(new["logits"], old["logits"]) and torch.equal(new["loss"], old["loss"])
    for n, ts in old["fq"].items():
        assert all(torch.equal(a, b) for a, b in zip(new["fq"][n], ts)), n
    worst, name = max((rel_l2_t(new["grads"][n], g), n) for n, g in old["grads"].items())
    print(f"HEAD_MFMA whole step {backend}: worst per-parameter gradient rel L2 against QATVIT_HEAD_MFMA=0: {worst:.3e} ({name})")
    assert worst <= 4 * STEP_MEASURED[backend], (worst, name)


def test_int8_student_at_1000_classes(native_lib):
    """The integer inference forward shares the head's forward: logits equal the frozen-observer fake-quant forward's bit for bit at 1000 classes too."""
    import qat_vit_amd
    from qat_vit_amd import functional as F
    from qat_vit_amd.export import Int8Student, export_int8
    from tests.util import prepare
    from torch.ao.quantization import disable_observer

    torch.manual_seed(3)
    model = prepare(qat_vit_amd.create_student("vit", num_classes=1000, qat_wrapper=True, depth=1).cuda(), "x86")
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(2, 3, 224, 224, generator=g).cuda(), torch.randint(0, 1000, (2,), generator=g).cuda()
    F.kd_ce_loss(model(x), None, y, 4.0, 0.5, 0.1)[0].backward()
    model.apply(disable_observer)
    model.eval()
    with torch.no_grad():
        ref = model(x).clone()
    assert torch.equal(Int8Student(export_int8(model))(x), ref)
