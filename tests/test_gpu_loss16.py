"""The class-parallel losses on fp16 / bf16 logits on an MI355X (qatvit_kd_ce_loss_rows16 / _topk16, qatvit_kd_bce_loss_topk16 through functional.py)
against a plain fp64 evaluation of the stated formulas on student.double().

Bounds.  out3: every case runs on SEEDS draws of its inputs; the fp32 entry's largest relative error against the fp64 reference over those draws
(measured here, on student.float()), times two, bounds the new entry's error on EVERY draw - only the order of the per-thread sums differs.  (One
draw's fp32 error is a single rounding error and can be 0; the draws of one (dtype, C, form) share its scale.)  dlogits, every element of every
draw: |d - g64 s| <= 2^-11 |g64 s| (fp16) or 2^-8 |g64 s| (bf16), below the normal range half the subnormal spacing, plus s times the fp32 entry's
largest absolute gradient error of that draw.  Every figure is printed before it is asserted (profiles/loss16_errors.txt)."""
import functools

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import functional as F
from qat_vit_amd import native

pytestmark = pytest.mark.gpu

T, ALPHA, EPS = 4.0, 0.5, 0.1
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {"fp16": (2.0 ** -11, 2.0 ** -25), "bf16": (2.0 ** -8, 2.0 ** -134)}   # relative in the normal range, absolute below it
CLASSES = [2, 7, 8, 9, 513, 1000, 1024, 1025, 4097, 8191, 8192, 8193, 32768]      # B = 3: rows 1 and 2 are misaligned where C is odd
FORMS = ["none", "teacher", "table", "table_mix", "topk1", "topk64_mix", "bce_topk_mix", "bce"]
SEEDS = 8
CASES = [(name, C, FORMS[(i + 3 * d) % len(FORMS)]) for d, name in enumerate(DTYPES) for i, C in enumerate(CLASSES)]
MIX = [[1, 0, 0, 0, 0, 0.3], [0, 0, 0, 0, 0, 1.0], [0, 0, 0, 0, 0, 0.75]]          # (partner, lam) of rows 0 .. 2


def mix_records(dev):
    m = torch.tensor(MIX, dtype=torch.float32)
    rec = m.to(torch.int32)
    rec[:, 5] = m[:, 5].contiguous().view(torch.int32)
    return rec.to(dev)


def ref64(x16, labels, rows=None, mix=False, bce=False):
    """(out3 fp64 [3], d loss / d x fp64 [B, C]) of the formulas of include/qatvit.h on x16.double(); rows: the teacher's dense row per sample."""
    x = x16.double().cpu().requires_grad_()
    B, C = x.shape
    y = labels.cpu()
    lam = torch.tensor([r[5] if mix else 1.0 for r in MIX], dtype=torch.float32)
    part = torch.tensor([r[0] if mix and r[5] != 1.0 else b for b, r in enumerate(MIX)])
    oml = (1 - lam).double()[:, None]
    lam = lam.double()[:, None]
    onehot = torch.nn.functional.one_hot(y, C).double()
    t = (1 - EPS) * (lam * onehot + oml * onehot[part]) + EPS / C
    if bce:
        hard = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="sum") / (B * C)
    else:
        hard = -(t * torch.log_softmax(x, 1)).sum(1).mean()
    if rows is None:
        out = torch.stack([hard, hard, torch.zeros((), dtype=torch.float64)])
    else:
        q = torch.softmax(rows.double().cpu() / T, 1)
        q = lam * q + oml * q[part]
        kd = (torch.xlogy(q, q) - q * torch.log_softmax(x / T, 1)).sum(1).mean() * T * T
        out = torch.stack([ALPHA * kd + (1 - ALPHA) * hard, hard, kd])
    out[0].backward()
    return out.detach(), x.grad


@functools.lru_cache(maxsize=None)
def case(name, C, form, seed, scale=None):
    """One draw of a case, evaluated once: the new entry on the 16-bit logits, the fp32 entry on their up-cast, the fp64 reference."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(100000 * seed + 2 * C + len(form))
    x16 = (torch.randn(3, C, generator=g) * 3).to(DTYPES[name]).to(dev)
    y = torch.randint(0, C, (3,), generator=g).to(dev)
    index = torch.tensor([2, 0, 1], device=dev)
    dense = (torch.randn(3, C, generator=g) * 3).to(dev)
    mix = mix_records(dev) if form.endswith("mix") else None
    gs = None if scale is None else torch.full((), float(scale), device=dev)
    topk = F.teacher_topk(dense, min(64 if form == "topk64_mix" else (1 if form == "topk1" else 16), C - 1), T) if "topk" in form else None
    rows = None
    if form == "teacher":
        rows = dense
    elif form in ("table", "table_mix"):
        rows = dense[index]
    elif topk is not None:   # the decompression rule of the header
        rows = topk[2][:, None].expand(3, C).clone().scatter_(1, topk[0].long(), topk[1])[index]

    def run(s, **kw):
        s = s.clone().requires_grad_()
        if form == "none":
            out = F.kd_ce_loss(s, None, y, T, ALPHA, EPS, class_parallel=True, **kw)
        elif form == "teacher":
            out = F.kd_ce_loss(s, dense, y, T, ALPHA, EPS, class_parallel=True, **kw)
        elif form in ("table", "table_mix"):
            out = F.kd_ce_loss_table_mix(s, dense, index, y, mix, T, ALPHA, EPS, class_parallel=True, **kw)
        elif form in ("topk1", "topk64_mix"):
            out = F.kd_ce_loss_topk(s, *topk, index, y, mix, T, ALPHA, EPS, **kw)
        elif form == "bce_topk_mix":
            out = F.kd_bce_loss_topk(s, y, *topk, index, mix, T, ALPHA, EPS, **kw)
        else:
            out = F.kd_bce_loss_topk(s, y, label_smoothing=EPS, **kw)
        out[0].backward(gradient=kw.get("grad_scale"))   # dloss = grad_scale: the factor of backward is exactly 1
        assert s.grad.dtype == s.dtype and out[1].dtype == torch.float32
        return out[1].double().cpu(), s.grad.double().cpu()

    out16, d16 = run(x16, grad_scale=gs)
    out32, d32 = run(x16.float())
    ref, g64 = ref64(x16, y, rows, mix is not None, form.startswith("bce"))
    assert torch.isfinite(ref).all() and torch.isfinite(g64).all()
    rel = lambda o: ((o - ref).abs() / ref.abs().clamp_min(1e-30))[:2 if rows is None else 3].max().item()   # noqa: E731
    return dict(out16=rel(out16), out32=rel(out32), d16=d16, g64=g64, e32=(d32 - g64).abs().max().item(), s=1.0 if scale is None else float(scale))


@pytest.mark.parametrize("name,C,form", CASES + [("fp16", 1000, "table_mix")], ids=lambda v: str(v))
def test_parity_with_fp64(name, C, form):
    scale = 65536.0 if (name, C, form) == ("fp16", 1000, "table_mix") else None
    draws = [case(name, C, form, seed, scale) for seed in range(SEEDS)]
    floor = max(r["out32"] for r in draws)
    rel, sub = HALF_ULP[name]
    over = []
    for r in draws:
        v = r["g64"] * r["s"]
        tol = torch.maximum(rel * v.abs(), torch.full_like(v, sub)) + r["s"] * r["e32"]
        over.append(((r["d16"] - v).abs() - tol).max().item())
    print(f"loss16 {name} C={C} {form} s={draws[0]['s']:g}, {SEEDS} draws: out3 rel err, worst {max(r['out16'] for r in draws):.3e} (fp32 entry: worst "
          f"{floor:.3e}, smallest {min(r['out32'] for r in draws):.3e}); fp32 entry grad abs err, worst {max(r['e32'] for r in draws):.3e}; "
          f"worst (|d - g64 s| - tol) {max(over):.3e} over {SEEDS} x {draws[0]['g64'].numel()} elements")
    assert all(r["out16"] <= 2 * floor for r in draws)
    assert max(over) <= 0


@pytest.mark.parametrize("name,C,form", [("fp16", 9, "table"), ("bf16", 1025, "table"), ("bf16", 9, "topk"), ("fp16", 1025, "topk"),
                                         ("fp16", 9, "bce_topk"), ("bf16", 1025, "bce_topk")])   # every kernel, wave and workgroup form
def test_special_rows_and_repeatability(name, C, form):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(3, C, generator=g) * 3).to(DTYPES[name]).to(dev)
    y = torch.randint(0, C, (3,), generator=g).to(dev)
    table, index = torch.randn(5, C, generator=g).to(dev), torch.tensor([4, 1, 0], device=dev)
    topk = F.teacher_topk(table, 4, T)
    ones = mix_records(dev)
    ones[:, 5] = torch.ones(3).view(torch.int32).to(dev)

    def run(s, index, mix=None):
        s = s.clone().requires_grad_()
        if form == "table":
            out = F.kd_ce_loss_table_mix(s, table, index, y, mix, T, ALPHA, EPS, class_parallel=True)
        elif form == "topk":
            out = F.kd_ce_loss_topk(s, *topk, index, y, mix, T, ALPHA, EPS)
        else:
            out = F.kd_bce_loss_topk(s, y, *topk, index, mix, T, ALPHA, EPS)
        out[0].backward()
        return out[1], s.grad

    out, d = run(x, index)
    assert torch.isfinite(out).all() and torch.isfinite(d).all()
    for other in (run(x, index), run(x, index, ones)):   # the same inputs, and records with lam = 1: the same bits
        assert torch.equal(out, other[0]) and torch.equal(d.view(torch.int16), other[1].view(torch.int16))
    xn = x.clone()
    xn[1, C - 2] = float("nan")
    bad = index.clone()
    bad[1] = 5
    for o, dn in (run(xn, index), run(x, bad)):   # a NaN logit, an index outside the table: that row and out3
        assert torch.isnan(dn[1]).all() and torch.isnan(o).all()
        assert torch.equal(dn[[0, 2]].view(torch.int16), d[[0, 2]].view(torch.int16))
    with pytest.raises(RuntimeError, match="expected float32"):
        F.kd_ce_loss(x, None, y, class_parallel=False)


def test_every_public_route_reaches_the_16_bit_entries():
    """The wrappers only pass on: each gives the bits of the functional form it stands for, loss, out3 and gradient."""
    dev, C = torch.device("cuda"), 5000   # above 4096 classes F.kd_bce_loss / BinaryCrossEntropy take the class-parallel BCE entry
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(3, C, generator=g) * 3).bfloat16().to(dev)
    y = torch.randint(0, C, (3,), generator=g).to(dev)
    dense, index, mix = torch.randn(3, C, generator=g).to(dev), torch.tensor([2, 0, 1], device=dev), mix_records(dev)
    ones = mix.clone()
    ones[:, 5] = torch.ones(3).view(torch.int32).to(dev)
    gs = torch.full((), 256.0, device=dev)
    tab = qat_vit_amd.TeacherLogitTable(dense, {"N": 3, "C": C, "teacher_form": 0, "transform": (), "data_digest": "", "param_digest": ""})
    tk = qat_vit_amd.TeacherTopKTable.from_dense(dense, 16, T)
    kw = dict(kd_temp=T, kd_alpha=ALPHA, label_smoothing=EPS, grad_scale=gs)

    def both(fn):
        s = x.clone().requires_grad_()
        out = fn(s)
        loss, out3 = out if isinstance(out, tuple) else (out, None)
        loss.backward()
        assert s.grad.dtype == torch.bfloat16
        return loss.detach(), out3, s.grad.view(torch.int16)

    def same(a, b, out3=True):
        a, b = both(a), both(b)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and (not out3 or torch.equal(a[1], b[1]))

    same(lambda s: tab.loss(s, index, y, mix=mix, class_parallel=True, **kw), lambda s: F.kd_ce_loss_table_mix(s, dense, index, y, mix, class_parallel=True, **kw))
    same(lambda s: tab.loss(s, index, y, class_parallel=True, **kw), lambda s: F.kd_ce_loss_table_mix(s, dense, index, y, ones, class_parallel=True, **kw))
    same(lambda s: F.kd_ce_loss_table(s, dense, index, y, class_parallel=True, **kw), lambda s: F.kd_ce_loss_table_mix(s, dense, index, y, ones, class_parallel=True, **kw))
    same(lambda s: F.kd_ce_loss(s, dense, y, class_parallel=True, **kw), lambda s: F.kd_ce_loss_mix(s, dense, y, ones, class_parallel=True, **kw))
    same(lambda s: tk.loss(s, index, y, mix=mix, **kw), lambda s: F.kd_ce_loss_topk(s, tk.idx, tk.val, tk.tail, index, y, mix, **kw))
    same(lambda s: tk.bce_loss(s, index, y, mix=mix, **kw), lambda s: F.kd_bce_loss_topk(s, y, tk.idx, tk.val, tk.tail, index, mix, **kw))
    same(lambda s: F.kd_bce_loss(s, y, mix=mix, label_smoothing=EPS, grad_scale=gs), lambda s: F.kd_bce_loss_topk(s, y, mix=mix, label_smoothing=EPS, grad_scale=gs))
    same(lambda s: qat_vit_amd.loss.BinaryCrossEntropy(EPS)(s, y, mix, grad_scale=gs), lambda s: F.kd_bce_loss(s, y, mix=mix, label_smoothing=EPS, grad_scale=gs), out3=False)
    for student, cp in ((x.float(), False), (x.float(), True)):   # a float32 student takes no grad_scale, in either form
        with pytest.raises(RuntimeError, match="grad_scale belongs to a float16 / bfloat16 student"):
            F.kd_ce_loss(student, None, y, class_parallel=cp, grad_scale=gs)


def test_backward_with_grad_scale_is_the_kernels_dlogits():
    dev, C = torch.device("cuda"), 1001
    x = (torch.randn(3, C, generator=torch.Generator().manual_seed(3)) * 3).half().to(dev).requires_grad_()
    y = torch.tensor([5, 1000, 0], device=dev)
    gs = torch.full((), 1024.0, device=dev)
    loss, out3 = F.kd_ce_loss(x, None, y, T, ALPHA, EPS, class_parallel=True, grad_scale=gs)
    (loss * gs).backward()   # what scaler.scale(loss).backward() does
    raw, partials, o = torch.empty_like(x), torch.empty(6, device=dev), torch.empty(3, device=dev)
    native.check(native.lib().qatvit_kd_ce_loss_rows16(x.data_ptr(), 1, None, None, 0, None, y.data_ptr(), None, 3, C, T, ALPHA, EPS, gs.data_ptr(),
                                                       partials.data_ptr(), o.data_ptr(), raw.data_ptr(), native.stream_ptr()), "qatvit_kd_ce_loss_rows16")
    assert x.grad.dtype == torch.float16 and torch.equal(x.grad.view(torch.int16), raw.view(torch.int16)) and torch.equal(o, out3)
