"""The native float student step (all three forms) and the native teacher forward away from the one shape every other test runs (197 tokens,
head_dim 64, 10 classes, batch >= 4), on an MI355X.

1. Whole steps of small models - the smallest shapes that reach each path no other test runs: the 2-key-tile and the head_dim-32 forms of the float
   attention forward, the fused 16-bit attention backward at Tp = 32 / 64 with masked rows, the fp32 attention backward on one ragged 64 x 64 tile, at
   T = 65 and at K = 32, the head kernels at 3 / 7 / 1000 classes, the row kernels at other T, the step's GEMMs at M = 2 / 15 / 130 / 250 rows, K = 3072
   (patch 32) and hidden 768.  Reference: the fp64 copy of the same tree; bounds: those of tests/test_gpu_float_{step,amp,bf16}.py, on the logits as a
   batch AND per image, and on every parameter gradient - once for the whole batch and once with the loss of every image but the last zeroed, so that
   the gradients come from that image's token rows alone (rows 65..129 of 130, rows 200..249 of 250: both straddle a row tile).
2. The fused 16-bit attention backward kernel alone, at the token counts around its 16-row tiles and 32-token padding, inside guarded operands.
3. The teacher forward at the same shapes, per image.
Measured values: profiles/float_step_shapes.txt."""
import copy
import functools

import pytest
import torch

import qat_vit_amd
from qat_vit_amd import native
from qat_vit_amd.float_engine import engine_of, is_native_float
from tests.kernel_check import assert_tiles_close, guarded, guarded_copy, rel_l2_t, tile_errors

pytestmark = pytest.mark.gpu
DEV = "cuda"

# case: (model keywords on top of vit_small_patch16_224_student (embed_dim 384), tokens, batch, classes)
CASES = {
    "A": (dict(img_size=16, num_heads=6, depth=2), 2, 1, 10),                   # M = 2, <64,2>, every tile almost empty
    "B": (dict(img_size=32, num_heads=12, depth=2), 5, 3, 3),                   # <32,2>, fused backward head_dim 32 at Tp = 32, fewer classes than waves
    "C": (dict(img_size=80, num_heads=6, depth=2), 26, 2, 10),                  # the 2-tile form with its second tile part full
    "D": (dict(img_size=96, num_heads=6, depth=2), 37, 2, 10),                  # first reachable T of the 14-tile form; Tp = 64, 27 masked rows
    "E": (dict(img_size=96, num_heads=12, depth=1), 37, 1, 1000),               # <32,14>, more classes than threads, the first block is the last
    "F": (dict(img_size=128, num_heads=6, depth=2, mlp_ratio=2), 65, 2, 10),    # T = 64 + 1, hidden 768, M = 130
    "G": (dict(img_size=224, patch_size=32, num_heads=6, depth=2), 50, 5, 7),   # K = 3072 patch GEMM, M = 250 straddles the 208-row tile
    "H": (dict(img_size=224, num_heads=12, depth=1), 197, 1, 10),               # head_dim 32 through a whole step at full T, M = 197 < 208
    "P": (dict(embed_dim=128, num_heads=4, img_size=32, depth=2), 5, 3, 10),    # N = 128 GEMM tiles with head_dim 32 (fp32 form and teacher only)
}
ISOLATED = "BCDFGP"      # batch > 1: the step again with the loss of the last image only
SEEDS = (2, 3, 4, 5)     # input seeds (same weights): the 16-bit forms' stock error of a tensor is the largest of the four
# form: (native_float's amp, autocast dtype, cap on every tensor, unit roundoff of the type)
FORMS = {"fp32": (False, None, 1e-4, None), "fp16": (True, torch.float16, 1e-2, 2.0 ** -11), "bf16": (torch.bfloat16, torch.bfloat16, 5e-2, 2.0 ** -8)}
BANNED = ("aten::mm", "aten::addmm", "aten::bmm", "aten::matmul", "aten::linear", "aten::conv2d", "aten::convolution", "aten::softmax", "aten::_softmax",
          "aten::layer_norm", "aten::native_layer_norm", "aten::gelu", "scaled_dot_product")


def _student(seed, classes, **kw):
    torch.manual_seed(seed)
    m = qat_vit_amd.create_model("vit_small_patch16_224_student", pretrained=False, num_classes=classes, qat_wrapper=True, **kw)
    with torch.no_grad():   # non-trivial biases / LayerNorm affines / cls token so that every gradient path carries signal
        for n, p in m.named_parameters():
            if n.endswith("bias") or "norm" in n or "cls_token" in n:
                p.add_(0.05 * torch.randn_like(p))
    return m


def _inputs(case, seed):
    kw, _, B, C = CASES[case]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, kw["img_size"], kw["img_size"], generator=g).cuda()
    r = torch.randn(B, C, generator=g).cuda()
    r_last = r.clone()
    r_last[:-1] = 0
    return x, ((("batch", r), ("last image", r_last)) if case in ISOLATED else (("batch", r),))


def _step(m, x, r, dt=None, double=False):
    """One step with the loss (out.float() * r).sum(): (logits, gradients in parameter order)."""
    for p in m.parameters():
        p.grad = None
    if double:
        out = m(x.double())
        (out * r.double()).sum().backward()
    elif dt is None:
        out = m(x)
        (out.float() * r).sum().backward()
    else:
        with torch.autocast("cuda", dtype=dt):
            out = m(x)
        (out.float() * r).sum().backward()
    return out.detach(), [p.grad.detach().clone() for p in m.parameters()], out.grad_fn


@functools.lru_cache(maxsize=None)
def _reference(case):
    """The case's weights (on the CPU) and the fp64 tree's steps on the GPU: {(seed, variant): (logits, gradients)}.  Computed once per case, shared by
    the three forms, never modified."""
    kw, T, B, C = CASES[case]
    base = _student(1, C, **kw)
    assert base.model.patch_embed.num_patches + 1 == T
    ref = copy.deepcopy(base).double().cuda().train()
    steps = {}
    for seed in SEEDS:
        x, variants = _inputs(case, seed)
        for variant, r in variants:
            steps[seed, variant] = _step(ref, x, r, double=True)[:2]
    return base, steps


def _errors(out, grads, ref_out, ref_grads, names):
    """Relative L2 against fp64 of: the logits as a batch, each image's logits, every parameter gradient - {name: (error, numel)}."""
    e = {"logits": (rel_l2_t(out, ref_out), out.numel())}
    for i in range(out.shape[0]):
        e[f"logits[{i}]"] = (rel_l2_t(out[i], ref_out[i]), out[i].numel())
    for n, a, b in zip(names, grads, ref_grads):
        e[n] = (rel_l2_t(a, b), a.numel())
    return e


def _assert_ran_natively(prof, m, form, B, steps):
    """As test_*_runs_only_native_kernels: no stock GEMM / attention / norm op, only this library's kernels - and the engine of the form took every step."""
    names = {e.name for e in prof.events()}
    hit = sorted(n for n in names if any(n.startswith(b) or b in n for b in BANNED))
    assert not hit, hit
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("qv::" in k or "_ZN2qv" in k for k in kernels), kernels
    # (stock kernels of the loss itself, (out.float() * r).sum(), and of clearing / cloning gradients: casts, products, one reduction, fills, copies)
    other = sorted(k for k in kernels if "qv::" not in k and "_ZN2qv" not in k
                   and not any(s in k.lower() for s in ("fill", "copy", "memset", "memcpy", "elementwise", "reduce_kernel")))
    assert not other, other
    if form != "fp32":
        assert any("k_fa_attn_bwd_fused" in k for k in kernels), kernels
    else:
        assert any("k_fs_attn_gemm" in k for k in kernels), kernels
    eng = engine_of(m)
    assert is_native_float(m) and eng is not None and eng.generation == steps
    f = {"fp32": eng.fp32, "fp16": eng.fp16, "bf16": eng.bf16}[form]
    assert f.capacity == B and all(o.capacity == 0 for o in (eng.fp32, eng.fp16, eng.bf16) if o is not f)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", list(CASES))
def test_step_parity_with_fp64_tree(case, form):
    from torch.profiler import ProfilerActivity, profile

    kw, T, B, C = CASES[case]
    amp, dt, cap, unit = FORMS[form]
    base, ref_steps = _reference(case)
    if case == "P" and form != "fp32":   # embed_dim 128: the 16-bit forms run on 384-wide tiles only and must say so
        with pytest.raises(RuntimeError, match="multiples of 384"):
            qat_vit_amd.native_float(copy.deepcopy(base).cuda().train(), amp=amp)
        return
    m = qat_vit_amd.native_float(copy.deepcopy(base).cuda().train(), amp=amp)
    stock = copy.deepcopy(base).cuda().train() if dt is not None else None
    names = [n for n, _ in m.named_parameters()]
    nat, sto, n_steps = {}, {}, 0
    for seed in SEEDS if dt is not None else SEEDS[:1]:
        x, variants = _inputs(case, seed)
        for variant, r in variants:
            last = seed == (SEEDS[-1] if dt is not None else SEEDS[0]) and variant == variants[-1][0]
            if last:    # the last native step under the profiler
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    out, grads, fn = _step(m, x, r, dt)
                    torch.cuda.synchronize()
            else:
                out, grads, fn = _step(m, x, r, dt)
            n_steps += 1
            assert type(fn).__name__ == ("_FloatStudentStepBackward" if dt is None else "_FloatStudentAmpStepBackward"), fn
            assert out.shape == (B, C) and out.dtype == (dt or torch.float32)
            assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads), (seed, variant)
            nat[seed, variant] = _errors(out, grads, *ref_steps[seed, variant], names)
            if stock is not None:
                out_s, grads_s, _ = _step(stock, x, r, dt)
                assert out_s.dtype == dt
                sto[seed, variant] = _errors(out_s, grads_s, *ref_steps[seed, variant], names)
    _assert_ran_natively(prof, m, form, B, n_steps)
    bad = []
    for variant in dict.fromkeys(v for _, v in nat):
        runs = [nat[k] for k in nat if k[1] == variant]
        floor = {t: (max(sto[k][t][0] for k in sto if k[1] == variant) if sto else 0.0) for t in runs[0]}
        worst = {t: max(run[t][0] for run in runs) for t in runs[0]}
        for t, a in worst.items():
            if dt is None:
                bound = 1e-4
            else:   # within twice stock autocast (the largest of its four samples) and inside the form's cap; a tensor of a few elements: four roundoffs
                bound = min(max(2 * floor[t], 1e-4, 4 * unit if runs[0][t][1] < 256 else 0.0), cap)
            if not a <= bound:
                bad.append((variant, t, a, floor[t], bound))
        imgs, prm = [t for t in worst if t.startswith("logits[")], [t for t in worst if not t.startswith("logits")]
        wi, wp = max(imgs, key=worst.get), max(prm, key=worst.get)
        st = (lambda t: f" (stock {floor[t]:.2e})") if sto else (lambda t: "")
        print(f"SHAPE {case} {form} {variant}: logits {worst['logits']:.2e}{st('logits')} worst image {wi} {worst[wi]:.2e}{st(wi)} "
              f"worst parameter {wp} {worst[wp]:.2e}{st(wp)}")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- the fused 16-bit attention backward
ATTN_T = (1, 2, 15, 16, 17, 32, 33, 64, 65, 224)
ATTN_FORMS = {"fp16": (torch.float16, "qatvit_float_student_amp_attn_backward", 3e-3), "bf16": (torch.bfloat16, "qatvit_float_student_bf16_attn_backward", 2.5e-2)}


@pytest.mark.parametrize("T", ATTN_T)
@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("form", list(ATTN_FORMS))
def test_attention_backward_kernel_token_edges(form, hd, T):
    """k_fa_attn_bwd_fused at one token, below / at / one past its 16-row tiles and its 32-token padding, and at 224 tokens (nothing masked), two images of
    6 / 12 heads (both strides matter), every operand inside poisoned padding and the output inside a canary: against the fp64 restatement of
    test_attention_backward_kernel_against_fp64 at that test's bound, whole tensor and per 16 x 16 tile.  One token: the reference dQ and dK are exactly zero
    (softmax of one score is the constant 1); what a correct kernel leaves there is dS = P (round(dP) - delta), the rounding of dP - bounded by twice the
    worst tile of a torch emulation with the kernel's rounding points (dP, P and dS rounded to the 16-bit type, delta from the rounded operands).  The same
    emulation is printed next to the kernel at every T.  (At T = 2, dS = P0 P1 (dP0 - dP1): a saturated softmax row leaves the rounding of dP only.  Over the
    24 / 48 rows here the worst tile is half the bar; over 8 rows (two heads) a kernel equal to its emulation was measured past it -
    profiles/float_step_shapes.txt.)"""
    E, fn, tol = ATTN_FORMS[form]
    B, H = 2, 6 if hd == 64 else 12     # (embed_dim 384, the heads of that test)
    D = H * hd
    g = torch.Generator().manual_seed(1000 * hd + T)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).cuda()
    dO = (torch.randn(B * T, D, generator=g) * 1e-2).cuda()
    q, k, v = qkv.to(E).double().view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    do = dO.to(E).double().view(B, T, H, hd).transpose(1, 2)
    s = hd ** -0.5
    S = s * q @ k.transpose(-1, -2)
    lse = torch.logsumexp(S, -1)                       # [B, H, T]
    P = torch.exp(S - lse[..., None])
    O = P @ v
    dV = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - (do * O).sum(-1, keepdim=True))
    dQ, dK = s * dS @ k, s * dS.transpose(-1, -2) @ q
    if T == 1:   # P = 1 and dP = delta exactly; fp64 leaves the two sums' last bits
        assert max(dQ.abs().max().item(), dK.abs().max().item()) < 1e-15
        dQ, dK = torch.zeros_like(dQ), torch.zeros_like(dK)
    O16 = O.transpose(1, 2).reshape(B * T, D).to(E).contiguous()
    checks = []

    def inp(t):
        t, c = guarded_copy(t)
        checks.append(c)
        return t

    qkv_g, O16_g, dO_g, lse_g = inp(qkv), inp(O16), inp(dO), inp(lse.float().contiguous())
    dqkv, canary = guarded(B * T, 3 * D, E, DEV)
    native.check(getattr(native.lib(), fn)(qkv_g.data_ptr(), O16_g.data_ptr(), lse_g.data_ptr(), dO_g.data_ptr(), B, T, H, D, dqkv.data_ptr(), native.stream_ptr()), fn)
    torch.cuda.synchronize()
    canary(f"{fn} dqkv")
    for c in checks:
        c(fn)
    assert torch.isfinite(dqkv).all()     # (an element the kernel did not store is still the canary's NaN)
    layout = lambda a, b, c: torch.stack((a, b, c)).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * D)   # noqa: E731  the qkv layout of the output
    want = layout(dQ, dK, dV)
    # the kernel's rounding points in stock torch (the comment above k_fa_attn_bwd_fused): the bound at one token, a printed figure next to the kernel's elsewhere
    Pe = torch.exp(S.float() - lse.float()[..., None])
    delta = (do.float() * O16.view(B, T, H, hd).transpose(1, 2).float()).sum(-1, keepdim=True)
    dSe = (Pe * (dP.to(E).float() - delta)).to(E).double()
    emu = layout((s * dSe @ k).to(E).double(), (s * dSe.transpose(-1, -2) @ q).to(E).double(), (Pe.to(E).double().transpose(-1, -2) @ do).to(E).double())
    for name, c0 in (("dQ", 0), ("dK", D), ("dV", 2 * D)):
        got, ref = dqkv[:, c0:c0 + D], want[:, c0:c0 + D]
        what = f"attn_bwd {form} hd{hd} T{T} {name}"
        e_worst = tile_errors(emu[:, c0:c0 + D], ref)[1]
        print(f"EMU {what}: emulation worst_tile {e_worst:.3e} whole {rel_l2_t(emu[:, c0:c0 + D], ref):.3e}; kernel against the emulation "
              f"{rel_l2_t(got, emu[:, c0:c0 + D]):.3e}" + (" (absolute: the reference is zero)" if T == 1 and name != "dV" else ""))
        if T == 1 and name != "dV":
            assert e_worst > 0.0
            assert_tiles_close(got, ref, 2 * e_worst, what=what)
            continue
        assert_tiles_close(got, ref, tol, what=what)
        assert rel_l2_t(got, ref) <= tol, (what, rel_l2_t(got, ref))


# ---------------------------------------------------------------------------------------------------------------- the teacher forward
@pytest.mark.parametrize("passes", [3, 2])
@pytest.mark.parametrize("case", ["B", "D", "E", "G", "H", "P"])
def test_native_teacher_forward_at_these_shapes(monkeypatch, case, passes):
    """test_native_teacher_forward_vs_fp64 at the shapes above: its batch bound on the batch and its per-image bound on every image."""
    from qat_vit_amd.teacher import _ENGINES as T_ENGINES
    from tests.test_gpu_step import TEACHER_TOL

    monkeypatch.setenv("QATVIT_TEACHER_PASSES", str(passes))
    tol, tol_img = TEACHER_TOL[passes]
    kw, T, B, C = CASES[case]
    torch.manual_seed(ord(case))
    m = qat_vit_amd.create_model("vit_small_patch16_224_student", pretrained=False, num_classes=C, **kw).cuda().eval()
    with torch.no_grad():
        for p in m.parameters():          # the init leaves biases at zero: make the test vector non-degenerate
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
        m.cls_token.normal_(std=0.02)
    x = torch.randn(B, 3, kw["img_size"], kw["img_size"], device=DEV)
    with torch.no_grad():
        out = m(x)                        # native (eval + no_grad + CUDA)
    # (embed_dim 128 has no fp16 form: the engine runs it in the three-pass form whatever is asked, and is held to the bound of the form asked for)
    assert m in T_ENGINES and T_ENGINES[m].passes == (3 if case == "P" else passes)
    assert out.shape == (B, C) and torch.isfinite(out).all()
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        ref = m64.head(m64.forward_features(x.double())[:, 0])
    whole, per = rel_l2_t(out, ref), [rel_l2_t(out[i], ref[i]) for i in range(B)]
    print(f"TEACHER {case} passes {passes}: batch {whole:.2e} (bound {tol:.1e}) worst image [{per.index(max(per))}] {max(per):.2e} (bound {tol_img:.1e})")
    assert whole < tol, whole
    assert max(per) < tol_img, per
