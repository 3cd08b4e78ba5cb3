"""norm1 / norm2 apply + quantise inside the statistics pass of qkv / fc1 (csrc/i8strip.hip, k_i8_strip<3, .., LN = true>; QATVIT_LN_STRIP): the same bits as the
LayerNorm launch followed by the statistics pass on its plane - at kernel level (plane, statistics, guard band) and over two whole training steps."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _fresh(dev):
    return torch.tensor([0xFF800000 - (1 << 32), 0x007FFFFF], dtype=torch.int32, device=dev)


# M: whole strips (208 k; K = 768: 112 k), ragged last strips - 788 = 4 x 197 is the knob worker's M - and a single partial strip
@pytest.mark.parametrize("per_channel", [0, 1])
@pytest.mark.parametrize("qrange", [(0, 255, 131, 128), (0, 127, 66, 64)])   # (qmin, qmax, zero point, center): the qnnpack and the x86 activation ranges
@pytest.mark.parametrize("M,N,K", [(208, 1152, 384), (208 * 3, 1536, 384), (788, 1152, 384), (788, 1536, 384), (1000, 1536, 384), (50, 1152, 384), (256 * 197, 1152, 384),
                                   (112 * 2, 2304, 768), (788, 3072, 768), (300, 2304, 768)])
def test_ln_strip_kernel_equals_ln_apply_then_statistics_pass(native_lib, M, N, K, per_channel, qrange):
    """qatvit_i8_strip_ln on random rows against qatvit_ln_apply_quant8 + qatvit_i8_strip(mode 3): the int8 plane is the one the LayerNorm kernel writes, the statistics
    accumulator the one the int8-plane statistics pass leaves, and a guard band behind row M of the plane (one whole strip of rows) keeps its fill."""
    torch.manual_seed(M + N + per_channel)
    dev = "cuda"
    qmin, qmax, zp, center = qrange
    x = torch.randn(M, K, device=dev) * (torch.rand(M, 1, device=dev) * 3 + 0.2) + torch.randn(M, 1, device=dev)
    mean = x.mean(1).contiguous()
    rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-6).contiguous()
    gamma = (torch.randn(K, device=dev) * 0.3 + 1.0).contiguous()
    beta = (torch.randn(K, device=dev) * 0.2).contiguous()
    scale = 0.0173 * 255 / (qmax - qmin)   # ~ +-2.2 around the zero point: some percent of the elements clip at either end
    aqp = torch.tensor([scale, 1 / scale, float(zp), 1.0], device=dev)
    W = torch.randint(-128, 128, (N, K), device=dev)
    B8 = W.to(torch.int8)
    B8f = torch.empty_like(B8)
    assert native_lib.qatvit_w8_fragment_order(B8.data_ptr(), B8f.data_ptr(), N, K, _st()) == 0, native_lib.qatvit_last_error()
    wsum = W.sum(1).to(torch.int32)
    s1 = aqp[:1].clone()
    s2 = torch.tensor([0.0041], device=dev)
    cs = (torch.rand(N, device=dev) * 0.01 + 0.001) if per_channel else None
    bias = torch.randn(N, device=dev)
    s2p, csp = (None, cs.data_ptr()) if per_channel else (s2.data_ptr(), None)
    guard = 224                          # rows behind M: more than the rows a ragged last strip holds past M
    FILL = 0x5A

    # reference: the LayerNorm launch, then the statistics pass on its plane
    ref8 = torch.full((M + guard, K), FILL, dtype=torch.int8, device=dev)
    assert native_lib.qatvit_ln_apply_quant8(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), aqp.data_ptr(), qmin, qmax,
                                             ref8.data_ptr(), center, M, K, _st()) == 0, native_lib.qatvit_last_error()
    st_ref = _fresh(dev)
    assert native_lib.qatvit_i8_strip(3, ref8.data_ptr(), B8f.data_ptr(), wsum.data_ptr(), aqp.data_ptr(), center, M, N, K, K, s1.data_ptr(), s2p, csp, bias.data_ptr(),
                                      st_ref.data_ptr(), None, qmin, qmax, None, None, 0, None, None, None, _st()) == 0, native_lib.qatvit_last_error()
    # fused
    out8 = torch.full((M + guard, K), FILL, dtype=torch.int8, device=dev)
    st_ln = _fresh(dev)
    assert native_lib.qatvit_i8_strip_ln(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), qmin, qmax, out8.data_ptr(), B8f.data_ptr(),
                                         wsum.data_ptr(), aqp.data_ptr(), center, M, N, K, K, s2p, csp, bias.data_ptr(), st_ln.data_ptr(), _st()) == 0, \
        native_lib.qatvit_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ref8[M:], torch.full_like(ref8[M:], FILL))
    assert torch.equal(out8[M:], torch.full_like(out8[M:], FILL)), "rows behind M of the plane were written"
    assert torch.equal(out8[:M], ref8[:M])
    codes = ref8[:M].int() + center
    clipped = ((codes == qmin) | (codes == qmax)).float().mean().item()
    assert 0.001 < clipped < 0.5, clipped    # the clamp is exercised
    assert torch.equal(st_ln, st_ref)
    assert st_ln[0].item() != _fresh(dev)[0].item() and st_ln[1].item() != _fresh(dev)[1].item()


def test_ln_strip_rejects_what_it_does_not_cover(native_lib):
    """N spread over several workgroups per strip (K = 384, N = 2304) would let two workgroups write one plane: the launcher refuses, nothing is launched."""
    z = torch.zeros(16, device="cuda")
    assert native_lib.qatvit_i8_strip_ln(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 255, z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                         z.data_ptr(), 128, 208, 2304, 384, 384, None, None, None, z.data_ptr(), _st()) != 0
    assert b"unsupported" in native_lib.qatvit_last_error()


ATOMIC = ("bias", "norm", "cls_token", "pos_embed")   # parameters whose gradients are accumulated with fp32 atomics (as in test_gpu_knobs.py)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _worker(tmp_path, tag, env_kv, backend):
    out = tmp_path / f"{tag}.pt"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QATVIT_")}
    if env_kv:
        k, v = env_kv.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "knob_worker.py"), str(out), backend], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (env_kv, r.stderr[-1500:])
    return torch.load(out, weights_only=False)


_FORM_PROBE = """
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from qat_vit_amd import native
c = native.Cfg(batch=4, img_size=224, patch_size=16, in_chans=3, embed_dim=384, depth=2, num_heads=6, mlp_hidden=1536, num_classes=10, act_qmin=0, act_qmax=int(sys.argv[2]),
               w_qmin=-128, w_qmax=127, w_per_channel=int(sys.argv[3]), averaging_const=0.01, ln_eps=1e-6)
L = native.lib()
print("forms", L.qatvit_student_ln_in_strip(ctypes.byref(c), 2), L.qatvit_student_ln_in_strip(ctypes.byref(c), 0))
"""


@pytest.mark.timeout(900)
@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_step_with_ln_in_strip_is_bit_identical_to_two_launches(native_lib, tmp_path, backend):
    """Two training steps of the knob worker (ViT-S width, depth 2, batch 4: M = 788, a ragged fourth strip) with QATVIT_LN_STRIP=0 and with the default: logits, loss, every
    parameter gradient and every quantizer's scale / zero_point / min_val / max_val are torch.equal in both steps (the gradients summed with fp32 atomics: see
    below).  The default arm ran the fused form in its
    second step (the one-plane step, whose forward writes the byte plane only) - the engine's decision function says so for that configuration in a process
    with the same environment, and says no under the knob."""
    import qat_vit_amd
    from qat_vit_amd.engine import engine_of
    from tests.util import prepare

    ref = _worker(tmp_path, "two_launches", "QATVIT_LN_STRIP=0", backend)
    got = _worker(tmp_path, "default", None, backend)
    assert ref["one_plane"] and got["one_plane"]
    act_qmax, per_channel = (255, 0) if backend == "qnnpack" else (127, 1)
    for env_kv, want in ((None, "forms 3 0"), ("QATVIT_LN_STRIP=0", "forms 0 0"), ("QATVIT_QP_LATE=0", "forms 0 0"), ("QATVIT_I8_STRIP=0", "forms 0 0")):
        env = {k: v for k, v in os.environ.items() if not k.startswith("QATVIT_")}
        if env_kv:
            env[env_kv.split("=")[0]] = env_kv.split("=")[1]
        r = subprocess.run([sys.executable, "-c", _FORM_PROBE, ROOT, str(act_qmax), str(per_channel)], env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == want, (env_kv, r.stdout, r.stderr[-800:])
    # ... and an engine in this process (default knobs unless the caller's environment says otherwise) reports what its own forwards ran
    if not any(k.startswith("QATVIT_") for k in os.environ):
        torch.manual_seed(3)
        stu = qat_vit_amd.create_student("vit", num_classes=10, qat_wrapper=True, embed_dim=384, depth=2, num_heads=6, img_size=224)
        p = prepare(stu.cuda(), backend)
        cfgq = None
        x = torch.randn(4, 3, 224, 224, device="cuda")
        seen = []
        for _ in range(2):
            p(x).sum().backward()
            torch.cuda.synchronize()
            e = engine_of(p)
            seen.append((bool(e._fwd_x16), e.ln_in_strip))
            cfgq = (e.cfg.act_qmax, e.cfg.w_per_channel)
        assert seen == [(False, 0), (True, 3)], seen
        assert cfgq == (act_qmax, per_channel), cfgq    # the probe above asked about the worker's configuration
    # Gradients that are summed with fp32 atomics (biases, LayerNorm affine parameters, cls / pos: ATOMIC in test_gpu_knobs.py) do not repeat bit for bit between two
    # runs of ONE arm - measured below, two-launch arm against itself: 1e-8 .. 5e-8 relative on about a dozen of them per run pair (which ones changes from pair to
    # pair), already in step 1, where neither arm runs the fused form.  torch.equal cannot be asked of them; they are held to 1e-5 relative, the bar
    # test_gpu_knobs.py sets for these parameters under every "bits" knob, and the same-arm figures are printed next to the cross-arm ones.  Everything else -
    # logits, loss, quantizer state, every weight gradient - is torch.equal.
    ref2 = _worker(tmp_path, "two_launches_again", "QATVIT_LN_STRIP=0", backend)
    bad, loose = [], {}
    for step in (1, 2):
        g, r, r2 = got[step], ref[step], ref2[step]
        if not torch.equal(g["logits"], r["logits"]) or not torch.equal(g["loss"], r["loss"]):
            bad.append((step, "logits / loss"))
        for n, (s, z, mn, mx) in r["fq"].items():
            gs, gz, gmn, gmx = g["fq"][n]
            if not (torch.equal(s, gs) and torch.equal(z, gz) and torch.equal(mn, gmn) and torch.equal(mx, gmx)):
                bad.append((step, "fake-quant state", n))
        assert set(g["grads"]) == set(r["grads"])
        for n, gr in r["grads"].items():
            if torch.equal(g["grads"][n], gr):
                continue
            d = _rel(g["grads"][n], gr)
            if any(t in n for t in ATOMIC):
                loose[(step, n)] = d
                if d > 1e-5:
                    bad.append((step, "gradient (atomics)", n, d))
            else:
                bad.append((step, "gradient", n, d))
        same_arm = {n: _rel(r2["grads"][n], gr) for n, gr in r["grads"].items() if not torch.equal(r2["grads"][n], gr)}
        assert all(any(t in n for t in ATOMIC) for n in same_arm), same_arm    # within one arm only the atomically summed gradients move
        print(f"step {step}: two-launch arm against itself, gradients that differ:", same_arm)
    print("fused arm against the two-launch arm, atomically summed gradients that differ:", loose)
    assert not bad, bad
