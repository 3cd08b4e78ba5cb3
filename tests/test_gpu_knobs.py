"""Every QATVIT_* A/B knob of the engine still runs, and the forms documented as "the same bits" are the same bits: one training step of a ViT-S-width
depth-2 student per knob, each in its own process (the knobs are read once per process), against the default configuration."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# knob -> how its step relates to the default one: "bits" = every output bit-identical (gradients that go through fp32 atomics - biases, LayerNorm
# affine parameters, cls / pos - are compared to 1e-5 instead), float tolerance otherwise
KNOBS = {
    "QATVIT_FC2_CODES=0": "bits",          # fc2 forward from the fp16 planes instead of codes + table
    "QATVIT_FC1_BITS=0": "bits",           # uint16 code plane instead of byte plane + mask bits
    "QATVIT_FC2W_CODES=0": "bits",         # fc2 weight gradient from the bf16 planes
    "QATVIT_QKV_2PASS=0": "bits",          # qkv GEMM once, fp32 output, attention quantises on load
    "QATVIT_F16_STRIP=0": "bits",          # fc2 dgrad + GELU backward of the one-plane backward on the general tall tile (epilogue 19) instead of the A-stationary strip kernel
    "QATVIT_DY16_MIRROR=0": "bits",        # the overflow flag read behind a stream synchronisation instead of from the pinned mirror the backward writes before its weight gradients
    "QATVIT_QP_LATE=0": "bits",            # a k_qparams launch behind every producer of statistics instead of the update inside the consumer kernel (72 launches per step)
    "QATVIT_I8_STRIP=0": "bits",           # the two-pass K = 384 GEMMs (qkv, fc1) on the general tall tile instead of the A-stationary strip kernel
    "QATVIT_I8=0": "bits",                 # grid x grid GEMMs on bf16 MFMA
    # float tolerance: (logits relative L2, worst parameter-gradient relative L2).  LNB_FUSE only reorders two fp32 sums.  The other two change a
    # forward float operand by <= 2^-17 per element, which on this depth-2 step flips a handful of codes by one step (measured 1.6e-2 .. 4.6e-2 on
    # the logits, 1e-2 .. 2.4e-2 on the gradients): at network level they can only be bounded at flip level, so the gradient DIRECTION is asserted
    # next to it, and the bf16-pair forward is checked tensor by tensor in test_stage_parity_under_f16_knob below.
    # the one-plane qkv / fc1 / fc2 weight gradients from the fp16 X plane / the expand-through-LDS kernel instead of k_gemm_tn_q8: the same products
    # (the X integers are exact either way), token splits of 64-token instead of 32-token steps - another fp32 summation order (measured 4e-8)
    "QATVIT_TN_Q8=0": (1e-9, 1e-6),
    # the one-plane weight gradients as one launch (+ reduction) per GEMM right where the reference computes them instead of one persistent stream-K launch per X form
    # at the end of the backward call: the same products, accumulated over the whole token range in registers instead of 21 - 85 partial tiles
    "QATVIT_TN_STREAM=0": (1e-9, 1e-6),
    "QATVIT_LNB_FUSE=0": (1e-6, 5e-6),      # LayerNorm backward as its own kernel (another summation order for dgamma / dbeta)
    # the two-kernel attention backward (k_attn_bwd_dq + k_attn_bwd_dkv) instead of the fused one: the same forward bit for bit (logits: 0), the same
    # products in the backward with delta = rowsum(dO . O) summed in another order
    # (measured 5.0e-6 on the worst parameter, a bias whose gradient is a near-cancelling sum)
    "QATVIT_ATTN_BWD_FUSED=0": (1e-9, 3e-5),
    "QATVIT_ATTN_CODES=0": (1e-9, 3e-5),    # attention backward re-quantises the fp32 qkv (implies the one-pass qkv GEMM and the two-kernel backward)
    # the backward's arithmetic forms (round 4): the default one-plane form against the bf16-pair form (every dY 2^-12 instead of 2^-17 per element:
    # 1e-3 per gradient tensor is the bar of tests/test_gpu_dy16.py; this depth-2 step stays far below it).  The forward is the same bit for bit (logits: 0).
    "QATVIT_DY16=0": "bits",
    "QATVIT_F16=0": (0.1, 0.06),            # bf16 pairs for the forward float operands (2^-17 instead of 2^-23: one-step flips possible)
}
ATOMIC = ("bias", "norm", "cls_token", "pos_embed")
ONE_PLANE_FORMS = ("QATVIT_DY16=0",)   # step 1 (calibration = the pair form) is bit-identical under it; step 2 differs at 2^-12 per element


def run(tmp_path, tag, env_kv, backend):
    out = tmp_path / f"{tag}.pt"
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("QATVIT_"):
            del env[k]
    if env_kv:
        k, v = env_kv.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "knob_worker.py"), str(out), backend], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (env_kv, r.stderr[-1500:])
    return torch.load(out, weights_only=False)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_knob_forms_match_the_default(native_lib, tmp_path, backend):
    ref = run(tmp_path, "default", None, backend)
    again = run(tmp_path, "default2", None, backend)
    assert ref["one_plane"], "the default second step is the one-plane backward"
    bad, measured = [], {}
    for step in (1, 2):
        assert torch.equal(ref[step]["logits"], again[step]["logits"])                      # the step itself is reproducible across processes
    for kv, how in KNOBS.items():
        got_all = run(tmp_path, kv.replace("=", "_"), kv, backend)
        for step in (1, 2):
            got, rf = got_all[step], ref[step]
            # a knob that leaves the one-plane form (or changes its arithmetic) is compared with the default's second step at the one-plane bar
            form_change = step == 2 and (kv in ONE_PLANE_FORMS or not got_all["one_plane"])
            if how == "bits" and not form_change:
                if not torch.equal(got["logits"], rf["logits"]) or not torch.equal(got["loss"], rf["loss"]):
                    bad.append((kv, step, "logits / loss differ", rel(got["logits"], rf["logits"])))
                for n, (s, z, mn, mx) in rf["fq"].items():
                    gs, gz, gmn, gmx = got["fq"][n]
                    if not (torch.equal(s, gs) and torch.equal(z, gz) and torch.equal(mn, gmn) and torch.equal(mx, gmx)):
                        bad.append((kv, step, "fake-quant state differs", n))
                        break
                for n, g in rf["grads"].items():
                    if any(t in n for t in ATOMIC):
                        if rel(got["grads"][n], g) > 1e-5:
                            bad.append((kv, step, "gradient (atomics) differs", n, rel(got["grads"][n], g)))
                    elif not torch.equal(got["grads"][n], g):
                        bad.append((kv, step, "gradient differs", n, rel(got["grads"][n], g)))
            else:
                tol_logits, tol_grads = (1e-9, 0.0) if how == "bits" else how
                if form_change:
                    tol_grads = max(tol_grads, 1e-3)
                m = (rel(got["logits"], rf["logits"]), max(rel(got["grads"][n], g) for n, g in rf["grads"].items()))
                measured[(kv, step)] = m
                if m[0] > tol_logits:
                    bad.append((kv, step, "logits", m[0]))
                if m[1] > tol_grads:
                    bad.append((kv, step, "gradients", m[1]))
                ga = torch.cat([got["grads"][n].double().flatten() for n in rf["grads"]])
                gb = torch.cat([g.double().flatten() for g in rf["grads"].values()])
                cosv = (ga @ gb / (ga.norm() * gb.norm())).item()
                if cosv < 0.999:
                    bad.append((kv, step, "gradient cosine", cosv))
    print("float-tolerance knobs (logits rel L2, worst gradient rel L2):", measured)
    assert not bad, bad


@pytest.mark.timeout(900)
def test_stage_parity_under_f16_knob(native_lib):
    """QATVIT_F16=0 (bf16 pairs as the float operands of the proj / fc2 FORWARD GEMMs) through the teacher-forced stage harness: every tensor of every
    stage within the fine table's limits (codes: < 1e-4 differing, one step; rel L2 <= 1e-3) - the check the network-level bound above cannot give."""
    env = dict(os.environ, QATVIT_F16="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_stage_parity.py"), "-q", "-m", "gpu", "-x", "-k", "c1_qnnpack"],
                       env=env, capture_output=True, text=True, timeout=850, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
