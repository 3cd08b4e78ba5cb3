"""The one-plane backward of the last block on the class-token rows (QATVIT_CLS_BWD): the student pools the class token, so the gradient
entering the last block is zero outside the B rows b * T; its MLP and proj backward run on those B rows of gathered operands.  A zero row of a dgrad operand
gives a zero output row and adds exact zeros to a weight gradient, so against QATVIT_CLS_BWD=0 (all B * T rows) only the grouping of fp32 sums changes."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

# the bounds tests/test_gpu_knobs.py sets for a re-grouped fp32 sum: the weight gradients as under QATVIT_TN_STREAM=0, and the gradients that go through
# fp32 atomics (its ATOMIC list: they do not repeat bit for bit between two runs of one build either - tests/test_gpu_ln_strip.py measures 1e-8 .. 5e-8)
from tests.test_gpu_knobs import ATOMIC, KNOBS  # noqa: E402

TOL_REGROUPED = KNOBS["QATVIT_TN_STREAM=0"][1]   # 1e-6 relative L2 per parameter
TOL_ATOMIC = 1e-5


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _worker(tmp_path, tag, env_kv, backend, batch=None, staged=False):
    out = tmp_path / f"{tag}.pt"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QATVIT_")}
    if env_kv:
        k, v = env_kv.split("=")
        env[k] = v
    cmd = [sys.executable, os.path.join(ROOT, "tests", "knob_worker.py"), str(out), backend]
    if batch is not None:
        cmd = [sys.executable, os.path.join(ROOT, "tests", "cls_bwd_worker.py"), str(out), backend, str(batch)] + (["staged"] if staged else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (env_kv, r.stderr[-1500:])
    return torch.load(out, weights_only=False)


def _compare(got, ref, what):
    """Both steps of a worker pair: forward and step 1 (the pair form) identical, step 2's gradients within the bounds of a re-grouped fp32 sum."""
    assert got["one_plane"] and ref["one_plane"], "the second step of both arms is the one-plane backward"
    bad, worst = [], {"weights": (0.0, None), "atomics": (0.0, None)}
    for step in (1, 2):
        g, r = got[step], ref[step]
        if not torch.equal(g["logits"], r["logits"]) or not torch.equal(g["loss"], r["loss"]):
            bad.append((step, "logits / loss"))
        for n, (s, z, mn, mx) in r["fq"].items():
            gs, gz, gmn, gmx = g["fq"][n]
            if not (torch.equal(s, gs) and torch.equal(z, gz) and torch.equal(mn, gmn) and torch.equal(mx, gmx)):
                bad.append((step, "fake-quant state", n))
        assert set(g["grads"]) == set(r["grads"])
        for n, gr in r["grads"].items():
            atomic = any(t in n for t in ATOMIC)
            d = _rel(g["grads"][n], gr)
            if step == 2:
                key = "atomics" if atomic else "weights"
                if d > worst[key][0]:
                    worst[key] = (d, n)
            if atomic:   # (step 1 too: see above)
                if d > TOL_ATOMIC:
                    bad.append((step, "gradient (atomics)", n, d))
            elif step == 1:
                if not torch.equal(g["grads"][n], gr):
                    bad.append((step, "gradient of the pair form differs", n, d))
            elif d > TOL_REGROUPED:
                bad.append((step, "gradient", n, d))
    print(f"CLS_BWD {what}: step 2 worst relative L2 against QATVIT_CLS_BWD=0: weights {worst['weights'][0]:.3e} ({worst['weights'][1]}), "
          f"atomically summed {worst['atomics'][0]:.3e} ({worst['atomics'][1]})")
    assert not bad, bad


@pytest.mark.timeout(600)
@pytest.mark.parametrize("backend", ["qnnpack", "x86"])
def test_step_on_cls_rows_matches_all_rows(native_lib, tmp_path, backend):
    """tests/knob_worker.py (ViT-S width, depth 2, batch 4, two steps) with the default and with QATVIT_CLS_BWD=0.  Measured worst values:
    profiles/cls_bwd_bench.txt."""
    _compare(_worker(tmp_path, "rows", None, backend), _worker(tmp_path, "dense", "QATVIT_CLS_BWD=0", backend), f"batch 4 {backend}")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("batch,backend", [(3, "qnnpack"), (1, "x86")])
def test_step_on_cls_rows_ragged_batches(native_lib, tmp_path, batch, backend):
    """The same at batch 3 and batch 1: B * T = 591 / 197 rows (no multiple of the 104- or 208-row tiles) and B below one 16-row MFMA fragment - every launcher of
    the class-token part runs a single ragged tile."""
    _compare(_worker(tmp_path, "rows", None, backend, batch), _worker(tmp_path, "dense", "QATVIT_CLS_BWD=0", backend, batch), f"batch {batch} {backend}")


@pytest.mark.timeout(600)
def test_staged_backward_keeps_the_cls_rows_between_calls(native_lib, tmp_path):
    """Stage 0 in one call, stages 1 .. last in the next (what the data-parallel bucketed backward does): the final norm's [B, D] outputs live in the workspace
    plan, so the gradients equal the single call's bit for bit - except the atomically summed ones, which do not repeat bit for bit between two runs of
    anything (ATOMIC above) and are held to the same 1e-5."""
    r = _worker(tmp_path, "staged", None, "qnnpack", 4, staged=True)
    assert r["one_plane"] and not r["overflowed"]
    bad, loose = [], {}
    for n, g in r["single"].items():
        if torch.equal(r["staged"][n], g):
            continue
        d = _rel(r["staged"][n], g)
        if any(t in n for t in ATOMIC):
            loose[n] = d
            if d > TOL_ATOMIC:
                bad.append(("gradient (atomics)", n, d))
        else:
            bad.append(("gradient", n, d))
    print("CLS_BWD staged against single call, atomically summed gradients that differ:", loose)
    assert not bad, bad
    # ... and they are the step the autograd path ran, up to the fp16 planes' rounding (its scales came from step 1's maxima: the one-plane bar of test_gpu_dy16.py)
    for n, g in r[2]["grads"].items():
        assert _rel(r["single"][n], g) <= 1e-3, n


@pytest.mark.parametrize("width,dtype", [(48, torch.uint8), (384, torch.uint8), (1536, torch.uint8), (1536, torch.float32)])
@pytest.mark.parametrize("T", [5, 197])
@pytest.mark.parametrize("B", [1, 3])
def test_rows_gather_and_scatter(native_lib, B, T, width, dtype):
    """qatvit_rows_gather / qatvit_rows_scatter alone, bit for bit against tensor[::T] and an index-put into zeros; guard bytes behind the compact buffer
    (gather) and behind the tall one (scatter) stay as they were, and the gather reads a tall tensor whose rows are wider than what it takes."""
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=DEV).manual_seed(B * 1000 + T * 10 + width)
    esz = torch.empty((), dtype=dtype).element_size()
    wb, guard = width * esz, 256
    if dtype == torch.float32:
        tall = torch.randn(B * T, width + 4, generator=gen, device=DEV)
    else:
        tall = torch.randint(0, 256, (B * T, width + 16), generator=gen, device=DEV, dtype=torch.uint8)
    buf = torch.full((B * wb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    assert native_lib.qatvit_rows_gather(tall.data_ptr(), buf.data_ptr(), B, T, wb, tall.stride(0) * esz, st) == 0, native_lib.qatvit_last_error()
    torch.cuda.synchronize()
    want = tall[::T, :width].contiguous()
    assert torch.equal(buf[:B * wb].view(dtype).view(B, width), want)
    assert bool((buf[B * wb:] == 0xA5).all()), "gather wrote past the compact buffer"
    out = torch.full((B * T * wb + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    assert native_lib.qatvit_rows_scatter(want.data_ptr(), out.data_ptr(), B, T, wb, st) == 0, native_lib.qatvit_last_error()
    torch.cuda.synchronize()
    ref = torch.zeros(B * T, width, dtype=dtype, device=DEV)
    ref[torch.arange(B, device=DEV) * T] = want
    assert torch.equal(out[:B * T * wb].view(torch.uint8), ref.view(torch.uint8).reshape(-1))
    assert bool((out[B * T * wb:] == 0x5A).all()), "scatter wrote past the tall tensor"


def test_rows_move_argument_errors(native_lib):
    """Refused before any launch: a width that is no multiple of the unit, a stride below the width, a null pointer."""
    x = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert native_lib.qatvit_rows_gather(x.data_ptr(), x.data_ptr(), 2, 5, 6, 8, st) != 0
    assert b"rows_gather" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_rows_gather(x.data_ptr(), x.data_ptr(), 2, 5, 16, 8, st) != 0
    assert native_lib.qatvit_rows_scatter(x.data_ptr(), x.data_ptr(), 2, 5, 24, st) != 0
    assert b"rows_scatter" in native_lib.qatvit_last_error()
    assert native_lib.qatvit_rows_scatter(None, x.data_ptr(), 2, 5, 16, st) != 0
