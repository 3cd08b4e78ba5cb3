"""The persistent form of the fused attention backward (k_attn_bwd_pipe, qatvit_attn_backward_form) against the per-head launches: the same bits.

form 0 = one workgroup per (image, head), form 1 = min(B * H, CU count) persistent workgroups, form 2 = the persistent kernel on 5 workgroups - every
workgroup then walks two or three heads (an uneven tail, a successor in another image), which is what can show a stale LDS image or a register
overwritten before its use.  Inputs as tests/test_gpu_attn_live.py builds them (clipped elements in query row 0 and key row T - 1), outputs in guarded
buffers, both output forms: the bf16 (hi, lo) pair, and the one fp16 plane + amax slots the benchmarked step runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.kernel_check import guarded, guarded_copy  # noqa: E402
from tests.test_gpu_attn_live import _setup  # noqa: E402

DEV = "cuda"
AMAX_SLOTS, AMAX_STRIDE = 8, 32      # include/qatvit.h QATVIT_DY16_AMAX_SLOTS / _STRIDE
MUL16 = 64.0                         # the one-plane form's scale (a power of two, as dy16 chooses them)
# (B, H, T): 12 heads; three key tiles, so five of the eight waves own none; fewer heads than CUs or than 2 x 5: form 1 fetches no successor;
# every key tile full (no padded-key branch, all 14 tiles owned); three key tiles, the last with ONE real key (12 items on 5 workgroups: an uneven tail)
CASES = [(2, 6, 197), (3, 6, 40), (1, 6, 197), (2, 6, 224), (2, 6, 33)]


def _run(native_lib, s, B, T, H, D, dO, cs, one_plane, form, what):
    """One backward in the given form; returns the raw bits of every output: (dqkv hi or the fp16 plane, dqkv lo or None, delta, amax or None)."""
    checks = []

    def out(rows, cols, dt, fill=None):
        t, c = guarded(rows, cols, dt, DEV, fill=fill)
        checks.append(c)
        return t

    gh = out(B * T, 3 * D, torch.float16 if one_plane else torch.bfloat16)
    gl = None if one_plane else out(B * T, 3 * D, torch.bfloat16)
    delta = out(B * H, s["TP"], torch.float32)
    amax = out(AMAX_SLOTS, AMAX_STRIDE, torch.int32, fill=0) if one_plane else None
    mul = torch.full((1,), MUL16, device=DEV)
    dOg, c = guarded_copy(dO)
    checks.append(c)
    rc = native_lib.qatvit_attn_backward_form(None, s["qp"].data_ptr(), s["qmin"], s["qmax"], B, T, H, D, s["Oh"].data_ptr(), s["Ol"].data_ptr(), s["lse"].data_ptr(),
                                              delta.data_ptr(), dOg.data_ptr(), gh.data_ptr(), None if one_plane else gl.data_ptr(),
                                              None if cs is None else cs.data_ptr(), s["codes"].data_ptr(), s["cmask"].data_ptr(),
                                              mul.data_ptr() if one_plane else None, amax.data_ptr() if one_plane else None, form,
                                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, native_lib.qatvit_last_error()
    torch.cuda.synchronize()
    for c in checks:
        c(what)
    assert not torch.isnan(gh.float()).any(), what          # every element of the plane was stored
    return (gh.view(torch.int16).clone(), None if one_plane else gl.view(torch.int16).clone(), delta.view(torch.int32).clone(),
            amax[:, 0].max().item() if one_plane else None)


@pytest.mark.parametrize("one_plane", [False, True], ids=["pair", "one-plane"])
@pytest.mark.parametrize("with_colscale", [False, True], ids=["", "colscale"])
@pytest.mark.parametrize("B,H,T", CASES)
def test_persistent_forms_write_the_bits_of_the_per_head_form(native_lib, B, H, T, with_colscale, one_plane):
    D = 64 * H
    s = _setup(native_lib, B, T, H, D, 3 * T + B)
    cs = (torch.rand(3 * D, device=DEV) + 0.5) if with_colscale else None
    dO = torch.randn(B * T, D, device=DEV)
    ref = _run(native_lib, s, B, T, H, D, dO, cs, one_plane, 0, f"form 0 B={B} T={T}")
    if one_plane:
        assert ref[3] > 0, "the amax slots were not written"
    for form in (1, 2):
        got = _run(native_lib, s, B, T, H, D, dO, cs, one_plane, form, f"form {form} B={B} T={T}")
        assert torch.equal(got[0], ref[0]), f"form {form}: dqkv {'plane' if one_plane else 'hi'} differs"
        if one_plane:
            assert got[3] == ref[3], f"form {form}: amax {got[3]:#x} against {ref[3]:#x}"
        else:
            assert torch.equal(got[1], ref[1]), f"form {form}: dqkv lo differs"
        assert torch.equal(got[2], ref[2]), f"form {form}: delta differs"


def test_per_head_form_is_the_old_entry(native_lib):
    """form 0 through the new entry and qatvit_attn_backward (which now takes the persistent form only above the CU count): the same bits."""
    B, H, T, D = 2, 6, 197, 384
    s = _setup(native_lib, B, T, H, D, 77)
    dO = torch.randn(B * T, D, device=DEV)
    ref = _run(native_lib, s, B, T, H, D, dO, None, False, 0, "form 0")
    gh, gl = torch.zeros(B * T, 3 * D, dtype=torch.bfloat16, device=DEV), torch.zeros(B * T, 3 * D, dtype=torch.bfloat16, device=DEV)
    delta = torch.zeros(B * H, s["TP"], device=DEV)
    assert native_lib.qatvit_attn_backward(None, s["qp"].data_ptr(), s["qmin"], s["qmax"], B, T, H, D, s["Oh"].data_ptr(), s["Ol"].data_ptr(), s["lse"].data_ptr(),
                                           delta.data_ptr(), dO.data_ptr(), gh.data_ptr(), gl.data_ptr(), None, s["codes"].data_ptr(), s["cmask"].data_ptr(),
                                           torch.cuda.current_stream().cuda_stream) == 0, native_lib.qatvit_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gh.view(torch.int16), ref[0]) and torch.equal(gl.view(torch.int16), ref[1])
    assert torch.equal(delta[:, :T].view(torch.int32), ref[2][:, :T])


@pytest.mark.parametrize("B,H,T,D", [(2, 6, 17, 384), (2, 12, 197, 384)], ids=["T=17", "head_dim 32"])
def test_persistent_form_refuses_shapes_without_a_kernel(native_lib, B, H, T, D):
    """form 1 where the fused kernel does not exist: an error with a message, and nothing launched - the outputs keep their sentinel."""
    s = _setup(native_lib, B, T, H, D, 5)
    dO = torch.randn(B * T, D, device=DEV)
    (gh, c0), (gl, c1), (delta, c2) = (guarded(B * T, 3 * D, torch.bfloat16, DEV), guarded(B * T, 3 * D, torch.bfloat16, DEV),
                                       guarded(B * H, s["TP"], torch.float32, DEV))
    before = [t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).clone() for t in (gh, gl, delta)]
    for form in (1, 2):
        rc = native_lib.qatvit_attn_backward_form(None, s["qp"].data_ptr(), s["qmin"], s["qmax"], B, T, H, D, s["Oh"].data_ptr(), s["Ol"].data_ptr(),
                                                  s["lse"].data_ptr(), delta.data_ptr(), dO.data_ptr(), gh.data_ptr(), gl.data_ptr(), None, s["codes"].data_ptr(),
                                                  s["cmask"].data_ptr(), None, None, form, torch.cuda.current_stream().cuda_stream)
        assert rc != 0
        assert b"persistent form" in native_lib.qatvit_last_error()
    torch.cuda.synchronize()
    for t, b in zip((gh, gl, delta), before):
        assert torch.equal(t.view(b.dtype), b), "a refused form wrote to its outputs"
    for c in (c0, c1, c2):
        c("refused form")
    assert native_lib.qatvit_attn_backward_form(None, s["qp"].data_ptr(), s["qmin"], s["qmax"], B, T, H, D, s["Oh"].data_ptr(), s["Ol"].data_ptr(), s["lse"].data_ptr(),
                                                delta.data_ptr(), dO.data_ptr(), gh.data_ptr(), gl.data_ptr(), None, s["codes"].data_ptr(), s["cmask"].data_ptr(),
                                                None, None, 3, torch.cuda.current_stream().cuda_stream) != 0      # an unknown form number
