"""The fused attention backward on the class-token gradient (qatvit_attn_backward_live): dO is zero in every query row but row 0 of each image, so only the
first query pair carries a dS.  With live_q_tiles = 1 the sweep visits that pair alone and stores zeros as the dQ of the others; dK and dV are complete.
Compared with the full count at the bound tests/test_gpu_attn.py applies against its fp64 reference, and the full count once more against that reference."""
import inspect

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.kernel_check import guarded, guarded_copy  # noqa: E402
from tests.test_gpu_attn import _backward_tile_bounds, _ref  # noqa: E402
from tests.util import rel_l2  # noqa: E402

TOL = inspect.signature(_backward_tile_bounds).parameters["tol"].default   # 3e-5: the module bound of test_gpu_attn.py
DEV = "cuda"


def _setup(native_lib, B, T, H, D, seed):
    torch.manual_seed(seed)
    qkv = torch.randn(B * T, 3 * D, device=DEV) * 1.5
    qkv[0, :7] = 40.0                      # clipped elements of query row 0: masked gradient
    qkv[T - 1, D + 3:D + 9] = -40.0
    scale, zp, qmin, qmax = 8.0 / 255, 120, 0, 255
    qp = torch.tensor([scale, 1.0, float(zp), 1.0], device=DEV)
    qp[1] = torch.ones(1, device=DEV)[0] / qp[0]
    TP = native_lib.qatvit_attn_padded_tokens(T)
    s = {"qkv": qkv, "qp": qp, "zp": zp, "qmin": qmin, "qmax": qmax, "TP": TP}
    for n, cols, dt in (("Oh", D, torch.bfloat16), ("Ol", D, torch.bfloat16), ("O16h", D, torch.float16), ("O16l", D, torch.float16)):
        s[n] = torch.zeros(B * T, cols, dtype=dt, device=DEV)
    s["lse"] = torch.zeros(B * H, TP, device=DEV)
    s["codes"] = torch.zeros(B * T, 3 * D, dtype=torch.uint8, device=DEV)
    s["cmask"] = torch.zeros(B * T, 3 * D // 8, dtype=torch.uint8, device=DEV)
    osc = torch.zeros(1, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert native_lib.qatvit_attn_forward_f16(qkv.data_ptr(), qp.data_ptr(), qmin, qmax, B, T, H, D, s["Oh"].data_ptr(), s["Ol"].data_ptr(), s["lse"].data_ptr(),
                                              s["O16h"].data_ptr(), s["O16l"].data_ptr(), osc.data_ptr(), s["codes"].data_ptr(), s["cmask"].data_ptr(), st) == 0, \
        native_lib.qatvit_last_error()
    return s


def _backward(native_lib, s, B, T, H, D, dO, cs, live, dO_cls, what):
    """One backward from the saved codes into guarded outputs; returns (dqkv as fp32, delta)."""
    checks = []

    def out(rows, cols, dt):
        t, c = guarded(rows, cols, dt, DEV)
        checks.append(c)
        return t

    gh, gl, delta = out(B * T, 3 * D, torch.bfloat16), out(B * T, 3 * D, torch.bfloat16), out(B * H, s["TP"], torch.float32)
    dOg, c = guarded_copy(dO)
    checks.append(c)
    st = torch.cuda.current_stream().cuda_stream
    args = (None, s["qp"].data_ptr(), s["qmin"], s["qmax"], B, T, H, D, s["Oh"].data_ptr(), s["Ol"].data_ptr(), s["lse"].data_ptr(), delta.data_ptr(), dOg.data_ptr(),
            gh.data_ptr(), gl.data_ptr(), None if cs is None else cs.data_ptr(), s["codes"].data_ptr(), s["cmask"].data_ptr())
    if live is None:
        rc = native_lib.qatvit_attn_backward(*args, st)
    else:
        rc = native_lib.qatvit_attn_backward_live(*args, live, dO_cls, st)
    assert rc == 0, native_lib.qatvit_last_error()
    torch.cuda.synchronize()
    for c in checks:
        c(what)
    dqkv = gh.float() + gl.float()
    assert not torch.isnan(dqkv).any()
    return dqkv, delta[:, :T].clone()


# 197: the benchmark's token count; 40: three key tiles, so five of the eight waves own none; 17: what the issue names for that - at <= 32 tokens the
# backward is the two-kernel form, which ignores the count (and must still give the same result from the full dO)
@pytest.mark.parametrize("T", [197, 40, 17])
@pytest.mark.parametrize("with_colscale", [False, True])
def test_live_query_tile_against_full_count(native_lib, T, with_colscale):
    B, H, D = 2, 6, 384
    s = _setup(native_lib, B, T, H, D, T + 11)
    cs = (torch.rand(3 * D, device=DEV) + 0.5) if with_colscale else None
    dO = torch.zeros(B * T, D, device=DEV)
    dO[::T] = torch.randn(B, D, device=DEV)                 # query row 0 of every image
    full, delta_full = _backward(native_lib, s, B, T, H, D, dO, cs, None, 0, f"full count T={T}")
    arms = [("live 1", dO, 0)]
    if T > 32:
        arms.append(("live 1, dO [B, D]", dO[::T].contiguous(), 1))
    row_in_image = torch.arange(B * T, device=DEV) % T
    for name, d_arg, d_cls in arms:
        got, delta = _backward(native_lib, s, B, T, H, D, d_arg, cs, 1, d_cls, f"{name} T={T}")
        eq = torch.equal(got, full)
        eK, eV = rel_l2(got[:, D:2 * D].cpu(), full[:, D:2 * D].cpu()), rel_l2(got[:, 2 * D:].cpu(), full[:, 2 * D:].cpu())
        lo = row_in_image < 16
        eQ = rel_l2(got[lo, :D].cpu(), full[lo, :D].cpu())
        print(f"LIVE T={T} colscale={with_colscale} {name}: dK {eK:.3e} dV {eV:.3e} dQ rows 0-15 {eQ:.3e} bit-identical {eq}")
        assert eK < TOL and eV < TOL and eQ < TOL
        assert bool((got[~lo, :D] == 0).all()), "dQ of a query row >= 16 is not zero"
        assert bool((got[0, :7] == 0).all())               # the clipped elements of query row 0 stay masked
        assert torch.equal(delta, delta_full)
    if T <= 32:   # the [B, D] form exists in the fused kernel only: refused, nothing launched
        st = torch.cuda.current_stream().cuda_stream
        x = dO[::T].contiguous()
        assert native_lib.qatvit_attn_backward_live(None, s["qp"].data_ptr(), 0, 255, B, T, H, D, s["Oh"].data_ptr(), s["Ol"].data_ptr(), s["lse"].data_ptr(),
                                                    delta_full.data_ptr(), x.data_ptr(), full.data_ptr(), full.data_ptr(), None, s["codes"].data_ptr(),
                                                    s["cmask"].data_ptr(), 1, 1, st) != 0
        assert b"fused kernel only" in native_lib.qatvit_last_error()


@pytest.mark.parametrize("T", [197, 40])
def test_full_count_with_dense_dO_against_fp64(native_lib, T):
    """The ordinary path through the new entry point (live_q_tiles = 0) and through the old one: the same bits, and the fp64 reference at the module bound."""
    B, H, D = 2, 6, 384
    s = _setup(native_lib, B, T, H, D, T + 5)
    dO = torch.randn(B * T, D, device=DEV)
    a, _ = _backward(native_lib, s, B, T, H, D, dO, None, 0, 0, f"live 0 T={T}")
    b, _ = _backward(native_lib, s, B, T, H, D, dO, None, None, 0, f"old entry T={T}")
    assert torch.equal(a, b)
    _, rg = _ref(s["qkv"], s["qp"][0], s["zp"], s["qmin"], s["qmax"], B, T, H, D, dO)
    for name, c0 in (("dQ", 0), ("dK", D), ("dV", 2 * D)):
        e = rel_l2(a[:, c0:c0 + D].cpu(), rg[:, c0:c0 + D].cpu())
        print(f"LIVE full count T={T} {name} against fp64: {e:.3e}")
        assert e < TOL
