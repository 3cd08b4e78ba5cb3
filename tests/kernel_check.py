"""Helpers of the kernel parity tests: an error bound per output tile, and operands with guarded padding.

tile_errors / assert_tiles_close: a kernel error confined to a few rows (the ragged last row tile of a GEMM epilogue, one key-tile tail of the
attention kernels) is diluted by sqrt(rows wrong / rows) in a whole-tensor relative L2 and passes it at the benchmarked sizes.  Per 16 x 16 tile,
normalised by the RMS of the whole reference, a correct result's worst tile is 1.3 - 1.9 x its whole-tensor value and a lost lo plane on one row is
two orders of magnitude above it (tests/test_kernel_check.py holds both records).

guarded: a [rows, cols] operand as the middle of one allocation of rows + 2 * pad rows filled with a sentinel.  Around an output the padding is a
canary (a store past the extent changes it); around an input it is poison (a result that depends on rows outside the extent becomes NaN, a wrong
integer or a poisoned min / max).  Everything stays inside memory the test owns."""
import numpy as np
import torch

# fp32: a quiet NaN with a recognisable payload; bf16 / fp16: NaN; int8: 0x80; uint8 (code planes, mask-bit planes): 0xFF; int32: 0x80808080
_SENTINEL = {
    torch.float32: (torch.int32, 0x7FC0BEEF),
    torch.bfloat16: (torch.int16, 0x7FDB),
    torch.float16: (torch.int16, 0x7EDB),
    torch.int8: (torch.int8, -128),
    torch.uint8: (torch.uint8, 0xFF),
    torch.int32: (torch.int32, 0x80808080 - (1 << 32)),
}
PAD = 224     # rows: covers the tallest row tile of any kernel (208)


def tile_errors(got, ref, tile=(16, 16)):
    """Per-tile RMS of got - ref (ragged edge tiles over their true element count) divided by the RMS of ref over the WHOLE tensor - a tile whose
    reference happens to be near zero does not blow up.  2-D tensors, fp64 on the device they live on.
    Returns (error map [ceil(M / th), ceil(N / tw)], worst value, (row0, col0) of the worst tile); a NaN tile counts as the worst."""
    assert got.dim() == 2 and got.shape == ref.shape, (got.shape, ref.shape)
    th, tw = tile
    M, N = ref.shape
    r = ref.double()
    d2 = (got.to(r.device).double() - r) ** 2
    mt, nt = -(-M // th), -(-N // tw)
    d2 = torch.nn.functional.pad(d2, (0, nt * tw - N, 0, mt * th - M))
    s = d2.view(mt, th, nt, tw).sum((1, 3))
    rows = torch.full((mt,), th, dtype=torch.float64, device=r.device)
    cols = torch.full((nt,), tw, dtype=torch.float64, device=r.device)
    rows[-1] = M - (mt - 1) * th
    cols[-1] = N - (nt - 1) * tw
    rms = r.pow(2).mean().sqrt().item()
    err = (s / (rows[:, None] * cols[None, :])).sqrt() / (rms if rms > 0 else 1.0)
    k = torch.nan_to_num(err, nan=float("inf"), posinf=float("inf")).argmax().item()
    i, j = divmod(k, nt)
    return err, err[i, j].item(), (i * th, j * tw)


def rel_l2_t(got, ref):
    """tests.util.rel_l2 on the device (fp64)."""
    r = ref.double()
    n = r.norm().item()
    d = (got.to(r.device).double() - r).norm().item()
    return d / n if n > 0 else d


def assert_tiles_close(got, ref, tol, tile=(16, 16), what=""):
    """Every tile of tile_errors(got, ref, tile) within tol.  Prints the figures first (pytest shows them with -s or on failure; profiles/kernel_tile_errors.txt
    is made of these lines)."""
    err, worst, (r0, c0) = tile_errors(got, ref, tile)
    over = int((~(err <= tol)).sum().item())       # NaN tiles count
    print(f"TILE {what}: whole {rel_l2_t(got, ref):.3e} worst_tile {worst:.3e} at ({r0}, {c0}) tile {tile[0]}x{tile[1]} of {tuple(ref.shape)} bound {tol:.3e}")
    assert over == 0, (f"{what}: worst {tile[0]} x {tile[1]} tile at rows {r0}.., cols {c0}..: {worst:.3e} (tolerance {tol:.1e}); whole-tensor rel_l2 "
                       f"{rel_l2_t(got, ref):.3e}; {over} of {err.numel()} tiles over the tolerance (tensor {tuple(ref.shape)})")
    return worst, (r0, c0)


class Guarded:
    """t = the [rows, cols] view to hand to a launcher; check() asserts the padding rows are still the sentinel, bit for bit."""

    def __init__(self, rows, cols, dtype, device, pad=PAD, fill=None):
        idt, pat = _SENTINEL[dtype]
        assert (pad * cols * torch.empty(0, dtype=dtype).element_size()) % 256 == 0, "the padding must keep the view 256-byte aligned"
        self.raw = torch.full((rows + 2 * pad, cols), pat, dtype=idt, device=device)
        self.pad, self.rows, self.pat = pad, rows, pat
        self.t = self.raw[pad:pad + rows].view(dtype)
        assert self.t.is_contiguous()
        if fill is not None:
            self.t.fill_(fill)

    def check(self, what=""):
        for name, part, row0 in (("before", self.raw[:self.pad], -self.pad), ("after", self.raw[self.pad + self.rows:], self.rows)):
            bad = (part != self.pat).nonzero()
            assert bad.numel() == 0, (f"{what}: {bad.shape[0]} sentinel element(s) {name} the extent were overwritten, the first at row "
                                      f"{row0 + bad[0, 0].item()} (extent: rows 0..{self.rows - 1}), column {bad[0, 1].item()}")


def guarded(rows, cols, dtype, device, pad=PAD, fill=None):
    """(view, check): see Guarded.  fill: an initial value of the view (default: it holds the sentinel too, so an element the kernel does not
    store stays a NaN / an impossible code)."""
    g = Guarded(rows, cols, dtype, device, pad, fill)
    return g.t, g.check


def guarded_copy(x, pad=None):
    """x (any shape, contiguous) copied into a guarded allocation of [numel / last dim, last dim]: (view of x's shape, check).  pad: PAD rows, or the
    2 / 4 / 8-fold of it that a short row (a scalar, a pair of statistics words) needs to keep the view 256-byte aligned."""
    x = x.contiguous()
    cols = x.shape[-1]
    if pad is None:
        pad = next(PAD * k for k in (1, 2, 4, 8) if (PAD * k * cols * x.element_size()) % 256 == 0)
    t, check = guarded(x.numel() // cols, cols, x.dtype, x.device, pad)
    t.copy_(x.reshape(-1, cols))
    return t.view(x.shape), check


def ord2f(k):
    """qv_common.h: the order-preserving uint32 of a statistics accumulator -> float."""
    k = int(k) & 0xFFFFFFFF
    u = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return np.frombuffer(np.uint32(u).tobytes(), dtype=np.float32)[0]
